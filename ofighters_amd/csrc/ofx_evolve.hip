// ofx_evolve.hip - device-resident neuroevolution of the from-scratch sigmoid MLP: a genome per ship
// (agents/neural_network.py:436-478 generate / evolution / mutate / reproduce / dafts around the network of :396-420,
//  one network per ship as in lib/battleground.py:52-76, the four-sigmoid decode of agents/brAIn.py:129-134).
//
// A population is P genomes of G float64 elements each, resident in HBM (include/ofx.h: element index e = the position
// in weights_layers + biases_layers; every random draw is keyed by (slot, e, generation, stream)).
//
// Storage of one genome (G doubles at data + slot * G, 64-bit offsets):
//   [0, nin*n1)   the first layer INPUT-major, W1T[k][o] = W_1[o][k]: the n1 weights of one input are contiguous (72 B at
//                 n1 = 9) and the weights of consecutive map cells - a disc's row of set cells - are one contiguous run
//   [nin*n1, G)   the remaining layers row-major and the biases, exactly as in the element order
// so storage position s and element e differ in the first layer only (s = k*n1 + o  <->  e = o*nin + k).
//
// k_pop_breed  one thread per storage position of one destination slot: coalesced 8-byte reads of the parent, coalesced
//              8-byte writes of the child, two Philox evaluations per element (one for a fresh genome).  In place: the
//              host has checked that a parent is a kept slot, so no source is a destination.
// k_pop_act    one 256-thread workgroup per (arena, ship), early exit for the unassigned and the dead.  Each of its four
//              waves walks a quarter of the arena's two 1-bit maps (POP_AHEAD batches of 64 words loaded ahead of the one
//              it looks at), compacts the set cells into its own LDS list (a wave scan, no block barrier, ascending
//              order) and gathers their W1T rows with lanes laid over (cell, neuron): consecutive lanes
//              read consecutive doubles, a run of set cells is one contiguous read.  Lane sums, then the 4 x (64 / n1)
//              partial sums per neuron, are added in a fixed order: no floating-point atomics, the same bits every call.
//              Head, bias, sigmoid, the remaining layers (activations in LDS), the decode and the stores follow in the
//              same launch.
// k_pop_grad / k_pop_apply  ofx_population_learn, a gradient step per genome on its own samples (include/ofx.h).  The
//              walk (pop_walk), the forward (pop_forward) and the decode (pop_emit) are __device__ bodies shared with
//              k_pop_act: each exists once.  Phase A (k_pop_grad, a workgroup per ship) runs the forward and leaves
//              every layer's activations and deltas, all from the OLD weights, in a workspace; phase B (k_pop_apply,
//              a workgroup per genome) adds its samples' terms in ascending ship order and touches, in the first layer,
//              only the n1-double runs of the set cells.  No floating-point atomics.
// k_pop_fitness  integer atomics only.
// k_es_act / k_es_update / k_es_step / k_es_member  seeded evolution strategies, at the end of this file: one centre
//              genome, the members' noise regenerated where it is read; k_es_act is pop_forward with another weight
//              reader, k_es_step is k_es_update with momentum or Adam state beside the centre.
// k_es_sigma_act / k_es_sigma_member / k_es_sigma_step  the same with a per-element exploration width sigma[e] beside
//              the centre, learned in the pass that steps the centre (PEPG with symmetric sampling).
#include "ofx_internal.h"
#include "ofx_arena.h"

#include <new>
#include <vector>

#define POP_MAX_LAYERS 8
#define POP_MAX_WIDTH 64
#define POP_LIST 2048               /* set cells one wave lists before it gathers: a batch of 64 words holds <= 2048 */
#define POP_MAX_ACTS ((POP_MAX_LAYERS - 2) * POP_MAX_WIDTH + 4) /* activations of one ship behind the input: <= 6 x 64 + 4 */
#define POP_AHEAD 16                /* batches of 64 map words a wave loads before it looks at the first              */

struct ofx_population {
  int n_layers;
  int32_t layers[POP_MAX_LAYERS];
  int64_t P;
  uint32_t G;        // elements of one genome
  uint32_t first;    // nin * n1: elements (and storage positions) of the first layer
  uint32_t n_w;      // weights of one genome; the biases follow
  double *data;      // [P][G]
  int32_t *jobs;     // [P][2] (destination, parent or -1) of the slots a breed rewrites
};

// numpy's 53-bit uniform in [0, 1): exact in float64
__host__ __device__ inline double pop_uniform(uint32_t hi, uint32_t lo) {
  return ((double)(hi >> 5) * 67108864.0 + (double)(lo >> 6)) / 9007199254740992.0;
}

// element index of storage position s
__device__ inline uint32_t pop_element(uint32_t s, uint32_t first, uint32_t nin, uint32_t n1) {
  if (s >= first) return s;
  const uint32_t k = s / n1, o = s - k * n1;
  return o * nin + k;
}

// jobs == nullptr: job j is a fresh genome in slot j (ofx_population_init)
__global__ __launch_bounds__(256) void k_pop_breed(double *data, const int32_t *jobs, int n_jobs, uint32_t G,
                                                   uint32_t first, uint32_t nin, uint32_t n1, double evo, double mut,
                                                   ofx_rng_key key, uint32_t generation) {
  const uint32_t s = blockIdx.x * 256u + threadIdx.x;
  if (s >= G) return;
  const uint32_t e = pop_element(s, first, nin, n1);
  for (int j = blockIdx.y; j < n_jobs; j += gridDim.y) {
    const int32_t dst = jobs ? jobs[2 * j] : j, src = jobs ? jobs[2 * j + 1] : -1;
    uint32_t r[4];
    double w;
    if (src < 0) {
      ofx_philox4x32_10((uint32_t)dst, e, generation, OFX_STREAM_FRESH, key, r);
      w = 2.0 * pop_uniform(r[0], r[1]) - 1.0;
    } else {
      w = data[(size_t)src * G + s];
      ofx_philox4x32_10((uint32_t)dst, e, generation, OFX_STREAM_EVOLVE, key, r);
      if (evo > 0.0) {
        const double c = (2.0 * pop_uniform(r[0], r[1]) - 1.0) * evo;
        const double cw = c * w;
        w = cw + w;
      }
      if (mut > 0.0 && pop_uniform(r[2], r[3]) < mut) {
        uint32_t q[4];
        ofx_philox4x32_10((uint32_t)dst, e, generation, OFX_STREAM_MUTATE, key, q);
        w = 2.0 * pop_uniform(q[0], q[1]) - 1.0;
      }
    }
    data[(size_t)dst * G + s] = w;
  }
}

__device__ inline double pop_sigmoid(double v) { return 1.0 / (1.0 + exp(-v)); }

struct pop_net {
  int n_layers;
  int32_t layers[POP_MAX_LAYERS];
};

// The walk over one arena's set cells, stated once for the forward (k_pop_act, k_pop_grad) and the first layer's update
// (k_pop_apply).  The two maps are one run of 2*words words (toVector: ship map, then laser map); wave wv of the four
// owns a quarter of it, lists the set cells of its quarter in ascending order in `mine` (POP_LIST entries of its own,
// a wave scan, no block barrier) and hands them to flush(n) - whenever the next batch would not fit, and once at the
// end (n may be 0).  The wavefront fences order the lanes' list writes before flush's reads and those before the next
// writes.
template <class Flush>
__device__ __forceinline__ void pop_walk(const unsigned *sb, const unsigned *lb, int words, int wv, int lane,
                                         uint32_t *mine, Flush flush) {
  const int total = 2 * words, per = (total + 3) / 4;
  const int w_end = min(total, (wv + 1) * per);
  int count = 0;                                // cells listed, uniform over the wave
  auto drain = [&]() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    flush(count);
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    count = 0;
  };
  // POP_AHEAD batches of 64 words are loaded before the first is looked at: the maps are ~1 % set, so the walk is a
  // chain of mostly empty loads and would otherwise pay one memory latency per 64 words
  for (int w0 = wv * per; w0 < w_end; w0 += 64 * POP_AHEAD) {
    unsigned v[POP_AHEAD];
#pragma unroll
    for (int j = 0; j < POP_AHEAD; j++) {
      const int w = w0 + j * 64 + lane;
      v[j] = w < w_end ? (w < words ? sb[w] : lb[w - words]) : 0u;
    }
#pragma unroll
    for (int j = 0; j < POP_AHEAD; j++) {
      unsigned x = v[j];
      if (__ballot(x != 0) == 0ull) continue;
      const int c = __popc(x);
      int inc = c;                              // inclusive scan over the wave
#pragma unroll
      for (int d = 1; d < 64; d <<= 1) {
        const int up = __shfl_up(inc, d);
        if (lane >= d) inc += up;
      }
      const int n_new = __shfl(inc, 63);
      if (count + n_new > POP_LIST) drain();
      const uint32_t cell0 = (uint32_t)(w0 + j * 64 + lane) * 32u;
      int at = count + inc - c;
      while (x) {
        const int b = __ffs((int)x) - 1;
        x &= x - 1;
        mine[at++] = cell0 + b;
      }
      count += n_new;
    }
  }
  drain();
}

// How pop_forward reads a weight, stated per caller: first(k, o) is W_1[o][k] at storage position k * n1 + o, at(s) the
// storage position s behind the first layer (there s is the element index).  pop_stored reads the genome as it lies in
// HBM (k_pop_act, k_pop_grad, the centre in k_es_act); es_member, further down, adds the member's noise to it.
struct pop_stored {
  const double *gen;
  __device__ __forceinline__ double first(size_t k, int o, int n1) const { return gen[k * n1 + o]; }
  __device__ __forceinline__ double at(size_t s) const { return gen[s]; }
};

// Neural_network.feed of the genome `rd` reads on ship s of arena a, by one 256-thread workgroup; returns the row of
// `act` that holds the four outputs.  KEEP = false (k_pop_act, k_es_act): two rows, layer l's activations in row l & 1.
// KEEP = true (k_pop_grad): a row per layer, a_{l+1} in row l, and the 8-scalar head of the observation in `head`.
template <bool KEEP, class Read>
__device__ __forceinline__ int pop_forward(int s, int a, int W, int H, const ofx_state &st, const unsigned *ship_bits,
                                           const unsigned *laser_bits, int words, const Read &rd, uint32_t first,
                                           uint32_t n_w, const pop_net &net, uint32_t (*list)[POP_LIST],
                                           double (*part)[64], double (*act)[POP_MAX_WIDTH], double *head) {
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int n1 = net.layers[1];
  const int groups = 64 / n1;                   // cells one wave gathers per pass
  const int o = lane % n1, grp = lane / n1;     // this lane's neuron and its place among the pass's cells
  const bool gathers = grp < groups;
  const unsigned *sb = ship_bits + (size_t)a * words, *lb = laser_bits + (size_t)a * words;
  uint32_t *mine = list[wv];
  double acc = 0.0;
  // gather what is listed: lane (grp, o) takes cells grp, grp + groups, ... in list order
  pop_walk(sb, lb, words, wv, lane, mine, [&](int count) {
    if (gathers) {
      int i = grp;
      for (; i + 7 * groups < count; i += 8 * groups) {
        double t[8];
#pragma unroll
        for (int q = 0; q < 8; q++) t[q] = rd.first(8u + mine[i + q * groups], o, n1);
#pragma unroll
        for (int q = 0; q < 8; q++) acc += t[q];
      }
      for (; i < count; i += groups) acc += rd.first(8u + mine[i], o, n1);
    }
  });
  part[wv][lane] = gathers ? acc : 0.0;
  __syncthreads();
  if (tid < n1) {
    // first layer of neuron tid: head in toVector order, the map cells in (wave, group) order, bias
    double v[8];
    ofx_obs_head(st, s, W, H, v);
    if (KEEP && tid == 0) {
#pragma unroll
      for (int k = 0; k < 8; k++) head[k] = v[k];
    }
    double z = rd.first(0, tid, n1) * v[0];
#pragma unroll
    for (int k = 1; k < 8; k++) z += rd.first(k, tid, n1) * v[k];
    for (int q = 0; q < 4; q++)
      for (int j = 0; j < groups; j++) z += part[q][j * n1 + tid];
    act[0][tid] = pop_sigmoid(z + rd.at(n_w + tid));
  }
  __syncthreads();
  uint32_t woff = first, boff = n_w + (uint32_t)n1;
  int cur = 0;
  for (int l = 1; l + 1 < net.n_layers; l++) {
    const int nin = net.layers[l], nout = net.layers[l + 1];
    const int nxt = KEEP ? l : cur ^ 1;
    if (tid < nout) {
      const size_t w = woff + (size_t)tid * nin;
      double z = 0.0;
      for (int k = 0; k < nin; k++) z += rd.at(w + k) * act[cur][k];
      act[nxt][tid] = pop_sigmoid(z + rd.at(boff + tid));
    }
    __syncthreads();
    woff += (uint32_t)(nin * nout);
    boff += (uint32_t)nout;
    cur = nxt;
  }
  return cur;
}

// the reference's decode of the four outputs `out` (brAIn.py:129-134, the arena's size in place of 400) and the stores
__device__ __forceinline__ void pop_emit(int s, int W, int H, const double *out, ofx_action *actions, double *y) {
  const int tid = threadIdx.x;
  if (actions && tid == 0) {
    const double y0 = out[0], y1 = out[1], y2 = out[2], y3 = out[3];
    ofx_action act;
    act.px = (int32_t)(y2 * (double)W);
    act.py = (int32_t)(y3 * (double)H);
    act.shoot = y0 > 0.5 ? 1 : 0;
    act.thrust = y1 > 0.5 ? 1 : 0;
    act.valid = 1;
    act._pad = 0;
    actions[s] = act;
  }
  if (y && tid < 4) y[(size_t)s * 4 + tid] = out[tid];
}

__global__ __launch_bounds__(256) void k_pop_act(int M, int W, int H, ofx_state st, const unsigned *ship_bits,
                                                 const unsigned *laser_bits, int words, const double *data, long long P,
                                                 uint32_t G, uint32_t first, uint32_t n_w, pop_net net,
                                                 const int32_t *genome_of, ofx_action *actions, double *y) {
  __shared__ uint32_t list[4][POP_LIST];
  __shared__ double part[4][64];
  __shared__ double act[2][POP_MAX_WIDTH];
  const int s = blockIdx.x, a = s / M;
  const int32_t g = genome_of[s];
  if (g < 0 || (long long)g >= P || !st.alive[s]) return;  // uniform over the workgroup
  const pop_stored rd = {data + (size_t)g * G};
  const int cur = pop_forward<false>(s, a, W, H, st, ship_bits, laser_bits, words, rd, first, n_w, net, list, part, act,
                                     nullptr);
  pop_emit(s, W, H, act[cur], actions, y);
}

// What one ofx_population_learn call keeps between its two kernels (learn_layout): per ship the activations and deltas
// of every layer packed one after the other (S = layers[1] + ... + layers[L] doubles each) and the observation's head,
// per ship the genome it is a sample of (-1: none), per genome its number of samples.
struct LearnWs {
  int32_t *sample_of;  // [N*M]
  int32_t *count;      // [P]
  double *a, *d;       // [N*M][S]
  double *head;        // [N*M][8]
};

// Phase A of ofx_population_learn: the forward of k_pop_act (the same bodies, the same bits), then for a sample the
// deltas of every layer from the genome's OLD weights.  One workgroup per (arena, ship).
__global__ __launch_bounds__(256) void k_pop_grad(int M, int W, int H, ofx_state st, const unsigned *ship_bits,
                                                  const unsigned *laser_bits, int words, const double *data, long long P,
                                                  uint32_t G, uint32_t first, uint32_t n_w, pop_net net, int S,
                                                  const int32_t *genome_of, const double *solution,
                                                  const uint8_t *learn_mask, ofx_action *actions, double *y, double *err,
                                                  LearnWs ws) {
  // 38 496 B: four workgroups fit a CU's 160 KB, as with k_pop_act (with the deltas in rows of their own, 42 080 B, three
  // did, and the call's phase A took 628 us against the forward's 459 at 4096 arenas)
  __shared__ __attribute__((aligned(16))) uint32_t list[4][POP_LIST];
  __shared__ double part[4][64];
  __shared__ double act[POP_MAX_LAYERS - 1][POP_MAX_WIDTH];
  __shared__ double head[8], diff[4];
  const int s = blockIdx.x, a = s / M;
  const int32_t g = genome_of[s];
  if (g < 0 || (long long)g >= P || !st.alive[s]) return;  // uniform over the workgroup
  const double *gen = data + (size_t)g * G;
  const pop_stored rd = {gen};
  const int top = pop_forward<true>(s, a, W, H, st, ship_bits, laser_bits, words, rd, first, n_w, net, list, part, act,
                                    head);
  pop_emit(s, W, H, act[top], actions, y);
  if (learn_mask && !learn_mask[s]) return;                // uniform over the workgroup
  const int tid = threadIdx.x;
  // the deltas take the cell lists' place: the forward's barriers stand behind every wave's last look at its list
  double (*dl)[POP_MAX_WIDTH] = reinterpret_cast<double (*)[POP_MAX_WIDTH]>(&list[0][0]);
  if (tid < 4) {
    const double out = act[top][tid], d = solution[(size_t)s * 4 + tid];
    const double df = d - out;
    diff[tid] = df;
    dl[top][tid] = df * (out * (1.0 - out));
  }
  __syncthreads();
  if (tid == 0) {
    if (err) err[s] = ((diff[0] * diff[0] + diff[1] * diff[1]) + diff[2] * diff[2]) + diff[3] * diff[3];
    ws.sample_of[s] = g;
    atomicAdd(ws.count + g, 1);
  }
  // delta_l = (W_{l+1}^T delta_{l+1}) * a_l (1 - a_l); row l holds layer l + 1, W_{l+1} is row-major behind the first layer
  uint32_t woff = n_w;
  for (int l = top - 1; l >= 0; l--) {
    const int nk = net.layers[l + 1], no = net.layers[l + 2];
    woff -= (uint32_t)(nk * no);
    if (tid < nk) {
      const double *w = gen + woff + tid;
      double sum = w[0] * dl[l + 1][0];
      for (int q = 1; q < no; q++) sum += w[(size_t)q * nk] * dl[l + 1][q];
      const double v = act[l][tid];
      dl[l][tid] = sum * (v * (1.0 - v));
    }
    __syncthreads();
  }
  int off = 0;
  for (int l = 0; l <= top; l++) {
    const int n = net.layers[l + 1];
    if (tid < n) {
      ws.a[(size_t)s * S + off + tid] = act[l][tid];
      ws.d[(size_t)s * S + off + tid] = dl[l][tid];
    }
    off += n;
  }
  if (tid < 8) ws.head[(size_t)s * 8 + tid] = head[tid];
}

// Phase B of ofx_population_learn: one workgroup per genome applies its samples' terms one sample after the other, in
// ascending flat ship index.  It finds them by scanning sample_of 256 entries at a time (a ballot per wave, the hits
// compacted in order into `found`), and per sample: the head rows of the first layer, the later layers and every bias
// with a thread per element, then the shared walk over the sample's arena with a read-add-write of the n1 contiguous
// doubles of each set cell, lanes over (cell, neuron) as in the gather.  Within one sample every address is distinct;
// two samples may meet in a cell from different waves, hence the barrier between samples.  A genome belongs to one
// workgroup alone.
__global__ __launch_bounds__(256) void k_pop_apply(int NM, int M, const unsigned *ship_bits, const unsigned *laser_bits,
                                                   int words, double *data, uint32_t G, uint32_t first, uint32_t n_w,
                                                   pop_net net, int S, LearnWs ws, double rate) {
  __shared__ uint32_t list[4][POP_LIST];
  __shared__ int32_t found[256];
  __shared__ int in_wave[4];
  __shared__ double sa[POP_MAX_ACTS], sd[POP_MAX_ACTS], sh[8];   // 40 080 B in all: four workgroups a CU
  const int g = blockIdx.x;
  const int n = ws.count[g];
  if (n == 0) return;                                      // uniform over the workgroup
  const double c = rate / (double)n;
  double *gen = data + (size_t)g * G;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int n1 = net.layers[1];
  const int groups = 64 / n1;
  const int o = lane % n1, grp = lane / n1;
  const bool gathers = grp < groups;
  uint32_t *mine = list[wv];
  int done = 0;
  for (int base = 0; base < NM && done < n; base += 256) {
    const int idx = base + tid;
    const bool hit = idx < NM && ws.sample_of[idx] == g;
    const unsigned long long b = __ballot(hit);
    if (lane == 0) in_wave[wv] = __popcll(b);
    __syncthreads();
    int before = 0, total = 0;
    for (int q = 0; q < 4; q++) {
      if (q < wv) before += in_wave[q];
      total += in_wave[q];
    }
    if (hit) found[before + __popcll(b & ((1ull << lane) - 1ull))] = idx;
    __syncthreads();
    for (int j = 0; j < total; j++) {
      const int s = found[j], a = s / M;
      for (int t = tid; t < S; t += 256) {                 // S can pass 256: 6 x 64 + 4
        sa[t] = ws.a[(size_t)s * S + t];
        sd[t] = c * ws.d[(size_t)s * S + t];
      }
      if (tid < 8) sh[tid] = ws.head[(size_t)s * 8 + tid];
      __syncthreads();
      // the 8 head inputs of the first layer: storage position k * n1 + o
      for (int e = tid; e < 8 * n1; e += 256) {
        const int k = e / n1;
        const double t = sd[e - k * n1] * sh[k];
        gen[e] = gen[e] + t;
      }
      uint32_t woff = first;
      int in = 0, out = n1;
      for (int l = 1; l + 1 < net.n_layers; l++) {
        const int nin = net.layers[l], nout = net.layers[l + 1];
        for (int e = tid; e < nin * nout; e += 256) {
          const int q = e / nin;
          const double t = sd[out + q] * sa[in + (e - q * nin)];
          gen[woff + e] = gen[woff + e] + t;
        }
        woff += (uint32_t)(nin * nout);
        in = out;
        out += nout;
      }
      for (int t = tid; t < S; t += 256) gen[n_w + t] = gen[n_w + t] + sd[t];
      // the set cells: the input is 1, the element becomes w + c * delta_1[o]
      const double cd = sd[o];
      pop_walk(ship_bits + (size_t)a * words, laser_bits + (size_t)a * words, words, wv, lane, mine, [&](int count) {
        if (gathers)
          for (int i = grp; i < count; i += groups) {
            double *w = gen + (size_t)(8u + mine[i]) * n1 + o;
            *w = *w + cd;
          }
      });
      __syncthreads();
    }
    done += total;
  }
}

// the teacher's action as a target: the inverse of pop_emit's decode; one thread per (arena, ship)
__global__ void k_pop_targets(int NM, int W, int H, const ofx_action *teacher, double *solution, uint8_t *mask) {
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= NM) return;
  const ofx_action t = teacher[s];
  const double x = ((double)t.px + 0.5) / (double)W, y = ((double)t.py + 0.5) / (double)H;
  double *out = solution + (size_t)s * 4;
  out[0] = t.shoot ? 1.0 : 0.0;
  out[1] = t.thrust ? 1.0 : 0.0;
  out[2] = x < 0.0 ? 0.0 : x > 1.0 ? 1.0 : x;
  out[3] = y < 0.0 ? 0.0 : y > 1.0 ? 1.0 : y;
  mask[s] = t.valid != 0;
}

// acc[0] += the err entries >= 0 (thread t adds entries t, t + 256, ... in that order, then the 256 partial sums are
// added in thread order: the same bits every call), acc[1] += their number; every entry is then set to -1 (no sample)
__global__ __launch_bounds__(256) void k_pop_err_reduce(int NM, double *err, double *acc) {
  __shared__ double sum[256];
  __shared__ int cnt[256];
  const int tid = threadIdx.x;
  double v = 0.0;
  int k = 0;
  for (int s = tid; s < NM; s += 256) {
    const double e = err[s];
    if (e >= 0.0) { v += e; k++; }
    err[s] = -1.0;
  }
  sum[tid] = v;
  cnt[tid] = k;
  __syncthreads();
  if (tid == 0) {
    double t = sum[0];
    int m = cnt[0];
    for (int q = 1; q < 256; q++) { t += sum[q]; m += cnt[q]; }
    acc[0] = acc[0] + t;
    acc[1] = acc[1] + (double)m;
  }
}

__global__ void k_pop_fitness(int NM, long long P, const int32_t *last_score, const int32_t *genome_of,
                              unsigned long long *sum, int *count) {
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= NM) return;
  const int32_t g = genome_of[s];
  if (g < 0 || (long long)g >= P) return;
  atomicAdd(sum + g, (unsigned long long)(long long)last_score[s]);
  atomicAdd(count + g, 1);
}

static ofx_population *&pop_of(ofx_handle *h) { return h->population; }

static pop_net net_of(const ofx_population *p) {
  pop_net net;
  net.n_layers = p->n_layers;
  for (int i = 0; i < POP_MAX_LAYERS; i++) net.layers[i] = i < p->n_layers ? p->layers[i] : 0;
  return net;
}

void ofx_population_free(ofx_handle *h) {
  ofx_population *p = pop_of(h);
  if (!p) return;
  if (p->data) (void)hipFree(p->data);
  if (p->jobs) (void)hipFree(p->jobs);
  delete p;
  pop_of(h) = nullptr;
}

static int need_population(ofx_handle *h, const char *who, ofx_population **out) {
  if (!h) { ofx_set_error("%s: null handle", who); return OFX_ERR_INVALID; }
  if (!pop_of(h)) { ofx_set_error("%s: the handle holds no population (ofx_population_create)", who); return OFX_ERR_STATE; }
  *out = pop_of(h);
  return OFX_OK;
}

// the topologies a genome can have on this handle, stated once for ofx_population_create and ofx_es_create (`who`);
// n_w, n_b: the weights and biases of one genome
static int check_topology(ofx_handle *h, const char *who, const int32_t *layers, int32_t n_layers,
                          unsigned long long *n_w, unsigned long long *n_b) {
  if (n_layers < 2 || n_layers > POP_MAX_LAYERS) {
    ofx_set_error("%s: need 2..%d layers (got %d)", who, POP_MAX_LAYERS, n_layers);
    return OFX_ERR_INVALID;
  }
  const ofx_config &c = h->cfg;
  const long long nin = 8 + 2ll * c.width * c.height;
  if (layers[0] != nin) {
    ofx_set_error("%s: layers[0] must be 8 + 2*W*H = %lld (got %d)", who, nin, layers[0]);
    return OFX_ERR_INVALID;
  }
  if (layers[n_layers - 1] != 4) {
    ofx_set_error("%s: the last layer must have 4 outputs, the reference's Action.size (got %d)", who,
                  layers[n_layers - 1]);
    return OFX_ERR_INVALID;
  }
  for (int i = 1; i < n_layers; i++)
    if (layers[i] < 1 || layers[i] > POP_MAX_WIDTH) {
      ofx_set_error("%s: layer %d must be 1..%d wide (got %d)", who, i, POP_MAX_WIDTH, layers[i]);
      return OFX_ERR_INVALID;
    }
  *n_w = *n_b = 0;
  for (int i = 0; i + 1 < n_layers; i++) { *n_w += (unsigned long long)layers[i] * layers[i + 1]; *n_b += layers[i + 1]; }
  if (*n_w + *n_b >= (1ull << 32)) { ofx_set_error("%s: a genome of %llu elements", who, *n_w + *n_b); return OFX_ERR_INVALID; }
  return OFX_OK;
}

extern "C" int ofx_population_create(ofx_handle *h, const int32_t *layers, int32_t n_layers, int64_t P) {
  if (!h || !layers) { ofx_set_error("ofx_population_create: null argument"); return OFX_ERR_INVALID; }
  if (pop_of(h)) { ofx_set_error("ofx_population_create: the handle already holds a population (ofx_population_destroy)"); return OFX_ERR_STATE; }
  unsigned long long n_w, n_b;
  const int rc = check_topology(h, "ofx_population_create", layers, n_layers, &n_w, &n_b);
  if (rc) return rc;
  if (P < 1 || P > 0x7fffffffll) { ofx_set_error("ofx_population_create: P must be in [1, 2^31) (got %lld)", (long long)P); return OFX_ERR_INVALID; }
  const ofx_config &c = h->cfg;
  OFX_HIP(hipSetDevice(c.device));
  ofx_population *p = new (std::nothrow) ofx_population();
  if (!p) { ofx_set_error("ofx_population_create: out of host memory"); return OFX_ERR_INVALID; }
  p->n_layers = n_layers;
  for (int i = 0; i < n_layers; i++) p->layers[i] = layers[i];
  p->P = P;
  p->G = (uint32_t)(n_w + n_b);
  p->first = (uint32_t)((unsigned long long)layers[0] * layers[1]);
  p->n_w = (uint32_t)n_w;
  p->data = nullptr;
  p->jobs = nullptr;
  const size_t bytes = (size_t)P * p->G * sizeof(double);
  hipError_t e = hipMalloc((void **)&p->data, bytes);
  if (e == hipSuccess) e = hipMalloc((void **)&p->jobs, (size_t)P * 2 * sizeof(int32_t));
  if (e != hipSuccess) {
    (void)hipGetLastError();
    ofx_set_error("ofx_population_create: allocating %zu bytes for %lld genomes of %u elements failed: %s", bytes,
                  (long long)P, p->G, hipGetErrorString(e));
    if (p->data) (void)hipFree(p->data);
    delete p;
    return OFX_ERR_HIP;
  }
  pop_of(h) = p;
  return OFX_OK;
}

extern "C" int ofx_population_destroy(ofx_handle *h) {
  if (!h) { ofx_set_error("ofx_population_destroy: null handle"); return OFX_ERR_INVALID; }
  OFX_HIP(hipSetDevice(h->cfg.device));
  OFX_HIP(hipStreamSynchronize(h->stream));
  ofx_population_free(h);
  return OFX_OK;
}

// k_pop_breed on the genomes at `data`, each G elements of the topology `layers` (the population's, or the ES centre)
static int launch_breed(ofx_handle *h, double *data, uint32_t G, uint32_t first, const int32_t *layers,
                        const int32_t *jobs, int n_jobs, double evo, double mut, uint64_t seed, uint32_t generation) {
  if (n_jobs < 1) return OFX_OK;
  const dim3 grid((G + 255u) / 256u, (unsigned)(n_jobs < 65535 ? n_jobs : 65535));
  hipLaunchKernelGGL(k_pop_breed, grid, dim3(256), 0, h->stream, data, jobs, n_jobs, G, first, (uint32_t)layers[0],
                     (uint32_t)layers[1], evo, mut, ofx_key(seed), generation);
  OFX_HIP(hipGetLastError());
  return OFX_OK;
}

extern "C" int ofx_population_init(ofx_handle *h, uint64_t seed, uint32_t generation) {
  ofx_population *p;
  int rc = need_population(h, "ofx_population_init", &p);
  if (rc) return rc;
  OFX_HIP(hipSetDevice(h->cfg.device));
  return launch_breed(h, p->data, p->G, p->first, p->layers, nullptr, (int)p->P, 0.0, 0.0, seed, generation);
}

// host <-> storage order of one genome: the first layer is transposed, the rest is the element order
static int check_slot(ofx_population *p, const char *who, int64_t slot, const void *w, const void *b) {
  if (!w || !b) { ofx_set_error("%s: null argument", who); return OFX_ERR_INVALID; }
  if (slot < 0 || slot >= p->P) { ofx_set_error("%s: slot %lld outside [0, %lld)", who, (long long)slot, (long long)p->P); return OFX_ERR_INVALID; }
  return OFX_OK;
}

// one genome in storage order at `src` -> the element order on the host (weights, then biases), and back; both wait
// for the handle's stream.  Stated once for the population's slots and the ES centre and members.
static int genome_to_host(ofx_handle *h, const double *src, const int32_t *layers, uint32_t first, uint32_t n_w,
                          uint32_t G, double *weights_host, double *biases_host) {
  std::vector<double> tmp(first);
  OFX_HIP(hipStreamSynchronize(h->stream));
  OFX_HIP(hipMemcpy(tmp.data(), src, (size_t)first * sizeof(double), hipMemcpyDeviceToHost));
  OFX_HIP(hipMemcpy(weights_host + first, src + first, (size_t)(n_w - first) * sizeof(double), hipMemcpyDeviceToHost));
  OFX_HIP(hipMemcpy(biases_host, src + n_w, (size_t)(G - n_w) * sizeof(double), hipMemcpyDeviceToHost));
  const size_t nin = (size_t)layers[0], n1 = (size_t)layers[1];
  for (size_t k = 0; k < nin; k++)
    for (size_t o = 0; o < n1; o++) weights_host[o * nin + k] = tmp[k * n1 + o];
  return OFX_OK;
}

static int genome_from_host(ofx_handle *h, double *dst, const int32_t *layers, uint32_t first, uint32_t n_w, uint32_t G,
                            const double *weights_host, const double *biases_host) {
  std::vector<double> tmp(first);
  const size_t nin = (size_t)layers[0], n1 = (size_t)layers[1];
  for (size_t k = 0; k < nin; k++)
    for (size_t o = 0; o < n1; o++) tmp[k * n1 + o] = weights_host[o * nin + k];
  OFX_HIP(hipStreamSynchronize(h->stream));
  OFX_HIP(hipMemcpy(dst, tmp.data(), (size_t)first * sizeof(double), hipMemcpyHostToDevice));
  OFX_HIP(hipMemcpy(dst + first, weights_host + first, (size_t)(n_w - first) * sizeof(double), hipMemcpyHostToDevice));
  OFX_HIP(hipMemcpy(dst + n_w, biases_host, (size_t)(G - n_w) * sizeof(double), hipMemcpyHostToDevice));
  return OFX_OK;
}

extern "C" int ofx_population_get(ofx_handle *h, int64_t slot, double *weights_host, double *biases_host) {
  ofx_population *p;
  int rc = need_population(h, "ofx_population_get", &p);
  if (rc || (rc = check_slot(p, "ofx_population_get", slot, weights_host, biases_host))) return rc;
  OFX_HIP(hipSetDevice(h->cfg.device));
  return genome_to_host(h, p->data + (size_t)slot * p->G, p->layers, p->first, p->n_w, p->G, weights_host, biases_host);
}

extern "C" int ofx_population_set(ofx_handle *h, int64_t slot, const double *weights_host, const double *biases_host) {
  ofx_population *p;
  int rc = need_population(h, "ofx_population_set", &p);
  if (rc || (rc = check_slot(p, "ofx_population_set", slot, weights_host, biases_host))) return rc;
  OFX_HIP(hipSetDevice(h->cfg.device));
  return genome_from_host(h, p->data + (size_t)slot * p->G, p->layers, p->first, p->n_w, p->G, weights_host, biases_host);
}

extern "C" int ofx_population_breed(ofx_handle *h, const int32_t *plan_host, double evolution_rate, double mutation_rate,
                                    uint64_t seed, uint32_t generation) {
  ofx_population *p;
  int rc = need_population(h, "ofx_population_breed", &p);
  if (rc) return rc;
  if (!plan_host) { ofx_set_error("ofx_population_breed: null plan"); return OFX_ERR_INVALID; }
  if (!(evolution_rate == evolution_rate) || !(mutation_rate == mutation_rate)) {
    ofx_set_error("ofx_population_breed: a rate is NaN");
    return OFX_ERR_INVALID;
  }
  // the whole plan is checked before anything is written: sources are never destinations
  std::vector<int32_t> jobs;
  for (int64_t s = 0; s < p->P; s++) {
    const int32_t q = plan_host[s];
    if (q < -1 || (int64_t)q >= p->P) {
      ofx_set_error("ofx_population_breed: plan[%lld] = %d outside [-1, %lld)", (long long)s, q, (long long)p->P);
      return OFX_ERR_INVALID;
    }
    if (q == (int32_t)s) continue;
    if (q >= 0 && plan_host[q] != q) {
      ofx_set_error("ofx_population_breed: plan[%lld] = %d, but slot %d is not kept (plan[%d] = %d): a parent must keep its slot",
                    (long long)s, q, q, q, plan_host[q]);
      return OFX_ERR_INVALID;
    }
    jobs.push_back((int32_t)s);
    jobs.push_back(q);
  }
  if (jobs.empty()) return OFX_OK;
  OFX_HIP(hipSetDevice(h->cfg.device));
  OFX_HIP(hipStreamSynchronize(h->stream));  // the last breed may still read the job list
  OFX_HIP(hipMemcpy(p->jobs, jobs.data(), jobs.size() * sizeof(int32_t), hipMemcpyHostToDevice));
  return launch_breed(h, p->data, p->G, p->first, p->layers, p->jobs, (int)(jobs.size() / 2), evolution_rate,
                      mutation_rate, seed, generation);
}

extern "C" int ofx_population_act(ofx_handle *h, const int32_t *genome_of, ofx_action *actions, double *y) {
  ofx_population *p;
  int rc = need_population(h, "ofx_population_act", &p);
  if (rc) return rc;
  if (!genome_of || !actions) { ofx_set_error("ofx_population_act: null argument"); return OFX_ERR_INVALID; }
  if (!h->spawned) { ofx_set_error("You must execute analyse_battleground first."); return OFX_ERR_STATE; }
  const ofx_config &c = h->cfg;
  OFX_HIP(hipSetDevice(c.device));
  if ((rc = ofx_launch_raster(h, OFX_MAP_BITS_LSB, nullptr, nullptr))) return rc;
  const pop_net net = net_of(p);
  const int words = (int)(((size_t)c.width * c.height) >> 5);
  hipLaunchKernelGGL(k_pop_act, dim3((unsigned)(c.n_arenas * c.n_ships)), dim3(256), 0, h->stream, c.n_ships, c.width,
                     c.height, h->st, (const unsigned *)h->maps[OFX_MAP_BITS_LSB][0],
                     (const unsigned *)h->maps[OFX_MAP_BITS_LSB][1], words, p->data, (long long)p->P, p->G, p->first,
                     p->n_w, net, genome_of, actions, y);
  OFX_HIP(hipGetLastError());
  return OFX_OK;
}

// the one statement of ofx_population_learn's workspace (ofx_arena.h): NM ships, S activations per ship, P genomes
static void learn_layout(Arena &A, size_t NM, size_t S, size_t P, LearnWs &W) {
  W.sample_of = A.n<int32_t>(NM);
  W.count = A.n<int32_t>(P);
  W.a = A.d(NM * S);
  W.d = A.d(NM * S);
  W.head = A.d(NM * 8);
}

extern "C" int ofx_population_learn(ofx_handle *h, const int32_t *genome_of, const double *solution,
                                    const uint8_t *learn_mask, double rate, ofx_action *actions, double *y, double *err) {
  ofx_population *p;
  int rc = need_population(h, "ofx_population_learn", &p);
  if (rc) return rc;
  if (!genome_of || !solution) { ofx_set_error("ofx_population_learn: genome_of or solution is NULL"); return OFX_ERR_INVALID; }
  if (!(rate - rate == 0.0)) { ofx_set_error("ofx_population_learn: rate is not finite"); return OFX_ERR_INVALID; }
  if (!h->spawned) { ofx_set_error("You must execute analyse_battleground first."); return OFX_ERR_STATE; }
  const ofx_config &c = h->cfg;
  OFX_HIP(hipSetDevice(c.device));
  const size_t NM = (size_t)c.n_arenas * c.n_ships;
  size_t S = 0;
  for (int i = 1; i < p->n_layers; i++) S += (size_t)p->layers[i];
  LearnWs ws;
  Arena measure;
  learn_layout(measure, NM, S, (size_t)p->P, ws);
  if ((rc = ofx_ensure_scratch(h, measure.used))) return rc;
  Arena A(h->scratch, measure.used);
  learn_layout(A, NM, S, (size_t)p->P, ws);
  if (!A.ok()) { ofx_set_error("ofx_population_learn: the workspace does not fit its block of %zu bytes", measure.used); return OFX_ERR_STATE; }
  if ((rc = ofx_launch_raster(h, OFX_MAP_BITS_LSB, nullptr, nullptr))) return rc;
  OFX_HIP(hipMemsetAsync(ws.sample_of, 0xff, NM * sizeof(int32_t), h->stream));   // -1: no sample
  OFX_HIP(hipMemsetAsync(ws.count, 0, (size_t)p->P * sizeof(int32_t), h->stream));
  const pop_net net = net_of(p);
  const int words = (int)(((size_t)c.width * c.height) >> 5);
  const unsigned *sb = (const unsigned *)h->maps[OFX_MAP_BITS_LSB][0], *lb = (const unsigned *)h->maps[OFX_MAP_BITS_LSB][1];
  hipLaunchKernelGGL(k_pop_grad, dim3((unsigned)NM), dim3(256), 0, h->stream, c.n_ships, c.width, c.height, h->st, sb, lb,
                     words, p->data, (long long)p->P, p->G, p->first, p->n_w, net, (int)S, genome_of, solution, learn_mask,
                     actions, y, err, ws);
  OFX_HIP(hipGetLastError());
  if (rate == 0.0) return OFX_OK;                          // outputs and err only: no genome changes a bit
  hipLaunchKernelGGL(k_pop_apply, dim3((unsigned)p->P), dim3(256), 0, h->stream, (int)NM, c.n_ships, sb, lb, words,
                     p->data, p->G, p->first, p->n_w, net, (int)S, ws, rate);
  OFX_HIP(hipGetLastError());
  return OFX_OK;
}

extern "C" int ofx_population_targets(ofx_handle *h, const ofx_action *teacher, double *solution, uint8_t *mask) {
  if (!h || !teacher || !solution || !mask) { ofx_set_error("ofx_population_targets: null argument"); return OFX_ERR_INVALID; }
  const ofx_config &c = h->cfg;
  OFX_HIP(hipSetDevice(c.device));
  const int NM = c.n_arenas * c.n_ships;
  hipLaunchKernelGGL(k_pop_targets, dim3((NM + 255) / 256), dim3(256), 0, h->stream, NM, c.width, c.height, teacher,
                     solution, mask);
  OFX_HIP(hipGetLastError());
  return OFX_OK;
}

extern "C" int ofx_population_err_reduce(ofx_handle *h, double *err, double *acc) {
  if (!h || !err || !acc) { ofx_set_error("ofx_population_err_reduce: null argument"); return OFX_ERR_INVALID; }
  const ofx_config &c = h->cfg;
  OFX_HIP(hipSetDevice(c.device));
  hipLaunchKernelGGL(k_pop_err_reduce, dim3(1), dim3(256), 0, h->stream, c.n_arenas * c.n_ships, err, acc);
  OFX_HIP(hipGetLastError());
  return OFX_OK;
}

extern "C" int ofx_population_fitness(ofx_handle *h, const int32_t *genome_of, int64_t *sum, int32_t *count,
                                      int32_t reset) {
  ofx_population *p;
  int rc = need_population(h, "ofx_population_fitness", &p);
  if (rc) return rc;
  if (!genome_of || !sum || !count) { ofx_set_error("ofx_population_fitness: null argument"); return OFX_ERR_INVALID; }
  if (!h->spawned) { ofx_set_error("ofx_population_fitness before ofx_spawn"); return OFX_ERR_STATE; }
  OFX_HIP(hipSetDevice(h->cfg.device));
  if (reset) {
    OFX_HIP(hipMemsetAsync(sum, 0, (size_t)p->P * sizeof(int64_t), h->stream));
    OFX_HIP(hipMemsetAsync(count, 0, (size_t)p->P * sizeof(int32_t), h->stream));
  }
  const int NM = h->cfg.n_arenas * h->cfg.n_ships;
  hipLaunchKernelGGL(k_pop_fitness, dim3((NM + 255) / 256), dim3(256), 0, h->stream, NM, (long long)p->P,
                     h->st.last_score, genome_of, (unsigned long long *)sum, count);
  OFX_HIP(hipGetLastError());
  return OFX_OK;
}

// ---- evolution strategies: a population that is never stored (include/ofx.h, "evolution strategies") ----------------
// One centre genome theta of G doubles in the storage layout above.  Member m = 2i + b of P = 2 n_pairs is
// theta + (+-sigma) * eps(i, e), eps a pure function of (seed, pair, element, generation) on stream 12; member P is
// theta itself.  Nothing of a member is ever kept: the forward regenerates the noise of the rows it gathers, the
// generation step is one pass over theta.
//
// k_es_act     k_pop_act's launch shape and bodies (pop_walk, pop_forward, pop_emit: each still exists once) with the
//              es_member reader: one Philox evaluation per weight read, set cells x n1 + 8 n1 + the later layers per ship.
//              Lane layout, list order and the order of every sum are pop_forward's, so a member's y has the bits
//              k_pop_act gives on a stored genome holding the member's elements.  The centre (member P) goes through
//              pop_stored: no Philox on that path.
// k_es_update  one thread per storage position, the loop over the pairs inside: coalesced reads and writes of theta,
//              (pair, d) read wave-uniformly, the sum in ascending pair order in a register.  No floating-point atomics.
//              Compute-bound on Philox by design: G x n_pairs evaluations against 16 G bytes.
// k_es_step    k_es_update's pass with the moments m (and, under Adam, v) read and written at theta's position: the
//              same G x n_pairs evaluations against 32 or 48 G bytes.  With stats, a
//              fixed-order sum per workgroup and k_es_stats over the workgroups; no floating-point atomics.
// k_es_member  a member materialised into a G-double buffer, for ofx_es_member.
struct ofx_es {
  int n_layers;
  int32_t layers[POP_MAX_LAYERS];
  uint32_t G, first, n_w;   // as in ofx_population
  double *theta;            // [G] the centre
  double *member;           // [G] ofx_es_member's buffer, allocated at its first call
  double *d;                // [d_cap] the nonzero pair weights of the running ofx_es_update, ascending pair order
  uint32_t *d_pair;         // [d_cap] their pairs
  size_t d_cap;
  double *m, *v;            // [G] each, theta's layout: the optimiser's moments (ofx_es_opt_create), null = none
  double *part;             // [3][ceil(G / 256)] k_es_step's per-workgroup sums of q^2, step^2, theta'^2
  double *sigma;            // [G] theta's layout: the per-element exploration width (ofx_es_sigma_create), null = none
  double *s;                // [s_cap] the listed pairs' sigma weights of the running ofx_es_sigma_step, beside d / d_pair
  size_t s_cap;
  double *sigma_part;       // [5][ceil(G / 256)] k_es_sigma_step's per-workgroup sums, allocated with sigma
};

// eps(i, e): the four stream-12 words of (pair, element, generation) summed, centred and scaled to (-2, 2).  The words
// are below 2^32 and their sum below 2^34, so the float64 sum IS the integer sum, and so are the difference from
// 2^33 - 2 and the scaling by 2^-32: every step is exact, no rounding and no libm between here and the oracle.
__host__ __device__ inline double es_eps(uint32_t pair, uint32_t e, uint32_t generation, ofx_rng_key key) {
  uint32_t r[4];
  ofx_philox4x32_10(pair, e, generation, OFX_ES_STREAM, key, r);
  const double S = ((double)r[0] + (double)r[1]) + ((double)r[2] + (double)r[3]);
  return (S - 8589934590.0) * 0x1p-32;
}

// pop_forward's reader for member 2 * pair + b of the centre `theta`: w = theta + (ss * eps), ss = +sigma or -sigma, the
// product rounded, then the sum (the library is built with -ffp-contract=off).  In the first layer storage position
// k * n1 + o is element o * nin + k; behind it the position is the element.
struct es_member {
  const double *theta;
  uint32_t nin, pair, generation;
  ofx_rng_key key;
  double ss;
  __device__ __forceinline__ double noisy(double w, uint32_t e) const {
    const double t = ss * es_eps(pair, e, generation, key);
    return w + t;
  }
  __device__ __forceinline__ double first(size_t k, int o, int n1) const {
    return noisy(theta[k * n1 + o], (uint32_t)o * nin + (uint32_t)k);
  }
  __device__ __forceinline__ double at(size_t s) const { return noisy(theta[s], (uint32_t)s); }
};

__global__ __launch_bounds__(256) void k_es_act(int M, int W, int H, ofx_state st, const unsigned *ship_bits,
                                                const unsigned *laser_bits, int words, const double *theta, int P,
                                                uint32_t first, uint32_t n_w, pop_net net, double sigma, ofx_rng_key key,
                                                uint32_t generation, const int32_t *member_of, ofx_action *actions,
                                                double *y) {
  __shared__ uint32_t list[4][POP_LIST];
  __shared__ double part[4][64];
  __shared__ double act[2][POP_MAX_WIDTH];
  const int s = blockIdx.x, a = s / M;
  const int32_t m = member_of[s];
  if (m < 0 || m > P || !st.alive[s]) return;              // uniform over the workgroup
  int cur;
  if (m == P) {                                            // the centre: the stored-genome path, no Philox
    const pop_stored rd = {theta};
    cur = pop_forward<false>(s, a, W, H, st, ship_bits, laser_bits, words, rd, first, n_w, net, list, part, act, nullptr);
  } else {
    const es_member rd = {theta, (uint32_t)net.layers[0], (uint32_t)m >> 1, generation, key, (m & 1) ? -sigma : sigma};
    cur = pop_forward<false>(s, a, W, H, st, ship_bits, laser_bits, words, rd, first, n_w, net, list, part, act, nullptr);
  }
  pop_emit(s, W, H, act[cur], actions, y);
}

// out[s] = member `m` of P at storage position s (m == P: the centre)
__global__ __launch_bounds__(256) void k_es_member(const double *theta, double *out, uint32_t G, uint32_t first,
                                                   uint32_t nin, uint32_t n1, int m, int P, double sigma,
                                                   ofx_rng_key key, uint32_t generation) {
  const uint32_t s = blockIdx.x * 256u + threadIdx.x;
  if (s >= G) return;
  double w = theta[s];
  if (m != P) {
    const double ss = (m & 1) ? -sigma : sigma;
    const double t = ss * es_eps((uint32_t)m >> 1, pop_element(s, first, nin, n1), generation, key);
    w = w + t;
  }
  out[s] = w;
}

// theta[e] += scale * (sum over the listed pairs, in list order, of d * eps(pair, e)): every product and sum rounded on
// its own, the sum kept in a register.  The list holds the pairs with d != 0 in ascending order (ofx_es_update).
__global__ __launch_bounds__(256) void k_es_update(double *theta, const double *__restrict__ d,
                                                   const uint32_t *__restrict__ d_pair, int n, uint32_t G,
                                                   uint32_t first, uint32_t nin, uint32_t n1, double scale,
                                                   ofx_rng_key key, uint32_t generation) {
  const uint32_t s = blockIdx.x * 256u + threadIdx.x;
  if (s >= G) return;
  const uint32_t e = pop_element(s, first, nin, n1);
  double g = 0.0;
#pragma unroll 4
  for (int j = 0; j < n; j++) {                            // d[j], d_pair[j]: the same address in every lane
    const double t = d[j] * es_eps(d_pair[j], e, generation, key);
    g = g + t;
  }
  const double step = scale * g;
  theta[s] = theta[s] + step;
}

// the scalars of ofx_es_step's law (include/ofx.h), all the caller's
struct es_law {
  double gscale, decay, alpha, c1, k1, c2, k2, eps;
};

// ofx_es_step: k_es_update's shape - one thread per storage position, the element by pop_element, the pair loop inside -
// with the moments m and v at the same position as theta (coalesced, one read and one write each; momentum never
// touches v).  Every line of the law is one rounded float64 operation; sqrt and / are the correctly rounded ones.
// STATS: the workgroup's sums of q^2, step^2 and theta'^2 go to part[k][blockIdx.x], added as a pairwise tree over the
// thread index (stride 128, 64, .. 1: x[t] = x[t] + x[t + stride]; a position past G adds +0.0); k_es_stats adds the
// workgroups'.  Without STATS none of that is compiled in.
template <bool ADAM, bool STATS>
__global__ __launch_bounds__(256) void k_es_step(double *theta, double *m, double *v, const double *__restrict__ d,
                                                 const uint32_t *__restrict__ d_pair, int n, uint32_t G, uint32_t first,
                                                 uint32_t nin, uint32_t n1, es_law c, ofx_rng_key key,
                                                 uint32_t generation, double *part) {
  const uint32_t s = blockIdx.x * 256u + threadIdx.x;
  double sq0 = 0.0, sq1 = 0.0, sq2 = 0.0;
  if (s < G) {
    const uint32_t e = pop_element(s, first, nin, n1);
    // k_es_update's sum, term for term.  es_eps is stated once; the loop stands in both kernels, because one shared
    // body changed k_es_update's instruction stream (an inverted loop branch, a commuted final add)
    double g = 0.0;
#pragma unroll 4
    for (int j = 0; j < n; j++) {
      const double t = d[j] * es_eps(d_pair[j], e, generation, key);
      g = g + t;
    }
    const double w = theta[s];
    const double ghat = c.gscale * g;
    const double wd = c.decay * w;
    const double q = ghat - wd;
    const double t1 = c.c1 * m[s];
    const double t2 = c.k1 * q;
    const double mn = t1 + t2;
    double quo = mn;
    if (ADAM) {
      const double qq = q * q;
      const double t3 = c.c2 * v[s];
      const double t4 = c.k2 * qq;
      const double vn = t3 + t4;
      const double r = sqrt(vn);
      const double den = r + c.eps;
      quo = mn / den;
      v[s] = vn;
    }
    const double step = c.alpha * quo;
    const double wn = w + step;
    m[s] = mn;
    theta[s] = wn;
    if (STATS) {
      sq0 = q * q;
      sq1 = step * step;
      sq2 = wn * wn;
    }
  }
  if (STATS) {
    __shared__ double red[3][256];
    const int tid = threadIdx.x;
    red[0][tid] = sq0;
    red[1][tid] = sq1;
    red[2][tid] = sq2;
    __syncthreads();
    for (int stride = 128; stride > 0; stride >>= 1) {
      if (tid < stride) {
#pragma unroll
        for (int k = 0; k < 3; k++) red[k][tid] = red[k][tid] + red[k][tid + stride];
      }
      __syncthreads();
    }
    if (tid < 3) part[(size_t)tid * gridDim.x + blockIdx.x] = red[tid][0];
  }
}

// stats[k] = the nb workgroup sums part[k][0 .. nb): thread t adds entries t, t + 256, ... in that order from 0.0, then
// thread k adds the 256 thread sums in thread order.  One workgroup: the same bits every call.  R rows: 3 for
// ofx_es_step, 5 for ofx_es_sigma_step.
template <int R>
__global__ __launch_bounds__(256) void k_es_stats(const double *part, int nb, double *stats) {
  __shared__ double sum[R][256];
  const int tid = threadIdx.x;
#pragma unroll
  for (int k = 0; k < R; k++) {
    double a = 0.0;
    for (int j = tid; j < nb; j += 256) a = a + part[(size_t)k * nb + j];
    sum[k][tid] = a;
  }
  __syncthreads();
  if (tid < R) {
    double t = sum[tid][0];
    for (int q = 1; q < 256; q++) t = t + sum[tid][q];
    stats[tid] = t;
  }
}

// ---- per-element adaptive sigma (include/ofx.h: ofx_es_sigma_*) ----
// pop_forward's reader for member 2 * pair + b with a width per element: w = theta + ((sgn * sigma) * eps), sgn = +1 or
// -1 (the sign is exact), the product rounded, then the sum.  sigma is read at the storage position theta is read at.
struct es_sigma_member {
  const double *theta, *sigma;
  uint32_t nin, pair, generation;
  ofx_rng_key key;
  double sgn;
  __device__ __forceinline__ double noisy(double w, double sg, uint32_t e) const {
    const double ss = sgn * sg;
    const double t = ss * es_eps(pair, e, generation, key);
    return w + t;
  }
  __device__ __forceinline__ double first(size_t k, int o, int n1) const {
    const size_t s = k * n1 + o;
    return noisy(theta[s], sigma[s], (uint32_t)o * nin + (uint32_t)k);
  }
  __device__ __forceinline__ double at(size_t s) const { return noisy(theta[s], sigma[s], (uint32_t)s); }
};

// k_es_act with the es_sigma_member reader; the centre still goes through pop_stored
__global__ __launch_bounds__(256) void k_es_sigma_act(int M, int W, int H, ofx_state st, const unsigned *ship_bits,
                                                      const unsigned *laser_bits, int words, const double *theta,
                                                      const double *sigma, int P, uint32_t first, uint32_t n_w,
                                                      pop_net net, ofx_rng_key key, uint32_t generation,
                                                      const int32_t *member_of, ofx_action *actions, double *y) {
  __shared__ uint32_t list[4][POP_LIST];
  __shared__ double part[4][64];
  __shared__ double act[2][POP_MAX_WIDTH];
  const int s = blockIdx.x, a = s / M;
  const int32_t m = member_of[s];
  if (m < 0 || m > P || !st.alive[s]) return;              // uniform over the workgroup
  int cur;
  if (m == P) {
    const pop_stored rd = {theta};
    cur = pop_forward<false>(s, a, W, H, st, ship_bits, laser_bits, words, rd, first, n_w, net, list, part, act, nullptr);
  } else {
    const es_sigma_member rd = {theta, sigma, (uint32_t)net.layers[0], (uint32_t)m >> 1, generation, key,
                                (m & 1) ? -1.0 : 1.0};
    cur = pop_forward<false>(s, a, W, H, st, ship_bits, laser_bits, words, rd, first, n_w, net, list, part, act, nullptr);
  }
  pop_emit(s, W, H, act[cur], actions, y);
}

// out[s] = member `m` of P at storage position s under sigma[s] (m == P: the centre)
__global__ __launch_bounds__(256) void k_es_sigma_member(const double *theta, const double *sigma, double *out,
                                                         uint32_t G, uint32_t first, uint32_t nin, uint32_t n1, int m,
                                                         int P, ofx_rng_key key, uint32_t generation) {
  const uint32_t s = blockIdx.x * 256u + threadIdx.x;
  if (s >= G) return;
  double w = theta[s];
  if (m != P) {
    const double sgn = (m & 1) ? -1.0 : 1.0;
    const double ss = sgn * sigma[s];
    const double t = ss * es_eps((uint32_t)m >> 1, pop_element(s, first, nin, n1), generation, key);
    w = w + t;
  }
  out[s] = w;
}

__global__ __launch_bounds__(256) void k_es_fill(double *out, uint32_t G, double value) {
  const uint32_t s = blockIdx.x * 256u + threadIdx.x;
  if (s < G) out[s] = value;
}

// the scalars ofx_es_sigma_step's law adds to es_law
struct es_sigma_law {
  double srate, smin, smax;
};

#define ES_SIGMA_THIRD 0x1.5555555555555p-2               /* eps's variance to the last bit but 2^-64 */

// ofx_es_sigma_step: k_es_step's shape - one thread per storage position, the element by pop_element, the pair loop
// inside - with a second register sum beside g: qs = sum s[j] * (eps^2 - 1/3), from the SAME eps evaluation, so the
// G x n Philox evaluations of the step are not repeated for sigma.  theta, sigma, m and v lie at the same position:
// each read once and written once, coalesced (PLAIN touches neither moment, MOMENTUM not v).  Every line is one rounded
// float64 operation.  The optimiser's lines are restated from k_es_step, not shared with it, for the reason given at
// its loop.  STATS: five workgroup sums - q^2, step^2, theta'^2, sigma'^2, clamped elements - in k_es_step's tree.
template <int RULE, bool STATS>
__global__ __launch_bounds__(256) void k_es_sigma_step(double *theta, double *sigma, double *m, double *v,
                                                       const double *__restrict__ d, const double *__restrict__ sw,
                                                       const uint32_t *__restrict__ d_pair, int n, uint32_t G,
                                                       uint32_t first, uint32_t nin, uint32_t n1, es_law c,
                                                       es_sigma_law z, ofx_rng_key key, uint32_t generation,
                                                       double *part) {
  const uint32_t s = blockIdx.x * 256u + threadIdx.x;
  double sq0 = 0.0, sq1 = 0.0, sq2 = 0.0, sq3 = 0.0, sq4 = 0.0;
  if (s < G) {
    const uint32_t e = pop_element(s, first, nin, n1);
    double g = 0.0, qs = 0.0;
#pragma unroll 4
    for (int j = 0; j < n; j++) {                          // d[j], sw[j], d_pair[j]: the same address in every lane
      const double x = es_eps(d_pair[j], e, generation, key);
      const double t = d[j] * x;
      g = g + t;
      const double xx = x * x;
      const double cc = xx - ES_SIGMA_THIRD;
      const double u = sw[j] * cc;
      qs = qs + u;
    }
    const double w = theta[s];
    const double sg = sigma[s];
    const double sgg = sg * g;
    const double ghat = c.gscale * sgg;
    const double wd = c.decay * w;
    const double q = ghat - wd;
    double step;
    if (RULE == OFX_ES_RULE_PLAIN) {
      step = c.alpha * q;
    } else {
      const double t1 = c.c1 * m[s];
      const double t2 = c.k1 * q;
      const double mn = t1 + t2;
      double quo = mn;
      if (RULE == OFX_ES_RULE_ADAM) {
        const double qq = q * q;
        const double t3 = c.c2 * v[s];
        const double t4 = c.k2 * qq;
        const double vn = t3 + t4;
        const double r = sqrt(vn);
        const double den = r + c.eps;
        quo = mn / den;
        v[s] = vn;
      }
      step = c.alpha * quo;
      m[s] = mn;
    }
    const double wn = w + step;
    theta[s] = wn;
    const double r = z.srate * qs;
    const double f = 1.0 + r;
    double sn = sg * f;
    bool clamped = false;
    if (sn < z.smin) { sn = z.smin; clamped = true; }
    if (sn > z.smax) { sn = z.smax; clamped = true; }
    sigma[s] = sn;
    if (STATS) {
      sq0 = q * q;
      sq1 = step * step;
      sq2 = wn * wn;
      sq3 = sn * sn;
      sq4 = clamped ? 1.0 : 0.0;
    }
  }
  if (STATS) {
    __shared__ double red[5][256];
    const int tid = threadIdx.x;
    red[0][tid] = sq0;
    red[1][tid] = sq1;
    red[2][tid] = sq2;
    red[3][tid] = sq3;
    red[4][tid] = sq4;
    __syncthreads();
    for (int stride = 128; stride > 0; stride >>= 1) {
      if (tid < stride) {
#pragma unroll
        for (int k = 0; k < 5; k++) red[k][tid] = red[k][tid] + red[k][tid + stride];
      }
      __syncthreads();
    }
    if (tid < 5) part[(size_t)tid * gridDim.x + blockIdx.x] = red[tid][0];
  }
}

static ofx_es *&es_of(ofx_handle *h) { return h->es; }

static pop_net net_of(const ofx_es *p) {
  pop_net net;
  net.n_layers = p->n_layers;
  for (int i = 0; i < POP_MAX_LAYERS; i++) net.layers[i] = i < p->n_layers ? p->layers[i] : 0;
  return net;
}

static void es_sigma_free(ofx_es *p) {
  if (p->sigma) (void)hipFree(p->sigma);
  if (p->s) (void)hipFree(p->s);
  if (p->sigma_part) (void)hipFree(p->sigma_part);
  p->sigma = p->s = p->sigma_part = nullptr;
  p->s_cap = 0;
}

static void es_opt_free(ofx_es *p) {
  if (p->m) (void)hipFree(p->m);
  if (p->v) (void)hipFree(p->v);
  if (p->part) (void)hipFree(p->part);
  p->m = p->v = p->part = nullptr;
}

void ofx_es_free(ofx_handle *h) {
  ofx_es *p = es_of(h);
  if (!p) return;
  if (p->theta) (void)hipFree(p->theta);
  if (p->member) (void)hipFree(p->member);
  if (p->d) (void)hipFree(p->d);
  if (p->d_pair) (void)hipFree(p->d_pair);
  es_opt_free(p);
  es_sigma_free(p);
  delete p;
  es_of(h) = nullptr;
}

static int need_es(ofx_handle *h, const char *who, ofx_es **out) {
  if (!h) { ofx_set_error("%s: null handle", who); return OFX_ERR_INVALID; }
  if (!es_of(h)) { ofx_set_error("%s: the handle holds no ES centre (ofx_es_create)", who); return OFX_ERR_STATE; }
  *out = es_of(h);
  return OFX_OK;
}

// P = 2 n_pairs members and their noise scale
static int check_members(const char *who, int64_t P, double sigma) {
  if (P < 2 || (P & 1) || P > 0x7ffffffell) {
    ofx_set_error("%s: P must be even and in [2, 2^31 - 2], two members per pair (got %lld)", who, (long long)P);
    return OFX_ERR_INVALID;
  }
  if (!(sigma - sigma == 0.0) || !(sigma > 0.0)) {
    ofx_set_error("%s: sigma must be finite and > 0 (got %g)", who, sigma);
    return OFX_ERR_INVALID;
  }
  return OFX_OK;
}

extern "C" int ofx_es_create(ofx_handle *h, const int32_t *layers, int32_t n_layers) {
  if (!h || !layers) { ofx_set_error("ofx_es_create: null argument"); return OFX_ERR_INVALID; }
  if (es_of(h)) { ofx_set_error("ofx_es_create: the handle already holds an ES centre (ofx_es_destroy)"); return OFX_ERR_STATE; }
  unsigned long long n_w, n_b;
  const int rc = check_topology(h, "ofx_es_create", layers, n_layers, &n_w, &n_b);
  if (rc) return rc;
  OFX_HIP(hipSetDevice(h->cfg.device));
  ofx_es *p = new (std::nothrow) ofx_es();
  if (!p) { ofx_set_error("ofx_es_create: out of host memory"); return OFX_ERR_INVALID; }
  p->n_layers = n_layers;
  for (int i = 0; i < n_layers; i++) p->layers[i] = layers[i];
  p->G = (uint32_t)(n_w + n_b);
  p->first = (uint32_t)((unsigned long long)layers[0] * layers[1]);
  p->n_w = (uint32_t)n_w;
  p->theta = p->member = p->d = nullptr;
  p->m = p->v = p->part = nullptr;
  p->d_pair = nullptr;
  p->d_cap = 0;
  p->sigma = p->s = p->sigma_part = nullptr;
  p->s_cap = 0;
  const size_t bytes = (size_t)p->G * sizeof(double);
  const hipError_t e = hipMalloc((void **)&p->theta, bytes);
  if (e != hipSuccess) {
    (void)hipGetLastError();
    ofx_set_error("ofx_es_create: allocating %zu bytes for a centre of %u elements failed: %s", bytes, p->G,
                  hipGetErrorString(e));
    delete p;
    return OFX_ERR_HIP;
  }
  es_of(h) = p;
  return OFX_OK;
}

extern "C" int ofx_es_destroy(ofx_handle *h) {
  if (!h) { ofx_set_error("ofx_es_destroy: null handle"); return OFX_ERR_INVALID; }
  OFX_HIP(hipSetDevice(h->cfg.device));
  OFX_HIP(hipStreamSynchronize(h->stream));
  ofx_es_free(h);
  return OFX_OK;
}

extern "C" int ofx_es_init(ofx_handle *h, uint64_t seed, uint32_t generation) {
  ofx_es *p;
  int rc = need_es(h, "ofx_es_init", &p);
  if (rc) return rc;
  OFX_HIP(hipSetDevice(h->cfg.device));
  // the fresh genome of slot 0: k_pop_breed with one job and no job list, as ofx_population_init runs it
  return launch_breed(h, p->theta, p->G, p->first, p->layers, nullptr, 1, 0.0, 0.0, seed, generation);
}

extern "C" int ofx_es_get(ofx_handle *h, double *weights_host, double *biases_host) {
  ofx_es *p;
  int rc = need_es(h, "ofx_es_get", &p);
  if (rc) return rc;
  if (!weights_host || !biases_host) { ofx_set_error("ofx_es_get: null argument"); return OFX_ERR_INVALID; }
  OFX_HIP(hipSetDevice(h->cfg.device));
  return genome_to_host(h, p->theta, p->layers, p->first, p->n_w, p->G, weights_host, biases_host);
}

extern "C" int ofx_es_set(ofx_handle *h, const double *weights_host, const double *biases_host) {
  ofx_es *p;
  int rc = need_es(h, "ofx_es_set", &p);
  if (rc) return rc;
  if (!weights_host || !biases_host) { ofx_set_error("ofx_es_set: null argument"); return OFX_ERR_INVALID; }
  OFX_HIP(hipSetDevice(h->cfg.device));
  return genome_from_host(h, p->theta, p->layers, p->first, p->n_w, p->G, weights_host, biases_host);
}

// the G-double buffer a member is materialised into, allocated at the first call that needs it (`who`)
static int member_buffer(ofx_es *p, const char *who) {
  if (p->member) return OFX_OK;
  const hipError_t e = hipMalloc((void **)&p->member, (size_t)p->G * sizeof(double));
  if (e != hipSuccess) {
    (void)hipGetLastError();
    p->member = nullptr;
    ofx_set_error("%s: allocating %zu bytes failed: %s", who, (size_t)p->G * sizeof(double), hipGetErrorString(e));
    return OFX_ERR_HIP;
  }
  return OFX_OK;
}

extern "C" int ofx_es_member(ofx_handle *h, int64_t member, int64_t P, double sigma, uint64_t seed, uint32_t generation,
                             double *weights_host, double *biases_host) {
  ofx_es *p;
  int rc = need_es(h, "ofx_es_member", &p);
  if (rc || (rc = check_members("ofx_es_member", P, sigma))) return rc;
  if (!weights_host || !biases_host) { ofx_set_error("ofx_es_member: null argument"); return OFX_ERR_INVALID; }
  if (member < 0 || member > P) {
    ofx_set_error("ofx_es_member: member %lld outside [0, %lld] (P is the centre)", (long long)member, (long long)P);
    return OFX_ERR_INVALID;
  }
  OFX_HIP(hipSetDevice(h->cfg.device));
  if ((rc = member_buffer(p, "ofx_es_member"))) return rc;
  hipLaunchKernelGGL(k_es_member, dim3((p->G + 255u) / 256u), dim3(256), 0, h->stream, p->theta, p->member, p->G, p->first,
                     (uint32_t)p->layers[0], (uint32_t)p->layers[1], (int)member, (int)P, sigma, ofx_key(seed), generation);
  OFX_HIP(hipGetLastError());
  return genome_to_host(h, p->member, p->layers, p->first, p->n_w, p->G, weights_host, biases_host);
}

extern "C" int ofx_es_act(ofx_handle *h, const int32_t *member_of, int64_t P, double sigma, uint64_t seed,
                          uint32_t generation, ofx_action *actions, double *y) {
  ofx_es *p;
  int rc = need_es(h, "ofx_es_act", &p);
  if (rc || (rc = check_members("ofx_es_act", P, sigma))) return rc;
  if (!member_of || !actions) { ofx_set_error("ofx_es_act: null argument"); return OFX_ERR_INVALID; }
  if (!h->spawned) { ofx_set_error("You must execute analyse_battleground first."); return OFX_ERR_STATE; }
  const ofx_config &c = h->cfg;
  OFX_HIP(hipSetDevice(c.device));
  if ((rc = ofx_launch_raster(h, OFX_MAP_BITS_LSB, nullptr, nullptr))) return rc;
  const pop_net net = net_of(p);
  const int words = (int)(((size_t)c.width * c.height) >> 5);
  hipLaunchKernelGGL(k_es_act, dim3((unsigned)(c.n_arenas * c.n_ships)), dim3(256), 0, h->stream, c.n_ships, c.width,
                     c.height, h->st, (const unsigned *)h->maps[OFX_MAP_BITS_LSB][0],
                     (const unsigned *)h->maps[OFX_MAP_BITS_LSB][1], words, p->theta, (int)P, p->first, p->n_w, net, sigma,
                     ofx_key(seed), generation, member_of, actions, y);
  OFX_HIP(hipGetLastError());
  return OFX_OK;
}

extern "C" int ofx_es_fitness(ofx_handle *h, const int32_t *member_of, int64_t P, int64_t *sum, int32_t *count,
                              int32_t reset) {
  ofx_es *p;
  int rc = need_es(h, "ofx_es_fitness", &p);
  if (rc || (rc = check_members("ofx_es_fitness", P, 1.0))) return rc;
  if (!member_of || !sum || !count) { ofx_set_error("ofx_es_fitness: null argument"); return OFX_ERR_INVALID; }
  if (!h->spawned) { ofx_set_error("ofx_es_fitness before ofx_spawn"); return OFX_ERR_STATE; }
  OFX_HIP(hipSetDevice(h->cfg.device));
  const size_t slots = (size_t)P + 1;                      // slot P: the centre
  if (reset) {
    OFX_HIP(hipMemsetAsync(sum, 0, slots * sizeof(int64_t), h->stream));
    OFX_HIP(hipMemsetAsync(count, 0, slots * sizeof(int32_t), h->stream));
  }
  const int NM = h->cfg.n_arenas * h->cfg.n_ships;
  hipLaunchKernelGGL(k_pop_fitness, dim3((NM + 255) / 256), dim3(256), 0, h->stream, NM, (long long)slots,
                     h->st.last_score, member_of, (unsigned long long *)sum, count);
  OFX_HIP(hipGetLastError());
  return OFX_OK;
}

// d_host[n_pairs] as the generation steps take it (`who`): not NULL, n_pairs in range
static int check_pairs(const char *who, const double *d_host, int64_t n_pairs) {
  if (!d_host) { ofx_set_error("%s: null argument", who); return OFX_ERR_INVALID; }
  if (n_pairs < 1 || n_pairs > 0x3fffffffll) {
    ofx_set_error("%s: n_pairs must be in [1, 2^30) (got %lld)", who, (long long)n_pairs);
    return OFX_ERR_INVALID;
  }
  return OFX_OK;
}

// The pairs with a weight, ascending.  A pair with d == 0 adds +-0 to a sum that starts at +0.0 and can never be -0.0
// (x + (-x) rounds to +0), so leaving it out changes no bit: ties and incomplete pairs, the common case, cost nothing.
static int nonzero_pairs(const char *who, const double *d_host, int64_t n_pairs, std::vector<double> &d,
                         std::vector<uint32_t> &pair) {
  for (int64_t i = 0; i < n_pairs; i++) {
    if (!(d_host[i] - d_host[i] == 0.0)) { ofx_set_error("%s: d[%lld] is not finite", who, (long long)i); return OFX_ERR_INVALID; }
    if (d_host[i] != 0.0) { d.push_back(d_host[i]); pair.push_back((uint32_t)i); }
  }
  return OFX_OK;
}

// the list into the centre's device copy, after the work already on the handle's stream
static int upload_pairs(ofx_handle *h, ofx_es *p, const std::vector<double> &d, const std::vector<uint32_t> &pair) {
  OFX_HIP(hipSetDevice(h->cfg.device));
  OFX_HIP(hipStreamSynchronize(h->stream));  // the last step may still read the list
  if (d.size() > p->d_cap) {
    if (p->d) (void)hipFree(p->d);
    if (p->d_pair) (void)hipFree(p->d_pair);
    p->d = nullptr;
    p->d_pair = nullptr;
    p->d_cap = 0;
    OFX_HIP(hipMalloc((void **)&p->d, d.size() * sizeof(double)));
    OFX_HIP(hipMalloc((void **)&p->d_pair, d.size() * sizeof(uint32_t)));
    p->d_cap = d.size();
  }
  if (!d.empty()) {
    OFX_HIP(hipMemcpy(p->d, d.data(), d.size() * sizeof(double), hipMemcpyHostToDevice));
    OFX_HIP(hipMemcpy(p->d_pair, pair.data(), pair.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
  }
  return OFX_OK;
}

extern "C" int ofx_es_update(ofx_handle *h, const double *d_host, int64_t n_pairs, double scale, uint64_t seed,
                             uint32_t generation) {
  ofx_es *p;
  int rc = need_es(h, "ofx_es_update", &p);
  if (rc || (rc = check_pairs("ofx_es_update", d_host, n_pairs))) return rc;
  if (!(scale - scale == 0.0)) { ofx_set_error("ofx_es_update: scale is not finite"); return OFX_ERR_INVALID; }
  std::vector<double> d;
  std::vector<uint32_t> pair;
  if ((rc = nonzero_pairs("ofx_es_update", d_host, n_pairs, d, pair)) || (rc = upload_pairs(h, p, d, pair))) return rc;
  hipLaunchKernelGGL(k_es_update, dim3((p->G + 255u) / 256u), dim3(256), 0, h->stream, p->theta, p->d, p->d_pair,
                     (int)d.size(), p->G, p->first, (uint32_t)p->layers[0], (uint32_t)p->layers[1], scale, ofx_key(seed),
                     generation);
  OFX_HIP(hipGetLastError());
  return OFX_OK;
}

// ---- the optimiser of the centre (include/ofx.h: ofx_es_opt_*, ofx_es_step) ----
static int need_opt(ofx_handle *h, const char *who, ofx_es **out) {
  const int rc = need_es(h, who, out);
  if (rc) return rc;
  if (!(*out)->m) { ofx_set_error("%s: the centre has no optimiser state (ofx_es_opt_create)", who); return OFX_ERR_STATE; }
  return OFX_OK;
}

extern "C" int ofx_es_opt_create(ofx_handle *h) {
  ofx_es *p;
  const int rc = need_es(h, "ofx_es_opt_create", &p);
  if (rc) return rc;
  if (p->m) { ofx_set_error("ofx_es_opt_create: the centre already has optimiser state (ofx_es_opt_destroy)"); return OFX_ERR_STATE; }
  OFX_HIP(hipSetDevice(h->cfg.device));
  const size_t bytes = (size_t)p->G * sizeof(double), nb = (p->G + 255u) / 256u;
  hipError_t e = hipMalloc((void **)&p->m, bytes);
  if (e == hipSuccess) e = hipMalloc((void **)&p->v, bytes);
  if (e == hipSuccess) e = hipMalloc((void **)&p->part, 3 * nb * sizeof(double));
  if (e != hipSuccess) {
    (void)hipGetLastError();
    ofx_set_error("ofx_es_opt_create: allocating 2 x %zu bytes for the moments of %u elements failed: %s", bytes, p->G,
                  hipGetErrorString(e));
    es_opt_free(p);
    return OFX_ERR_HIP;
  }
  e = hipMemsetAsync(p->m, 0, bytes, h->stream);
  if (e == hipSuccess) e = hipMemsetAsync(p->v, 0, bytes, h->stream);
  if (e != hipSuccess) {
    (void)hipGetLastError();
    ofx_set_error("ofx_es_opt_create: zeroing the moments failed: %s", hipGetErrorString(e));
    (void)hipStreamSynchronize(h->stream);
    es_opt_free(p);
    return OFX_ERR_HIP;
  }
  return OFX_OK;
}

extern "C" int ofx_es_opt_destroy(ofx_handle *h) {
  ofx_es *p;
  const int rc = need_opt(h, "ofx_es_opt_destroy", &p);
  if (rc) return rc;
  OFX_HIP(hipSetDevice(h->cfg.device));
  OFX_HIP(hipStreamSynchronize(h->stream));
  es_opt_free(p);
  return OFX_OK;
}

extern "C" int ofx_es_opt_get(ofx_handle *h, double *m_weights, double *m_biases, double *v_weights, double *v_biases) {
  ofx_es *p;
  int rc = need_opt(h, "ofx_es_opt_get", &p);
  if (rc) return rc;
  if (!m_weights || !m_biases || !v_weights || !v_biases) { ofx_set_error("ofx_es_opt_get: null argument"); return OFX_ERR_INVALID; }
  OFX_HIP(hipSetDevice(h->cfg.device));
  if ((rc = genome_to_host(h, p->m, p->layers, p->first, p->n_w, p->G, m_weights, m_biases))) return rc;
  return genome_to_host(h, p->v, p->layers, p->first, p->n_w, p->G, v_weights, v_biases);
}

extern "C" int ofx_es_opt_set(ofx_handle *h, const double *m_weights, const double *m_biases, const double *v_weights,
                              const double *v_biases) {
  ofx_es *p;
  int rc = need_opt(h, "ofx_es_opt_set", &p);
  if (rc) return rc;
  if (!m_weights || !m_biases || !v_weights || !v_biases) { ofx_set_error("ofx_es_opt_set: null argument"); return OFX_ERR_INVALID; }
  OFX_HIP(hipSetDevice(h->cfg.device));
  if ((rc = genome_from_host(h, p->m, p->layers, p->first, p->n_w, p->G, m_weights, m_biases))) return rc;
  return genome_from_host(h, p->v, p->layers, p->first, p->n_w, p->G, v_weights, v_biases);
}

template <bool ADAM, bool STATS>
static void launch_step(ofx_handle *h, ofx_es *p, int n, const es_law &law, uint64_t seed, uint32_t generation) {
  hipLaunchKernelGGL((k_es_step<ADAM, STATS>), dim3((p->G + 255u) / 256u), dim3(256), 0, h->stream, p->theta, p->m, p->v,
                     p->d, p->d_pair, n, p->G, p->first, (uint32_t)p->layers[0], (uint32_t)p->layers[1], law,
                     ofx_key(seed), generation, p->part);
}

extern "C" int ofx_es_step(ofx_handle *h, const double *d_host, int64_t n_pairs, int32_t rule, double gscale,
                           double decay, double alpha, double c1, double k1, double c2, double k2, double eps,
                           uint64_t seed, uint32_t generation, double *stats) {
  ofx_es *p;
  int rc = need_opt(h, "ofx_es_step", &p);
  if (rc || (rc = check_pairs("ofx_es_step", d_host, n_pairs))) return rc;
  if (rule != OFX_ES_RULE_MOMENTUM && rule != OFX_ES_RULE_ADAM) {
    ofx_set_error("ofx_es_step: rule must be OFX_ES_RULE_MOMENTUM (1) or OFX_ES_RULE_ADAM (2) (got %d)", rule);
    return OFX_ERR_INVALID;
  }
  const es_law law = {gscale, decay, alpha, c1, k1, c2, k2, eps};
  const double scalars[8] = {gscale, decay, alpha, c1, k1, c2, k2, eps};
  static const char *const names[8] = {"gscale", "decay", "alpha", "c1", "k1", "c2", "k2", "eps"};
  for (int i = 0; i < 8; i++)
    if (!(scalars[i] - scalars[i] == 0.0)) { ofx_set_error("ofx_es_step: %s is not finite", names[i]); return OFX_ERR_INVALID; }
  if (decay < 0.0) { ofx_set_error("ofx_es_step: decay must be >= 0 (got %g)", decay); return OFX_ERR_INVALID; }
  if (rule == OFX_ES_RULE_ADAM && !(eps > 0.0)) { ofx_set_error("ofx_es_step: eps must be > 0 under Adam (got %g)", eps); return OFX_ERR_INVALID; }
  std::vector<double> d;
  std::vector<uint32_t> pair;
  if ((rc = nonzero_pairs("ofx_es_step", d_host, n_pairs, d, pair)) || (rc = upload_pairs(h, p, d, pair))) return rc;
  const int n = (int)d.size();
  const bool adam = rule == OFX_ES_RULE_ADAM;
  if (stats) {
    if (adam) launch_step<true, true>(h, p, n, law, seed, generation);
    else launch_step<false, true>(h, p, n, law, seed, generation);
    OFX_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_es_stats<3>, dim3(1), dim3(256), 0, h->stream, p->part, (int)((p->G + 255u) / 256u), stats);
  } else {
    if (adam) launch_step<true, false>(h, p, n, law, seed, generation);
    else launch_step<false, false>(h, p, n, law, seed, generation);
  }
  OFX_HIP(hipGetLastError());
  return OFX_OK;
}

// ---- per-element adaptive sigma (include/ofx.h: ofx_es_sigma_*) ----
static int need_sigma(ofx_handle *h, const char *who, ofx_es **out) {
  const int rc = need_es(h, who, out);
  if (rc) return rc;
  if (!(*out)->sigma) { ofx_set_error("%s: the centre has no sigma vector (ofx_es_sigma_create)", who); return OFX_ERR_STATE; }
  return OFX_OK;
}

extern "C" int ofx_es_sigma_create(ofx_handle *h, double sigma0) {
  ofx_es *p;
  const int rc = need_es(h, "ofx_es_sigma_create", &p);
  if (rc) return rc;
  if (p->sigma) { ofx_set_error("ofx_es_sigma_create: the centre already has a sigma vector (ofx_es_sigma_destroy)"); return OFX_ERR_STATE; }
  if (!(sigma0 - sigma0 == 0.0) || !(sigma0 > 0.0)) {
    ofx_set_error("ofx_es_sigma_create: sigma0 must be finite and > 0 (got %g)", sigma0);
    return OFX_ERR_INVALID;
  }
  OFX_HIP(hipSetDevice(h->cfg.device));
  const size_t bytes = (size_t)p->G * sizeof(double), nb = (p->G + 255u) / 256u;
  hipError_t e = hipMalloc((void **)&p->sigma, bytes);
  if (e == hipSuccess) e = hipMalloc((void **)&p->sigma_part, 5 * nb * sizeof(double));
  if (e != hipSuccess) {
    (void)hipGetLastError();
    ofx_set_error("ofx_es_sigma_create: allocating %zu bytes for the sigma of %u elements failed: %s", bytes, p->G,
                  hipGetErrorString(e));
    es_sigma_free(p);
    return OFX_ERR_HIP;
  }
  hipLaunchKernelGGL(k_es_fill, dim3((unsigned)nb), dim3(256), 0, h->stream, p->sigma, p->G, sigma0);
  e = hipGetLastError();
  if (e != hipSuccess) {
    ofx_set_error("ofx_es_sigma_create: filling the vector failed: %s", hipGetErrorString(e));
    (void)hipStreamSynchronize(h->stream);
    es_sigma_free(p);
    return OFX_ERR_HIP;
  }
  return OFX_OK;
}

extern "C" int ofx_es_sigma_destroy(ofx_handle *h) {
  ofx_es *p;
  const int rc = need_sigma(h, "ofx_es_sigma_destroy", &p);
  if (rc) return rc;
  OFX_HIP(hipSetDevice(h->cfg.device));
  OFX_HIP(hipStreamSynchronize(h->stream));
  es_sigma_free(p);
  return OFX_OK;
}

extern "C" int ofx_es_sigma_get(ofx_handle *h, double *weights_host, double *biases_host) {
  ofx_es *p;
  int rc = need_sigma(h, "ofx_es_sigma_get", &p);
  if (rc) return rc;
  if (!weights_host || !biases_host) { ofx_set_error("ofx_es_sigma_get: null argument"); return OFX_ERR_INVALID; }
  OFX_HIP(hipSetDevice(h->cfg.device));
  return genome_to_host(h, p->sigma, p->layers, p->first, p->n_w, p->G, weights_host, biases_host);
}

extern "C" int ofx_es_sigma_set(ofx_handle *h, const double *weights_host, const double *biases_host) {
  ofx_es *p;
  int rc = need_sigma(h, "ofx_es_sigma_set", &p);
  if (rc) return rc;
  if (!weights_host || !biases_host) { ofx_set_error("ofx_es_sigma_set: null argument"); return OFX_ERR_INVALID; }
  for (uint32_t i = 0; i < p->G; i++) {
    const double x = i < p->n_w ? weights_host[i] : biases_host[i - p->n_w];
    if (!(x - x == 0.0) || !(x > 0.0)) {
      ofx_set_error("ofx_es_sigma_set: sigma[%u] must be finite and > 0 (got %g)", i, x);
      return OFX_ERR_INVALID;
    }
  }
  OFX_HIP(hipSetDevice(h->cfg.device));
  return genome_from_host(h, p->sigma, p->layers, p->first, p->n_w, p->G, weights_host, biases_host);
}

extern "C" int ofx_es_sigma_member(ofx_handle *h, int64_t member, int64_t P, uint64_t seed, uint32_t generation,
                                   double *weights_host, double *biases_host) {
  ofx_es *p;
  int rc = need_sigma(h, "ofx_es_sigma_member", &p);
  if (rc || (rc = check_members("ofx_es_sigma_member", P, 1.0))) return rc;
  if (!weights_host || !biases_host) { ofx_set_error("ofx_es_sigma_member: null argument"); return OFX_ERR_INVALID; }
  if (member < 0 || member > P) {
    ofx_set_error("ofx_es_sigma_member: member %lld outside [0, %lld] (P is the centre)", (long long)member, (long long)P);
    return OFX_ERR_INVALID;
  }
  OFX_HIP(hipSetDevice(h->cfg.device));
  if ((rc = member_buffer(p, "ofx_es_sigma_member"))) return rc;
  hipLaunchKernelGGL(k_es_sigma_member, dim3((p->G + 255u) / 256u), dim3(256), 0, h->stream, p->theta, p->sigma, p->member,
                     p->G, p->first, (uint32_t)p->layers[0], (uint32_t)p->layers[1], (int)member, (int)P, ofx_key(seed),
                     generation);
  OFX_HIP(hipGetLastError());
  return genome_to_host(h, p->member, p->layers, p->first, p->n_w, p->G, weights_host, biases_host);
}

extern "C" int ofx_es_sigma_act(ofx_handle *h, const int32_t *member_of, int64_t P, uint64_t seed, uint32_t generation,
                                ofx_action *actions, double *y) {
  ofx_es *p;
  int rc = need_sigma(h, "ofx_es_sigma_act", &p);
  if (rc || (rc = check_members("ofx_es_sigma_act", P, 1.0))) return rc;
  if (!member_of || !actions) { ofx_set_error("ofx_es_sigma_act: null argument"); return OFX_ERR_INVALID; }
  if (!h->spawned) { ofx_set_error("You must execute analyse_battleground first."); return OFX_ERR_STATE; }
  const ofx_config &c = h->cfg;
  OFX_HIP(hipSetDevice(c.device));
  if ((rc = ofx_launch_raster(h, OFX_MAP_BITS_LSB, nullptr, nullptr))) return rc;
  const pop_net net = net_of(p);
  const int words = (int)(((size_t)c.width * c.height) >> 5);
  hipLaunchKernelGGL(k_es_sigma_act, dim3((unsigned)(c.n_arenas * c.n_ships)), dim3(256), 0, h->stream, c.n_ships,
                     c.width, c.height, h->st, (const unsigned *)h->maps[OFX_MAP_BITS_LSB][0],
                     (const unsigned *)h->maps[OFX_MAP_BITS_LSB][1], words, p->theta, p->sigma, (int)P, p->first, p->n_w,
                     net, ofx_key(seed), generation, member_of, actions, y);
  OFX_HIP(hipGetLastError());
  return OFX_OK;
}

// the listed pairs' sigma weights into the centre's device copy, after upload_pairs (which has synchronised)
static int upload_sigma_weights(ofx_es *p, const std::vector<double> &s) {
  if (s.size() > p->s_cap) {
    if (p->s) (void)hipFree(p->s);
    p->s = nullptr;
    p->s_cap = 0;
    OFX_HIP(hipMalloc((void **)&p->s, s.size() * sizeof(double)));
    p->s_cap = s.size();
  }
  if (!s.empty()) OFX_HIP(hipMemcpy(p->s, s.data(), s.size() * sizeof(double), hipMemcpyHostToDevice));
  return OFX_OK;
}

template <int RULE, bool STATS>
static void launch_sigma_step(ofx_handle *h, ofx_es *p, int n, const es_law &law, const es_sigma_law &z, uint64_t seed,
                              uint32_t generation) {
  hipLaunchKernelGGL((k_es_sigma_step<RULE, STATS>), dim3((p->G + 255u) / 256u), dim3(256), 0, h->stream, p->theta,
                     p->sigma, p->m, p->v, p->d, p->s, p->d_pair, n, p->G, p->first, (uint32_t)p->layers[0],
                     (uint32_t)p->layers[1], law, z, ofx_key(seed), generation, p->sigma_part);
}

extern "C" int ofx_es_sigma_step(ofx_handle *h, const double *d_host, const double *s_host, int64_t n_pairs, int32_t rule,
                                 double gscale, double decay, double alpha, double c1, double k1, double c2, double k2,
                                 double eps, double srate, double smin, double smax, uint64_t seed, uint32_t generation,
                                 double *stats) {
  ofx_es *p;
  int rc = need_sigma(h, "ofx_es_sigma_step", &p);
  if (rc || (rc = check_pairs("ofx_es_sigma_step", d_host, n_pairs))) return rc;
  if (!s_host) { ofx_set_error("ofx_es_sigma_step: null argument"); return OFX_ERR_INVALID; }
  if (rule != OFX_ES_RULE_PLAIN && rule != OFX_ES_RULE_MOMENTUM && rule != OFX_ES_RULE_ADAM) {
    ofx_set_error("ofx_es_sigma_step: rule must be OFX_ES_RULE_PLAIN (0), _MOMENTUM (1) or _ADAM (2) (got %d)", rule);
    return OFX_ERR_INVALID;
  }
  const es_law law = {gscale, decay, alpha, c1, k1, c2, k2, eps};
  const es_sigma_law z = {srate, smin, smax};
  const double scalars[11] = {gscale, decay, alpha, c1, k1, c2, k2, eps, srate, smin, smax};
  static const char *const names[11] = {"gscale", "decay", "alpha", "c1", "k1", "c2", "k2", "eps", "srate", "smin", "smax"};
  for (int i = 0; i < 11; i++)
    if (!(scalars[i] - scalars[i] == 0.0)) { ofx_set_error("ofx_es_sigma_step: %s is not finite", names[i]); return OFX_ERR_INVALID; }
  if (decay < 0.0) { ofx_set_error("ofx_es_sigma_step: decay must be >= 0 (got %g)", decay); return OFX_ERR_INVALID; }
  if (rule == OFX_ES_RULE_ADAM && !(eps > 0.0)) { ofx_set_error("ofx_es_sigma_step: eps must be > 0 under Adam (got %g)", eps); return OFX_ERR_INVALID; }
  if (!(smin > 0.0)) { ofx_set_error("ofx_es_sigma_step: smin must be > 0 (got %g)", smin); return OFX_ERR_INVALID; }
  if (smax < smin) { ofx_set_error("ofx_es_sigma_step: smax must be >= smin (got smax %g, smin %g)", smax, smin); return OFX_ERR_INVALID; }
  if (rule != OFX_ES_RULE_PLAIN && !p->m) {
    ofx_set_error("ofx_es_sigma_step: the centre has no optimiser state (ofx_es_opt_create), which rule %d needs", rule);
    return OFX_ERR_STATE;
  }
  // the pairs with either weight, ascending: a pair with both zero adds +-0 to two sums that are never -0.0
  std::vector<double> d, s;
  std::vector<uint32_t> pair;
  for (int64_t i = 0; i < n_pairs; i++) {
    if (!(d_host[i] - d_host[i] == 0.0)) { ofx_set_error("ofx_es_sigma_step: d[%lld] is not finite", (long long)i); return OFX_ERR_INVALID; }
    if (!(s_host[i] - s_host[i] == 0.0)) { ofx_set_error("ofx_es_sigma_step: s[%lld] is not finite", (long long)i); return OFX_ERR_INVALID; }
    if (d_host[i] != 0.0 || s_host[i] != 0.0) { d.push_back(d_host[i]); s.push_back(s_host[i]); pair.push_back((uint32_t)i); }
  }
  if ((rc = upload_pairs(h, p, d, pair)) || (rc = upload_sigma_weights(p, s))) return rc;
  const int n = (int)d.size();
  if (stats) {
    if (rule == OFX_ES_RULE_ADAM) launch_sigma_step<OFX_ES_RULE_ADAM, true>(h, p, n, law, z, seed, generation);
    else if (rule == OFX_ES_RULE_MOMENTUM) launch_sigma_step<OFX_ES_RULE_MOMENTUM, true>(h, p, n, law, z, seed, generation);
    else launch_sigma_step<OFX_ES_RULE_PLAIN, true>(h, p, n, law, z, seed, generation);
    OFX_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_es_stats<5>, dim3(1), dim3(256), 0, h->stream, p->sigma_part, (int)((p->G + 255u) / 256u), stats);
  } else {
    if (rule == OFX_ES_RULE_ADAM) launch_sigma_step<OFX_ES_RULE_ADAM, false>(h, p, n, law, z, seed, generation);
    else if (rule == OFX_ES_RULE_MOMENTUM) launch_sigma_step<OFX_ES_RULE_MOMENTUM, false>(h, p, n, law, z, seed, generation);
    else launch_sigma_step<OFX_ES_RULE_PLAIN, false>(h, p, n, law, z, seed, generation);
  }
  OFX_HIP(hipGetLastError());
  return OFX_OK;
}
