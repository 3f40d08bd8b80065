// ofx_genome.h - what the stored population (ofx_evolve.hip) and the evolution strategy (ofx_es.hip) share: the genome
// of the from-scratch sigmoid MLP and the forward over one ship's observation, each __device__ body once.
//
// Storage of one genome (G doubles, 64-bit offsets; element index e as in include/ofx.h):
//   [0, nin*n1)   the first layer INPUT-major, W1T[k][o] = W_1[o][k]: the n1 weights of one input are contiguous (72 B at
//                 n1 = 9) and the weights of consecutive map cells - a disc's row of set cells - are one contiguous run
//   [nin*n1, G)   the remaining layers row-major and the biases, exactly as in the element order
// so storage position s and element e differ in the first layer only (s = k*n1 + o  <->  e = o*nin + k).
#pragma once
#include "ofx_internal.h"

#define POP_MAX_LAYERS 8
#define POP_MAX_WIDTH 64
#define POP_LIST 2048               /* set cells one wave lists before it gathers: a batch of 64 words holds <= 2048 */
#define POP_MAX_ACTS ((POP_MAX_LAYERS - 2) * POP_MAX_WIDTH + 4) /* activations of one ship behind the input: <= 6 x 64 + 4 */
#define POP_AHEAD 16                /* batches of 64 map words a wave loads before it looks at the first              */

// the shape of one genome, filled by check_topology alone
struct genome_shape {
  int n_layers;
  int32_t layers[POP_MAX_LAYERS];
  uint32_t G;        // elements of one genome
  uint32_t first;    // nin * n1: elements (and storage positions) of the first layer
  uint32_t n_w;      // weights of one genome; the biases follow
  uint32_t nin() const { return (uint32_t)layers[0]; }
  uint32_t n1() const { return (uint32_t)layers[1]; }
  unsigned blocks() const { return (G + 255u) / 256u; }    // 256-thread workgroups over the storage positions
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

__device__ inline double pop_sigmoid(double v) { return 1.0 / (1.0 + exp(-v)); }

struct pop_net {
  int n_layers;
  int32_t layers[POP_MAX_LAYERS];
};

// The walk over one arena's set cells, stated once for the forward (k_pop_act, k_pop_grad, k_es_act) and the first
// layer's update (k_pop_apply).  The two maps are one run of 2*words words (toVector: ship map, then laser map); wave wv
// of the four owns a quarter of it, lists the set cells of its quarter in ascending order in `mine` (POP_LIST entries of
// its own, a wave scan, no block barrier) and hands them to flush(n) - whenever the next batch would not fit, and once
// at the end (n may be 0).  The wavefront fences order the lanes' list writes before flush's reads and those before the
// next writes.
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
// HBM (k_pop_act, k_pop_grad, the centre in k_es_act); es_member (ofx_es.hip) adds the member's noise to it.
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

// ---- host side, defined in ofx_evolve.hip ----
template <class T>
inline void genome_drop(T *&p) {                           // free a device buffer that may be null
  if (p) (void)hipFree(p);
  p = nullptr;
}

// the topologies a genome can have on this handle (`who`: ofx_population_create or ofx_es_create); fills *shape
int check_topology(ofx_handle *h, const char *who, const int32_t *layers, int32_t n_layers, genome_shape *shape);
pop_net net_of(const genome_shape &g);

// what a forward over the arenas starts with: the spawned check, the 1-bit rasteriser on the handle's stream, where its
// maps lie and the grid, one workgroup per (arena, ship)
struct pop_maps {
  const unsigned *ship_bits, *laser_bits;
  int words;
  dim3 grid;
};
int pop_forward_begin(ofx_handle *h, pop_maps *maps);

// k_pop_breed on the genomes at `data`; k_pop_fitness over `slots` sums and counts, zeroed first if `reset`
int launch_breed(ofx_handle *h, double *data, const genome_shape &g, const int32_t *jobs, int n_jobs, double evo,
                 double mut, uint64_t seed, uint32_t generation);
int launch_fitness(ofx_handle *h, size_t slots, const int32_t *genome_of, int64_t *sum, int32_t *count, int32_t reset);

// one genome in storage order at `src` -> the element order on the host (weights, then biases), and back; both sync
int genome_to_host(ofx_handle *h, const double *src, const genome_shape &g, double *weights_host, double *biases_host);
int genome_from_host(ofx_handle *h, double *dst, const genome_shape &g, const double *weights_host,
                     const double *biases_host);
