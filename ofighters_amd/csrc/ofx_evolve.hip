// ofx_evolve.hip - device-resident neuroevolution of the from-scratch sigmoid MLP: a genome per ship
// (agents/neural_network.py:436-478 generate / evolution / mutate / reproduce / dafts around the network of :396-420,
//  one network per ship as in lib/battleground.py:52-76, the four-sigmoid decode of agents/brAIn.py:129-134).
//
// A population is P genomes of G float64 elements each, resident in HBM (include/ofx.h: element index e = the position
// in weights_layers + biases_layers; every random draw is keyed by (slot, e, generation, stream)).  Genome `slot` lies
// at data + slot * G in the storage layout of ofx_genome.h, which also holds the walk, the forward and the decode.
// This file also defines the host functions that header declares for the evolution strategy (ofx_es.hip).
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
#include "ofx_genome.h"
#include "ofx_arena.h"

#include <new>
#include <vector>

struct ofx_population {
  genome_shape shape;
  int64_t P;
  double *data;      // [P][G]
  int32_t *jobs;     // [P][2] (destination, parent or -1) of the slots a breed rewrites
};

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

pop_net net_of(const genome_shape &g) {
  pop_net net;
  net.n_layers = g.n_layers;
  for (int i = 0; i < POP_MAX_LAYERS; i++) net.layers[i] = i < g.n_layers ? g.layers[i] : 0;
  return net;
}

void ofx_population_free(ofx_handle *h) {
  ofx_population *p = pop_of(h);
  if (!p) return;
  genome_drop(p->data);
  genome_drop(p->jobs);
  delete p;
  pop_of(h) = nullptr;
}

static int need_population(ofx_handle *h, const char *who, ofx_population **out) {
  if (!h) { ofx_set_error("%s: null handle", who); return OFX_ERR_INVALID; }
  if (!pop_of(h)) { ofx_set_error("%s: the handle holds no population (ofx_population_create)", who); return OFX_ERR_STATE; }
  *out = pop_of(h);
  return OFX_OK;
}

// the topologies a genome can have on this handle, stated once for ofx_population_create and ofx_es_create (`who`),
// and the one place that fills a genome_shape
int check_topology(ofx_handle *h, const char *who, const int32_t *layers, int32_t n_layers, genome_shape *shape) {
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
  unsigned long long n_w = 0, n_b = 0;                     // the weights and biases of one genome
  for (int i = 0; i + 1 < n_layers; i++) { n_w += (unsigned long long)layers[i] * layers[i + 1]; n_b += layers[i + 1]; }
  if (n_w + n_b >= (1ull << 32)) { ofx_set_error("%s: a genome of %llu elements", who, n_w + n_b); return OFX_ERR_INVALID; }
  *shape = genome_shape();
  shape->n_layers = n_layers;
  for (int i = 0; i < n_layers; i++) shape->layers[i] = layers[i];
  shape->G = (uint32_t)(n_w + n_b);
  shape->first = (uint32_t)((unsigned long long)layers[0] * layers[1]);
  shape->n_w = (uint32_t)n_w;
  return OFX_OK;
}

extern "C" int ofx_population_create(ofx_handle *h, const int32_t *layers, int32_t n_layers, int64_t P) {
  if (!h || !layers) { ofx_set_error("ofx_population_create: null argument"); return OFX_ERR_INVALID; }
  if (pop_of(h)) { ofx_set_error("ofx_population_create: the handle already holds a population (ofx_population_destroy)"); return OFX_ERR_STATE; }
  genome_shape shape;
  const int rc = check_topology(h, "ofx_population_create", layers, n_layers, &shape);
  if (rc) return rc;
  if (P < 1 || P > 0x7fffffffll) { ofx_set_error("ofx_population_create: P must be in [1, 2^31) (got %lld)", (long long)P); return OFX_ERR_INVALID; }
  OFX_HIP(hipSetDevice(h->cfg.device));
  ofx_population *p = new (std::nothrow) ofx_population();   // every pointer null
  if (!p) { ofx_set_error("ofx_population_create: out of host memory"); return OFX_ERR_INVALID; }
  p->shape = shape;
  p->P = P;
  pop_of(h) = p;
  const size_t bytes = (size_t)P * shape.G * sizeof(double);
  hipError_t e = hipMalloc((void **)&p->data, bytes);
  if (e == hipSuccess) e = hipMalloc((void **)&p->jobs, (size_t)P * 2 * sizeof(int32_t));
  if (e != hipSuccess) {
    (void)hipGetLastError();
    ofx_set_error("ofx_population_create: allocating %zu bytes for %lld genomes of %u elements failed: %s", bytes,
                  (long long)P, shape.G, hipGetErrorString(e));
    ofx_population_free(h);
    return OFX_ERR_HIP;
  }
  return OFX_OK;
}

extern "C" int ofx_population_destroy(ofx_handle *h) {
  if (!h) { ofx_set_error("ofx_population_destroy: null handle"); return OFX_ERR_INVALID; }
  OFX_HIP(hipSetDevice(h->cfg.device));
  OFX_HIP(hipStreamSynchronize(h->stream));
  ofx_population_free(h);
  return OFX_OK;
}

int launch_breed(ofx_handle *h, double *data, const genome_shape &g, const int32_t *jobs, int n_jobs, double evo,
                 double mut, uint64_t seed, uint32_t generation) {
  if (n_jobs < 1) return OFX_OK;
  const dim3 grid(g.blocks(), (unsigned)(n_jobs < 65535 ? n_jobs : 65535));
  hipLaunchKernelGGL(k_pop_breed, grid, dim3(256), 0, h->stream, data, jobs, n_jobs, g.G, g.first, g.nin(), g.n1(), evo,
                     mut, ofx_key(seed), generation);
  OFX_HIP(hipGetLastError());
  return OFX_OK;
}

extern "C" int ofx_population_init(ofx_handle *h, uint64_t seed, uint32_t generation) {
  ofx_population *p;
  int rc = need_population(h, "ofx_population_init", &p);
  if (rc) return rc;
  OFX_HIP(hipSetDevice(h->cfg.device));
  return launch_breed(h, p->data, p->shape, nullptr, (int)p->P, 0.0, 0.0, seed, generation);
}

// host <-> storage order of one genome: the first layer is transposed, the rest is the element order
static int check_slot(ofx_population *p, const char *who, int64_t slot, const void *w, const void *b) {
  if (!w || !b) { ofx_set_error("%s: null argument", who); return OFX_ERR_INVALID; }
  if (slot < 0 || slot >= p->P) { ofx_set_error("%s: slot %lld outside [0, %lld)", who, (long long)slot, (long long)p->P); return OFX_ERR_INVALID; }
  return OFX_OK;
}

// ofx_genome.h: stated once for the population's slots and the ES centre, members, moments and sigma
int genome_to_host(ofx_handle *h, const double *src, const genome_shape &g, double *weights_host, double *biases_host) {
  const uint32_t first = g.first, n_w = g.n_w, G = g.G;
  std::vector<double> tmp(first);
  OFX_HIP(hipStreamSynchronize(h->stream));
  OFX_HIP(hipMemcpy(tmp.data(), src, (size_t)first * sizeof(double), hipMemcpyDeviceToHost));
  OFX_HIP(hipMemcpy(weights_host + first, src + first, (size_t)(n_w - first) * sizeof(double), hipMemcpyDeviceToHost));
  OFX_HIP(hipMemcpy(biases_host, src + n_w, (size_t)(G - n_w) * sizeof(double), hipMemcpyDeviceToHost));
  const size_t nin = g.nin(), n1 = g.n1();
  for (size_t k = 0; k < nin; k++)
    for (size_t o = 0; o < n1; o++) weights_host[o * nin + k] = tmp[k * n1 + o];
  return OFX_OK;
}

int genome_from_host(ofx_handle *h, double *dst, const genome_shape &g, const double *weights_host,
                     const double *biases_host) {
  const uint32_t first = g.first, n_w = g.n_w, G = g.G;
  std::vector<double> tmp(first);
  const size_t nin = g.nin(), n1 = g.n1();
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
  return genome_to_host(h, p->data + (size_t)slot * p->shape.G, p->shape, weights_host, biases_host);
}

extern "C" int ofx_population_set(ofx_handle *h, int64_t slot, const double *weights_host, const double *biases_host) {
  ofx_population *p;
  int rc = need_population(h, "ofx_population_set", &p);
  if (rc || (rc = check_slot(p, "ofx_population_set", slot, weights_host, biases_host))) return rc;
  OFX_HIP(hipSetDevice(h->cfg.device));
  return genome_from_host(h, p->data + (size_t)slot * p->shape.G, p->shape, weights_host, biases_host);
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
  return launch_breed(h, p->data, p->shape, p->jobs, (int)(jobs.size() / 2), evolution_rate, mutation_rate, seed,
                      generation);
}

int pop_forward_begin(ofx_handle *h, pop_maps *maps) {
  if (!h->spawned) { ofx_set_error("You must execute analyse_battleground first."); return OFX_ERR_STATE; }
  const ofx_config &c = h->cfg;
  OFX_HIP(hipSetDevice(c.device));
  const int rc = ofx_launch_raster(h, OFX_MAP_BITS_LSB, nullptr, nullptr);
  if (rc) return rc;
  maps->ship_bits = (const unsigned *)h->maps[OFX_MAP_BITS_LSB][0];
  maps->laser_bits = (const unsigned *)h->maps[OFX_MAP_BITS_LSB][1];
  maps->words = (int)(((size_t)c.width * c.height) >> 5);
  maps->grid = dim3((unsigned)(c.n_arenas * c.n_ships));
  return OFX_OK;
}

extern "C" int ofx_population_act(ofx_handle *h, const int32_t *genome_of, ofx_action *actions, double *y) {
  ofx_population *p;
  int rc = need_population(h, "ofx_population_act", &p);
  if (rc) return rc;
  if (!genome_of || !actions) { ofx_set_error("ofx_population_act: null argument"); return OFX_ERR_INVALID; }
  pop_maps mp;
  if ((rc = pop_forward_begin(h, &mp))) return rc;
  const ofx_config &c = h->cfg;
  const genome_shape &g = p->shape;
  hipLaunchKernelGGL(k_pop_act, mp.grid, dim3(256), 0, h->stream, c.n_ships, c.width, c.height, h->st, mp.ship_bits,
                     mp.laser_bits, mp.words, p->data, (long long)p->P, g.G, g.first, g.n_w, net_of(g), genome_of, actions,
                     y);
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
  pop_maps mp;                                             // the rasteriser touches no scratch: it may go first
  if ((rc = pop_forward_begin(h, &mp))) return rc;
  const ofx_config &c = h->cfg;
  const genome_shape &g = p->shape;
  const size_t NM = (size_t)c.n_arenas * c.n_ships;
  size_t S = 0;
  for (int i = 1; i < g.n_layers; i++) S += (size_t)g.layers[i];
  LearnWs ws;
  Arena measure;
  learn_layout(measure, NM, S, (size_t)p->P, ws);
  if ((rc = ofx_ensure_scratch(h, measure.used))) return rc;
  Arena A(h->scratch, measure.used);
  learn_layout(A, NM, S, (size_t)p->P, ws);
  if (!A.ok()) { ofx_set_error("ofx_population_learn: the workspace does not fit its block of %zu bytes", measure.used); return OFX_ERR_STATE; }
  OFX_HIP(hipMemsetAsync(ws.sample_of, 0xff, NM * sizeof(int32_t), h->stream));   // -1: no sample
  OFX_HIP(hipMemsetAsync(ws.count, 0, (size_t)p->P * sizeof(int32_t), h->stream));
  const pop_net net = net_of(g);
  hipLaunchKernelGGL(k_pop_grad, mp.grid, dim3(256), 0, h->stream, c.n_ships, c.width, c.height, h->st, mp.ship_bits,
                     mp.laser_bits, mp.words, p->data, (long long)p->P, g.G, g.first, g.n_w, net, (int)S, genome_of,
                     solution, learn_mask, actions, y, err, ws);
  OFX_HIP(hipGetLastError());
  if (rate == 0.0) return OFX_OK;                          // outputs and err only: no genome changes a bit
  hipLaunchKernelGGL(k_pop_apply, dim3((unsigned)p->P), dim3(256), 0, h->stream, (int)NM, c.n_ships, mp.ship_bits,
                     mp.laser_bits, mp.words, p->data, g.G, g.first, g.n_w, net, (int)S, ws, rate);
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
  return launch_fitness(h, (size_t)p->P, genome_of, sum, count, reset);
}

int launch_fitness(ofx_handle *h, size_t slots, const int32_t *genome_of, int64_t *sum, int32_t *count, int32_t reset) {
  OFX_HIP(hipSetDevice(h->cfg.device));
  if (reset) {
    OFX_HIP(hipMemsetAsync(sum, 0, slots * sizeof(int64_t), h->stream));
    OFX_HIP(hipMemsetAsync(count, 0, slots * sizeof(int32_t), h->stream));
  }
  const int NM = h->cfg.n_arenas * h->cfg.n_ships;
  hipLaunchKernelGGL(k_pop_fitness, dim3((NM + 255) / 256), dim3(256), 0, h->stream, NM, (long long)slots,
                     h->st.last_score, genome_of, (unsigned long long *)sum, count);
  OFX_HIP(hipGetLastError());
  return OFX_OK;
}

