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
// k_pop_fitness  integer atomics only.
#include "ofx_internal.h"

#include <new>
#include <vector>

#define POP_MAX_LAYERS 8
#define POP_MAX_WIDTH 64
#define POP_LIST 2048               /* set cells one wave lists before it gathers: a batch of 64 words holds <= 2048 */
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
  const double *gen = data + (size_t)g * G;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int n1 = net.layers[1];
  const int groups = 64 / n1;                   // cells one wave gathers per pass
  const int o = lane % n1, grp = lane / n1;     // this lane's neuron and its place among the pass's cells
  const bool gathers = grp < groups;
  const unsigned *sb = ship_bits + (size_t)a * words, *lb = laser_bits + (size_t)a * words;
  // the two maps are one run of 2*words words (toVector: ship map, then laser map); a wave owns a quarter of it
  const int total = 2 * words, per = (total + 3) / 4;
  const int w_end = min(total, (wv + 1) * per);
  uint32_t *mine = list[wv];
  int count = 0;                                // cells listed, uniform over the wave
  double acc = 0.0;
  // gather what is listed: lane (grp, o) takes cells grp, grp + groups, ... in list order
  auto gather = [&]() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    if (gathers) {
      int i = grp;
      for (; i + 7 * groups < count; i += 8 * groups) {
        double t[8];
#pragma unroll
        for (int q = 0; q < 8; q++) t[q] = gen[(size_t)(8u + mine[i + q * groups]) * n1 + o];
#pragma unroll
        for (int q = 0; q < 8; q++) acc += t[q];
      }
      for (; i < count; i += groups) acc += gen[(size_t)(8u + mine[i]) * n1 + o];
    }
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
      if (count + n_new > POP_LIST) gather();
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
  gather();
  part[wv][lane] = gathers ? acc : 0.0;
  __syncthreads();
  if (tid < n1) {
    // first layer of neuron tid: head in toVector order, the map cells in (wave, group) order, bias
    double v[8];
    ofx_obs_head(st, s, W, H, v);
    double z = gen[tid] * v[0];
#pragma unroll
    for (int k = 1; k < 8; k++) z += gen[(size_t)k * n1 + tid] * v[k];
    for (int q = 0; q < 4; q++)
      for (int j = 0; j < groups; j++) z += part[q][j * n1 + tid];
    act[0][tid] = pop_sigmoid(z + gen[n_w + tid]);
  }
  __syncthreads();
  uint32_t woff = first, boff = n_w + (uint32_t)n1;
  int cur = 0;
  for (int l = 1; l + 1 < net.n_layers; l++) {
    const int nin = net.layers[l], nout = net.layers[l + 1];
    if (tid < nout) {
      const double *w = gen + woff + (size_t)tid * nin;
      double z = 0.0;
      for (int k = 0; k < nin; k++) z += w[k] * act[cur][k];
      act[cur ^ 1][tid] = pop_sigmoid(z + gen[boff + tid]);
    }
    __syncthreads();
    woff += (uint32_t)(nin * nout);
    boff += (uint32_t)nout;
    cur ^= 1;
  }
  if (tid == 0) {
    const double y0 = act[cur][0], y1 = act[cur][1], y2 = act[cur][2], y3 = act[cur][3];
    ofx_action out;
    out.px = (int32_t)(y2 * (double)W);
    out.py = (int32_t)(y3 * (double)H);
    out.shoot = y0 > 0.5 ? 1 : 0;
    out.thrust = y1 > 0.5 ? 1 : 0;
    out.valid = 1;
    out._pad = 0;
    actions[s] = out;
  }
  if (y && tid < 4) y[(size_t)s * 4 + tid] = act[cur][tid];
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

extern "C" int ofx_population_create(ofx_handle *h, const int32_t *layers, int32_t n_layers, int64_t P) {
  if (!h || !layers) { ofx_set_error("ofx_population_create: null argument"); return OFX_ERR_INVALID; }
  if (pop_of(h)) { ofx_set_error("ofx_population_create: the handle already holds a population (ofx_population_destroy)"); return OFX_ERR_STATE; }
  if (n_layers < 2 || n_layers > POP_MAX_LAYERS) {
    ofx_set_error("ofx_population_create: need 2..%d layers (got %d)", POP_MAX_LAYERS, n_layers);
    return OFX_ERR_INVALID;
  }
  const ofx_config &c = h->cfg;
  const long long nin = 8 + 2ll * c.width * c.height;
  if (layers[0] != nin) {
    ofx_set_error("ofx_population_create: layers[0] must be 8 + 2*W*H = %lld (got %d)", nin, layers[0]);
    return OFX_ERR_INVALID;
  }
  if (layers[n_layers - 1] != 4) {
    ofx_set_error("ofx_population_create: the last layer must have 4 outputs, the reference's Action.size (got %d)",
                  layers[n_layers - 1]);
    return OFX_ERR_INVALID;
  }
  for (int i = 1; i < n_layers; i++)
    if (layers[i] < 1 || layers[i] > POP_MAX_WIDTH) {
      ofx_set_error("ofx_population_create: layer %d must be 1..%d wide (got %d)", i, POP_MAX_WIDTH, layers[i]);
      return OFX_ERR_INVALID;
    }
  if (P < 1 || P > 0x7fffffffll) { ofx_set_error("ofx_population_create: P must be in [1, 2^31) (got %lld)", (long long)P); return OFX_ERR_INVALID; }
  unsigned long long n_w = 0, n_b = 0;
  for (int i = 0; i + 1 < n_layers; i++) { n_w += (unsigned long long)layers[i] * layers[i + 1]; n_b += layers[i + 1]; }
  if (n_w + n_b >= (1ull << 32)) { ofx_set_error("ofx_population_create: a genome of %llu elements", n_w + n_b); return OFX_ERR_INVALID; }
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

static int launch_breed(ofx_handle *h, ofx_population *p, const int32_t *jobs, int n_jobs, double evo, double mut,
                        uint64_t seed, uint32_t generation) {
  if (n_jobs < 1) return OFX_OK;
  const dim3 grid((p->G + 255u) / 256u, (unsigned)(n_jobs < 65535 ? n_jobs : 65535));
  hipLaunchKernelGGL(k_pop_breed, grid, dim3(256), 0, h->stream, p->data, jobs, n_jobs, p->G, p->first,
                     (uint32_t)p->layers[0], (uint32_t)p->layers[1], evo, mut, ofx_key(seed), generation);
  OFX_HIP(hipGetLastError());
  return OFX_OK;
}

extern "C" int ofx_population_init(ofx_handle *h, uint64_t seed, uint32_t generation) {
  ofx_population *p;
  int rc = need_population(h, "ofx_population_init", &p);
  if (rc) return rc;
  OFX_HIP(hipSetDevice(h->cfg.device));
  return launch_breed(h, p, nullptr, (int)p->P, 0.0, 0.0, seed, generation);
}

// host <-> storage order of one genome: the first layer is transposed, the rest is the element order
static int check_slot(ofx_population *p, const char *who, int64_t slot, const void *w, const void *b) {
  if (!w || !b) { ofx_set_error("%s: null argument", who); return OFX_ERR_INVALID; }
  if (slot < 0 || slot >= p->P) { ofx_set_error("%s: slot %lld outside [0, %lld)", who, (long long)slot, (long long)p->P); return OFX_ERR_INVALID; }
  return OFX_OK;
}

extern "C" int ofx_population_get(ofx_handle *h, int64_t slot, double *weights_host, double *biases_host) {
  ofx_population *p;
  int rc = need_population(h, "ofx_population_get", &p);
  if (rc || (rc = check_slot(p, "ofx_population_get", slot, weights_host, biases_host))) return rc;
  OFX_HIP(hipSetDevice(h->cfg.device));
  std::vector<double> tmp(p->first);
  const double *src = p->data + (size_t)slot * p->G;
  OFX_HIP(hipStreamSynchronize(h->stream));
  OFX_HIP(hipMemcpy(tmp.data(), src, (size_t)p->first * sizeof(double), hipMemcpyDeviceToHost));
  OFX_HIP(hipMemcpy(weights_host + p->first, src + p->first, (size_t)(p->n_w - p->first) * sizeof(double), hipMemcpyDeviceToHost));
  OFX_HIP(hipMemcpy(biases_host, src + p->n_w, (size_t)(p->G - p->n_w) * sizeof(double), hipMemcpyDeviceToHost));
  const size_t nin = (size_t)p->layers[0], n1 = (size_t)p->layers[1];
  for (size_t k = 0; k < nin; k++)
    for (size_t o = 0; o < n1; o++) weights_host[o * nin + k] = tmp[k * n1 + o];
  return OFX_OK;
}

extern "C" int ofx_population_set(ofx_handle *h, int64_t slot, const double *weights_host, const double *biases_host) {
  ofx_population *p;
  int rc = need_population(h, "ofx_population_set", &p);
  if (rc || (rc = check_slot(p, "ofx_population_set", slot, weights_host, biases_host))) return rc;
  OFX_HIP(hipSetDevice(h->cfg.device));
  std::vector<double> tmp(p->first);
  const size_t nin = (size_t)p->layers[0], n1 = (size_t)p->layers[1];
  for (size_t k = 0; k < nin; k++)
    for (size_t o = 0; o < n1; o++) tmp[k * n1 + o] = weights_host[o * nin + k];
  double *dst = p->data + (size_t)slot * p->G;
  OFX_HIP(hipStreamSynchronize(h->stream));
  OFX_HIP(hipMemcpy(dst, tmp.data(), (size_t)p->first * sizeof(double), hipMemcpyHostToDevice));
  OFX_HIP(hipMemcpy(dst + p->first, weights_host + p->first, (size_t)(p->n_w - p->first) * sizeof(double), hipMemcpyHostToDevice));
  OFX_HIP(hipMemcpy(dst + p->n_w, biases_host, (size_t)(p->G - p->n_w) * sizeof(double), hipMemcpyHostToDevice));
  return OFX_OK;
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
  return launch_breed(h, p, p->jobs, (int)(jobs.size() / 2), evolution_rate, mutation_rate, seed, generation);
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
  pop_net net;
  net.n_layers = p->n_layers;
  for (int i = 0; i < POP_MAX_LAYERS; i++) net.layers[i] = i < p->n_layers ? p->layers[i] : 0;
  const int words = (int)(((size_t)c.width * c.height) >> 5);
  hipLaunchKernelGGL(k_pop_act, dim3((unsigned)(c.n_arenas * c.n_ships)), dim3(256), 0, h->stream, c.n_ships, c.width,
                     c.height, h->st, (const unsigned *)h->maps[OFX_MAP_BITS_LSB][0],
                     (const unsigned *)h->maps[OFX_MAP_BITS_LSB][1], words, p->data, (long long)p->P, p->G, p->first,
                     p->n_w, net, genome_of, actions, y);
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
