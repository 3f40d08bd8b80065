// ofx_es.hip - seeded evolution strategies: a population that is never stored (include/ofx.h, "evolution strategies")
// One centre genome theta of G doubles in the storage layout of ofx_genome.h.  Member m = 2i + b of P = 2 n_pairs is
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
// k_es_sigma_act / k_es_sigma_member / k_es_sigma_step  the same with a per-element exploration width sigma[e] beside
//              the centre, learned in the pass that steps the centre (PEPG with symmetric sampling).
// k_es_requeue_bank / k_es_requeue_assign  ofx_es_requeue: the ships of restarted arenas bank to the member they flew
//              (integer atomics) and take the next members of a device-side queue; tickets are ranks from a prefix count
//              over the arenas, never the order atomics land in.
#include "ofx_genome.h"

#include <new>
#include <vector>

struct ofx_es {
  genome_shape shape;
  double *theta;            // [G] the centre
  double *member;           // [G] ofx_es_member's buffer, allocated at its first call
  double *d;                // [d_cap] the listed pairs' weights of the running generation step, ascending pair order
  uint32_t *d_pair;         // [pair_cap] their pairs
  double *s;                // [s_cap] their sigma weights (ofx_es_sigma_step)
  size_t d_cap, pair_cap, s_cap;   // each list's device copy grows when a longer list comes (upload_list)
  double *m, *v;            // [G] each, theta's layout: the optimiser's moments (ofx_es_opt_create), null = none
  double *part;             // [3][ceil(G / 256)] k_es_step's per-workgroup sums of q^2, step^2, theta'^2
  double *sigma;            // [G] theta's layout: the per-element exploration width (ofx_es_sigma_create), null = none
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

// The signed width of a member at storage position s, stated per kind of ES: one scalar, ss = +sigma or -sigma, or a
// width per element, sgn * sigma[s] with sgn = +1 or -1 (the sign is exact), read where theta is read.
struct es_width_scalar {
  double ss;
  __device__ __forceinline__ double at(size_t) const { return ss; }
};
struct es_width_vector {
  const double *sigma;
  double sgn;
  __device__ __forceinline__ double at(size_t s) const { return sgn * sigma[s]; }
};
__device__ __forceinline__ es_width_scalar es_width_of(int m, double sigma) { return {(m & 1) ? -sigma : sigma}; }
__device__ __forceinline__ es_width_vector es_width_of(int m, const double *sigma) { return {sigma, (m & 1) ? -1.0 : 1.0}; }

// pop_forward's reader for member 2 * pair + b of the centre `theta`: w = theta + (ss * eps), the product rounded, then
// the sum (the library is built with -ffp-contract=off).  In the first layer storage position k * n1 + o is element
// o * nin + k; behind it the position is the element.
template <class Width>
struct es_member {
  const double *theta;
  uint32_t nin, pair, generation;
  ofx_rng_key key;
  Width width;
  __device__ __forceinline__ double noisy(double w, size_t s, uint32_t e) const {
    const double ss = width.at(s);
    const double t = ss * es_eps(pair, e, generation, key);
    return w + t;
  }
  __device__ __forceinline__ double first(size_t k, int o, int n1) const {
    const size_t s = k * n1 + o;
    return noisy(theta[s], s, (uint32_t)o * nin + (uint32_t)k);
  }
  __device__ __forceinline__ double at(size_t s) const { return noisy(theta[s], s, (uint32_t)s); }
};

// k_es_act and k_es_sigma_act stay two bodies: as one templated __device__ body (the width's kind deduced from sigma,
// arguments by value or by reference) both lost ~90 of their ~10 500 instructions - other streams, so not taken
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
    const es_member<es_width_scalar> rd = {theta, (uint32_t)net.layers[0], (uint32_t)m >> 1, generation, key,
                                           es_width_of(m, sigma)};
    cur = pop_forward<false>(s, a, W, H, st, ship_bits, laser_bits, words, rd, first, n_w, net, list, part, act, nullptr);
  }
  pop_emit(s, W, H, act[cur], actions, y);
}

// out[s] = member `m` of P at storage position s (m == P: the centre), under the scalar width or the vector `sigma`
template <class Sigma>
__device__ __forceinline__ void es_materialise(const double *theta, double *out, uint32_t G, uint32_t first,
                                               uint32_t nin, uint32_t n1, int m, int P, Sigma sigma, ofx_rng_key key,
                                               uint32_t generation) {
  const uint32_t s = blockIdx.x * 256u + threadIdx.x;
  if (s >= G) return;
  double w = theta[s];
  if (m != P) {
    const double ss = es_width_of(m, sigma).at(s);
    const double t = ss * es_eps((uint32_t)m >> 1, pop_element(s, first, nin, n1), generation, key);
    w = w + t;
  }
  out[s] = w;
}

__global__ __launch_bounds__(256) void k_es_member(const double *theta, double *out, uint32_t G, uint32_t first,
                                                   uint32_t nin, uint32_t n1, int m, int P, double sigma,
                                                   ofx_rng_key key, uint32_t generation) {
  es_materialise(theta, out, G, first, nin, n1, m, P, sigma, key, generation);
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

// The momentum and Adam lines of both steps for the element at s with gradient q; momentum never touches v.  The new
// first moment `mn` is the caller's to store: with the store in here, k_es_step<false, false> added w + step behind it.
template <bool ADAM>
__device__ __forceinline__ double es_moment_step(const es_law &c, double q, const double *m, double *v, uint32_t s,
                                                 double &mn) {
  const double t1 = c.c1 * m[s];
  const double t2 = c.k1 * q;
  mn = t1 + t2;
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
  return c.alpha * quo;
}

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
    double mn;
    const double step = es_moment_step<ADAM>(c, q, m, v, s, mn);
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
    // the tree stands here and in k_es_sigma_step: as one es_block_sums<R> body (with the LDS array in it, or handed
    // to it) the last stride and the final store came out as other instructions in every STATS kernel
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
// k_es_act with a width per element (es_width_vector); the centre still goes through pop_stored
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
    const es_member<es_width_vector> rd = {theta, (uint32_t)net.layers[0], (uint32_t)m >> 1, generation, key,
                                           es_width_of(m, sigma)};
    cur = pop_forward<false>(s, a, W, H, st, ship_bits, laser_bits, words, rd, first, n_w, net, list, part, act, nullptr);
  }
  pop_emit(s, W, H, act[cur], actions, y);
}

__global__ __launch_bounds__(256) void k_es_sigma_member(const double *theta, const double *sigma, double *out,
                                                         uint32_t G, uint32_t first, uint32_t nin, uint32_t n1, int m,
                                                         int P, ofx_rng_key key, uint32_t generation) {
  es_materialise(theta, out, G, first, nin, n1, m, P, sigma, key, generation);
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
// float64 operation; the optimiser's are k_es_step's (es_moment_step).  STATS: five workgroup sums - q^2, step^2,
// theta'^2, sigma'^2, clamped elements - in k_es_step's tree.
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
      double mn;
      step = es_moment_step<RULE == OFX_ES_RULE_ADAM>(c, q, m, v, s, mn);
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

// ---- host side ----
// ofx_es_requeue, pass 1 (include/ofx.h has the law).  One 64-lane wave per arena, lane = ship, four arenas per block as
// in k_restart_finished; an arena that did not restart costs its wave one byte read and one store.  Banking is integer
// atomics (exact in any order); what the arena wants from the queue is a ballot.  No block barrier.
__global__ __launch_bounds__(256) void k_es_requeue_bank(int N, int M, long long P, int bank, const uint8_t *restarted,
                                                         const int32_t *last_score, const int32_t *member_of,
                                                         const uint8_t *queue_mask, unsigned long long *sum, int *count,
                                                         int32_t *want, unsigned long long *completed) {
  const int a = blockIdx.x * OFX_ARENAS_PER_BLOCK + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (a >= N) return;  // wave-uniform
  if (!restarted[a]) {  // wave-uniform
    if (lane == 0) want[a] = 0;
    return;
  }
  const bool ship = lane < M;
  const size_t t = (size_t)a * M + lane;  // used under `ship` only
  const long long m = ship ? (long long)member_of[t] : -1;
  const bool banked = bank && m >= 0 && m <= P;
  if (banked) {
    atomicAdd(sum + m, (unsigned long long)(long long)last_score[t]);
    atomicAdd(count + m, 1);
  }
  const unsigned long long done = __ballot(banked && m < P), asks = __ballot(ship && queue_mask[t] != 0);
  if (lane == 0) {
    want[a] = __popcll(asks);
    if (done) atomicAdd(completed, (unsigned long long)__popcll(done));
  }
}

// Pass 2: ONE 256-thread workgroup.  Thread t owns the contiguous run of `run` = ceil(N / 256) arenas from t * run; the
// exclusive prefix of the runs' wants - a shuffle scan inside each wave, the four wave totals through LDS - is the rank of
// the run's first ticket, so tickets go out in ascending (arena, ship) order whatever order anything executes in.  A
// thread then walks only the arenas of its run that want tickets (want > 0 implies restarted).
__global__ __launch_bounds__(256) void k_es_requeue_assign(int N, int M, int run, long long P, long long total,
                                                           const int32_t *want, const uint8_t *queue_mask,
                                                           int32_t *member_of, long long *queue) {
  __shared__ int wave_sum[4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int first = min(tid * run, N), last = min(first + run, N);  // (run <= 2^23: tid * run fits)
  int mine = 0;
  for (int a = first; a < last; a++) mine += want[a];
  int incl = mine;
  for (int d = 1; d < 64; d <<= 1) {
    const int up = __shfl_up(incl, d);
    if (lane >= d) incl += up;
  }
  if (lane == 63) wave_sum[wave] = incl;
  __syncthreads();
  int base = incl - mine, all = 0;
  for (int w = 0; w < 4; w++) {
    if (w < wave) base += wave_sum[w];
    all += wave_sum[w];
  }
  const long long next = queue[0];
  const long long left = total > next ? total - next : 0;   // tickets still in the queue
  if (mine > 0) {
    long long rank = base;
    long long m = rank < left ? (next + rank) % P : 0;       // one division per thread; then m walks round P
    for (int a = first; a < last; a++) {
      if (want[a] == 0) continue;
      const size_t row = (size_t)a * M;
      for (int i = 0; i < M; i++) {
        if (!queue_mask[row + i]) continue;
        if (rank < left) {
          member_of[row + i] = (int32_t)m;
          if (++m == P) m = 0;
        } else {
          member_of[row + i] = -1;
        }
        rank++;
      }
    }
  }
  __syncthreads();  // every thread has read queue[0]
  if (tid == 0) queue[0] = next + (all < left ? (long long)all : left);
}

static ofx_es *&es_of(ofx_handle *h) { return h->es; }
static unsigned es_blocks(const ofx_es *p) { return p->shape.blocks(); }   // one thread per storage position

static void es_sigma_free(ofx_es *p) {
  genome_drop(p->sigma);
  genome_drop(p->sigma_part);
  genome_drop(p->s);
  p->s_cap = 0;
}

static void es_opt_free(ofx_es *p) {
  genome_drop(p->m);
  genome_drop(p->v);
  genome_drop(p->part);
}

void ofx_es_free(ofx_handle *h) {
  ofx_es *p = es_of(h);
  if (!p) return;
  genome_drop(p->theta);
  genome_drop(p->member);
  genome_drop(p->d);
  genome_drop(p->d_pair);
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

static int need_opt(ofx_handle *h, const char *who, ofx_es **out) {
  const int rc = need_es(h, who, out);
  if (!rc && !(*out)->m) { ofx_set_error("%s: the centre has no optimiser state (ofx_es_opt_create)", who); return OFX_ERR_STATE; }
  return rc;
}

static int need_sigma(ofx_handle *h, const char *who, ofx_es **out) {
  const int rc = need_es(h, who, out);
  if (!rc && !(*out)->sigma) { ofx_set_error("%s: the centre has no sigma vector (ofx_es_sigma_create)", who); return OFX_ERR_STATE; }
  return rc;
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

// a (weights, biases) pair of the caller's (`who`)
static int check_pair(const char *who, const void *weights_host, const void *biases_host) {
  if (!weights_host || !biases_host) { ofx_set_error("%s: null argument", who); return OFX_ERR_INVALID; }
  return OFX_OK;
}

extern "C" int ofx_es_create(ofx_handle *h, const int32_t *layers, int32_t n_layers) {
  if (!h || !layers) { ofx_set_error("ofx_es_create: null argument"); return OFX_ERR_INVALID; }
  if (es_of(h)) { ofx_set_error("ofx_es_create: the handle already holds an ES centre (ofx_es_destroy)"); return OFX_ERR_STATE; }
  genome_shape shape;
  const int rc = check_topology(h, "ofx_es_create", layers, n_layers, &shape);
  if (rc) return rc;
  OFX_HIP(hipSetDevice(h->cfg.device));
  ofx_es *p = new (std::nothrow) ofx_es();                 // every pointer null, every capacity 0
  if (!p) { ofx_set_error("ofx_es_create: out of host memory"); return OFX_ERR_INVALID; }
  p->shape = shape;
  const size_t bytes = (size_t)shape.G * sizeof(double);
  const hipError_t e = hipMalloc((void **)&p->theta, bytes);
  if (e != hipSuccess) {
    (void)hipGetLastError();
    ofx_set_error("ofx_es_create: allocating %zu bytes for a centre of %u elements failed: %s", bytes, shape.G,
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
  return launch_breed(h, p->theta, p->shape, nullptr, 1, 0.0, 0.0, seed, generation);
}

extern "C" int ofx_es_get(ofx_handle *h, double *weights_host, double *biases_host) {
  ofx_es *p;
  int rc = need_es(h, "ofx_es_get", &p);
  if (rc || (rc = check_pair("ofx_es_get", weights_host, biases_host))) return rc;
  OFX_HIP(hipSetDevice(h->cfg.device));
  return genome_to_host(h, p->theta, p->shape, weights_host, biases_host);
}

extern "C" int ofx_es_set(ofx_handle *h, const double *weights_host, const double *biases_host) {
  ofx_es *p;
  int rc = need_es(h, "ofx_es_set", &p);
  if (rc || (rc = check_pair("ofx_es_set", weights_host, biases_host))) return rc;
  OFX_HIP(hipSetDevice(h->cfg.device));
  return genome_from_host(h, p->theta, p->shape, weights_host, biases_host);
}

// The body of ofx_es_member and ofx_es_sigma_member (`who`, which has checked the centre and P): the member under the
// scalar `sigma`, or per_element under the sigma vector, into the member buffer - allocated here first - and to the host.
static int es_member_to_host(ofx_handle *h, ofx_es *p, const char *who, bool per_element, int64_t member, int64_t P,
                             double sigma, uint64_t seed, uint32_t generation, double *weights_host,
                             double *biases_host) {
  int rc = check_pair(who, weights_host, biases_host);
  if (rc) return rc;
  if (member < 0 || member > P) {
    ofx_set_error("%s: member %lld outside [0, %lld] (P is the centre)", who, (long long)member, (long long)P);
    return OFX_ERR_INVALID;
  }
  OFX_HIP(hipSetDevice(h->cfg.device));
  const genome_shape &g = p->shape;
  if (!p->member) {
    const hipError_t e = hipMalloc((void **)&p->member, (size_t)g.G * sizeof(double));
    if (e != hipSuccess) {
      (void)hipGetLastError();
      p->member = nullptr;
      ofx_set_error("%s: allocating %zu bytes failed: %s", who, (size_t)g.G * sizeof(double), hipGetErrorString(e));
      return OFX_ERR_HIP;
    }
  }
  if (per_element)
    hipLaunchKernelGGL(k_es_sigma_member, dim3(es_blocks(p)), dim3(256), 0, h->stream, p->theta, p->sigma, p->member, g.G,
                       g.first, g.nin(), g.n1(), (int)member, (int)P, ofx_key(seed), generation);
  else
    hipLaunchKernelGGL(k_es_member, dim3(es_blocks(p)), dim3(256), 0, h->stream, p->theta, p->member, g.G, g.first,
                       g.nin(), g.n1(), (int)member, (int)P, sigma, ofx_key(seed), generation);
  OFX_HIP(hipGetLastError());
  return genome_to_host(h, p->member, g, weights_host, biases_host);
}

extern "C" int ofx_es_member(ofx_handle *h, int64_t member, int64_t P, double sigma, uint64_t seed, uint32_t generation,
                             double *weights_host, double *biases_host) {
  ofx_es *p;
  int rc = need_es(h, "ofx_es_member", &p);
  if (rc || (rc = check_members("ofx_es_member", P, sigma))) return rc;
  return es_member_to_host(h, p, "ofx_es_member", false, member, P, sigma, seed, generation, weights_host, biases_host);
}

// the body of ofx_es_act and ofx_es_sigma_act (`who`, which has checked the centre and P): as es_member_to_host
static int es_forward(ofx_handle *h, ofx_es *p, const char *who, bool per_element, const int32_t *member_of, int64_t P,
                      double sigma, uint64_t seed, uint32_t generation, ofx_action *actions, double *y) {
  if (!member_of || !actions) { ofx_set_error("%s: null argument", who); return OFX_ERR_INVALID; }
  pop_maps mp;
  const int rc = pop_forward_begin(h, &mp);
  if (rc) return rc;
  const ofx_config &c = h->cfg;
  const genome_shape &g = p->shape;
  if (per_element)
    hipLaunchKernelGGL(k_es_sigma_act, mp.grid, dim3(256), 0, h->stream, c.n_ships, c.width, c.height, h->st, mp.ship_bits,
                       mp.laser_bits, mp.words, p->theta, p->sigma, (int)P, g.first, g.n_w, net_of(g), ofx_key(seed),
                       generation, member_of, actions, y);
  else
    hipLaunchKernelGGL(k_es_act, mp.grid, dim3(256), 0, h->stream, c.n_ships, c.width, c.height, h->st, mp.ship_bits,
                       mp.laser_bits, mp.words, p->theta, (int)P, g.first, g.n_w, net_of(g), sigma, ofx_key(seed),
                       generation, member_of, actions, y);
  OFX_HIP(hipGetLastError());
  return OFX_OK;
}

extern "C" int ofx_es_act(ofx_handle *h, const int32_t *member_of, int64_t P, double sigma, uint64_t seed,
                          uint32_t generation, ofx_action *actions, double *y) {
  ofx_es *p;
  int rc = need_es(h, "ofx_es_act", &p);
  if (rc || (rc = check_members("ofx_es_act", P, sigma))) return rc;
  return es_forward(h, p, "ofx_es_act", false, member_of, P, sigma, seed, generation, actions, y);
}

extern "C" int ofx_es_fitness(ofx_handle *h, const int32_t *member_of, int64_t P, int64_t *sum, int32_t *count,
                              int32_t reset) {
  ofx_es *p;
  int rc = need_es(h, "ofx_es_fitness", &p);
  if (rc || (rc = check_members("ofx_es_fitness", P, 1.0))) return rc;
  if (!member_of || !sum || !count) { ofx_set_error("ofx_es_fitness: null argument"); return OFX_ERR_INVALID; }
  if (!h->spawned) { ofx_set_error("ofx_es_fitness before ofx_spawn"); return OFX_ERR_STATE; }
  return launch_fitness(h, (size_t)P + 1, member_of, sum, count, reset);   // slot P: the centre
}

extern "C" int ofx_es_requeue(ofx_handle *h, int32_t *member_of, const uint8_t *queue_mask, int64_t P, int64_t total,
                              int64_t *queue, int64_t *sum, int32_t *count, int32_t bank) {
  if (!h) { ofx_set_error("ofx_es_requeue: null handle"); return OFX_ERR_INVALID; }
  if (!member_of || !queue_mask || !queue || !sum || !count) {
    ofx_set_error("ofx_es_requeue: null argument");
    return OFX_ERR_INVALID;
  }
  const int rc = check_members("ofx_es_requeue", P, 1.0);
  if (rc) return rc;
  if (total < 0) { ofx_set_error("ofx_es_requeue: total must be >= 0 (got %lld)", (long long)total); return OFX_ERR_INVALID; }
  if (!h->ar_restarted) {
    ofx_set_error("ofx_es_requeue: no arena has its own episodes yet (ofx_restart_finished or ofx_restart_arenas first)");
    return OFX_ERR_STATE;
  }
  OFX_HIP(hipSetDevice(h->cfg.device));
  const int N = h->cfg.n_arenas, M = h->cfg.n_ships;
  if (!h->ar_want) OFX_HIP(hipMalloc((void **)&h->ar_want, (size_t)N * sizeof(int32_t)));  // pass 1 writes all of it
  hipLaunchKernelGGL(k_es_requeue_bank, dim3(arena_blocks(N)), dim3(256), 0, h->stream, N, M, (long long)P, (int)(bank != 0),
                     h->ar_restarted, h->st.last_score, member_of, queue_mask, (unsigned long long *)sum, count, h->ar_want,
                     (unsigned long long *)(queue + 1));
  OFX_HIP(hipGetLastError());
  hipLaunchKernelGGL(k_es_requeue_assign, dim3(1), dim3(256), 0, h->stream, N, M, (N + 255) / 256, (long long)P,
                     (long long)total, h->ar_want, queue_mask, member_of, (long long *)queue);
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

// what one generation step lists: the pairs with a weight, ascending, and their weights
struct es_pairs {
  std::vector<double> d, s;
  std::vector<uint32_t> pair;
};

// The pairs with a weight - d, or s where the step has one (s_host != NULL).  A pair whose weights are 0 adds +-0 to
// sums that start at +0.0 and can never be -0.0 (x + (-x) rounds to +0), so leaving it out changes no bit: ties and
// incomplete pairs, the common case, cost nothing.
static int listed_pairs(const char *who, const double *d_host, const double *s_host, int64_t n_pairs, es_pairs &out) {
  for (int64_t i = 0; i < n_pairs; i++) {
    if (!(d_host[i] - d_host[i] == 0.0)) { ofx_set_error("%s: d[%lld] is not finite", who, (long long)i); return OFX_ERR_INVALID; }
    if (s_host && !(s_host[i] - s_host[i] == 0.0)) { ofx_set_error("%s: s[%lld] is not finite", who, (long long)i); return OFX_ERR_INVALID; }
    if (d_host[i] == 0.0 && !(s_host && s_host[i] != 0.0)) continue;
    out.d.push_back(d_host[i]);
    if (s_host) out.s.push_back(s_host[i]);
    out.pair.push_back((uint32_t)i);
  }
  return OFX_OK;
}

// a host list into its device copy, which grows when the list is longer than any before it
template <class T>
static int upload_list(T *&dev, size_t &cap, const std::vector<T> &host) {
  if (host.size() > cap) {
    genome_drop(dev);
    cap = 0;
    OFX_HIP(hipMalloc((void **)&dev, host.size() * sizeof(T)));
    cap = host.size();
  }
  if (!host.empty()) OFX_HIP(hipMemcpy(dev, host.data(), host.size() * sizeof(T), hipMemcpyHostToDevice));
  return OFX_OK;
}

// the step's lists into the centre's device copies, after the work already on the handle's stream
static int upload_pairs(ofx_handle *h, ofx_es *p, const es_pairs &l) {
  OFX_HIP(hipSetDevice(h->cfg.device));
  OFX_HIP(hipStreamSynchronize(h->stream));  // the last step may still read the lists
  int rc = upload_list(p->d, p->d_cap, l.d);
  if (!rc) rc = upload_list(p->d_pair, p->pair_cap, l.pair);
  if (!rc) rc = upload_list(p->s, p->s_cap, l.s);
  return rc;
}

extern "C" int ofx_es_update(ofx_handle *h, const double *d_host, int64_t n_pairs, double scale, uint64_t seed,
                             uint32_t generation) {
  ofx_es *p;
  int rc = need_es(h, "ofx_es_update", &p);
  if (rc || (rc = check_pairs("ofx_es_update", d_host, n_pairs))) return rc;
  if (!(scale - scale == 0.0)) { ofx_set_error("ofx_es_update: scale is not finite"); return OFX_ERR_INVALID; }
  es_pairs l;
  if ((rc = listed_pairs("ofx_es_update", d_host, nullptr, n_pairs, l)) || (rc = upload_pairs(h, p, l))) return rc;
  const genome_shape &g = p->shape;
  hipLaunchKernelGGL(k_es_update, dim3(es_blocks(p)), dim3(256), 0, h->stream, p->theta, p->d, p->d_pair,
                     (int)l.d.size(), g.G, g.first, g.nin(), g.n1(), scale, ofx_key(seed), generation);
  OFX_HIP(hipGetLastError());
  return OFX_OK;
}

// ---- the optimiser of the centre (include/ofx.h: ofx_es_opt_*, ofx_es_step) ----
extern "C" int ofx_es_opt_create(ofx_handle *h) {
  ofx_es *p;
  const int rc = need_es(h, "ofx_es_opt_create", &p);
  if (rc) return rc;
  if (p->m) { ofx_set_error("ofx_es_opt_create: the centre already has optimiser state (ofx_es_opt_destroy)"); return OFX_ERR_STATE; }
  OFX_HIP(hipSetDevice(h->cfg.device));
  const size_t bytes = (size_t)p->shape.G * sizeof(double);
  hipError_t e = hipMalloc((void **)&p->m, bytes);
  if (e == hipSuccess) e = hipMalloc((void **)&p->v, bytes);
  if (e == hipSuccess) e = hipMalloc((void **)&p->part, 3 * (size_t)es_blocks(p) * sizeof(double));
  if (e != hipSuccess) {
    (void)hipGetLastError();
    ofx_set_error("ofx_es_opt_create: allocating 2 x %zu bytes for the moments of %u elements failed: %s", bytes,
                  p->shape.G, hipGetErrorString(e));
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
  if ((rc = genome_to_host(h, p->m, p->shape, m_weights, m_biases))) return rc;
  return genome_to_host(h, p->v, p->shape, v_weights, v_biases);
}

extern "C" int ofx_es_opt_set(ofx_handle *h, const double *m_weights, const double *m_biases, const double *v_weights,
                              const double *v_biases) {
  ofx_es *p;
  int rc = need_opt(h, "ofx_es_opt_set", &p);
  if (rc) return rc;
  if (!m_weights || !m_biases || !v_weights || !v_biases) { ofx_set_error("ofx_es_opt_set: null argument"); return OFX_ERR_INVALID; }
  OFX_HIP(hipSetDevice(h->cfg.device));
  if ((rc = genome_from_host(h, p->m, p->shape, m_weights, m_biases))) return rc;
  return genome_from_host(h, p->v, p->shape, v_weights, v_biases);
}

// The scalars of a step law as both generation steps take them (`who`; z: the three ofx_es_sigma_step adds, or NULL):
// every one finite, then the ranges.  The rule itself is the caller's to check: the two steps accept different ones.
static int check_law(const char *who, int32_t rule, const es_law &c, const es_sigma_law *z) {
  static const char *const names[11] = {"gscale", "decay", "alpha", "c1", "k1", "c2", "k2", "eps", "srate", "smin", "smax"};
  const double scalars[11] = {c.gscale, c.decay, c.alpha, c.c1, c.k1, c.c2, c.k2, c.eps,
                              z ? z->srate : 0.0, z ? z->smin : 0.0, z ? z->smax : 0.0};
  for (int i = 0; i < (z ? 11 : 8); i++)
    if (!(scalars[i] - scalars[i] == 0.0)) { ofx_set_error("%s: %s is not finite", who, names[i]); return OFX_ERR_INVALID; }
  if (c.decay < 0.0) { ofx_set_error("%s: decay must be >= 0 (got %g)", who, c.decay); return OFX_ERR_INVALID; }
  if (rule == OFX_ES_RULE_ADAM && !(c.eps > 0.0)) { ofx_set_error("%s: eps must be > 0 under Adam (got %g)", who, c.eps); return OFX_ERR_INVALID; }
  if (!z) return OFX_OK;
  if (!(z->smin > 0.0)) { ofx_set_error("%s: smin must be > 0 (got %g)", who, z->smin); return OFX_ERR_INVALID; }
  if (z->smax < z->smin) { ofx_set_error("%s: smax must be >= smin (got smax %g, smin %g)", who, z->smax, z->smin); return OFX_ERR_INVALID; }
  return OFX_OK;
}

// k_es_stats over the nb workgroup sums a step with stats has just left in `part`
template <int R>
static int launch_stats(ofx_handle *h, const ofx_es *p, const double *part, double *stats) {
  hipLaunchKernelGGL(k_es_stats<R>, dim3(1), dim3(256), 0, h->stream, part, (int)es_blocks(p), stats);
  OFX_HIP(hipGetLastError());
  return OFX_OK;
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
  es_pairs l;
  if ((rc = check_law("ofx_es_step", rule, law, nullptr)) || (rc = listed_pairs("ofx_es_step", d_host, nullptr, n_pairs, l)) ||
      (rc = upload_pairs(h, p, l)))
    return rc;
  // the kernel instance of (rule, stats): [Adam][stats]
  static const decltype(&k_es_step<false, false>) kernel[2][2] = {{k_es_step<false, false>, k_es_step<false, true>},
                                                                  {k_es_step<true, false>, k_es_step<true, true>}};
  const genome_shape &g = p->shape;
  hipLaunchKernelGGL(kernel[rule == OFX_ES_RULE_ADAM][stats != nullptr], dim3(es_blocks(p)), dim3(256), 0, h->stream,
                     p->theta, p->m, p->v, p->d, p->d_pair, (int)l.d.size(), g.G, g.first, g.nin(), g.n1(), law,
                     ofx_key(seed), generation, p->part);
  OFX_HIP(hipGetLastError());
  return stats ? launch_stats<3>(h, p, p->part, stats) : OFX_OK;
}

// ---- per-element adaptive sigma (include/ofx.h: ofx_es_sigma_*) ----
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
  const size_t bytes = (size_t)p->shape.G * sizeof(double);
  hipError_t e = hipMalloc((void **)&p->sigma, bytes);
  if (e == hipSuccess) e = hipMalloc((void **)&p->sigma_part, 5 * (size_t)es_blocks(p) * sizeof(double));
  if (e != hipSuccess) {
    (void)hipGetLastError();
    ofx_set_error("ofx_es_sigma_create: allocating %zu bytes for the sigma of %u elements failed: %s", bytes, p->shape.G,
                  hipGetErrorString(e));
    es_sigma_free(p);
    return OFX_ERR_HIP;
  }
  hipLaunchKernelGGL(k_es_fill, dim3(es_blocks(p)), dim3(256), 0, h->stream, p->sigma, p->shape.G, sigma0);
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
  if (rc || (rc = check_pair("ofx_es_sigma_get", weights_host, biases_host))) return rc;
  OFX_HIP(hipSetDevice(h->cfg.device));
  return genome_to_host(h, p->sigma, p->shape, weights_host, biases_host);
}

extern "C" int ofx_es_sigma_set(ofx_handle *h, const double *weights_host, const double *biases_host) {
  ofx_es *p;
  int rc = need_sigma(h, "ofx_es_sigma_set", &p);
  if (rc || (rc = check_pair("ofx_es_sigma_set", weights_host, biases_host))) return rc;
  const genome_shape &g = p->shape;
  for (uint32_t i = 0; i < g.G; i++) {
    const double x = i < g.n_w ? weights_host[i] : biases_host[i - g.n_w];
    if (!(x - x == 0.0) || !(x > 0.0)) {
      ofx_set_error("ofx_es_sigma_set: sigma[%u] must be finite and > 0 (got %g)", i, x);
      return OFX_ERR_INVALID;
    }
  }
  OFX_HIP(hipSetDevice(h->cfg.device));
  return genome_from_host(h, p->sigma, g, weights_host, biases_host);
}

extern "C" int ofx_es_sigma_member(ofx_handle *h, int64_t member, int64_t P, uint64_t seed, uint32_t generation,
                                   double *weights_host, double *biases_host) {
  ofx_es *p;
  int rc = need_sigma(h, "ofx_es_sigma_member", &p);
  if (rc || (rc = check_members("ofx_es_sigma_member", P, 1.0))) return rc;
  return es_member_to_host(h, p, "ofx_es_sigma_member", true, member, P, 1.0, seed, generation, weights_host,
                           biases_host);
}

extern "C" int ofx_es_sigma_act(ofx_handle *h, const int32_t *member_of, int64_t P, uint64_t seed, uint32_t generation,
                                ofx_action *actions, double *y) {
  ofx_es *p;
  int rc = need_sigma(h, "ofx_es_sigma_act", &p);
  if (rc || (rc = check_members("ofx_es_sigma_act", P, 1.0))) return rc;
  return es_forward(h, p, "ofx_es_sigma_act", true, member_of, P, 1.0, seed, generation, actions, y);
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
  if ((rc = check_law("ofx_es_sigma_step", rule, law, &z))) return rc;
  if (rule != OFX_ES_RULE_PLAIN && !p->m) {
    ofx_set_error("ofx_es_sigma_step: the centre has no optimiser state (ofx_es_opt_create), which rule %d needs", rule);
    return OFX_ERR_STATE;
  }
  es_pairs l;
  if ((rc = listed_pairs("ofx_es_sigma_step", d_host, s_host, n_pairs, l)) || (rc = upload_pairs(h, p, l))) return rc;
  static_assert(OFX_ES_RULE_PLAIN == 0 && OFX_ES_RULE_MOMENTUM == 1 && OFX_ES_RULE_ADAM == 2, "kernel[rule][stats]");
  static const decltype(&k_es_sigma_step<0, false>) kernel[3][2] = {
      {k_es_sigma_step<OFX_ES_RULE_PLAIN, false>, k_es_sigma_step<OFX_ES_RULE_PLAIN, true>},
      {k_es_sigma_step<OFX_ES_RULE_MOMENTUM, false>, k_es_sigma_step<OFX_ES_RULE_MOMENTUM, true>},
      {k_es_sigma_step<OFX_ES_RULE_ADAM, false>, k_es_sigma_step<OFX_ES_RULE_ADAM, true>}};
  const genome_shape &g = p->shape;
  hipLaunchKernelGGL(kernel[rule][stats != nullptr], dim3(es_blocks(p)), dim3(256), 0, h->stream, p->theta, p->sigma,
                     p->m, p->v, p->d, p->s, p->d_pair, (int)l.d.size(), g.G, g.first, g.nin(), g.n1(), law, z,
                     ofx_key(seed), generation, p->sigma_part);
  OFX_HIP(hipGetLastError());
  return stats ? launch_stats<5>(h, p, p->sigma_part, stats) : OFX_OK;
}

