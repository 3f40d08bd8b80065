// ofx_replay.hip - device-side transition capture: the batched form of Trainer.memory = deque(maxlen=memory_size)
// (agents/qlearnIA_V2.py:58), Trainer.remember (:237-238) and the bookkeeping of QlearnIA.play (:370-403) /
// QlearnIA.reset (:360-368).  Every arena owns one memory (the reference has one arena and one shared TRAINER).
//
// Layout in HBM (288 GB per GPU: the whole memory stays resident; only a checkpoint takes it to the host, the frame ring
// packed to its nonzero words - ofx_replay_export at the end of this file):
//   frames  [N][F][2][W*H/32] u32   1-bit observation maps (20 KB per map): a ring of F frames per arena.  An arena
//                                    stores a frame only on lock-steps where one of its agents plays; the maps are
//                                    shared by every ship of the arena and by the two transitions that touch them
//                                    (next_state of t-1 -> t, state of t -> t+1), so they are stored once.
//   rows    [N][C] ofx_transition    ring of the last C transitions per arena in append order (lock-step, then ship
//                                    index: the order of request_actions, battleground.py:146-150)
//   per ship [N][M]                  previous_obs / previous_action / previous_pointer (+ the toVector head) and the
//                                    agent's `done` latch
// Packed form of the frame ring (ofx_replay_create_packed; include/ofx.h, "packed frame store", states the contract):
//   pool      [N][pool_pairs] uint2   cyclic buffer of (word index, word) pairs of the nonzero words of the live frames
//   frame_off [N][F] u32, frame_cnt [N][F][2] u32, pool_head [N] u32, live [N] u32, evicted [N] i64
// Every reader of a frame goes through frame_read below; the dense form is the plain 16-byte copy it always was.
#include "ofx_internal.h"
#include "ofx_packed.h"
#include <float.h>
#include <string.h>

struct ofx_replay {
  int32_t capacity, frames, words;
  uint32_t *frame_bits;    // [N][F][2][words]
  int32_t *frame_tick;     // [N][F]  lock-step stored in the slot, -1 = empty
  int32_t *frame_head;     // [N] next slot
  int32_t *cur_slot;       // [N] slot written by the running capture, -1 = none
  ofx_transition *rows;    // [N][C]
  int32_t *head;           // [N] next write position
  int32_t *count;          // [N] min(appended, C)
  long long *appended;     // [N]
  // per ship
  uint8_t *has_prev, *latched;
  int32_t *prev_iaction, *prev_px, *prev_py, *prev_tick, *prev_slot;
  float *prev_head;        // [N][M][8]
  int32_t *scan_off;       // [N + 1] prefix sums of ofx_replay_gather_valid (kept: no allocation per replay)
  // prioritized replay (ofx_replay_prioritize), null = off
  float *mass;             // [N][C] p^alpha, same ring positions as rows
  float *mmax;             // [N] running maximum mass: what a new row gets
  float alpha, eps;
  // actor-side initial priorities (ofx_replay_actor_priorities), null = off
  float *prev_q;           // [N][M][2] (q_sa, p_sp) of each ship's previous_*, next to prev_iaction
  float actor_gamma;
  // packed frame store (ofx_replay_create_packed), frame_bits is null then
  int32_t packed;
  uint32_t pool_pairs;     // per arena
  uint2 *pool;             // [N][pool_pairs]
  uint32_t *frame_off;     // [N][F]    pool position of the slot's first pair
  uint32_t *frame_cnt;     // [N][F][2] pairs of the ship map / of the laser map; 0 in slots that hold no live frame
  uint32_t *pool_head;     // [N]
  uint32_t *live;          // [N] pairs of all live frames
  long long *evicted;      // [N] frames released early, since create
  // workspace of the global sampler (ofx_replay_sample_global), allocated at its first call; not part of a checkpoint
  int32_t *g_skip, *g_v;   // [N] expired oldest rows / eligible rows
  long long *g_voff;       // [N + 1] exclusive scan of g_v, R in [N]
  double *g_T, *g_G;       // [N] arena mass totals / their inclusive cross-arena prefix
  double *g_gs;            // [ceil(N / 256)] the groups' last running sums
  // ofx_replay_reward_source: caller-owned device [N][M] a completed row's reward comes from, null = the state's field
  const int32_t *reward_src;
};

void ofx_replay_free(ofx_handle *h) {
  ofx_replay *r = h->replay;
  if (!r) return;
  void *ptrs[] = {r->frame_bits, r->frame_tick, r->rows, r->head, r->count, r->appended, r->has_prev, r->latched,
                  r->prev_iaction, r->prev_px, r->prev_py, r->prev_tick, r->prev_head, r->frame_head, r->cur_slot,
                  r->prev_slot, r->scan_off, r->mass, r->mmax, r->pool, r->frame_off, r->frame_cnt, r->pool_head, r->live,
                  r->evicted, r->g_skip, r->g_v, r->g_voff, r->g_T, r->g_G, r->g_gs, r->prev_q};
  for (void *p : ptrs) if (p) (void)hipFree(p);
  delete r;
  h->replay = nullptr;
}

// The rows of one arena as every reader sees them: `count` rows, oldest first, that end in front of `head` in a ring of
// C positions (rows and mass share the positions).  at(i) is the ring position of oldest-first row i.
struct RowRing {
  int C, first, count;
  __host__ __device__ __forceinline__ int at(int i) const { return (first + i) % C; }
};
__host__ __device__ __forceinline__ RowRing row_ring(int C, int head, int count) {
  return RowRing{C, ((head - count) % C + C) % C, count};
}

template <typename T>
static int zalloc(T **p, size_t count, int fill = 0) {
  OFX_HIP(hipMalloc((void **)p, sizeof(T) * count));
  OFX_HIP(hipMemset(*p, fill, sizeof(T) * count));
  return OFX_OK;
}

#define OFX_LDS_LIMIT (64 * 1024) /* dynamic LDS a launch may ask for: the packed readers build a frame's two maps there */

// ofx_replay_create (pool_pairs < 0: the dense ring) and ofx_replay_create_packed (pool_pairs >= 0)
static int replay_create(ofx_handle *h, const char *who, int32_t capacity, int32_t frames, int64_t pool_pairs) {
  if (!h) { ofx_set_error("%s: null handle", who); return OFX_ERR_INVALID; }
  if (capacity <= 0 || frames < 0 || frames == 1) {
    ofx_set_error("%s: capacity must be > 0 and frames >= 2 (or 0 = capacity + capacity / 4 + 2), got %d, %d", who,
                  capacity, frames);
    return OFX_ERR_INVALID;
  }
  if (((size_t)h->cfg.width * h->cfg.height) % 128) {
    ofx_set_error("%s: width*height must be a multiple of 128", who);
    return OFX_ERR_INVALID;
  }
  const bool packed = pool_pairs >= 0;
  if (packed) {
    const int32_t F = frames ? frames : capacity + capacity / 4 + 2, words = (int32_t)(((size_t)h->cfg.width * h->cfg.height) >> 5);
    int64_t low, high;
    const int64_t want = pool_pairs;
    pool_pairs = ofx_packed_pool_pairs(want, F, words, &low, &high);
    if (!pool_pairs) {
      ofx_set_error("%s: pool_pairs must be 0 (= max(512 * frames, 4 * words)) or lie in [4 * words, 2^31) = [%lld, %lld), got %lld",
                    who, (long long)low, (long long)high, (long long)(want ? want : 512 * (int64_t)F));
      return OFX_ERR_INVALID;
    }
    if ((size_t)words * 8 > OFX_LDS_LIMIT) {
      ofx_set_error("%s: the two maps of a frame (%zu bytes) exceed the %d bytes of LDS the packed gather builds them in", who,
                    (size_t)words * 8, OFX_LDS_LIMIT);
      return OFX_ERR_INVALID;
    }
  }
  OFX_HIP(hipSetDevice(h->cfg.device));
  OFX_HIP(hipStreamSynchronize(h->stream));
  ofx_replay_free(h);
  ofx_replay *r = new ofx_replay();
  memset(r, 0, sizeof(*r));
  h->replay = r;
  const size_t N = h->cfg.n_arenas, M = h->cfg.n_ships;
  r->capacity = capacity;
  // C rows made of runs of consecutive plays need C + (number of runs) frames; 2C covers every case
  r->frames = frames ? frames : capacity + capacity / 4 + 2;
  r->words = (int32_t)(((size_t)h->cfg.width * h->cfg.height) >> 5);
  int rc;
#define A(field, count, fill) if ((rc = zalloc(&r->field, (count), (fill)))) { ofx_replay_free(h); return rc; }
  if (packed) {
    r->packed = 1;
    r->pool_pairs = (uint32_t)pool_pairs;
    A(pool, N * (size_t)pool_pairs, 0)
    A(frame_off, N * (size_t)r->frames, 0) A(frame_cnt, N * (size_t)r->frames * 2, 0)
    A(pool_head, N, 0) A(live, N, 0) A(evicted, N, 0)
  } else {
    A(frame_bits, (size_t)r->frames * 2 * N * r->words, 0)
  }
  A(frame_tick, N * (size_t)r->frames, 0xFF)
  A(frame_head, N, 0) A(cur_slot, N, 0xFF) A(prev_slot, N * M, 0)
  A(rows, N * (size_t)capacity, 0)
  A(head, N, 0) A(count, N, 0) A(appended, N, 0)
  A(has_prev, N * M, 0) A(latched, N * M, 0)
  A(prev_iaction, N * M, 0) A(prev_px, N * M, 0) A(prev_py, N * M, 0) A(prev_tick, N * M, 0)
  A(prev_head, N * M * 8, 0)
  A(scan_off, N + 1, 0)
#undef A
  OFX_HIP(hipDeviceSynchronize());  // null-stream fills vs the handle's non-blocking stream
  return OFX_OK;
}

extern "C" int ofx_replay_create(ofx_handle *h, int32_t capacity, int32_t frames) {
  return replay_create(h, "ofx_replay_create", capacity, frames, -1);
}

extern "C" int ofx_replay_create_packed(ofx_handle *h, int32_t capacity, int32_t frames, int64_t pool_pairs) {
  if (pool_pairs < 0) {
    ofx_set_error("ofx_replay_create_packed: pool_pairs must be 0 (the default) or lie in [4 * words, 2^31), got %lld",
                  (long long)pool_pairs);
    return OFX_ERR_INVALID;
  }
  return replay_create(h, "ofx_replay_create_packed", capacity, frames, pool_pairs);
}

extern "C" int ofx_replay_store_stats(ofx_handle *h, int64_t *stats_host) {
  if (!h || !stats_host) { ofx_set_error("ofx_replay_store_stats: null argument"); return OFX_ERR_INVALID; }
  ofx_replay *r = h->replay;
  if (!r) { ofx_set_error("ofx_replay_store_stats: no replay memory"); return OFX_ERR_STATE; }
  OFX_HIP(hipSetDevice(h->cfg.device));
  OFX_HIP(hipStreamSynchronize(h->stream));
  const size_t N = h->cfg.n_arenas;
  for (int i = 0; i < 6; i++) stats_host[i] = 0;
  if (!r->packed) {
    stats_host[5] = (int64_t)(sizeof(uint32_t) * N * (size_t)r->frames * 2 * r->words);
    return OFX_OK;
  }
  uint32_t *live = (uint32_t *)malloc(sizeof(uint32_t) * N);
  long long *ev = (long long *)malloc(sizeof(long long) * N);
  hipError_t e = (live && ev) ? hipMemcpy(live, r->live, sizeof(uint32_t) * N, hipMemcpyDeviceToHost) : hipErrorOutOfMemory;
  if (e == hipSuccess) e = hipMemcpy(ev, r->evicted, sizeof(long long) * N, hipMemcpyDeviceToHost);
  if (e == hipSuccess) {
    stats_host[0] = 1;
    stats_host[1] = r->pool_pairs;
    for (size_t a = 0; a < N; a++) {
      if ((int64_t)live[a] > stats_host[2]) stats_host[2] = live[a];
      stats_host[3] += live[a];
      stats_host[4] += ev[a];
    }
    stats_host[5] = ofx_packed_store_bytes((int64_t)N, r->frames, r->pool_pairs);
  }
  free(live);
  free(ev);
  OFX_HIP(e);
  return OFX_OK;
}

extern "C" int ofx_replay_destroy(ofx_handle *h) {
  if (!h) return OFX_OK;
  (void)hipSetDevice(h->cfg.device);
  if (h->stream) (void)hipStreamSynchronize(h->stream);
  ofx_replay_free(h);
  return OFX_OK;
}

// QlearnIA.reset (qlearnIA_V2.py:360-368): done = False, previous_* = None.  The memory itself survives.
__global__ void k_replay_episode(int N, int M, const uint8_t *arena_mask, uint8_t *has_prev, uint8_t *latched) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= N * M) return;
  if (arena_mask && !arena_mask[t / M]) return;
  has_prev[t] = 0;
  latched[t] = 0;
}

int ofx_replay_episode_reset(ofx_handle *h, const uint8_t *arena_mask) {
  ofx_replay *r = h->replay;
  if (!r) return OFX_OK;
  const int T = h->cfg.n_arenas * h->cfg.n_ships;
  hipLaunchKernelGGL(k_replay_episode, dim3((T + 255) / 256), dim3(256), 0, h->stream, h->cfg.n_arenas, h->cfg.n_ships,
                     arena_mask, r->has_prev, r->latched);
  OFX_HIP(hipGetLastError());
  return OFX_OK;
}

struct CaptureParams {
  int N, M, W, H, C, F;
  int tick;
  ofx_state st;
  const uint8_t *mask;
  const int32_t *iaction, *ipointer;
  const float *q_sa, *p_sp, *v_act, *v_ptr;  // [N][M] of ofx_replay_capture_valued, unread by the plain form
  ofx_replay r;
};

// PER mass of a row from its two signed TD errors (both finite): the write-backs and the valued capture share it
__device__ __forceinline__ float per_mass(float e1, float e2, float eps, float alpha) {
  return powf(fabsf(e1) + fabsf(e2) + eps, alpha);
}

// One 64-lane wave per arena, lane = ship.  QlearnIA.play (qlearnIA_V2.py:370-403) per capturing ship:
//   if self.done: return                      -> nothing, not even previous_* changes
//   if obs.done: self.done = True             -> the losing frame is still remembered below
//   if previous_*: remember(previous_obs, previous_action, previous_pointer, obs.reward, obs, obs.done)
//   previous_* = obs, iaction, ipointer
// Rows are appended in ship-index order (ballot prefix), exactly the deque's append order.
// VALUED (ofx_replay_capture_valued): the same rows and frames; a completed row's mass comes from the actor's one-step TD
// errors - k_dqn_targets' float32 arithmetic on (prev_q, this lock-step's maxima) - instead of the running maximum, which
// stays the fallback for a non-finite error and is raised by one wave reduction (an arena is one wave: no atomics).
template <bool VALUED>
__global__ __launch_bounds__(256) void k_replay_capture(CaptureParams p) {
  const int a = blockIdx.x * OFX_ARENAS_PER_BLOCK + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (a >= p.N) return;  // wave-uniform
  const int t = a * p.M + lane;
  const bool ship = lane < p.M && (!p.mask || p.mask[t]);
  const bool plays = ship && !p.r.latched[t];
  float hd[8];
  int done = 0, reward = 0;
  if (plays) {
    reward = p.st.reward[t];  // obs.reward
    done = p.st.alive[t] ? 0 : 1;
    ofx_obs_head(p.st, t, p.W, p.H, hd);  // the head the live forward feeds
    // the row's reward (and the valued form's targets) may come from a span's sum; hd[0] stays the state's reward
    if (p.r.reward_src) reward = p.r.reward_src[t];
  }
  // the arena keeps this lock-step's maps iff one of its agents plays (k_replay_frames copies them afterwards)
  int slot = -1;
  if (__ballot(plays)) {
    slot = p.r.frame_head[a];
    if (lane == 0) {
      p.r.frame_head[a] = (slot + 1) % p.F;
      p.r.frame_tick[(size_t)a * p.F + slot] = p.tick;
    }
  }
  if (lane == 0) p.r.cur_slot[a] = slot;
  const bool trans = plays && p.r.has_prev[t];
  const unsigned long long bal = __ballot(trans);
  const int n_new = __popcll(bal);
  const int pos = __popcll(bal & ((1ull << lane) - 1ull));
  const int head = p.r.head[a];
  const float mm = VALUED ? p.r.mmax[a] : 0.f;  // as read before this lock-step's raises
  float raised = 0.f;                           // masses are >= 0
  if (trans) {
    ofx_transition row;
    row.tick_prev = p.r.prev_tick[t];
    row.tick_next = p.tick;
    row.frame_prev = p.r.prev_slot[t];
    row.frame_next = slot;
    row.ship = lane;
    row.iaction = p.r.prev_iaction[t];
    row.px = p.r.prev_px[t];
    row.py = p.r.prev_py[t];
    row.reward = reward;
    row.done = done;
#pragma unroll
    for (int k = 0; k < 8; k++) { row.head_prev[k] = p.r.prev_head[(size_t)t * 8 + k]; row.head_next[k] = hd[k]; }
    p.r.rows[(size_t)a * p.C + (head + pos) % p.C] = row;
    if (VALUED) {
      float y1 = (float)reward, y2 = (float)reward;  // a done row never reads v_*
      if (!done) {
        y1 = (float)reward + p.r.actor_gamma * p.v_act[t];
        y2 = (float)reward + p.r.actor_gamma * p.v_ptr[t];
      }
      const float e1 = p.r.prev_q[2 * (size_t)t] - y1, e2 = p.r.prev_q[2 * (size_t)t + 1] - y2;
      float m = mm;
      if (isfinite(e1) && isfinite(e2)) raised = m = per_mass(e1, e2, p.r.eps, p.r.alpha);
      p.r.mass[(size_t)a * p.C + (head + pos) % p.C] = m;
    } else if (p.r.mass) {
      p.r.mass[(size_t)a * p.C + (head + pos) % p.C] = p.r.mmax[a];  // PER: a new row gets the running max
    }
  }
  if (VALUED) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) raised = fmaxf(raised, __shfl_xor(raised, o));
  }
  if (plays) {
    if (done) p.r.latched[t] = 1;
    p.r.has_prev[t] = 1;
    p.r.prev_tick[t] = p.tick;
    p.r.prev_slot[t] = slot;
    p.r.prev_iaction[t] = p.iaction[t];
    p.r.prev_px[t] = p.ipointer[2 * t];
    p.r.prev_py[t] = p.ipointer[2 * t + 1];
#pragma unroll
    for (int k = 0; k < 8; k++) p.r.prev_head[(size_t)t * 8 + k] = hd[k];
    if (VALUED) {
      p.r.prev_q[2 * (size_t)t] = p.q_sa[t];
      p.r.prev_q[2 * (size_t)t + 1] = p.p_sp[t];
    }
  }
  if (lane == 0 && n_new) {
    if (VALUED) p.r.mmax[a] = fmaxf(mm, raised);
    p.r.head[a] = (head + n_new) % p.C;
    p.r.count[a] = min(p.r.count[a] + n_new, p.C);
    p.r.appended[a] += n_new;
  }
}

// copies the current 1-bit maps of every arena that stores a frame this lock-step into its ring slot
__global__ __launch_bounds__(256) void k_replay_frames(int N, int F, int words, const uint32_t *ship_bits,
                                                       const uint32_t *laser_bits, ofx_replay r) {
  const int a = blockIdx.x;
  const int slot = r.cur_slot[a];
  if (slot < 0) return;  // block-uniform
  uint4 *dst = reinterpret_cast<uint4 *>(r.frame_bits + ((size_t)a * F + slot) * 2 * words);
  const uint4 *s0 = reinterpret_cast<const uint4 *>(ship_bits + (size_t)a * words);
  const uint4 *s1 = reinterpret_cast<const uint4 *>(laser_bits + (size_t)a * words);
  const int q = words / 4;
  for (int k = threadIdx.x; k < q; k += 256) { dst[k] = s0[k]; dst[q + k] = s1[k]; }
}

// Where a lane's nonzero words go when a wave packs 64 uint4s (w: the lane's four words) in ascending word order, which
// is lane-major, then component: returns *run + the nonzero words of all four components in the lanes below; the lane's
// own nonzero words follow from there.  *run moves past the wave's.  Every lane of the wave must call it.
template <typename T>
__device__ __forceinline__ T nonzero_place(const uint32_t w[4], int lane, T *run) {
  const unsigned long long below = (1ull << lane) - 1ull;
  T pos = *run;
#pragma unroll
  for (int c = 0; c < 4; c++) {
    const unsigned long long bal = __ballot(w[c] != 0u);
    pos += (T)__popcll(bal & below);
    *run += (T)__popcll(bal);
  }
  return pos;
}

// The packed form of k_replay_frames: one workgroup per arena that stores a frame, four waves.  A map is q = words / 4
// uint4s = P = ceil(q / 64) passes of 64 lanes; wave w takes the passes [w * per, (w + 1) * per) of BOTH maps, so within a
// map the waves' pairs follow each other in wave order.  Count pass (ballots of the nonzero components), the waves' counts
// through LDS, lane 0 runs steps 1 and 2 of the storing rule (include/ofx.h) and publishes the base, then the write pass
// repeats the walk: a lane's position is its wave's base + the nonzero words in the lanes and components below it.
// k_replay_capture has already written frame_tick of the new slot s: step 1 reads the slot's old counts (0 unless it
// held a live frame) and the eviction walk covers the F - 1 other slots only.
__global__ __launch_bounds__(256) void k_replay_frames_packed(int N, int F, int words, const uint32_t *ship_bits,
                                                              const uint32_t *laser_bits, ofx_replay r) {
  __shared__ uint32_t wcnt[2][4];
  __shared__ uint32_t base_s;
  const int a = blockIdx.x;
  const int s = r.cur_slot[a];
  if (s < 0) return;  // block-uniform
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const uint4 *src[2] = {reinterpret_cast<const uint4 *>(ship_bits + (size_t)a * words),
                         reinterpret_cast<const uint4 *>(laser_bits + (size_t)a * words)};
  const int q = words >> 2, P = (q + 63) >> 6, per = (P + 3) >> 2;
  const int p0 = min(wave * per, P), p1 = min(p0 + per, P);  // wave-uniform
  for (int m = 0; m < 2; m++) {
    uint32_t run = 0;
    for (int pass = p0; pass < p1; pass++) {  // wave-uniform trip count: the ballots see every lane
      const int k = pass * 64 + lane;
      uint4 v = make_uint4(0u, 0u, 0u, 0u);
      if (k < q) v = src[m][k];
      const uint32_t w4[4] = {v.x, v.y, v.z, v.w};
      (void)nonzero_place(w4, lane, &run);
    }
    if (lane == 0) wcnt[m][wave] = run;
  }
  __syncthreads();
  const uint32_t k_ship = wcnt[0][0] + wcnt[0][1] + wcnt[0][2] + wcnt[0][3];
  const uint32_t k_laser = wcnt[1][0] + wcnt[1][1] + wcnt[1][2] + wcnt[1][3];
  const uint32_t pool_pairs = r.pool_pairs;
  if (threadIdx.x == 0) {
    const uint32_t k = k_ship + k_laser;  // <= 2 * words <= pool_pairs / 2
    uint32_t *cnt = r.frame_cnt + (size_t)a * F * 2;
    int32_t *tick = r.frame_tick + (size_t)a * F;
    uint32_t live = r.live[a] - (cnt[2 * s] + cnt[2 * s + 1]);  // step 1: the slot ring has wrapped onto its oldest frame
    long long ev = 0;
    for (int i = 1, j = s + 1; i < F && live + k > pool_pairs; i++, j++) {  // step 2: early eviction, oldest first
      if (j >= F) j -= F;
      if (tick[j] < 0) continue;
      live -= cnt[2 * j] + cnt[2 * j + 1];
      tick[j] = -1;
      cnt[2 * j] = 0u;
      cnt[2 * j + 1] = 0u;
      ev++;
    }
    const uint32_t head = r.pool_head[a];
    r.frame_off[(size_t)a * F + s] = head;  // step 3
    cnt[2 * s] = k_ship;
    cnt[2 * s + 1] = k_laser;
    r.pool_head[a] = (head + k) % pool_pairs;
    r.live[a] = live + k;
    if (ev) r.evicted[a] += ev;
    base_s = head;
  }
  __syncthreads();
  uint2 *pool = r.pool + (size_t)a * pool_pairs;
  for (int m = 0; m < 2; m++) {
    uint32_t run = base_s + (m ? k_ship : 0u);
    for (int w = 0; w < wave; w++) run += wcnt[m][w];
    for (int pass = p0; pass < p1; pass++) {
      const int k = pass * 64 + lane;
      uint4 v = make_uint4(0u, 0u, 0u, 0u);
      if (k < q) v = src[m][k];
      const uint32_t w4[4] = {v.x, v.y, v.z, v.w};
      uint32_t pos = nonzero_place(w4, lane, &run);
#pragma unroll
      for (int c = 0; c < 4; c++)
        if (w4[c] != 0u) {  // base < pool_pairs and at most 2 * words pairs follow it: one wrap at the most, then < pool_pairs
          const uint32_t at = pos >= pool_pairs ? pos - pool_pairs : pos;
          pool[at] = make_uint2((uint32_t)(4 * k + c), w4[c]);
          pos++;
        }
    }
  }
}

// ofx_replay_capture (q_sa null) and ofx_replay_capture_valued (the four value arrays given)
static int replay_capture(ofx_handle *h, const char *who, uint32_t tick, const uint8_t *ship_mask, const int32_t *iaction,
                          const int32_t *ipointer, const float *q_sa, const float *p_sp, const float *v_act,
                          const float *v_ptr) {
  ofx_replay *r = h->replay;
  if (!h->spawned) { ofx_set_error("You must execute analyse_battleground first."); return OFX_ERR_STATE; }
  if ((int32_t)tick < 0) { ofx_set_error("%s: tick must be < 2^31", who); return OFX_ERR_INVALID; }
  if (h->cfg.n_ships > OFX_WAVE) { ofx_set_error("%s: n_ships > 64", who); return OFX_ERR_INVALID; }
  OFX_HIP(hipSetDevice(h->cfg.device));
  int rc;
  int32_t *ria, *rip;  // null = the handle's results
  if ((rc = ofx_policy_results(h, &ria, &rip))) return rc;
  if (!iaction) iaction = ria;
  if (!ipointer) ipointer = rip;
  // the observation maps of this lock-step (the same 1-bit maps the policy trunk reads)
  if ((rc = ofx_launch_raster(h, OFX_MAP_BITS_LSB, nullptr, nullptr))) return rc;
  CaptureParams p;
  p.N = h->cfg.n_arenas; p.M = h->cfg.n_ships; p.W = h->cfg.width; p.H = h->cfg.height; p.C = r->capacity;
  p.F = r->frames;
  p.tick = (int)tick; p.st = h->st; p.mask = ship_mask; p.iaction = iaction; p.ipointer = ipointer; p.r = *r;
  p.q_sa = q_sa; p.p_sp = p_sp; p.v_act = v_act; p.v_ptr = v_ptr;
  if (q_sa) hipLaunchKernelGGL(k_replay_capture<true>, dim3(arena_blocks(p.N)), dim3(256), 0, h->stream, p);
  else hipLaunchKernelGGL(k_replay_capture<false>, dim3(arena_blocks(p.N)), dim3(256), 0, h->stream, p);
  OFX_HIP(hipGetLastError());
  if (r->packed)
    hipLaunchKernelGGL(k_replay_frames_packed, dim3((unsigned)p.N), dim3(256), 0, h->stream, p.N, r->frames, r->words,
                       (const uint32_t *)h->maps[OFX_MAP_BITS_LSB][0], (const uint32_t *)h->maps[OFX_MAP_BITS_LSB][1], *r);
  else
    hipLaunchKernelGGL(k_replay_frames, dim3((unsigned)p.N), dim3(256), 0, h->stream, p.N, r->frames, r->words,
                       (const uint32_t *)h->maps[OFX_MAP_BITS_LSB][0], (const uint32_t *)h->maps[OFX_MAP_BITS_LSB][1], *r);
  OFX_HIP(hipGetLastError());
  return OFX_OK;
}

extern "C" int ofx_replay_capture(ofx_handle *h, uint32_t tick, const uint8_t *ship_mask, const int32_t *iaction,
                                  const int32_t *ipointer) {
  if (!h) { ofx_set_error("ofx_replay_capture: null handle"); return OFX_ERR_INVALID; }
  if (!h->replay) { ofx_set_error("ofx_replay_capture before ofx_replay_create"); return OFX_ERR_STATE; }
  return replay_capture(h, "ofx_replay_capture", tick, ship_mask, iaction, ipointer, nullptr, nullptr, nullptr, nullptr);
}

extern "C" int ofx_replay_reward_source(ofx_handle *h, const int32_t *reward) {
  if (!h) { ofx_set_error("ofx_replay_reward_source: null handle"); return OFX_ERR_INVALID; }
  if (!h->replay) { ofx_set_error("ofx_replay_reward_source before ofx_replay_create"); return OFX_ERR_STATE; }
  h->replay->reward_src = reward;  // read by the captures enqueued from now on
  return OFX_OK;
}

// first-seen deaths of the selected ships (QlearnIA.play's done latch, agents/qlearnIA_V2.py:376-384)
__global__ void k_first_done(int n, const uint8_t *alive, const uint8_t *mask, uint8_t *seen, int *count) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  bool first = false;
  if (i < n && alive[i] == 0 && (!mask || mask[i]) && !seen[i]) {
    seen[i] = 1;
    first = true;
  }
  const unsigned long long b = __builtin_amdgcn_ballot_w64(first);
  if ((threadIdx.x & 63) == 0 && b) atomicAdd(count, __popcll(b));
}

extern "C" int ofx_agents_first_done(ofx_handle *h, const uint8_t *ship_mask, uint8_t *seen, int32_t *count_host) {
  if (!h || !seen || !count_host) { ofx_set_error("ofx_agents_first_done: null argument"); return OFX_ERR_INVALID; }
  if (!h->spawned) { ofx_set_error("ofx_agents_first_done before ofx_spawn"); return OFX_ERR_STATE; }
  OFX_HIP(hipSetDevice(h->cfg.device));
  int32_t *cnt;
  int rc = ofx_counter(h, OFX_COUNTER_FIRST_DONE, &cnt);
  if (rc) return rc;
  OFX_HIP(hipMemsetAsync(cnt, 0, sizeof(int), h->stream));
  const int n = h->cfg.n_arenas * h->cfg.n_ships;
  hipLaunchKernelGGL(k_first_done, dim3((n + 255) / 256), dim3(256), 0, h->stream, n, h->st.alive, ship_mask, seen, cnt);
  OFX_HIP(hipGetLastError());
  OFX_HIP(hipMemcpyAsync(count_host, cnt, sizeof(int), hipMemcpyDeviceToHost, h->stream));
  OFX_HIP(hipStreamSynchronize(h->stream));
  return OFX_OK;
}

extern "C" int ofx_replay_count(ofx_handle *h, int32_t *count_host, int64_t *appended_host) {
  if (!h || !h->replay) { ofx_set_error("ofx_replay_count: no replay memory"); return OFX_ERR_STATE; }
  OFX_HIP(hipSetDevice(h->cfg.device));
  OFX_HIP(hipStreamSynchronize(h->stream));
  const size_t N = h->cfg.n_arenas;
  if (count_host) OFX_HIP(hipMemcpy(count_host, h->replay->count, sizeof(int32_t) * N, hipMemcpyDeviceToHost));
  if (appended_host) OFX_HIP(hipMemcpy(appended_host, h->replay->appended, sizeof(int64_t) * N, hipMemcpyDeviceToHost));
  return OFX_OK;
}

// one arena's part of a ring array (rows or mass, `size` bytes per position) to the host, oldest first; synchronises
static int ring_to_host(ofx_handle *h, int32_t arena, const void *array, size_t size, void *dst_host, int32_t *n_host) {
  ofx_replay *r = h->replay;
  OFX_HIP(hipSetDevice(h->cfg.device));
  OFX_HIP(hipStreamSynchronize(h->stream));
  int32_t head, count;
  OFX_HIP(hipMemcpy(&head, r->head + arena, 4, hipMemcpyDeviceToHost));
  OFX_HIP(hipMemcpy(&count, r->count + arena, 4, hipMemcpyDeviceToHost));
  const RowRing ring = row_ring(r->capacity, head, count);
  const uint8_t *base = (const uint8_t *)array + size * (size_t)arena * ring.C;
  const int n1 = min(count, ring.C - ring.first);  // the rows up to the ring's end, then the ones that wrapped
  if (n1 > 0) OFX_HIP(hipMemcpy(dst_host, base + size * ring.first, size * n1, hipMemcpyDeviceToHost));
  if (count > n1) OFX_HIP(hipMemcpy((uint8_t *)dst_host + size * n1, base, size * (count - n1), hipMemcpyDeviceToHost));
  *n_host = count;
  return OFX_OK;
}

// rows of one arena, oldest first (list(memory))
extern "C" int ofx_replay_rows_host(ofx_handle *h, int32_t arena, ofx_transition *rows_host, int32_t *n_host) {
  if (!h || !h->replay || !rows_host || !n_host) { ofx_set_error("ofx_replay_rows_host: bad argument"); return OFX_ERR_INVALID; }
  if (arena < 0 || arena >= h->cfg.n_arenas) { ofx_set_error("ofx_replay_rows_host: arena out of range"); return OFX_ERR_INVALID; }
  return ring_to_host(h, arena, h->replay->rows, sizeof(ofx_transition), rows_host, n_host);
}

// ---- the one reader of a stored frame: slot `slot` of arena a -> out[2][words] (16-byte aligned), every word written ----
// Dense: the 16-byte copy.  Packed: the workgroup (256 threads, all of them must call) builds the two maps in LDS - zero,
// barrier, scatter the slot's pairs, barrier - and streams them out with 16-byte stores; the launch gives 8 * words bytes
// of dynamic LDS.  A slot without a live frame has counts 0 and reads as two empty maps.
template <bool PACKED>
__device__ __forceinline__ void frame_read(const ofx_replay &r, int a, int F, int words, int slot, uint32_t *out) {
  uint4 *out4 = reinterpret_cast<uint4 *>(out);
  const int n4 = 2 * words / 4;
  if constexpr (!PACKED) {
    const uint4 *in = reinterpret_cast<const uint4 *>(r.frame_bits + ((size_t)a * F + slot) * 2 * words);
    for (int k = threadIdx.x; k < n4; k += 256) out4[k] = in[k];
  } else {
    extern __shared__ uint4 frame_lds[];
    uint32_t *lds = reinterpret_cast<uint32_t *>(frame_lds);
    for (int k = threadIdx.x; k < n4; k += 256) frame_lds[k] = make_uint4(0u, 0u, 0u, 0u);
    const size_t fs = (size_t)a * F + slot;
    const uint32_t c0 = r.frame_cnt[2 * fs], n = c0 + r.frame_cnt[2 * fs + 1], off = r.frame_off[fs];
    const uint32_t pool_pairs = r.pool_pairs;
    const uint2 *pool = r.pool + (size_t)a * pool_pairs;
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < n; i += 256) {
      uint32_t at = off + i;  // off < pool_pairs, i < 2 * words <= pool_pairs / 2
      if (at >= pool_pairs) at -= pool_pairs;
      const uint2 pr = pool[at];
      if (pr.x < (uint32_t)words) lds[(i < c0 ? 0u : (uint32_t)words) + pr.x] = pr.y;
    }
    __syncthreads();
    for (int k = threadIdx.x; k < n4; k += 256) out4[k] = frame_lds[k];
    __syncthreads();  // the next frame_read of this workgroup zeroes the LDS again
  }
}

// ofx_replay_frame_host on a packed memory: the frame through frame_read into a device buffer
__global__ __launch_bounds__(256) void k_replay_frame_read(int a, int F, int words, int slot, ofx_replay r, uint32_t *out) {
  frame_read<true>(r, a, F, words, slot, out);
}

// the 1-bit maps of one stored lock-step of one arena (pixel p -> bit (p & 7) of byte p >> 3, i.e.
// numpy.unpackbits(..., bitorder='little')); OFX_ERR_STATE when the frame has left the ring
extern "C" int ofx_replay_frame_host(ofx_handle *h, int32_t arena, int32_t tick, void *ship_bits_host,
                                     void *laser_bits_host) {
  if (!h || !h->replay || !ship_bits_host || !laser_bits_host) { ofx_set_error("ofx_replay_frame_host: bad argument"); return OFX_ERR_INVALID; }
  if (arena < 0 || arena >= h->cfg.n_arenas || tick < 0) { ofx_set_error("ofx_replay_frame_host: out of range"); return OFX_ERR_INVALID; }
  ofx_replay *r = h->replay;
  OFX_HIP(hipSetDevice(h->cfg.device));
  OFX_HIP(hipStreamSynchronize(h->stream));
  int32_t *ticks = (int32_t *)malloc(sizeof(int32_t) * r->frames);
  if (!ticks) { ofx_set_error("ofx_replay_frame_host: out of host memory"); return OFX_ERR_INVALID; }
  hipError_t e = hipMemcpy(ticks, r->frame_tick + (size_t)arena * r->frames, sizeof(int32_t) * r->frames, hipMemcpyDeviceToHost);
  int f = -1;
  for (int i = 0; e == hipSuccess && i < r->frames; i++) if (ticks[i] == tick) f = i;
  free(ticks);
  OFX_HIP(e);
  if (f < 0) { ofx_set_error("ofx_replay_frame_host: lock-step %d is not in the frame ring of arena %d", tick, arena); return OFX_ERR_STATE; }
  const size_t wb = (size_t)r->words * 4;
  const uint32_t *slot;
  if (r->packed) {
    int rc;
    if ((rc = ofx_ensure_scratch(h, 2 * wb))) return rc;
    hipLaunchKernelGGL(k_replay_frame_read, dim3(1), dim3(256), 2 * wb, h->stream, arena, r->frames, r->words, f, *r,
                       (uint32_t *)h->scratch);
    OFX_HIP(hipGetLastError());
    OFX_HIP(hipStreamSynchronize(h->stream));
    slot = (const uint32_t *)h->scratch;
  } else {
    slot = r->frame_bits + ((size_t)arena * r->frames + f) * 2 * r->words;
  }
  OFX_HIP(hipMemcpy(ship_bits_host, slot, wb, hipMemcpyDeviceToHost));
  OFX_HIP(hipMemcpy(laser_bits_host, slot + r->words, wb, hipMemcpyDeviceToHost));
  return OFX_OK;
}

// ---- minibatch: random.sample(memory, min(batch, len(memory))) per arena (qlearnIA_V2.py:241-243) ----------------
// Floyd's subset sampling (uniform over the subsets, no replacement) on Philox draws: counter (global arena, j,
// draw, OFX_STREAM_REPLAY).  Transitions whose `state` frame has already left the arena's frame ring are not eligible (only
// possible when the ring is shorter than the rows need: C rows in runs of consecutive plays use C + #runs frames).  slot[a][j] indexes the arena's rows oldest-first, -1 pads.

// Eligibility: row o of arena a can be sampled while its `state` frame is still in the frame ring, i.e. the slot it
// names still holds its lock-step.  Rows are chronological, so the expired ones are an arena's oldest.
__device__ __forceinline__ bool state_frame_live(const ofx_replay &r, int a, int F, const ofx_transition &o) {
  const int f = o.frame_prev;
  return (unsigned)f < (unsigned)F && r.frame_tick[(size_t)a * F + f] == o.tick_prev;
}

// The expired oldest rows of arena a, counted by its wave: 64 rows per ballot, the first live one ends the walk.  A frame
// ring as long as the rows need expires nothing, so the oldest row is tried first, by all lanes at one address: the
// usual arena then costs one cache line, not the 64 of a ballot round.
__device__ __forceinline__ int expired_rows_wave(const ofx_replay &r, int a, int F, const RowRing &ring, int lane) {
  const ofx_transition *rows = r.rows + (size_t)a * ring.C;
  if (ring.count && state_frame_live(r, a, F, rows[ring.at(0)])) return 0;  // wave-uniform
  for (int base = 0; base < ring.count; base += 64) {  // wave-uniform trip count
    const int i = base + lane;
    const unsigned long long hit = __ballot(i < ring.count && state_frame_live(r, a, F, rows[ring.at(i)]));
    if (hit) return base + __ffsll((long long)hit) - 1;
  }
  return ring.count;
}

__global__ void k_replay_sample(int N, int C, int F, int batch, int arena_base, ofx_rng_key key, uint32_t draw,
                                ofx_replay r, int32_t *slot, int32_t *n_out) {
  const int a = blockIdx.x * blockDim.x + threadIdx.x;
  if (a >= N) return;
  const RowRing ring = row_ring(C, r.head[a], r.count[a]);
  const ofx_transition *rows = r.rows + (size_t)a * C;
  int skip = 0;  // one thread per arena: the serial walk
  while (skip < ring.count && !state_frame_live(r, a, F, rows[ring.at(skip)])) skip++;
  const int valid = ring.count - skip, n = min(batch, valid);
  int32_t *out = slot + (size_t)a * batch;
  for (int j = 0; j < n; j++) {
    const int top = valid - n + j;  // draw t in [0, top]
    uint32_t rr[4];
    ofx_philox4x32_10((uint32_t)(arena_base + a), (uint32_t)j, draw, OFX_STREAM_REPLAY, key, rr);
    int tsel = ofx_draw_int(rr[0], top);
    for (int q = 0; q < j; q++) if (out[q] == skip + tsel) { tsel = top; break; }
    out[j] = skip + tsel;
  }
  for (int j = n; j < batch; j++) out[j] = -1;
  if (n_out) n_out[a] = n;
}

extern "C" int ofx_replay_sample(ofx_handle *h, uint64_t seed, uint32_t draw, int32_t batch, int32_t *slot,
                                 int32_t *n_sampled) {
  if (!h || !h->replay || !slot || batch <= 0) { ofx_set_error("ofx_replay_sample: bad argument"); return OFX_ERR_INVALID; }
  ofx_replay *r = h->replay;
  OFX_HIP(hipSetDevice(h->cfg.device));
  const int N = h->cfg.n_arenas;
  hipLaunchKernelGGL(k_replay_sample, dim3((N + 63) / 64), dim3(64), 0, h->stream, N, r->capacity, r->frames, batch,
                     h->cfg.arena_base, ofx_key(seed), draw, *r, slot, n_sampled);
  OFX_HIP(hipGetLastError());
  return OFX_OK;
}

// ---- gather a sampled minibatch into dense tensors (the arrays Trainer.replay builds, qlearnIA_V2.py:246-283) -------
struct GatherParams {
  int N, C, F, batch, words;
  ofx_replay r;
  const int32_t *slot;
  ofx_transition *rows;      // [N][batch]
  uint32_t *bits_prev, *bits_next;  // [N][batch][2][words] or null
};
static GatherParams gather_params(ofx_handle *h, const int32_t *slot, int32_t batch, ofx_transition *rows, void *bits_prev,
                                  void *bits_next) {
  const ofx_replay *r = h->replay;
  return GatherParams{h->cfg.n_arenas, r->capacity, r->frames, batch, r->words, *r, slot, rows, (uint32_t *)bits_prev,
                      (uint32_t *)bits_next};
}

// n-step returns (ofx_replay_gather_nstep; include/ofx.h states the contract): chain length, discount and outputs
struct NstepParams {
  int nstep;
  double gamma;
  float *ret, *disc;  // [max_rows]
};

// The padding row of a gather (P: GatherParams or GatherListParams) at destination d: an all-zero row with ship = -1 and
// empty maps (never uninitialised memory); NSTEP: ret = disc = 0 as well.  The whole workgroup calls it.
template <bool NSTEP, typename P>
__device__ __forceinline__ void gather_pad_row(const P &p, size_t d, const NstepParams &q) {
  if (threadIdx.x < sizeof(ofx_transition) / 4) ((int32_t *)(p.rows + d))[threadIdx.x] = threadIdx.x == 4 ? -1 : 0;
  uint32_t *pads[2] = {p.bits_prev, p.bits_next};
  for (int w = 0; w < 2; w++) {
    if (!pads[w]) continue;
    uint4 *out = reinterpret_cast<uint4 *>(pads[w] + d * 2 * p.words);
    for (int k = threadIdx.x; k < 2 * p.words / 4; k += 256) out[k] = make_uint4(0u, 0u, 0u, 0u);
  }
  if (NSTEP && threadIdx.x == 0) { q.ret[d] = 0.f; q.disc[d] = 0.f; }
}

// exclusive scan of n_sampled[N] by one workgroup -> off[N], total in off[N] (int32 for the gathers' windows, 64-bit
// sums for the checkpoint's pair offsets)
template <typename In, typename Out>
__global__ __launch_bounds__(1024) void k_replay_scan(int N, const In *n_sampled, Out *off) {
  __shared__ Out part[1024];
  const int tid = threadIdx.x, per = (N + 1023) / 1024, lo = min(tid * per, N), hi = min(lo + per, N);
  Out sum = 0;
  for (int i = lo; i < hi; i++) sum += n_sampled[i];
  part[tid] = sum;
  __syncthreads();
  for (int d = 1; d < 1024; d <<= 1) {  // Hillis-Steele inclusive scan of the partial sums
    const Out v = tid >= d ? part[tid - d] : 0;
    __syncthreads();
    part[tid] += v;
    __syncthreads();
  }
  Out run = tid ? part[tid - 1] : 0;
  for (int i = lo; i < hi; i++) { off[i] = run; run += n_sampled[i]; }
  if (tid == 1023) off[N] = part[1023];
}

// Wave 0 of the workgroup: the n-step chain from oldest-first row s.  Per step the 64 lanes test 64 consecutive rows
// after the current one; the lowest row of the same ship is the ship's next row in append order, and it is the
// successor iff its tick_prev is the current row's tick_next (a ship's tick_prev values increase strictly; a restart
// in between leaves a gap).  Lane 0 writes ret / disc; returns the oldest-first index of the chain's last row.
__device__ int nstep_chain(const ofx_transition *rows, const RowRing &ring, int s, int lane, int d, const NstepParams &q) {
  int cur = s, L = 0;
  double acc = 0.0, pw = 1.0;
  for (;;) {
    const ofx_transition *r = rows + ring.at(cur);
    const int done = r->done, ship = r->ship, tick = r->tick_next;
    acc += pw * (double)r->reward;  // -ffp-contract=off: the product and the sum round on their own
    pw *= q.gamma;
    if (done || ++L == q.nstep) break;
    int next = -1;
    for (int base = cur + 1; base < ring.count; base += 64) {  // wave-uniform trip count
      const int i = base + lane;
      bool same = false;
      int tp = 0;
      if (i < ring.count) {
        const ofx_transition *c = rows + ring.at(i);
        same = c->ship == ship;
        tp = c->tick_prev;
      }
      const unsigned long long hit = __ballot(same);
      if (hit) {
        const int l = __ffsll((long long)hit) - 1;
        if (__shfl(tp, l) == tick) next = base + l;
        break;
      }
    }
    if (next < 0) break;  // restart (the ship's next row does not chain) or ring head (no next row yet)
    cur = next;
  }
  if (lane == 0) {
    q.ret[d] = (float)acc;
    q.disc[d] = rows[ring.at(cur)].done ? 0.f : (float)pw;
  }
  return cur;
}

// One gathered row (P: GatherParams or GatherListParams), by the whole workgroup: oldest-first row s of arena a, which
// holds count rows, becomes row d of the output with its two frames' maps.  NSTEP: the row is the composite of the
// n-step chain from it (wave 0 walks the chain first; one LDS word carries its end to the other waves).
template <bool NSTEP, bool PACKED, typename P>
__device__ __forceinline__ void gather_row(const P &p, int a, int s, int count, int d, const NstepParams &q) {
  const RowRing ring = row_ring(p.C, p.r.head[a], count);
  const ofx_transition *rows = p.r.rows + (size_t)a * p.C;
  const ofx_transition *src = rows + ring.at(s);
  const ofx_transition *end = src;  // the row whose next state is gathered
  if constexpr (NSTEP) {
    __shared__ int end_s;
    if (threadIdx.x < 64) {
      const int e = nstep_chain(rows, ring, s, threadIdx.x, d, q);
      if (threadIdx.x == 0) end_s = e;
    }
    __syncthreads();
    end = rows + ring.at(end_s);
  }
  ofx_transition *dst = p.rows + d;
  if (threadIdx.x < sizeof(ofx_transition) / 4) {
    const int w = threadIdx.x;  // tick_next, frame_next, done and head_next come from the chain's last row
    const bool from_end = w == 1 || w == 3 || w == 9 || w >= (int)(offsetof(ofx_transition, head_next) / 4);
    ((int32_t *)dst)[w] = ((const int32_t *)(from_end ? end : src))[w];
  }
  const int slots[2] = {src->frame_prev, end->frame_next};
  uint32_t *outs[2] = {p.bits_prev, p.bits_next};
  for (int w = 0; w < 2; w++) {
    if (!outs[w]) continue;  // block-uniform
    frame_read<PACKED>(p.r, a, p.F, p.words, slots[w], outs[w] + (size_t)d * 2 * p.words);
  }
}

// ofx_replay_gather: one workgroup per (arena, j), row a * batch + j of the padded output
template <bool PACKED>
__global__ __launch_bounds__(256) void k_replay_gather(GatherParams p) {
  const int a = blockIdx.x / p.batch;
  const int s = p.slot[blockIdx.x];
  if (s < 0) gather_pad_row<false>(p, (size_t)blockIdx.x, NstepParams{});  // block-uniform
  else gather_row<false, PACKED>(p, a, s, p.r.count[a], (int)blockIdx.x, NstepParams{});
}

extern "C" int ofx_replay_gather(ofx_handle *h, const int32_t *slot, int32_t batch, ofx_transition *rows,
                                 void *bits_prev, void *bits_next) {
  if (!h || !h->replay || !slot || !rows || batch <= 0) { ofx_set_error("ofx_replay_gather: bad argument"); return OFX_ERR_INVALID; }
  ofx_replay *r = h->replay;
  OFX_HIP(hipSetDevice(h->cfg.device));
  const GatherParams p = gather_params(h, slot, batch, rows, bits_prev, bits_next);
  if (r->packed)
    hipLaunchKernelGGL(k_replay_gather<true>, dim3((unsigned)(p.N * batch)), dim3(256), (size_t)r->words * 8, h->stream, p);
  else
    hipLaunchKernelGGL(k_replay_gather<false>, dim3((unsigned)(p.N * batch)), dim3(256), 0, h->stream, p);
  OFX_HIP(hipGetLastError());
  return OFX_OK;
}

// ---- the same minibatch without padding: only the rows that exist, packed (Trainer.replay never pads: its batch is
// min(batch_size, len(memory)) real transitions, qlearnIA_V2.py:241-243) ------------------------------------------------
// one workgroup per (arena, j): sampled entry j of arena a is packed row off[a] + j - first, when it falls into
// [0, max_rows)
template <bool NSTEP, bool PACKED>
__global__ __launch_bounds__(256) void k_replay_gather_valid(GatherParams p, const int32_t *n_sampled, const int32_t *off, int first,
                                                             int max_rows, NstepParams q) {
  const int a = blockIdx.x / p.batch, j = blockIdx.x - a * p.batch;
  if (j >= n_sampled[a]) return;
  const int d = off[a] + j - first;
  if (d < 0 || d >= max_rows) return;
  gather_row<NSTEP, PACKED>(p, a, p.slot[(size_t)a * p.batch + j], p.r.count[a], d, q);
}

// ofx_replay_gather_valid (q == null) and ofx_replay_gather_nstep: the same window, scan and synchronisation
static int gather_window(ofx_handle *h, const char *who, const int32_t *slot, const int32_t *n_sampled, int32_t batch,
                         int32_t first, int32_t max_rows, ofx_transition *rows, void *bits_prev, void *bits_next,
                         int32_t *n_rows_host, const NstepParams *q) {
  if (!h || !h->replay || !slot || !n_sampled || !rows || !n_rows_host || batch <= 0 || first < 0 || max_rows <= 0) {
    ofx_set_error("%s: bad argument", who);
    return OFX_ERR_INVALID;
  }
  ofx_replay *r = h->replay;
  OFX_HIP(hipSetDevice(h->cfg.device));
  const int N = h->cfg.n_arenas;
  int32_t *off = r->scan_off;
  hipLaunchKernelGGL((k_replay_scan<int32_t, int32_t>), dim3(1), dim3(1024), 0, h->stream, N, n_sampled, off);
  const GatherParams p = gather_params(h, slot, batch, rows, bits_prev, bits_next);
  const dim3 grid((unsigned)(N * batch));
  const size_t lds = (size_t)r->words * 8;  // packed: the two maps of a frame
  if (q && r->packed)
    hipLaunchKernelGGL((k_replay_gather_valid<true, true>), grid, dim3(256), lds, h->stream, p, n_sampled,
                       (const int32_t *)off, first, max_rows, *q);
  else if (q)
    hipLaunchKernelGGL((k_replay_gather_valid<true, false>), grid, dim3(256), 0, h->stream, p, n_sampled,
                       (const int32_t *)off, first, max_rows, *q);
  else if (r->packed)
    hipLaunchKernelGGL((k_replay_gather_valid<false, true>), grid, dim3(256), lds, h->stream, p, n_sampled,
                       (const int32_t *)off, first, max_rows, NstepParams{});
  else
    hipLaunchKernelGGL((k_replay_gather_valid<false, false>), grid, dim3(256), 0, h->stream, p, n_sampled,
                       (const int32_t *)off, first, max_rows, NstepParams{});
  hipError_t e = hipGetLastError();
  int32_t total = 0;
  if (e == hipSuccess) e = hipMemcpyAsync(&total, off + N, sizeof(total), hipMemcpyDeviceToHost, h->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
  if (e != hipSuccess) { ofx_set_error("%s: %s", who, hipGetErrorString(e)); return OFX_ERR_HIP; }
  *n_rows_host = total - first < 0 ? 0 : (total - first > max_rows ? max_rows : total - first);
  return OFX_OK;
}

extern "C" int ofx_replay_gather_valid(ofx_handle *h, const int32_t *slot, const int32_t *n_sampled, int32_t batch,
                                       int32_t first, int32_t max_rows, ofx_transition *rows, void *bits_prev,
                                       void *bits_next, int32_t *n_rows_host) {
  return gather_window(h, "ofx_replay_gather_valid", slot, n_sampled, batch, first, max_rows, rows, bits_prev, bits_next,
                       n_rows_host, nullptr);
}

extern "C" int ofx_replay_gather_nstep(ofx_handle *h, const int32_t *slot, const int32_t *n_sampled, int32_t batch,
                                       int32_t first, int32_t max_rows, int32_t nstep, float gamma, ofx_transition *rows,
                                       void *bits_prev, void *bits_next, float *ret, float *disc, int32_t *n_rows_host) {
  if (!ret || !disc || nstep < 1 || nstep > 64 || !(gamma >= 0.f && gamma <= 1.f)) {  // (NaN fails the gamma test)
    ofx_set_error("ofx_replay_gather_nstep: ret and disc must be given, nstep in 1..64 and gamma in [0, 1], got %d, %g",
                  nstep, (double)gamma);
    return OFX_ERR_INVALID;
  }
  const NstepParams q{nstep, (double)gamma, ret, disc};
  return gather_window(h, "ofx_replay_gather_nstep", slot, n_sampled, batch, first, max_rows, rows, bits_prev, bits_next,
                       n_rows_host, &q);
}

// ---- prioritized experience replay (Schaul et al. 2016, proportional variant; include/ofx.h states the contract) ------
// mass[a][ring position] = p^alpha beside every row; sampling is stratified proportional over the arena's eligible rows,
// with a summation order fixed so that a CPU restatement (tests/per_oracle.py) picks the same slots: float64 sums, 64
// chunks of ceil(valid / 64) consecutive rows each summed in row order, chunk totals chained in chunk order.
__global__ void k_fill_f32(size_t count, float v, float *out) {
  const size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
  if (i < count) out[i] = v;
}

extern "C" int ofx_replay_prioritize(ofx_handle *h, float alpha, float eps) {
  if (!h) { ofx_set_error("ofx_replay_prioritize: null handle"); return OFX_ERR_INVALID; }
  ofx_replay *r = h->replay;
  if (!r) { ofx_set_error("ofx_replay_prioritize before ofx_replay_create"); return OFX_ERR_STATE; }
  if (!(alpha >= 0.f && alpha <= FLT_MAX) || !(eps > 0.f && eps <= FLT_MAX)) {  // (NaN fails both)
    ofx_set_error("ofx_replay_prioritize: alpha must be >= 0 and eps > 0, got %g, %g", (double)alpha, (double)eps);
    return OFX_ERR_INVALID;
  }
  OFX_HIP(hipSetDevice(h->cfg.device));
  OFX_HIP(hipStreamSynchronize(h->stream));
  const size_t N = h->cfg.n_arenas, NC = N * (size_t)r->capacity;
  if (!r->mass) {
    OFX_HIP(hipMalloc((void **)&r->mass, sizeof(float) * NC));
    OFX_HIP(hipMalloc((void **)&r->mmax, sizeof(float) * N));
  }
  r->alpha = alpha;
  r->eps = eps;
  // every row already in the memory, and every new one until the first update, has mass 1
  hipLaunchKernelGGL(k_fill_f32, dim3((unsigned)((NC + 255) / 256)), dim3(256), 0, h->stream, NC, 1.f, r->mass);
  hipLaunchKernelGGL(k_fill_f32, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, h->stream, N, 1.f, r->mmax);
  OFX_HIP(hipGetLastError());
  OFX_HIP(hipStreamSynchronize(h->stream));
  return OFX_OK;
}

static int per_ready(ofx_handle *h, const char *who) {
  if (!h || !h->replay) { ofx_set_error("%s: no replay memory", who); return OFX_ERR_STATE; }
  if (!h->replay->mass) { ofx_set_error("%s: prioritized replay is off (ofx_replay_prioritize)", who); return OFX_ERR_STATE; }
  return OFX_OK;
}

struct PerSampleParams {
  int N, C, F, batch, arena_base;
  ofx_rng_key key;
  uint32_t draw;
  double beta;
  ofx_replay r;
  int32_t *slot, *n_out;
  float *is_weight;
};

// The summation order of the proportional pick, by the arena's wave: lane L sums chunk L of the `valid` eligible rows
// behind the `skip` expired ones, every lane then runs the same sequential chain over the 64 chunk totals.  Returns the
// total, *incl = the lane's inclusive chunk prefix.
__device__ __forceinline__ double arena_chunk_chain(const float *mass, const RowRing &ring, int skip, int valid, int lane,
                                                    double *incl) {
  const int cs = (valid + 63) / 64;
  const int lo = min(lane * cs, valid), hi = min(lo + cs, valid);
  double t = 0.0;
  for (int i = lo; i < hi; i++) t += (double)mass[ring.at(skip + i)];
  double total = 0.0, in = 0.0;
  for (int k = 0; k < 64; k++) {
    total += __shfl(t, k);
    if (k == lane) in = total;
  }
  *incl = in;
  return total;
}

// The walk inside chunk k, whose exclusive prefix is ex: it rebuilds the chunk's running sum - prefix(row) = ex + running
// sum, which reaches the chunk's inclusive prefix exactly at its last row - and returns the first eligible row whose
// prefix exceeds u (the chunk's last row when rounding left none).
__device__ __forceinline__ int chunk_pick(const float *mass, const RowRing &ring, int skip, int valid, int k, double ex,
                                          double u) {
  const int cs = (valid + 63) / 64, r0 = k * cs, r1 = min(r0 + cs, valid);
  double run = 0.0;
  for (int i = r0; i < r1; i++) {
    run += (double)mass[ring.at(skip + i)];
    if (ex + run > u) return i;
  }
  return r1 - 1;
}

// raw importance-sampling weight of a row of mass m drawn from `rows` eligible rows of `total` mass: (rows * P(row))^-beta
__device__ __forceinline__ float is_weight_raw(double rows, double m, double total, double beta) {
  return total > 0.0 ? (float)pow(rows * m / total, -beta) : 1.f;
}

// One 64-lane wave per arena.  Every lane keeps its own inclusive chunk prefix.  Draw j belongs to lane j % 64: binary
// search over shuffles for the first chunk whose inclusive prefix exceeds u (the prefixes are monotone), then the walk
// inside it.  k_global_draw keeps its own chunk search: there u is wave-uniform and one ballot finds the chunk.
__global__ __launch_bounds__(256) void k_replay_sample_per(PerSampleParams p) {
  const int a = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (a >= p.N) return;  // wave-uniform
  const RowRing ring = row_ring(p.C, p.r.head[a], p.r.count[a]);
  const int skip = expired_rows_wave(p.r, a, p.F, ring, lane);
  const int valid = ring.count - skip, n = min(p.batch, valid);
  const float *mass = p.r.mass + (size_t)a * p.C;
  const int cs = (valid + 63) / 64, nchunks = cs ? (valid + cs - 1) / cs : 0;
  double incl;
  const double total = arena_chunk_chain(mass, ring, skip, valid, lane, &incl);
  int32_t *out = p.slot + (size_t)a * p.batch;
  float *wout = p.is_weight + (size_t)a * p.batch;
  for (int j0 = 0; j0 < n; j0 += 64) {  // wave-uniform trip count: the shuffles below see every lane
    const int j = j0 + lane;
    double u = 0.0;
    if (j < n) {
      uint32_t rr[4];
      ofx_philox4x32_10((uint32_t)(p.arena_base + a), (uint32_t)j, p.draw, OFX_STREAM_PER, p.key, rr);
      const double U = ofx_unit(rr[0]);
      u = ((double)j + U) / n * total;
    }
    int klo = 0, khi = nchunks;  // first chunk with incl > u lies in [klo, khi]; khi == nchunks: none
    for (int it = 0; it < 7; it++) {
      const int mid = (klo + khi) >> 1;
      const double v = __shfl(incl, min(mid, 63));
      if (klo < khi) {
        if (v > u) khi = mid;
        else klo = mid + 1;
      }
    }
    double ex = __shfl(incl, max(klo - 1, 0));
    if (klo == 0) ex = 0.0;
    if (j < n) {
      // klo == nchunks: rounding left no row above u, the last eligible row
      const int pick = klo < nchunks ? chunk_pick(mass, ring, skip, valid, klo, ex, u) : valid - 1;
      out[j] = skip + pick;
      wout[j] = is_weight_raw((double)valid, (double)mass[ring.at(skip + pick)], total, p.beta);
    }
  }
  for (int j = n + lane; j < p.batch; j += 64) { out[j] = -1; wout[j] = 0.f; }
  if (p.n_out && lane == 0) p.n_out[a] = n;
}

extern "C" int ofx_replay_sample_prioritized(ofx_handle *h, uint64_t seed, uint32_t draw, int32_t batch, double beta,
                                             int32_t *slot, int32_t *n_sampled, float *is_weight) {
  int rc;
  if ((rc = per_ready(h, "ofx_replay_sample_prioritized"))) return rc;
  if (!slot || !is_weight || batch <= 0 || !(beta >= -DBL_MAX && beta <= DBL_MAX)) {
    ofx_set_error("ofx_replay_sample_prioritized: bad argument");
    return OFX_ERR_INVALID;
  }
  OFX_HIP(hipSetDevice(h->cfg.device));
  PerSampleParams p;
  p.N = h->cfg.n_arenas; p.C = h->replay->capacity; p.F = h->replay->frames; p.batch = batch;
  p.arena_base = h->cfg.arena_base; p.key = ofx_key(seed); p.draw = draw; p.beta = beta;
  p.r = *h->replay; p.slot = slot; p.n_out = n_sampled; p.is_weight = is_weight;
  hipLaunchKernelGGL(k_replay_sample_per, dim3((unsigned)((p.N + 3) / 4)), dim3(256), 0, h->stream, p);
  OFX_HIP(hipGetLastError());
  return OFX_OK;
}

// packed entry d = off[a] + j - first of the window (ofx_replay_gather_valid's order) <- is_weight[a][j]
__global__ __launch_bounds__(256) void k_replay_window_pack(int N, int batch, const float *is_weight, const int32_t *n_sampled,
                                                            const int32_t *off, int first, int max_rows, float *out) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= N * batch) return;
  const int a = t / batch, j = t - a * batch;
  if (j >= n_sampled[a]) return;
  const int d = off[a] + j - first;
  if (d < 0 || d >= max_rows) return;
  out[d] = is_weight[t];
}

// the maximum of v[0 .. n) and 0 in every thread of a workgroup of 1024 (the max is exact in any order)
__device__ __forceinline__ float block_max(const float *v, int n) {
  __shared__ float red[1024];
  const int tid = threadIdx.x;
  float m = 0.f;
  for (int d = tid; d < n; d += 1024) m = fmaxf(m, v[d]);
  red[tid] = m;
  __syncthreads();
  for (int k = 512; k > 0; k >>= 1) {
    if (tid < k) red[tid] = fmaxf(red[tid], red[tid + k]);
    __syncthreads();
  }
  return red[0];
}

// The raw weights of a minibatch over their maximum.  The minibatch is what an exclusive scan (k_replay_scan) counted,
// from entry `first` on and `cap` entries at the most: w[0 .. n), n = min(max(*total - first, 0), cap).
template <typename T>
__global__ __launch_bounds__(1024) void k_replay_norm(const T *total, int first, int cap, float *w) {
  const long long left = (long long)*total - first;
  const int n = (int)(left < 0 ? 0 : left < cap ? left : cap);
  const float mx = block_max(w, n);
  if (mx > 0.f)
    for (int d = threadIdx.x; d < n; d += 1024) w[d] = w[d] / mx;
}

extern "C" int ofx_replay_window_weights(ofx_handle *h, const float *is_weight, const int32_t *n_sampled, int32_t batch,
                                         int32_t first, int32_t max_rows, float *out) {
  int rc;
  if ((rc = per_ready(h, "ofx_replay_window_weights"))) return rc;
  if (!is_weight || !n_sampled || !out || batch <= 0 || first < 0 || max_rows <= 0) {
    ofx_set_error("ofx_replay_window_weights: bad argument");
    return OFX_ERR_INVALID;
  }
  OFX_HIP(hipSetDevice(h->cfg.device));
  const int N = h->cfg.n_arenas;
  int32_t *off = h->replay->scan_off;
  hipLaunchKernelGGL((k_replay_scan<int32_t, int32_t>), dim3(1), dim3(1024), 0, h->stream, N, n_sampled, off);
  hipLaunchKernelGGL(k_replay_window_pack, dim3((unsigned)((N * batch + 255) / 256)), dim3(256), 0, h->stream, N, batch,
                     is_weight, n_sampled, (const int32_t *)off, first, max_rows, out);
  hipLaunchKernelGGL(k_replay_norm<int32_t>, dim3(1), dim3(1024), 0, h->stream, (const int32_t *)off + N, first, max_rows, out);
  OFX_HIP(hipGetLastError());
  return OFX_OK;
}

// Whether a write-back entry lands - oldest-first row s of arena a (whose rows are `ring`), gathered as g, with the two
// errors e: the row is in range, the ring row still holds the gathered (tick_prev, ship), both errors are finite.
// *pos_out = the row's position in rows / mass.
__device__ __forceinline__ bool entry_lands(const ofx_replay &r, const RowRing &ring, int a, int s, const ofx_transition &g,
                                            const float *e, size_t *pos_out) {
  if (s < 0 || s >= ring.count) return false;
  const size_t pos = (size_t)a * ring.C + ring.at(s);
  if (r.rows[pos].tick_prev != g.tick_prev || r.rows[pos].ship != g.ship) return false;  // overwritten since sampling
  if (!isfinite(e[0]) || !isfinite(e[1])) return false;
  *pos_out = pos;
  return true;
}

// one thread per arena, j in order: a duplicate row takes the later packed position's priority
__global__ void k_replay_update_per(int N, int C, int batch, const int32_t *slot, const int32_t *n_sampled, const int32_t *off,
                                    int first, int n_rows, const ofx_transition *rows, const float *td, ofx_replay r) {
  const int a = blockIdx.x * blockDim.x + threadIdx.x;
  if (a >= N) return;
  const RowRing ring = row_ring(C, r.head[a], r.count[a]);
  const int j0 = max(0, first - off[a]), j1 = min(n_sampled[a], first + n_rows - off[a]);
  float mx = r.mmax[a];
  for (int j = j0; j < j1; j++) {
    const int d = off[a] + j - first;
    const float *e = td + 2 * (size_t)d;
    size_t pos;
    if (!entry_lands(r, ring, a, slot[(size_t)a * batch + j], rows[d], e, &pos)) continue;
    const float m = per_mass(e[0], e[1], r.eps, r.alpha);
    r.mass[pos] = m;
    mx = fmaxf(mx, m);
  }
  r.mmax[a] = mx;
}

extern "C" int ofx_replay_update_priorities(ofx_handle *h, const int32_t *slot, const int32_t *n_sampled, int32_t batch,
                                            int32_t first, int32_t n_rows, const ofx_transition *rows, const float *td) {
  int rc;
  if ((rc = per_ready(h, "ofx_replay_update_priorities"))) return rc;
  if (!slot || !n_sampled || !rows || !td || batch <= 0 || first < 0 || n_rows < 0) {
    ofx_set_error("ofx_replay_update_priorities: bad argument");
    return OFX_ERR_INVALID;
  }
  if (n_rows == 0) return OFX_OK;
  OFX_HIP(hipSetDevice(h->cfg.device));
  const int N = h->cfg.n_arenas;
  int32_t *off = h->replay->scan_off;  // recomputed here: never the offsets an earlier call left behind
  hipLaunchKernelGGL((k_replay_scan<int32_t, int32_t>), dim3(1), dim3(1024), 0, h->stream, N, n_sampled, off);
  hipLaunchKernelGGL(k_replay_update_per, dim3((N + 63) / 64), dim3(64), 0, h->stream, N, h->replay->capacity, batch, slot,
                     n_sampled, (const int32_t *)off, first, n_rows, rows, td, *h->replay);
  OFX_HIP(hipGetLastError());
  return OFX_OK;
}

// masses of one arena, oldest first (the order of ofx_replay_rows_host)
extern "C" int ofx_replay_priorities_host(ofx_handle *h, int32_t arena, float *mass_host, int32_t *n_host) {
  int rc;
  if ((rc = per_ready(h, "ofx_replay_priorities_host"))) return rc;
  if (!mass_host || !n_host) { ofx_set_error("ofx_replay_priorities_host: bad argument"); return OFX_ERR_INVALID; }
  if (arena < 0 || arena >= h->cfg.n_arenas) { ofx_set_error("ofx_replay_priorities_host: arena out of range"); return OFX_ERR_INVALID; }
  return ring_to_host(h, arena, h->replay->mass, sizeof(float), mass_host, n_host);
}

// ---- actor-side initial priorities (Horgan et al. 2018; include/ofx.h states the contract) ---------------------------
static int actor_ready(ofx_handle *h, const char *who) {
  int rc;
  if ((rc = per_ready(h, who))) return rc;
  if (!h->replay->prev_q) { ofx_set_error("%s: actor priorities are off (ofx_replay_actor_priorities)", who); return OFX_ERR_STATE; }
  return OFX_OK;
}

extern "C" int ofx_replay_actor_priorities(ofx_handle *h, float gamma) {
  int rc;
  if ((rc = per_ready(h, "ofx_replay_actor_priorities"))) return rc;
  if (!(gamma >= 0.f && gamma <= 1.f)) {  // (NaN fails both)
    ofx_set_error("ofx_replay_actor_priorities: gamma must lie in [0, 1], got %g", (double)gamma);
    return OFX_ERR_INVALID;
  }
  ofx_replay *r = h->replay;
  OFX_HIP(hipSetDevice(h->cfg.device));
  OFX_HIP(hipStreamSynchronize(h->stream));
  const size_t T = (size_t)h->cfg.n_arenas * h->cfg.n_ships;
  if (!r->prev_q) OFX_HIP(hipMalloc((void **)&r->prev_q, sizeof(float) * 2 * T));
  OFX_HIP(hipMemset(r->prev_q, 0, sizeof(float) * 2 * T));
  OFX_HIP(hipDeviceSynchronize());  // null-stream fill vs the handle's non-blocking stream
  r->actor_gamma = gamma;
  return OFX_OK;
}

extern "C" int ofx_replay_capture_valued(ofx_handle *h, uint32_t tick, const uint8_t *ship_mask, const int32_t *iaction,
                                         const int32_t *ipointer, const float *q_sa, const float *p_sp, const float *v_act,
                                         const float *v_ptr) {
  if (!h) { ofx_set_error("ofx_replay_capture_valued: null handle"); return OFX_ERR_INVALID; }
  int rc;
  if ((rc = actor_ready(h, "ofx_replay_capture_valued"))) return rc;
  const int given = (q_sa != nullptr) + (p_sp != nullptr) + (v_act != nullptr) + (v_ptr != nullptr);
  if (given != 0 && given != 4) {
    ofx_set_error("ofx_replay_capture_valued: pass all of q_sa, p_sp, v_act, v_ptr or none (the last ofx_policy_act's)");
    return OFX_ERR_INVALID;
  }
  if (!given && ofx_policy_act_values(h, &q_sa, &p_sp, &v_act, &v_ptr)) {
    ofx_set_error("ofx_replay_capture_valued: no values given and the handle holds none (the last ofx_policy_act must have had all four outputs NULL)");
    return OFX_ERR_STATE;
  }
  return replay_capture(h, "ofx_replay_capture_valued", tick, ship_mask, iaction, ipointer, q_sa, p_sp, v_act, v_ptr);
}

// prev_q crosses to the host on its own, so that the replay blob keeps its format
extern "C" int ofx_replay_actor_values_host(ofx_handle *h, float *dst_host) {
  int rc;
  if ((rc = actor_ready(h, "ofx_replay_actor_values_host"))) return rc;
  if (!dst_host) { ofx_set_error("ofx_replay_actor_values_host: null argument"); return OFX_ERR_INVALID; }
  OFX_HIP(hipSetDevice(h->cfg.device));
  OFX_HIP(hipStreamSynchronize(h->stream));
  OFX_HIP(hipMemcpy(dst_host, h->replay->prev_q, sizeof(float) * 2 * (size_t)h->cfg.n_arenas * h->cfg.n_ships, hipMemcpyDeviceToHost));
  return OFX_OK;
}

extern "C" int ofx_replay_set_actor_values(ofx_handle *h, const float *src_host) {
  int rc;
  if ((rc = actor_ready(h, "ofx_replay_set_actor_values"))) return rc;
  if (!src_host) { ofx_set_error("ofx_replay_set_actor_values: null argument"); return OFX_ERR_INVALID; }
  OFX_HIP(hipSetDevice(h->cfg.device));
  OFX_HIP(hipStreamSynchronize(h->stream));
  OFX_HIP(hipMemcpy(h->replay->prev_q, src_host, sizeof(float) * 2 * (size_t)h->cfg.n_arenas * h->cfg.n_ships, hipMemcpyHostToDevice));
  return OFX_OK;
}

// ---- global minibatch sampling: n rows from the union of all arenas' memories (include/ofx.h states the contract) -----
// Per-arena pass (skip, v, T) -> integer scan of v -> float64 group scan of T (PER) -> one wave per draw -> the weights
// over their maximum.  The list gather and the list write-back take the (arena, slot) pairs the sampler wrote.
#define OFX_GLOBAL_GROUP 256

// One wave per arena: skip, v and, PER, T[a] by the chunk scheme.
template <bool PER>
__global__ __launch_bounds__(256) void k_global_arena(int N, int C, int F, ofx_replay r) {
  const int a = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (a >= N) return;  // wave-uniform
  const RowRing ring = row_ring(C, r.head[a], r.count[a]);
  const int skip = expired_rows_wave(r, a, F, ring, lane);
  const int valid = ring.count - skip;
  if constexpr (PER) {
    double incl;
    const double total = arena_chunk_chain(r.mass + (size_t)a * C, ring, skip, valid, lane, &incl);
    if (lane == 0) r.g_T[a] = total;
  }
  if (lane == 0) { r.g_skip[a] = skip; r.g_v[a] = valid; }
}

// one workgroup per group of 256 consecutive arenas: s = the sequential running sum of T in arena order
__global__ __launch_bounds__(OFX_GLOBAL_GROUP) void k_global_group_sum(int N, ofx_replay r) {
  __shared__ double s[OFX_GLOBAL_GROUP];
  const int a0 = blockIdx.x * OFX_GLOBAL_GROUP, a = a0 + threadIdx.x, cnt = min(OFX_GLOBAL_GROUP, N - a0);
  s[threadIdx.x] = a < N ? r.g_T[a] : 0.0;
  __syncthreads();
  if (threadIdx.x == 0) {
    double run = 0.0;
    for (int i = 0; i < cnt; i++) { run += s[i]; s[i] = run; }
    r.g_gs[blockIdx.x] = run;
  }
  __syncthreads();
  if (a < N) r.g_G[a] = s[threadIdx.x];
}

// G[a] = X_k + s_a with X_k the chain of the group totals before group k
__global__ __launch_bounds__(256) void k_global_group_chain(int N, ofx_replay r) {
  const int a = blockIdx.x * 256 + threadIdx.x;
  if (a >= N) return;
  const int k = a / OFX_GLOBAL_GROUP;
  double X = 0.0;
  for (int i = 0; i < k; i++) X += r.g_gs[i];
  r.g_G[a] = X + r.g_G[a];
}

struct GlobalDrawParams {
  int N, C, n_rows, arena_base;
  ofx_rng_key key;
  uint32_t draw;
  double beta;
  ofx_replay r;
  int32_t *arena, *slot;
  float *is_weight;
};

// the arena that holds eligible row idx of the (arena, oldest-first) sequence: the last a with voff[a] <= idx
__device__ __forceinline__ int global_arena_of(const long long *voff, int N, long long idx) {
  int lo = 0, hi = N - 1;  // voff[0] = 0 <= idx
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (voff[mid] <= idx) lo = mid;
    else hi = mid - 1;
  }
  return lo;
}

// One wave per draw j; every lane runs the searches on the same values, the lanes share the in-arena chunk sums.
template <bool PER>
__global__ __launch_bounds__(256) void k_global_draw(GlobalDrawParams p) {
  const int j = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (j >= p.n_rows) return;  // wave-uniform
  const long long R = p.r.g_voff[p.N];
  const long long n = R < (long long)p.n_rows ? R : (long long)p.n_rows;
  if (j >= n) {  // wave-uniform: padding
    if (lane == 0) {
      p.arena[j] = -1;
      p.slot[j] = -1;
      if (p.is_weight) p.is_weight[j] = 0.f;
    }
    return;
  }
  uint32_t rr[4];
  ofx_philox4x32_10((uint32_t)p.arena_base, (uint32_t)j, p.draw, OFX_STREAM_GLOBAL, p.key, rr);
  if constexpr (!PER) {
    const long long lo = (long long)j * R / n, hi = ((long long)j + 1) * R / n;
    const long long idx = lo + ofx_draw_int(rr[0], (int32_t)(hi - lo - 1));
    const int a = global_arena_of(p.r.g_voff, p.N, idx);
    if (lane == 0) {
      p.arena[j] = a;
      p.slot[j] = p.r.g_skip[a] + (int)(idx - p.r.g_voff[a]);
      if (p.is_weight) p.is_weight[j] = 1.f;
    }
  } else {
    const double total = p.r.g_G[p.N - 1];
    const double U = ofx_unit(rr[0]);
    const double u = ((double)j + U) / (double)n * total;
    int lo = 0, hi = p.N;  // the first arena with G > u lies in [lo, hi]; hi == N: none
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (p.r.g_G[mid] > u) hi = mid;
      else lo = mid + 1;
    }
    const int a = lo < p.N ? lo : global_arena_of(p.r.g_voff, p.N, R - 1);
    const double up = u - (a ? p.r.g_G[a - 1] : 0.0);
    const RowRing ring = row_ring(p.C, p.r.head[a], p.r.count[a]);
    const int skip = p.r.g_skip[a], valid = p.r.g_v[a];
    const float *mass = p.r.mass + (size_t)a * p.C;
    int pick = valid - 1;  // rounding left no row above u': the arena's last eligible row
    if (valid > 0) {       // wave-uniform (an arena with G > G[a - 1] has rows; the fallback arena has one too)
      double incl;
      arena_chunk_chain(mass, ring, skip, valid, lane, &incl);
      const int cs = (valid + 63) / 64, nchunks = (valid + cs - 1) / cs;
      const unsigned long long hit = __ballot(lane < nchunks && incl > up);  // u' is wave-uniform: one ballot finds the chunk
      if (hit) {
        const int k = __ffsll((long long)hit) - 1;
        double ex = __shfl(incl, max(k - 1, 0));
        if (k == 0) ex = 0.0;
        pick = chunk_pick(mass, ring, skip, valid, k, ex, up);
      }
    }
    if (lane == 0) {
      const double m = valid > 0 ? (double)mass[ring.at(skip + pick)] : 0.0;
      p.arena[j] = a;
      p.slot[j] = skip + pick;
      p.is_weight[j] = is_weight_raw((double)R, m, total, p.beta);
    }
  }
}

static int global_workspace(ofx_handle *h) {
  ofx_replay *r = h->replay;
  if (r->g_skip) return OFX_OK;
  const size_t N = h->cfg.n_arenas, groups = (N + OFX_GLOBAL_GROUP - 1) / OFX_GLOBAL_GROUP;
  OFX_HIP(hipMalloc((void **)&r->g_skip, sizeof(int32_t) * N));
  OFX_HIP(hipMalloc((void **)&r->g_v, sizeof(int32_t) * N));
  OFX_HIP(hipMalloc((void **)&r->g_voff, sizeof(long long) * (N + 1)));
  OFX_HIP(hipMalloc((void **)&r->g_T, sizeof(double) * N));
  OFX_HIP(hipMalloc((void **)&r->g_G, sizeof(double) * N));
  OFX_HIP(hipMalloc((void **)&r->g_gs, sizeof(double) * groups));
  return OFX_OK;
}

extern "C" int ofx_replay_sample_global(ofx_handle *h, uint64_t seed, uint32_t draw, int32_t n_rows, int32_t prioritized,
                                        double beta, int32_t *arena, int32_t *slot, float *is_weight,
                                        int32_t *n_drawn_host, int64_t *eligible_host) {
  if (!h || !h->replay) { ofx_set_error("ofx_replay_sample_global: no replay memory"); return OFX_ERR_STATE; }
  int rc;
  if (prioritized && (rc = per_ready(h, "ofx_replay_sample_global"))) return rc;
  if (!arena || !slot || !n_drawn_host || n_rows <= 0 || (prioritized && !is_weight) ||
      !(beta >= -DBL_MAX && beta <= DBL_MAX)) {
    ofx_set_error("ofx_replay_sample_global: bad argument");
    return OFX_ERR_INVALID;
  }
  ofx_replay *r = h->replay;
  const int N = h->cfg.n_arenas;
  if ((long long)N * r->capacity > 0x7fffffffLL) {
    ofx_set_error("ofx_replay_sample_global: n_arenas * capacity must be < 2^31");
    return OFX_ERR_INVALID;
  }
  OFX_HIP(hipSetDevice(h->cfg.device));
  if ((rc = global_workspace(h))) return rc;
  const dim3 waves((unsigned)((N + 3) / 4));
  if (prioritized)
    hipLaunchKernelGGL(k_global_arena<true>, waves, dim3(256), 0, h->stream, N, r->capacity, r->frames, *r);
  else
    hipLaunchKernelGGL(k_global_arena<false>, waves, dim3(256), 0, h->stream, N, r->capacity, r->frames, *r);
  hipLaunchKernelGGL((k_replay_scan<int32_t, long long>), dim3(1), dim3(1024), 0, h->stream, N, (const int32_t *)r->g_v,
                     r->g_voff);
  GlobalDrawParams p;
  p.N = N; p.C = r->capacity; p.n_rows = n_rows; p.arena_base = h->cfg.arena_base;
  p.key = ofx_key(seed); p.draw = draw; p.beta = beta;
  p.r = *r; p.arena = arena; p.slot = slot; p.is_weight = is_weight;
  const dim3 draws((unsigned)((n_rows + 3) / 4));
  if (prioritized) {
    hipLaunchKernelGGL(k_global_group_sum, dim3((unsigned)((N + OFX_GLOBAL_GROUP - 1) / OFX_GLOBAL_GROUP)),
                       dim3(OFX_GLOBAL_GROUP), 0, h->stream, N, *r);
    hipLaunchKernelGGL(k_global_group_chain, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, h->stream, N, *r);
    hipLaunchKernelGGL(k_global_draw<true>, draws, dim3(256), 0, h->stream, p);
    hipLaunchKernelGGL(k_replay_norm<long long>, dim3(1), dim3(1024), 0, h->stream, (const long long *)r->g_voff + N, 0, n_rows,
                       is_weight);
  } else {
    hipLaunchKernelGGL(k_global_draw<false>, draws, dim3(256), 0, h->stream, p);
  }
  hipError_t e = hipGetLastError();
  long long R = 0;
  if (e == hipSuccess) e = hipMemcpyAsync(&R, r->g_voff + N, sizeof(R), hipMemcpyDeviceToHost, h->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
  if (e != hipSuccess) { ofx_set_error("ofx_replay_sample_global: %s", hipGetErrorString(e)); return OFX_ERR_HIP; }
  *n_drawn_host = (int32_t)(R < (long long)n_rows ? R : (long long)n_rows);
  if (eligible_host) *eligible_host = (int64_t)R;
  return OFX_OK;
}

struct GatherListParams {
  int N, C, F, words, n;
  ofx_replay r;
  const int32_t *arena, *slot;
  ofx_transition *rows;             // [n]
  uint32_t *bits_prev, *bits_next;  // [n][2][words] or null
};

// one workgroup per listed row d: what k_replay_gather_valid writes for the same (arena, slot); an entry that names no
// row gets k_replay_gather's padding row and empty maps
template <bool NSTEP, bool PACKED>
__global__ __launch_bounds__(256) void k_replay_gather_list(GatherListParams p, NstepParams q) {
  const int d = blockIdx.x;
  const int a = p.arena[d], s = p.slot[d];
  const int count = (a >= 0 && a < p.N) ? p.r.count[a] : 0;
  if (s < 0 || s >= count) {  // block-uniform
    gather_pad_row<NSTEP>(p, (size_t)d, q);
    return;
  }
  gather_row<NSTEP, PACKED>(p, a, s, count, d, q);
}

extern "C" int ofx_replay_gather_list(ofx_handle *h, const int32_t *arena, const int32_t *slot, int32_t n, int32_t nstep,
                                      float gamma, ofx_transition *rows, void *bits_prev, void *bits_next, float *ret,
                                      float *disc) {
  if (!h || !h->replay || !arena || !slot || !rows || n <= 0) { ofx_set_error("ofx_replay_gather_list: bad argument"); return OFX_ERR_INVALID; }
  if (nstep < 1 || nstep > 64 || !(gamma >= 0.f && gamma <= 1.f) || (nstep > 1 && (!ret || !disc))) {  // (NaN fails the gamma test)
    ofx_set_error("ofx_replay_gather_list: nstep in 1..64, gamma in [0, 1] and, with nstep > 1, ret and disc must be given, got %d, %g",
                  nstep, (double)gamma);
    return OFX_ERR_INVALID;
  }
  ofx_replay *r = h->replay;
  OFX_HIP(hipSetDevice(h->cfg.device));
  GatherListParams p;
  p.N = h->cfg.n_arenas; p.C = r->capacity; p.F = r->frames; p.words = r->words; p.n = n;
  p.r = *r; p.arena = arena; p.slot = slot; p.rows = rows; p.bits_prev = (uint32_t *)bits_prev; p.bits_next = (uint32_t *)bits_next;
  const bool chain = ret && disc;  // nstep == 1 with both given: ret = reward, disc = gamma * (not done), as the window form
  const NstepParams q{nstep, (double)gamma, ret, disc};
  const dim3 grid((unsigned)n);
  const size_t lds = (size_t)r->words * 8;  // packed: the two maps of a frame
  if (chain && r->packed) hipLaunchKernelGGL((k_replay_gather_list<true, true>), grid, dim3(256), lds, h->stream, p, q);
  else if (chain) hipLaunchKernelGGL((k_replay_gather_list<true, false>), grid, dim3(256), 0, h->stream, p, q);
  else if (r->packed) hipLaunchKernelGGL((k_replay_gather_list<false, true>), grid, dim3(256), lds, h->stream, p, NstepParams{});
  else hipLaunchKernelGGL((k_replay_gather_list<false, false>), grid, dim3(256), 0, h->stream, p, NstepParams{});
  OFX_HIP(hipGetLastError());
  return OFX_OK;
}

// One thread per entry.  Every entry that lands raises mmax; of a run of adjacent entries naming one (arena, slot) the
// last one that lands writes the mass (the outcome of k_replay_update_per's serial walk, without the walk).
__global__ __launch_bounds__(256) void k_replay_update_list(int N, int C, int n, const int32_t *arena, const int32_t *slot,
                                                            const ofx_transition *rows, const float *td, ofx_replay r) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= n) return;
  const int a = arena[j], s = slot[j];
  if (a < 0 || a >= N) return;  // the entry names no arena
  const RowRing ring = row_ring(C, r.head[a], r.count[a]);
  size_t pos;
  if (!entry_lands(r, ring, a, s, rows[j], td + 2 * (size_t)j, &pos)) return;
  const float m = per_mass(td[2 * (size_t)j], td[2 * (size_t)j + 1], r.eps, r.alpha);
  atomicMax(reinterpret_cast<unsigned int *>(r.mmax + a), __float_as_uint(m));  // masses are >= 0: the bit patterns order like the values
  for (int k = j + 1; k < n && arena[k] == a && slot[k] == s; k++) {
    size_t other;
    if (entry_lands(r, ring, a, s, rows[k], td + 2 * (size_t)k, &other)) return;  // a later entry of the run wins
  }
  r.mass[pos] = m;
}

// every arena's mmax <- the maximum over the arenas: under global competition a new row enters at the global maximum
__global__ __launch_bounds__(1024) void k_replay_level_mmax(int N, float *mmax) {
  const float mx = block_max(mmax, N);
  for (int a = threadIdx.x; a < N; a += 1024) mmax[a] = mx;
}

extern "C" int ofx_replay_update_priorities_list(ofx_handle *h, const int32_t *arena, const int32_t *slot, int32_t n,
                                                 const ofx_transition *rows, const float *td) {
  int rc;
  if ((rc = per_ready(h, "ofx_replay_update_priorities_list"))) return rc;
  if (!arena || !slot || !rows || !td || n < 0) { ofx_set_error("ofx_replay_update_priorities_list: bad argument"); return OFX_ERR_INVALID; }
  if (n == 0) return OFX_OK;
  OFX_HIP(hipSetDevice(h->cfg.device));
  const int N = h->cfg.n_arenas;
  hipLaunchKernelGGL(k_replay_update_list, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, h->stream, N, h->replay->capacity,
                     n, arena, slot, rows, td, *h->replay);
  hipLaunchKernelGGL(k_replay_level_mmax, dim3(1), dim3(1024), 0, h->stream, N, h->replay->mmax);
  OFX_HIP(hipGetLastError());
  return OFX_OK;
}

// ---- checkpoint: export / import of the memory of a chunk of arenas (include/ofx.h states the blob's layout) --------
// The frame ring is 1-bit discs of a few ships and lasers: nearly every word is zero.  It crosses to the host as
// (word index, word) pairs of its nonzero words, packed on the device: a count pass (one wave per (arena, slot, map),
// 16-byte loads, a ballot of the nonzero words per component), an exclusive scan of the counts, and a write pass that
// repeats the traversal - a lane's position is the map's base + the popcount of the ballots below it, so the pairs land
// in ascending word order without atomics and two exports of one state give the same bytes.
#define OFX_BLOB_MAGIC 0x5258464Fu /* "OFXR" */
#define OFX_BLOB_VERSION 1u
#define OFX_BLOB_HEADER 80

struct BlobDims {
  int32_t W, H, M, C, F, words, n, per;
};
// the raw arrays in struct order: bytes per arena, and where each array starts inside the raw section
enum { RAW_FRAME_TICK, RAW_FRAME_HEAD, RAW_CUR_SLOT, RAW_ROWS, RAW_HEAD, RAW_COUNT, RAW_APPENDED, RAW_HAS_PREV,
       RAW_LATCHED, RAW_PREV_IACTION, RAW_PREV_PX, RAW_PREV_PY, RAW_PREV_TICK, RAW_PREV_SLOT, RAW_PREV_HEAD, RAW_MASS,
       RAW_MMAX, RAW_N };
static size_t pad8(size_t b) { return (b + 7) & ~(size_t)7; }

static void raw_layout(const BlobDims &d, size_t per_arena[RAW_N], size_t off[RAW_N + 1]) {
  const size_t M = d.M, C = d.C, F = d.F;
  const size_t sz[RAW_N] = {4 * F, 4, 4, sizeof(ofx_transition) * C, 4, 4, 8, M, M, 4 * M, 4 * M, 4 * M, 4 * M, 4 * M,
                            32 * M, d.per ? 4 * C : 0, d.per ? (size_t)4 : 0};
  off[0] = 0;
  for (int i = 0; i < RAW_N; i++) {
    per_arena[i] = sz[i];
    off[i + 1] = off[i] + pad8(sz[i] * (size_t)d.n);
  }
}

static void raw_device(const ofx_replay *r, void *ptrs[RAW_N]) {
  void *p[RAW_N] = {r->frame_tick, r->frame_head, r->cur_slot, r->rows, r->head, r->count, r->appended, r->has_prev,
                    r->latched, r->prev_iaction, r->prev_px, r->prev_py, r->prev_tick, r->prev_slot, r->prev_head,
                    r->mass, r->mmax};
  memcpy(ptrs, p, sizeof(p));
}

template <typename T>
static T rd(const uint8_t *p) {  // a blob read from a file sits at any alignment
  T v;
  memcpy(&v, p, sizeof(T));
  return v;
}
template <typename T>
static void wr(uint8_t *p, T v) { memcpy(p, &v, sizeof(T)); }

// One wave per map m = (arena * F + slot) * 2 + which of the chunk.  WRITE = false: counts[m] = nonzero words;
// WRITE = true: the map's pairs at pairs[off[m] ...] in ascending word index.  Lane l of iteration k0 holds words
// 4 (k0 + l) .. + 3: nonzero_place's order.
template <bool WRITE>
__global__ __launch_bounds__(256) void k_replay_pack(int n_maps, int words, const uint32_t *bits, const int32_t *frame_tick,
                                                     uint32_t *counts, const unsigned long long *off, uint2 *pairs) {
  const int m = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (m >= n_maps) return;  // wave-uniform
  if (frame_tick[m >> 1] < 0) {  // an empty slot (its words are zero since ofx_replay_create / the import's clear)
    if (!WRITE && lane == 0) counts[m] = 0u;
    return;
  }
  const uint4 *src = reinterpret_cast<const uint4 *>(bits + (size_t)m * words);
  const int q = words >> 2;
  unsigned long long run = 0ull;
  if constexpr (WRITE) run = off[m];
  for (int k0 = 0; k0 < q; k0 += 64) {  // wave-uniform trip count: the ballots see every lane
    const int k = k0 + lane;
    uint4 v = make_uint4(0u, 0u, 0u, 0u);
    if (k < q) v = src[k];
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
    unsigned long long pos = nonzero_place(w, lane, &run);
    if constexpr (WRITE) {
#pragma unroll
      for (int c = 0; c < 4; c++)
        if (w[c] != 0u) pairs[pos++] = make_uint2((uint32_t)(4 * k + c), w[c]);
    }
  }
  if (!WRITE && lane == 0) counts[m] = (uint32_t)run;
}

// Exclusive scan of counts[n] in 64 bits -> off[n], total in off[n], in three launches: a chunk of 4096 arenas has 4 M
// maps, which one workgroup takes longer to walk than the count pass takes to produce (profiles/r08_checkpoint_4096.txt).
// The sums of segments of PACK_SEG counts, their scan by one workgroup (k_replay_scan), then every segment's own scan on
// top of its offset.  Every sum is an integer: any order gives the same bytes.
#define PACK_SEG 2048
__device__ inline unsigned long long wave_incl_scan(unsigned long long v, int lane) {
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const unsigned long long u = __shfl_up(v, d);
    if (lane >= d) v += u;
  }
  return v;
}

__global__ __launch_bounds__(256) void k_replay_pack_segsum(int n, const uint32_t *counts, unsigned long long *seg) {
  __shared__ unsigned long long part[4];
  const int lo = blockIdx.x * PACK_SEG, hi = min(lo + PACK_SEG, n), lane = threadIdx.x & 63;
  unsigned long long sum = 0ull;
  for (int i = lo + threadIdx.x; i < hi; i += 256) sum += counts[i];
  sum = wave_incl_scan(sum, lane);
  if (lane == 63) part[threadIdx.x >> 6] = sum;
  __syncthreads();
  if (threadIdx.x == 0) seg[blockIdx.x] = part[0] + part[1] + part[2] + part[3];
}

__global__ __launch_bounds__(256) void k_replay_pack_offsets(int n, int n_seg, const uint32_t *counts,
                                                             const unsigned long long *seg_off, unsigned long long *off) {
  __shared__ unsigned long long part[4];
  const int lo = blockIdx.x * PACK_SEG, hi = min(lo + PACK_SEG, n), lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  unsigned long long carry = seg_off[blockIdx.x];
  for (int base = lo; base < hi; base += 256) {  // block-uniform trip count
    const int i = base + threadIdx.x;
    const unsigned long long c = i < hi ? counts[i] : 0u;
    const unsigned long long incl = wave_incl_scan(c, lane);
    if (lane == 63) part[wave] = incl;
    __syncthreads();
    unsigned long long before = carry;
    for (int w = 0; w < wave; w++) before += part[w];
    if (i < hi) off[i] = before + incl - c;
    carry += part[0] + part[1] + part[2] + part[3];
    __syncthreads();
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) off[n] = seg_off[n_seg];
}

// off[n + 1] <- the scan of counts[n]; off has room for pack_scan_words(n) entries (the segment arrays follow off[n])
static size_t pack_scan_words(int n) { return (size_t)n + 1 + 2 * (size_t)((n + PACK_SEG - 1) / PACK_SEG) + 1; }
static void launch_pack_scan(ofx_handle *h, int n, const uint32_t *counts, unsigned long long *off) {
  const int n_seg = (n + PACK_SEG - 1) / PACK_SEG;
  unsigned long long *seg = off + n + 1, *seg_off = seg + n_seg;
  hipLaunchKernelGGL(k_replay_pack_segsum, dim3((unsigned)n_seg), dim3(256), 0, h->stream, n, counts, seg);
  hipLaunchKernelGGL((k_replay_scan<unsigned long long, unsigned long long>), dim3(1), dim3(1024), 0, h->stream, n_seg,
                     (const unsigned long long *)seg, seg_off);
  hipLaunchKernelGGL(k_replay_pack_offsets, dim3((unsigned)n_seg), dim3(256), 0, h->stream, n, n_seg, counts,
                     (const unsigned long long *)seg_off, off);
}

// the import's scatter: one wave per map walks its pair range (indices checked on the host by ofx_replay_blob_check)
__global__ __launch_bounds__(256) void k_replay_unpack(int n_maps, int words, const unsigned long long *off, const uint2 *pairs,
                                                       uint32_t *bits) {
  const int m = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (m >= n_maps) return;
  uint32_t *dst = bits + (size_t)m * words;
  const unsigned long long lo = off[m], hi = off[m + 1];
  for (unsigned long long i = lo + lane; i < hi; i += 64) {
    const uint2 p = pairs[i];
    if (p.x < (uint32_t)words) dst[p.x] = p.y;
  }
}

// The packed store's side of the blob.  One wave per map m = (arena * F + slot) * 2 + which of the chunk; the map's pairs
// lie in the arena's pool at frame_off (+ the ship map's count for the laser map), cyclically.  TO_POOL = false: the
// export un-wraps them into the blob's pair section at off[m]; TO_POOL = true: the import writes them to where
// ofx_packed_place put the frame.  frame_off / frame_cnt point at the chunk's first arena, pool likewise.
template <bool TO_POOL>
__global__ __launch_bounds__(256) void k_replay_pool_copy(int n_maps, int F, uint32_t pool_pairs, const uint32_t *frame_off,
                                                          const uint32_t *frame_cnt, const unsigned long long *off, uint2 *pool,
                                                          uint2 *pairs) {
  const int m = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (m >= n_maps) return;
  const int fs = m >> 1;
  const uint32_t cnt = frame_cnt[m];
  uint32_t start = frame_off[fs] + ((m & 1) ? frame_cnt[m - 1] : 0u);  // < 2 * pool_pairs
  if (start >= pool_pairs) start -= pool_pairs;
  uint2 *arena_pool = pool + (size_t)(fs / F) * pool_pairs;
  const unsigned long long lo = off[m];
  for (uint32_t i = lane; i < cnt; i += 64) {
    uint32_t at = start + i;  // cnt <= words <= pool_pairs / 4
    if (at >= pool_pairs) at -= pool_pairs;
    if constexpr (TO_POOL) arena_pool[at] = pairs[lo + i];
    else pairs[lo + i] = arena_pool[at];
  }
}

// handle, memory and chunk of an export / import call
static int chunk_ready(ofx_handle *h, const char *who, int32_t arena0, int32_t n_arenas, BlobDims *d) {
  if (!h) { ofx_set_error("%s: null handle", who); return OFX_ERR_INVALID; }
  ofx_replay *r = h->replay;
  if (!r) { ofx_set_error("%s before ofx_replay_create", who); return OFX_ERR_STATE; }
  if (arena0 < 0 || n_arenas <= 0 || (long long)arena0 + n_arenas > h->cfg.n_arenas) {
    ofx_set_error("%s: arenas [%d, %d + %d) outside the handle's %d", who, arena0, arena0, n_arenas, h->cfg.n_arenas);
    return OFX_ERR_INVALID;
  }
  if ((long long)n_arenas * r->frames * 2 > 0x7FFFFFFFll) {
    ofx_set_error("%s: %d arenas x %d frames is more than one chunk can hold: split the chunk", who, n_arenas, r->frames);
    return OFX_ERR_INVALID;
  }
  d->W = h->cfg.width; d->H = h->cfg.height; d->M = h->cfg.n_ships; d->C = r->capacity; d->F = r->frames;
  d->words = r->words; d->n = n_arenas; d->per = r->mass ? 1 : 0;
  return OFX_OK;
}

// counts and offsets of the chunk's maps in two fresh device arrays (the caller frees them); synchronises
static int pack_count(ofx_handle *h, const BlobDims &d, int32_t arena0, uint32_t **counts, unsigned long long **off,
                      unsigned long long *total) {
  ofx_replay *r = h->replay;
  const int n_maps = d.n * d.F * 2;
  *counts = nullptr;
  *off = nullptr;
  OFX_HIP(hipMalloc((void **)counts, sizeof(uint32_t) * (size_t)n_maps));
  hipError_t e = hipMalloc((void **)off, sizeof(unsigned long long) * pack_scan_words(n_maps));
  if (e == hipSuccess && r->packed)  // the store keeps the counts
    e = hipMemcpyAsync(*counts, r->frame_cnt + (size_t)arena0 * d.F * 2, sizeof(uint32_t) * (size_t)n_maps,
                       hipMemcpyDeviceToDevice, h->stream);
  if (e == hipSuccess) {
    if (!r->packed)
      hipLaunchKernelGGL(k_replay_pack<false>, dim3((unsigned)((n_maps + 3) / 4)), dim3(256), 0, h->stream, n_maps, d.words,
                         r->frame_bits + (size_t)arena0 * d.F * 2 * d.words, r->frame_tick + (size_t)arena0 * d.F, *counts,
                         (const unsigned long long *)nullptr, (uint2 *)nullptr);
    launch_pack_scan(h, n_maps, *counts, *off);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpyAsync(total, *off + n_maps, sizeof(*total), hipMemcpyDeviceToHost, h->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
  if (e != hipSuccess) {
    (void)hipFree(*counts);
    if (*off) (void)hipFree(*off);
    *counts = nullptr;
    *off = nullptr;
    ofx_set_error("ofx_replay_export: %s", hipGetErrorString(e));
    return OFX_ERR_HIP;
  }
  return OFX_OK;
}

static size_t blob_bytes(const BlobDims &d, unsigned long long total_pairs) {
  size_t per_arena[RAW_N], off[RAW_N + 1];
  raw_layout(d, per_arena, off);
  return OFX_BLOB_HEADER + off[RAW_N] + sizeof(uint32_t) * (size_t)d.n * d.F * 2 + 8 * (size_t)total_pairs;
}

extern "C" int ofx_replay_export_bytes(ofx_handle *h, int32_t arena0, int32_t n_arenas, size_t *bytes_host) {
  BlobDims d;
  int rc;
  if ((rc = chunk_ready(h, "ofx_replay_export_bytes", arena0, n_arenas, &d))) return rc;
  if (!bytes_host) { ofx_set_error("ofx_replay_export_bytes: null bytes_host"); return OFX_ERR_INVALID; }
  OFX_HIP(hipSetDevice(h->cfg.device));
  uint32_t *counts;
  unsigned long long *off, total = 0;
  if ((rc = pack_count(h, d, arena0, &counts, &off, &total))) return rc;
  (void)hipFree(counts);
  (void)hipFree(off);
  *bytes_host = blob_bytes(d, total);
  return OFX_OK;
}

extern "C" int ofx_replay_export(ofx_handle *h, int32_t arena0, int32_t n_arenas, void *dst_host, size_t bytes,
                                 size_t *written_host) {
  BlobDims d;
  int rc;
  if ((rc = chunk_ready(h, "ofx_replay_export", arena0, n_arenas, &d))) return rc;
  if (!dst_host || !written_host) { ofx_set_error("ofx_replay_export: null argument"); return OFX_ERR_INVALID; }
  ofx_replay *r = h->replay;
  OFX_HIP(hipSetDevice(h->cfg.device));
  uint32_t *counts;
  unsigned long long *off, total = 0;
  if ((rc = pack_count(h, d, arena0, &counts, &off, &total))) return rc;
  const size_t need = blob_bytes(d, total);
  uint2 *pairs = nullptr;
  hipError_t e = hipSuccess;
  rc = OFX_OK;
  if (bytes < need) {
    ofx_set_error("ofx_replay_export: the chunk needs %zu bytes, the destination has %zu", need, bytes);
    rc = OFX_ERR_INVALID;
  }
  const int n_maps = d.n * d.F * 2;
  if (rc == OFX_OK && total) {
    e = hipMalloc((void **)&pairs, 8 * (size_t)total);
    if (e == hipSuccess) {
      if (r->packed)
        hipLaunchKernelGGL(k_replay_pool_copy<false>, dim3((unsigned)((n_maps + 3) / 4)), dim3(256), 0, h->stream, n_maps, d.F,
                           r->pool_pairs, (const uint32_t *)r->frame_off + (size_t)arena0 * d.F,
                           (const uint32_t *)r->frame_cnt + (size_t)arena0 * d.F * 2, (const unsigned long long *)off,
                           r->pool + (size_t)arena0 * r->pool_pairs, pairs);
      else
        hipLaunchKernelGGL(k_replay_pack<true>, dim3((unsigned)((n_maps + 3) / 4)), dim3(256), 0, h->stream, n_maps, d.words,
                           r->frame_bits + (size_t)arena0 * d.F * 2 * d.words, r->frame_tick + (size_t)arena0 * d.F,
                           (uint32_t *)nullptr, (const unsigned long long *)off, pairs);
      e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
  }
  if (rc == OFX_OK && e == hipSuccess) {
    uint8_t *dst = (uint8_t *)dst_host;
    size_t per_arena[RAW_N], roff[RAW_N + 1];
    raw_layout(d, per_arena, roff);
    memset(dst, 0, OFX_BLOB_HEADER);
    wr<uint32_t>(dst + 0, OFX_BLOB_MAGIC); wr<uint32_t>(dst + 4, OFX_BLOB_VERSION);
    wr<int32_t>(dst + 8, d.W); wr<int32_t>(dst + 12, d.H); wr<int32_t>(dst + 16, d.M); wr<int32_t>(dst + 20, d.C);
    wr<int32_t>(dst + 24, d.F); wr<int32_t>(dst + 28, d.words); wr<int32_t>(dst + 32, d.n); wr<int32_t>(dst + 36, d.per);
    wr<float>(dst + 40, d.per ? r->alpha : 0.f); wr<float>(dst + 44, d.per ? r->eps : 0.f);
    wr<uint64_t>(dst + 48, (uint64_t)roff[RAW_N]); wr<uint64_t>(dst + 56, (uint64_t)4 * n_maps);
    wr<uint64_t>(dst + 64, (uint64_t)8 * total);
    void *dev[RAW_N];
    raw_device(r, dev);
    uint8_t *raw = dst + OFX_BLOB_HEADER;
    for (int i = 0; i < RAW_N && e == hipSuccess; i++) {
      const size_t nb = per_arena[i] * (size_t)d.n;
      if (!nb) continue;
      e = hipMemcpy(raw + roff[i], (const uint8_t *)dev[i] + per_arena[i] * (size_t)arena0, nb, hipMemcpyDeviceToHost);
      memset(raw + roff[i] + nb, 0, roff[i + 1] - roff[i] - nb);  // padding is zero: equal states give equal bytes
    }
    uint8_t *cnt = raw + roff[RAW_N];
    if (e == hipSuccess) e = hipMemcpy(cnt, counts, (size_t)4 * n_maps, hipMemcpyDeviceToHost);
    if (e == hipSuccess && total) e = hipMemcpy(cnt + (size_t)4 * n_maps, pairs, 8 * (size_t)total, hipMemcpyDeviceToHost);
    if (e == hipSuccess) *written_host = need;
  }
  (void)hipFree(counts);
  (void)hipFree(off);
  if (pairs) (void)hipFree(pairs);
  if (e != hipSuccess) { ofx_set_error("ofx_replay_export: %s", hipGetErrorString(e)); return OFX_ERR_HIP; }
  return rc;
}

#define BLOB_FAIL(...) do { ofx_set_error("ofx_replay_blob_check: " __VA_ARGS__); return OFX_ERR_INVALID; } while (0)

// Host only: the one place that decides whether a blob may reach the kernels (no handle, no device).
extern "C" int ofx_replay_blob_check(const void *src_host, size_t bytes, int32_t n_ships, int32_t width, int32_t height,
                                     int32_t capacity, int32_t frames, int32_t prioritized, int32_t n_arenas) {
  if (!src_host) BLOB_FAIL("null blob");
  if (n_ships <= 0 || width <= 0 || height <= 0 || capacity <= 0 || frames < 2 || n_arenas <= 0 ||
      ((size_t)width * height) % 128 || (long long)n_arenas * frames * 2 > 0x7FFFFFFFll)
    BLOB_FAIL("bad dimensions to check against (n_ships %d, %d x %d, capacity %d, frames %d, n_arenas %d)", n_ships, width,
              height, capacity, frames, n_arenas);
  const uint8_t *p = (const uint8_t *)src_host;
  if (bytes < OFX_BLOB_HEADER) BLOB_FAIL("truncated: %zu bytes do not hold the %d-byte header", bytes, OFX_BLOB_HEADER);
  if (rd<uint32_t>(p) != OFX_BLOB_MAGIC) BLOB_FAIL("wrong magic 0x%08x", rd<uint32_t>(p));
  if (rd<uint32_t>(p + 4) != OFX_BLOB_VERSION) BLOB_FAIL("unknown format version %u", rd<uint32_t>(p + 4));
  BlobDims d;
  d.W = width; d.H = height; d.M = n_ships; d.C = capacity; d.F = frames;
  d.words = (int32_t)(((size_t)width * height) >> 5); d.n = n_arenas; d.per = prioritized ? 1 : 0;
  const struct { const char *name; int off; int32_t want; } dims[] = {
      {"width", 8, d.W}, {"height", 12, d.H}, {"n_ships", 16, d.M}, {"capacity", 20, d.C}, {"frames", 24, d.F},
      {"words", 28, d.words}, {"n_arenas", 32, d.n}, {"prioritized", 36, d.per}};
  for (const auto &q : dims)
    if (rd<int32_t>(p + q.off) != q.want) BLOB_FAIL("%s is %d in the blob, expected %d", q.name, rd<int32_t>(p + q.off), q.want);
  size_t per_arena[RAW_N], roff[RAW_N + 1];
  raw_layout(d, per_arena, roff);
  const size_t n_maps = (size_t)d.n * d.F * 2;
  const uint64_t raw_bytes = rd<uint64_t>(p + 48), count_bytes = rd<uint64_t>(p + 56), pair_bytes = rd<uint64_t>(p + 64);
  if (raw_bytes != roff[RAW_N]) BLOB_FAIL("raw section size is %llu, expected %zu", (unsigned long long)raw_bytes, roff[RAW_N]);
  if (count_bytes != 4 * n_maps) BLOB_FAIL("count section size is %llu, expected %zu", (unsigned long long)count_bytes, 4 * n_maps);
  if (pair_bytes % 8 || pair_bytes > 8 * n_maps * (uint64_t)d.words)
    BLOB_FAIL("pair section size %llu is impossible", (unsigned long long)pair_bytes);
  const size_t raw_at = OFX_BLOB_HEADER, cnt_at = raw_at + roff[RAW_N], pair_at = cnt_at + 4 * n_maps;
  const size_t end = pair_at + (size_t)pair_bytes;
  if (bytes < cnt_at) BLOB_FAIL("truncated inside the raw section (%zu bytes, the section ends at %zu)", bytes, cnt_at);
  if (bytes < pair_at) BLOB_FAIL("truncated inside the count section (%zu bytes, the section ends at %zu)", bytes, pair_at);
  if (bytes < end) BLOB_FAIL("truncated inside the pair section (%zu bytes, the section ends at %zu)", bytes, end);
  if (bytes > end) BLOB_FAIL("%zu bytes, the sections end at %zu", bytes, end);
  const uint8_t *raw = p + raw_at, *cnt = p + cnt_at, *pr = p + pair_at;
  // the raw arrays
  const uint8_t *ft = raw + roff[RAW_FRAME_TICK];
  for (size_t i = 0; i < (size_t)d.n * d.F; i++)
    if (rd<int32_t>(ft + 4 * i) < -1) BLOB_FAIL("frame_tick %d of arena %zu slot %zu is below -1", rd<int32_t>(ft + 4 * i), i / d.F, i % d.F);
  for (int a = 0; a < d.n; a++) {
    const int32_t fh = rd<int32_t>(raw + roff[RAW_FRAME_HEAD] + 4 * (size_t)a), cs = rd<int32_t>(raw + roff[RAW_CUR_SLOT] + 4 * (size_t)a);
    const int32_t head = rd<int32_t>(raw + roff[RAW_HEAD] + 4 * (size_t)a), count = rd<int32_t>(raw + roff[RAW_COUNT] + 4 * (size_t)a);
    const int64_t app = rd<int64_t>(raw + roff[RAW_APPENDED] + 8 * (size_t)a);
    if (fh < 0 || fh >= d.F) BLOB_FAIL("frame_head %d of arena %d outside [0, %d)", fh, a, d.F);
    if (cs < -1 || cs >= d.F) BLOB_FAIL("cur_slot %d of arena %d outside [-1, %d)", cs, a, d.F);
    if (head < 0 || head >= d.C) BLOB_FAIL("head %d of arena %d outside [0, %d)", head, a, d.C);
    if (count < 0 || count > d.C) BLOB_FAIL("count %d of arena %d outside [0, %d]", count, a, d.C);
    if (app < count) BLOB_FAIL("appended %lld of arena %d below its count %d", (long long)app, a, count);
    const uint8_t *rows = raw + roff[RAW_ROWS] + sizeof(ofx_transition) * (size_t)a * d.C;
    const RowRing ring = row_ring(d.C, head, count);
    for (int i = 0; i < count; i++) {  // the live rows: the sampler and the fit index with these
      const ofx_transition t = rd<ofx_transition>(rows + sizeof(ofx_transition) * (size_t)ring.at(i));
      if (t.frame_prev < 0 || t.frame_prev >= d.F) BLOB_FAIL("row %d of arena %d: frame_prev %d outside [0, %d)", i, a, t.frame_prev, d.F);
      if (t.frame_next < 0 || t.frame_next >= d.F) BLOB_FAIL("row %d of arena %d: frame_next %d outside [0, %d)", i, a, t.frame_next, d.F);
      if (t.ship < 0 || t.ship >= d.M) BLOB_FAIL("row %d of arena %d: ship %d outside [0, %d)", i, a, t.ship, d.M);
      if (t.iaction < 0 || t.iaction > 1) BLOB_FAIL("row %d of arena %d: iaction %d outside [0, 2)", i, a, t.iaction);
      if (t.px < 0 || t.px >= d.W) BLOB_FAIL("row %d of arena %d: px %d outside [0, %d)", i, a, t.px, d.W);
      if (t.py < 0 || t.py >= d.H) BLOB_FAIL("row %d of arena %d: py %d outside [0, %d)", i, a, t.py, d.H);
    }
    for (int s = 0; s < d.M; s++) {  // previous_* of a ship become the indices of its next row
      const size_t t = (size_t)a * d.M + s;
      if (!raw[roff[RAW_HAS_PREV] + t]) continue;
      const int32_t ps = rd<int32_t>(raw + roff[RAW_PREV_SLOT] + 4 * t), ia = rd<int32_t>(raw + roff[RAW_PREV_IACTION] + 4 * t);
      const int32_t px = rd<int32_t>(raw + roff[RAW_PREV_PX] + 4 * t), py = rd<int32_t>(raw + roff[RAW_PREV_PY] + 4 * t);
      if (ps < 0 || ps >= d.F) BLOB_FAIL("prev_slot %d of arena %d ship %d outside [0, %d)", ps, a, s, d.F);
      if (ia < 0 || ia > 1) BLOB_FAIL("prev_iaction %d of arena %d ship %d outside [0, 2)", ia, a, s);
      if (px < 0 || px >= d.W || py < 0 || py >= d.H) BLOB_FAIL("prev_px / prev_py (%d, %d) of arena %d ship %d outside the map", px, py, a, s);
    }
    if (d.per) {
      const uint8_t *mass = raw + roff[RAW_MASS] + 4 * (size_t)a * d.C;
      for (int i = 0; i < d.C; i++) {
        const float m = rd<float>(mass + 4 * (size_t)i);
        if (!(m >= 0.f && m <= FLT_MAX)) BLOB_FAIL("mass %g at ring position %d of arena %d is not finite and >= 0", (double)m, i, a);
      }
      const float mm = rd<float>(raw + roff[RAW_MMAX] + 4 * (size_t)a);
      if (!(mm >= 0.f && mm <= FLT_MAX)) BLOB_FAIL("mmax %g of arena %d is not finite and >= 0", (double)mm, a);
    }
  }
  // the packed frames
  uint64_t total = 0;
  for (size_t m = 0; m < n_maps; m++) {
    const uint32_t c = rd<uint32_t>(cnt + 4 * m);
    if (c > (uint32_t)d.words) BLOB_FAIL("count %u of map %zu exceeds the %d words of a map", c, m, d.words);
    if (c && rd<int32_t>(ft + 4 * (m >> 1)) < 0) BLOB_FAIL("map %zu of an empty slot has count %u", m, c);
    total += c;
  }
  if (total * 8 != pair_bytes) BLOB_FAIL("the counts sum to %llu pairs, the pair section holds %llu", (unsigned long long)total, (unsigned long long)(pair_bytes / 8));
  const uint8_t *q = pr;
  for (size_t m = 0; m < n_maps; m++) {
    const uint32_t c = rd<uint32_t>(cnt + 4 * m);
    int64_t last = -1;
    for (uint32_t i = 0; i < c; i++, q += 8) {
      const uint32_t idx = rd<uint32_t>(q), word = rd<uint32_t>(q + 4);
      if (idx >= (uint32_t)d.words) BLOB_FAIL("word index %u of map %zu is outside the %d words of a map", idx, m, d.words);
      if ((int64_t)idx <= last) BLOB_FAIL("word indices of map %zu do not ascend strictly (%u after %lld)", m, idx, (long long)last);
      if (!word) BLOB_FAIL("zero word at index %u of map %zu", idx, m);
      last = idx;
    }
  }
  return OFX_OK;
}
#undef BLOB_FAIL

extern "C" int ofx_replay_import(ofx_handle *h, int32_t arena0, int32_t n_arenas, const void *src_host, size_t bytes) {
  BlobDims d;
  int rc;
  if ((rc = chunk_ready(h, "ofx_replay_import", arena0, n_arenas, &d))) return rc;
  if (!src_host) { ofx_set_error("ofx_replay_import: null blob"); return OFX_ERR_INVALID; }
  ofx_replay *r = h->replay;
  if ((rc = ofx_replay_blob_check(src_host, bytes, d.M, d.W, d.H, d.C, d.F, d.per, d.n))) return rc;
  const uint8_t *p = (const uint8_t *)src_host;
  if (d.per && (memcmp(p + 40, &r->alpha, 4) || memcmp(p + 44, &r->eps, 4))) {
    ofx_set_error("ofx_replay_import: alpha / eps are %g / %g in the blob, %g / %g in the handle (ofx_replay_prioritize)",
                  (double)rd<float>(p + 40), (double)rd<float>(p + 44), (double)r->alpha, (double)r->eps);
    return OFX_ERR_INVALID;
  }
  size_t per_arena[RAW_N], roff[RAW_N + 1];
  raw_layout(d, per_arena, roff);
  const int n_maps = d.n * d.F * 2;
  const uint8_t *raw = p + OFX_BLOB_HEADER, *cnt = raw + roff[RAW_N], *pr = cnt + (size_t)4 * n_maps;
  const size_t pair_bytes = (size_t)rd<uint64_t>(p + 64);
  // a packed store: where every live frame goes, and whether every arena's pool can hold its frames - before any write
  uint32_t *place = nullptr, *place_off = nullptr, *place_head = nullptr, *place_live = nullptr;
  if (r->packed) {
    const size_t nf = (size_t)d.n * d.F;
    place = (uint32_t *)malloc(sizeof(uint32_t) * (nf + 2 * (size_t)d.n));
    if (!place) { ofx_set_error("ofx_replay_import: out of host memory"); return OFX_ERR_INVALID; }
    place_off = place; place_head = place + nf; place_live = place_head + d.n;
    int64_t need = 0;
    const int bad = ofx_packed_place(d.n, d.F, r->pool_pairs, raw + roff[RAW_FRAME_TICK], raw + roff[RAW_FRAME_HEAD], cnt,
                                     place_off, place_head, place_live, &need);
    if (bad >= 0) {
      free(place);
      ofx_set_error("ofx_replay_import: the live frames of arena %d of the chunk hold %lld pairs, the pool %u (pool_pairs of "
                    "ofx_replay_create_packed)", bad, (long long)need, r->pool_pairs);
      return OFX_ERR_INVALID;
    }
  }
  hipError_t e0 = hipSetDevice(h->cfg.device);
  if (e0 == hipSuccess) e0 = hipStreamSynchronize(h->stream);
  if (e0 != hipSuccess) { free(place); OFX_HIP(e0); }
  // staging first: a failed allocation leaves the memory as it was
  uint32_t *counts = nullptr;
  unsigned long long *off = nullptr;
  uint2 *pairs = nullptr;
  hipError_t e = hipMalloc((void **)&counts, (size_t)4 * n_maps);
  if (e == hipSuccess) e = hipMalloc((void **)&off, sizeof(unsigned long long) * pack_scan_words(n_maps));
  if (e == hipSuccess && pair_bytes) e = hipMalloc((void **)&pairs, pair_bytes);
  if (e == hipSuccess) e = hipMemcpy(counts, cnt, (size_t)4 * n_maps, hipMemcpyHostToDevice);
  if (e == hipSuccess && pair_bytes) e = hipMemcpy(pairs, pr, pair_bytes, hipMemcpyHostToDevice);
  void *dev[RAW_N];
  raw_device(r, dev);
  for (int i = 0; i < RAW_N && e == hipSuccess; i++) {
    const size_t nb = per_arena[i] * (size_t)d.n;
    if (nb) e = hipMemcpy((uint8_t *)dev[i] + per_arena[i] * (size_t)arena0, raw + roff[i], nb, hipMemcpyHostToDevice);
  }
  if (r->packed) {
    const size_t nf = (size_t)d.n * d.F;
    if (e == hipSuccess) e = hipMemcpy(r->frame_off + (size_t)arena0 * d.F, place_off, 4 * nf, hipMemcpyHostToDevice);
    if (e == hipSuccess)  // on the stream: the scatter below reads it
      e = hipMemcpyAsync(r->frame_cnt + (size_t)arena0 * d.F * 2, counts, (size_t)4 * n_maps, hipMemcpyDeviceToDevice, h->stream);
    if (e == hipSuccess) e = hipMemcpy(r->pool_head + arena0, place_head, 4 * (size_t)d.n, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(r->live + arena0, place_live, 4 * (size_t)d.n, hipMemcpyHostToDevice);
    free(place);
    if (e == hipSuccess) {
      launch_pack_scan(h, n_maps, counts, off);
      if (pair_bytes)
        hipLaunchKernelGGL(k_replay_pool_copy<true>, dim3((unsigned)((n_maps + 3) / 4)), dim3(256), 0, h->stream, n_maps, d.F,
                           r->pool_pairs, (const uint32_t *)r->frame_off + (size_t)arena0 * d.F,
                           (const uint32_t *)r->frame_cnt + (size_t)arena0 * d.F * 2, (const unsigned long long *)off,
                           r->pool + (size_t)arena0 * r->pool_pairs, pairs);
      e = hipGetLastError();
    }
  } else if (e == hipSuccess) {
    uint32_t *bits = r->frame_bits + (size_t)arena0 * d.F * 2 * d.words;
    e = hipMemsetAsync(bits, 0, sizeof(uint32_t) * (size_t)n_maps * d.words, h->stream);
    if (e == hipSuccess) {
      launch_pack_scan(h, n_maps, counts, off);
      if (pair_bytes)
        hipLaunchKernelGGL(k_replay_unpack, dim3((unsigned)((n_maps + 3) / 4)), dim3(256), 0, h->stream, n_maps, d.words,
                           (const unsigned long long *)off, (const uint2 *)pairs, bits);
      e = hipGetLastError();
    }
  }
  const hipError_t es = hipStreamSynchronize(h->stream);
  if (e == hipSuccess) e = es;
  if (counts) (void)hipFree(counts);
  if (off) (void)hipFree(off);
  if (pairs) (void)hipFree(pairs);
  if (e != hipSuccess) { ofx_set_error("ofx_replay_import: %s", hipGetErrorString(e)); return OFX_ERR_HIP; }
  return OFX_OK;
}
