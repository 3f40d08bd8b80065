// ofx_replay.hip - device-side transition capture: the batched form of Trainer.memory = deque(maxlen=memory_size)
// (agents/qlearnIA_V2.py:58), Trainer.remember (:237-238) and the bookkeeping of QlearnIA.play (:370-403) /
// QlearnIA.reset (:360-368).  Every arena owns one memory (the reference has one arena and one shared TRAINER).
//
// Layout in HBM (288 GB per GPU: the whole memory stays resident, nothing goes to the host):
//   frames  [N][F][2][W*H/32] u32   1-bit observation maps (20 KB per map): a ring of F frames per arena.  An arena
//                                    stores a frame only on lock-steps where one of its agents plays; the maps are
//                                    shared by every ship of the arena and by the two transitions that touch them
//                                    (next_state of t-1 -> t, state of t -> t+1), so they are stored once.
//   rows    [N][C] ofx_transition    ring of the last C transitions per arena in append order (lock-step, then ship
//                                    index: the order of request_actions, battleground.py:146-150)
//   per ship [N][M]                  previous_obs / previous_action / previous_pointer (+ the toVector head) and the
//                                    agent's `done` latch
#include "ofx_internal.h"
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
};

void ofx_replay_free(ofx_handle *h) {
  ofx_replay *r = h->replay;
  if (!r) return;
  void *ptrs[] = {r->frame_bits, r->frame_tick, r->rows, r->head, r->count, r->appended, r->has_prev, r->latched,
                  r->prev_iaction, r->prev_px, r->prev_py, r->prev_tick, r->prev_head, r->frame_head, r->cur_slot,
                  r->prev_slot, r->scan_off, r->mass, r->mmax};
  for (void *p : ptrs) if (p) (void)hipFree(p);
  delete r;
  h->replay = nullptr;
}

template <typename T>
static int zalloc(T **p, size_t count, int fill = 0) {
  OFX_HIP(hipMalloc((void **)p, sizeof(T) * count));
  OFX_HIP(hipMemset(*p, fill, sizeof(T) * count));
  return OFX_OK;
}

extern "C" int ofx_replay_create(ofx_handle *h, int32_t capacity, int32_t frames) {
  if (!h) { ofx_set_error("ofx_replay_create: null handle"); return OFX_ERR_INVALID; }
  if (capacity <= 0 || frames < 0 || frames == 1) {
    ofx_set_error("ofx_replay_create: capacity must be > 0 and frames >= 2 (or 0 = capacity + capacity / 4 + 2), got %d, %d",
                  capacity, frames);
    return OFX_ERR_INVALID;
  }
  if (((size_t)h->cfg.width * h->cfg.height) % 128) {
    ofx_set_error("ofx_replay_create: width*height must be a multiple of 128");
    return OFX_ERR_INVALID;
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
  A(frame_bits, (size_t)r->frames * 2 * N * r->words, 0)
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
  ofx_replay r;
};

// One 64-lane wave per arena, lane = ship.  QlearnIA.play (qlearnIA_V2.py:370-403) per capturing ship:
//   if self.done: return                      -> nothing, not even previous_* changes
//   if obs.done: self.done = True             -> the losing frame is still remembered below
//   if previous_*: remember(previous_obs, previous_action, previous_pointer, obs.reward, obs, obs.done)
//   previous_* = obs, iaction, ipointer
// Rows are appended in ship-index order (ballot prefix), exactly the deque's append order.
__global__ __launch_bounds__(256) void k_replay_capture(CaptureParams p) {
  const int a = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (a >= p.N) return;  // wave-uniform
  const int t = a * p.M + lane;
  const bool ship = lane < p.M && (!p.mask || p.mask[t]);
  const bool plays = ship && !p.r.latched[t];
  float hd[8];
  int done = 0, reward = 0;
  if (plays) {
    reward = p.st.reward[t];  // obs.reward: sampled before Agent.step zeroes it (agent.py:73-74)
    done = p.st.alive[t] ? 0 : 1;
    hd[0] = (float)reward; hd[1] = 1.f;
    hd[2] = (float)p.st.ship_px[t]; hd[3] = (float)p.st.ship_py[t];
    hd[4] = (float)p.W; hd[5] = (float)p.H;
    hd[6] = (float)p.st.ship_x[t]; hd[7] = (float)p.st.ship_y[t];
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
    if (p.r.mass) p.r.mass[(size_t)a * p.C + (head + pos) % p.C] = p.r.mmax[a];  // PER: a new row gets the running max
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
  }
  if (lane == 0 && n_new) {
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

extern "C" int ofx_replay_capture(ofx_handle *h, uint32_t tick, const uint8_t *ship_mask, const int32_t *iaction,
                                  const int32_t *ipointer) {
  if (!h) { ofx_set_error("ofx_replay_capture: null handle"); return OFX_ERR_INVALID; }
  ofx_replay *r = h->replay;
  if (!r) { ofx_set_error("ofx_replay_capture before ofx_replay_create"); return OFX_ERR_STATE; }
  if (!h->spawned) { ofx_set_error("You must execute analyse_battleground first."); return OFX_ERR_STATE; }
  if ((int32_t)tick < 0) { ofx_set_error("ofx_replay_capture: tick must be < 2^31"); return OFX_ERR_INVALID; }
  if (h->cfg.n_ships > OFX_WAVE) { ofx_set_error("ofx_replay_capture: n_ships > 64"); return OFX_ERR_INVALID; }
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
  hipLaunchKernelGGL(k_replay_capture, dim3((p.N + 3) / 4), dim3(256), 0, h->stream, p);
  OFX_HIP(hipGetLastError());
  hipLaunchKernelGGL(k_replay_frames, dim3((unsigned)p.N), dim3(256), 0, h->stream, p.N, r->frames, r->words,
                     (const uint32_t *)h->maps[OFX_MAP_BITS_LSB][0], (const uint32_t *)h->maps[OFX_MAP_BITS_LSB][1], *r);
  OFX_HIP(hipGetLastError());
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

// rows of one arena, oldest first (list(memory))
extern "C" int ofx_replay_rows_host(ofx_handle *h, int32_t arena, ofx_transition *rows_host, int32_t *n_host) {
  if (!h || !h->replay || !rows_host || !n_host) { ofx_set_error("ofx_replay_rows_host: bad argument"); return OFX_ERR_INVALID; }
  if (arena < 0 || arena >= h->cfg.n_arenas) { ofx_set_error("ofx_replay_rows_host: arena out of range"); return OFX_ERR_INVALID; }
  ofx_replay *r = h->replay;
  OFX_HIP(hipSetDevice(h->cfg.device));
  OFX_HIP(hipStreamSynchronize(h->stream));
  int32_t head, count;
  OFX_HIP(hipMemcpy(&head, r->head + arena, 4, hipMemcpyDeviceToHost));
  OFX_HIP(hipMemcpy(&count, r->count + arena, 4, hipMemcpyDeviceToHost));
  const int C = r->capacity;
  const int first = ((head - count) % C + C) % C;
  const ofx_transition *base = r->rows + (size_t)arena * C;
  const int n1 = min(count, C - first);
  if (n1 > 0) OFX_HIP(hipMemcpy(rows_host, base + first, sizeof(ofx_transition) * n1, hipMemcpyDeviceToHost));
  if (count > n1) OFX_HIP(hipMemcpy(rows_host + n1, base, sizeof(ofx_transition) * (count - n1), hipMemcpyDeviceToHost));
  *n_host = count;
  return OFX_OK;
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
  const uint32_t *slot = r->frame_bits + ((size_t)arena * r->frames + f) * 2 * r->words;
  OFX_HIP(hipMemcpy(ship_bits_host, slot, wb, hipMemcpyDeviceToHost));
  OFX_HIP(hipMemcpy(laser_bits_host, slot + r->words, wb, hipMemcpyDeviceToHost));
  return OFX_OK;
}

// ---- minibatch: random.sample(memory, min(batch, len(memory))) per arena (qlearnIA_V2.py:241-243) ----------------
// Floyd's subset sampling (uniform over the subsets, no replacement) on Philox draws: counter (global arena, j,
// draw, stream 3).  Transitions whose `state` frame has already left the arena's frame ring are not eligible (only
// possible when the ring is shorter than the rows need: C rows in runs of consecutive plays use C + #runs frames).  slot[a][j] indexes the arena's rows oldest-first, -1 pads.
#define OFX_STREAM_REPLAY 3u
__global__ void k_replay_sample(int N, int C, int F, int batch, int arena_base, uint32_t k0, uint32_t k1, uint32_t draw,
                                ofx_replay r, int32_t *slot, int32_t *n_out) {
  const int a = blockIdx.x * blockDim.x + threadIdx.x;
  if (a >= N) return;
  const int count = r.count[a], head = r.head[a];
  const int first = ((head - count) % C + C) % C;
  const ofx_transition *rows = r.rows + (size_t)a * C;
  int skip = 0;  // rows are chronological: the expired ones are the oldest
  while (skip < count) {
    const ofx_transition &o = rows[(first + skip) % C];
    if (r.frame_tick[(size_t)a * F + o.frame_prev] == o.tick_prev) break;
    skip++;
  }
  const int valid = count - skip, n = min(batch, valid);
  int32_t *out = slot + (size_t)a * batch;
  for (int j = 0; j < n; j++) {
    const int top = valid - n + j;  // draw t in [0, top]
    uint32_t rr[4];
    ofx_philox4x32_10((uint32_t)(arena_base + a), (uint32_t)j, draw, OFX_STREAM_REPLAY, k0, k1, rr);
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
                     h->cfg.arena_base, (uint32_t)seed, (uint32_t)(seed >> 32), draw, *r, slot, n_sampled);
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

// one workgroup per (arena, j): row copy + the two frames' bit maps (16-byte loads/stores)
__global__ __launch_bounds__(256) void k_replay_gather(GatherParams p) {
  const int a = blockIdx.x / p.batch, j = blockIdx.x - a * p.batch;
  const int s = p.slot[(size_t)a * p.batch + j];
  ofx_transition *dst = p.rows + (size_t)a * p.batch + j;
  if (s < 0) {  // padding: an all-zero row with ship = -1 and empty maps (never uninitialised memory)
    if (threadIdx.x < sizeof(ofx_transition) / 4) ((int32_t *)dst)[threadIdx.x] = threadIdx.x == 4 ? -1 : 0;
    uint32_t *pads[2] = {p.bits_prev, p.bits_next};
    for (int w = 0; w < 2; w++) {
      if (!pads[w]) continue;
      uint4 *out = reinterpret_cast<uint4 *>(pads[w] + ((size_t)a * p.batch + j) * 2 * p.words);
      for (int k = threadIdx.x; k < 2 * p.words / 4; k += 256) out[k] = make_uint4(0u, 0u, 0u, 0u);
    }
    return;
  }
  const int count = p.r.count[a], head = p.r.head[a];
  const int first = ((head - count) % p.C + p.C) % p.C;
  const ofx_transition *src = p.r.rows + (size_t)a * p.C + (first + s) % p.C;
  if (threadIdx.x < sizeof(ofx_transition) / 4) ((int32_t *)dst)[threadIdx.x] = ((const int32_t *)src)[threadIdx.x];
  const int slots[2] = {src->frame_prev, src->frame_next};
  uint32_t *outs[2] = {p.bits_prev, p.bits_next};
  for (int w = 0; w < 2; w++) {
    if (!outs[w]) continue;
    const uint4 *in = reinterpret_cast<const uint4 *>(p.r.frame_bits + ((size_t)a * p.F + slots[w]) * 2 * p.words);
    uint4 *out = reinterpret_cast<uint4 *>(outs[w] + ((size_t)a * p.batch + j) * 2 * p.words);
    for (int k = threadIdx.x; k < 2 * p.words / 4; k += 256) out[k] = in[k];
  }
}

extern "C" int ofx_replay_gather(ofx_handle *h, const int32_t *slot, int32_t batch, ofx_transition *rows,
                                 void *bits_prev, void *bits_next) {
  if (!h || !h->replay || !slot || !rows || batch <= 0) { ofx_set_error("ofx_replay_gather: bad argument"); return OFX_ERR_INVALID; }
  ofx_replay *r = h->replay;
  OFX_HIP(hipSetDevice(h->cfg.device));
  GatherParams p;
  p.N = h->cfg.n_arenas; p.C = r->capacity; p.F = r->frames; p.batch = batch; p.words = r->words;
  p.r = *r; p.slot = slot; p.rows = rows; p.bits_prev = (uint32_t *)bits_prev; p.bits_next = (uint32_t *)bits_next;
  hipLaunchKernelGGL(k_replay_gather, dim3((unsigned)(p.N * batch)), dim3(256), 0, h->stream, p);
  OFX_HIP(hipGetLastError());
  return OFX_OK;
}

// ---- the same minibatch without padding: only the rows that exist, packed (Trainer.replay never pads: its batch is
// min(batch_size, len(memory)) real transitions, qlearnIA_V2.py:241-243) ------------------------------------------------
// exclusive scan of n_sampled[N] by one workgroup -> off[N], total in off[N]
__global__ __launch_bounds__(1024) void k_replay_scan(int N, const int32_t *n_sampled, int32_t *off) {
  __shared__ int part[1024];
  const int tid = threadIdx.x, per = (N + 1023) / 1024, lo = min(tid * per, N), hi = min(lo + per, N);
  int sum = 0;
  for (int i = lo; i < hi; i++) sum += n_sampled[i];
  part[tid] = sum;
  __syncthreads();
  for (int d = 1; d < 1024; d <<= 1) {  // Hillis-Steele inclusive scan of the partial sums
    const int v = tid >= d ? part[tid - d] : 0;
    __syncthreads();
    part[tid] += v;
    __syncthreads();
  }
  int run = tid ? part[tid - 1] : 0;
  for (int i = lo; i < hi; i++) { off[i] = run; run += n_sampled[i]; }
  if (tid == 1023) off[N] = part[1023];
}

// n-step returns (ofx_replay_gather_nstep; include/ofx.h states the contract): chain length, discount and outputs
struct NstepParams {
  int nstep;
  double gamma;
  float *ret, *disc;  // [max_rows]
};

// Wave 0 of the workgroup: the n-step chain from oldest-first row s.  Per step the 64 lanes test 64 consecutive rows
// after the current one; the lowest row of the same ship is the ship's next row in append order, and it is the
// successor iff its tick_prev is the current row's tick_next (a ship's tick_prev values increase strictly; a restart
// in between leaves a gap).  Lane 0 writes ret / disc; returns the oldest-first index of the chain's last row.
__device__ int nstep_chain(const ofx_transition *ring, int C, int first_row, int count, int s, int lane, int d,
                           const NstepParams &q) {
  int cur = s, L = 0;
  double acc = 0.0, pw = 1.0;
  for (;;) {
    const ofx_transition *r = ring + (first_row + cur) % C;
    const int done = r->done, ship = r->ship, tick = r->tick_next;
    acc += pw * (double)r->reward;  // -ffp-contract=off: the product and the sum round on their own
    pw *= q.gamma;
    if (done || ++L == q.nstep) break;
    int next = -1;
    for (int base = cur + 1; base < count; base += 64) {  // wave-uniform trip count
      const int i = base + lane;
      bool same = false;
      int tp = 0;
      if (i < count) {
        const ofx_transition *c = ring + (first_row + i) % C;
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
    q.disc[d] = ring[(first_row + cur) % C].done ? 0.f : (float)pw;
  }
  return cur;
}

// one workgroup per (arena, j): sampled entry j of arena a is packed row off[a] + j - first, when it falls into
// [0, max_rows).  NSTEP: the row is the composite of the n-step chain from it (wave 0 walks the chain first).
template <bool NSTEP>
__global__ __launch_bounds__(256) void k_replay_gather_valid(GatherParams p, const int32_t *n_sampled, const int32_t *off, int first,
                                                             int max_rows, NstepParams q) {
  const int a = blockIdx.x / p.batch, j = blockIdx.x - a * p.batch;
  if (j >= n_sampled[a]) return;
  const int d = off[a] + j - first;
  if (d < 0 || d >= max_rows) return;
  const int s = p.slot[(size_t)a * p.batch + j];
  const int count = p.r.count[a], head = p.r.head[a];
  const int first_row = ((head - count) % p.C + p.C) % p.C;
  const ofx_transition *ring = p.r.rows + (size_t)a * p.C;
  const ofx_transition *src = ring + (first_row + s) % p.C;
  const ofx_transition *end = src;  // the row whose next state is gathered
  if constexpr (NSTEP) {
    __shared__ int end_s;
    if (threadIdx.x < 64) {
      const int e = nstep_chain(ring, p.C, first_row, count, s, threadIdx.x, d, q);
      if (threadIdx.x == 0) end_s = e;
    }
    __syncthreads();
    end = ring + (first_row + end_s) % p.C;
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
    if (!outs[w]) continue;
    const uint4 *in = reinterpret_cast<const uint4 *>(p.r.frame_bits + ((size_t)a * p.F + slots[w]) * 2 * p.words);
    uint4 *out = reinterpret_cast<uint4 *>(outs[w] + (size_t)d * 2 * p.words);
    for (int k = threadIdx.x; k < 2 * p.words / 4; k += 256) out[k] = in[k];
  }
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
  hipLaunchKernelGGL(k_replay_scan, dim3(1), dim3(1024), 0, h->stream, N, n_sampled, off);
  GatherParams p;
  p.N = N; p.C = r->capacity; p.F = r->frames; p.batch = batch; p.words = r->words;
  p.r = *r; p.slot = slot; p.rows = rows; p.bits_prev = (uint32_t *)bits_prev; p.bits_next = (uint32_t *)bits_next;
  if (q)
    hipLaunchKernelGGL(k_replay_gather_valid<true>, dim3((unsigned)(N * batch)), dim3(256), 0, h->stream, p, n_sampled,
                       (const int32_t *)off, first, max_rows, *q);
  else
    hipLaunchKernelGGL(k_replay_gather_valid<false>, dim3((unsigned)(N * batch)), dim3(256), 0, h->stream, p, n_sampled,
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
#define OFX_STREAM_PER 4u
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
  uint32_t k0, k1, draw;
  double beta;
  ofx_replay r;
  int32_t *slot, *n_out;
  float *is_weight;
};

// One 64-lane wave per arena.  Lane L sums chunk L; every lane then runs the same sequential chain over the 64 chunk
// totals and keeps its own inclusive prefix.  Draw j belongs to lane j % 64: binary search for the first chunk whose
// inclusive prefix exceeds u (the prefixes are monotone), then a sequential walk inside it that rebuilds the chunk's
// running sum - prefix(row) = excl(chunk) + running sum, which reaches the chunk's inclusive prefix exactly at its last row.
__global__ __launch_bounds__(256) void k_replay_sample_per(PerSampleParams p) {
  const int a = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (a >= p.N) return;  // wave-uniform
  const int C = p.C;
  const int count = p.r.count[a], head = p.r.head[a];
  const int first = ((head - count) % C + C) % C;
  const ofx_transition *rows = p.r.rows + (size_t)a * C;
  int skip = 0;  // the same eligibility as k_replay_sample: the oldest rows whose `state` frame has left the ring
  while (skip < count) {
    const ofx_transition &o = rows[(first + skip) % C];
    if (p.r.frame_tick[(size_t)a * p.F + o.frame_prev] == o.tick_prev) break;
    skip++;
  }
  const int valid = count - skip, n = min(p.batch, valid);
  const float *mass = p.r.mass + (size_t)a * C;
  const int base = first + skip;  // eligible row i sits at ring position (base + i) % C
  const int cs = (valid + 63) / 64, nchunks = cs ? (valid + cs - 1) / cs : 0;
  const int lo = min(lane * cs, valid), hi = min(lo + cs, valid);
  double t = 0.0;
  for (int i = lo; i < hi; i++) t += (double)mass[(base + i) % C];
  double total = 0.0, incl = 0.0;
  for (int k = 0; k < 64; k++) {
    total += __shfl(t, k);
    if (k == lane) incl = total;
  }
  int32_t *out = p.slot + (size_t)a * p.batch;
  float *wout = p.is_weight + (size_t)a * p.batch;
  for (int j0 = 0; j0 < n; j0 += 64) {  // wave-uniform trip count: the shuffles below see every lane
    const int j = j0 + lane;
    double u = 0.0;
    if (j < n) {
      uint32_t rr[4];
      ofx_philox4x32_10((uint32_t)(p.arena_base + a), (uint32_t)j, p.draw, OFX_STREAM_PER, p.k0, p.k1, rr);
      const double U = (double)rr[0] * 0x1p-32;
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
      int pick = valid - 1;  // rounding left no row above u: the last eligible row
      if (klo < nchunks) {
        const int r0 = klo * cs, r1 = min(r0 + cs, valid);
        double run = 0.0;
        pick = r1 - 1;
        for (int i = r0; i < r1; i++) {
          run += (double)mass[(base + i) % C];
          if (ex + run > u) { pick = i; break; }
        }
      }
      const double m = (double)mass[(base + pick) % C];
      out[j] = skip + pick;
      wout[j] = total > 0.0 ? (float)pow((double)valid * m / total, -p.beta) : 1.f;
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
  p.arena_base = h->cfg.arena_base; p.k0 = (uint32_t)seed; p.k1 = (uint32_t)(seed >> 32); p.draw = draw; p.beta = beta;
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
// the window's weights over their maximum (the max is exact in any order)
__global__ __launch_bounds__(1024) void k_replay_window_norm(int N, const int32_t *off, int first, int max_rows, float *out) {
  __shared__ float red[1024];
  const int tid = threadIdx.x, n = min(max(off[N] - first, 0), max_rows);
  float m = 0.f;
  for (int d = tid; d < n; d += 1024) m = fmaxf(m, out[d]);
  red[tid] = m;
  __syncthreads();
  for (int k = 512; k > 0; k >>= 1) {
    if (tid < k) red[tid] = fmaxf(red[tid], red[tid + k]);
    __syncthreads();
  }
  const float mx = red[0];
  if (mx > 0.f)
    for (int d = tid; d < n; d += 1024) out[d] = out[d] / mx;
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
  hipLaunchKernelGGL(k_replay_scan, dim3(1), dim3(1024), 0, h->stream, N, n_sampled, off);
  hipLaunchKernelGGL(k_replay_window_pack, dim3((unsigned)((N * batch + 255) / 256)), dim3(256), 0, h->stream, N, batch,
                     is_weight, n_sampled, (const int32_t *)off, first, max_rows, out);
  hipLaunchKernelGGL(k_replay_window_norm, dim3(1), dim3(1024), 0, h->stream, N, (const int32_t *)off, first, max_rows, out);
  OFX_HIP(hipGetLastError());
  return OFX_OK;
}

// one thread per arena, j in order: a duplicate row takes the later packed position's priority
__global__ void k_replay_update_per(int N, int C, int batch, const int32_t *slot, const int32_t *n_sampled, const int32_t *off,
                                    int first, int n_rows, const ofx_transition *rows, const float *td, ofx_replay r) {
  const int a = blockIdx.x * blockDim.x + threadIdx.x;
  if (a >= N) return;
  const int count = r.count[a], head = r.head[a];
  const int first_row = ((head - count) % C + C) % C;
  const int j0 = max(0, first - off[a]), j1 = min(n_sampled[a], first + n_rows - off[a]);
  float mx = r.mmax[a];
  for (int j = j0; j < j1; j++) {
    const int d = off[a] + j - first;
    const int s = slot[(size_t)a * batch + j];
    if (s < 0 || s >= count) continue;
    const size_t pos = (size_t)a * C + (first_row + s) % C;
    const ofx_transition &g = rows[d];
    if (r.rows[pos].tick_prev != g.tick_prev || r.rows[pos].ship != g.ship) continue;  // overwritten since sampling
    const float e1 = td[2 * (size_t)d], e2 = td[2 * (size_t)d + 1];
    if (!isfinite(e1) || !isfinite(e2)) continue;
    const float m = powf(fabsf(e1) + fabsf(e2) + r.eps, r.alpha);
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
  hipLaunchKernelGGL(k_replay_scan, dim3(1), dim3(1024), 0, h->stream, N, n_sampled, off);
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
  ofx_replay *r = h->replay;
  OFX_HIP(hipSetDevice(h->cfg.device));
  OFX_HIP(hipStreamSynchronize(h->stream));
  int32_t head, count;
  OFX_HIP(hipMemcpy(&head, r->head + arena, 4, hipMemcpyDeviceToHost));
  OFX_HIP(hipMemcpy(&count, r->count + arena, 4, hipMemcpyDeviceToHost));
  const int C = r->capacity;
  const int first = ((head - count) % C + C) % C;
  const float *base = r->mass + (size_t)arena * C;
  const int n1 = min(count, C - first);
  if (n1 > 0) OFX_HIP(hipMemcpy(mass_host, base + first, sizeof(float) * n1, hipMemcpyDeviceToHost));
  if (count > n1) OFX_HIP(hipMemcpy(mass_host + n1, base, sizeof(float) * (count - n1), hipMemcpyDeviceToHost));
  *n_host = count;
  return OFX_OK;
}
