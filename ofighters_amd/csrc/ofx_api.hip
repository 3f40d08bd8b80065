// ofx_api.hip - C-ABI entry points of libofx.so (see include/ofx.h) and the
// small per-(arena, ship) kernels: spawn, restart, obs head (the lock-step and the bots: ofx_step.hip).
#include <math.h>
#include <stdarg.h>
#include <stdlib.h>
#include <string.h>

#include <new>

#include "ofx_internal.h"

// ------------------------------------------------------------------ errors
static thread_local char g_err[512] = "";

void ofx_set_error(const char *fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}

extern "C" const char *ofx_last_error(void) { return g_err; }
extern "C" int ofx_version(void) { return OFX_VERSION; }

extern "C" int ofx_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

extern "C" void ofx_default_config(ofx_config *c) {
  memset(c, 0, sizeof(*c));
  c->n_arenas = 1;
  c->n_ships = 8;
  c->laser_cap = 512;
  c->width = 400;           // lib/observation.py:10-11
  c->height = 400;
  c->ship_radius = 8;       // lib/ship.py:43
  c->laser_radius = 2;      // lib/laser.py:23
  c->ship_speed = 8;        // lib/ship.py:24
  c->laser_speed = 10;      // lib/ship.py:86 x lib/laser.py:13
  c->reward_death = 0;      // agents/qlearnIA_V2.py:39-44
  c->reward_kill = 0;
  c->reward_aim = 2;
  c->reward_trajectory = 1;
  c->episode_ticks = 200;   // lib/ofighters.py:59
  c->device = 0;
  c->arena_base = 0;
}

static int require_device(void) {
  if (ofx_device_count() <= 0) {
    ofx_set_error("no HIP device visible: libofx has no CPU fallback");
    return OFX_ERR_NO_DEVICE;
  }
  return OFX_OK;
}

// ------------------------------------------------------------ device memory
extern "C" int ofx_malloc(void **dev_ptr, size_t bytes) {
  int rc = require_device();
  if (rc) return rc;
  OFX_HIP(hipMalloc(dev_ptr, bytes ? bytes : 1));
  return OFX_OK;
}
extern "C" int ofx_free(void *dev_ptr) {
  if (dev_ptr) OFX_HIP(hipFree(dev_ptr));
  return OFX_OK;
}
extern "C" int ofx_memcpy_h2d(void *dst, const void *src, size_t bytes) {
  OFX_HIP(hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice));
  // a copy from pageable memory may still be in flight when hipMemcpy returns, and handles run on
  // non-blocking streams: make the bytes visible to every stream before returning (host-convenience path only)
  OFX_HIP(hipDeviceSynchronize());
  return OFX_OK;
}
extern "C" int ofx_memcpy_d2h(void *dst, const void *src, size_t bytes) {
  OFX_HIP(hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost));
  return OFX_OK;
}

// ---------------------------------------------------------------- lifetime
// largest double t with rn(sqrt(t)) <= r  (x86 sqrt is correctly rounded)
static double sqrt_le_threshold(double r) {
  double t = r * r;
  while (sqrt(nextafter(t, INFINITY)) <= r) t = nextafter(t, INFINITY);
  while (sqrt(t) > r) t = nextafter(t, -INFINITY);
  return t;
}

template <typename T>
static int dev_alloc_zero(T **p, size_t count) {
  OFX_HIP(hipMalloc((void **)p, count * sizeof(T) ? count * sizeof(T) : 1));
  // hipMemset on the null stream returns before the fill has run and is NOT ordered with the handle's
  // non-blocking stream: ofx_create synchronises the device once after all allocations (see there)
  OFX_HIP(hipMemset(*p, 0, count * sizeof(T)));
  return OFX_OK;
}

extern "C" int ofx_create(const ofx_config *cfg, ofx_handle **out) {
  if (!cfg || !out) { ofx_set_error("ofx_create: null argument"); return OFX_ERR_INVALID; }
  *out = nullptr;
  if (cfg->n_arenas < 1 || cfg->n_ships < 1 || cfg->n_ships > 64) {
    ofx_set_error("ofx_create: need n_arenas >= 1 and 1 <= n_ships <= 64 (got %d, %d)", cfg->n_arenas, cfg->n_ships);
    return OFX_ERR_INVALID;
  }
  if (cfg->laser_cap < 64 || cfg->laser_cap % 64 || cfg->laser_cap > 32704) {
    ofx_set_error("ofx_create: laser_cap must be a multiple of 64 in [64, 32704] (got %d)", cfg->laser_cap);
    return OFX_ERR_INVALID;
  }
  if (cfg->width < 1 || cfg->height < 1 || ((long long)cfg->width * cfg->height) % 32 ||
      (long long)cfg->width * cfg->height > 524288) {
    ofx_set_error("ofx_create: width*height must be a positive multiple of 32 and <= 524288 (got %d x %d)",
                  cfg->width, cfg->height);
    return OFX_ERR_INVALID;
  }
  if (cfg->ship_radius < 1 || cfg->laser_radius < 1 || cfg->ship_speed < 0 || cfg->laser_speed < 0) {
    ofx_set_error("ofx_create: radii must be >= 1 and speeds >= 0");
    return OFX_ERR_INVALID;
  }
  int rc = require_device();
  if (rc) return rc;
  if (cfg->device < 0 || cfg->device >= ofx_device_count()) {
    ofx_set_error("ofx_create: device %d out of range", cfg->device);
    return OFX_ERR_INVALID;
  }
  OFX_HIP(hipSetDevice(cfg->device));
  ofx_handle *h = new (std::nothrow) ofx_handle();
  if (!h) { ofx_set_error("ofx_create: out of host memory"); return OFX_ERR_INVALID; }
  memset(h, 0, sizeof(*h));
  h->cfg = *cfg;
  h->hit_thresh = sqrt_le_threshold((double)(cfg->laser_radius + cfg->ship_radius));
  const size_t NM = (size_t)cfg->n_arenas * cfg->n_ships, NL = (size_t)cfg->n_arenas * cfg->laser_cap,
               N = (size_t)cfg->n_arenas;
  ofx_state &s = h->st;
#define A(field, count) if ((rc = dev_alloc_zero(&s.field, count))) { ofx_destroy(h); return rc; }
  A(ship_x, NM) A(ship_y, NM) A(ship_px, NM) A(ship_py, NM) A(hull, NM)
  A(reward, NM) A(score, NM) A(obs_reward, NM) A(last_score, NM)
  A(alive, NM) A(killer, NM)
  A(time, N) A(n_lasers, N)
  A(laser_x, NL) A(laser_y, NL) A(laser_dx, NL) A(laser_dy, NL)
  A(laser_owner, NL) A(laser_dead, NL)
  A(overflow, 1) A(episode_sums, (size_t)cfg->n_ships + 1)
#undef A
  if ((rc = dev_alloc_zero(&h->bot_behaviours, (size_t)cfg->n_ships))) { ofx_destroy(h); return rc; }
  h->n_cus = 256;  // MI355X; read from the device below
  { int v = 0; if (hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, cfg->device) == hipSuccess && v > 0) h->n_cus = v; }
  hipError_t e = hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking);
  if (e != hipSuccess) { ofx_set_error("hipStreamCreate: %s", hipGetErrorString(e)); ofx_destroy(h); return OFX_ERR_HIP; }
  h->own_stream = true;
  h->prof_base = -1;
  // the zero fills above ran on the null stream; the handle's stream is non-blocking, so without this a kernel
  // enqueued right after ofx_create (k_spawn) could be overtaken by a late memset (seen with two handles in a row)
  e = hipDeviceSynchronize();
  if (e != hipSuccess) { ofx_set_error("hipDeviceSynchronize: %s", hipGetErrorString(e)); ofx_destroy(h); return OFX_ERR_HIP; }
  *out = h;
  return OFX_OK;
}

extern "C" int ofx_destroy(ofx_handle *h) {
  if (!h) return OFX_OK;
  (void)hipSetDevice(h->cfg.device);
  if (h->stream) (void)hipStreamSynchronize(h->stream);
  ofx_replay_free(h);
  ofx_population_free(h);
  ofx_es_free(h);
  ofx_state &s = h->st;
  void *ptrs[] = {s.ship_x, s.ship_y, s.ship_px, s.ship_py, s.hull, s.reward, s.score, s.obs_reward, s.last_score,
                  s.alive, s.killer, s.time, s.n_lasers, s.laser_x, s.laser_y, s.laser_dx, s.laser_dy,
                  s.laser_owner, s.laser_dead, s.overflow, s.episode_sums, h->bot_behaviours, h->scratch, h->aux, h->prep, h->prep_tmp, h->counter, h->res_iaction, h->fitws, h->fitws2, h->applyws, h->trunk_stat, h->act_vals, h->eps_expo,
                  h->ar_episode, h->ar_dead_once, h->ar_restarted, h->ar_want};
  for (void *p : ptrs) if (p) (void)hipFree(p);
  for (int t = 0; t < 5; t++) for (int w = 0; w < 2; w++) if (h->maps[t][w]) (void)hipFree(h->maps[t][w]);
  if (h->events) { (void)hipEventDestroy(h->ev0); (void)hipEventDestroy(h->ev1); }
  if (h->ring) {
    for (int i = 0; i < h->ring_n; i++) if (h->ring[i]) (void)hipEventDestroy(h->ring[i]);
    free(h->ring);
  }
  if (h->own_stream && h->stream) (void)hipStreamDestroy(h->stream);
  delete h;
  return OFX_OK;
}

extern "C" int ofx_sync(ofx_handle *h) {
  if (!h) { ofx_set_error("null handle"); return OFX_ERR_INVALID; }
  OFX_HIP(hipStreamSynchronize(h->stream));
  return OFX_OK;
}

extern "C" void *ofx_stream(ofx_handle *h) { return h ? (void *)h->stream : nullptr; }

extern "C" int ofx_set_stream(ofx_handle *h, void *stream) {
  if (!h) { ofx_set_error("null handle"); return OFX_ERR_INVALID; }
  OFX_HIP(hipStreamSynchronize(h->stream));
  if (h->own_stream && h->stream) (void)hipStreamDestroy(h->stream);
  h->stream = (hipStream_t)stream;
  h->own_stream = false;
  return OFX_OK;
}

int ofx_ensure_buffer(ofx_handle *h, void **buf, size_t *have, size_t bytes) {
  if (*have >= bytes) return OFX_OK;
  OFX_HIP(hipStreamSynchronize(h->stream));
  if (*buf) (void)hipFree(*buf);
  *buf = nullptr;
  *have = 0;
  OFX_HIP(hipMalloc(buf, bytes));
  *have = bytes;
  return OFX_OK;
}
int ofx_ensure_scratch(ofx_handle *h, size_t bytes) { return ofx_ensure_buffer(h, &h->scratch, &h->scratch_bytes, bytes); }

int ofx_counter(ofx_handle *h, int slot, int32_t **counter) {
  if (!h->counter) OFX_HIP(hipMalloc((void **)&h->counter, 4 * sizeof(int32_t)));
  *counter = h->counter + slot;
  return OFX_OK;
}

int ofx_policy_results(ofx_handle *h, int32_t **iaction, int32_t **ipointer) {
  const size_t S = (size_t)h->cfg.n_arenas * h->cfg.n_ships;
  if (!h->res_iaction) {  // one block for both; zeros until the first forward: an action packed too early is in range
    OFX_HIP(hipMalloc((void **)&h->res_iaction, 3 * S * sizeof(int32_t)));
    OFX_HIP(hipMemsetAsync(h->res_iaction, 0, 3 * S * sizeof(int32_t), h->stream));
    h->res_ipointer = h->res_iaction + S;
  }
  *iaction = h->res_iaction;
  *ipointer = h->res_ipointer;
  return OFX_OK;
}

// ----------------------------------------------------------- spawn / restart
struct ResetParams {
  int N, M, W, H, arena_base;
  ofx_state st;
  const int32_t *draws;      // [N][M][2] or null -> counter RNG
  const uint8_t *mask;       // [N] or null
  uint8_t *dead_once;        // [N][M] of ofx_restart_finished or null: cleared for the arenas that restart
  ofx_rng_key key;
  uint32_t episode;
};

// Battleground.__init__ -> Ship.__init__ (battleground.py:79-81, ship.py:35-58)
__global__ void k_spawn(ResetParams p) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= p.N * p.M) return;
  const int a = t / p.M, i = t - a * p.M;
  int dx, dy;
  if (p.draws) {
    dx = p.draws[2 * t];
    dy = p.draws[2 * t + 1];
  } else {
    ofx_reset_draw(p.key, p.W, p.H, (uint32_t)(p.arena_base + a), (uint32_t)i, p.episode, &dx, &dy);
  }
  p.st.ship_x[t] = dx; p.st.ship_y[t] = dy;
  p.st.ship_px[t] = dx; p.st.ship_py[t] = dy;
  p.st.hull[t] = 1;
  p.st.reward[t] = 0; p.st.score[t] = 0; p.st.obs_reward[t] = 0; p.st.last_score[t] = 0;
  p.st.alive[t] = 1;
  p.st.killer[t] = -1;
  if (i == 0) { p.st.time[a] = 0; p.st.n_lasers[a] = 0; }
}

// Battleground.restart -> Ship.reset -> Agent.reset for ONE ship on the draws (dx, dy)
// (battleground.py:108-117, ship.py:92-106, agent.py:59-64): the one place the quirks live, shared by k_restart and
// k_restart_finished.  The banked score goes to sums[i] and the arena count to sums[M]; with `lengths` the arena's
// clock, as it stood, is added there too before it is zeroed.  sums == null: nothing is counted.
__device__ __forceinline__ void restart_ship(const ofx_state &st, int M, int a, int i, int dx, int dy, long long *sums,
                                             long long *lengths) {
  const int t = a * M + i;
  const int sc = st.score[t];
  st.last_score[t] = sc;                         // scores.append(score)
  if (sums) atomicAdd((unsigned long long *)&sums[i], (unsigned long long)(long long)sc);
  st.score[t] = 0;                               // reward is NOT cleared (agent.py:59-64)
  const int ox = st.ship_x[t], oy = st.ship_y[t];
  st.ship_px[t] = ox;                            // pointing = Point(old x, old y)  ship.py:99
  st.ship_py[t] = oy;
  st.ship_x[t] = dx ? dx : ox;                   // `x or self.body.x`            ship.py:100-101
  st.ship_y[t] = dy ? dy : oy;
  st.alive[t] = 1;                               // state = "flying"; hull NOT restored
  st.killer[t] = -1;
  if (i == 0) {
    if (sums && lengths) atomicAdd((unsigned long long *)lengths, (unsigned long long)(long long)st.time[a]);
    st.time[a] = 0;
    st.n_lasers[a] = 0;                          // self.lasers = []
    if (sums) atomicAdd((unsigned long long *)&sums[M], 1ull);
  }
}

__global__ void k_restart(ResetParams p) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= p.N * p.M) return;
  const int a = t / p.M, i = t - a * p.M;
  if (p.mask && !p.mask[a]) return;
  int dx, dy;
  if (p.draws) {
    dx = p.draws[2 * t];
    dy = p.draws[2 * t + 1];
  } else {
    ofx_reset_draw(p.key, p.W, p.H, (uint32_t)(p.arena_base + a), (uint32_t)i, p.episode, &dx, &dy);
  }
  restart_ship(p.st, p.M, a, i, dx, dy, p.st.episode_sums, nullptr);
  if (p.dead_once) p.dead_once[t] = 0;
}

// ofx_restart_finished (include/ofx.h has the rule).  One 64-lane wave per arena, lane = ship, four arenas per block
// as in k_replay_capture; the decision is a ballot over the selected lanes, so every branch below it is wave-uniform.
// No block barrier; lanes >= M take part in no ballot and touch no memory.
struct FinishedParams {
  int N, M, W, H, arena_base, max_ticks, n_groups;
  ofx_state st;
  const uint8_t *ship_mask;  // [N][M] or null = every ship
  uint8_t *seen;             // [N][M] or null
  const int32_t *group;      // [N] or null = group 0
  long long *sums;           // [n_groups][M+2] or null
  uint32_t *arena_episode;   // [N]
  uint8_t *dead_once;        // [N][M]
  uint8_t *restarted;        // [N]
  ofx_rng_key key;
};

__global__ __launch_bounds__(256) void k_restart_finished(FinishedParams p) {
  const int a = blockIdx.x * OFX_ARENAS_PER_BLOCK + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (a >= p.N) return;  // wave-uniform
  const bool ship = lane < p.M;
  const int t = a * p.M + lane;  // used under `ship` only
  const bool selected = ship && (!p.ship_mask || p.ship_mask[t]);
  bool finished = false;
  if (selected && !p.st.alive[t]) {
    if (p.dead_once[t]) finished = true;
    else p.dead_once[t] = 1;   // seen dead once: the lock-step that follows captures the losing frame
  }
  const unsigned long long sel = __ballot(selected), fin = __ballot(finished);
  const int time = p.st.time[a];
  const bool go = (sel != 0ull && fin == sel) || (p.max_ticks > 0 && time >= p.max_ticks);
  if (lane == 0) p.restarted[a] = go ? 1 : 0;
  if (!go) return;  // wave-uniform
  const uint32_t episode = p.arena_episode[a] + 1u;
  if (lane == 0) p.arena_episode[a] = episode;
  if (!ship) return;
  int dx, dy;
  ofx_reset_draw(p.key, p.W, p.H, (uint32_t)(p.arena_base + a), (uint32_t)lane, episode, &dx, &dy);
  long long *row = nullptr;
  if (p.sums) {
    const int g = p.group ? p.group[a] : 0;
    if (g >= 0 && g < p.n_groups) row = p.sums + (size_t)g * (p.M + 2);
  }
  restart_ship(p.st, p.M, a, lane, dx, dy, row, row ? row + p.M + 1 : nullptr);
  p.dead_once[t] = 0;
  if (p.seen) p.seen[t] = 0;
}

// ofx_restart_arenas: k_restart_finished's restart branch for the arenas of `arena_mask` (null = all), decided by the
// caller.  The same launch shape - wave per arena, lane = ship, every branch wave-uniform, no block barrier - and no
// sums, no `seen`.
struct ArenasParams {
  int N, M, W, H, arena_base;
  ofx_state st;
  const uint8_t *arena_mask; // [N] or null = every arena
  uint32_t *arena_episode;   // [N]
  uint8_t *dead_once;        // [N][M]
  uint8_t *restarted;        // [N]
  ofx_rng_key key;
};

__global__ __launch_bounds__(256) void k_restart_arenas(ArenasParams p) {
  const int a = blockIdx.x * OFX_ARENAS_PER_BLOCK + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (a >= p.N) return;  // wave-uniform
  const bool go = !p.arena_mask || p.arena_mask[a] != 0;
  if (lane == 0) p.restarted[a] = go ? 1 : 0;
  if (!go) return;  // wave-uniform
  const uint32_t episode = p.arena_episode[a] + 1u;
  if (lane == 0) p.arena_episode[a] = episode;
  if (lane >= p.M) return;
  int dx, dy;
  ofx_reset_draw(p.key, p.W, p.H, (uint32_t)(p.arena_base + a), (uint32_t)lane, episode, &dx, &dy);
  restart_ship(p.st, p.M, a, lane, dx, dy, nullptr, nullptr);
  p.dead_once[a * p.M + lane] = 0;
}

static ResetParams reset_params(ofx_handle *h, const int32_t *draws, const uint8_t *mask, uint64_t seed,
                                uint32_t episode) {
  ResetParams p;
  p.N = h->cfg.n_arenas; p.M = h->cfg.n_ships; p.W = h->cfg.width; p.H = h->cfg.height;
  p.arena_base = h->cfg.arena_base;
  p.st = h->st; p.draws = draws; p.mask = mask; p.dead_once = h->ar_dead_once;
  p.key = ofx_key(seed); p.episode = episode;
  return p;
}

static int do_spawn(ofx_handle *h, const int32_t *draws, uint64_t seed) {
  if (!h) { ofx_set_error("null handle"); return OFX_ERR_INVALID; }
  OFX_HIP(hipSetDevice(h->cfg.device));
  ResetParams p = reset_params(h, draws, nullptr, seed, 0);
  const int T = p.N * p.M;
  OFX_HIP(hipMemsetAsync(h->st.episode_sums, 0, sizeof(long long) * (p.M + 1), h->stream));
  hipLaunchKernelGGL(k_spawn, dim3((T + 255) / 256), dim3(256), 0, h->stream, p);
  OFX_HIP(hipGetLastError());
  if (h->ar_episode) {  // ofx_restart_finished's counters start again with the arenas
    OFX_HIP(hipMemsetAsync(h->ar_episode, 0, sizeof(uint32_t) * p.N, h->stream));
    OFX_HIP(hipMemsetAsync(h->ar_dead_once, 0, (size_t)T, h->stream));
  }
  h->spawned = true;
  return ofx_replay_episode_reset(h, nullptr);  // fresh agents: previous_* = None
}

static int do_restart(ofx_handle *h, const int32_t *draws, const uint8_t *mask, uint64_t seed, uint32_t episode) {
  if (!h) { ofx_set_error("null handle"); return OFX_ERR_INVALID; }
  if (!h->spawned) { ofx_set_error("ofx_restart before ofx_spawn"); return OFX_ERR_STATE; }
  OFX_HIP(hipSetDevice(h->cfg.device));
  ResetParams p = reset_params(h, draws, mask, seed, episode);
  const int T = p.N * p.M;
  OFX_HIP(hipMemsetAsync(h->st.episode_sums, 0, sizeof(long long) * (p.M + 1), h->stream));
  hipLaunchKernelGGL(k_restart, dim3((T + 255) / 256), dim3(256), 0, h->stream, p);
  OFX_HIP(hipGetLastError());
  return ofx_replay_episode_reset(h, mask);  // QlearnIA.reset (qlearnIA_V2.py:360-368)
}

extern "C" int ofx_spawn(ofx_handle *h, const int32_t *draws) {
  if (!draws) { ofx_set_error("ofx_spawn: null draws"); return OFX_ERR_INVALID; }
  return do_spawn(h, draws, 0);
}
extern "C" int ofx_spawn_random(ofx_handle *h, uint64_t seed) { return do_spawn(h, nullptr, seed); }
extern "C" int ofx_restart(ofx_handle *h, const int32_t *draws, const uint8_t *arena_mask) {
  if (!draws) { ofx_set_error("ofx_restart: null draws"); return OFX_ERR_INVALID; }
  return do_restart(h, draws, arena_mask, 0, 0);
}
extern "C" int ofx_restart_random(ofx_handle *h, uint64_t seed, uint32_t episode) {
  return do_restart(h, nullptr, nullptr, seed, episode);
}

// ------------------------------------------------ per-arena episodes: restart the arenas whose own episode is over
// one block for the three arrays, zeroed on the handle's stream (in order with whatever is enqueued next)
static int autoreset_alloc(ofx_handle *h) {
  if (h->ar_episode) return OFX_OK;
  const size_t N = (size_t)h->cfg.n_arenas, NM = N * h->cfg.n_ships;
  OFX_HIP(hipMalloc((void **)&h->ar_episode, N * sizeof(uint32_t)));
  if (hipMalloc((void **)&h->ar_dead_once, NM) != hipSuccess || hipMalloc((void **)&h->ar_restarted, N) != hipSuccess) {
    if (h->ar_dead_once) (void)hipFree(h->ar_dead_once);
    (void)hipFree(h->ar_episode);
    h->ar_episode = nullptr; h->ar_dead_once = nullptr; h->ar_restarted = nullptr;
    ofx_set_error("ofx_restart_finished: out of device memory");
    return OFX_ERR_HIP;
  }
  OFX_HIP(hipMemsetAsync(h->ar_episode, 0, N * sizeof(uint32_t), h->stream));
  OFX_HIP(hipMemsetAsync(h->ar_dead_once, 0, NM, h->stream));
  OFX_HIP(hipMemsetAsync(h->ar_restarted, 0, N, h->stream));
  return OFX_OK;
}

extern "C" int ofx_restart_finished(ofx_handle *h, uint64_t seed, const uint8_t *ship_mask, int32_t max_ticks,
                                    uint8_t *seen, const int32_t *group, int32_t n_groups, int64_t *sums) {
  if (!h) { ofx_set_error("null handle"); return OFX_ERR_INVALID; }
  if (max_ticks < 0) { ofx_set_error("ofx_restart_finished: max_ticks must be >= 0 (0 = no clock), got %d", max_ticks); return OFX_ERR_INVALID; }
  if (n_groups < 1 || n_groups > h->cfg.n_arenas) {
    ofx_set_error("ofx_restart_finished: n_groups must be in [1, %d] (got %d)", h->cfg.n_arenas, n_groups);
    return OFX_ERR_INVALID;
  }
  if (group && !sums) { ofx_set_error("ofx_restart_finished: group given without sums"); return OFX_ERR_INVALID; }
  if (!h->spawned) { ofx_set_error("ofx_restart_finished before ofx_spawn"); return OFX_ERR_STATE; }
  OFX_HIP(hipSetDevice(h->cfg.device));
  int rc = autoreset_alloc(h);
  if (rc) return rc;
  FinishedParams p;
  p.N = h->cfg.n_arenas; p.M = h->cfg.n_ships; p.W = h->cfg.width; p.H = h->cfg.height;
  p.arena_base = h->cfg.arena_base; p.max_ticks = max_ticks; p.n_groups = n_groups;
  p.st = h->st; p.ship_mask = ship_mask; p.seen = seen; p.group = group; p.sums = (long long *)sums;
  p.arena_episode = h->ar_episode; p.dead_once = h->ar_dead_once; p.restarted = h->ar_restarted;
  p.key = ofx_key(seed);
  hipLaunchKernelGGL(k_restart_finished, dim3(arena_blocks(p.N)), dim3(256), 0, h->stream, p);
  OFX_HIP(hipGetLastError());
  return ofx_replay_episode_reset(h, h->ar_restarted);  // QlearnIA.reset of the restarted arenas' agents
}

extern "C" int ofx_restart_arenas(ofx_handle *h, uint64_t seed, const uint8_t *arena_mask) {
  if (!h) { ofx_set_error("null handle"); return OFX_ERR_INVALID; }
  if (!h->spawned) { ofx_set_error("ofx_restart_arenas before ofx_spawn"); return OFX_ERR_STATE; }
  OFX_HIP(hipSetDevice(h->cfg.device));
  int rc = autoreset_alloc(h);
  if (rc) return rc;
  ArenasParams p;
  p.N = h->cfg.n_arenas; p.M = h->cfg.n_ships; p.W = h->cfg.width; p.H = h->cfg.height;
  p.arena_base = h->cfg.arena_base;
  p.st = h->st; p.arena_mask = arena_mask;
  p.arena_episode = h->ar_episode; p.dead_once = h->ar_dead_once; p.restarted = h->ar_restarted;
  p.key = ofx_key(seed);
  hipLaunchKernelGGL(k_restart_arenas, dim3(arena_blocks(p.N)), dim3(256), 0, h->stream, p);
  OFX_HIP(hipGetLastError());
  return ofx_replay_episode_reset(h, h->ar_restarted);
}

extern "C" int ofx_autoreset_state_host(ofx_handle *h, uint32_t *episode_host, uint8_t *dead_once_host,
                                        uint8_t *restarted_host) {
  if (!h) { ofx_set_error("null handle"); return OFX_ERR_INVALID; }
  if (!h->ar_episode) { ofx_set_error("ofx_autoreset_state_host before ofx_restart_finished"); return OFX_ERR_STATE; }
  OFX_HIP(hipSetDevice(h->cfg.device));
  const size_t N = (size_t)h->cfg.n_arenas, NM = N * h->cfg.n_ships;
  if (episode_host) OFX_HIP(hipMemcpyAsync(episode_host, h->ar_episode, N * sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
  if (dead_once_host) OFX_HIP(hipMemcpyAsync(dead_once_host, h->ar_dead_once, NM, hipMemcpyDeviceToHost, h->stream));
  if (restarted_host) OFX_HIP(hipMemcpyAsync(restarted_host, h->ar_restarted, N, hipMemcpyDeviceToHost, h->stream));
  OFX_HIP(hipStreamSynchronize(h->stream));
  return OFX_OK;
}

extern "C" int ofx_autoreset_set_state(ofx_handle *h, const uint32_t *episode_host, const uint8_t *dead_once_host) {
  if (!h) { ofx_set_error("null handle"); return OFX_ERR_INVALID; }
  if (!h->spawned) { ofx_set_error("ofx_autoreset_set_state before ofx_spawn"); return OFX_ERR_STATE; }
  OFX_HIP(hipSetDevice(h->cfg.device));
  int rc = autoreset_alloc(h);
  if (rc) return rc;
  const size_t N = (size_t)h->cfg.n_arenas, NM = N * h->cfg.n_ships;
  if (episode_host) OFX_HIP(hipMemcpyAsync(h->ar_episode, episode_host, N * sizeof(uint32_t), hipMemcpyHostToDevice, h->stream));
  if (dead_once_host) OFX_HIP(hipMemcpyAsync(h->ar_dead_once, dead_once_host, NM, hipMemcpyHostToDevice, h->stream));
  OFX_HIP(hipStreamSynchronize(h->stream));  // the host arrays are the caller's again
  return OFX_OK;
}

// ------------------------------------------------------------------ obs head
// Observation.analyse_ship + toVector head (observation.py:101-123)
__global__ void k_obs_head(int N, int M, int W, int H, ofx_state st, double *head, uint8_t *done) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= N * M) return;
  ofx_obs_head(st, t, W, H, head + (size_t)t * 8);
  if (done) done[t] = st.alive[t] ? 0 : 1;
}

extern "C" int ofx_observe_head(ofx_handle *h, double *head, uint8_t *done) {
  if (!h || !head) { ofx_set_error("ofx_observe_head: null argument"); return OFX_ERR_INVALID; }
  if (!h->spawned) { ofx_set_error("You must execute analyse_battleground first."); return OFX_ERR_STATE; }
  OFX_HIP(hipSetDevice(h->cfg.device));
  const int T = h->cfg.n_arenas * h->cfg.n_ships;
  hipLaunchKernelGGL(k_obs_head, dim3((T + 255) / 256), dim3(256), 0, h->stream, h->cfg.n_arenas, h->cfg.n_ships,
                     h->cfg.width, h->cfg.height, h->st, head, done);
  OFX_HIP(hipGetLastError());
  return OFX_OK;
}

extern "C" int ofx_rasterise(ofx_handle *h, int map_type, void *ship_map, void *laser_map) {
  if (!h) { ofx_set_error("null handle"); return OFX_ERR_INVALID; }
  if (!h->spawned) { ofx_set_error("ofx_rasterise before ofx_spawn"); return OFX_ERR_STATE; }
  if (map_type < OFX_MAP_U8 || map_type > OFX_MAP_BITS_LSB) {
    ofx_set_error("ofx_rasterise: unknown map type %d", map_type);
    return OFX_ERR_INVALID;
  }
  if ((ship_map == nullptr) != (laser_map == nullptr)) {
    ofx_set_error("ofx_rasterise: pass both map pointers or neither");
    return OFX_ERR_INVALID;
  }
  OFX_HIP(hipSetDevice(h->cfg.device));
  return ofx_launch_raster(h, map_type, ship_map, laser_map);
}

extern "C" size_t ofx_map_bytes(const ofx_handle *h, int map_type) {
  if (!h) return 0;
  const size_t cells = (size_t)h->cfg.width * h->cfg.height;
  switch (map_type) {
    case OFX_MAP_U8: return cells;
    case OFX_MAP_F32: return cells * 4;
    case OFX_MAP_F64: return cells * 8;
    case OFX_MAP_BITS:
    case OFX_MAP_BITS_LSB: return cells / 8;
    default: return 0;
  }
}

extern "C" void *ofx_map_ptr(ofx_handle *h, int map_type, int which) {
  if (!h || map_type < 0 || map_type > OFX_MAP_BITS_LSB || which < 0 || which > 1) return nullptr;
  return h->maps[map_type][which];
}

// -------------------------------------------------------------- state access
static void *field_ptr(const ofx_handle *h, int f, size_t *bytes) {
  const ofx_state &s = h->st;
  const size_t NM = (size_t)h->cfg.n_arenas * h->cfg.n_ships, NL = (size_t)h->cfg.n_arenas * h->cfg.laser_cap,
               N = (size_t)h->cfg.n_arenas;
  switch (f) {
    case OFX_F_SHIP_X: *bytes = NM * 4; return s.ship_x;
    case OFX_F_SHIP_Y: *bytes = NM * 4; return s.ship_y;
    case OFX_F_SHIP_PX: *bytes = NM * 4; return s.ship_px;
    case OFX_F_SHIP_PY: *bytes = NM * 4; return s.ship_py;
    case OFX_F_SHIP_ALIVE: *bytes = NM; return s.alive;
    case OFX_F_REWARD: *bytes = NM * 4; return s.reward;
    case OFX_F_SCORE: *bytes = NM * 4; return s.score;
    case OFX_F_N_LASERS: *bytes = N * 4; return s.n_lasers;
    case OFX_F_LASER_X: *bytes = NL * 8; return s.laser_x;
    case OFX_F_LASER_Y: *bytes = NL * 8; return s.laser_y;
    case OFX_F_LASER_OWNER: *bytes = NL; return s.laser_owner;
    case OFX_F_LASER_DEAD: *bytes = NL; return s.laser_dead;
    case OFX_F_KILLER: *bytes = NM * 2; return s.killer;
    case OFX_F_TIME: *bytes = N * 4; return s.time;
    case OFX_F_LAST_SCORES: *bytes = NM * 4; return s.last_score;
    case OFX_F_HULL: *bytes = NM * 4; return s.hull;
    case OFX_F_LASER_DX: *bytes = NL * 8; return s.laser_dx;
    case OFX_F_LASER_DY: *bytes = NL * 8; return s.laser_dy;
    case OFX_F_OBS_REWARD: *bytes = NM * 4; return s.obs_reward;
    default: *bytes = 0; return nullptr;
  }
}

extern "C" size_t ofx_field_bytes(const ofx_handle *h, int field) {
  size_t b = 0;
  if (h) field_ptr(h, field, &b);
  return b;
}

extern "C" void *ofx_device_ptr(ofx_handle *h, int field) {
  size_t b;
  return h ? field_ptr(h, field, &b) : nullptr;
}

// ---- zero-copy views (ofx_field_desc / ofx_map_desc)
static void desc_fill(ofx_tensor_desc *d, void *data, int dtype, int device, int ndim, int64_t s0, int64_t s1, int64_t s2) {
  static const int isz[] = {1, 2, 4, 8, 4, 8};
  d->data = data;
  d->dtype = dtype;
  d->itemsize = isz[dtype];
  d->ndim = ndim;
  d->device = device;
  const int64_t sh[4] = {s0, s1, s2, 1};
  int64_t st = 1;
  for (int i = 3; i >= 0; i--) {
    d->shape[i] = i < ndim ? sh[i] : 1;
    d->stride[i] = i < ndim ? st : 0;
    if (i < ndim) st *= sh[i];
  }
}

extern "C" int ofx_field_desc(ofx_handle *h, int field, ofx_tensor_desc *out) {
  if (!h || !out) { ofx_set_error("ofx_field_desc: null argument"); return OFX_ERR_INVALID; }
  size_t b;
  void *ptr = field_ptr(h, field, &b);
  if (!ptr) { ofx_set_error("ofx_field_desc: unknown field %d", field); return OFX_ERR_INVALID; }
  const int64_t N = h->cfg.n_arenas, M = h->cfg.n_ships, L = h->cfg.laser_cap;
  switch (field) {
    case OFX_F_SHIP_ALIVE: desc_fill(out, ptr, OFX_DT_U8, h->cfg.device, 2, N, M, 1); break;
    case OFX_F_KILLER: desc_fill(out, ptr, OFX_DT_I16, h->cfg.device, 2, N, M, 1); break;
    case OFX_F_N_LASERS:
    case OFX_F_TIME: desc_fill(out, ptr, OFX_DT_I32, h->cfg.device, 1, N, 1, 1); break;
    case OFX_F_LASER_X:
    case OFX_F_LASER_Y:
    case OFX_F_LASER_DX:
    case OFX_F_LASER_DY: desc_fill(out, ptr, OFX_DT_F64, h->cfg.device, 2, N, L, 1); break;
    case OFX_F_LASER_OWNER:
    case OFX_F_LASER_DEAD: desc_fill(out, ptr, OFX_DT_U8, h->cfg.device, 2, N, L, 1); break;
    default: desc_fill(out, ptr, OFX_DT_I32, h->cfg.device, 2, N, M, 1); break;   // the [N][M] int32 ship / agent fields
  }
  if ((size_t)(out->shape[0] * (out->ndim > 1 ? out->shape[1] : 1)) * (size_t)out->itemsize != b) {
    ofx_set_error("ofx_field_desc: field %d: description and size disagree", field);
    return OFX_ERR_STATE;
  }
  return OFX_OK;
}

extern "C" int ofx_map_desc(ofx_handle *h, int map_type, int which, ofx_tensor_desc *out) {
  if (!h || !out) { ofx_set_error("ofx_map_desc: null argument"); return OFX_ERR_INVALID; }
  if (map_type < OFX_MAP_U8 || map_type > OFX_MAP_BITS || which < 0 || which > 1) {
    ofx_set_error("ofx_map_desc: map type %d / map %d", map_type, which);
    return OFX_ERR_INVALID;
  }
  OFX_HIP(hipSetDevice(h->cfg.device));
  const size_t per_map = ofx_map_bytes(h, map_type);
  for (int w = 0; w < 2; w++)
    if (!h->maps[map_type][w]) {   // the buffer ofx_rasterise(h, map_type, NULL, NULL) fills: the same lazy allocation
      OFX_HIP(hipMalloc(&h->maps[map_type][w], per_map * (size_t)h->cfg.n_arenas));
      OFX_HIP(hipMemsetAsync(h->maps[map_type][w], 0, per_map * (size_t)h->cfg.n_arenas, h->stream));
    }
  const int64_t N = h->cfg.n_arenas, W = h->cfg.width, H = h->cfg.height;
  void *ptr = h->maps[map_type][which];
  switch (map_type) {
    case OFX_MAP_U8: desc_fill(out, ptr, OFX_DT_U8, h->cfg.device, 3, N, W, H); break;
    case OFX_MAP_F32: desc_fill(out, ptr, OFX_DT_F32, h->cfg.device, 3, N, W, H); break;
    case OFX_MAP_F64: desc_fill(out, ptr, OFX_DT_F64, h->cfg.device, 3, N, W, H); break;
    default: desc_fill(out, ptr, OFX_DT_U8, h->cfg.device, 2, N, (int64_t)per_map, 1); break;
  }
  return OFX_OK;
}

extern "C" int ofx_get_host(ofx_handle *h, int field, void *dst_host, size_t bytes) {
  if (!h || !dst_host) { ofx_set_error("ofx_get_host: null argument"); return OFX_ERR_INVALID; }
  size_t b;
  void *src = field_ptr(h, field, &b);
  if (!src) { ofx_set_error("ofx_get_host: unknown field %d", field); return OFX_ERR_INVALID; }
  if (bytes != b) { ofx_set_error("ofx_get_host: field %d is %zu bytes, caller passed %zu", field, b, bytes); return OFX_ERR_INVALID; }
  OFX_HIP(hipSetDevice(h->cfg.device));
  OFX_HIP(hipMemcpyAsync(dst_host, src, b, hipMemcpyDeviceToHost, h->stream));
  OFX_HIP(hipStreamSynchronize(h->stream));
  return OFX_OK;
}

extern "C" int ofx_overflow_count(ofx_handle *h, int64_t *count_host) {
  if (!h || !count_host) { ofx_set_error("ofx_overflow_count: null argument"); return OFX_ERR_INVALID; }
  OFX_HIP(hipSetDevice(h->cfg.device));
  unsigned long long v = 0;
  OFX_HIP(hipMemcpyAsync(&v, h->st.overflow, sizeof(v), hipMemcpyDeviceToHost, h->stream));
  OFX_HIP(hipMemsetAsync(h->st.overflow, 0, sizeof(v), h->stream));
  OFX_HIP(hipStreamSynchronize(h->stream));
  *count_host = (int64_t)v;
  return OFX_OK;
}

extern "C" int ofx_episode_scores(ofx_handle *h, int64_t *sums) {
  if (!h || !sums) { ofx_set_error("ofx_episode_scores: null argument"); return OFX_ERR_INVALID; }
  OFX_HIP(hipSetDevice(h->cfg.device));
  OFX_HIP(hipMemcpyAsync(sums, h->st.episode_sums, sizeof(int64_t) * (h->cfg.n_ships + 1), hipMemcpyDeviceToDevice,
                         h->stream));
  return OFX_OK;
}

// Per-group sums of the banked scores: block g walks the arenas, a thread per arena, and adds the rows of the arenas
// with group[a] == g into the block's LDS accumulators (integers: exact in any order).  No global atomics and no
// zero fill: every block writes its whole row of `sums`.  A group value no block stands for is never matched.
__global__ void k_scores_grouped(int N, int M, const int32_t *last_score, const int32_t *group, long long *sums) {
  __shared__ unsigned long long acc[65];  // n_ships <= 64 (ofx_create), then the arena count
  const int g = blockIdx.x;
  for (int i = threadIdx.x; i <= M; i += blockDim.x) acc[i] = 0ull;
  __syncthreads();
  for (int a = threadIdx.x; a < N; a += blockDim.x) {
    if (group[a] != g) continue;
    const int32_t *row = last_score + (size_t)a * M;
    for (int k = 0; k < M; k++) {
      int i = k + (int)(threadIdx.x & 63);  // lanes of a wave start at different slots: fewer same-address adds
      i %= M;
      atomicAdd(&acc[i], (unsigned long long)(long long)row[i]);
    }
    atomicAdd(&acc[M], 1ull);
  }
  __syncthreads();
  for (int i = threadIdx.x; i <= M; i += blockDim.x) sums[(size_t)g * (M + 1) + i] = (long long)acc[i];
}

extern "C" int ofx_episode_scores_grouped(ofx_handle *h, const int32_t *group, int32_t n_groups, int64_t *sums) {
  if (!h || !group || !sums) { ofx_set_error("ofx_episode_scores_grouped: null argument"); return OFX_ERR_INVALID; }
  if (n_groups < 1 || n_groups > h->cfg.n_arenas) {
    ofx_set_error("ofx_episode_scores_grouped: n_groups must be in [1, %d] (got %d)", h->cfg.n_arenas, n_groups);
    return OFX_ERR_INVALID;
  }
  OFX_HIP(hipSetDevice(h->cfg.device));
  hipLaunchKernelGGL(k_scores_grouped, dim3(n_groups), dim3(256), 0, h->stream, h->cfg.n_arenas, h->cfg.n_ships,
                     h->st.last_score, group, (long long *)sums);
  OFX_HIP(hipGetLastError());
  return OFX_OK;
}

// The one collective of the path for a C consumer of libofx.so: ofx_episode_scores + an in-place RCCL sum over the
// ranks of `nccl_comm` (an ncclComm_t the caller created with ncclCommInitRank, one rank per GPU), on the handle's
// stream.  libofx.so does not link RCCL: ncclAllReduce is looked up in the process at the first call (the library the
// caller's communicator came from; otherwise librccl.so.1 is opened), so a single-GPU user never loads it.
#include <dlfcn.h>
typedef int (*ofx_nccl_allreduce_fn)(const void *, void *, size_t, int, int, void *, hipStream_t);
extern "C" int ofx_scores_allreduce(ofx_handle *h, void *nccl_comm, int64_t *sums) {
  if (!h || !nccl_comm || !sums) { ofx_set_error("ofx_scores_allreduce: null argument"); return OFX_ERR_INVALID; }
  static ofx_nccl_allreduce_fn fn = nullptr;
  if (!fn) {
    fn = (ofx_nccl_allreduce_fn)dlsym(RTLD_DEFAULT, "ncclAllReduce");
    if (!fn) {
      void *lib = dlopen("librccl.so.1", RTLD_NOW | RTLD_GLOBAL);
      if (!lib) lib = dlopen("librccl.so", RTLD_NOW | RTLD_GLOBAL);
      if (lib) fn = (ofx_nccl_allreduce_fn)dlsym(lib, "ncclAllReduce");
    }
    if (!fn) { ofx_set_error("ofx_scores_allreduce: ncclAllReduce not found (librccl.so is not loadable)"); return OFX_ERR_STATE; }
  }
  int rc = ofx_episode_scores(h, sums);
  if (rc) return rc;
  const int kNcclInt64 = 4, kNcclSum = 0;  // rccl.h: ncclDataType_t ncclInt64 = 4, ncclRedOp_t ncclSum = 0
  const int e = fn(sums, sums, (size_t)h->cfg.n_ships + 1, kNcclInt64, kNcclSum, nccl_comm, h->stream);
  if (e != 0) { ofx_set_error("ofx_scores_allreduce: ncclAllReduce failed with ncclResult_t %d", e); return OFX_ERR_HIP; }
  return OFX_OK;
}

// -------------------------------------------------------------------- timing
extern "C" int ofx_timer_start(ofx_handle *h) {
  if (!h) { ofx_set_error("null handle"); return OFX_ERR_INVALID; }
  OFX_HIP(hipSetDevice(h->cfg.device));
  if (!h->events) {
    OFX_HIP(hipEventCreate(&h->ev0));
    OFX_HIP(hipEventCreate(&h->ev1));
    h->events = true;
  }
  OFX_HIP(hipEventRecord(h->ev0, h->stream));
  return OFX_OK;
}

extern "C" int ofx_timer_stop(ofx_handle *h, float *ms_host) {
  if (!h || !ms_host || !h->events) { ofx_set_error("ofx_timer_stop without ofx_timer_start"); return OFX_ERR_STATE; }
  OFX_HIP(hipEventRecord(h->ev1, h->stream));
  OFX_HIP(hipEventSynchronize(h->ev1));
  OFX_HIP(hipEventElapsedTime(ms_host, h->ev0, h->ev1));
  return OFX_OK;
}

extern "C" int ofx_event_record(ofx_handle *h, int32_t idx) {
  if (!h || idx < 0 || idx >= OFX_RING_MAX) { ofx_set_error("ofx_event_record: bad index %d", idx); return OFX_ERR_INVALID; }
  OFX_HIP(hipSetDevice(h->cfg.device));
  if (!h->ring) {
    h->ring = (hipEvent_t *)calloc(OFX_RING_MAX, sizeof(hipEvent_t));
    if (!h->ring) { ofx_set_error("out of host memory"); return OFX_ERR_INVALID; }
    h->ring_n = OFX_RING_MAX;
  }
  if (!h->ring[idx]) OFX_HIP(hipEventCreate(&h->ring[idx]));
  OFX_HIP(hipEventRecord(h->ring[idx], h->stream));
  return OFX_OK;
}

extern "C" int ofx_event_elapsed(ofx_handle *h, int32_t a, int32_t b, float *ms_host) {
  if (!h || !ms_host || !h->ring || a < 0 || b < 0 || a >= OFX_RING_MAX || b >= OFX_RING_MAX || !h->ring[a] ||
      !h->ring[b]) {
    ofx_set_error("ofx_event_elapsed: events %d / %d were not recorded", a, b);
    return OFX_ERR_STATE;
  }
  OFX_HIP(hipEventSynchronize(h->ring[b]));
  OFX_HIP(hipEventElapsedTime(ms_host, h->ring[a], h->ring[b]));
  return OFX_OK;
}

extern "C" int ofx_policy_profile(ofx_handle *h, int32_t event_base) {
  if (!h || event_base >= OFX_RING_MAX - 1) { ofx_set_error("ofx_policy_profile: bad event base %d", event_base); return OFX_ERR_INVALID; }
  h->prof_base = event_base < 0 ? -1 : event_base;
  return OFX_OK;
}
