/*
 * ofx.h - C-ABI of the MI355X-native batched Ofighters arena engine.
 *
 * This is the drop-in boundary for the hot path named in BASELINE.json
 * (north_star): Battleground.frame() = request_actions -> generate_frame ->
 * Observation(battleground) for thousands of independent arenas in lock-step,
 * plus the policy forwards.  The reference has no FFI of its own (it is pure
 * Python); each entry point below cites the reference interface it replaces
 * (paths relative to /root/reference/ofighters).  INTEGRATION.md shows the
 * ctypes stub a maintainer of the reference would add.
 *
 * Conventions
 *  - extern "C", plain pointers and sizes only; no C++ / torch types.
 *  - Every bulk pointer is a DEVICE (HBM) pointer unless the name ends in
 *    `_host`.  ofx_malloc/ofx_free/ofx_memcpy_* let a host without torch own
 *    device buffers; a torch tensor's data_ptr() is equally valid.
 *  - All kernels are enqueued on the handle's HIP stream and return
 *    immediately; ofx_sync() waits.  Entry points that copy to `_host`
 *    pointers synchronise the stream themselves.
 *  - Return value: 0 = OFX_OK, <0 = error; ofx_last_error() returns the
 *    thread-local message (the reference raises bare Exception(msg):
 *    lib/battleground.py:30, lib/action.py:40,63, agents/agent.py:51).
 *  - There is NO CPU fallback in this library: without a HIP device every
 *    compute entry point fails with OFX_ERR_NO_DEVICE.
 *  - A handle is thread-compatible, not thread-safe (the reference is single
 *    threaded: lib/ofighters.py:697).
 */
#ifndef OFX_H
#define OFX_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define OFX_VERSION 1

enum {
  OFX_OK = 0,
  OFX_ERR_INVALID = -1,   /* bad argument / config                         */
  OFX_ERR_NO_DEVICE = -2, /* no HIP device: there is no CPU fallback       */
  OFX_ERR_HIP = -3,       /* a HIP runtime call failed (message has detail) */
  OFX_ERR_STATE = -4,     /* call order violated (e.g. step before spawn)  */
  OFX_ERR_OVERFLOW = -5   /* laser capacity exceeded since the last check  */
};

/* One POD with the reference's module-level constants as defaults
 * (ofx_default_config fills them in):
 *   width/height 400           lib/observation.py:10-11
 *   ship_radius 8, hull 1      lib/ship.py:43-45
 *   laser_radius 2             lib/laser.py:23
 *   ship_speed 8               lib/ship.py:24
 *   laser_speed 10 * LIGHT 1   lib/ship.py:86, lib/laser.py:13,24
 *   rewards death 0 kill 0 aim 2 trajectory 1   agents/qlearnIA_V2.py:39-44
 *   episode_ticks 200          lib/ofighters.py:59 (MAX_TIME)               */
typedef struct ofx_config {
  int32_t n_arenas;     /* N  arenas advanced in lock-step on this device   */
  int32_t n_ships;      /* M  ships per arena, 1..64                        */
  int32_t laser_cap;    /* L  laser slots per arena (multiple of 64)        */
  int32_t width, height;
  int32_t ship_radius, laser_radius;
  int32_t ship_speed, laser_speed;
  int32_t reward_death, reward_kill, reward_aim, reward_trajectory;
  int32_t episode_ticks;
  int32_t device;       /* HIP device ordinal                               */
  int32_t arena_base;   /* global id of local arena 0 (multi-GPU sharding:
                           keys the counter RNG so results do not depend on
                           the number of GPUs)                              */
} ofx_config;

/* One ship's action for one tick == lib/action.py:12-56 Action
 * (shoot, thrust, pointing) ; valid==0 is the reference's `None`
 * (lib/ship.py:308: no-op).  Array layout [N][M].                           */
typedef struct ofx_action {
  int32_t px, py;
  uint8_t shoot, thrust, valid, _pad;
} ofx_action;

/* scripted behaviours of agents/agent.py:38-51 (+ "none" = always None)     */
enum {
  OFX_BOT_IDLE = 0,   /* idlebot          agent.py:99-104  */
  OFX_BOT_RANDOM = 1, /* random_play      agent.py:123-133 */
  OFX_BOT_TURRET = 2, /* crazy_turret     agent.py:136-144 */
  OFX_BOT_RUNNER = 3, /* crazy_runner     agent.py:147-155 */
  OFX_BOT_THRUST = 4, /* never_back_down  agent.py:107-112 */
  OFX_BOT_SHOOT = 5   /* mass_shooter     agent.py:115-120 */
};

/* state fields readable through ofx_get_host / ofx_device_ptr               */
enum {
  OFX_F_SHIP_X = 0,      /* int32 [N][M]   Ship.body.x            ship.py:43   */
  OFX_F_SHIP_Y = 1,      /* int32 [N][M]                                       */
  OFX_F_SHIP_PX = 2,     /* int32 [N][M]   Ship.pointing.x        ship.py:53   */
  OFX_F_SHIP_PY = 3,     /* int32 [N][M]                                       */
  OFX_F_SHIP_ALIVE = 4,  /* uint8 [N][M]   Ship.is_playable()     ship.py:108  */
  OFX_F_REWARD = 5,      /* int32 [N][M]   Agent.reward           agent.py:25  */
  OFX_F_SCORE = 6,       /* int32 [N][M]   Agent.score            agent.py:23  */
  OFX_F_N_LASERS = 7,    /* int32 [N]      len(Battleground.lasers)            */
  OFX_F_LASER_X = 8,     /* float64 [N][L] Laser.body.x           laser.py:23  */
  OFX_F_LASER_Y = 9,     /* float64 [N][L]                                     */
  OFX_F_LASER_OWNER = 10,/* uint8 [N][L]   index of Laser.owner in ships       */
  OFX_F_LASER_DEAD = 11, /* uint8 [N][L]   Laser.state=="destroyed" laser.py:66 */
  OFX_F_KILLER = 12,     /* int16 [N][M]   list index of the laser that killed
                            the ship THIS tick, -1 otherwise (laser.py:52-60) */
  OFX_F_TIME = 13,       /* int32 [N]      Battleground.time  battleground.py:154 */
  OFX_F_LAST_SCORES = 14,/* int32 [N][M]   Agent.scores[-1]       agent.py:62  */
  OFX_F_HULL = 15,       /* int32 [N][M]   Ship.hull              ship.py:45,129 */
  OFX_F_LASER_DX = 16,   /* float64 [N][L] per-tick displacement  laser.py:45  */
  OFX_F_LASER_DY = 17,   /* float64 [N][L]                                     */
  OFX_F_OBS_REWARD = 18, /* int32 [N][M]   reward as seen by Agent.step this
                            tick (obs.reward, observation.py:103)             */
  OFX_F_COUNT = 19
};

/* observation map element types for ofx_rasterise                           */
enum {
  OFX_MAP_U8 = 0,   /* 1 byte / cell  (default; 320 000 B per arena)         */
  OFX_MAP_F32 = 1,
  OFX_MAP_F64 = 2,  /* the reference's dtype (observation.py:86,91)          */
  OFX_MAP_BITS = 3  /* 1 bit / cell, MSB-first per byte == numpy.packbits;
                       row stride = ceil(W/8)*... see ofx_map_bytes          */
};

typedef struct ofx_handle ofx_handle;

/* ---- library ---------------------------------------------------------- */
int ofx_version(void);
const char *ofx_last_error(void);
int ofx_device_count(void); /* 0 when no HIP device is visible              */
void ofx_default_config(ofx_config *cfg);

/* ---- device memory helpers (host side needs no torch) ------------------ */
int ofx_malloc(void **dev_ptr, size_t bytes);
int ofx_free(void *dev_ptr);
int ofx_memcpy_h2d(void *dst_dev, const void *src_host, size_t bytes);
int ofx_memcpy_d2h(void *dst_host, const void *src_dev, size_t bytes);

/* ---- lifetime ----------------------------------------------------------
 * replaces Battleground.__init__ (lib/battleground.py:13-106) for N arenas   */
int ofx_create(const ofx_config *cfg, ofx_handle **out);
int ofx_destroy(ofx_handle *h);
int ofx_sync(ofx_handle *h);
void *ofx_stream(ofx_handle *h);             /* the hipStream_t of the handle */
int ofx_set_stream(ofx_handle *h, void *hip_stream); /* adopt caller's stream */

/* ---- spawn / restart ---------------------------------------------------
 * ofx_spawn: ships at draws[N][M][2] (x,y), pointing = position, alive,
 *   reward = score = 0, no lasers            (battleground.py:79-81, ship.py:35-58)
 * ofx_restart: Battleground.restart (battleground.py:108-117) -> Ship.reset
 *   (ship.py:92-106) -> Agent.reset (agent.py:59-64) with their quirks:
 *   pointing = OLD position, `x or old` keeps the coordinate when the draw is 0,
 *   hull not restored, reward NOT cleared, score appended then zeroed.
 *   arena_mask[N] (uint8, may be NULL = all) selects the arenas to restart.
 * draws are the reference's randint(0, dim) values (inclusive: may equal W/H). */
int ofx_spawn(ofx_handle *h, const int32_t *draws);
int ofx_restart(ofx_handle *h, const int32_t *draws, const uint8_t *arena_mask);
/* same, draws generated on device by the counter RNG (seed, episode)         */
int ofx_spawn_random(ofx_handle *h, uint64_t seed);
int ofx_restart_random(ofx_handle *h, uint64_t seed, uint32_t episode);

/* ---- per-arena episodes (opt-in): restart an arena when its own episode is over ---------
 * Every vectorised RL environment restarts a sub-environment when ITS episode ends; ofx_restart* restart on a clock the
 * caller keeps for all arenas.  ofx_restart_finished is the device-side rule, called once per decision at the head of
 * the lock-step - where the caller's episode-end check stands, before ofx_bot_actions and the forward.  One kernel (wave
 * per arena, lane = ship, the decision one ballot, no block barrier), enqueued on the handle's stream; does not
 * synchronise.  All pointers are DEVICE pointers.
 * Handle-owned state, allocated and zeroed by the first call (or by ofx_autoreset_set_state), freed by ofx_destroy:
 *   arena_episode uint32 [N], dead_once uint8 [N][M], restarted uint8 [N] (the arenas the LAST call restarted).
 * The rule, per arena a:
 *  - ship i is selected when ship_mask[a][i] != 0 (uint8 [N][M]); ship_mask == NULL selects every ship.
 *  - a selected ship that is not alive is FINISHED iff dead_once[a][i] was already set; otherwise the call sets
 *    dead_once[a][i] and the ship is not finished yet.  A destroyed ship is therefore finished on the SECOND call that
 *    sees it dead: between the two the caller's one lock-step captured the losing frame (done = 1) and latched the agent,
 *    the reference's order (agents/qlearnIA_V2.py:376-391).
 *  - the arena restarts iff at least one ship is selected and every selected ship is finished, or
 *    max_ticks > 0 && OFX_F_TIME[a] >= max_ticks (max_ticks == 0: no clock).
 * A restart: arena_episode[a] += 1; every ship of the arena gets exactly ofx_restart's treatment, quirks included, on
 * the draws of ofx_restart_random(seed, arena_episode[a]) for that arena - Philox counter (global arena, ship,
 * arena_episode[a]), the reset stream; with sums != NULL and g = group ? group[a] : 0 inside [0, n_groups):
 * sums[g][i] += the score banked, sums[g][M] += 1, sums[g][M+1] += OFX_F_TIME[a] before it is zeroed (the episode's
 * length in lock-steps) - sums is the caller's int64 [n_groups][M+2], added to with 64-bit atomics and zeroed by the
 * caller, ofx_episode_scores' sums are not touched; dead_once[a][*] = 0; seen[a][*] = 0 when seen (uint8 [N][M], the
 * latch array of ofx_agents_first_done) is given; and, while a replay memory exists, the arena's agents forget
 * previous_* and their done latch as at ofx_restart.  An arena that does not restart changes in dead_once alone.
 * ofx_spawn* zero arena_episode and dead_once; ofx_restart* clear dead_once of the arenas they restart and leave
 * arena_episode alone.
 * OFX_ERR_INVALID: NULL handle, max_ticks < 0, n_groups < 1 or > N, group without sums; OFX_ERR_STATE before ofx_spawn.
 * ofx_autoreset_state_host reads the state (any pointer may be NULL; synchronises), ofx_autoreset_set_state writes
 * arena_episode and dead_once from the host for a checkpoint (NULL: that array stays; allocates; synchronises).  The
 * reader returns OFX_ERR_STATE while nothing is allocated, the setter before ofx_spawn.                              */
int ofx_restart_finished(ofx_handle *h, uint64_t seed, const uint8_t *ship_mask, int32_t max_ticks, uint8_t *seen,
                         const int32_t *group, int32_t n_groups, int64_t *sums);
int ofx_autoreset_state_host(ofx_handle *h, uint32_t *episode_host, uint8_t *dead_once_host, uint8_t *restarted_host);
int ofx_autoreset_set_state(ofx_handle *h, const uint32_t *episode_host, const uint8_t *dead_once_host);
/* The restart of ofx_restart_finished, decided by the caller: every arena with arena_mask[a] != 0 (DEVICE uint8 [N],
 * NULL = all) restarts, whatever its ships and its clock say.  For such an arena arena_episode[a] += 1, every ship gets
 * ofx_restart's treatment, quirks included, on the draws of counter (global arena, ship, arena_episode[a]), and
 * dead_once[a][*] = 0; nothing is summed and there is no `seen`.  restarted[a] = (arena_mask[a] != 0) is written for
 * EVERY arena; an arena that is not selected changes in nothing else.  Allocates the state above like
 * ofx_restart_finished, and like it ends by making the restarted arenas' agents forget previous_* while a replay memory
 * exists.  One kernel of ofx_restart_finished's shape; does not synchronise.
 * OFX_ERR_INVALID: NULL handle; OFX_ERR_STATE before ofx_spawn.                                                       */
int ofx_restart_arenas(ofx_handle *h, uint64_t seed, const uint8_t *arena_mask);

/* ---- the tick ----------------------------------------------------------
 * ofx_step = Agent.step bookkeeping for every ship, dead included
 *            (score += reward; reward = 0: agents/agent.py:66-74, ship.py:260-262)
 *          + GUI laser clean-up of lasers destroyed in the previous tick
 *            (lib/ofighters.py:619-625,702-707)
 *          + Battleground.generate_frame(actions) (battleground.py:153-160):
 *            Laser.move for every laser in list order (laser.py:36-62), then
 *            Ship.move(action) in index order (ship.py:303-339: pointing,
 *            thrust ship.py:213-222, shoot ship.py:134-156 + form.py:159-188,
 *            aim / trajectory rewards ship.py:158-210).
 * actions: device [N][M] ofx_action.                                         */
int ofx_step(ofx_handle *h, const ofx_action *actions);

/* ---- observation -------------------------------------------------------
 * ofx_rasterise = Observation.analyse_battleground (lib/observation.py:79-95)
 *   with Circle.binary_draw -> skimage.draw.disk((y,x), r, shape) arithmetic
 *   (lib/form.py:222-228; scikit-image 0.18.3 draw.py:11-43,46-143).
 *   Maps are [N][W rows = y][H cols = x]; playable ships (r=ship_radius) into
 *   ship_map, every listed laser incl. just-destroyed (r=laser_radius) into
 *   laser_map.  NULL output pointers select the handle's internal buffers
 *   (see ofx_map_ptr).
 * ofx_observe_head = Observation.analyse_ship + toVector head
 *   (observation.py:101-123): float64 [N][M][8] =
 *   reward, can_shoot(1), pointing.x, pointing.y, dim.x, dim.y, pos.x, pos.y;
 *   done[N][M] uint8 = not playable (may be NULL).                           */
int ofx_rasterise(ofx_handle *h, int map_type, void *ship_map, void *laser_map);
size_t ofx_map_bytes(const ofx_handle *h, int map_type); /* bytes of ONE arena's ONE map */
void *ofx_map_ptr(ofx_handle *h, int map_type, int which /*0 ship,1 laser*/);
int ofx_observe_head(ofx_handle *h, double *head, uint8_t *done);

/* ---- scripted bots on device -------------------------------------------
 * behaviours[M] (host, OFX_BOT_*) ; actions out device [N][M].  Draws come
 * from Philox4x32-10 keyed by (seed) with counter (global arena, ship, tick),
 * so any GPU count reproduces the same stream.  Same action LAW as
 * agents/agent.py:99-155 (not the Mersenne-Twister stream).                  */
int ofx_bot_actions(ofx_handle *h, const int32_t *behaviours_host, uint64_t seed,
                    uint32_t tick, ofx_action *actions);

/* ---- the headless loop ---------------------------------------------------
 * Battleground.run (lib/battleground.py:169-173) for arenas flown by the scripted bots: n_ticks lock-steps of
 * request_actions (the ofx_bot_actions law, counter ticks tick0 .. tick0 + n_ticks - 1) -> generate_frame (ofx_step)
 * -> Observation(battleground) (ofx_rasterise into the handle's maps of observe_map_type, or -1 = no maps) enqueued by
 * ONE host call; state afterwards is bit-identical to n_ticks x (ofx_bot_actions, ofx_step[, ofx_rasterise]).  The
 * bots' law is evaluated inside the step kernel, and without an observer between them all n_ticks lock-steps run
 * inside one launch (an arena belongs to one wavefront for the whole launch).  Episode ends stay with the caller
 * (ofx_restart* between two calls).  With ofx_policy_profile switched on, one event pair brackets the call's
 * dominant kernel (the K-tick step launch, or the last lock-step's rasteriser).                                  */
int ofx_rollout(ofx_handle *h, const int32_t *behaviours_host, uint64_t seed, uint32_t tick0, int32_t n_ticks,
                int32_t observe_map_type);

/* ---- action repeat (opt-in): K lock-steps per decision in one launch ---------
 * Mnih et al. 2015's frame skip for a learning agent: n_ticks >= 1 lock-steps in ONE launch of the step kernel's third
 * form (wave per arena, no block barrier, the wavefront fence of ofx_rollout between lock-steps).
 *  - hold_mask: DEVICE uint8 [N][M] or NULL (nobody).  A ship with hold_mask[a][i] != 0 plays actions[a][i] (DEVICE
 *    [N][M] ofx_action, e.g. what ofx_policy_actions wrote; loaded once, before the first lock-step) on EVERY lock-step
 *    of the launch under ofx_step's own rule `valid && alive`, alive being the ship's CURRENT state: a ship destroyed
 *    inside the span stops acting, an action with valid = 0 never acts.  Its behaviours entry is not used (it must still
 *    be an OFX_BOT_* value).  Every other ship follows the ofx_bot_actions law of lock-step tick0 + j, as in ofx_rollout.
 *  - span_reward: DEVICE int32 [N][M] or NULL; receives for EVERY ship, held or not, dead or not, the sum over the
 *    launch's lock-steps of the reward earned in that lock-step (the value each lock-step leaves in OFX_F_REWARD; the
 *    state keeps only the last one, the earlier ones are in OFX_F_SCORE).  Undiscounted.  See ofx_replay_reward_source.
 *  - observe_map_type: as in ofx_rollout, but the maps are rasterised ONCE, after the last lock-step; -1 = none.
 * The state afterwards - every field, the lasers - is bit-identical to n_ticks x (ofx_bot_actions(tick0 + j), the held
 * ships' entries overwritten by `actions`, ofx_step); span_reward is the sum of OFX_F_REWARD read after each of those
 * steps, the maps are the last step's ofx_rasterise.  With hold_mask == NULL the state is that of ofx_rollout(...,
 * n_ticks, -1).  OFX_ERR_INVALID: NULL handle or behaviours, n_ticks < 1, hold_mask without actions; OFX_ERR_STATE
 * before ofx_spawn.  Keeps the behaviours on the device like ofx_rollout.  Does not synchronise.                    */
int ofx_step_repeat(ofx_handle *h, const int32_t *behaviours_host, uint64_t seed, uint32_t tick0, int32_t n_ticks,
                    const uint8_t *hold_mask, const ofx_action *actions, int32_t *span_reward,
                    int32_t observe_map_type);

/* ---- state access ------------------------------------------------------ */
int ofx_get_host(ofx_handle *h, int field, void *dst_host, size_t bytes);
void *ofx_device_ptr(ofx_handle *h, int field);
size_t ofx_field_bytes(const ofx_handle *h, int field);
/* ---- zero-copy views of the handle's arrays -----------------------------
 * The reference's plugin seam is "any object with .play(obs)" (agents/agent.py:34-37); its learning agent reads
 * obs.ship_map / obs.laser_map / obs.vector[:8] and answers an Action (agents/qlearnIA_V2.py:206-220,447-454).  For a
 * batch the same seam is an EXTERNAL POLICY that reads the maps and the state of all N x M ships where they lie in HBM
 * and writes its [N][M] ofx_action array there: ofx_field_desc / ofx_map_desc describe a handle-owned array (pointer,
 * element type, shape, strides in elements, device) so that a host framework can wrap it WITHOUT a copy - a DLPack
 * capsule, __cuda_array_interface__, torch.as_tensor (ofighters_amd/engine.py: ArenaBatch.tensor / maps_tensor).
 * Ownership: the memory belongs to the handle and lives until ofx_destroy; the CONTENTS of a state field are
 * those of the last ofx_step / ofx_restart* / ofx_spawn*, of a map those of the last ofx_rasterise of that type, and the
 * next such call overwrites them in place.  Everything runs on ofx_stream(h): read and write the views on that stream
 * (or order yours against it), never concurrently with an entry point that writes them.                            */
enum { OFX_DT_U8 = 0, OFX_DT_I16 = 1, OFX_DT_I32 = 2, OFX_DT_I64 = 3, OFX_DT_F32 = 4, OFX_DT_F64 = 5 };
typedef struct ofx_tensor_desc {
  void *data;          /* device pointer                                    */
  int32_t dtype;       /* OFX_DT_*                                          */
  int32_t itemsize;    /* bytes per element                                 */
  int32_t ndim;        /* 1..4                                              */
  int32_t device;      /* HIP device ordinal of the handle                  */
  int64_t shape[4];
  int64_t stride[4];   /* in elements; dense row-major                      */
} ofx_tensor_desc;
/* state field `field` (OFX_F_*): [N][M], [N][L] or [N]                      */
int ofx_field_desc(ofx_handle *h, int field, ofx_tensor_desc *out);
/* map `which` (0 ship, 1 laser) of `map_type`: [N][W rows = y][H cols = x] of uint8 / float32 / float64, or
 * [N][W*H/8] uint8 for OFX_MAP_BITS; the handle's internal buffer (allocated at the first ofx_rasterise of that type
 * with NULL outputs, or here)                                               */
int ofx_map_desc(ofx_handle *h, int map_type, int which, ofx_tensor_desc *out);

/* number of lasers dropped because an arena's list was full since the last
 * call (never silent truncation); resets the counter.  "Since the last call"
 * is per process: a checkpoint does not carry the counter over.              */
int ofx_overflow_count(ofx_handle *h, int64_t *count_host);

/* ---- episodic scores (the only cross-GPU quantity) ----------------------
 * Writes int64 [M+1] to a DEVICE buffer: sum over local arenas of the score
 * each ship slot banked at the most recent ofx_restart (Agent.reset:
 * scores.append(score), agents/agent.py:61-63) and, last, the arena count.
 * The caller all-reduces it (RCCL via torch.distributed).                    */
int ofx_episode_scores(ofx_handle *h, int64_t *sums);
/* The same per group of arenas (opt-in: the score of each rung of an exploration ladder, or of the greedy evaluation
 * arenas, next to the shard's total).  group: DEVICE int32 [N], the group of every local arena; sums: DEVICE int64
 * [n_groups][M+1]: sums[g][i] = the sum of OFX_F_LAST_SCORES[a][i] over the local arenas with group[a] == g, and
 * sums[g][M] = the number of those arenas.  group[a] == -1 leaves arena a out; a value outside [-1, n_groups) is
 * ignored like -1.  Integer sums: exact in any summation order, so with every arena in a group the sum over g equals
 * ofx_episode_scores.  Enqueued on the handle's stream, does not synchronise.  OFX_ERR_INVALID: a NULL pointer,
 * n_groups < 1 or n_groups > N.                                                                                    */
int ofx_episode_scores_grouped(ofx_handle *h, const int32_t *group, int32_t n_groups, int64_t *sums);
/* The same followed by the all-reduce itself, for a host that is not torch: ncclAllReduce(sum, int64, in place) of the
 * [M+1] vector over the ranks of `nccl_comm` - an ncclComm_t the caller made with ncclCommInitRank, one rank per GPU
 * (RCCL over xGMI) - enqueued on the handle's stream.  libofx.so does not link RCCL; the symbol is resolved in the
 * process (or librccl.so.1 is opened) at the first call.  SURVEY 8b / 8e: the only collective of the path.          */
int ofx_scores_allreduce(ofx_handle *h, void *nccl_comm, int64_t *sums);

/* ---- scratch MLP forward -----------------------------------------------
 * Neural_network.feed (agents/neural_network.py:396-420): a <- sigmoid(W a + b)
 * per layer, float64, column vectors.  layers_host[n_layers] sizes;
 * weights: concatenated row-major W_i (n_{i+1} x n_i); biases concatenated;
 * x [batch][layers[0]] ; y [batch][layers[-1]] ; argmax int32 [batch] may be
 * NULL (Neural_network.max_sol_index, neural_network.py:423-429).            */
int ofx_scratch_feed(ofx_handle *h, const int32_t *layers_host, int32_t n_layers,
                     const double *weights, const double *biases, const double *x,
                     int32_t batch, double *y, int32_t *argmax);
/* same network fed with the live observation vector of every (arena, ship)
 * (toVector order, observation.py:119-125; needs layers[0] == 8 + 2*W*H):
 * the binary map tail is consumed as a sparse gather of W_1 columns.
 * y [N][M][layers[-1]].  layers[1] <= 2048: the gather keeps 32 * layers[1]
 * bytes in LDS; a wider first layer returns OFX_ERR_INVALID with a message
 * naming the limit, before anything is enqueued.                             */
int ofx_scratch_feed_obs(ofx_handle *h, const int32_t *layers_host, int32_t n_layers,
                         const double *weights, const double *biases, double *y,
                         int32_t *argmax);

/* ---- neuroevolution of the scratch MLP (opt-in): a genome per ship --------------------------
 * The reference's second learner: the scratch network above with a genetic algorithm around it - Neural_network.generate /
 * evolution / mutate / reproduce / dafts (agents/neural_network.py:436-478), one network per ship
 * (lib/battleground.py:52-76), the four-sigmoid decode of agents/brAIn.py:129-134.  A handle holds ONE population of P
 * genomes of the topology layers_host[n_layers], resident in HBM; ofx_destroy frees it.  All sizes and element offsets
 * are 64-bit (P x elements passes 2^31 at 746 genomes of [320008, 9, 4]).
 * ofx_population_create refuses, each with a message (OFX_ERR_INVALID): layers[0] != 8 + 2*W*H; layers[-1] != 4 (the
 * reference's Action.size); fewer than 2 or more than 8 layers; a layer after the input wider than 64 (a ship's
 * activations stay in one workgroup's LDS); P < 1.  A handle that already holds a population: OFX_ERR_STATE.  An
 * allocation that fails: OFX_ERR_HIP, the message names the bytes asked for.
 * ELEMENTS.  ofx_population_get / _set move genome `p` in ofx_scratch_feed's layout: every W_l row-major
 * [n_{l+1}][n_l], layer by layer, then every bias - weights_layers + biases_layers of the reference.  A genome's ELEMENT
 * INDEX e is the position in that concatenation, weights first; every random draw below is keyed by it, and an exported
 * genome can be handed to ofx_scratch_feed_obs unchanged.  (On the device the first layer is kept input-major: the n1
 * weights of one input are contiguous.  DESIGN.md section 3.)  Both calls synchronise.
 * DRAWS.  u(r_hi, r_lo) = ((r_hi >> 5) * 2^26 + (r_lo >> 6)) / 2^53 from two Philox words: numpy's 53-bit double in
 * [0, 1), exact in float64.  Words come from Philox4x32-10 keyed by `seed` with counter (slot p, e, generation, stream);
 * the streams are 9 (evolve: words 0, 1 the coefficient, words 2, 3 the mutation selector), 10 (the replacement value of
 * a mutated element, words 0, 1) and 11 (a fresh genome, words 0, 1).
 * ofx_population_init writes 2 u - 1 on stream 11 to every element of every slot: Neural_network.__init__'s U[-1, 1)
 * (neural_network.py:108-111), the same law on the project's counter stream.  Does not synchronise.                   */
int ofx_population_create(ofx_handle *h, const int32_t *layers_host, int32_t n_layers, int64_t P);
int ofx_population_destroy(ofx_handle *h);
int ofx_population_init(ofx_handle *h, uint64_t seed, uint32_t generation);
int ofx_population_get(ofx_handle *h, int64_t p, double *weights_host, double *biases_host);
int ofx_population_set(ofx_handle *h, int64_t p, const double *weights_host, const double *biases_host);
/* Reproduction in place.  plan_host: HOST int32 [P], the fate of each slot:
 *   plan[p] == p        kept, not one bit changed
 *   plan[p] == q != p   the slot becomes a child of q, and q must itself be kept (plan[q] == q)
 *   plan[p] == -1       a fresh genome, as in dafts: stream 11 at this `generation`
 * The whole plan is checked before any launch; a value outside [-1, P) or a parent that is not kept returns
 * OFX_ERR_INVALID with nothing written.  Sources are never destinations, so there is no second buffer.
 * A child is deepcopy(parent).evolution(rate).mutate(rate) (neural_network.py:436-467), per element e of slot p with the
 * stream-9 words r0..r3 of counter (p, e, generation, 9):
 *   w = parent[e]
 *   evolution_rate > 0:                                   c = (2 u(r0, r1) - 1) * evolution_rate;  w = c * w + w
 *                                                         (three separately rounded float64 operations, no FMA)
 *   mutation_rate > 0 and u(r2, r3) < mutation_rate:      w = 2 u(s0, s1) - 1, s = the stream-10 words of (p, e, generation)
 * A rate <= 0 skips its step.  One kernel, one pass.  Does not synchronise (the plan is copied before the call returns). */
int ofx_population_breed(ofx_handle *h, const int32_t *plan_host, double evolution_rate, double mutation_rate,
                         uint64_t seed, uint32_t generation);
/* The forward with a genome per ship.  genome_of: DEVICE int32 [N][M], -1 = this ship is not evolved; actions: DEVICE
 * [N][M] ofx_action, updated in place; y: DEVICE float64 [N][M][4] or NULL.  Rasterises the handle's 1-bit maps as
 * ofx_scratch_feed_obs does; then, in one launch, for every LIVE ship with 0 <= genome_of < P: Neural_network.feed with
 * that genome on the ship's live observation vector (toVector order: the 8-scalar head of ofx_observe_head, then the two
 * binary maps, consumed sparsely), and the reference's decode of a four-sigmoid output with the arena's size in place of
 * 400: shoot = y0 > 0.5, thrust = y1 > 0.5, px = (int)(y2 * W), py = (int)(y3 * H), valid = 1; no clamp, as there.
 * Entries (actions and y) of dead, unassigned or out-of-range ships are NOT written: run ofx_bot_actions first, this
 * call overwrites the evolved ships the way ofx_policy_actions does.  Fixed summation order, no floating-point
 * atomics: the same bits on every call.  Does not synchronise.                                                       */
int ofx_population_act(ofx_handle *h, const int32_t *genome_of, ofx_action *actions, double *y);
/* Fitness.  sum: DEVICE int64 [P], count: DEVICE int32 [P].  After a restart: sum[g] += OFX_F_LAST_SCORES of every
 * (arena, ship) with genome_of == g, count[g] += 1; reset != 0 zeroes both first.  Integer atomics: exact in any order.
 * Does not synchronise.                                                                                              */
int ofx_population_fitness(ofx_handle *h, const int32_t *genome_of, int64_t *sum, int32_t *count, int32_t reset);
/* A learning step per genome: Neural_network.backprop (agents/neural_network.py:338-393) and the step of update_network
 * (:241-300) / update_network_continuous (:319-334), for every genome on its own ships' observations, on the device.
 * All pointers are DEVICE pointers.  genome_of: int32 [N][M] as in ofx_population_act; solution: float64 [N][M][4], the
 * target output; learn_mask: uint8 [N][M] or NULL (= all ones); actions: [N][M] ofx_action or NULL; y: float64 [N][M][4]
 * or NULL; err: float64 [N][M] or NULL.  Rasterises the handle's 1-bit maps as ofx_population_act does.
 * SAMPLES.  A ship is a sample iff it is alive, 0 <= genome_of < P and its mask entry is nonzero.  The samples of genome
 * g in ascending flat index a*M + i are j_1 < ... < j_n; two ships of one arena on the same genome are two samples.
 * FORWARD OUTPUTS.  For every live assigned ship, sample or not, actions and y get what ofx_population_act would have
 * written from the weights BEFORE this call, bit for bit (the same device code); dead, unassigned and out-of-range
 * entries are not written.  One forward per lock-step is enough: this call stands where the acting call stood.
 * GRADIENT.  Per sample, with the OLD weights of its genome and the forward's z_l, a_l (the same bits):
 *   d = solution - a_L;  delta_L[o] = d[o] * (a_L[o] * (1 - a_L[o]))
 *   l = L-1 .. 1:  delta_l[k] = (sum over o ascending of W_{l+1}[o][k] * delta_{l+1}[o]) * (a_l[k] * (1 - a_l[k]))
 * every product and sum rounded on its own (no FMA).  The reference's sigmoid_prime(z) recomputes sigmoid(z): the same
 * function of the same input, so a (1 - a) is the same number.  err[j] = d0^2 + d1^2 + d2^2 + d3^2, added in that
 * order, for samples only.
 * APPLY.  c = rate / (double)n; for j = j_1 .. j_n in that order
 *   W_l[o][k] <- W_l[o][k] + (c * delta_{l,j}[o]) * a_{l-1,j}[k]        b_l[o] <- b_l[o] + c * delta_{l,j}[o]
 * In the first layer a map input is 0 or 1: at a set cell the element becomes w + c * delta_1[o], at an unset cell it is
 * NOT written (an update touches set cells x n1 doubles of a genome, not all of it); the 8 head inputs are ordinary
 * doubles.  A genome with n = 0 keeps every bit.  rate == 0 skips the apply; the forward outputs and err are written.
 * This is update_network's step on the average gradient scaled by `rate`: rate = 1 is update_network, n = 1 is
 * update_network_continuous(obs, sol, rate).  ONE DIFFERENCE: the reference sums the per-sample terms, divides and adds
 * the sum to the weight once; here each sample's term is added to the weight one after the other, which differs in the
 * last bits only and lets the sparse first layer go without an accumulator the size of a genome.
 * No floating-point atomics: the same state gives the same bits on every call.  Refused, each with a message and before
 * anything is enqueued: no population (OFX_ERR_STATE); genome_of or solution NULL, rate not finite (OFX_ERR_INVALID).
 * Two launches (every delta of a genome's samples comes from the old weights).  Does not synchronise.                */
int ofx_population_learn(ofx_handle *h, const int32_t *genome_of, const double *solution, const uint8_t *learn_mask,
                         double rate, ofx_action *actions, double *y, double *err);
/* The teacher's action as a target, for every (arena, ship); teacher: DEVICE [N][M] ofx_action (what ofx_bot_actions
 * wrote), solution: DEVICE float64 [N][M][4], mask: DEVICE uint8 [N][M].
 *   solution = (shoot ? 1 : 0, thrust ? 1 : 0, clamp((px + 0.5) / W, 0, 1), clamp((py + 0.5) / H, 0, 1))
 *   mask = teacher.valid != 0
 * The inverse of ofx_population_act's decode: for 0 <= px < W the decode of the target gives px back.  OFX_ERR_INVALID
 * for a NULL pointer.  Does not synchronise.                                                                          */
int ofx_population_targets(ofx_handle *h, const ofx_action *teacher, double *solution, uint8_t *mask);
/* The imitation log's reduction.  err: DEVICE float64 [N][M], acc: DEVICE float64 [2].  acc[0] += the entries of err that
 * are >= 0, acc[1] += their number; every entry of err is then set to -1 ("no sample": ofx_population_learn writes the
 * samples' entries only, and an err is never negative).  One workgroup, a fixed order of additions: the same bits every
 * call.  OFX_ERR_INVALID for a NULL pointer.  Does not synchronise.                                                   */
int ofx_population_err_reduce(ofx_handle *h, double *err, double *acc);

/* ---- evolution strategies (opt-in): a population that is never stored ------------------------
 * Not in the reference.  Salimans, Ho, Chen, Sidor, Sutskever 2017, "Evolution Strategies as a Scalable Alternative to
 * Reinforcement Learning" (OpenAI-ES) with mirrored sampling: ONE centre genome theta, and every member of the population
 * is theta +- sigma * eps with eps a pure function of (seed, pair, element, generation).  Nothing of a member is stored:
 * the forward regenerates the noise of the rows it gathers, the generation step is one pass over theta, and a population
 * of any P costs one genome of HBM.  Selection and breeding become a rank-weighted gradient step.
 * STATE.  A handle may hold one ES centre, independent of its population (both may exist at once): one genome of G
 * float64 of the topology layers_host[n_layers], in the storage layout of the neuroevolution section (first layer
 * input-major); ofx_destroy frees it.  ofx_es_create refuses what ofx_population_create refuses, with the same messages
 * (there is no P here); a handle that already holds a centre: OFX_ERR_STATE.
 * ELEMENTS.  The element index e is exactly that of the neuroevolution section: an exported centre or member can be
 * handed to ofx_population_set and ofx_scratch_feed_obs unchanged.
 * NOISE.  r0..r3 = the Philox4x32-10 words of counter (pair i, e, generation, 12), keyed by `seed` (stream 12,
 * OFX_ES_STREAM).  S = r0 + r1 + r2 + r3 as an integer, and
 *   eps(i, e) = (double)(S - (2^33 - 2)) * 2^-32
 * an Irwin-Hall sum of four uniforms: bell-shaped, bounded to (-2, 2), and EXACTLY symmetric - complementing the four
 * words negates eps.  Every step is exact in float64 (|S - (2^33 - 2)| < 2^34), so device and numpy agree to the bit
 * with no libm in play.  Its variance is (1 - 2^-64) / 3: sigma and the learning rate are in units of THIS eps, not of
 * a unit normal (a unit-variance sigma is sigma * sqrt(3) here).
 * MEMBERS.  P = 2 * n_pairs.  Member m = 2 i + b has sign s = +1 for b = 0 and -1 for b = 1, and its element is
 *   w_m[e] = theta[e] + (s * sigma) * eps(i, e)
 * the product rounded, then the sum rounded, no FMA.  Member index P is the centre itself, w = theta[e] (evaluation).
 * Every layer and every bias is perturbed.
 * REFUSALS, each with a message and before anything is enqueued: no centre (OFX_ERR_STATE); P odd or < 2; sigma not
 * finite or <= 0; scale or any d[i] not finite; a NULL pointer; member outside [0, P] (OFX_ERR_INVALID).            */
int ofx_es_create(ofx_handle *h, const int32_t *layers_host, int32_t n_layers);
int ofx_es_destroy(ofx_handle *h);
/* The centre becomes the fresh genome of slot 0: stream 11, the law (and the kernel) of ofx_population_init.  Does not
 * synchronise.                                                                                                       */
int ofx_es_init(ofx_handle *h, uint64_t seed, uint32_t generation);
/* The centre in the element order, as ofx_population_get / _set move a slot.  Both synchronise.                       */
int ofx_es_get(ofx_handle *h, double *weights_host, double *biases_host);
int ofx_es_set(ofx_handle *h, const double *weights_host, const double *biases_host);
/* Member `member` of P (P: the centre), materialised on the device and copied out in the element order.  Synchronises. */
int ofx_es_member(ofx_handle *h, int64_t member, int64_t P, double sigma, uint64_t seed, uint32_t generation,
                  double *weights_host, double *biases_host);
/* ofx_population_act with a member per ship.  member_of: DEVICE int32 [N][M] with values in [-1, P]: -1 = not evolved,
 * P = the centre.  Rasterises the same way, then ONE forward launch; entries of dead, unassigned (-1) and out-of-range
 * ships are not written.  The device code is ofx_population_act's with another way to read a weight - the same lanes,
 * the same list order, the same order of every sum - so y and the actions equal, BIT FOR BIT, those of
 * ofx_population_act on a stored genome that holds the member's elements.  The centre takes a path without any Philox
 * evaluation.  Does not synchronise.                                                                                 */
int ofx_es_act(ofx_handle *h, const int32_t *member_of, int64_t P, double sigma, uint64_t seed, uint32_t generation,
               ofx_action *actions, double *y);
/* ofx_population_fitness over members.  sum: DEVICE int64 [P + 1], count: DEVICE int32 [P + 1]; slot P is the centre.
 * Integer atomics.  Does not synchronise.                                                                            */
int ofx_es_fitness(ofx_handle *h, const int32_t *member_of, int64_t P, int64_t *sum, int32_t *count, int32_t reset);
/* THE MEMBER QUEUE (opt-in): with per-arena episodes (ofx_restart_finished, ofx_restart_arenas) the ships of an arena
 * that restarts bank the score of the episode to the member they flew and take the next member from a queue on the
 * device, so P no longer depends on the number of arenas.  All pointers are DEVICE pointers: member_of int32 [N][M],
 * queue_mask uint8 [N][M] (the ships that draw from the queue), queue int64 [2] = (next, completed), sum int64 [P + 1],
 * count int32 [P + 1].  The call reads the handle's restarted[N] as the last ofx_restart_finished / ofx_restart_arenas
 * left it, and OFX_F_LAST_SCORES.  queue[0] >= 0 is the caller's to keep (a queue starts at (0, 0) and the call only
 * counts up).  The law:
 *   next = queue[0];  completed = queue[1]
 *   for a = 0 .. N-1 ascending, if restarted[a] != 0:
 *     for i = 0 .. M-1 ascending:
 *       m = member_of[a][i]
 *       if bank != 0 and 0 <= m <= P:
 *           sum[m] += last_score[a][i];  count[m] += 1;  if m < P: completed += 1
 *       if queue_mask[a][i] != 0:
 *           if next < total:  member_of[a][i] = (int32)(next % P);  next += 1
 *           else:             member_of[a][i] = -1
 *   queue[0] = next;  queue[1] = completed
 * Ticket t is member t % P: total = E * P flies every member exactly E times, and the two signs of a pair hold adjacent
 * tickets.  A ship outside the queue mask keeps its member - an evaluation arena's centre, member P, banks to slot P on
 * its own restarts.  A value of member_of outside [-1, P] is never banked; an arena with restarted[a] == 0 is not
 * touched.  Two kernels: a wave per arena banks (integer atomics: exact in any order) and counts the tickets the arena
 * asks for; one 256-thread workgroup scans the N counts and hands the tickets out.  A ticket is the RANK of its ship
 * among the asking ships in ascending (a, i) order, from a prefix count - never the order atomics land in: the same
 * state gives the same bits on every call.  Does not synchronise.
 * Refusals, each with a message and before anything is enqueued: OFX_ERR_STATE while the handle has no per-arena
 * episode state; OFX_ERR_INVALID for a NULL pointer, P odd or < 2, total < 0.                                          */
int ofx_es_requeue(ofx_handle *h, int32_t *member_of, const uint8_t *queue_mask, int64_t P, int64_t total,
                   int64_t *queue, int64_t *sum, int32_t *count, int32_t bank);
/* The generation step.  d_host: HOST float64 [n_pairs], the weight of each pair (ofighters_amd.es.pair_weights).  Per
 * element e:
 *   g = 0.0;   for i = 0 .. n_pairs - 1 ascending:  g = g + d[i] * eps(i, e);   theta[e] = theta[e] + scale * g
 * every product and every sum rounded on its own, no FMA, no floating-point atomics: the same bits on every call.  (A
 * pair with d[i] == 0 adds +-0 to a sum that is never -0.0; the library leaves such pairs out, which changes no bit.)
 * `generation` is the one the members flew with.  One kernel, one pass over theta.  Does not wait for the update (d is
 * copied before the call returns, after the work already on the handle's stream).                                    */
int ofx_es_update(ofx_handle *h, const double *d_host, int64_t n_pairs, double scale, uint64_t seed, uint32_t generation);
/* The optimiser of the centre (opt-in): momentum or Adam on the rank-weighted estimate minus an L2 term, as Salimans et
 * al.'s published implementation steps (there: Adam or SGD with momentum, l2coeff 0.005).  The estimate
 * G_e = sum_i d_i eps(i, e) exists only in the registers of the generation step, so the optimiser is a kernel of its own
 * that keeps the single pass over theta.
 * STATE.  ofx_es_opt_create gives the centre two more buffers of G float64, m and v, zeroed, in theta's storage layout
 * (first layer input-major): the centre then costs 3 G doubles of HBM, still at any P.  ofx_es_opt_destroy frees them;
 * ofx_es_destroy and ofx_destroy free them too.  No centre, state already present (create) or absent (every other
 * call): OFX_ERR_STATE.  An allocation that fails: OFX_ERR_HIP, the message naming the bytes.  The library holds only m
 * and v: the step count and every scalar derived from it are the caller's.
 * ofx_es_opt_get / _set move m and v in the element order, each as (weights, biases), the way ofx_es_get / _set move
 * theta (the same host path).  Both synchronise.  OFX_ERR_INVALID for a NULL pointer.                                 */
int ofx_es_opt_create(ofx_handle *h);
int ofx_es_opt_destroy(ofx_handle *h);
int ofx_es_opt_get(ofx_handle *h, double *m_weights, double *m_biases, double *v_weights, double *v_biases);
int ofx_es_opt_set(ofx_handle *h, const double *m_weights, const double *m_biases, const double *v_weights,
                   const double *v_biases);
#define OFX_ES_RULE_MOMENTUM 1
#define OFX_ES_RULE_ADAM 2
/* The generation step through the optimiser.  d_host, n_pairs, seed, generation: as in ofx_es_update.  stats: DEVICE
 * float64 [3] or NULL.  Per element e, G_e is exactly ofx_es_update's register sum (g = 0.0; g = g + d[i] * eps(i, e),
 * ascending over the pairs with d != 0), and every line below is ONE separately rounded float64 operation, no FMA:
 *   ghat = gscale * G_e
 *   wd   = decay * theta
 *   q    = ghat - wd
 *   t1 = c1 * m;  t2 = k1 * q;  m' = t1 + t2
 *   MOMENTUM:  step = alpha * m';                                            theta' = theta + step
 *   ADAM:      qq = q * q;  t3 = c2 * v;  t4 = k2 * qq;  v' = t3 + t4
 *              r = sqrt(v');  den = r + eps;  quo = m' / den;  step = alpha * quo;  theta' = theta + step
 * Ascent on fitness - (decay / 2) |theta|^2.  c1 = 0, k1 = 1 is plain SGD with decay.  Under MOMENTUM v is neither read
 * nor written.  sqrt and / are IEEE 754's correctly rounded operations (the library is built without fast-math), so
 * theta', m' and v' are specified to the bit.  With Adam's bias correction folded into the step size, the caller passes
 * k1 = 1 - beta1, k2 = 1 - beta2, alpha = lr * sqrt(1 - beta2^t) / (1 - beta1^t) at step t (ofighters_amd.es.ES.update).
 * One kernel, one pass: theta, m (and v) read once and written once, coalesced.
 * STATS.  When stats is not NULL: stats[0] = sum over e of q * q, stats[1] = sum of step * step, stats[2] = sum of
 * theta' * theta', each in this fixed order.  A workgroup holds 256 consecutive STORAGE positions (a position past G
 * holds +0.0) and adds its terms as a pairwise tree over the position within the workgroup: for stride = 128, 64, .. 1,
 * x[t] = x[t] + x[t + stride] for t < stride.  The workgroup sums lie in a buffer the handle owns; one workgroup then
 * adds them: thread t adds the sums of workgroups t, t + 256, ... in that order starting from 0.0, and the 256 thread
 * sums are added in thread order.  No floating-point atomics: the same state gives the same bits on every call.  With
 * stats == NULL the kernel carries none of this and theta', m', v' are the same bits.
 * REFUSALS, each with a message and before anything is enqueued or written: no optimiser state (OFX_ERR_STATE); NULL
 * d_host; n_pairs outside [1, 2^30); a rule other than the two; any scalar or any d[i] not finite; decay < 0; under
 * ADAM eps <= 0 (OFX_ERR_INVALID).  Does not wait for the step (d is copied before the call returns).               */
int ofx_es_step(ofx_handle *h, const double *d_host, int64_t n_pairs, int32_t rule, double gscale, double decay,
                double alpha, double c1, double k1, double c2, double k2, double eps, uint64_t seed, uint32_t generation,
                double *stats);
/* Per-element adaptive sigma (opt-in): parameter-exploring policy gradients with symmetric sampling (Sehnke, Osendorfer,
 * Rueckstiess, Graves, Peters, Schmidhuber 2010; the separable case of natural evolution strategies).  The mirrored
 * pairs are already the population, and both sums the method needs come from the same eps(i, e): the centre's
 * sum d_i eps and sigma's sum s_i (eps^2 - 1/3).  The generation step is bound by its G x n_pairs Philox evaluations,
 * so sigma is learned in the pass that steps the centre: a kernel of its own, one more genome of HBM, still at any P.
 * STATE.  ofx_es_sigma_create gives the centre one more buffer of G float64, sigma, in theta's storage layout (first
 * layer input-major), every element sigma0.  ofx_es_sigma_destroy frees it; ofx_es_destroy and ofx_destroy free it too.
 * ofx_es_sigma_get / _set move it in the element order as (weights, biases), on the host path of ofx_es_get / _set; both
 * synchronise.  ofx_es_update and ofx_es_step neither read nor write it.
 * REFUSALS, each with a message and before anything is enqueued or written: no centre, a vector that is already there
 * (create), no vector (every other call): OFX_ERR_STATE.  sigma0, or any element given to _set, not finite or <= 0;
 * a NULL pointer; P odd or < 2; member outside [0, P]: OFX_ERR_INVALID.  An allocation that fails: OFX_ERR_HIP, the
 * message naming the bytes.
 * MEMBERS.  Member m = 2 i + b of P is
 *   w_m[e] = theta[e] + (s * sigma[e]) * eps(i, e)
 * s = +1 (b = 0) or -1 (b = 1): the sign is exact, the product is rounded, then the sum, no FMA.  Member P is the centre.
 * With every sigma[e] equal to one value this is ofx_es_member's and ofx_es_act's law bit for bit.
 * ofx_es_sigma_member is ofx_es_member and ofx_es_sigma_act is ofx_es_act under this law: the forward's device code is
 * ofx_es_act's with a reader that reads sigma at the storage position where it reads theta - the same lanes, the same
 * list order, the same order of every sum - and the centre takes the stored-genome path.                             */
int ofx_es_sigma_create(ofx_handle *h, double sigma0);
int ofx_es_sigma_destroy(ofx_handle *h);
int ofx_es_sigma_get(ofx_handle *h, double *weights_host, double *biases_host);
int ofx_es_sigma_set(ofx_handle *h, const double *weights_host, const double *biases_host);
int ofx_es_sigma_member(ofx_handle *h, int64_t member, int64_t P, uint64_t seed, uint32_t generation,
                        double *weights_host, double *biases_host);
int ofx_es_sigma_act(ofx_handle *h, const int32_t *member_of, int64_t P, uint64_t seed, uint32_t generation,
                     ofx_action *actions, double *y);
#define OFX_ES_RULE_PLAIN 0
/* The generation step of the centre AND of sigma.  d_host, s_host: HOST float64 [n_pairs], the pair's weight for the
 * centre (u_{2i} - u_{2i+1}) and for sigma (u_{2i} + u_{2i+1}; ofighters_amd.es.pair_utilities).  The library lists the
 * pairs with d[i] != 0 OR s[i] != 0, ascending: leaving out a pair whose two weights are both zero changes no bit, and a
 * listed pair whose d or whose s is zero adds +-0 to a sum that is never -0.0 - so g is exactly ofx_es_update's register
 * sum.  Per element e, with THIRD = 0x1.5555555555555p-2 (eps's variance to the last bit but 2^-64), every line ONE
 * separately rounded float64 operation, no FMA:
 *   g = 0.0;  qs = 0.0
 *   for each listed pair j, ascending:
 *       x = eps(pair_j, e)
 *       t = d[j] * x;   g = g + t
 *       xx = x * x;  c = xx - THIRD;  u = s[j] * c;  qs = qs + u
 *   sg   = sigma * g
 *   ghat = gscale * sg
 *   wd   = decay * theta
 *   q    = ghat - wd
 *   PLAIN:     step = alpha * q
 *   MOMENTUM:  t1 = c1 * m;  t2 = k1 * q;  m' = t1 + t2;  step = alpha * m'
 *   ADAM:      t1 = c1 * m;  t2 = k1 * q;  m' = t1 + t2;  qq = q * q;  t3 = c2 * v;  t4 = k2 * qq;  v' = t3 + t4
 *              r = sqrt(v');  den = r + eps;  quo = m' / den;  step = alpha * quo
 *   theta' = theta + step
 *   r  = srate * qs
 *   f  = 1.0 + r
 *   sn = sigma * f
 *   if sn < smin: sn = smin
 *   if sn > smax: sn = smax
 *   sigma' = sn
 * The sigma read is the one the members flew with.  sigma[e] stands inside the law, so the caller's gscale is 1 / n_c
 * (PEPG's form), not ofx_es_step's 1 / (n_c sigma).  PLAIN needs no moments; MOMENTUM and ADAM need ofx_es_opt_create's
 * state (else OFX_ERR_STATE), MOMENTUM leaves v alone.  One kernel, one pass: theta, sigma, m, v are each read once and
 * written once, coalesced; no floating-point atomics.
 * STATS.  stats: DEVICE float64 [5] or NULL.  stats[0] = sum of q * q, stats[1] = sum of step * step, stats[2] = sum of
 * theta' * theta', stats[3] = sum of sigma' * sigma', stats[4] = the number of elements a clamp changed (1.0 each), in
 * ofx_es_step's summation order: the pairwise tree over the 256 positions of a workgroup, then one workgroup over the
 * workgroup sums.  NULL compiles none of it and gives the same state bits.
 * REFUSALS beyond those above (OFX_ERR_INVALID): NULL d_host or s_host; n_pairs outside [1, 2^30); a rule outside the
 * three; any scalar, d[i] or s[i] not finite; decay < 0; eps <= 0 under ADAM; smin <= 0 or smax < smin.  Does not wait
 * for the step (d and s are copied before the call returns).                                                          */
int ofx_es_sigma_step(ofx_handle *h, const double *d_host, const double *s_host, int64_t n_pairs, int32_t rule,
                      double gscale, double decay, double alpha, double c1, double k1, double c2, double k2, double eps,
                      double srate, double smin, double smax, uint64_t seed, uint32_t generation, double *stats);

/* ---- bi-head policy forward --------------------------------------------
 * Trainer.pointer_model graph + inference glue
 * (agents/qlearnIA_V2.py:123-190, 206-220).  See ofx_policy.h-style layout
 * notes in DESIGN.md; weights are one float32 blob described by
 * ofx_policy_layout().                                                       */
typedef struct ofx_policy_desc {
  int32_t n_floats;        /* total length of the weight blob                 */
  int32_t offset[64];      /* start of each tensor, order given in DESIGN.md  */
  int32_t count[64];
  int32_t n_tensors;
} ofx_policy_desc;
int ofx_policy_layout(const ofx_handle *h, ofx_policy_desc *desc_host);
/* ship_mask[N][M] uint8 (NULL = every ship) selects which ships get a
 * forward; act_values float32 [N][M][2]; iaction int32 [N][M];
 * ipointer int32 [N][M][2] = (x, y) of the heat-map arg-max
 * (unravel_index(order='F'), qlearnIA_V2.py:218-220); heatmap float32
 * [N][M][W][H] or NULL (never materialised when NULL).  NULL iaction /
 * ipointer: the handle keeps them for ofx_policy_explore / ofx_policy_actions /
 * ofx_replay_capture, whatever else is called in between.                    */
int ofx_policy_forward(ofx_handle *h, const float *weights, const uint8_t *ship_mask,
                       float *act_values, int32_t *iaction, int32_t *ipointer,
                       float *heatmap);
/* Keras keeps a compiled model between predict() calls (the module-level TRAINER, agents/qlearnIA_V2.py:308); the
 * counterpart here: a forward first folds BatchNorm into the convolutions and builds its phase weights / tables from
 * the blob (two small launches).  Pinning a blob does that once: every following forward that names the same
 * pointer reuses the prepared weights, until another blob (or NULL) is pinned.  ofx_dqn_fit on a pinned blob
 * re-prepares behind its update; after changing a pinned blob any other way, pin it again.                     */
int ofx_policy_pin_weights(ofx_handle *h, const float *weights);
/* Diagnostic switches of the policy forward (value 0 / 1): results agree up to fp32 summation order.              */
#define OFX_OPT_TRUNK_PLAIN 1 /* the four trunk layers through the plain VALU convolution (test reference)        */
#define OFX_OPT_FRAMES_REF  2 /* frame lines of the head from the definition instead of the phase form (reference) */
#define OFX_OPT_TRUNK_FUSE  4 /* the streaming form of the trunk (conv1 -> conv2 fused in one persistent kernel, conv3 on
                                LDS-direct loads): 0 auto (when the images fill the CUs four times over), 1 always,
                                2 never; bit-identical results either way                                          */
/* NOT a diagnostic: which bilinear UpSampling2D((2,2), interpolation='bilinear') (qlearnIA_V2.py:166,172,178,184) means.
 * The reference's unpinned keras / tensorflow range admits two: 0 (default) half-pixel centres (TF2 tf.image.resize),
 * 1 the TF1 legacy resize_bilinear(align_corners=False), src = dst / 2.  Weights trained under one give a different
 * heat map under the other.  Applies to the forward, the DQN targets and ofx_dqn_fit; a pinned blob is re-prepared. */
#define OFX_OPT_BILINEAR_LEGACY 3
/* OPT-IN reduced precision, never the default and never the headline number: ofx_policy_forward (the rollout's forward
 * on the live state; ofx_policy_forward_obs, the DQN targets and the fit stay fp32) feeds conv2, conv3, conv4 of the
 * STREAMING trunk (OFX_OPT_TRUNK_FUSE; the unfused trunk has no 16-bit form and stays fp32) and upconv3 to the 16-bit
 * matrix instructions: operands rounded to nearest even, sums in fp32.  The operands are, and nothing else is:
 *   conv2-4  the layer's input activations and its BatchNorm-folded kernel (the fold itself is fp32); the folded bias,
 *            ReLU and max-pool are fp32, conv4's output enters dense1 unrounded;
 *   upconv3  the uprelu2 values and the PHASE weights (rounded after the fp32 combination of the folded kernel with the
 *            bilinear coefficients, not before); bias fp32; the frame lines (rows / columns 0 and 199) exact fp32.
 * conv1, the dense layers, upconv1, upconv2 and upconv4 (its up-sampling included) are the fp32 path's.
 * tests/policy_lowp_ref.py is this contract as a float64 graph.  Against it (tests/test_gpu_policy_lowp.py) the kernels
 * stay at the fp32 path's own bounds - act_values within 1.5e-5, the heat map within 8e-6 of its maximum - on all but the
 * pixels behind an operand that sits within fp32 error of a 16-bit rounding boundary, which fp32 and float64 round to
 * different neighbours: measured at most 0.31 % of a ship's pixels, up to 9e-4 (bf16) / 2.6e-4 (fp16) there.
 * value 1: bf16 operands (8 significant bits); value 2: fp16 operands (11 significant bits; operands beyond
 * 65504 would overflow - activations behind BatchNorm + ReLU and folded weights are far below); value 0: fp32.  The
 * reference's Keras model is fp32 (agents/qlearnIA_V2.py:123-190): with this switch the heat map differs from the
 * UNROUNDED graph by 3.9e-3 (bf16) / 4.6e-4 (fp16) of its maximum on the tests' trained-like weights (3.3e-3 / 4.2e-4
 * on bench.py's) and near-ties of its arg-max can resolve differently; bench.py reports the
 * measured error against the float64 graph and the arg-max agreement next to the speed.                              */
#define OFX_OPT_POLICY_BF16 5
/* Diagnostic: ofx_dqn_fit / ofx_dqn_fit_reference in their PLAIN form (value 1): one kernel per layer and pass, every
 * activation, pooled / up-sampled input and gradient of the graph in HBM (37 MB per row of the minibatch).  The default
 * (0) is the lean form: only the pre-activation tensor of every convolution and the trunk's pooled activations are kept (9.4 MB per row; the first layer is never materialised), everything else
 * is recomputed inside fused tiles.  Same function; the results agree up to fp32 summation order (tests/test_train.py).*/
#define OFX_OPT_FIT_PLAIN 6
/* EXACT, THE DEFAULT: the streaming trunk (OFX_OPT_TRUNK_FUSE) uses the sparsity of its input.  The two input planes are
 * 1-bit maps with ~1 % of the cells set (lib/observation.py:79-95): conv1 of an empty neighbourhood is ONE value per
 * channel, and most of conv2's 16-pixel M-tiles multiply that constant.  A wave of pixel pairs whose bit windows are all
 * empty writes that value instead of looking its table rows up, and an M-tile whose whole input window holds it (and
 * touches no zero padding) stores the constant the dense matrix sequence produces for it instead of running the
 * sequence.  The results are BIT-IDENTICAL to the dense form (tests/test_gpu_policy.py, tests/test_gpu_trunk_default.py),
 * also under OFX_OPT_POLICY_BF16 (the constant then comes from the 16-bit sequence).  The option is tri-state:
 *   never set (a fresh handle): the sparse form, no counters (no allocation, no atomics);
 *   1: the sparse form with the counters of ofx_policy_trunk_stats;
 *   0: the DENSE kernel for the live forward (ofx_policy_forward on the handle's arenas) - the diagnostic form and the
 *      reference of the == tests.  The forwards on stored observations (ofx_policy_forward_obs, the DQN targets) run the
 *      sparse form whatever the value.
 * ofx_policy_trunk_stats: since the last call, M-tiles run / all and table passes run / all [4] (resets; synchronises);
 * all zero unless the option is 1.
 * conv3 follows the sparse form: the streaming conv1 -> conv2 kernel leaves a bit map of the conv2 outputs that may
 * differ from conv2's constant, and the streaming conv3 stores ITS constant for the M-tiles whose window is unmarked and
 * off the padding (bit-identical again, tests/test_gpu_conv3_sparse.py).  The sparse conv3 runs exactly when the sparse
 * conv1 -> conv2 made its input; value 0 gives the dense pair.
 * ofx_policy_trunk_stats3: conv3's M-tiles run / all since ITS last call, under the same rule (zero unless the option is 1).
 * ofx_policy_trunk_features (diagnostic): the trunk's output [n_images][5000], (h, w, c) order, of the last forward of
 * n_images images x m samples per image on this handle, copied out of the forward's workspace - valid only right
 * behind that forward (OFX_ERR_STATE when no workspace of that size stands). */
#define OFX_OPT_TRUNK_SPARSE 7
int ofx_policy_trunk_stats(ofx_handle *h, int64_t *counts_host);
int ofx_policy_trunk_stats3(ofx_handle *h, int64_t *run_host, int64_t *total_host);
int ofx_policy_trunk_features(ofx_handle *h, int32_t n_images, int32_t m, float *out_host);
int ofx_set_option(ofx_handle *h, int32_t option, int32_t value);
/* Exploration of the bi-head action space (Trainer.get_best_action epsilon branch, agents/qlearnIA_V2.py:199-204,
 * and the collecting phase :393-395): for every selected ship, with probability `epsilon` - or always when
 * `collecting` != 0 - replace (iaction, ipointer) by random_play() (:317-321): iaction = randint(0, 1),
 * ipointer = (randint(0, W-1), randint(0, H-1)).  Draws: Philox4x32-10 keyed by `seed`, counter
 * (global arena, ship, tick, stream 2).  NULL iaction / ipointer = the handle's results of the last
 * ofx_policy_forward / ofx_policy_explore.                                                                     */
int ofx_policy_explore(ofx_handle *h, double epsilon, uint64_t seed, uint32_t tick, int32_t collecting,
                       const uint8_t *ship_mask, int32_t *iaction, int32_t *ipointer);
/* Opt-in exploration ladder (Horgan et al. 2018, Ape-X: every actor explores at its own rate; here an arena is an
 * actor).  expo_host: HOST double [N], one exponent per local arena, copied into a handle-owned device array
 * (ofx_destroy frees it); NULL removes the ladder and the behaviour is exactly that without one.  Each value must be
 * >= 0 or +INFINITY: a NaN or a negative value returns OFX_ERR_INVALID and changes nothing.  A set-up call: it
 * synchronises.  While a ladder is set, a ship of local arena a explores in ofx_policy_explore / ofx_policy_act iff
 * `collecting || u <= eps_a` with
 *   expo[a] == +inf   never - a greedy (evaluation) arena; `collecting` is ignored for it, and in ofx_policy_act its
 *                     ships get p_sp = v_ptr
 *   expo[a] == 1      eps_a = epsilon, bit for bit (no pow)
 *   otherwise         eps_a = pow(epsilon, expo[a]) in float64; pow(x, 0) = 1, so exponent 0 always explores
 * The Philox words, u and the random play (iaction, ipointer) drawn from them are those of the scalar rule: only
 * WHETHER a ship explores changes.  The checks of `epsilon` stay as they are.
 * ofx_policy_epsilon_ladder_host reads the exponents back into HOST double [N]; OFX_ERR_STATE while no ladder is set. */
int ofx_policy_epsilon_ladder(ofx_handle *h, const double *expo_host);
int ofx_policy_epsilon_ladder_host(ofx_handle *h, double *dst_host);
/* ofx_policy_forward and ofx_policy_explore in one call, with the values of what was chosen (opt-in; the input of the
 * actor-side initial priorities below).  Afterwards the handle-kept (iaction, ipointer) are bit for bit those of
 * ofx_policy_forward(h, weights, ship_mask, NULL, NULL, NULL, NULL) followed by ofx_policy_explore(h, epsilon, seed,
 * tick, collecting, ship_mask, NULL, NULL); pinning, the OFX_OPT_* switches and the argument checks are those of the two
 * calls.  The exploration draw depends on (arena, ship, tick) alone, so it is made before the forward and handed to the
 * head kernel as a probe: the heat map's value at an exploratory pointer leaves the pass that finds the maximum.  For
 * every selected ship (device float32 [N][M] each; ships outside ship_mask are not written):
 *   q_sa   act_values[chosen iaction]
 *   p_sp   the heat map's value at the chosen pointer: its maximum for a greedy ship, the probed value for an exploring one
 *   v_act  max(act_values)
 *   v_ptr  the heat map's maximum
 * A NULL output goes to a handle-owned [N][M] array (allocated at the first call, freed by ofx_destroy).  A call with
 * ALL FOUR outputs NULL makes those arrays what ofx_replay_capture_valued reads when it is given no values; a call
 * with any explicit output withdraws that again (the handle's arrays would be partly stale).  Does not synchronise.   */
int ofx_policy_act(ofx_handle *h, const float *weights, const uint8_t *ship_mask, double epsilon, uint64_t seed,
                   uint32_t tick, int32_t collecting, float *q_sa, float *p_sp, float *v_act, float *v_ptr);
/* Opt-in Boltzmann exploration: ofx_policy_act with both heads SAMPLED from softmax(Q / T) instead of the epsilon-greedy
 * choice (not in the reference).  Argument checks, pinning, the OFX_OPT_* switches, the handle-kept (iaction, ipointer),
 * the four values and the NULL-output rule are ofx_policy_act's; tau_act and tau_ptr must be finite and >= 0
 * (OFX_ERR_INVALID otherwise, nothing changes).  Does not synchronise.
 *   temperature  per local arena a: T_act[a] = tau_act * (float)eps_a, T_ptr[a] = tau_ptr * (float)eps_a in float32, with
 *                eps_a the float64 rate of ofx_policy_explore: `epsilon` without a ladder and at exponent 1 (bit for
 *                bit), pow(epsilon, expo[a]) otherwise, 0 at exponent +inf (a greedy arena).  The epsilon schedule is
 *                the annealing schedule.
 *   collecting   != 0: the call IS ofx_policy_act(..., collecting = 1), bit for bit in actions and values.
 *   noise        standard Gumbel from a Philox4x32-10 word r keyed by `seed`: w = (r + 0.5) / 2^32, E = -ln(1 - w),
 *                g = -ln(E).  Pointer: pixel (x, y) of ship i of global arena G takes word [x & 3] of counter
 *                (G, i * (W*H/4) + (y*W + x) / 4, tick, stream 6); action k takes word [k] of (G, i, tick, stream 7).
 *                The noise is keyed by the pixel, so the choice is a function of (seed, arena, ship, tick, heat map).
 *   pointer      the first maximum in C order of fmaf(T_ptr[a], g, heat) in float32, heat bit for bit what
 *                ofx_policy_forward writes into a heat-map buffer; by the Gumbel-max identity an exact sample from
 *                softmax(heat / T).  T_ptr[a] == 0 draws no noise: the greedy pointer, bit for bit.
 *   action       1 iff fmaf(T_act[a], g1, act_values[1]) > fmaf(T_act[a], g0, act_values[0]) (a tie gives 0).
 *   values       q_sa = act_values[iaction], v_act = max(act_values), v_ptr = the RAW heat map's maximum (the bits
 *                ofx_policy_act returns), p_sp = the RAW heat value at the chosen pointer.
 * The float32 form of g never rounds 1 - w (that would quantise g by 1e-2 around g = 12, the tail that wins among
 * 160 000 pixels); ofx_policy_gumbel runs the kernels' own function on n device words (a diagnostic).  Largest
 * |g - float64| over the edge words (0, 1, 2^32 - 1, 2^k, 2^k +- 1) and 2^20 Philox words on the MI355X:
 * 9.3e-6, at words just above 2^30 (the tests allow twice that, tests/boltzmann_oracle.py GUMBEL_ABS_ERR; the contract's
 * bound is 1e-4).                                                                                                       */
int ofx_policy_act_boltzmann(ofx_handle *h, const float *weights, const uint8_t *ship_mask, double epsilon,
                             float tau_act, float tau_ptr, uint64_t seed, uint32_t tick, int32_t collecting,
                             float *q_sa, float *p_sp, float *v_act, float *v_ptr);
int ofx_policy_gumbel(ofx_handle *h, const uint32_t *words_dev, int32_t n, float *g_dev);
/* QlearnIA.play action packing (qlearnIA_V2.py:447-454): exactly one of
 * shoot/thrust set, pointer always set.  NULL iaction / ipointer = the handle's
 * results of the last ofx_policy_forward / ofx_policy_explore.               */
int ofx_policy_actions(ofx_handle *h, const int32_t *iaction, const int32_t *ipointer,
                       const uint8_t *ship_mask, ofx_action *actions);

/* ---- transition capture: the replay memory -----------------------------
 * Trainer.memory = deque(maxlen=memory_size) + Trainer.remember
 * (agents/qlearnIA_V2.py:58,237-238), fed by the bookkeeping of QlearnIA.play
 * (:370-403: nothing once the agent's `done` latch is set; the losing frame is
 * still remembered; previous_obs/action/pointer) and cleared per episode by
 * QlearnIA.reset (:360-368) - ofx_spawn* / ofx_restart* do that here.  Every
 * arena owns one memory; rows are appended in (lock-step, ship index) order,
 * the order of request_actions (lib/battleground.py:146-150).
 * One row = [state, iaction, ipointer, reward, next_state, done]; the two
 * observations are kept as the lock-step numbers of their 1-bit maps in the
 * frame ring plus the ship's own toVector head.  (In the reference every ship
 * of a tick shares ONE mutated Observation object, battleground.py:150, so the
 * head found in its memory is the LAST analysed ship's; the per-ship head is
 * stored here and that aliasing is not reproduced.)                          */
typedef struct ofx_transition {
  int32_t tick_prev, tick_next;   /* lock-steps of state / next_state         */
  int32_t frame_prev, frame_next; /* their slots in the arena's frame ring     */
  int32_t ship;                   /* -1 in padding rows of a gathered batch    */
  int32_t iaction, px, py;        /* previous_action, previous_pointer (x, y) */
  int32_t reward;                 /* obs.reward of next_state                  */
  int32_t done;                   /* obs.done of next_state                    */
  float head_prev[8], head_next[8];
} ofx_transition;                 /* 104 bytes                                 */
/* capacity = memory_size (400 in the reference); frames = length of every
 * arena's ring of stored observation maps (0 = capacity + capacity/4 + 2).  An
 * arena stores a frame only on lock-steps where one of its agents plays, and
 * C rows made of runs of consecutive plays reference C + #runs frames (with K
 * capturing ships per arena about C / K); a row whose `state` frame has been
 * overwritten is no longer eligible for sampling.  A frame costs 2 * W*H/8
 * bytes per arena (40 KB at 400x400).                                         */
int ofx_replay_create(ofx_handle *h, int32_t capacity, int32_t frames);
int ofx_replay_destroy(ofx_handle *h); /* also done by ofx_destroy            */
/* Call once per lock-step after the action choice and BEFORE ofx_step: stores
 * the current observation maps as frame `tick` of every arena with a playing
 * agent and runs the play() bookkeeping for every ship selected by ship_mask
 * (NULL = all) with its chosen (iaction, ipointer) (NULL = the handle's results
 * of the last ofx_policy_forward / ofx_policy_explore).  `tick` must increase by
 * one per call and not restart at episode boundaries.                         */
int ofx_replay_capture(ofx_handle *h, uint32_t tick, const uint8_t *ship_mask, const int32_t *iaction,
                       const int32_t *ipointer);
/* Where a completed row's `reward` comes from (opt-in; for ofx_step_repeat's span_reward, when one capture stands for
 * K lock-steps).  reward: DEVICE int32 [N][M], caller-owned, read by every following capture; NULL, the default, is
 * the state's reward field - today's behaviour, bit for bit.  While it is set:
 *  - both capture forms (ofx_replay_capture, ofx_replay_capture_valued) take row.reward from reward[a][i], and the
 *    valued form's y1 / y2 (its initial priorities) are formed with the same value;
 *  - element 0 of the observation head (head_prev[0] / head_next[0]) STAYS the state's reward: it is what the live
 *    forward feeds the network (vec[0] = OFX_F_REWARD), and the forward on stored observations must reproduce it.
 * Dropped with the memory (ofx_replay_create* / ofx_replay_destroy); not part of the replay blob.  Does not
 * synchronise.  OFX_ERR_INVALID for a NULL handle, OFX_ERR_STATE without a replay memory.                          */
int ofx_replay_reward_source(ofx_handle *h, const int32_t *reward);
/* QlearnIA.play's `if obs.done: ... self.done = True` (agents/qlearnIA_V2.py:376-384) for a caller that drives the
 * learning schedule: counts the selected ships (ship_mask [N][M] uint8, NULL = all) that are destroyed now and were
 * not yet marked in seen[N][M] (device uint8, caller-owned, zeroed by the caller at episode starts), marks them, and
 * returns the count - the number of learning agents that see their death for the first time on this lock-step, i.e.
 * how often the reference would call Trainer.replay here.  One 4-byte read instead of an [N][M] download.
 * Synchronises.                                                                */
int ofx_agents_first_done(ofx_handle *h, const uint8_t *ship_mask, uint8_t *seen, int32_t *count_host);
/* len(memory) per arena [N] and the number of rows ever appended [N]; either
 * may be NULL.  Synchronises.                                                 */
int ofx_replay_count(ofx_handle *h, int32_t *count_host, int64_t *appended_host);
/* list(memory) of one arena, oldest first; rows_host holds `capacity` rows.  */
int ofx_replay_rows_host(ofx_handle *h, int32_t arena, ofx_transition *rows_host, int32_t *n_host);
/* 1-bit maps of a stored lock-step of one arena, W*H/8 bytes each: pixel
 * p = y*W + x -> bit (p & 7) of byte p >> 3 (numpy.unpackbits bitorder=
 * 'little').  OFX_ERR_STATE when the arena's ring does not hold that frame.   */
int ofx_replay_frame_host(ofx_handle *h, int32_t arena, int32_t tick, void *ship_bits_host, void *laser_bits_host);
/* random.sample(memory, min(batch, len(memory))) for every arena
 * (qlearnIA_V2.py:241-243): slot[N][batch] (device) receives row indices
 * (oldest first, -1 pads), n_sampled[N] (device, may be NULL) the number drawn.
 * Uniform without replacement (Floyd), Philox counter (global arena, j, draw,
 * stream 3).                                                                  */
int ofx_replay_sample(ofx_handle *h, uint64_t seed, uint32_t draw, int32_t batch, int32_t *slot, int32_t *n_sampled);
/* Materialise sampled rows (device pointers): rows[N][batch] and, when not
 * NULL, the 1-bit maps of state / next_state [N][batch][2 (ship, laser)]
 * [W*H/32] uint32 in the layout ofx_policy_forward's trunk reads.             */
int ofx_replay_gather(ofx_handle *h, const int32_t *slot, int32_t batch, ofx_transition *rows, void *bits_prev,
                      void *bits_next);
/* The same minibatch WITHOUT padding, the form Trainer.replay works on (its batch is min(batch_size, len(memory)) real
 * transitions, qlearnIA_V2.py:241-243): the sampled entries of all arenas in (arena, j) order, packed; entries `first`
 * .. `first + max_rows - 1` of that sequence land in rows[max_rows] / bits_*[max_rows][2][W*H/32] (device, maps may be
 * NULL) and *n_rows_host receives how many were written.  slot / n_sampled as written by ofx_replay_sample.
 * Synchronises.  This is what ofx_dqn_targets / ofx_dqn_fit take: the fit refuses padding rows.                      */
int ofx_replay_gather_valid(ofx_handle *h, const int32_t *slot, const int32_t *n_sampled, int32_t batch, int32_t first,
                            int32_t max_rows, ofx_transition *rows, void *bits_prev, void *bits_next,
                            int32_t *n_rows_host);

/* ---- prioritized experience replay (opt-in) -----------------------------
 * Schaul et al. 2016, proportional variant, per arena like the memories.  Off unless ofx_replay_prioritize is called;
 * then nothing of the uniform path above changes either.
 *  - Masses: float32 m = p^alpha per row, [N][C] in the ring positions of the rows (an append that overwrites a row
 *    overwrites its mass).  A new row gets the arena's running maximum mmax[a] (starts at 1.0); rows already in the
 *    memory when PER is enabled get 1.0.  An update sets p = |e1| + |e2| + eps (float32; e1, e2 = the row's signed TD
 *    errors on the two heads), m = powf(p, alpha) and raises mmax[a] if needed; a non-finite error leaves the mass as it was.
 *  - Sampling: stratified proportional, with replacement, within each arena over its ELIGIBLE rows (those
 *    ofx_replay_sample uses: the oldest rows whose `state` frame has left the ring are skipped).  n = min(batch, valid)
 *    draws.  Draw j: Philox counter (global arena, j, draw, stream 4), U = rr[0] * 2^-32,
 *    u = ((double)j + U) / n * total; the row drawn is the first eligible row whose inclusive prefix mass is > u (none,
 *    through rounding: the last eligible row).  Summation order, part of the contract: all sums in float64; the eligible
 *    rows form 64 contiguous chunks of ceil(valid / 64) rows, each summed sequentially; the chunk totals are chained
 *    sequentially in chunk order (excl[k] = chain before chunk k, total = the whole chain); the prefix of a row of chunk
 *    k is excl[k] + (the sequential sum of chunk k's rows up to it).
 *  - IS weights: raw w = (valid * m / total)^(-beta) in float64, stored as float32 (total = 0: 1); they correct back to
 *    the uniform sampler's distribution (uniform within each arena, equal rows per arena).  alpha = 0 gives w = 1.
 *  - Loss: Keras sample_weight semantics, sum w e1^2 / (2 n) + sum w e2^2 / (160000 n) (divided by n, not by sum w).
 *  - Write-back: one thread per arena walks the window's entries in packed order, so a row drawn twice keeps the later
 *    entry's priority.  An entry is skipped when the ring row its slot names (oldest-first, as ofx_replay_gather_valid
 *    reads it NOW) no longer holds the gathered (tick_prev, ship): overwritten, or shifted by captures since sampling.
 * ofx_replay_create / ofx_replay_destroy drop the priorities with the memory.                                        */
/* Allocate mass [N][C] and mmax [N] and enable PER (OFX_ERR_STATE without ofx_replay_create; alpha < 0 or eps <= 0:
 * OFX_ERR_INVALID).  Called again: new alpha / eps, every mass and mmax back to 1.0.  Synchronises.                */
int ofx_replay_prioritize(ofx_handle *h, float alpha, float eps);
/* The sampler above: slot[N][batch] / n_sampled[N] with ofx_replay_sample's layout and meaning (oldest-first indices,
 * -1 pads), is_weight[N][batch] the raw IS weights (0 in pads).  Device pointers; n_sampled may be NULL.          */
int ofx_replay_sample_prioritized(ofx_handle *h, uint64_t seed, uint32_t draw, int32_t batch, double beta, int32_t *slot,
                                  int32_t *n_sampled, float *is_weight);
/* The IS weights of the window ofx_replay_gather_valid gathers with the same (n_sampled, batch, first, max_rows):
 * packed in its (arena, j) order into out[max_rows] (device) and divided by the window's maximum.                 */
int ofx_replay_window_weights(ofx_handle *h, const float *is_weight, const int32_t *n_sampled, int32_t batch,
                              int32_t first, int32_t max_rows, float *out);
/* Write-back for the n_rows rows of that window: rows[n_rows] as ofx_replay_gather_valid wrote them, td[n_rows][2]
 * = (e1, e2) (from ofx_dqn_fit_weighted's td_out or from the caller).  Device pointers.                           */
int ofx_replay_update_priorities(ofx_handle *h, const int32_t *slot, const int32_t *n_sampled, int32_t batch,
                                 int32_t first, int32_t n_rows, const ofx_transition *rows, const float *td);
/* Masses of one arena, oldest first (the order of ofx_replay_rows_host); mass_host holds `capacity` floats.        */
int ofx_replay_priorities_host(ofx_handle *h, int32_t arena, float *mass_host, int32_t *n_host);

/* ---- actor-side initial priorities (opt-in) --------------------------------
 * Horgan et al. 2018 (Ape-X): with many actors per learner nearly every row leaves the memory before it is ever fitted,
 * so the priority it ENTERS with decides what is sampled - and under the rule above that is the same mmax for all of
 * them.  Here the actor and the learner share a device: the forward of lock-step t + 1 has max act_values(s') and
 * max heat(s'), the one of lock-step t had Q(s, a) and heat(s) at the chosen pointer (ofx_policy_act), so the row's
 * one-step TD errors exist the moment it is captured.  Off unless ofx_replay_actor_priorities is called; then
 * ofx_replay_capture still works as before (mass = mmax[a], prev_q untouched).
 *  - prev_q: float32 [N][M][2] = (q_sa, p_sp) of each ship's previous_*, zeros at first; dropped with the memory.
 *  - ofx_replay_capture_valued does everything ofx_replay_capture does - rows and frames come out byte-identical - and
 *    every playing ship stores this lock-step's (q_sa, p_sp) into prev_q.  A ship whose row completes forms, in float32
 *    and in the operation order of ofx_dqn_targets (the actor and the learner agree on equal inputs),
 *      y1 = reward + gamma * v_act * (1 - done), e1 = prev_q_sa - y1;  y2 = reward + gamma * v_ptr * (1 - done),
 *      e2 = prev_p_sp - y2   (a done row never reads v_*),
 *    and its row's mass is the write-back's p = |e1| + |e2| + eps, m = powf(p, alpha) (one device function for both).
 *    A non-finite e1 or e2: the row takes mmax[a] as it was BEFORE this lock-step, the old rule.  Afterwards
 *    mmax[a] = max(old, the new masses of this arena formed from finite errors) - one wave reduction, no atomics.
 *  - The initial priority is the ONE-STEP error of the blob the forward ran on, in inference mode, whatever targets the
 *    learner forms (n-step, a target network, Double DQN); the first write-back replaces it with the learner's error.
 * The replay blob (below) does not carry prev_q and keeps its format: a checkpoint moves it with the host pair.        */
/* Enable (OFX_ERR_STATE without ofx_replay_prioritize; gamma outside [0, 1] or NaN: OFX_ERR_INVALID).  Called again:
 * the new gamma, prev_q back to zeros.  Synchronises.                                                                */
int ofx_replay_actor_priorities(ofx_handle *h, float gamma);
/* Device float32 [N][M] each: all four NULL = the handle's arrays of the last ofx_policy_act (OFX_ERR_STATE before its
 * first call, or when the last one was given an explicit output), else all four given (OFX_ERR_INVALID otherwise).  tick, ship_mask, iaction, ipointer: ofx_replay_capture's.
 * OFX_ERR_STATE unless actor priorities are enabled.                                                                 */
int ofx_replay_capture_valued(ofx_handle *h, uint32_t tick, const uint8_t *ship_mask, const int32_t *iaction,
                              const int32_t *ipointer, const float *q_sa, const float *p_sp, const float *v_act,
                              const float *v_ptr);
/* prev_q to / from the host, float32 [N][M][2].  OFX_ERR_STATE unless actor priorities are enabled.  Synchronise.    */
int ofx_replay_actor_values_host(ofx_handle *h, float *dst_host);
int ofx_replay_set_actor_values(ofx_handle *h, const float *src_host);

/* ---- global minibatch sampling (opt-in) ----------------------------------
 * The samplers above draw `batch` rows in EVERY arena.  ofx_replay_sample_global draws n_rows rows from the union of all
 * arenas' memories instead - uniform over rows, or proportional to priority ACROSS arenas - and writes them as a list of
 * (arena, slot) pairs, which ofx_replay_gather_list materialises and ofx_replay_update_priorities_list writes back.
 * Nothing of the per-arena calls changes.
 *  - Eligibility is ofx_replay_sample's: the oldest skip[a] rows of arena a whose `state` frame has left the ring (dense
 *    or packed store) are out, v[a] = count[a] - skip[a], R = sum of v.  slot keeps its meaning: the oldest-first index
 *    into the arena's rows, expired rows included (slot = skip[a] + index among the eligible rows).
 *  - n = min(n_rows, R) rows are drawn into arena[j] / slot[j] / is_weight[j], j < n; entries n .. n_rows - 1 receive
 *    -1 / -1 / 0.  *n_drawn_host = n, *eligible_host = R (may be NULL): the call's one synchronisation.
 *  - Draw j uses Philox counter (arena_base, j, draw, stream 5), key = seed, rr = its four words: two shards with
 *    different arena_base draw different rows.
 *  - Uniform (prioritized == 0; needs no ofx_replay_prioritize), without replacement: the eligible rows of all arenas
 *    form one sequence in (arena, oldest-first) order; stratum j is the integer range [j * R / n, (j + 1) * R / n)
 *    (64-bit integer arithmetic, floor); the row drawn is lo + ofx_draw_int(rr[0], hi - lo - 1) = lo + (rr[0] * (hi -
 *    lo)) >> 32, mapped back to (arena, slot) through the exclusive scan of v.  The strata are disjoint: the output is
 *    strictly ascending in (arena, slot), and n_rows >= R returns every eligible row exactly once.  A row is drawn
 *    with probability 1 / (hi - lo) of its stratum: n / R exactly when n divides R, otherwise n / R up to the rounding of
 *    the strata's bounds (a relative n / R at the most).  is_weight, when given, receives 1.
 *  - Prioritized (prioritized != 0; OFX_ERR_STATE without ofx_replay_prioritize), stratified proportional with
 *    replacement over all eligible rows.  Arena masses: the total T[a] and the inclusive prefix of a row inside its arena
 *    are ofx_replay_sample_prioritized's (float64, 64 chunks of ceil(v / 64) rows summed in row order, chunk totals
 *    chained in order).  Cross-arena prefix, a fixed order: groups of 256 consecutive arenas; s_a = the sequential float64
 *    running sum of T inside the group in arena order (starting from 0.0 at the group's first arena); X_0 = 0,
 *    X_{k+1} = X_k + s_last(k); arena a of group k has inclusive prefix G[a] = X_k + s_a and exclusive prefix E[a] =
 *    G[a - 1] (0 for arena 0); total = G[N - 1].  G is monotone by construction.  Draw j: U = rr[0] * 2^-32,
 *    u = ((double)j + U) / n * total; the arena is the first with G[a] > u (none: the last arena with an eligible row);
 *    inside it u' = u - E[a] and the row is the first eligible row whose per-arena inclusive prefix is > u' (none: the
 *    arena's last eligible row).  Draws come out non-decreasing in (arena, slot); duplicates are adjacent.
 *  - IS weights: raw w = ((double)R * m / total)^(-beta) in float64 (total == 0: 1), rounded to float32, then divided
 *    in float32 by the maximum over the n drawn rows.  They correct to UNIFORM OVER ROWS of the whole memory - the
 *    distribution of the uniform mode above - not to the per-arena sampler's "equal rows per arena".
 * Errors: OFX_ERR_STATE without a replay memory (or without PER when prioritized); OFX_ERR_INVALID for a NULL arena /
 * slot / n_drawn_host, a NULL is_weight when prioritized, n_rows <= 0, a non-finite beta, or n_arenas * capacity >= 2^31.
 * The [N]-sized workspace (skip, v, their scan, T, G) belongs to the handle: allocated at the first call, freed by
 * ofx_replay_destroy / ofx_replay_create, not part of a checkpoint.                                                  */
int ofx_replay_sample_global(ofx_handle *h, uint64_t seed, uint32_t draw, int32_t n_rows, int32_t prioritized, double beta,
                             int32_t *arena, int32_t *slot, float *is_weight, int32_t *n_drawn_host,
                             int64_t *eligible_host);
/* Output d of the n listed rows is what ofx_replay_gather_valid (ret and disc NULL) or ofx_replay_gather_nstep (ret and
 * disc given: the composite row of the n-step chain, ret[d], disc[d]) writes for the same (arena, slot): the row and
 * both maps [n][2][W*H/32] in the trunk's layout (maps may be NULL).  One workgroup per listed row.  An entry whose
 * arena is outside [0, N) or whose slot is outside [0, count[arena]) cannot be checked on the host (device pointers): it
 * receives ofx_replay_gather's padding row (ship = -1, zero maps, ret = disc = 0) and nothing is read for it.
 * OFX_ERR_INVALID for n <= 0, nstep outside 1 .. 64, gamma outside [0, 1] (NaN included), or nstep > 1 without ret and
 * disc.  Does not synchronise.                                                                                      */
int ofx_replay_gather_list(ofx_handle *h, const int32_t *arena, const int32_t *slot, int32_t n, int32_t nstep, float gamma,
                           ofx_transition *rows, void *bits_prev, void *bits_next, float *ret, float *disc);
/* Write-back for a gathered list: rows[n] as ofx_replay_gather_list wrote them, td[n][2] = (e1, e2).  Mass formula,
 * finiteness test and staleness test are ofx_replay_update_priorities': entry j LANDS when its (arena, slot) names a row,
 * that ring row still holds the gathered (tick_prev, ship) and both errors are finite.  Every entry that lands raises
 * mmax[arena]; of a run of ADJACENT entries naming the same (arena, slot) the last one that lands sets the mass (a row
 * drawn twice keeps the later entry's priority; the sampler's lists have their duplicates adjacent).  Precondition:
 * duplicates that are not adjacent are not ordered - one of them sets the mass.  Then every arena's mmax is raised to
 * the maximum over all arenas, so that a row captured next enters at the global maximum, as global competition needs
 * (ofx_replay_capture itself is unchanged).  OFX_ERR_STATE without PER.  Does not synchronise.                        */
int ofx_replay_update_priorities_list(ofx_handle *h, const int32_t *arena, const int32_t *slot, int32_t n,
                                      const ofx_transition *rows, const float *td);

/* ---- checkpoint: export / import of the replay memory --------------------
 * What a training run must carry across processes besides the weights (checkpoints).  A CHUNK is the
 * whole memory of local arenas [arena0, arena0 + n_arenas): the caller bounds host memory by choosing the chunk.  The
 * frame ring is packed on the device - its maps are 1-bit discs, nearly every word is zero - and only the packed
 * result crosses to the host.  A chunk is one self-describing little-endian blob of four sections, back to back:
 *
 *  1. Header, 80 bytes:
 *       offset  0 uint32 magic 0x5258464F (the bytes "OFXR")     offset  4 uint32 format version, 1
 *       offset  8 int32 width W    12 int32 height H    16 int32 n_ships M    20 int32 capacity C
 *       offset 24 int32 frames F (the ring's real length, never 0)     28 int32 words = W * H / 32
 *       offset 32 int32 n_arenas n of the chunk      36 int32 prioritized (0 / 1)
 *       offset 40 float32 alpha    44 float32 eps    (of ofx_replay_prioritize; 0 without PER)
 *       offset 48 uint64 raw_bytes    56 uint64 count_bytes    64 uint64 pair_bytes    72 uint64 zero
 *  2. Raw section (raw_bytes): every per-arena and per-ship array of the memory that is state, in this order, each the
 *     chunk's slice [n]... of the device array as it lies there, each padded with zero bytes to a multiple of 8:
 *       frame_tick int32 [n][F]      lock-step held by each ring slot, -1 = empty
 *       frame_head int32 [n]         next slot to write, in [0, F)
 *       cur_slot   int32 [n]         slot written by the last capture, -1 = none, in [-1, F)
 *       rows       ofx_transition [n][C]   the whole ring of rows in ring position order, stale ones included; the
 *                                    live rows are the `count` positions before `head`: (head - count + i) mod C,
 *                                    i = 0 (oldest) .. count - 1
 *       head       int32 [n]         next ring position to write, in [0, C)
 *       count      int32 [n]         min(appended, C)
 *       appended   int64 [n]
 *       has_prev   uint8 [n][M]      the ship has previous_* (QlearnIA.play)
 *       latched    uint8 [n][M]      the agent's `done` latch
 *       prev_iaction, prev_px, prev_py, prev_tick, prev_slot   int32 [n][M] each (five arrays, in this order)
 *       prev_head  float32 [n][M][8]
 *       mass       float32 [n][C]    only with prioritized = 1: p^alpha in the ring positions of `rows`
 *       mmax       float32 [n]       only with prioritized = 1
 *     raw_bytes is the sum of the padded sizes.  The offsets scratch of the gathers is not state and not saved.
 *  3. Count section (count_bytes = 4 * n * F * 2): uint32 count[n][F][2] - for every (arena, slot, map: 0 ship,
 *     1 laser) the number of nonzero 32-bit words of that stored map (pixel p -> bit (p & 31) of word p >> 5).  A slot
 *     with frame_tick == -1 has count 0.
 *  4. Pair section (pair_bytes = 8 * the sum of the counts): for every map in the same (arena, slot, map) order its
 *     count pairs (uint32 word index, uint32 word), ascending in word index, all concatenated.
 * The blob is exactly 80 + raw_bytes + count_bytes + pair_bytes long.  Two exports of the same state are
 * byte-identical.
 *
 * ofx_replay_export_bytes runs the count pass and returns the exact size of the chunk's blob.  ofx_replay_export
 * counts again and writes the blob to dst_host (*written_host = its size); with `bytes` too small it fails with
 * OFX_ERR_INVALID and touches nothing.  Both synchronise.
 * ofx_replay_import replaces the memory of the chunk's arenas by the blob's: the handle must have a replay memory of
 * the blob's capacity, frames and PER state (alpha and eps bit for bit) on arenas of the blob's M, W, H, and n_arenas
 * must be the blob's - otherwise OFX_ERR_STATE (no memory) or OFX_ERR_INVALID with a message naming the field.  The
 * blob goes through ofx_replay_blob_check before anything on the device is written: a refused blob leaves the handle
 * as it was.  Then the chunk's part of the ring is cleared, the raw arrays are uploaded and the pairs are scattered.
 * Synchronises.
 * ofx_replay_blob_check needs no handle and no device.  It is the single place that decides whether a blob may reach
 * the kernels; `frames` is the ring's real length.  OFX_ERR_INVALID with a message naming the fault for: a wrong magic
 * or version; any header dimension that differs from the arguments; section sizes that differ from what the dimensions
 * give, or that do not add up to `bytes`; a count above `words`, a nonzero count in an empty slot, counts that do not sum
 * to the pair section; a word index >= words, indices that do not ascend strictly within a map, a zero word;
 * frame_tick < -1, frame_head / cur_slot / head / count outside the ranges above, appended < count; a live row with
 * frame_prev / frame_next outside [0, F), ship outside [0, M), iaction outside [0, 2), px outside [0, W) or py outside
 * [0, H); a ship with has_prev whose prev_slot / prev_iaction / prev_px / prev_py are outside those ranges; with PER a
 * mass or mmax that is not finite and >= 0.                                                                        */
int ofx_replay_export_bytes(ofx_handle *h, int32_t arena0, int32_t n_arenas, size_t *bytes_host);
int ofx_replay_export(ofx_handle *h, int32_t arena0, int32_t n_arenas, void *dst_host, size_t bytes, size_t *written_host);
int ofx_replay_import(ofx_handle *h, int32_t arena0, int32_t n_arenas, const void *src_host, size_t bytes);
int ofx_replay_blob_check(const void *src_host, size_t bytes, int32_t n_ships, int32_t width, int32_t height,
                          int32_t capacity, int32_t frames, int32_t prioritized, int32_t n_arenas);

/* ---- packed frame store (opt-in, exact) ----------------------------------
 * The frame ring of ofx_replay_create is frame_bits [N][F][2][W*H/32]: 40 KB per stored lock-step and arena at 400x400,
 * 82 GB at 4096 arenas with capacity 400.  Its maps are 1-bit discs, nearly every word zero.  ofx_replay_create_packed
 * builds the same memory - capacity, frames (0 = capacity + capacity/4 + 2), the same checks - that KEEPS its frames as
 * the (word index, word) pairs of their nonzero words, the form the checkpoint blob already has.  Nothing else differs:
 * every entry point above that reads the memory returns the bytes it returns from the dense ring holding the same
 * frames, the blob format stays version 1, and a blob exported from either form imports into the other.
 *  - Storage per arena: a POOL of pool_pairs uint2 (word index, word), a cyclic buffer (position i means i mod
 *    pool_pairs), and
 *       frame_off [N][F] uint32      pool position of the slot's first pair
 *       frame_cnt [N][F][2] uint32   pairs of the slot's ship map and of its laser map; 0 in a slot without a live frame
 *       pool_head [N] uint32, live [N] uint32 (pairs of all live frames), evicted [N] int64
 *    A slot's pairs are its ship map's, then its laser map's; within a map the word index ascends strictly, a zero word
 *    is never stored, and pixel p is bit (p & 31) of word p >> 5 - the order of the blob's pair section.
 *  - Sizing: pool_pairs = 0 selects max(512 * frames, 4 * words), words = W*H/32.  512 pairs per slot is about twice the
 *    mean of the densest run on record (245 pairs per frame, every ship capturing, profiles/r08_checkpoint_4096.txt) and
 *    8.2 GB instead of 82 GB at the size above; it rests on that one profile, and profiles/r09_packed_replay.txt has what
 *    a training run needs.  Any other value must lie in [4 * words, 2^31): a frame has at most 2 * words pairs, so the
 *    newest frame and its predecessor - the two a transition needs - always fit together.  Otherwise OFX_ERR_INVALID
 *    naming the bound; also when the two maps of a frame (8 * words bytes) exceed the 64 KB of LDS in which the
 *    readers rebuild them, i.e. for arenas above W*H = 262 144 (the dense ring serves those).
 *  - Storing a frame of k = k_ship + k_laser pairs into slot s = frame_head (ofx_replay_capture), the rule:
 *      1. If slot s still holds a live frame (the slot ring has wrapped), release it: live -= its pairs.  It is the
 *         oldest frame.
 *      2. While live + k > pool_pairs, release the oldest live frame - the first slot with frame_tick >= 0 walking
 *         cyclically from s + 1: frame_tick = -1, both counts 0, live -= its pairs, evicted[a] += 1.  EARLY EVICTION.
 *      3. frame_off[s] = pool_head; the k pairs go to pool_head .. pool_head + k - 1 (mod pool_pairs); pool_head =
 *         (pool_head + k) mod pool_pairs, live += k, frame_tick[s] = tick.
 *    So frames leave oldest-first under both mechanisms; the live frames are a cyclic run of slots ending at
 *    frame_head - 1 and their pairs a cyclic run of the pool ending at pool_head; live depends on the live frames'
 *    counts only, never on where they lie.  An early-evicted frame is to every reader what an overwritten frame is:
 *    ofx_replay_frame_host answers OFX_ERR_STATE, and the rows whose `state` frame is gone stay in the row ring and are
 *    skipped by both samplers (frame_tick[frame_prev] != tick_prev).  Nothing is truncated silently: a pool that is
 *    too small shows as fewer eligible rows and in ofx_replay_store_stats.
 *  - Checkpoint: the export's count section is frame_cnt and its pair section the slots' pair ranges, un-wrapped -
 *    byte for byte the dense ring's blob of the same frames (an early-evicted slot is an empty slot).  The import runs
 *    ofx_replay_blob_check, then places every arena's live frames in chronological order (the slots walked from
 *    frame_head, oldest first) from pool position 0 and sets frame_off, frame_cnt, pool_head and live accordingly; the
 *    memory behaves from then on as the one that was exported.  If an arena's live pairs exceed pool_pairs the import
 *    fails with OFX_ERR_INVALID naming the arena and both numbers before anything on the device is written.  evicted is
 *    a per-process counter like ofx_overflow_count and not carried.
 * ofx_replay_store_stats synchronises and fills stats_host[6]: [0] 1 packed / 0 dense, [1] pool_pairs per arena,
 * [2] max over arenas of live, [3] sum over arenas of live, [4] sum of evicted since create, [5] bytes of HBM the frame
 * store holds (dense: frame_bits; packed: pool + frame_off + frame_cnt + pool_head + live + evicted).  A dense memory
 * reports [1] .. [4] as 0.  OFX_ERR_STATE without a replay memory.                                                  */
int ofx_replay_create_packed(ofx_handle *h, int32_t capacity, int32_t frames, int64_t pool_pairs);
int ofx_replay_store_stats(ofx_handle *h, int64_t *stats_host /* [6] */);

/* ---- n-step returns (opt-in) --------------------------------------------
 * Not in the reference.  Off unless these two calls are used; nothing above changes.
 *  - Window: ofx_replay_gather_nstep gathers the window ofx_replay_gather_valid gathers for the same (slot, n_sampled,
 *    batch, first, max_rows): the same packed (arena, j) order, the same *n_rows_host, the same synchronisation.
 *  - Chain: from the sampled row r0, r_{k+1} is the row of the same arena and ship with tick_prev == r_k.tick_next
 *    (unique: a ship appends at most one row per capture tick, and the capture tick never restarts).  The chain stops
 *    after L = nstep rows, after a row with done != 0, or when no such row is in the memory (an episode restart cleared
 *    previous_*, so the ticks do not chain, or the successor is not captured yet); a truncated chain is no error and
 *    bootstraps from its last row with gamma^L.  The walk only reads the memory.
 *  - Composite row: r0 with tick_next, frame_next, head_next and done of r_{L-1} (ship, tick_prev, frame_prev, iaction,
 *    px, py, head_prev and reward stay r0's, so ofx_replay_update_priorities writes PER priorities back unchanged).
 *    bits_prev[d] = r0's state maps, bits_next[d] = r_{L-1}'s next-state maps (newer than r0's state frame, so still in
 *    the ring whenever r0 is eligible).
 *  - Return and discount, float64 with every operation rounded on its own (no FMA): g = (double)gamma, acc = 0, p = 1;
 *    for k = 0 .. L-1: acc += p * r_k.reward, then p *= g.  ret[d] = (float)acc, disc[d] = r_{L-1}.done ? 0 : (float)p.
 *  - Targets: ofx_dqn_targets_nstep is ofx_dqn_targets with y_act = ret + disc * max(act_values(next_state)) and
 *    y_ptr = ret + disc * max(heat(next_state)) in float32, the product rounded, then the sum (no FMA).  q_sa / p_sp,
 *    their NULL rule and padding rows as in ofx_dqn_targets.
 *  - nstep = 1 gives ofx_replay_gather_valid's rows and maps bit for bit with ret = reward, disc = gamma * (not done),
 *    and those fed to ofx_dqn_targets_nstep give ofx_dqn_targets' y_act / y_ptr bit for bit.
 * Errors: OFX_ERR_INVALID where ofx_replay_gather_valid fails so, for nstep outside 1 .. 64, for gamma not finite or
 * outside [0, 1], and (both calls) for a NULL ret or disc.                                                          */
/* ret[max_rows] / disc[max_rows] float32, device pointers like the rest; maps may be NULL.  Synchronises.          */
int ofx_replay_gather_nstep(ofx_handle *h, const int32_t *slot, const int32_t *n_sampled, int32_t batch, int32_t first,
                            int32_t max_rows, int32_t nstep, float gamma, ofx_transition *rows, void *bits_prev,
                            void *bits_next, float *ret, float *disc, int32_t *n_rows_host);
/* ret[n] / disc[n] as ofx_replay_gather_nstep wrote them, for the n rows it gathered.                              */
int ofx_dqn_targets_nstep(ofx_handle *h, const float *weights, int32_t n, const ofx_transition *rows,
                          const void *bits_prev, const void *bits_next, const float *ret, const float *disc,
                          float *q_sa, float *p_sp, float *y_act, float *y_ptr);

/* ---- target network and Double DQN (opt-in) -----------------------------
 * Not in the reference.  Off unless these two calls are used; nothing above changes.  A target network is a second
 * weight blob in the ofx_policy_layout order that the caller keeps and moves towards the trained one with
 * ofx_policy_blend_weights; the plain targets bootstrap from it when ofx_dqn_targets / ofx_dqn_targets_nstep are given
 * that blob.  Double DQN (van Hasselt et al. 2016) selects with the online blob and evaluates with the target blob:
 *  - Selection, per real row i: a* = iaction and p* = ipointer that ofx_policy_forward_obs(online, next_state) returns
 *    (the first maximum, as np.argmax).
 *  - Evaluation: v_act = act_values(target, next_state)[a*]; v_ptr = ptr_probe of
 *    ofx_policy_forward_obs(target, next_state, probe = p*), the value the target's arg-max pass holds at that pixel.
 *  - One-step form (ret == disc == NULL): y_act = (float)reward + gamma * v_act * live and
 *    y_ptr = (float)reward + gamma * v_ptr * live with live = done ? 0 : 1 - the expression and the rounding of
 *    ofx_dqn_targets, every operation rounded on its own.
 *  - n-step form (ret and disc given, as ofx_replay_gather_nstep wrote them): y = ret + disc * v in float32, the product
 *    rounded, then the sum (no FMA); gamma is ignored.  Exactly one of ret / disc NULL is OFX_ERR_INVALID.
 *  - Everything else as ofx_dqn_targets: q_sa / p_sp come from `online` on `state`, both NULL or both given (NULL skips
 *    that forward); padding rows (ship < 0) give zeros; the same argument checks (a NULL target is OFX_ERR_INVALID).
 *  - target == online (the same pointer) is allowed: the value at the arg-max is the maximum, so the results are
 *    ofx_dqn_targets' / ofx_dqn_targets_nstep's bit for bit (NaN outputs excepted: max() skips a NaN, a selection does
 *    not).
 *  - Order on the handle's stream: online on `state` (when asked for), online on next_state, target on next_state, one
 *    kernel for the selection and the TD arithmetic.  A pinned online blob uses its prepared weights; the target blob is
 *    prepared per call in the handle's second slot, so the pinned preparation survives.  Does not synchronise.
 *  - Blend: ofx_policy_blend_weights moves the whole blob (ofx_policy_layout n_floats, every tensor, the BatchNorm
 *    moving statistics included): dst[i] = c * dst[i] + tau * src[i] with c = 1.0f - tau formed once in float32, both
 *    products rounded, then the sum (no FMA).  tau == 1 is a plain device copy (a dst that has become NaN recovers on
 *    a hard sync), tau == 0 changes nothing.  Runs on the handle's stream, does not synchronise.  When dst is the
 *    handle's pinned blob its preparation is redone, as after a fit.  dst and src must not overlap.
 * Errors (nothing is written): ofx_policy_blend_weights gives OFX_ERR_INVALID for a NULL handle or blob, for
 * dst == src and for tau not finite or outside [0, 1].                                                             */
int ofx_dqn_targets_double(ofx_handle *h, const float *online, const float *target, int32_t n,
                           const ofx_transition *rows, const void *bits_prev, const void *bits_next, float gamma,
                           const float *ret, const float *disc, float *q_sa, float *p_sp, float *y_act, float *y_ptr);
int ofx_policy_blend_weights(ofx_handle *h, float *dst, const float *src, float tau);

/* ---- forward on stored observations, TD targets -------------------------
 * The predictions Trainer.replay makes on a minibatch (agents/qlearnIA_V2.py:251-268): n_obs observations given as
 * 1-bit map pairs bits[n_obs][2 (ship, laser)][W*H/32] uint32 (the layout ofx_replay_gather writes) + their toVector
 * heads vec8[n_obs][8]; every observation gets its own trunk run.  Outputs (device, any may be NULL): act_values
 * [n_obs][2], iaction [n_obs], ipointer [n_obs][2], ptr_max [n_obs] = np.max of the heat map; with probe [n_obs][2]
 * (x, y) also ptr_probe [n_obs] = the heat-map value at that pointer.                                            */
int ofx_policy_forward_obs(ofx_handle *h, const float *weights, int32_t n_obs, const void *bits, const float *vec8,
                           float *act_values, int32_t *iaction, int32_t *ipointer, float *ptr_max,
                           const int32_t *probe, float *ptr_probe);
/* The targets Trainer.replay builds (:269-270) for n gathered transitions (rows, bits_prev, bits_next from
 * ofx_replay_gather): two forwards, then per row
 *   q_sa  = act_values(state)[iaction]           y_act = reward + gamma * max(act_values(next_state)) * (not done)
 *   p_sp  = heat(state) at ipointer              y_ptr = reward + gamma * max(heat(next_state))       * (not done)
 * i.e. the current values and the values written into target[iaction] / ptr_target[ipointer]; their squared
 * differences are the two MSE terms ofx_dqn_fit minimises.  The reference indexes ptr_target[x][y] on a [y][x] map
 * (:280) and fits on next_state's inputs (:282-283); here the pointer addresses the pixel it was chosen as
 * (ofx_dqn_fit_reference reproduces the reference as written).  Padding rows (ship < 0) give zeros.  q_sa and p_sp may
 * both be NULL: the forward on `state` is then skipped (ofx_dqn_fit needs only y_act / y_ptr).                    */
int ofx_dqn_targets(ofx_handle *h, const float *weights, int32_t n, const ofx_transition *rows, const void *bits_prev,
                    const void *bits_next, float gamma, float *q_sa, float *p_sp, float *y_act, float *y_ptr);

/* One fit step of Trainer.replay (model.fit, agents/qlearnIA_V2.py:284; loss 'mse' on both heads, Adam(lr) :190) on n
 * gathered transitions: forward in training mode (BatchNorm on the batch statistics, moving statistics updated with
 * momentum 0.99 like Keras), targets = the current predictions except target[iaction] = y_act[i] and
 * ptr_target at the pointer = y_ptr[i] (from ofx_dqn_targets), backward, Adam (beta 0.9 / 0.999, eps 1e-7, `step`
 * 1-based).  weights / adam_m / adam_v: device float32 [n_floats] in the ofx_policy_layout order, updated in place;
 * grad_out (device, may be NULL) receives the gradient; loss_host[2] = the two mse terms.  Inputs are the
 * transitions' `state` observations and the pointer addresses heat[y][x] (the reference fits on next_state's inputs
 * and indexes [x][y], :280-283: that form is ofx_dqn_fit_reference).  Every row must be a real transition (ship >= 0; use
 * ofx_replay_gather_valid): a padding row would enter the BatchNorm batch statistics and the loss scale, so the call
 * fails with OFX_ERR_INVALID before anything is updated.  The handle keeps a workspace of 9.4 MB per row between calls (given back when a call needs less than a quarter of it)
 * (OFX_OPT_FIT_PLAIN: 37 MB); every reduction has a fixed order, so the same call on the same state gives the same bits.
 * fp32 on the vector ALU (not the hot path): 3.6 ms for 64 rows, 42 ms for 4096 with the target forward (ofx_dqn_fit_reference: 4.7 / 65 ms); synchronises. */
int ofx_dqn_fit(ofx_handle *h, float *weights, float *adam_m, float *adam_v, int32_t step, float lr, int32_t n,
                const ofx_transition *rows, const void *bits_prev, const float *y_act, const float *y_ptr,
                float *grad_out, float *loss_host);
/* ofx_dqn_fit with per-row loss weights (Keras sample_weight: sum w e1^2 / (2 n) + sum w e2^2 / (160000 n)) and the rows'
 * errors from its own training-mode forward: row_weight [n] / td_out [n][2] = (e1, e2) = (prediction - target) on the
 * two heads before the update, device pointers, either may be NULL.  The weight is the first factor of every seed, so
 * a NULL row_weight or weights of 1.0 give ofx_dqn_fit bit for bit (lean and OFX_OPT_FIT_PLAIN forms).           */
int ofx_dqn_fit_weighted(ofx_handle *h, float *weights, float *adam_m, float *adam_v, int32_t step, float lr, int32_t n,
                         const ofx_transition *rows, const void *bits_prev, const float *y_act, const float *y_ptr,
                         float *grad_out, float *loss_host, const float *row_weight, float *td_out);
/* ofx_dqn_fit_weighted with the two error bounds every DQN since Mnih et al. 2015 carries, both opt-in (0 = off):
 *   huber_delta > 0: Keras Huber(delta) in place of the squared error, h(e) = 0.5 e^2 for |e| <= delta, else
 *     delta |e| - 0.5 delta^2; loss1 = sum w h(e1) / (2 n), loss2 = sum w h(e2) / (160000 n), seeds
 *     w clamp(e, -delta, delta) over the same denominators.  Inside the quadratic zone that is HALF the gradient of the
 *     'mse' fit (0.5 e^2 against e^2), as in Keras: a delta above every error is not the squared-error fit but that fit at
 *     half the learning signal.  td_out keeps the raw (e1, e2) - priorities stay |TD error| - and loss_host returns the
 *     Huber losses.
 *   clip_norm > 0: torch.nn.utils.clip_grad_norm_ over the whole gradient blob: norm = sqrt(sum g^2) (summed in double
 *     in a fixed order: the step stays reproducible to the bit), Adam consumes min(1, clip_norm / (norm + 1e-6)) g.
 *     grad_out receives the gradient BEFORE scaling.
 * grad_norm_host (may be NULL) receives the norm before clipping; it is computed when it is asked for or clip_norm > 0
 * and read back with the loss (no further synchronisation).  Textbook (sparse-target) form only, lean and
 * OFX_OPT_FIT_PLAIN.  A negative or non-finite huber_delta / clip_norm fails with OFX_ERR_INVALID before anything is
 * launched.  huber_delta == 0, clip_norm == 0 and grad_norm_host == NULL launch exactly what ofx_dqn_fit_weighted does. */
int ofx_dqn_fit_robust(ofx_handle *h, float *weights, float *adam_m, float *adam_v, int32_t step, float lr, int32_t n,
                       const ofx_transition *rows, const void *bits_prev, const float *y_act, const float *y_ptr,
                       float *grad_out, float *loss_host, const float *row_weight, float *td_out, float huber_delta,
                       float clip_norm, float *grad_norm_host);
/* The same step with Trainer.replay's quirks reproduced as written (agents/qlearnIA_V2.py:251-285), for a user who
 * wants the reference's training dynamics rather than the textbook DQN step above:
 *   - targets are whole predictions of `state` ([target, ptr_target] = predict(state), inference-mode BatchNorm) with
 *     target[iaction] and ptr_target[ipointer] replaced (:279-280);
 *   - ipointer = (x, y) indexes the (400, 400, 1) prediction as [x][y] - row x, column y, the transpose of the pixel
 *     get_best_action named (:218-220 vs :280);
 *   - the fit's inputs are NEXT_state's maps and head (img_input is re-bound at :273; :282-283), so every output
 *     element carries an error (training-mode forward on next_state against targets built from state).
 * Computes the targets itself (gamma = Trainer.gamma, 0.9 at :60): rows / bits_prev / bits_next from
 * ofx_replay_gather_valid.  Everything else (loss scale, Adam, moving statistics, padding refusal, outputs) as
 * ofx_dqn_fit.  Parity with Keras is unpinned for both forms.                                                     */
int ofx_dqn_fit_reference(ofx_handle *h, float *weights, float *adam_m, float *adam_v, int32_t step, float lr, int32_t n,
                          const ofx_transition *rows, const void *bits_prev, const void *bits_next, float gamma,
                          float *grad_out, float *loss_host);

/* ---- the fit step in two halves: gradient, then apply (gradient accumulation; the seam for a data-parallel sum) ----
 * ofx_dqn_fit_robust split where its gradient is complete, with a device buffer between the halves, for the textbook
 * (sparse-target) fit in both forms (lean and OFX_OPT_FIT_PLAIN).  The three fused entries above are untouched.
 *
 * The accumulator `acc` is ONE contiguous device float32 buffer of ofx_dqn_acc_floats(h) = n_floats + OFX_ACC_TAIL
 * floats (a data-parallel caller needs one SUM all-reduce over it):
 *   [0, n_floats)                         the gradient in the ofx_policy_layout order, untrained slots zero (grad_out)
 *   tail + OFX_ACC_STAT_FLOATS * k, k < 7  BatchNorm batch statistics of trunk layers 0-3 (k = 0-3) and head-2 layers
 *                                         0-2 (k = 4-6): {mean, var} pairs, [2 * c] / [2 * c + 1] of channel c, zeros
 *                                         after the layer's channels
 *   tail + OFX_ACC_LOSS, + 1              loss1, loss2
 *   tail + OFX_ACC_COUNT                  how many micro-batches were summed in (a float count)
 *   the rest                              zero
 * with tail = n_floats.                                                                                            */
#define OFX_ACC_TAIL 256
#define OFX_ACC_STAT_FLOATS 32
#define OFX_ACC_LOSS (7 * OFX_ACC_STAT_FLOATS)
#define OFX_ACC_COUNT (OFX_ACC_LOSS + 2)
int32_t ofx_dqn_acc_floats(const ofx_handle *h);      /* n_floats + OFX_ACC_TAIL; negative on a NULL handle */
/* The gradient half.  For the n rows exactly the gradient, losses, batch statistics and td_out that
 * ofx_dqn_fit_robust(..., row_weight, td_out, huber_delta, clip_norm = 0) computes: the same kernels in the same order,
 * so acc[0, n_floats) after reset holds the bits of that call's grad_out.  Neither `weights` nor any Adam moment is
 * written and a pinned blob is not prepared again.  Then the accumulator is updated in one pass of fixed order:
 *   reset != 0:  acc = this micro-batch's values, the whole buffer, count = 1
 *   reset == 0:  acc[e] += value[e], a plain fp32 add per element (no scale, no fma), count += 1
 * loss_host may be NULL: the call then synchronises no further than the padding check does; with it the call
 * synchronises and loss_host[2] = this micro-batch's two losses.  Padding rows are refused as in ofx_dqn_fit; a NULL
 * acc, n < 1 or a negative or non-finite huber_delta give OFX_ERR_INVALID before anything is launched.  The workspace is
 * that of a fit of n rows (kept by the handle like ofx_dqn_fit's): k micro-batches of n rows cost the memory of one.  */
int ofx_dqn_grad(ofx_handle *h, const float *weights, int32_t n, const ofx_transition *rows, const void *bits_prev,
                 const float *y_act, const float *y_ptr, const float *row_weight, float *td_out, float huber_delta,
                 float *acc, int32_t reset, float *loss_host);
/* The apply half: the tail of a fit step on an accumulator, the effective gradient being scale * acc (scale = 1 / the
 * count for the mean over micro-batches of equal size).
 *   clip_norm > 0 or grad_norm_host: the norm over acc[0, n_floats) in ofx_dqn_fit_robust's grid and order, times scale;
 *     Adam consumes (min(1, clip_norm / (norm + 1e-6)) * scale) * acc, the two factors multiplied once in fp32 into one
 *     factor kept in device memory.  scale == 1 gives the fused call's norm and update bit for bit, and scale == 1 with
 *     clip_norm == 0 runs the unscaled Adam kernel.
 *   moving statistics: 0.99 * moving + 0.01 * (scale * stat);  loss_host[2] = scale * (loss1, loss2) of the tail;
 *   grad_norm_host = the scaled norm before clipping.
 * Adam's constants, the bias correction and `step` (1-based) are ofx_dqn_fit's.  Synchronises once (the read-back), then
 * a pinned blob is prepared again.  OFX_ERR_INVALID for a NULL pointer (loss_host / grad_norm_host may be NULL),
 * step < 1, a scale that is not finite and > 0 or a clip_norm that is negative or non-finite, before anything is
 * launched.  ofx_dqn_grad(reset = 1) + ofx_dqn_apply(scale = 1) on n rows is ofx_dqn_fit_robust on them, bit for bit. */
int ofx_dqn_apply(ofx_handle *h, float *weights, float *adam_m, float *adam_v, int32_t step, float lr, const float *acc,
                  float scale, float clip_norm, float *loss_host, float *grad_norm_host);

/* ---- soft and Munchausen targets (opt-in) --------------------------------
 * Not in the reference.  Off unless these two calls are used; nothing above changes.  The hard maximum of the next
 * state is replaced by the soft (entropy-regularised) value V_T = T ln sum_a exp(Q(a) / T) of soft Q-learning, and
 * Munchausen-DQN (Vieillard et al. 2020) adds the scaled, clipped log-policy of the action taken to the reward.
 *
 * ofx_policy_forward_obs_soft is ofx_policy_forward_obs with two more per-observation outputs (device float32 [n_obs],
 * either may be NULL) and an optional heatmap:
 *  - ptr_mass = Z = sum over the 160 000 pixels of exp((heat - M) / tau_ptr), M = ptr_max (the term of the maximum is 1,
 *    so Z >= 1); ptr_soft = M + tau_ptr * ln Z.  M is ptr_max bit for bit.  A map with no finite value gives NaN in
 *    both, as in ptr_max.
 *  - heatmap (may be NULL): float32 [n_obs][400][400], the bits ofx_policy_forward writes for the same observation.
 *  - Every output ofx_policy_forward_obs has comes out bit for bit as from that call.
 *  - tau_ptr must be 0, or finite in [1e-6, 1e30]; anything else is OFX_ERR_INVALID and nothing is launched.  At
 *    tau_ptr == 0 the default kernel runs: ptr_soft has ptr_max's bits and ptr_mass is 1.
 *  - The heat map is never formed for the sum: the streaming head kernel keeps an online (maximum, sum) per lane next to
 *    its arg-max, merges the lanes of a wave in a fixed tree and the 8 waves of a ship in slot order (no atomics), so a
 *    row's result is the same bits whatever n_obs is and wherever the row stands.
 *  - Accuracy against the float64 log-sum-exp of the float32 heat map the call wrote: |ptr_mass - ref| <= 1e-4 ref and
 *    |ptr_soft - ref| <= 1e-4 tau_ptr + 4 ulp(ref) (DESIGN.md has the derivation; measured: tests/soft_oracle.py).
 *  - Does not synchronise.
 *
 * ofx_dqn_targets_soft is ofx_dqn_targets (ret == disc == NULL) / ofx_dqn_targets_nstep (both given; exactly one NULL is
 * OFX_ERR_INVALID) with the two maxima of `weights` on next_state replaced by soft values:
 *  - V_ptr = ptr_soft at tau_ptr;  V_act = tau_act == 0 ? max(a0, a1) : max(a0, a1) + tau_act * log1p(exp(-|a0 - a1| /
 *    tau_act)), in float32 (expf, log1pf), every operation rounded on its own.
 *  - One-step form: y = (float)reward + gamma * V * live;  n-step form: y = ret + disc * V (gamma ignored): the
 *    expressions and the rounding order of ofx_dqn_targets / _nstep.  tau_act == tau_ptr == 0 with m_alpha == 0 gives
 *    those calls' results bit for bit.
 *  - Munchausen (m_alpha > 0; one-step form only): the forward on `state` runs with `weights` whether or not q_sa / p_sp
 *    are asked for, with the probe at the row's pointer and the soft value;
 *      t = (float)reward + m_alpha * clamp(q - V(state), m_clip, 0)   per head: q = act(state)[iaction] against V_act(state),
 *                                                                      q = the probed heat value against V_ptr(state)
 *      y = t + gamma * V(next_state) * live
 *    (q - V is T ln pi(a | s) of the softmax policy, <= 0 up to rounding.)
 *  - q_sa / p_sp: both NULL or both given; padding rows (ship < 0) give zeros; a pinned blob uses its preparation.
 *  - OFX_ERR_INVALID, before anything is launched: a NULL handle, blob, rows, bits or y; n < 1; a tau that is neither 0
 *    nor finite in [1e-6, 1e30]; m_alpha outside [0, 1] or NaN; and with m_alpha > 0: ret / disc given, a tau that is
 *    0, m_clip not finite or > 0.
 *  - Accuracy against a float64 evaluation of these formulas on the float32 outputs of ofx_policy_forward_obs_soft:
 *    2e-6 * max(1, |reward| + |m_alpha * m_clip| + |V|).  Does not synchronise.                                        */
int ofx_policy_forward_obs_soft(ofx_handle *h, const float *weights, int32_t n_obs, const void *bits, const float *vec8,
                                float tau_ptr, float *act_values, int32_t *iaction, int32_t *ipointer, float *ptr_max,
                                const int32_t *probe, float *ptr_probe, float *ptr_soft, float *ptr_mass, float *heatmap);
int ofx_dqn_targets_soft(ofx_handle *h, const float *weights, int32_t n, const ofx_transition *rows, const void *bits_prev,
                         const void *bits_next, float gamma, const float *ret, const float *disc, float tau_act,
                         float tau_ptr, float m_alpha, float m_clip, float *q_sa, float *p_sp, float *y_act, float *y_ptr);

/* ---- symmetry augmentation (opt-in) ---------------------------------------
 * Not in the reference.  Off unless these two calls are used; nothing above changes.  The arena is a square with walls,
 * ships are clamped to [0, W-1] and discs are drawn around integer centres, so an observation mirrored or rotated on
 * the pixel grid is (up to sub-pixel effects of the step) an observation of the same game: RAD / DrQ-style
 * augmentation of a sampled minibatch by the eight isometries of the square (the dihedral group D4).
 *
 * An element is g in 0 .. 7: three bits, applied IN THIS ORDER to a position (x, y):                                  */
#define OFX_SYM_TRANSPOSE 1 /* (x, y) -> (y, x); needs width == height                                               */
#define OFX_SYM_FLIP_X    2 /* x -> W - 1 - x                                                                        */
#define OFX_SYM_FLIP_Y    4 /* y -> H - 1 - y                                                                        */
/* g = 0 is the identity, 6 the half turn, 3 and 5 the two quarter turns - the only elements that are not their own
 * inverse.  With a . b = "a first, then b":
 *   inverse [g]    = {0, 1, 2, 5, 4, 3, 6, 7}
 *   compose [a][b] = {{0, 1, 2, 3, 4, 5, 6, 7}, {1, 0, 3, 2, 5, 4, 7, 6}, {2, 5, 0, 7, 6, 1, 4, 3}, {3, 4, 1, 6, 7, 0, 5, 2},
 *                     {4, 3, 6, 1, 0, 7, 2, 5}, {5, 2, 7, 0, 1, 6, 3, 4}, {6, 7, 4, 5, 2, 3, 0, 1}, {7, 6, 5, 4, 3, 2, 1, 0}}
 * Applied to one observation:
 *  - maps: both 1-bit maps (ship, laser; pixel p = y*W + x at bit p & 31 of word p >> 5) satisfy out[y'][x'] = in[y][x]
 *    with (x', y') the image of (x, y).  Every word of the observation is written and nothing outside its 2 * W*H/32
 *    words is touched; the transformation is exact and in place.
 *  - head vec8: elements 2, 3 (pointing) and 6, 7 (position) go through the same map in float32, a flip being
 *    (float)(W - 1) - v: exact for the integer values the engine stores.  Elements 0, 1 (reward, can_shoot) and 4, 5
 *    (dim; invariant because a transpose needs W == H) keep their bits.
 *  - pointer: (px, py) int32 goes through the same map.
 *  - Nothing is clamped: the formula is computed as it stands.  A ship spawned at coordinate W (the spawn's randint is
 *    inclusive) keeps that value until its first thrust, and a flip maps it to -1.
 *
 * ofx_obs_transform applies op[i] to observation i of n_obs: bits [n_obs][2][W*H/32] uint32 in place, vec8 [n_obs][8]
 * and pointer [n_obs][2] when not NULL (all device memory).  op is device memory and cannot be checked on the host: an
 * op[i] above 7, or one with the transpose bit while width != height, leaves observation i untouched.
 * OFX_ERR_INVALID, before anything is launched, for a NULL handle, op or bits, n_obs < 1, width*height no multiple of
 * 128, or a frame whose two maps (W*H/4 bytes) exceed the 64 KB of LDS the packed frame readers are held to.
 *
 * ofx_replay_augment draws one element per row of a gathered batch and applies it to the whole transition:
 *  - bits_prev / bits_next [n][2][W*H/32], head_prev, head_next and (px, py) of rows[n] are transformed in place;
 *    tick_*, frame_*, ship, iaction, reward and done keep their bits (the priority write-backs find a row's ring
 *    position through (tick_prev, ship), which a transformed copy still carries), and so do an n-step gather's ret /
 *    disc, which the call never sees.
 *  - Row d uses Philox counter (arena_base, first + d, draw, stream 8), key = seed, rr = its four words: with
 *    k = popcount(op_mask), the element is the ofx_draw_int(rr[0], k - 1)-th set bit of op_mask in ascending order.
 *    `first` is the row's position in the draw: the chunks of one draw, first = 0, m, 2m, ..., get the operations one
 *    call over all of them would give.
 *  - A padding row (ship < 0) is left as it is; op_out [n] (device uint8, may be NULL) receives each row's element, 0 for
 *    a padding row.
 *  - op_mask == 1 (the identity alone): no kernel is launched; op_out, if given, is zeroed.
 *  - OFX_ERR_INVALID, before anything is launched: a NULL handle, rows or bits; n < 1, first < 0 or first + n >= 2^31;
 *    op_mask with no bit of 0xFF or with a bit above it; an odd (transposing) element allowed while width != height; and
 *    the two frame conditions of ofx_obs_transform.
 * One workgroup per observation, the two maps staged in LDS.  Neither call synchronises.                              */
int ofx_obs_transform(ofx_handle *h, int32_t n_obs, const uint8_t *op, void *bits, float *vec8, int32_t *pointer);
int ofx_replay_augment(ofx_handle *h, uint64_t seed, uint32_t draw, int32_t first, int32_t n, uint32_t op_mask,
                       ofx_transition *rows, void *bits_prev, void *bits_next, uint8_t *op_out);

/* ---- timing helpers (HIP events on the handle's stream) ---------------- */
int ofx_timer_start(ofx_handle *h);
int ofx_timer_stop(ofx_handle *h, float *ms_host); /* synchronises */
/* Non-blocking per-kernel timing for bench.py: record numbered events on the
 * handle's stream (created on first use, idx in [0, 65536)), read the elapsed
 * time between two of them later (synchronises on the second).              */
int ofx_event_record(ofx_handle *h, int32_t idx);
/* When event_base >= 0 every following ofx_policy_forward records events event_base / event_base+1 around its
 * dominant kernel (k_head_stream: upconv2-4 + arg-max) and then advances event_base by 2; it switches itself off
 * when the event ring is full; -1 switches it off.                                                               */
int ofx_policy_profile(ofx_handle *h, int32_t event_base);
int ofx_event_elapsed(ofx_handle *h, int32_t idx_from, int32_t idx_to, float *ms_host);

#ifdef __cplusplus
}
#endif
#endif /* OFX_H */
