// ofx_internal.h - handle layout and helpers shared by the HIP translation
// units of libofx.so (gfx950 only; no CPU fallback, no CUDA shims).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/ofx.h"
#include "ofx_rng.h"

#define OFX_WAVE 64
#define OFX_ARENAS_PER_BLOCK 4 /* one 64-lane wave per arena, 256-thread blocks */
static inline int arena_blocks(int N) { return (N + OFX_ARENAS_PER_BLOCK - 1) / OFX_ARENAS_PER_BLOCK; }

void ofx_set_error(const char *fmt, ...);

#define OFX_HIP(call)                                                                  \
  do {                                                                                 \
    hipError_t _e = (call);                                                            \
    if (_e != hipSuccess) {                                                            \
      ofx_set_error("%s failed: %s (%s:%d)", #call, hipGetErrorString(_e), __FILE__,   \
                    __LINE__);                                                         \
      return OFX_ERR_HIP;                                                              \
    }                                                                                  \
  } while (0)

// Structure-of-arrays arena state, all in HBM.  Ships: [N][M]; lasers [N][L];
// per-arena scalars [N].  A wave reads one arena's M ship words / 64 laser
// slots as one coalesced segment per array.
struct ofx_state {
  int32_t *ship_x, *ship_y, *ship_px, *ship_py, *hull;
  int32_t *reward, *score, *obs_reward, *last_score;
  uint8_t *alive;
  int16_t *killer;
  int32_t *time, *n_lasers;
  double *laser_x, *laser_y, *laser_dx, *laser_dy;
  uint8_t *laser_owner, *laser_dead;
  unsigned long long *overflow;    // [1]
  long long *episode_sums;         // [M+1]
};

struct ofx_replay;  // ofx_replay.hip
struct ofx_population;  // ofx_evolve.hip: the stored population
struct ofx_es;          // ofx_es.hip: the centre of the evolution strategy

struct ofx_handle {
  ofx_config cfg;
  hipStream_t stream;
  bool own_stream;
  bool spawned;
  ofx_state st;
  double hit_thresh;               // largest d2 with rn(sqrt(d2)) <= r_laser + r_ship
  // observation maps (lazily allocated per type): [type][which]
  void *maps[5][2];
  int32_t *bot_behaviours;         // device [M]
  // scratch for nn / policy
  void *scratch;
  size_t scratch_bytes;
  hipEvent_t ev0, ev1;
  bool events;
  hipEvent_t *ring;                // numbered events for ofx_event_record
  int ring_n;
  int prof_base;                   // ofx_policy_profile: next event pair, -1 = off
  ofx_replay *replay;              // transition memory (ofx_replay_create), null = none
  // Hand-carved blocks (aux, fitws, fitws2, applyws, scratch under the forward): each is laid out by one function on an
  // Arena (ofx_arena.h), run once to measure and once on the block; the buffers and their counts are stated there alone.
  void *aux;                       // temporaries of ofx_dqn_targets (grown on demand)
  size_t aux_bytes;
  void *fitws;                     // workspace of ofx_dqn_fit / ofx_dqn_fit_reference, kept between calls (a fresh 4 GB
  size_t fitws_bytes;              // hipMalloc per replay cost ~60 ms of mapping: r03), grown on demand
  void *fitws2;                    // the reference form's dense targets, kept likewise
  size_t fitws2_bytes;
  void *applyws;                   // ofx_dqn_apply's {loss, norm, factor} slot and norm partials (2.3 KB), kept likewise
  size_t applyws_bytes;
  int32_t *counter;                // [4] small device counters, one slot per user (ofx_counter; allocated on first use)
  int32_t *res_iaction;            // [N*M]    (iaction, ipointer) of the last ofx_policy_forward / ofx_policy_explore that
  int32_t *res_ipointer;           // [N*M][2] was given null result pointers (ofx_policy_results: one block, allocated on first use)
  float *prep;                     // prepared policy weights (BN folded, phase weights, tables): ofx_policy.hip
  float *prep_tmp;                 // the same for a blob that is not the pinned one (rebuilt per forward)
  const float *prep_pinned;        // the blob `prep` was built from while it is pinned (ofx_policy_pin_weights)
  int opt_trunk_fuse;              // OFX_OPT_TRUNK_FUSE: 0 auto, 1 always, 2 never
  int n_cus;                       // compute units of the device (grid of the persistent trunk kernel)
  bool opt_trunk_plain, opt_frames_ref, opt_bilinear_legacy;  // ofx_set_option
  int opt_policy_lowp;             // OFX_OPT_POLICY_BF16: 0 fp32, 1 bf16 operands, 2 fp16 operands (opt-in)
  bool opt_fit_plain;              // OFX_OPT_FIT_PLAIN: the fit's layer-by-layer form (test reference)
  // OFX_OPT_TRUNK_SPARSE is tri-state.  Never set (both false): the streaming trunk skips constant windows (exact), no
  // counters.  1: the same with the counters of ofx_policy_trunk_stats.  0: the dense kernel for the live forward
  // (diagnostic, the reference of the == tests); the forwards on stored observations stay sparse.
  bool opt_trunk_dense, opt_trunk_count;
  unsigned long long *trunk_stat;  // [6] device counters of the sparse trunk (allocated with value 1 of the option)
  // ofx_policy_act (one block, allocated at its first call): the four value arrays a null output stands for, then the
  // forward's results they are selected from and the pre-drawn exploration
  float *act_vals;                 // one packed block: q_sa, p_sp, v_act, v_ptr [N*M] each, then ... (act_block, ofx_policy.hip)
  bool act_called;                 // the LAST ofx_policy_act wrote all four of the handle's arrays (all outputs NULL)
  double *eps_expo;                // [N] ofx_policy_epsilon_ladder: arena a explores at epsilon^eps_expo[a] (+inf: never); null = no ladder
  // ofx_restart_finished (one allocation at its first call, null before): per-arena episode counter, the ships seen
  // dead by one call already, and the arenas the last call restarted
  uint32_t *ar_episode;            // [N]
  uint8_t *ar_dead_once;           // [N][M]
  uint8_t *ar_restarted;           // [N]
  int32_t *ar_want;                // [N] ofx_es_requeue: the tickets each arena asks for (allocated at its first call)
  ofx_population *population;      // genomes of the neuroevolution (ofx_population_create), null = none
  ofx_es *es;                      // centre of the evolution strategy (ofx_es_create), null = none
};
#define OFX_RING_MAX 65536         /* numbered events of ofx_event_record */

// kernels / launchers implemented in the other translation units
int ofx_launch_raster(ofx_handle *h, int map_type, void *ship_map, void *laser_map);
int ofx_ensure_buffer(ofx_handle *h, void **buf, size_t *have, size_t bytes);  // a handle-kept block, grown on demand
int ofx_ensure_scratch(ofx_handle *h, size_t bytes);   // h->scratch; transient: the next caller may overwrite or re-allocate it
enum { OFX_COUNTER_PADS, OFX_COUNTER_FIRST_DONE };      // slots of the handle's counter block
int ofx_counter(ofx_handle *h, int slot, int32_t **counter);
// the handle's own (iaction [N*M], ipointer [N*M][2]): what a null result pointer of ofx_policy_forward /
// ofx_policy_explore / ofx_policy_actions / ofx_replay_capture stands for
int ofx_policy_results(ofx_handle *h, int32_t **iaction, int32_t **ipointer);
// the handle's (q_sa, p_sp, v_act, v_ptr) [N*M] of ofx_policy_act; OFX_ERR_STATE unless the last one wrote all four
int ofx_policy_act_values(ofx_handle *h, const float **q_sa, const float **p_sp, const float **v_act, const float **v_ptr);
void ofx_replay_free(ofx_handle *h);
void ofx_population_free(ofx_handle *h);
void ofx_es_free(ofx_handle *h);
int ofx_replay_episode_reset(ofx_handle *h, const uint8_t *arena_mask);
// C[M][N] = act(A[M][K] (lda) x B[K][N] (ldb) + bias[N]) on the f32 MFMA (k_gemm_f32, ofx_policy.hip)
int ofx_launch_gemm(ofx_handle *h, const float *A, int lda, const float *B, int ldb, const float *bias, float *C, int ldc,
                    int M, int N, int K, int relu, const int32_t *live = nullptr);
int ofx_policy_weights_updated(ofx_handle *h, const float *weights);  // the blob was changed in place (ofx_dqn_fit)
// model.predict on n stored observations: act_values [n][2], heatmap [n][H][W], ptr_max [n] (any may be null)
int ofx_policy_predict_obs(ofx_handle *h, const float *weights, int32_t n_obs, const void *bits, const float *vec8,
                           float *act_values, float *heatmap, float *ptr_max);

#define OFX_MAP_BITS_LSB 4 /* internal: 1 bit / cell, pixel p -> bit (p & 31) of word p >> 5 */

#include "ofx_sim.h"  // the arena rules more than one kernel applies: bots' law, reset draw, observation head
