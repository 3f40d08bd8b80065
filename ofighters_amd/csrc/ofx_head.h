// ofx_head.h - head-2 tail of the bi-head policy (upconv2 -> upconv3 -> upconv4 -> arg-max) as a row-streaming
// kernel pair (ofx_head.hip); called by policy_forward_impl (ofx_policy.hip).
#pragma once
#include "ofx_internal.h"

struct HeadParams2 {
  int S;                        // policy samples (ships)
  const float *up1;             // planar [S][2][50][50] uprelu1
  const float *w2mf, *b2;       // upconv2 phase weights [20][16] (PrepLayout::w2mf), folded bias [4]
  const float *w2raw;           // BN-folded upconv2 kernel [9][2][4]
  const float *w3mf, *b3;       // upconv3 phase weights [2][36][16] (PrepLayout::w3mf), folded bias [8]
  const float *w3raw;           // BN-folded upconv3 kernel [9][4][8]
  const float *w4eff_c, *b4;    // upconv4 phase weights [ci 8][phase 4][tap 9], bias [1]
  const float *w4raw;           // upconv4 kernel [9][8]
  const float *w2fr, *w3fr;     // frame-line variants of the phase weights (PrepLayout::w2fr, w3fr)
  const float *efr;             // frame phase weights of upconv4 [line h|v][side][parity 2][3][8] (PrepLayout::efr)
  float *u2fr;                  // [S][4][100][4] exact frame lines of uprelu2: row 0, row 99, col 0, col 99
  float *vfr;                   // [S][4][200][9] exact frame lines of the tap planes V_t = sum_c w4[t][c] uprelu3_c (top, bottom, left, right)
  float *c4;                    // [S][1664]     zero-padding corrections of the heat-map frame pixels: four lines of 400, the
                                //               column lines padded with zeros (HC4_*, ofx_head.hip)
  const uint8_t *mask;          // [S] or null
  int32_t *live;                // with a mask: scratch [1 + S], filled here with the count and the ordered list of the
                                // selected ships - workgroup i works on live[1 + i], so the live workgroups are the
                                // FIRST ones of the grid whatever the mask's pattern (spread over XCDs and CUs)
  int live_ready;               // the caller has filled `live` already (ofx_head_compact)
  unsigned long long *best;     // [S] packed (ordered value << 32) | ~index, zeroed by the caller
  float *heat;                  // [S][400][400] or null
  const int32_t *probe;         // [S][2] (x, y) or null
  float *ptr_probe;             // [S] heat-map value at the probe
  int frames_ref;               // frame lines through the from-the-definition kernel (OFX_OPT_FRAMES_REF)
  int legacy;                   // TF1 legacy bilinear instead of half-pixel centres (OFX_OPT_BILINEAR_LEGACY)
  int bf16;                     // OFX_OPT_POLICY_BF16: 1 bf16 / 2 fp16 operands in upconv3 (opt-in, not the default)
  int event_base;               // >= 0: ofx_event_record(event_base / event_base + 1) around k_head_stream
  int ablate;                   // diagnostics (OFX_HEAD_HOOKS builds only)
  unsigned long long *dbg;      // diagnostics: [blocks][8 waves][6] s_memtime sums
  // ---- Boltzmann sampling of the pointer (ofx_policy_act_boltzmann): k_head_stream_sample instead of k_head_stream
  int sample;                   // != 0: the sampling kernel; `best`, `heat` and the probe are not used
  int M, arena_base;            // ships per arena, first global arena of the handle: the noise is keyed by (global arena, ship)
  unsigned nk0, nk1, ntick;     // Philox key (the seed's halves) and the tick of the noise
  const float *t_ptr;           // [S] temperature of the ship's arena (0 = greedy: no noise is drawn)
  unsigned long long *cand_key; // [S][8] per consumer wave (2 strips x 4): (ordered perturbed value << 32) | ~index, 0 = none
  float *cand_raw;              // [S][8] the raw heat-map value at that candidate's pixel
  unsigned *cand_max;           // [S][8] the wave's raw maximum as an ordered word (hd_ordered_f32)
  // ---- soft value of the pointer head (ofx_policy_forward_obs_soft): k_head_stream_soft instead of k_head_stream (fp32)
  float soft_k;                 // != 0: the soft kernel; log2(e) / T, one temperature for the launch
  float *soft_m, *soft_z;       // [S][8] per consumer wave (the slots of cand_*): its maximum and sum exp((v - m) / T)
};

#ifdef __HIPCC__
// Standard Gumbel noise from one Philox word r, in float32: w = (r + 0.5) / 2^32, E = -ln(1 - w), g = -ln(E).
// Rounding 1 - w to float32 would quantise g by about 1e-2 around g = 12, the tail that wins among 160 000 pixels, so
// E never goes through a rounded 1 - w:
//   r <  2^30 (w < 1/4)  E = 2 atanh(s), s = w / (2 - w), as an odd series up to s^9 (truncation below 3e-10 relative)
//   otherwise            1 - w = (2 k + 1) / 2^33 with k = ~r, so E = ln 2 (33 - log2(2 k + 1)), E >= 0.287
// and the two logs are the hardware's (v_log_f32, 1 ulp of the base-2 logarithm: below 4e-6 at |log2| <= 33).
// Largest |g - float64| over the edge words and 2^20 Philox words, measured on the MI355X: 9.3e-6, at words just above
// 2^30 where E is smallest on the second route (include/ofx.h; the contract's bound is 1e-4).
// Every multiply-add is an explicit fmaf and no product feeds a sum: the function gives the same bits in every
// translation unit, whatever its contraction setting (k_head_stream_sample, k_policy_boltz_finish, k_head_gumbel).
__device__ __forceinline__ float hd_gumbel(unsigned r) {
  const float w = fmaf((float)r, 0x1p-32f, 0x1p-33f);
  const float s = w * __builtin_amdgcn_rcpf(2.f - w), s2 = s * s;
  float q = fmaf(s2, 1.f / 9.f, 1.f / 7.f);
  q = fmaf(s2, q, 1.f / 5.f);
  q = fmaf(s2, q, 1.f / 3.f);
  q = fmaf(s2, q, 1.f);
  const float e_lo = 2.f * s * q;
  const float m = fmaf((float)(~r), 2.f, 1.f);
  const float e_hi = 0.693147180559945f * (33.f - __builtin_amdgcn_logf(m));
  const float E = r < 0x40000000u ? e_lo : e_hi;
  return -0.693147180559945f * __builtin_amdgcn_logf(E);
}

// Soft value of the pointer head (k_head_stream_soft, k_policy_soft_finish): exp((v - m) / T) as v_exp_f32((v - m) * k),
// k = log2(e) / T.  The difference is formed first and rounded on its own (v * k - m * k would carry the rounding of
// m * k, |m| / T ulps, into every term alike).  m >= v: the argument is <= 0 and the term in [0, 1]; v = m gives 1.
__device__ __forceinline__ float hd_soft_w(float v, float m, float k) { return __builtin_amdgcn_exp2f((v - m) * k); }
typedef float hd_f32x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ hd_f32x4 hd_soft_exp4(hd_f32x4 v, float m, float k) {
  const hd_f32x4 x = (v - (hd_f32x4){m, m, m, m}) * (hd_f32x4){k, k, k, k};
  return (hd_f32x4){__builtin_amdgcn_exp2f(x[0]), __builtin_amdgcn_exp2f(x[1]), __builtin_amdgcn_exp2f(x[2]), __builtin_amdgcn_exp2f(x[3])};
}
// a partial sum z over maximum m, rescaled to the maximum M >= m of a merge; a part that holds no value (m = -inf, an
// idle lane) weighs nothing
__device__ __forceinline__ float hd_soft_term(float m, float z, float M, float k) {
  return m > -INFINITY ? z * hd_soft_w(m, M, k) : 0.f;
}
#endif

// bytes of the three frame buffers for S samples
size_t ofx_head_frame_bytes(size_t S, size_t *u2fr, size_t *vfr, size_t *c4);
// mask [S] -> live[0] = count, live[1 + i] = i-th selected ship (one workgroup, a scan)
int ofx_head_compact(ofx_handle *h, int S, const uint8_t *mask, int32_t *live);
// k_head_frames + k_head_stream on the handle's stream
int ofx_launch_head(ofx_handle *h, const HeadParams2 &p);
// g[i] = hd_gumbel(words[i]) on the handle's stream (ofx_policy_gumbel)
int ofx_head_gumbel(ofx_handle *h, const uint32_t *words, int n, float *g);
