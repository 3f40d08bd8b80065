// ofx_policy.hip - bi-head "pointer_model" forward for every (arena, ship)
// (agents/qlearnIA_V2.py:123-190 graph, :206-220 inference glue, :447-454
// action packing).  fp32 like Keras.  Conventions (BN eps 1e-3, HWIO kernels,
// (h,w,c) flatten, vector-first concat, half-pixel bilinear x2) are the ones
// declared in oracle/policy_oracle.c; parity of this path is UNPINNED
// (keras/tensorflow and weights are absent), it is checked against that
// restatement with an fp32 tolerance.
//
//
// Work split (what is shared per arena):
//   trunk   4 x [conv3x3 + BN + ReLU + maxpool2]   once per ARENA  (image is the same for its ships): ofx_trunk.hip
//   dense1  [5008 -> 100]: the 5000 trunk features once per arena on MFMA
//           (v_mfma_f32_32x32x2_f32, exact fp32), the 8-scalar head per ship
//   head-1  dense2 + output1 per ship (VALU, tiny)
//   head-2  updense1 [100 -> 625] on MFMA, then 4 x [bilinear x2 + conv3x3]
//           per ship: upconv1 here (1 -> 2 @ 50x50, bilinear up-sampling fused into its LDS staging), upconv2-4 + arg-max
//           in the row-streaming kernel of ofx_head.hip (4-phase low-resolution form, the (400,400) heat-map is only
//           materialised on request).
//
// This unit: the blob and prepared-weight layouts (BatchNorm is folded into the conv weights by k_policy_prepare, for
// the trunk and the head alike), the dense-layer kernels, the forward's driver, explore and action packing.
#include <string.h>

#include "ofx_internal.h"
#include "ofx_arena.h"
#include "ofx_blob.h"
#include "ofx_trunk.h"
#include "ofx_head.h"

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

// ---- user blob layout (ofx_blob.h) -------------------------------------------------

extern "C" int ofx_policy_layout(const ofx_handle *h, ofx_policy_desc *desc) {
  (void)h;
  if (!desc) { ofx_set_error("ofx_policy_layout: null desc"); return OFX_ERR_INVALID; }
  memset(desc, 0, sizeof(*desc));
  desc->n_tensors = policy_layout(desc->offset, desc->count);
  desc->n_floats = desc->offset[desc->n_tensors];
  return OFX_OK;
}

// ---- prepared (BN-folded) weights ------------------------------------------------
struct PrepLayout {
  int tw[4], tb[4];   // trunk folded kernels [9][cin][8], biases [8]
  int uw[3], ub[3];   // upconv1..3 folded
  int w3mf;           // [half 2][k = tap*4 + ci (36)][n = phase*4 + co_local (16)]  MFMA B operand
  int w2mf;           // upconv2 in phase form: [k = tap*2 + ci (18, padded to 20)][n = phase*4 + co (16)]
  int w2fr;           // [variant top|bottom|left|right][20][16]: w2mf with the taps that fall into the zero padding of the
                      // variant's frame line dropped (k_head_frames: exact frame bands of uprelu2)
  int w3fr;           // [variant][k = tap*4 + ci (36)][n = parity*8 + co (16)]: upconv3 phase weights of one frame line
                      // (top / bottom: row phase fixed, n's parity = column phase; left / right the other way round)
  int w4eff_c;        // [8 ci][4 phases][9 taps] (fused kernel: one contiguous slice per input channel)
  int w4raw;          // [9][8]
  int efr;            // [line h|v][side first|last][parity 2][low-res offset 3][ci 8]: phase weights of the taps of
                      // upconv4 that fall into the zero padding of a frame pixel (k_head_tail border pass)
  int b4;             // [1]
  int zero16;         // [4] zeros (never written: the block is cleared when it is allocated)
  int wbm[3];         // conv2..4: the banded B operand of k_convm laid out per lane: [j 24][lane 64]
  int lut1;           // conv1 on the binary maps as a table: [ci 2][3x3 bit pattern 512][co 8] = sum of the folded
                      // weights of the set taps (k_conv1_lut)
  int total;
};

static PrepLayout prep_layout() {
  PrepLayout L;
  int off = 0;
  for (int i = 0; i < 4; i++) { L.tw[i] = off; off += 9 * kTrunkCin[i] * 8; L.tb[i] = off; off += 8; }
  for (int i = 0; i < 3; i++) { L.uw[i] = off; off += 9 * kUpCin[i] * kUpCout[i]; L.ub[i] = off; off += kUpCout[i]; }
  L.w3mf = off; off += 36 * 32;
  L.w2mf = off; off += 20 * 16;
  L.w2fr = off; off += 4 * 20 * 16;
  L.w3fr = off; off += 4 * 36 * 16;
  L.w4eff_c = off; off += 8 * 4 * 9;
  L.w4raw = off; off += 72;
  L.efr = off; off += 2 * 2 * 2 * 3 * 8;
  L.b4 = off; off += 1;
  off = (off + 3) & ~3;
  L.zero16 = off; off += 4;      // 16 zero bytes, 16-byte aligned: the source of the padding cells of k_conv3_stream's LDS-direct loads
  L.lut1 = off; off += 2 * 512 * 8;
  for (int i = 0; i < 3; i++) { L.wbm[i] = off; off += 24 * 64; }
  L.total = (off + 63) & ~63;
  return L;
}

struct PrepParams {
  const float *w;
  float *prep;
  int src_k[7], src_b[7], src_g[7], cin[7], cout[7], dst_w[7], dst_b[7];
  int src_k4, src_b4, dst_w4raw, dst_b4, dst_efr;
  int dst_w4eff_c, dst_w3mf, dst_w2mf, dst_w2fr, dst_w3fr, dst_lut1, dst_wbm[3];
  int phase;
  int legacy;                      // OFX_OPT_BILINEAR_LEGACY
};

// interpolation coefficients of the x2 bilinear up-sampling: output row 2i+a, conv tap dy in {-1,0,1} touches low-res
// rows i-1, i, i+1 with these weights.  Half-pixel centres (default): up[2i] = .25 L[i-1] + .75 L[i],
// up[2i+1] = .75 L[i] + .25 L[i+1].  Legacy (TF1 resize_bilinear, OFX_OPT_BILINEAR_LEGACY): up[2i] = L[i],
// up[2i+1] = .5 L[i] + .5 L[i+1].  Both clamp at the edge, so the phase form and its frame handling are the same.
__device__ inline float up_coef(int a, int dy, int t, int legacy) {
  // a=0: dy-1 -> row 2i-1, dy0 -> row 2i, dy+1 -> row 2i+1 ; a=1: rows 2i, 2i+1, 2i+2
  const float c0[3][3] = {{0.75f, 0.25f, 0.f}, {0.25f, 0.75f, 0.f}, {0.f, 0.75f, 0.25f}};
  const float c1[3][3] = {{0.25f, 0.75f, 0.f}, {0.f, 0.75f, 0.25f}, {0.f, 0.25f, 0.75f}};
  const float l0[3][3] = {{0.5f, 0.5f, 0.f}, {0.f, 1.f, 0.f}, {0.f, 0.5f, 0.5f}};
  const float l1[3][3] = {{0.f, 1.f, 0.f}, {0.f, 0.5f, 0.5f}, {0.f, 0.f, 1.f}};
  if (legacy) return a ? l1[dy][t] : l0[dy][t];
  return a ? c1[dy][t] : c0[dy][t];
}

// Two launches: phase 0 (many workgroups) folds and builds every table that depends on the raw weights only; phase 1
// builds what needs the folded kernels (k_convm's per-lane B operands).
__global__ void k_policy_prepare(PrepParams p) {
  const int tid = blockIdx.x * blockDim.x + threadIdx.x, nthr = gridDim.x * blockDim.x;
  if (p.phase == 0) {
  for (int l = 0; l < 7; l++) {  // BN fold: y = (conv + b) * inv + (beta - mean * inv)
    const int cin = p.cin[l], cout = p.cout[l];
    const float *g = p.w + p.src_g[l];  // gamma, beta, mean, var consecutive, each [cout]
    for (int e = tid; e < 9 * cin * cout; e += nthr) {
      const int co = e % cout;
      const float inv = g[co] / sqrtf(g[3 * cout + co] + 1e-3f);
      p.prep[p.dst_w[l] + e] = p.w[p.src_k[l] + e] * inv;
    }
    for (int co = tid; co < cout; co += nthr) {
      const float inv = g[co] / sqrtf(g[3 * cout + co] + 1e-3f);
      p.prep[p.dst_b[l] + co] = p.w[p.src_b[l] + co] * inv + (g[cout + co] - g[2 * cout + co] * inv);
    }
  }
  // upconv4 (linear, no BN): effective weights of the 4 output phases on the low-res grid
  for (int e = tid; e < 4 * 9 * 8; e += nthr) {
    const int ci = e % 8, tap = (e / 8) % 9, ph = e / 72;
    const int a = ph >> 1, b = ph & 1, ty = tap / 3, tx = tap % 3;
    float acc = 0.f;
    for (int dy = 0; dy < 3; dy++)
      for (int dx = 0; dx < 3; dx++)
        acc += p.w[p.src_k4 + (dy * 3 + dx) * 8 + ci] * (up_coef(a, dy, ty, p.legacy) * up_coef(b, dx, tx, p.legacy));
    p.prep[p.dst_w4eff_c + (ci * 4 + ph) * 9 + tap] = acc;
  }
  for (int e = tid; e < 72; e += nthr) p.prep[p.dst_w4raw + e] = p.w[p.src_k4 + e];
  // frame pixels of the heat map: the conv taps of the row (column) outside the image, in phase form along the
  // line: pixel 2j + b of the line gets sum_o E[b][o] L[j + o - 1] of the low-res frame row (column) L
  for (int e = tid; e < 2 * 2 * 2 * 3 * 8; e += nthr) {
    const int ci = e % 8, o = (e / 8) % 3, b = (e / 24) % 2, side = (e / 48) % 2, isv = e / 96;
    float acc = 0.f;
    for (int d = 0; d < 3; d++) {
      const int tap = isv ? d * 3 + (side ? 2 : 0) : (side ? 2 : 0) * 3 + d;
      acc += p.w[p.src_k4 + tap * 8 + ci] * up_coef(b, d, o, p.legacy);
    }
    p.prep[p.dst_efr + e] = acc;
  }
  // upconv3 (layer index 6): phase weights from the BN-folded kernel (folded in place, same thread order
  // would race with the fold above: recompute the fold here)
  {
    const int cout = 8, cin = 4;
    const float *g = p.w + p.src_g[6];
    for (int e = tid; e < 4 * 9 * cin * cout; e += nthr) {
      const int co = e % cout, ci = (e / cout) % cin, tap = (e / (cout * cin)) % 9, ph = e / (cout * cin * 9);
      const int a = ph >> 1, b = ph & 1, ty = tap / 3, tx = tap % 3;
      const float inv = g[co] / sqrtf(g[3 * cout + co] + 1e-3f);
      float acc = 0.f;
      for (int dy = 0; dy < 3; dy++)
        for (int dx = 0; dx < 3; dx++)
          acc += (p.w[p.src_k[6] + ((dy * 3 + dx) * cin + ci) * cout + co] * inv) * (up_coef(a, dy, ty, p.legacy) * up_coef(b, dx, tx, p.legacy));
      p.prep[p.dst_w3mf + ((co >> 2) * 36 + tap * 4 + ci) * 16 + ph * 4 + (co & 3)] = acc;
    }
  }
  // conv1 (layer 0) reads two BINARY maps: the response of a 3x3 window of one map is one of 512 values per output
  // channel.  Same fold as above (recomputed: the in-place fold may still be running in other threads); bit
  // (dy*3 + dx) of the pattern <-> tap (dy, dx), taps summed in tap order.
  {
    const float *g = p.w + p.src_g[0];
    for (int e = tid; e < 2 * 512 * 8; e += nthr) {
      const int co = e & 7, pat = (e >> 3) & 511, ci = e >> 12;
      const float inv = g[co] / sqrtf(g[3 * 8 + co] + 1e-3f);
      // the folded bias rides in the table of channel 0: out = LUT[0][pattern0] + LUT[1][pattern1]
      float acc = ci == 0 ? p.w[p.src_b[0] + co] * inv + (g[8 + co] - g[2 * 8 + co] * inv) : 0.f;
      for (int tap = 0; tap < 9; tap++)
        if ((pat >> tap) & 1) acc += p.w[p.src_k[0] + (tap * 2 + ci) * 8 + co] * inv;
      p.prep[p.dst_lut1 + e] = acc;
    }
  }
  // upconv2 (layer index 5): the same for the 2 -> 4 layer, K padded from 18 to 20 with zero rows
  {
    const int cout = 4, cin = 2;
    const float *g = p.w + p.src_g[5];
    for (int e = tid; e < 20 * 16; e += nthr) {
      const int n = e % 16, k = e / 16, co = n & 3, ph = n >> 2, ci = k & 1, tap = k >> 1;
      float acc = 0.f;
      if (k < 18) {
        const int a = ph >> 1, b = ph & 1, ty = tap / 3, tx = tap % 3;
        const float inv = g[co] / sqrtf(g[3 * cout + co] + 1e-3f);
        for (int dy = 0; dy < 3; dy++)
          for (int dx = 0; dx < 3; dx++)
            acc += (p.w[p.src_k[5] + ((dy * 3 + dx) * cin + ci) * cout + co] * inv) * (up_coef(a, dy, ty, p.legacy) * up_coef(b, dx, tx, p.legacy));
      }
      p.prep[p.dst_w2mf + e] = acc;
    }
  }
  // frame-line variants of the phase weights (k_head_frames): the conv taps that fall into the zero padding of the
  // variant's frame line are left out.  v = 0 top (row phase 0 loses dy = 0), 1 bottom (row phase 1 loses dy = 2),
  // 2 left (column phase 0 loses dx = 0), 3 right (column phase 1 loses dx = 2)
  {
    const float *g2 = p.w + p.src_g[5], *g3 = p.w + p.src_g[6];
    for (int e = tid; e < 4 * 20 * 16; e += nthr) {
      const int n = e % 16, k = (e / 16) % 20, v = e / 320, co = n & 3, ph = n >> 2, ci = k & 1, tap = k >> 1;
      float acc = 0.f;
      if (k < 18) {
        const int a = ph >> 1, b = ph & 1, ty = tap / 3, tx = tap % 3;
        const float inv = g2[co] / sqrtf(g2[3 * 4 + co] + 1e-3f);
        for (int dy = 0; dy < 3; dy++)
          for (int dx = 0; dx < 3; dx++) {
            const bool drop = (v == 0 && a == 0 && dy == 0) || (v == 1 && a == 1 && dy == 2) || (v == 2 && b == 0 && dx == 0) ||
                              (v == 3 && b == 1 && dx == 2);
            if (!drop) acc += (p.w[p.src_k[5] + ((dy * 3 + dx) * 2 + ci) * 4 + co] * inv) * (up_coef(a, dy, ty, p.legacy) * up_coef(b, dx, tx, p.legacy));
          }
      }
      p.prep[p.dst_w2fr + e] = acc;
    }
    for (int e = tid; e < 4 * 36 * 16; e += nthr) {
      const int n = e % 16, k = (e / 16) % 36, v = e / 576, co = n & 7, q = n >> 3, ci = k & 3, tap = k >> 2;
      const int a = v == 0 ? 0 : v == 1 ? 1 : q, b = v == 2 ? 0 : v == 3 ? 1 : q, ty = tap / 3, tx = tap % 3;
      const float inv = g3[co] / sqrtf(g3[3 * 8 + co] + 1e-3f);
      float acc = 0.f;
      for (int dy = 0; dy < 3; dy++)
        for (int dx = 0; dx < 3; dx++) {
          const bool drop = (v == 0 && dy == 0) || (v == 1 && dy == 2) || (v == 2 && dx == 0) || (v == 3 && dx == 2);
          if (!drop) acc += (p.w[p.src_k[6] + ((dy * 3 + dx) * 4 + ci) * 8 + co] * inv) * (up_coef(a, dy, ty, p.legacy) * up_coef(b, dx, tx, p.legacy));
        }
      p.prep[p.dst_w3fr + e] = acc;
    }
  }
  if (tid == 0) p.prep[p.dst_b4] = p.w[p.src_b4];
  } else {
  // k_convm's B operand for the 8 -> 8 layers, exactly as lane (n = (co, r), kq) of MFMA step j wants it:
  // B[k = 4 j + kq][(co, r)] = w[row - r][dx][ci][co] for k = (row * 3 + dx) * 8 + ci inside the 3-row window, else 0
  for (int l = 1; l < 4; l++)
    for (int e = tid; e < 24 * 64; e += nthr) {
      const int lane = e & 63, j = e >> 6, n16 = lane & 15, kq = lane >> 4, co = n16 >> 1, r = n16 & 1;
      const int k = 4 * j + kq, rd = k >> 3, ci = k & 7, row = rd / 3, dx = rd - row * 3, tr = row - r;
      p.prep[p.dst_wbm[l - 1] + e] = (tr >= 0 && tr < 3) ? p.prep[p.dst_w[l] + ((tr * 3 + dx) * 8 + ci) * 8 + co] : 0.f;
    }
  }
}

// ---- upconv1 (1 -> 2 channels @ 50x50 behind a x2 bilinear up-sampling of the 25x25 dense output) --------------------
// One workgroup per policy sample: the zero-padded up-sampled plane lives in LDS (the generic k_conv gathered every
// staged cell from global memory with four loads: 0.26 ms for 32768 ships; this form 0.19 for 0.66 GB of output,
// profiles/r19_head_front.txt).  Up-sample x first, then y (the restatement's order), taps in (dy, dx) order with fma,
// bias behind the sum, ReLU.  A thread owns 10 adjacent pixels of a row.
//
// The up-sampling pass has no index arithmetic per cell: the source indices and the weight of an up-res coordinate
// g = 2 k + odd are a closed form of (k, odd) - half-pixel centres: odd -> (k, k + 1, .25), even -> (k - 1, k, .75);
// legacy (src = g / 2): (k, k + 1, odd ? .5 : 0), both clamped to 0 .. 24 - and a thread keeps its column: thread
// (seg, c) of the first 208 owns column c of the padded plane on the rows R .. R + n - 1 of segment seg (R = 0, 14, 26,
// 40, n = 14, 12, 14, 12).  Every R is even, so the row pair (R + 2 m, R + 2 m + 1) = up-res rows 2 (K + m) - 1 and
// 2 (K + m), K = R / 2, takes the same two x-interpolated source rows K + m - 1, K + m (legacy: the second row of the
// pair takes K + m, K + m + 1) and all row indices are compile-time offsets from K.  The x-interpolated values of the
// thread's column on its 8 (9) source rows come straight from global memory - 16 (18) loads in flight, no staging of
// the 625 inputs, one barrier less - and each is used by up to four rows.  Per cell that leaves the two lerps, written
// as before: top = a + (b - a) lx (the same value for every row that uses it), v = top + (bot - top) ly.
template <bool LEGACY>
__global__ __launch_bounds__(256) void k_upconv1(ConvParams p) {
  __shared__ float up[52][53];   // up-sampled plane with its zero frame; pitch 53: the 5 segments of a row start on different banks
  __shared__ __align__(16) float outs[5000];   // the ship's output block, stored with 16-byte lines (below)
  const int tid = threadIdx.x;
  const int seg = tid / 52, c = tid - 52 * seg;             // seg 4 (tid >= 208): no up-sampling work
  const int R = 13 * seg + (seg & 1), K = R >> 1, nrow = 14 - 2 * (seg & 1);
  const int gx = c - 1, kx = gx >> 1, oddx = gx & 1;        // gx = -1, 50: the zero frame
  const bool colv = gx >= 0 && gx < 50;
  const int xa = min(max(LEGACY ? kx : kx - 1 + oddx, 0), 24), xb = min(max(LEGACY ? kx + 1 : kx + oddx, 0), 24);
  const float lx = LEGACY ? (oddx ? 0.5f : 0.f) : (oddx ? 0.25f : 0.75f);
  constexpr int nt = LEGACY ? 9 : 8;                       // source rows K - 1 .. K + nt - 2 (clamped)
  // work item it = the it-th ship (of the ordered list `live` with a mask): a bounded grid walks the items, so a
  // masked launch pays for its selected ships only (32768 workgroups that exit at once cost 0.13 ms)
  const int n_items = p.live ? p.live[0] : p.images;
#pragma unroll 1
  for (int it = blockIdx.x; it < n_items; it += gridDim.x) {
  const int img = p.live ? p.live[1 + it] : it;
  float t[9];
  if (tid < 208) {
    const float *src = p.in + (size_t)img * 625;
    float a[9], b[9];
#pragma unroll
    for (int i = 0; i < 9; i++)
      if (i < nt) {
        const unsigned y25 = 25u * (unsigned)min(max(K - 1 + i, 0), 24);   // uniform base + 32-bit lane offset
        a[i] = src[y25 + (unsigned)xa];
        b[i] = src[y25 + (unsigned)xb];
      }
#pragma unroll
    for (int i = 0; i < 9; i++) t[i] = i < nt ? a[i] + (b[i] - a[i]) * lx : 0.f;
  }
  __syncthreads();  // the previous item's readers of up are done
  if (tid < 208) {
#pragma unroll
    for (int j = 0; j < 14; j++) {
      const int m = j >> 1, r = R + j;
      float v;
      if constexpr (LEGACY) {
        const float top = t[m + (j & 1)], bot = t[m + (j & 1) + 1];
        v = top + (bot - top) * ((j & 1) ? 0.f : 0.5f);
      } else {
        const float top = t[m], bot = t[m + 1];
        v = top + (bot - top) * ((j & 1) ? 0.75f : 0.25f);
      }
      if (j < nrow) up[r][c] = (colv && r >= 1 && r <= 50) ? v : 0.f;
    }
  }
  __syncthreads();
  if (tid < 250) {
  const int row = tid / 5, x0 = 10 * (tid - 5 * row);
  float acc[2][10];
#pragma unroll
  for (int co = 0; co < 2; co++)
#pragma unroll
    for (int i = 0; i < 10; i++) acc[co][i] = 0.f;
#pragma unroll
  for (int dy = 0; dy < 3; dy++) {
    float v[12];
#pragma unroll
    for (int i = 0; i < 12; i++) v[i] = up[row + dy][x0 + i];
#pragma unroll
    for (int dx = 0; dx < 3; dx++)
#pragma unroll
      for (int co = 0; co < 2; co++) {
        const float wv = p.w[(dy * 3 + dx) * 2 + co];  // uniform -> scalar load
#pragma unroll
        for (int i = 0; i < 10; i++) acc[co][i] = __builtin_fmaf(v[i + dx], wv, acc[co][i]);
      }
  }
#pragma unroll
  for (int co = 0; co < 2; co++) {
    const float bias = p.b[co];
    float *o = outs + (co * 50 + row) * 50 + x0;
#pragma unroll
    for (int i = 0; i < 10; i += 2)
      *reinterpret_cast<float2 *>(o + i) = make_float2(fmaxf(acc[co][i] + bias, 0.f), fmaxf(acc[co][i + 1] + bias, 0.f));
  }
  }  // tid < 250
  // a thread's 10 pixels are 40 bytes apart from its neighbour's: stored from the registers, every store instruction
  // touched each 128-byte line of the block with 8 bytes per lane (0.211 ms for 32768 ships).  Through LDS the block
  // leaves as 1250 consecutive float4 (0.183 ms).  The next item writes `outs` behind its two barriers.
  __syncthreads();
  for (int e = tid; e < 1250; e += 256)
    *reinterpret_cast<float4 *>(p.out + (size_t)img * 5000 + 4 * e) = *reinterpret_cast<const float4 *>(outs + 4 * e);
  }  // work items
}

// ---- fp32 MFMA GEMM for the dense layers -------------------------------------------
// C[M][N] = act(A[M][K] (lda) x B[K][N] (ldb) + bias[N])   one wave per 32x32 tile,
// v_mfma_f32_32x32x2_f32: lane l holds A[row l&31][k l>>5], B[k l>>5][col l&31];
// C/D: col = l&31, row = (reg&3) + 8*(reg>>2) + 4*(l>>5).

// `live` (may be null): ordered list of the rows to compute, live[0] = count, live[1 + i] = row (a masked forward:
// the i-th selected ship) - the M-tiles run over the list, A is read and C written at the listed rows
__global__ __launch_bounds__(256) void k_gemm_f32(const float *A, int lda, const float *B, int ldb, const float *bias,
                                                  float *C, int ldc, int M, int N, int K, int relu, const int32_t *live) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int tiles_n = (N + 31) / 32;
  const int tile = blockIdx.x * 4 + wv;
  if (live) M = live[0];
  if (tile >= ((M + 31) / 32) * tiles_n) return;
  const int m0 = (tile / tiles_n) * 32, n0 = (tile % tiles_n) * 32;
  const int r0 = m0 + (lane & 31), c = n0 + (lane & 31), kh = lane >> 5;
  const bool rv = r0 < M, cv = c < N;
  const int r = live ? live[1 + (rv ? r0 : 0)] : r0;
  f32x16 acc;
#pragma unroll
  for (int i = 0; i < 16; i++) acc[i] = 0.f;
  const float *ap = A + (size_t)(rv ? r : 0) * lda + kh;
  const float *bp = B + (size_t)kh * ldb + (cv ? c : 0);
  for (int k0 = 0; k0 < K; k0 += 2) {
    const bool kv = k0 + kh < K;
    const float a = (rv && kv) ? ap[k0] : 0.f;
    const float b = (cv && kv) ? bp[(size_t)k0 * ldb] : 0.f;
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, acc, 0, 0, 0);
  }
  if (cv) {
    const float bv = bias ? bias[c] : 0.f;
#pragma unroll
    for (int i = 0; i < 16; i++) {
      const int row = m0 + (i & 3) + 8 * (i >> 2) + 4 * kh;
      if (row < M) {
        float v = acc[i] + bv;
        if (relu) v = fmaxf(v, 0.f);
        C[(size_t)(live ? live[1 + row] : row) * ldc + c] = v;
      }
    }
  }
}

// The same GEMM for K = 100 (updense1 and dense2: A = d1 [.][100], 16-byte aligned rows): a workgroup = one N tile and
// four M tiles, one per wave.  The 100 x 32 weight tile is staged in LDS once, in the order lane (column, kh) walks it -
// B[2 t + kh][column], t = 0 .. 49, as 13 groups of four t: one 16-byte LDS read per four MFMAs - and an A row arrives as
// 25 16-byte loads in three batches: float4 u of the row holds the lane's operand of MFMA 2 u (.x | .y by kh) and of
// MFMA 2 u + 1 (.z | .w).  MFMA t still multiplies k = 2 t, 2 t + 1: every output keeps k_gemm_f32's k order, bit for
// bit.  Rows / columns outside the matrix compute on clamped addresses and are not stored.
__global__ __launch_bounds__(256) void k_gemm_f32_k100(const float *A, int lda, const float *B, int ldb, const float *bias,
                                                       float *C, int ldc, int M, int N, int relu, const int32_t *live,
                                                       int tiles_n) {
  constexpr int K = 100, NT = K / 2, NQ = (NT + 3) / 4;   // 50 MFMAs, 13 groups of four
  __shared__ __align__(16) float bs[NQ * 2 * 32 * 4];
  const int tid = threadIdx.x, lane = tid & 63, wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int nt = blockIdx.x % tiles_n, mg = blockIdx.x / tiles_n;
  if (live) M = live[0];
  if (mg * 128 >= M) return;  // block-uniform (a masked launch is sized for every ship)
  const int m0 = (mg * 4 + wv) * 32, n0 = nt * 32;
  const int r0 = m0 + (lane & 31), c = n0 + (lane & 31), kh = lane >> 5;
  const bool rv = r0 < M, cv = c < N;
  {  // thread (column tid & 31, (group, kh) = tid >> 5 + 8 i): its four rows -> one float4
    const float *bp = B + (n0 + (tid & 31) < N ? n0 + (tid & 31) : 0);
    f32x4 w[(2 * NQ + 7) / 8];
#pragma unroll
    for (int i = 0; i < (2 * NQ + 7) / 8; i++) {
      const int gk = min((tid >> 5) + 8 * i, 2 * NQ - 1), q = gk >> 1, h = gk & 1;
#pragma unroll
      for (int j = 0; j < 4; j++) w[i][j] = bp[(size_t)(2 * min(4 * q + j, NT - 1) + h) * ldb];
    }
#pragma unroll
    for (int i = 0; i < (2 * NQ + 7) / 8; i++) {
      const int gk = (tid >> 5) + 8 * i;
      if (gk < 2 * NQ) *reinterpret_cast<f32x4 *>(bs + (gk * 32 + (tid & 31)) * 4) = w[i];
    }
  }
  const int r = live ? live[1 + (rv ? r0 : 0)] : (rv ? r0 : 0);
  const float *ap = A + (size_t)r * lda;
  constexpr int NU = K / 4, NB0 = 9, NB1 = 8;   // batches of the row's 25 float4: 9, 8, 8
  f32x4 a[NU];
#pragma unroll
  for (int u = 0; u < NB0; u++) a[u] = *reinterpret_cast<const f32x4 *>(ap + 4 * u);
  __syncthreads();
  if (m0 >= M) return;  // wave-uniform; behind the workgroup's only barrier
  f32x16 acc;
#pragma unroll
  for (int i = 0; i < 16; i++) acc[i] = 0.f;
  const float *bl = bs + (kh * 32 + (lane & 31)) * 4;
  f32x4 b4[NQ];
#pragma unroll
  for (int u = 0; u < NU; u++) {  // float4 u of the row: MFMAs t = 2 u, 2 u + 1
    if (u == 0) {
#pragma unroll
      for (int i = NB0; i < NB0 + NB1; i++) a[i] = *reinterpret_cast<const f32x4 *>(ap + 4 * i);
    }
    if (u == NB0) {
#pragma unroll
      for (int i = NB0 + NB1; i < NU; i++) a[i] = *reinterpret_cast<const f32x4 *>(ap + 4 * i);
    }
    if ((u & 1) == 0) b4[u >> 1] = *reinterpret_cast<const f32x4 *>(bl + (u >> 1) * 2 * 32 * 4);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(kh ? a[u][1] : a[u][0], b4[u >> 1][(2 * u) & 3], acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(kh ? a[u][3] : a[u][2], b4[u >> 1][(2 * u + 1) & 3], acc, 0, 0, 0);
  }
  if (cv) {
    const float bv = bias ? bias[c] : 0.f;
#pragma unroll
    for (int i = 0; i < 16; i++) {
      const int row = m0 + (i & 3) + 8 * (i >> 2) + 4 * kh;
      if (row < M) {
        float v = acc[i] + bv;
        if (relu) v = fmaxf(v, 0.f);
        C[(size_t)(live ? live[1 + row] : row) * ldc + c] = v;
      }
    }
  }
}

// Split-K form for the tall-K dense1 (M = arenas, N = 100, K = 5000): one wave per (32x32 tile, K chunk of 200), partial
// sums P[chunk][M][N] reduced in a fixed order by the consumer (k_head_dense) - no atomics, bit-reproducible.
// K is walked 8 at a time with the k-slots permuted (slot kh of step j <-> k = k0 + 4 kh + j) so that a lane
// fetches its A operands with one 16-byte load per 4 MFMAs; Kc % 8 == 0, lda % 4 == 0, A 16-byte aligned.
//
// A workgroup = one (K chunk, N tile) and four M tiles, one per wave: the chunk's 200 x 32 weight tile is staged in LDS
// once ([k / 4][column][k % 4]: the four B operands of a k-step are one 16-byte LDS read) instead of being fetched by
// every lane with four scalar-indexed global loads per k-step, and the A rows arrive in three batches of 16-byte loads,
// a batch in flight while the one before feeds the MFMAs.  A lane's operands of a row (column) outside the matrix
// are whatever the clamped address holds: an MFMA row (column) depends on its own operands only and those outputs are
// not stored.  Blocks that follow each other share their four A tiles (the N tile runs fastest).
constexpr int kSplitKc = 200;
__global__ __launch_bounds__(256) void k_gemm_f32_splitk(const float *A, int lda, const float *B, int ldb, float *P,
                                                         int M, int N, int tiles_n, int groups_m) {
  constexpr int Kc = kSplitKc, KG = Kc / 4, STEPS = Kc / 8;   // 50 k-groups of 4, 25 k-steps of 8
  __shared__ __align__(16) float bs[KG * 32 * 4];
  const int tid = threadIdx.x, lane = tid & 63, wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int nt = blockIdx.x % tiles_n, rest = blockIdx.x / tiles_n, mg = rest % groups_m, chunk = rest / groups_m;
  const int m0 = (mg * 4 + wv) * 32, n0 = nt * 32;
  const int r = m0 + (lane & 31), c = n0 + (lane & 31), kh = lane >> 5;
  const bool rv = r < M, cv = c < N;
  {  // the weight tile: thread (column tid & 31, k-group tid >> 5 + 8 i) loads its four rows and stores them as one float4
    const float *bp = B + (size_t)chunk * Kc * ldb + (n0 + (tid & 31) < N ? n0 + (tid & 31) : 0);
    f32x4 w[(KG + 7) / 8];
#pragma unroll
    for (int i = 0; i < (KG + 7) / 8; i++) {
      const int g = min((tid >> 5) + 8 * i, KG - 1);
#pragma unroll
      for (int j = 0; j < 4; j++) w[i][j] = bp[(size_t)(4 * g + j) * ldb];
    }
#pragma unroll
    for (int i = 0; i < (KG + 7) / 8; i++) {
      const int g = (tid >> 5) + 8 * i;
      if (g < KG) *reinterpret_cast<f32x4 *>(bs + (g * 32 + (tid & 31)) * 4) = w[i];
    }
  }
  const float *ap = A + (size_t)(rv ? r : 0) * lda + (size_t)chunk * Kc + 4 * kh;
  constexpr int NB0 = 9, NB1 = 8;   // batches of the 25 k-steps: 9, 8, 8
  f32x4 a[STEPS];
#pragma unroll
  for (int i = 0; i < NB0; i++) a[i] = *reinterpret_cast<const f32x4 *>(ap + 8 * i);
  __syncthreads();
  if (m0 >= M) return;  // wave-uniform; behind the workgroup's only barrier
  f32x16 acc;
#pragma unroll
  for (int i = 0; i < 16; i++) acc[i] = 0.f;
  const float *bl = bs + (kh * 32 + (lane & 31)) * 4;
#pragma unroll
  for (int s = 0; s < STEPS; s++) {  // k-step s: k = 8 s + 4 kh + j in MFMA j
    if (s == 0) {
#pragma unroll
      for (int i = NB0; i < NB0 + NB1; i++) a[i] = *reinterpret_cast<const f32x4 *>(ap + 8 * i);
    }
    if (s == NB0) {
#pragma unroll
      for (int i = NB0 + NB1; i < STEPS; i++) a[i] = *reinterpret_cast<const f32x4 *>(ap + 8 * i);
    }
    const f32x4 b4 = *reinterpret_cast<const f32x4 *>(bl + s * 2 * 32 * 4);
#pragma unroll
    for (int j = 0; j < 4; j++) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[s][j], b4[j], acc, 0, 0, 0);
  }
  if (cv) {
    float *out = P + (size_t)chunk * M * N;
#pragma unroll
    for (int i = 0; i < 16; i++) {
      const int row = m0 + (i & 3) + 8 * (i >> 2) + 4 * kh;
      if (row < M) out[(size_t)row * N + c] = acc[i];
    }
  }
}

// ---- per-ship dense1 finish + head-1 ---------------------------------------------
// d1 = relu(G1[arena] + vec8 . K1[0:8] + b1) ; d2 = relu(d1 K2 + b2) ; act = d2 K3 + b3
struct HeadParams {
  int N, M;
  ofx_state st;
  const float *g1;            // [g1_chunks][N][100]  trunk part of dense1 (no bias), split-K partial sums
  int g1_chunks;
  const float *k1, *b1, *k2, *b2, *k3, *b3;
  const int32_t *live;   // ordered list of the selected ships (with a mask) or null
  const uint8_t *mask;
  const float *vec8;          // [S][8] explicit observation heads (ofx_policy_forward_obs) or null = the live state
  float *d1;                  // [S][100]
  float *act;                 // [S][2] or null
  int32_t *iaction;           // [S] or null
};

__global__ __launch_bounds__(256) void k_head_dense(HeadParams p) {
  __shared__ float sd1[4][100];
  __shared__ float sd2[4][50];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  // with a mask: work item i = the i-th selected ship (p.live: count, then the ordered list); the blocks behind the
  // count leave at once
  const int item = blockIdx.x * 4 + wv, n_items = p.live ? p.live[0] : p.N * p.M;
  if ((int)blockIdx.x * 4 >= n_items) return;  // block-uniform
  const bool on = item < n_items;
  const int s = on ? (p.live ? p.live[1 + item] : item) : 0;
  const int a = s / p.M;
  float vec[8];
  if (on) {  // obs.vector[:8] (observation.py:119-123): reward, can_shoot, pointing, dim, pos
    if (p.vec8) {
#pragma unroll
      for (int k = 0; k < 8; k++) vec[k] = p.vec8[(size_t)s * 8 + k];
    } else {
      ofx_obs_head(p.st, s, PS, PS, vec);
    }
    for (int o = lane; o < 100; o += 64) {
      float acc = 0.f;
#pragma unroll
      for (int k = 0; k < 8; k++) acc += vec[k] * p.k1[k * 100 + o];
      float g = 0.f;
      for (int ch = 0; ch < p.g1_chunks; ch++) g += p.g1[((size_t)ch * p.N + a) * 100 + o];  // fixed order
      acc += g;
      acc += p.b1[o];
      acc = fmaxf(acc, 0.f);
      sd1[wv][o] = acc;
      p.d1[(size_t)s * 100 + o] = acc;
    }
  }
  __syncthreads();
  if (on && lane < 50) {
    float acc = 0.f;
    for (int k = 0; k < 100; k++) acc += sd1[wv][k] * p.k2[k * 50 + lane];
    sd2[wv][lane] = fmaxf(acc + p.b2[lane], 0.f);
  }
  __syncthreads();
  if (on && lane < 2) {
    float acc = 0.f;
    for (int k = 0; k < 50; k++) acc += sd2[wv][k] * p.k3[k * 2 + lane];
    acc += p.b3[lane];
    if (p.act) p.act[(size_t)s * 2 + lane] = acc;
    const float other = __shfl_xor(acc, 1);
    if (lane == 0 && p.iaction) p.iaction[s] = other > acc ? 1 : 0;  // np.argmax: first maximum
  }
}

__device__ inline float unordered_f32(unsigned o) {  // inverse of ordered_f32
  return __uint_as_float((o & 0x80000000u) ? (o & 0x7FFFFFFFu) : ~o);
}

__global__ void k_policy_finish(int S, const uint8_t *mask, const unsigned long long *best, int32_t *ipointer,
                                float *ptr_max) {
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= S || (mask && !mask[s])) return;
  // best == 0: no value ever beat the initial -inf, i.e. the whole map is NaN (a diverged fit) or -inf: np.argmax
  // answers 0 there (the first NaN / the first element) and np.max NaN / -inf; never an out-of-range pointer
  const bool none = best[s] == 0ull;
  const unsigned k = none ? 0u : ~(unsigned)(best[s] & 0xFFFFFFFFull);
  ipointer[2 * s] = (int)(k % PS);      // unravel_index(order='F') of a C-order flat index = (x, y)
  ipointer[2 * s + 1] = (int)(k / PS);  // qlearnIA_V2.py:218-220
  if (ptr_max) ptr_max[s] = none ? __builtin_nanf("") : unordered_f32((unsigned)(best[s] >> 32));  // np.max(ptr_prediction)
}

// Behind k_head_stream_soft (ofx_policy_forward_obs_soft): the ship's 8 per-wave pairs (m, z) merged in slot order against
// the ship's maximum M - the float of the `best` key, so the bits of ptr_max - into Z = sum z_c exp((m_c - M) / T) and
// the soft value M + T ln Z (one fmaf: the same bits under either contraction setting).  k = log2(e) / T; k == 0 is
// the call at T == 0, where the default kernel ran: the soft value is the maximum, the mass 1.  No finite value
// (key == 0): NaN, as ptr_max.
__global__ void k_policy_soft_finish(int S, const unsigned long long *best, const float *soft_m, const float *soft_z,
                                     float T, float k, float *ptr_soft, float *ptr_mass) {
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= S) return;
  const bool none = best[s] == 0ull;
  const float M = none ? __builtin_nanf("") : unordered_f32((unsigned)(best[s] >> 32));
  float Z = 1.f, V = M;
  if (k != 0.f) {
    Z = 0.f;
    for (int c = 0; c < 8; c++) Z += hd_soft_term(soft_m[(size_t)s * 8 + c], soft_z[(size_t)s * 8 + c], M, k);
    if (none) Z = __builtin_nanf("");
    V = fmaf(T, logf(Z), M);
  }
  if (ptr_soft) ptr_soft[s] = V;
  if (ptr_mass) ptr_mass[s] = Z;
}

// QlearnIA.play packing (qlearnIA_V2.py:447-454): exactly one of shoot / thrust, pointer always set
__global__ void k_policy_actions(int S, const ofx_state st, const int32_t *iaction, const int32_t *ipointer,
                                 const uint8_t *mask, ofx_action *out) {
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= S || (mask && !mask[s])) return;
  ofx_action a;
  a.valid = st.alive[s] ? 1 : 0;  // a dead ship's action is None (ship.py:260-262)
  a.shoot = iaction[s] == 0;
  a.thrust = iaction[s] == 1;
  a.px = ipointer[2 * s];
  a.py = ipointer[2 * s + 1];
  a._pad = 0;
  out[s] = a;
}

// The exploration rate of local arena a under the ladder (`expo` null = none): epsilon itself at exponent 1 (no pow),
// pow(epsilon, exponent) in float64 otherwise (pow(x, 0) = 1: exponent 0 always explores); *greedy at +inf.
__device__ __forceinline__ double arena_eps(double eps, const double *expo, int a, bool *greedy) {
  *greedy = false;
  if (expo) {
    const double x = expo[a];
    if (x == (double)INFINITY) { *greedy = true; return 0.0; }
    if (x != 1.0) eps = pow(eps, x);
  }
  return eps;
}

// ---- Boltzmann exploration (ofx_policy_act_boltzmann) ----------------------------------------------------------
// what the forward needs to sample instead of taking the arg-max
struct BoltzArgs {
  double eps;
  float tau_act, tau_ptr;
  ofx_rng_key key;
  uint32_t tick;
  float *q_sa, *p_sp, *v_act, *v_ptr;
};

// per ship: the temperatures of its arena, T = tau * (float)eps_a in float32 (a greedy arena: 0)
__global__ void k_boltz_temps(int N, int M, double eps, const double *expo, float tau_act, float tau_ptr, float *t_act,
                              float *t_ptr) {
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= N * M) return;
  bool greedy;
  const float e = (float)arena_eps(eps, expo, s / M, &greedy);
  t_act[s] = tau_act * e;
  t_ptr[s] = tau_ptr * e;
}

// Behind k_head_stream_sample: the ship's winner among its 8 waves' candidates (the largest key: the largest perturbed
// value, the first pixel in C order among equals), the raw heat value there and the raw maximum; the action head
// sampled the same way from two Gumbel words of its own stream.
__global__ void k_policy_boltz_finish(int S, int M, int arena_base, const uint8_t *mask, const unsigned long long *cand_key,
                                      const float *cand_raw, const unsigned *cand_max, const float *act, const float *t_act,
                                      ofx_rng_key noise_key, uint32_t tick, int32_t *iaction, int32_t *ipointer,
                                      float *q_sa, float *p_sp, float *v_act, float *v_ptr) {
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= S || (mask && !mask[s])) return;
  unsigned long long key = 0ull;
  float raw = __builtin_nanf("");
  unsigned om = 0u;
  for (int c = 0; c < 8; c++) {
    const unsigned long long k = cand_key[(size_t)s * 8 + c];
    if (k > key) { key = k; raw = cand_raw[(size_t)s * 8 + c]; }
    om = max(om, cand_max[(size_t)s * 8 + c]);
  }
  // key == 0: no value ever beat -inf (a NaN or -inf map), as in k_policy_finish: pointer 0, NaN values
  const unsigned idx = key ? ~(unsigned)(key & 0xFFFFFFFFull) : 0u;
  ipointer[2 * s] = (int)(idx % PS);
  ipointer[2 * s + 1] = (int)(idx / PS);
  p_sp[s] = raw;
  v_ptr[s] = key ? unordered_f32(om) : __builtin_nanf("");
  const int a = s / M, i = s - a * M;
  const float a0 = act[2 * s], a1 = act[2 * s + 1], T = t_act[s];
  int ia = a1 > a0 ? 1 : 0;   // np.argmax: first maximum
  if (T != 0.f) {
    uint32_t r[4];
    ofx_philox4x32_10((uint32_t)(arena_base + a), (uint32_t)i, tick, OFX_STREAM_BOLTZMANN_ACT, noise_key, r);
    ia = fmaf(T, hd_gumbel(r[1]), a1) > fmaf(T, hd_gumbel(r[0]), a0) ? 1 : 0;
  }
  iaction[s] = ia;
  q_sa[s] = ia ? a1 : a0;
  v_act[s] = fmaxf(a0, a1);
}

// ---- workspace -----------------------------------------------------------------------
struct PolicyWs {
  float *p1, *p2, *p3, *p4, *g1, *d1, *u0, *up1, *u2fr, *vfr, *c4;
  unsigned *nz2;            // streaming trunk only: the p2 marks k_trunk12 leaves for k_conv3_stream, 1.6 KB per image ...
  float *k2;                // ... and conv2's constant [8]; no bytes in the per-layer form
  unsigned long long *best;
  int32_t *iaction, *ipointer, *live;
  // sampling forwards only: per-ship temperatures, per-wave candidates of k_head_stream_sample.  Otherwise the five have no
  // bytes (they point at the block's end) and no kernel gets them; so p1, which points at p2, in the fused form of the trunk.
  float *t_act, *t_ptr, *cand_raw;
  unsigned long long *cand_key;
  unsigned *cand_max;
  float *soft_m, *soft_z;   // soft forwards only: per-wave (maximum, sum) of k_head_stream_soft; no bytes otherwise
};

constexpr int kDense1Chunks = 25;  // split-K of dense1: 5000 = 25 x 200

// N images (trunk runs), S policy samples (heads).  Everything here is transient: a later forward with other sizes or
// any other user of the handle's scratch block may overwrite or re-allocate it.  The (iaction, ipointer) slots only
// take results nobody asked for (ofx_policy_forward_obs with null outputs); the results that ofx_policy_forward keeps
// for ofx_policy_explore / ofx_policy_actions / ofx_replay_capture live in the handle (ofx_policy_results).
static void policy_layout_ws(Arena &A, bool fused, size_t N, size_t S, bool sample, bool soft, PolicyWs &W) {
  size_t f2, f3, f4;
  ofx_head_frame_bytes(S, &f2, &f3, &f4);
  W.p1 = A.f(fused ? 0 : N * 8 * 200 * 200);   // (5.2 GB at 4096 arenas) only in the two-kernel form of the trunk
  W.p2 = A.f(N * 8 * 100 * 100); W.p3 = A.f(N * 8 * 50 * 50); W.p4 = A.f(N * 5000); W.g1 = A.f(N * 100 * kDense1Chunks);
  W.d1 = A.f(S * 100); W.u0 = A.f(S * 625); W.up1 = A.f(S * 2 * 50 * 50);
  W.u2fr = (float *)A.take(f2); W.vfr = (float *)A.take(f3); W.c4 = (float *)A.take(f4);
  W.nz2 = A.n<unsigned>(fused ? N * 100 * 4 : 0); W.k2 = A.f(fused ? 8 : 0);
  W.best = A.n<unsigned long long>(S); W.iaction = A.n<int32_t>(S); W.ipointer = A.n<int32_t>(2 * S); W.live = A.n<int32_t>(S + 1);
  // the sampling forward's arrays stand behind everything else: the other forwards' layout is unchanged
  const size_t Q = sample ? S : 0;
  W.t_act = A.f(Q); W.t_ptr = A.f(Q); W.cand_raw = A.f(8 * Q); W.cand_key = A.n<unsigned long long>(8 * Q); W.cand_max = A.n<unsigned>(8 * Q);
  // and the soft forward's behind those
  const size_t Qs = soft ? S : 0;
  W.soft_m = A.f(8 * Qs); W.soft_z = A.f(8 * Qs);
}
static int policy_workspace(ofx_handle *h, PolicyWs *ws, size_t N, size_t S, bool sample = false, bool soft = false) {
  const bool fused = ofx_trunk_fused(h, N);
  Arena measure;
  policy_layout_ws(measure, fused, N, S, sample, soft, *ws);
  const int rc = ofx_ensure_scratch(h, measure.used);
  if (rc) return rc;
  Arena A(h->scratch, measure.used);
  policy_layout_ws(A, fused, N, S, sample, soft, *ws);
  if (!A.ok()) { ofx_set_error("policy forward: internal workspace sized too small"); return OFX_ERR_STATE; }
  return OFX_OK;
}

const float *ofx_policy_ws_p4(ofx_handle *h, size_t N, size_t S) {  // ofx_trunk.h
  PolicyWs ws;
  Arena measure;
  policy_layout_ws(measure, ofx_trunk_fused(h, N), N, S, false, false, ws);
  if (!h->scratch || h->scratch_bytes < measure.used) return nullptr;
  Arena A(h->scratch, measure.used);
  policy_layout_ws(A, ofx_trunk_fused(h, N), N, S, false, false, ws);
  return A.ok() ? ws.p4 : nullptr;
}

// (also the dense layers of the fit's forward, ofx_train.hip)
int ofx_launch_gemm(ofx_handle *h, const float *A, int lda, const float *B, int ldb, const float *bias, float *C, int ldc,
                    int M, int N, int K, int relu, const int32_t *live) {
  const int tiles_m = (M + 31) / 32, tiles_n = (N + 31) / 32, tiles = tiles_m * tiles_n;
  if (K == 100 && lda % 4 == 0 && ((uintptr_t)A & 15) == 0)  // the layers behind d1: the same sums, operands through LDS
    hipLaunchKernelGGL(k_gemm_f32_k100, dim3((unsigned)(((tiles_m + 3) / 4) * tiles_n)), dim3(256), 0, h->stream, A, lda, B, ldb,
                       bias, C, ldc, M, N, relu, live, tiles_n);
  else
    hipLaunchKernelGGL(k_gemm_f32, dim3((tiles + 3) / 4), dim3(256), 0, h->stream, A, lda, B, ldb, bias, C, ldc, M, N, K,
                       relu, live);
  OFX_HIP(hipGetLastError());
  return OFX_OK;
}

// BN folding, phase weights, tables: `weights` -> the handle's prepared-weights buffer (two small launches)
// `slot`: &h->prep (the pinned blob's buffer) or &h->prep_tmp (any other blob: a target network or a one-off forward
// next to a pinned blob must not overwrite the pinned blob's prepared weights)
static int policy_prepare(ofx_handle *h, const float *weights, float **slot) {
  const PrepLayout L = prep_layout();
  if (!*slot) {
    OFX_HIP(hipMalloc((void **)slot, sizeof(float) * L.total));
    OFX_HIP(hipMemsetAsync(*slot, 0, sizeof(float) * L.total, h->stream));
  }
  int32_t off[64], cnt[64];
  policy_layout(off, cnt);
  PrepParams pp;
  pp.w = weights; pp.prep = *slot;
  for (int i = 0; i < 4; i++) {
    pp.src_k[i] = off[ofx_t_trunk(i)]; pp.src_b[i] = off[ofx_t_trunk(i, OFX_T_BIAS)]; pp.src_g[i] = off[ofx_t_trunk(i, OFX_T_GAMMA)];
    pp.cin[i] = kTrunkCin[i]; pp.cout[i] = 8; pp.dst_w[i] = L.tw[i]; pp.dst_b[i] = L.tb[i];
  }
  for (int i = 0; i < 3; i++) {
    pp.src_k[4 + i] = off[ofx_t_up(i)]; pp.src_b[4 + i] = off[ofx_t_up(i, OFX_T_BIAS)]; pp.src_g[4 + i] = off[ofx_t_up(i, OFX_T_GAMMA)];
    pp.cin[4 + i] = kUpCin[i]; pp.cout[4 + i] = kUpCout[i]; pp.dst_w[4 + i] = L.uw[i]; pp.dst_b[4 + i] = L.ub[i];
  }
  pp.src_k4 = off[OFX_T_OUT2]; pp.src_b4 = off[OFX_T_OUT2 + 1];
  pp.dst_w4raw = L.w4raw; pp.dst_b4 = L.b4; pp.dst_efr = L.efr;
  pp.dst_w4eff_c = L.w4eff_c; pp.dst_w3mf = L.w3mf; pp.dst_w2mf = L.w2mf; pp.dst_w2fr = L.w2fr; pp.dst_w3fr = L.w3fr; pp.dst_lut1 = L.lut1;
  for (int i = 0; i < 3; i++) pp.dst_wbm[i] = L.wbm[i];
  pp.legacy = h->opt_bilinear_legacy;
  pp.phase = 0;
  hipLaunchKernelGGL(k_policy_prepare, dim3(32), dim3(256), 0, h->stream, pp);
  pp.phase = 1;
  hipLaunchKernelGGL(k_policy_prepare, dim3(4), dim3(256), 0, h->stream, pp);
  OFX_HIP(hipGetLastError());
  return OFX_OK;
}

// Pinned weights: prepared once, reused by every forward that names the same blob until it is unpinned, re-pinned or
// trained on (ofx_dqn_fit re-prepares a pinned blob behind its update).
extern "C" int ofx_policy_pin_weights(ofx_handle *h, const float *weights) {
  if (!h) { ofx_set_error("ofx_policy_pin_weights: null handle"); return OFX_ERR_INVALID; }
  OFX_HIP(hipSetDevice(h->cfg.device));
  h->prep_pinned = nullptr;
  if (!weights) return OFX_OK;
  int rc = policy_prepare(h, weights, &h->prep);
  if (rc) return rc;
  h->prep_pinned = weights;
  return OFX_OK;
}

int ofx_policy_weights_updated(ofx_handle *h, const float *weights) {  // ofx_train.hip: the blob changed in place
  if (h->prep_pinned && h->prep_pinned == weights) return policy_prepare(h, weights, &h->prep);
  return OFX_OK;
}

extern "C" int ofx_set_option(ofx_handle *h, int32_t option, int32_t value) {
  if (!h) { ofx_set_error("ofx_set_option: null handle"); return OFX_ERR_INVALID; }
  switch (option) {
    case OFX_OPT_TRUNK_PLAIN: h->opt_trunk_plain = value != 0; return OFX_OK;
    case OFX_OPT_TRUNK_FUSE:
      if (value < 0 || value > 2) { ofx_set_error("ofx_set_option: OFX_OPT_TRUNK_FUSE takes 0 (auto), 1 (always), 2 (never)"); return OFX_ERR_INVALID; }
      h->opt_trunk_fuse = value; return OFX_OK;
    case OFX_OPT_FRAMES_REF: h->opt_frames_ref = value != 0; return OFX_OK;
    case OFX_OPT_TRUNK_SPARSE:
      if (value && !h->trunk_stat) {
        OFX_HIP(hipSetDevice(h->cfg.device));
        OFX_HIP(hipMalloc((void **)&h->trunk_stat, 6 * sizeof(unsigned long long)));
        OFX_HIP(hipMemsetAsync(h->trunk_stat, 0, 6 * sizeof(unsigned long long), h->stream));
      }
      h->opt_trunk_dense = value == 0; h->opt_trunk_count = value != 0; return OFX_OK;
    case OFX_OPT_FIT_PLAIN: h->opt_fit_plain = value != 0; return OFX_OK;
    case OFX_OPT_POLICY_BF16:
      if (value < 0 || value > 2) { ofx_set_error("ofx_set_option: OFX_OPT_POLICY_BF16 takes 0 (fp32), 1 (bf16 operands), 2 (fp16 operands)"); return OFX_ERR_INVALID; }
      h->opt_policy_lowp = value; return OFX_OK;
    case OFX_OPT_BILINEAR_LEGACY:  // a different function, not a variant: the prepared phase weights depend on it
      if (h->opt_bilinear_legacy == (value != 0)) return OFX_OK;
      h->opt_bilinear_legacy = value != 0;
      OFX_HIP(hipSetDevice(h->cfg.device));
      return h->prep_pinned ? policy_prepare(h, h->prep_pinned, &h->prep) : OFX_OK;
    default: ofx_set_error("ofx_set_option: unknown option %d", option); return OFX_ERR_INVALID;
  }
}

// One forward: N images (two 1-bit maps each: word bits[ci][img * bits_stride + w]) with M policy samples per image.
struct ForwardArgs {
  const float *weights;
  int N, M;
  const unsigned *bits[2];
  size_t bits_stride;
  const float *vec8;               // explicit observation heads [N*M][8] or null (the live state of the handle's arenas)
  const uint8_t *ship_mask;        // [N*M] or null
  // results as in include/ofx.h, each may be null; null iaction / ipointer go to a throw-away slot of the workspace
  float *act_values, *heatmap, *ptr_max, *ptr_probe;
  int32_t *iaction, *ipointer;
  const int32_t *probe;
  const BoltzArgs *boltz;          // non-null: sample both heads (k_head_stream_sample + k_policy_boltz_finish); needs act_values
  // ofx_policy_forward_obs_soft: soft != 0 asks for ptr_soft / ptr_mass [N*M] (either may be null) at temperature tau_ptr;
  // tau_ptr == 0 runs the default kernel (k_policy_soft_finish copies the maximum)
  int soft;
  float tau_ptr;
  float *ptr_soft, *ptr_mass;
};

static int policy_forward_impl(ofx_handle *h, const ForwardArgs &a) {
  const int N = a.N, S = a.N * a.M;
  const float *weights = a.weights;
  PolicyWs ws;
  // k_head_stream_soft takes the place of k_head_stream - when an output asks for its sums
  const bool soft = a.soft && a.tau_ptr != 0.f && (a.ptr_soft || a.ptr_mass);
  if (a.soft && (a.boltz || a.ship_mask)) { ofx_set_error("policy forward: the soft form takes no mask and no sampling"); return OFX_ERR_STATE; }
  int rc = policy_workspace(h, &ws, N, S, a.boltz != nullptr, soft);
  if (rc) return rc;
  int32_t off[64], cnt[64];
  policy_layout(off, cnt);
  const PrepLayout L = prep_layout();

  // 0. prepared weights: reused when the blob is pinned
  //    (h->prep holds exactly the pinned blob's preparation; every other blob goes through h->prep_tmp)
  const bool pinned = h->prep && h->prep_pinned == weights;
  if (!pinned && (rc = policy_prepare(h, weights, &h->prep_tmp))) return rc;
  const float *prep = pinned ? h->prep : h->prep_tmp;

  // 1. trunk, once per arena (ofx_trunk.hip)
  const int lowp = a.vec8 == nullptr ? h->opt_policy_lowp : 0;  // opt-in (1 bf16, 2 fp16 operands), the rollout's forward only
  TrunkParams tp;
  memset(&tp, 0, sizeof(tp));
  tp.bits[0] = a.bits[0]; tp.bits[1] = a.bits[1]; tp.bits_stride = a.bits_stride; tp.images = N;
  for (int i = 0; i < 4; i++) { tp.tw[i] = prep + L.tw[i]; tp.tb[i] = prep + L.tb[i]; }
  for (int i = 0; i < 3; i++) tp.wbm[i] = prep + L.wbm[i];
  tp.lut1 = prep + L.lut1; tp.zero16 = prep + L.zero16;
  tp.p1 = ws.p1; tp.p2 = ws.p2; tp.p3 = ws.p3; tp.p4 = ws.p4; tp.nz2 = ws.nz2; tp.k2 = ws.k2;
  // the sparse kernel is exact, so it is the default; OFX_OPT_TRUNK_SPARSE = 0 asks for the dense one (live forward only:
  // the forwards on stored observations, i.e. the DQN targets, always take the sparse one), = 1 for the counters
  tp.lowp = lowp; tp.sparse = !h->opt_trunk_dense || a.vec8 != nullptr;
  tp.stat = h->opt_trunk_count ? h->trunk_stat : nullptr;
  if ((rc = ofx_launch_trunk(h, tp))) return rc;

  // 2. dense1: trunk features on MFMA once per arena; head + head-1 per ship
  const float *k1 = weights + off[OFX_T_DENSE1];
  {
    static_assert(5000 == kDense1Chunks * kSplitKc, "k_gemm_f32_splitk's chunk");
    const int tiles_n = (100 + 31) / 32, groups_m = ((N + 31) / 32 + 3) / 4;
    hipLaunchKernelGGL(k_gemm_f32_splitk, dim3((unsigned)(tiles_n * groups_m * kDense1Chunks)), dim3(256), 0, h->stream, ws.p4,
                       5000, k1 + 8 * 100, 100, ws.g1, N, 100, tiles_n, groups_m);
    OFX_HIP(hipGetLastError());
  }
  HeadParams hp;
  hp.N = N; hp.M = a.M; hp.st = h->st; hp.vec8 = a.vec8; hp.g1 = ws.g1; hp.g1_chunks = kDense1Chunks;
  hp.k1 = k1; hp.b1 = weights + off[OFX_T_DENSE1 + 1];
  hp.k2 = weights + off[OFX_T_DENSE2]; hp.b2 = weights + off[OFX_T_DENSE2 + 1];
  hp.k3 = weights + off[OFX_T_OUT1]; hp.b3 = weights + off[OFX_T_OUT1 + 1];
  // a masked forward works on the ordered list of the selected ships from here on (one scan of the mask)
  const int32_t *live = nullptr;
  if (a.ship_mask) {
    if ((rc = ofx_head_compact(h, S, a.ship_mask, ws.live))) return rc;
    live = ws.live;
  }
  hp.mask = a.ship_mask; hp.live = live; hp.d1 = ws.d1; hp.act = a.act_values; hp.iaction = a.iaction ? a.iaction : ws.iaction;
  hipLaunchKernelGGL(k_head_dense, dim3((S + 3) / 4), dim3(256), 0, h->stream, hp);
  OFX_HIP(hipGetLastError());

  // 3. head-2: updense1 on MFMA, upconv1 (1 -> 2 @ 50x50), then upconv2-4 + arg-max in the streaming kernel (ofx_head.hip)
  if ((rc = ofx_launch_gemm(h, ws.d1, 100, weights + off[OFX_T_UPDENSE], 625, weights + off[OFX_T_UPDENSE + 1], ws.u0, 625, S, 625, 100, 1, live)))
    return rc;
  ConvParams up;
  memset(&up, 0, sizeof(up));
  up.live = live; up.images = S; up.legacy = h->opt_bilinear_legacy;
  up.in = ws.u0; up.w = prep + L.uw[0]; up.b = prep + L.ub[0]; up.out = ws.up1;
  // every ship: one workgroup each (0.22 ms; a bounded grid that loops is 0.02 ms slower); with a mask: a bounded grid over the list
  if (up.legacy) hipLaunchKernelGGL(k_upconv1<true>, dim3((unsigned)(live && S > 4096 ? 4096 : S)), dim3(256), 0, h->stream, up);
  else hipLaunchKernelGGL(k_upconv1<false>, dim3((unsigned)(live && S > 4096 ? 4096 : S)), dim3(256), 0, h->stream, up);
  OFX_HIP(hipGetLastError());
  if (!a.boltz) OFX_HIP(hipMemsetAsync(ws.best, 0, sizeof(unsigned long long) * S, h->stream));
  HeadParams2 hp2;
  memset(&hp2, 0, sizeof(hp2));
  hp2.S = S; hp2.up1 = ws.up1;
  hp2.w2mf = prep + L.w2mf; hp2.b2 = prep + L.ub[1]; hp2.w2raw = prep + L.uw[1];
  hp2.w3mf = prep + L.w3mf; hp2.b3 = prep + L.ub[2]; hp2.w3raw = prep + L.uw[2];
  hp2.w4eff_c = prep + L.w4eff_c; hp2.b4 = prep + L.b4; hp2.w4raw = prep + L.w4raw;
  hp2.w2fr = prep + L.w2fr; hp2.w3fr = prep + L.w3fr; hp2.efr = prep + L.efr;
  hp2.u2fr = ws.u2fr; hp2.vfr = ws.vfr; hp2.c4 = ws.c4;
  hp2.frames_ref = h->opt_frames_ref; hp2.legacy = h->opt_bilinear_legacy;
  hp2.bf16 = lowp;  // the rollout's forward only: targets and fit stay fp32
  hp2.mask = a.ship_mask; hp2.live = ws.live; hp2.live_ready = a.ship_mask != nullptr; hp2.best = ws.best; hp2.heat = a.heatmap;
  hp2.probe = a.probe; hp2.ptr_probe = a.probe ? a.ptr_probe : nullptr;
  if (a.boltz) {
    const BoltzArgs &b = *a.boltz;
    hipLaunchKernelGGL(k_boltz_temps, dim3((S + 255) / 256), dim3(256), 0, h->stream, N, a.M, b.eps, h->eps_expo, b.tau_act,
                       b.tau_ptr, ws.t_act, ws.t_ptr);
    OFX_HIP(hipGetLastError());
    hp2.sample = 1; hp2.M = a.M; hp2.arena_base = h->cfg.arena_base;
    hp2.nk0 = b.key.k0; hp2.nk1 = b.key.k1; hp2.ntick = b.tick; hp2.t_ptr = ws.t_ptr;
    hp2.cand_key = ws.cand_key; hp2.cand_raw = ws.cand_raw; hp2.cand_max = ws.cand_max;
  }
  const float soft_k = soft ? (float)(1.4426950408889634 / (double)a.tau_ptr) : 0.f;   // log2(e) / T
  if (soft) { hp2.soft_k = soft_k; hp2.soft_m = ws.soft_m; hp2.soft_z = ws.soft_z; }
  const int pb = h->prof_base;  // ofx_policy_profile: events around the dominant kernel, until the ring is full
  hp2.event_base = pb;
  if ((rc = ofx_launch_head(h, hp2))) return rc;
  if (pb >= 0) h->prof_base = pb + 3 < OFX_RING_MAX ? pb + 2 : -1;
  if (a.boltz) {
    const BoltzArgs &b = *a.boltz;
    hipLaunchKernelGGL(k_policy_boltz_finish, dim3((S + 255) / 256), dim3(256), 0, h->stream, S, a.M, h->cfg.arena_base,
                       a.ship_mask, ws.cand_key, ws.cand_raw, ws.cand_max, a.act_values, ws.t_act, b.key, b.tick,
                       a.iaction ? a.iaction : ws.iaction, a.ipointer ? a.ipointer : ws.ipointer, b.q_sa, b.p_sp, b.v_act,
                       b.v_ptr);
    OFX_HIP(hipGetLastError());
    return OFX_OK;
  }
  hipLaunchKernelGGL(k_policy_finish, dim3((S + 255) / 256), dim3(256), 0, h->stream, S, a.ship_mask, ws.best,
                     a.ipointer ? a.ipointer : ws.ipointer, a.ptr_max);
  OFX_HIP(hipGetLastError());
  if (a.soft && (a.ptr_soft || a.ptr_mass)) {
    hipLaunchKernelGGL(k_policy_soft_finish, dim3((S + 255) / 256), dim3(256), 0, h->stream, S, ws.best, ws.soft_m, ws.soft_z,
                       a.tau_ptr, soft_k, a.ptr_soft, a.ptr_mass);
    OFX_HIP(hipGetLastError());
  }
  return OFX_OK;
}

// the argument checks of a forward on the live state, and the forward itself: `a` carries the results wanted, the
// weights and the mask; the images are the handle's arenas
static int live_forward_check(ofx_handle *h, const float *weights, const char *who) {
  if (!h || !weights) { ofx_set_error("%s: null argument", who); return OFX_ERR_INVALID; }
  if (!h->spawned) { ofx_set_error("You must execute analyse_battleground first."); return OFX_ERR_STATE; }
  const ofx_config &c = h->cfg;
  if (c.width != PS || c.height != PS) {
    // Input((DEFAULT_WIDTH, DEFAULT_HEIGHT, 2)) is fixed at 400x400 (qlearnIA_V2.py:125)
    ofx_set_error("%s: the pointer_model takes 400x400 maps (got %d x %d)", who, c.width, c.height);
    return OFX_ERR_INVALID;
  }
  return OFX_OK;
}

static int live_forward(ofx_handle *h, ForwardArgs &a) {
  const ofx_config &c = h->cfg;
  int rc = ofx_launch_raster(h, OFX_MAP_BITS_LSB, nullptr, nullptr);  // the observation as 1-bit maps
  if (rc) return rc;
  int32_t *ria, *rip;  // null = the handle's results
  if ((rc = ofx_policy_results(h, &ria, &rip))) return rc;
  if (!a.iaction) a.iaction = ria;
  if (!a.ipointer) a.ipointer = rip;
  a.N = c.n_arenas; a.M = c.n_ships;
  a.bits[0] = (const unsigned *)h->maps[OFX_MAP_BITS_LSB][0]; a.bits[1] = (const unsigned *)h->maps[OFX_MAP_BITS_LSB][1];
  a.bits_stride = (size_t)(PS * PS) >> 5;
  return policy_forward_impl(h, a);
}

extern "C" int ofx_policy_forward(ofx_handle *h, const float *weights, const uint8_t *ship_mask, float *act_values,
                                  int32_t *iaction, int32_t *ipointer, float *heatmap) {
  int rc = live_forward_check(h, weights, "ofx_policy_forward");
  if (rc) return rc;
  OFX_HIP(hipSetDevice(h->cfg.device));
  ForwardArgs a{};
  a.weights = weights;
  a.ship_mask = ship_mask; a.act_values = act_values; a.iaction = iaction; a.ipointer = ipointer; a.heatmap = heatmap;
  return live_forward(h, a);
}

// n stored observations (bits [n][2][5000], vec8 [n][8]), one policy sample each
static ForwardArgs obs_args(const float *weights, int32_t n_obs, const void *bits, const float *vec8) {
  const size_t words = (size_t)(PS * PS) >> 5;
  ForwardArgs a{};
  a.weights = weights; a.N = n_obs; a.M = 1;
  a.bits[0] = (const unsigned *)bits; a.bits[1] = a.bits[0] + words; a.bits_stride = 2 * words;
  a.vec8 = vec8;
  return a;
}

extern "C" int ofx_policy_forward_obs(ofx_handle *h, const float *weights, int32_t n_obs, const void *bits,
                                      const float *vec8, float *act_values, int32_t *iaction, int32_t *ipointer,
                                      float *ptr_max, const int32_t *probe, float *ptr_probe) {
  if (!h || !weights || !bits || !vec8 || n_obs < 1) { ofx_set_error("ofx_policy_forward_obs: bad argument"); return OFX_ERR_INVALID; }
  if ((probe == nullptr) != (ptr_probe == nullptr)) { ofx_set_error("ofx_policy_forward_obs: pass probe and ptr_probe together"); return OFX_ERR_INVALID; }
  OFX_HIP(hipSetDevice(h->cfg.device));
  ForwardArgs a = obs_args(weights, n_obs, bits, vec8);
  a.act_values = act_values; a.iaction = iaction; a.ipointer = ipointer; a.ptr_max = ptr_max; a.probe = probe; a.ptr_probe = ptr_probe;
  return policy_forward_impl(h, a);
}

// ofx_policy_forward_obs with the soft value of the pointer head (and, on request, the heat map it was reduced from)
extern "C" int ofx_policy_forward_obs_soft(ofx_handle *h, const float *weights, int32_t n_obs, const void *bits,
                                           const float *vec8, float tau_ptr, float *act_values, int32_t *iaction,
                                           int32_t *ipointer, float *ptr_max, const int32_t *probe, float *ptr_probe,
                                           float *ptr_soft, float *ptr_mass, float *heatmap) {
  if (!h || !weights || !bits || !vec8 || n_obs < 1) { ofx_set_error("ofx_policy_forward_obs_soft: bad argument"); return OFX_ERR_INVALID; }
  if ((probe == nullptr) != (ptr_probe == nullptr)) { ofx_set_error("ofx_policy_forward_obs_soft: pass probe and ptr_probe together"); return OFX_ERR_INVALID; }
  if (!(tau_ptr == 0.f || (tau_ptr >= 1e-6f && tau_ptr <= 1e30f))) {   // NaN fails every comparison
    ofx_set_error("ofx_policy_forward_obs_soft: tau_ptr = %g; it must be 0 or lie in [1e-6, 1e30]", (double)tau_ptr);
    return OFX_ERR_INVALID;
  }
  OFX_HIP(hipSetDevice(h->cfg.device));
  ForwardArgs a = obs_args(weights, n_obs, bits, vec8);
  a.act_values = act_values; a.iaction = iaction; a.ipointer = ipointer; a.ptr_max = ptr_max; a.probe = probe; a.ptr_probe = ptr_probe;
  a.heatmap = heatmap;
  a.soft = 1; a.tau_ptr = tau_ptr; a.ptr_soft = ptr_soft; a.ptr_mass = ptr_mass;
  return policy_forward_impl(h, a);
}

// model.predict on stored observations with the whole heat map written out (ofx_dqn_fit_reference, ofx_train.hip)
int ofx_policy_predict_obs(ofx_handle *h, const float *weights, int32_t n_obs, const void *bits, const float *vec8,
                           float *act_values, float *heatmap, float *ptr_max) {
  ForwardArgs a = obs_args(weights, n_obs, bits, vec8);
  a.act_values = act_values; a.heatmap = heatmap; a.ptr_max = ptr_max;
  return policy_forward_impl(h, a);
}

// The draw of ship i of arena a at `tick`: true when the ship explores, i.e. random_play() replaces its greedy choice
// (np.random.rand() <= epsilon, qlearnIA_V2.py:201, or the collecting phase).  The Philox words exist either way, so
// (*ia, *px, *py) is a valid random choice for every ship - ofx_policy_act probes the heat map there before it knows.
// `expo` (ofx_policy_epsilon_ladder, null = none) changes only WHETHER the ship explores: arena a explores at
// epsilon^expo[a]; exponent 1 leaves epsilon as it is (no pow), +inf is a greedy arena that not even `collecting` moves.
__device__ __forceinline__ bool explore_draw(int a, int i, int W, int H, int arena_base, double eps, const double *expo,
                                             ofx_rng_key key, uint32_t tick, int collecting, int32_t *ia,
                                             int32_t *px, int32_t *py) {
  uint32_t r[4];
  ofx_philox4x32_10((uint32_t)(arena_base + a), (uint32_t)i, tick, OFX_STREAM_EXPLORE, key, r);
  const double u = ofx_unit(r[0]);
  *ia = ofx_draw_int(r[1], 1);
  *px = ofx_draw_int(r[2], W - 1);
  *py = ofx_draw_int(r[3], H - 1);
  bool greedy;
  eps = arena_eps(eps, expo, a, &greedy);
  if (greedy) return false;
  return collecting || u <= eps;
}

__global__ void k_policy_explore(int N, int M, int W, int H, int arena_base, double eps, const double *expo, ofx_rng_key key,
                                 uint32_t tick, int collecting, const uint8_t *mask, int32_t *iaction,
                                 int32_t *ipointer) {
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= N * M || (mask && !mask[s])) return;
  const int a = s / M, i = s - a * M;
  int32_t ia, px, py;
  if (explore_draw(a, i, W, H, arena_base, eps, expo, key, tick, collecting, &ia, &px, &py)) {
    iaction[s] = ia;
    ipointer[2 * s] = px;
    ipointer[2 * s + 1] = py;
  }
}

extern "C" int ofx_policy_explore(ofx_handle *h, double epsilon, uint64_t seed, uint32_t tick, int32_t collecting,
                                  const uint8_t *ship_mask, int32_t *iaction, int32_t *ipointer) {
  if (!h) { ofx_set_error("ofx_policy_explore: null handle"); return OFX_ERR_INVALID; }
  if (!h->spawned) { ofx_set_error("ofx_policy_explore before ofx_spawn"); return OFX_ERR_STATE; }
  if (epsilon < 0.0 || epsilon > 1.0) { ofx_set_error("Value must me in range [0,1]"); return OFX_ERR_INVALID; }  // epsilon.py:56
  OFX_HIP(hipSetDevice(h->cfg.device));
  int rc;
  int32_t *ria, *rip;  // null = the handle's results
  if ((rc = ofx_policy_results(h, &ria, &rip))) return rc;
  if (!iaction) iaction = ria;
  if (!ipointer) ipointer = rip;
  const int S = h->cfg.n_arenas * h->cfg.n_ships;
  hipLaunchKernelGGL(k_policy_explore, dim3((S + 255) / 256), dim3(256), 0, h->stream, h->cfg.n_arenas, h->cfg.n_ships,
                     h->cfg.width, h->cfg.height, h->cfg.arena_base, epsilon, h->eps_expo, ofx_key(seed), tick, collecting, ship_mask, iaction, ipointer);
  OFX_HIP(hipGetLastError());
  return OFX_OK;
}

// ---- the exploration ladder: one exponent per local arena, kept by the handle (set-up calls: both synchronise)
extern "C" int ofx_policy_epsilon_ladder(ofx_handle *h, const double *expo_host) {
  if (!h) { ofx_set_error("ofx_policy_epsilon_ladder: null handle"); return OFX_ERR_INVALID; }
  const int N = h->cfg.n_arenas;
  if (expo_host)
    for (int a = 0; a < N; a++)
      if (!(expo_host[a] >= 0.0)) {  // NaN fails the comparison too; +inf passes
        ofx_set_error("ofx_policy_epsilon_ladder: exponent %d is %g; each must be >= 0 (+inf = a greedy arena)", a, expo_host[a]);
        return OFX_ERR_INVALID;
      }
  OFX_HIP(hipSetDevice(h->cfg.device));
  OFX_HIP(hipStreamSynchronize(h->stream));  // a kernel in flight may still read the old ladder
  if (!expo_host) {
    if (h->eps_expo) OFX_HIP(hipFree(h->eps_expo));
    h->eps_expo = nullptr;
    return OFX_OK;
  }
  if (!h->eps_expo) OFX_HIP(hipMalloc((void **)&h->eps_expo, sizeof(double) * N));
  OFX_HIP(hipMemcpy(h->eps_expo, expo_host, sizeof(double) * N, hipMemcpyHostToDevice));
  OFX_HIP(hipDeviceSynchronize());  // the copy from pageable memory is not ordered with the handle's non-blocking stream
  return OFX_OK;
}

extern "C" int ofx_policy_epsilon_ladder_host(ofx_handle *h, double *dst_host) {
  if (!h || !dst_host) { ofx_set_error("ofx_policy_epsilon_ladder_host: null argument"); return OFX_ERR_INVALID; }
  if (!h->eps_expo) { ofx_set_error("ofx_policy_epsilon_ladder_host: no ladder is set"); return OFX_ERR_STATE; }
  OFX_HIP(hipSetDevice(h->cfg.device));
  OFX_HIP(hipStreamSynchronize(h->stream));
  OFX_HIP(hipMemcpy(dst_host, h->eps_expo, sizeof(double) * h->cfg.n_arenas, hipMemcpyDeviceToHost));
  return OFX_OK;
}

// ---- ofx_policy_act: forward + exploration in one call, with the values of what was chosen --------------------------
// The exploration draw depends on (arena, ship, tick) alone, so it is made BEFORE the forward and handed to the head
// kernel as its probe: the heat map's value at an exploratory pointer leaves the same pass that finds the maximum.
// Everything is addressed by ship index s = a * M + i (a masked forward walks the compacted list, but hd_ship maps
// every work item back to s before it reads the probe or writes a result).
__global__ void k_policy_predraw(int N, int M, int W, int H, int arena_base, double eps, const double *expo, ofx_rng_key key,
                                 uint32_t tick, int collecting, const uint8_t *mask, uint8_t *explores,
                                 int32_t *draw_ia, int32_t *probe) {
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= N * M) return;
  if (mask && !mask[s]) {  // never read by the head, but never left uninitialised either
    explores[s] = 0; draw_ia[s] = 0; probe[2 * s] = probe[2 * s + 1] = 0;
    return;
  }
  const int a = s / M, i = s - a * M;
  int32_t ia, px, py;
  explores[s] = explore_draw(a, i, W, H, arena_base, eps, expo, key, tick, collecting, &ia, &px, &py) ? 1 : 0;
  draw_ia[s] = ia;
  probe[2 * s] = px;
  probe[2 * s + 1] = py;
}

__global__ void k_policy_act_finish(int S, const uint8_t *mask, const uint8_t *explores, const int32_t *draw_ia,
                                    const int32_t *probe, const float *act, const float *ptr_max, const float *ptr_probe,
                                    int32_t *iaction, int32_t *ipointer, float *q_sa, float *p_sp, float *v_act,
                                    float *v_ptr) {
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= S || (mask && !mask[s])) return;
  const bool ex = explores[s] != 0;
  if (ex) {
    iaction[s] = draw_ia[s];
    ipointer[2 * s] = probe[2 * s];
    ipointer[2 * s + 1] = probe[2 * s + 1];
  }
  const float a0 = act[2 * s], a1 = act[2 * s + 1];
  q_sa[s] = iaction[s] ? a1 : a0;
  v_act[s] = fmaxf(a0, a1);                   // np.max(prediction), as k_dqn_targets forms it
  v_ptr[s] = ptr_max[s];
  p_sp[s] = ex ? ptr_probe[s] : ptr_max[s];   // the greedy pointer is the arg-max: its value is the maximum
}

// the handle's block of ofx_policy_act, allocated once and kept: the arrays stand back to back in this order (floats, then
// int32, then bytes - every one aligned for its type with no rounding in between), S = N*M
struct ActBlock {
  float *q_sa, *p_sp, *v_act, *v_ptr;   // [S] each: what a null output of ofx_policy_act stands for
  float *act, *ptr_max, *ptr_probe;     // [S][2], [S], [S]: the forward's results they are selected from
  int32_t *draw_ia, *probe;             // [S], [S][2]: the pre-drawn exploration
  uint8_t *explores;                    // [S]
  size_t bytes;
};
static ActBlock act_block(const ofx_handle *h) {   // (before the block exists: null pointers, bytes alone)
  const size_t S = (size_t)h->cfg.n_arenas * h->cfg.n_ships;
  ActBlock B;
  B.bytes = 0;
  auto put = [&](size_t bytes) { char *p = h->act_vals ? (char *)h->act_vals + B.bytes : nullptr; B.bytes += bytes; return p; };
  B.q_sa = (float *)put(4 * S); B.p_sp = (float *)put(4 * S); B.v_act = (float *)put(4 * S); B.v_ptr = (float *)put(4 * S);
  B.act = (float *)put(4 * 2 * S); B.ptr_max = (float *)put(4 * S); B.ptr_probe = (float *)put(4 * S);
  B.draw_ia = (int32_t *)put(4 * S); B.probe = (int32_t *)put(4 * 2 * S); B.explores = (uint8_t *)put(S);
  return B;
}
static int policy_act_block(ofx_handle *h, ActBlock *B) {
  const size_t bytes = act_block(h).bytes;
  if (!h->act_vals) {
    OFX_HIP(hipMalloc((void **)&h->act_vals, bytes));
    OFX_HIP(hipMemsetAsync(h->act_vals, 0, bytes, h->stream));
  }
  *B = act_block(h);
  return OFX_OK;
}

int ofx_policy_act_values(ofx_handle *h, const float **q_sa, const float **p_sp, const float **v_act, const float **v_ptr) {
  if (!h->act_called) return OFX_ERR_STATE;
  const ActBlock B = act_block(h);
  *q_sa = B.q_sa; *p_sp = B.p_sp; *v_act = B.v_act; *v_ptr = B.v_ptr;
  return OFX_OK;
}

extern "C" int ofx_policy_act(ofx_handle *h, const float *weights, const uint8_t *ship_mask, double epsilon, uint64_t seed,
                              uint32_t tick, int32_t collecting, float *q_sa, float *p_sp, float *v_act, float *v_ptr) {
  int rc = live_forward_check(h, weights, "ofx_policy_act");
  if (rc) return rc;
  if (epsilon < 0.0 || epsilon > 1.0) { ofx_set_error("Value must me in range [0,1]"); return OFX_ERR_INVALID; }  // epsilon.py:56
  OFX_HIP(hipSetDevice(h->cfg.device));
  ActBlock B;
  if ((rc = policy_act_block(h, &B))) return rc;
  const int S = h->cfg.n_arenas * h->cfg.n_ships;
  // the handle's four arrays stand for "the last ofx_policy_act" only when that call wrote all four of them
  const bool kept = !q_sa && !p_sp && !v_act && !v_ptr;
  q_sa = q_sa ? q_sa : B.q_sa; p_sp = p_sp ? p_sp : B.p_sp;
  v_act = v_act ? v_act : B.v_act; v_ptr = v_ptr ? v_ptr : B.v_ptr;
  hipLaunchKernelGGL(k_policy_predraw, dim3((S + 255) / 256), dim3(256), 0, h->stream, h->cfg.n_arenas, h->cfg.n_ships,
                     h->cfg.width, h->cfg.height, h->cfg.arena_base, epsilon, h->eps_expo, ofx_key(seed), tick, collecting, ship_mask, B.explores, B.draw_ia, B.probe);
  OFX_HIP(hipGetLastError());
  ForwardArgs a{};
  a.weights = weights; a.ship_mask = ship_mask;
  a.act_values = B.act; a.ptr_max = B.ptr_max; a.probe = B.probe; a.ptr_probe = B.ptr_probe;
  h->act_called = false;
  if ((rc = live_forward(h, a))) return rc;   // (iaction, ipointer): the handle's results
  hipLaunchKernelGGL(k_policy_act_finish, dim3((S + 255) / 256), dim3(256), 0, h->stream, S, ship_mask, B.explores, B.draw_ia,
                     B.probe, B.act, B.ptr_max, B.ptr_probe, a.iaction, a.ipointer, q_sa, p_sp, v_act, v_ptr);
  OFX_HIP(hipGetLastError());
  h->act_called = kept;
  return OFX_OK;
}

// ---- ofx_policy_act_boltzmann: the same call with both heads sampled from softmax(Q / T) ---------------------------
// The pointer is sampled inside the streaming kernel (Gumbel-max on per-pixel noise, ofx_head.hip), the action by the
// finish kernel; nothing is drawn in front of the forward.  The collecting phase is ofx_policy_act's.
extern "C" int ofx_policy_act_boltzmann(ofx_handle *h, const float *weights, const uint8_t *ship_mask, double epsilon,
                                        float tau_act, float tau_ptr, uint64_t seed, uint32_t tick, int32_t collecting,
                                        float *q_sa, float *p_sp, float *v_act, float *v_ptr) {
  int rc = live_forward_check(h, weights, "ofx_policy_act_boltzmann");
  if (rc) return rc;
  if (epsilon < 0.0 || epsilon > 1.0) { ofx_set_error("Value must me in range [0,1]"); return OFX_ERR_INVALID; }  // epsilon.py:56
  if (!(tau_act >= 0.f && tau_act < INFINITY && tau_ptr >= 0.f && tau_ptr < INFINITY)) {   // NaN fails the comparisons
    ofx_set_error("ofx_policy_act_boltzmann: tau_act = %g, tau_ptr = %g; both must be finite and >= 0", (double)tau_act, (double)tau_ptr);
    return OFX_ERR_INVALID;
  }
  if (collecting) return ofx_policy_act(h, weights, ship_mask, epsilon, seed, tick, 1, q_sa, p_sp, v_act, v_ptr);
  OFX_HIP(hipSetDevice(h->cfg.device));
  ActBlock B;
  if ((rc = policy_act_block(h, &B))) return rc;
  const bool kept = !q_sa && !p_sp && !v_act && !v_ptr;   // as in ofx_policy_act
  BoltzArgs b;
  b.eps = epsilon; b.tau_act = tau_act; b.tau_ptr = tau_ptr;
  b.key = ofx_key(seed); b.tick = tick;
  b.q_sa = q_sa ? q_sa : B.q_sa; b.p_sp = p_sp ? p_sp : B.p_sp;
  b.v_act = v_act ? v_act : B.v_act; b.v_ptr = v_ptr ? v_ptr : B.v_ptr;
  ForwardArgs a{};
  a.weights = weights; a.ship_mask = ship_mask;
  a.act_values = B.act;
  a.boltz = &b;
  h->act_called = false;
  if ((rc = live_forward(h, a))) return rc;   // (iaction, ipointer): the handle's results
  h->act_called = kept;
  return OFX_OK;
}

// diagnostic: g_dev[i] = the sampling kernels' float32 Gumbel noise of Philox word words_dev[i]
extern "C" int ofx_policy_gumbel(ofx_handle *h, const uint32_t *words_dev, int32_t n, float *g_dev) {
  if (!h || !words_dev || !g_dev || n < 1) { ofx_set_error("ofx_policy_gumbel: bad argument"); return OFX_ERR_INVALID; }
  OFX_HIP(hipSetDevice(h->cfg.device));
  return ofx_head_gumbel(h, words_dev, n, g_dev);
}

extern "C" int ofx_policy_actions(ofx_handle *h, const int32_t *iaction, const int32_t *ipointer,
                                  const uint8_t *ship_mask, ofx_action *actions) {
  if (!h || !actions) { ofx_set_error("ofx_policy_actions: null argument"); return OFX_ERR_INVALID; }
  if (!h->spawned) { ofx_set_error("ofx_policy_actions before ofx_spawn"); return OFX_ERR_STATE; }
  OFX_HIP(hipSetDevice(h->cfg.device));
  const int S = h->cfg.n_arenas * h->cfg.n_ships;
  int rc;
  int32_t *ria, *rip;  // null = the handle's results
  if ((rc = ofx_policy_results(h, &ria, &rip))) return rc;
  if (!iaction) iaction = ria;
  if (!ipointer) ipointer = rip;
  hipLaunchKernelGGL(k_policy_actions, dim3((S + 255) / 256), dim3(256), 0, h->stream, S, h->st, iaction, ipointer,
                     ship_mask, actions);
  OFX_HIP(hipGetLastError());
  return OFX_OK;
}
