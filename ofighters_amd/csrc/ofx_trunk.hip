// ofx_trunk.hip - the trunk of the bi-head policy forward, 4 x [conv3x3 + BN + ReLU + maxpool2] once per image
// (conventions: ofx_policy.hip, whose k_policy_prepare folds BatchNorm into the weights this unit gets as pointers).
// The convolutions run on the matrix cores (k_convm: banded GEMM); conv1 reads the 1-bit maps through a 512-entry table
// (k_conv1_lut); large batches stream (k_trunk12: conv1 -> conv2 fused, k_conv3_stream).  k_conv is the plain VALU
// convolution: under OFX_OPT_TRUNK_PLAIN, the reference trunk of the agreement test.
#include "ofx_trunk.h"
#include "ofx_diag.h"
#include "ofx_lowp.h"
#include "ofx_trunk_tile.h"

// ---- generic direct 3x3 convolution ------------------------------------------------
// MODE: 0 planar f32 input, 1 two 1-bit maps
template <int CIN, int COUT, int TH, int TW, int MODE, bool POOL, bool OUT_HWC>
__global__ __launch_bounds__(((TH / 2) * (TW / 2) + 63) / 64 * 64) void k_conv(ConvParams p) {
  constexpr int NT = (TH / 2) * (TW / 2);
  constexpr int NTB = (NT + 63) / 64 * 64;
  constexpr int TWP = TW + 2;
  __shared__ __align__(16) float tile[CIN][TH + 2][TWP];
  const int img = blockIdx.x / p.tiles, t = blockIdx.x - img * p.tiles;
  if (p.mask && !p.mask[img]) return;  // block-uniform
  const int ty0 = (t / p.tiles_x) * TH, tx0 = (t % p.tiles_x) * TW;
  const int tid = threadIdx.x;
  const int H = p.H, W = p.W;

  // ---- stage the (TH+2) x (TW+2) x CIN input patch (zero outside the image: padding 'same').
  // Loads are issued in batches of SU before any LDS store so one memory latency covers SU elements.
  constexpr int TOTAL = CIN * (TH + 2) * TWP;
  constexpr int SU = 8;
  for (int base = 0; base < TOTAL; base += NTB * SU) {
    float vals[SU];
#pragma unroll
    for (int u = 0; u < SU; u++) {
      const int e = base + u * NTB + tid;
      float v = 0.f;
      if (e < TOTAL) {
        const int c = e % TWP, r = (e / TWP) % (TH + 2), ci = e / (TWP * (TH + 2));
        const int gy = ty0 - 1 + r, gx = tx0 - 1 + c;
        if (gy >= 0 && gy < H && gx >= 0 && gx < W) {
          if (MODE == 0) {
            v = p.in[(((size_t)img * CIN + ci) * H + gy) * W + gx];
          } else if (MODE == 1) {
            const int cell = gy * W + gx;
            v = (float)((p.bits[ci][(size_t)img * p.bits_stride + (cell >> 5)] >> (cell & 31)) & 1u);
          }
        }
      }
      vals[u] = v;
    }
#pragma unroll
    for (int u = 0; u < SU; u++) {
      const int e = base + u * NTB + tid;
      if (e < TOTAL) (&tile[0][0][0])[e] = vals[u];
    }
  }
  __syncthreads();
  if (tid >= NT) return;
  const int tr = tid / (TW / 2), tc = tid - tr * (TW / 2);

  float acc[2][2][COUT];
#pragma unroll
  for (int i = 0; i < 2; i++)
#pragma unroll
    for (int j = 0; j < 2; j++)
#pragma unroll
      for (int co = 0; co < COUT; co++) acc[i][j][co] = 0.f;

#pragma unroll
  for (int ci = 0; ci < CIN; ci++) {
    float v[4][4];
#pragma unroll
    for (int r = 0; r < 4; r++) {
      const float2 lo = *reinterpret_cast<const float2 *>(&tile[ci][2 * tr + r][2 * tc]);
      const float2 hi = *reinterpret_cast<const float2 *>(&tile[ci][2 * tr + r][2 * tc + 2]);
      v[r][0] = lo.x; v[r][1] = lo.y; v[r][2] = hi.x; v[r][3] = hi.y;
    }
#pragma unroll
    for (int dy = 0; dy < 3; dy++)
#pragma unroll
      for (int dx = 0; dx < 3; dx++)
#pragma unroll
        for (int co = 0; co < COUT; co++) {
          const float wv = p.w[((dy * 3 + dx) * CIN + ci) * COUT + co];  // wave-uniform -> scalar load
#pragma unroll
          for (int i = 0; i < 2; i++)
#pragma unroll
            for (int j = 0; j < 2; j++) acc[i][j][co] = __builtin_fmaf(v[i + dy][j + dx], wv, acc[i][j][co]);
        }
  }

  // ---- epilogue: folded bias, ReLU, optional 2x2 max-pool ----
  const int oy = ty0 + 2 * tr, ox = tx0 + 2 * tc;
#pragma unroll
  for (int co = 0; co < COUT; co++) {
    const float bias = p.b[co];
    float o00 = fmaxf(acc[0][0][co] + bias, 0.f), o01 = fmaxf(acc[0][1][co] + bias, 0.f);
    float o10 = fmaxf(acc[1][0][co] + bias, 0.f), o11 = fmaxf(acc[1][1][co] + bias, 0.f);
    if (POOL) {
      const float m = fmaxf(fmaxf(o00, o01), fmaxf(o10, o11));
      const int Ho = H >> 1, Wo = W >> 1, py = oy >> 1, px = ox >> 1;
      if (OUT_HWC) p.out[(((size_t)img * Ho + py) * Wo + px) * COUT + co] = m;
      else p.out[(((size_t)img * COUT + co) * Ho + py) * Wo + px] = m;
    } else {
      float *o = p.out + (((size_t)img * COUT + co) * H + oy) * W + ox;
      *reinterpret_cast<float2 *>(o) = make_float2(o00, o01);
      *reinterpret_cast<float2 *>(o + W) = make_float2(o10, o11);
    }
  }
}

// ---- trunk convolution on the matrix cores ---------------------------------------------------------------------
// conv3x3 (zero padding) + folded BN + ReLU + 2x2 max-pool as a GEMM whose N dimension is 8 output channels x 2
// adjacent output rows:  D[pixel x][(co, r)] = sum_k A[x][k] B[k][(co, r)],  k = (input row 0..3, dx, ci),
// B[k][(co, r)] = w[row - r][dx][ci][co] when 0 <= row - r <= 2, else 0  -> K = 12 CIN, 3/4 of the MACs useful, but a
// v_mfma_f32_16x16x4_f32 retires 32 MAC/cycle against 16 for v_fmac_f32 (both share the SIMD's issue slots on gfx950,
// tools/ubench_mix.hip), and the whole epilogue of an M-tile (2x2 pool, ReLU, store) is ~10 VALU instructions.
// A[x][k] is gathered from an LDS copy of the input tile (one ds_read_b32 per lane per MFMA, immediate offsets);
// the row pair of a column group shares one accumulator quad: lane (n = (co, r), kq) holds pixels 4 kq .. 4 kq + 3,
// so the x-pool is in-lane and the y-pool is one DPP quad swap.
// The M-tile itself - taps, matrix sequence, pool - is stated in ofx_trunk_tile.h for every kernel below.
// OFX_OPT_POLICY_BF16 (opt-in): the same banded GEMM on v_mfma_f32_16x16x16_bf16 / _f16 - K = 96 as 6 MFMAs of K = 16
// instead of 24 of K = 4.  MFMA J, lane (pixel n16, k-quarter kq), element i: k <-> (tap = 2 J + (kq >> 1), ci = 4 (kq & 1) + i):
// the A operand is the four channel planes 4 (kq & 1) .. + 3 at the tap's (row, dx) of the fp32 LDS tile, rounded to
// 16 bits on the way in; the B operand is packed once from the same PrepLayout::wbm the fp32 kernel uses: the lane's six
// from wbm [24][64] (value for MFMA j of the fp32 form, lane l: k = l >> 4 -> ci = (l >> 4) + 4 (j & 1), tap j >> 1).
// fp32 accumulation, same epilogue.
template <int LP>
__device__ __forceinline__ void ts_bw_lp(const float *wbm, int n16, int kq, lp_x4 (&bwb)[6]) {
#pragma unroll
  for (int J = 0; J < 6; J++) {
    const int j = 2 * (2 * J + (kq >> 1)) + (kq & 1);
    const float *q = wbm + j * 64 + n16;
    bwb[J] = lp_pk4<LP>(q[0], q[16], q[32], q[48]);
  }
}
// Planar f32 input [img][8][H][W] (conv1 reads the bit maps through k_conv1_lut).  Output: planar [img][8][H/2][W/2] or
// (OUT_HWC) [img][H/2][W/2][8].  TH rows x 16 NG columns per workgroup, TH even, H % TH == 0; W is masked.
// A workgroup walks TPW consecutive tiles of one image: the weights are fetched once, the global loads of tile i+1 are
// in flight (in registers) while tile i computes, and the grid stays small (the dispatcher needs ~5 ns per workgroup:
// one workgroup per tile cost 1.6 ms of launch floor for conv2 alone).
template <int TH, int NG, bool OUT_HWC, int TPW, int LP = 0>
__global__ __launch_bounds__(256) void k_convm(ConvParams p) {
  constexpr bool BF16 = LP != 0;
  constexpr int CIN = 8;
  constexpr int TW = 16 * NG, LS = TW + 8;  // LDS row: image column tx0 + c sits at index c + 4 (16-byte aligned interior),
                                            // the left / right halo columns at 3 and TW + 4
  constexpr int PLS = ((TH + 2) * LS + 63) / 64 * 64 + 16;  // plane stride = 16 mod 64: the 4 k-quarters hit different banks
  constexpr int NK = 3 * CIN;                                // MFMAs per M-tile (K = 12 CIN)
  constexpr int JOBS = NG * (TH / 2);
  constexpr int ROWS = CIN * (TH + 2);
  constexpr bool VEC = !OUT_HWC;                             // rows of W floats are 16-byte aligned (W % 4 == 0)
  __shared__ __align__(16) float tile[CIN * PLS];
  const unsigned bid = blockIdx.x;
  // XCD-aware order: workgroups go round-robin over the 8 XCDs (each with its own L2), so workgroup b works on image
  // 8 (b / 8 / wpi) + b % 8: the tiles of one image run back to back on ONE XCD and the halo rows a tile shares with
  // its vertical neighbour come out of that L2 (conv2: FETCH_SIZE 10.6 -> 5.1 GB for a 5.24 GB input; same time - the
  // kernel is bound by its compute phase, 2.45 ms with the staging ablated, 1.19 ms with only the staging)
  const int wpi = p.tiles / TPW, j = (int)(bid >> 3);        // p.tiles % TPW == 0: all tiles of a workgroup share the image
  const int img = (j / wpi) * 8 + (int)(bid & 7u), t_first = (j % wpi) * TPW;
  if (img >= p.images) return;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int H = p.H, W = p.W;
  const int n16 = lane & 15, kq = lane >> 4, co = n16 >> 1, r = n16 & 1;

  // B operand: the lane's column (co, r) of the banded weight matrix, rows k = 4 j + kq (16-bit: ts_bw_lp)
  float bw[BF16 ? 1 : NK];
  lp_x4 bwb[6];
  int toff[6];
  if constexpr (BF16) {
    ts_bw_lp<LP ? LP : 1>(p.wbm, n16, kq, bwb);
    mt_toff<LS, PLS>(kq, toff);
  } else {
#pragma unroll
    for (int j = 0; j < NK; j++) bw[j] = p.wbm[j * 64 + lane];  // pre-arranged by k_policy_prepare: one coalesced load
  }
  const float bias = p.b[co];
  const f32x4 binit = {bias, bias, bias, bias};
  const int H2 = H >> 1, W2 = W >> 1;

  // ---- staging, split into fetch (global -> registers) and commit (registers -> LDS) ----
  constexpr int V4 = TW / 4, RPW = VEC ? (ROWS + 3) / 4 : 1;       // VEC: float4 per row, rows per wave
  static_assert(!VEC || V4 + 2 <= 64, "tile row wider than one wave");
  f32x4 vpre[RPW];  // native vectors: a float4 select is lowered to a pointer select + flat loads
  const f32x4 z4 = {0.f, 0.f, 0.f, 0.f};

  auto fetch = [&](int t) {
    const int ty0 = (t / p.tiles_x) * TH, tx0 = (t % p.tiles_x) * TW;
    if constexpr (VEC) {
      // a wave moves one tile row per step: lane i < V4 the i-th float4 of the interior, lanes V4 / V4+1 the float4
      // that holds the left / right halo column
      const int gxl = lane < V4 ? tx0 + 4 * lane : (lane == V4 ? tx0 - 4 : tx0 + TW);
      const bool colok = lane < V4 + 2 && gxl >= 0 && gxl < W;
      const float *imgbase = p.in + (size_t)img * CIN * H * W;
#pragma unroll
      for (int u = 0; u < RPW; u++) {
        const int rr = wv + 4 * u;
        const int ci = rr / (TH + 2), r_ = rr - ci * (TH + 2), gy = ty0 - 1 + r_;
        const bool rowok = rr < ROWS && gy >= 0 && gy < H;  // wave-uniform
        // 32-bit offset from the image's base (scalar base + vector offset addressing; an image is < 4 GB)
        const unsigned off = (unsigned)((rowok ? ci * H + gy : 0) * W + gxl);
        vpre[u] = z4;
        if (rowok && colok) vpre[u] = *reinterpret_cast<const f32x4 *>(imgbase + off);  // exec-masked global load
      }
    }
  };

  auto commit = [&](int t) {
    const int ty0 = (t / p.tiles_x) * TH, tx0 = (t % p.tiles_x) * TW;
    if constexpr (VEC) {
#pragma unroll
      for (int u = 0; u < RPW; u++) {
        const int rr = wv + 4 * u;
        if (rr >= ROWS) break;  // wave-uniform
        const int ci = rr / (TH + 2), r_ = rr - ci * (TH + 2);
        float *trow = &tile[ci * PLS + r_ * LS];
        if (lane < V4) *reinterpret_cast<f32x4 *>(trow + 4 + 4 * lane) = vpre[u];
        else if (lane == V4) trow[3] = vpre[u][3];
        else if (lane == V4 + 1) trow[TW + 4] = vpre[u][0];
      }
    } else {  // rows that are not a multiple of 16 bytes (the 50x50 layer: W even, W <= TW): 8-byte pieces, every load of
              // a thread in flight before the first LDS store; the halo columns are zeroed once (see below)
      constexpr int TOTAL = CIN * (TH + 2) * (TW / 2), SU = (TOTAL + 255) / 256;
      (void)tx0;  // one tile per image row (launch_convm checks)
      f32x2 vals[SU];
      const int W2c = W >> 1;
#pragma unroll
      for (int u = 0; u < SU; u++) {
        const int e = u * 256 + tid;
        const int j = e % (TW / 2), rr = (e / (TW / 2)) % (TH + 2), ci = e / ((TW / 2) * (TH + 2));
        const int gy = ty0 - 1 + rr;
        vals[u] = (f32x2){0.f, 0.f};
        if (e < TOTAL && j < W2c && gy >= 0 && gy < H)
          vals[u] = *reinterpret_cast<const f32x2 *>(p.in + (((size_t)img * CIN + ci) * H + gy) * W + 2 * j);
      }
#pragma unroll
      for (int u = 0; u < SU; u++) {
        const int e = u * 256 + tid;
        const int j = e % (TW / 2), rr = (e / (TW / 2)) % (TH + 2), ci = e / ((TW / 2) * (TH + 2));
        if (e < TOTAL && j <= W2c) *reinterpret_cast<f32x2 *>(&tile[ci * PLS + rr * LS + 4 + 2 * j]) = vals[u];
      }
    }
  };

  const float *abase = &tile[kq * PLS + n16 + 3];  // the lane's A row of the M-tile at the tile's origin (taps: mt_aof)
  if constexpr (!VEC) {  // left halo column (image column -1): never written by the staging above
    for (int e = tid; e < CIN * (TH + 2); e += 256) tile[(e / (TH + 2)) * PLS + (e % (TH + 2)) * LS + 3] = 0.f;
  }
  fetch(t_first);
#pragma unroll 1
  for (int i = 0; i < TPW; i++) {
    const int t = t_first + i;
    const int ty0 = (t / p.tiles_x) * TH, tx0 = (t % p.tiles_x) * TW;
    commit(t);
    __syncthreads();
    if (i + 1 < TPW) fetch(t + 1);

    // epilogue of an M-tile: pool + ReLU (mt_pool), one 8-byte store from the r = 0 lanes
    float *const obase = OUT_HWC ? p.out + (((size_t)img * H2 + (ty0 >> 1)) * W2 + (tx0 >> 1) + 2 * kq) * 8 + co
                                 : p.out + (((size_t)img * 8 + co) * H2 + (ty0 >> 1)) * W2 + (tx0 >> 1) + 2 * kq;
    auto finish = [&](const f32x4 d, int g, int tt) {
      const f32x2 q = mt_pool(d);
      const float q0 = q[0], q1 = q[1];
      const int px = ((tx0 + 16 * g) >> 1) + 2 * kq;
      if (r == 0 && px < W2) {
        if (OUT_HWC) {
          float *op = obase + ((size_t)tt * W2 + 8 * g) * 8;
          op[0] = q0;
          if (px + 1 < W2) op[8] = q1;
        } else {  // W2 is even here: px < W2 implies px + 1 < W2
          *reinterpret_cast<float2 *>(obase + tt * W2 + 8 * g) = make_float2(q0, q1);
        }
      }
    };
    // two M-tiles per iteration (independent accumulator chains keep the matrix pipe busy); a trailing odd one alone
#pragma unroll 1
    for (int job = wv; job < JOBS; job += 8) {
      const int job1 = job + 4;
      const int g0 = job % NG, t0 = job / NG;
      const float *a0 = abase + (2 * t0) * LS + 16 * g0;
      if (job1 < JOBS) {  // wave-uniform
        const int g1 = job1 % NG, t1 = job1 / NG;
        const float *a1 = abase + (2 * t1) * LS + 16 * g1;
        f32x4 d0 = binit, d1 = binit;
#pragma unroll
        for (int j = 0; j < MT_NJ<LP>; j++) mt_step<LP, LS, PLS>(j, bw, bwb, toff, MtAcc{a0, d0}, MtAcc{a1, d1});
        finish(d0, g0, t0);
        finish(d1, g1, t1);
      } else {
        f32x4 d0 = binit;
#pragma unroll
        for (int j = 0; j < MT_NJ<LP>; j++) mt_step<LP, LS, PLS>(j, bw, bwb, toff, MtAcc{a0, d0});
        finish(d0, g0, t0);
      }
    }
    if (i + 1 < TPW) __syncthreads();  // the next commit overwrites the tile
  }
}

template <int TH, int NG, bool OUT_HWC, int TPW, int LP = 0>
static int launch_convm(ofx_handle *h, ConvParams p, int images, int H) {
  p.H = H; p.W = H;
  p.tiles_x = (H + 16 * NG - 1) / (16 * NG);
  p.tiles = p.tiles_x * (H / TH);
  if (p.tiles % TPW) { ofx_set_error("launch_convm: %d tiles per image not divisible by %d", p.tiles, TPW); return OFX_ERR_INVALID; }
  if (OUT_HWC && (H % 2 || H > 16 * NG)) { ofx_set_error("launch_convm: the 8-byte staging takes even rows of one tile width"); return OFX_ERR_INVALID; }
  p.images = images;
  hipLaunchKernelGGL((k_convm<TH, NG, OUT_HWC, TPW, LP>), dim3((unsigned)((images + 7) / 8 * 8 * (p.tiles / TPW))), dim3(256), 0,
                     h->stream, p);
  OFX_HIP(hipGetLastError());
  return OFX_OK;
}

// ---- conv1 on the binary observation maps as a table lookup ------------------------------------------------------
// The two input channels are 1-bit maps, so conv3x3 of one channel at one pixel takes one of 512 values per output
// channel: out[co] = b[co] + LUT[0][pattern0][co] + LUT[1][pattern1][co] (PrepLayout::lut1, 32 KB, staged in LDS).
// Every pixel is evaluated (no sparsity shortcut); a thread owns one pooled output pixel = 2x2 conv outputs = a
// 4x4 bit window per channel: 8 aligned word pairs + funnel shifts give the windows, 16 ds_read_b128 the table rows,
// then 2x2 max-pool + ReLU and 8 coalesced stores (planar [img][8][200][200]).  ~170 VALU instructions per pooled
// pixel against 6 MFMAs + epilogue per 16 in the GEMM form (3.4 ms): the kernel is bound by its 5.2 GB of output.
// Input rows are re-aligned while staging: bit x + 1 of LDS row r <-> image column x of row ty0 - 1 + r (bit 0 and
// the bits past column W-1 are the zero padding).
// staged bits x0 .. x0 + NB - 1 of a staged row
template <int NB>
__device__ __forceinline__ unsigned c1_window(const unsigned *row, int x0) {
  const unsigned *rw = row + (x0 >> 5);
  return __funnelshift_r(rw[0], rw[1], (unsigned)(x0 & 31)) & ((1u << NB) - 1u);
}
template <int TH>
__global__ __launch_bounds__(256) void k_conv1_lut(ConvParams p, const float *lut) {
  constexpr int W = PS, H = PS, WR = 14;                       // words per staged row (402 bits)
  constexpr int W2 = W / 2, NPX = (TH / 2) * W2;
  __shared__ __align__(16) float slut[2 * 512 * 8];
  __shared__ unsigned rows[2][TH + 2][WR];
  const int tiles = H / TH;
  const int img = blockIdx.x / tiles, ty0 = (blockIdx.x - img * tiles) * TH;
  const int tid = threadIdx.x;
  for (int e = tid; e < 2 * 512 * 8 / 4; e += 256)
    reinterpret_cast<float4 *>(slut)[e] = reinterpret_cast<const float4 *>(lut)[e];
  for (int e = tid; e < 2 * (TH + 2) * WR; e += 256) {
    const int w = e % WR, r = (e / WR) % (TH + 2), ci = e / (WR * (TH + 2));
    const int gy = ty0 - 1 + r;
    unsigned out = 0u;
    if (gy >= 0 && gy < H) {
      // output bits b = 0..31 <-> column x = 32 w - 1 + b <-> cell gy * W + x
      const long long s0 = (long long)gy * W + 32 * w - 1;        // cell of output bit 0 (-1 only for gy = 0, w = 0)
      const unsigned *bits = p.bits[ci] + (size_t)img * p.bits_stride;
      const long long sw = s0 >> 5;                               // arithmetic shift: -1 -> word -1
      const unsigned lo = (sw >= 0 && sw < (PS * PS) >> 5) ? bits[sw] : 0u;
      const unsigned hi = (sw + 1 < (PS * PS) >> 5) ? bits[sw + 1] : 0u;
      out = __funnelshift_r(lo, hi, (unsigned)(s0 & 31));
      // keep only columns 0 <= x < W of THIS row
      const int xlo = 32 * w - 1;
      if (xlo < 0) out &= ~1u;
      const int over = xlo + 32 - W;                              // bits past the last column
      if (over > 0) out = over >= 32 ? 0u : (out & (0xFFFFFFFFu >> over));
    }
    rows[ci][r][w] = out;
  }
  __syncthreads();
  float *const obase = p.out + ((size_t)img * 8 * (H / 2) + (ty0 >> 1)) * W2;  // wave-uniform: scalar base + 32-bit offsets
  // a thread owns FOUR horizontally adjacent pooled pixels: the kernel is bound by its 5.2 GB of output, and 16-byte
  // stores (1 KB contiguous per wave and channel plane) use the write path better than 4-byte ones (256 B)
  constexpr int NQ = NPX / 4, QR = W2 / 4;                       // quads of the tile, quads per pooled row
  for (int qd = tid; qd < NQ; qd += 256) {
    const int py = qd / QR, pq = qd - py * QR;
    const int x0 = 8 * pq;                                        // window = staged bits x0 .. x0 + 9 of rows 2 py .. 2 py + 3
    unsigned f[2][4];
#pragma unroll
    for (int ci = 0; ci < 2; ci++)
#pragma unroll
      for (int r = 0; r < 4; r++) f[ci][r] = c1_window<10>(rows[ci][2 * py + r], x0);
    f32x4 m4[8];                                                  // [channel] = the 4 pixels
#pragma unroll
    for (int j = 0; j < 4; j++) {
      f32x4 acc[4][2];                                            // [2x2 pixel][channels 0-3 | 4-7]
#pragma unroll
      for (int ci = 0; ci < 2; ci++)
#pragma unroll
        for (int q = 0; q < 4; q++) {
          const int dy = q >> 1, sh = 2 * j + (q & 1);
          const unsigned pat = ((f[ci][dy] >> sh) & 7u) | (((f[ci][dy + 1] >> sh) & 7u) << 3) | (((f[ci][dy + 2] >> sh) & 7u) << 6);
          const f32x4 *e = reinterpret_cast<const f32x4 *>(&slut[(ci * 512 + pat) * 8]);
          if (ci == 0) { acc[q][0] = e[0]; acc[q][1] = e[1]; }    // the table of channel 0 carries the bias
          else { acc[q][0] += e[0]; acc[q][1] += e[1]; }
        }
#pragma unroll
      for (int co = 0; co < 8; co++) {
        float m;  // the operands are ordinary VALU results (interlocked), not MFMA results: asm is safe here
        asm("v_max3_f32 %0, %1, %2, 0" : "=v"(m) : "v"(acc[0][co >> 2][co & 3]), "v"(acc[1][co >> 2][co & 3]));
        asm("v_max3_f32 %0, %1, %2, %3" : "=v"(m) : "v"(acc[2][co >> 2][co & 3]), "v"(acc[3][co >> 2][co & 3]), "v"(m));
        m4[co][j] = m;
      }
    }
    const unsigned off = (unsigned)(py * W2 + 4 * pq);
#pragma unroll
    for (int co = 0; co < 8; co++) *reinterpret_cast<f32x4 *>(obase + (size_t)co * (H / 2) * W2 + off) = m4[co];
  }
}

// ---- streaming trunk kernels (k_trunk12, k_conv3_stream): the GEMM phase ---------------------------------------------
// k_convm's banded GEMM over an LDS tile of RP row pairs x WD columns (planes PLS apart, rows LS apart; abase = the
// lane's k-quarter plane at column -1 of tile row 0), built from ofx_trunk_tile.h: the flat M-tiles, their A rows and their
// store (MtFlat), the matrix sequence (mt_step), the epilogue (mt_pool).  What the drivers below add is the schedule:
//   fp32, dense:   wave w takes tiles w, w + 16, w + 32, w + 48 as four interleaved accumulator chains (a wave with
//                  three: a pair and a single);
//   16-bit, dense: pairs, the last tile twice when it is alone;
//   sparse:        the tiles that have to run, dealt to the waves by one ballot, as pairs and a single.
// orow = the lane's channel plane at the step's first pooled row (planar [.][WD/2]).
template <int WD, int RP, int LS, int PLS, int LP>
__device__ __forceinline__ void ts_gemm_phase(const float *abase, const float (&bw)[LP ? 1 : 24], const lp_x4 (&bwb)[6],
                                              const f32x4 binit, int wv, int n16, int kq, int r, float *orow) {
  using F = MtFlat<WD, RP, LS>;
  constexpr int NT = F::NT;
  int toff[6];
  if constexpr (LP != 0) mt_toff<LS, PLS>(kq, toff);  // the 16-bit taps; fp32 reads none
  auto finish = [&](const f32x4 d, int T) { F::finish(d, orow, T, kq, r); };
  auto a_of_tile = [&](int T) { return F::a_of_tile(abase, T, n16); };
  if constexpr (LP != 0) {
#pragma unroll 1
    for (int T = wv; T < NT; T += 32) {  // two M-tiles at a time: two accumulator chains (the last tile twice when it is alone)
      const int T1 = T + 16;
      const bool two = T1 < NT;          // wave-uniform
      const float *a0 = a_of_tile(T), *a1 = a_of_tile(two ? T1 : T);
      f32x4 d0 = binit, d1 = binit;
#pragma unroll
      for (int j = 0; j < MT_NJ<LP>; j++) mt_step<LP, LS, PLS>(j, bw, bwb, toff, MtAcc{a0, d0}, MtAcc{a1, d1});
      finish(d0, T);
      if (two) finish(d1, T1);
    }
  } else if (wv + 48 < NT) {  // all four M-tiles of the wave at once (k_trunk12: 3.0 -> 2.84 ms against two pairs)
    const float *a0 = a_of_tile(wv), *a1 = a_of_tile(wv + 16), *a2 = a_of_tile(wv + 32), *a3 = a_of_tile(wv + 48);
    f32x4 d0 = binit, d1 = binit, d2 = binit, d3 = binit;
#pragma unroll
    for (int j = 0; j < MT_NJ<LP>; j++) mt_step<LP, LS, PLS>(j, bw, bwb, toff, MtAcc{a0, d0}, MtAcc{a1, d1}, MtAcc{a2, d2}, MtAcc{a3, d3});
    finish(d0, wv); finish(d1, wv + 16); finish(d2, wv + 32); finish(d3, wv + 48);
  } else {
#pragma unroll 1
    for (int T = wv; T < NT; T += 32) {
      const int T1 = T + 16;
      const float *a0 = a_of_tile(T);
      if (T1 < NT) {  // wave-uniform
        const float *a1 = a_of_tile(T1);
        f32x4 d0 = binit, d1 = binit;
#pragma unroll
        for (int j = 0; j < MT_NJ<LP>; j++) mt_step<LP, LS, PLS>(j, bw, bwb, toff, MtAcc{a0, d0}, MtAcc{a1, d1});
        finish(d0, T);
        finish(d1, T1);
      } else {
        f32x4 d0 = binit;
#pragma unroll
        for (int j = 0; j < MT_NJ<LP>; j++) mt_step<LP, LS, PLS>(j, bw, bwb, toff, MtAcc{a0, d0});
        finish(d0, T);
      }
    }
  }
}

// OFX_OPT_TRUNK_SPARSE (exact; the default): the same GEMM phase, but an M-tile whose whole input window - 4 tile rows x 18
// columns - holds the layer's CONSTANT input (conv1 of an empty neighbourhood: every channel plane at K1[ci]) and touches
// no zero padding stores the constant K2[co] the dense MFMA sequence gives for such a window (computed by that very
// sequence once per workgroup: the same bits) instead of running its 24 MFMAs.  nz: per tile row 8 words, bit x set
// <-> column x of that row is NOT known to be constant (phase A).  An M-tile that crosses from one row pair into the
// next contains columns 199 and 0, i.e. touches the padding: only tiles inside one row pair with 1 <= x, x + 15 <= 198
// can be constant.  top / bottom: tile row 0 / the last tile row is a padding row of the image.
// LP != 0: the same with the 16-bit operand sequence (K2 then comes from THAT sequence: mt_const).
template <int WD, int RP, int LS, int PLS, int LP>
__device__ __forceinline__ void ts_gemm_phase_sparse(const float *abase, const float (&bw)[LP ? 1 : 24], const lp_x4 (&bwb)[6],
                                                     const f32x4 binit, int wv, int lane,
                                                     int n16, int kq, int r, float *orow, const unsigned *nz, float k2,
                                                     bool top, bool bottom, unsigned &n_exec, unsigned &n_all,
                                                     unsigned *marks = nullptr, unsigned long long *dbg = nullptr) {
#if OFX_TRUNK_STAMPS
  unsigned long long g_last = __builtin_amdgcn_s_memtime();
#define TSG_STAMP(i) do { const unsigned long long t_ = __builtin_amdgcn_s_memtime(); dbg[i] += t_ - g_last; g_last = t_; } while (0)
#else
#define TSG_STAMP(i) do { } while (0)
#endif
  using F = MtFlat<WD, RP, LS>;
  constexpr int NPX = F::NPX, NT = F::NT;
  int toff[6];
  if constexpr (LP != 0) mt_toff<LS, PLS>(kq, toff);  // the 16-bit taps; fp32 reads none
  // the M-tile's matrix sequence on one or two accumulator chains, and its epilogue
  auto mm = [&](auto... c) {
#pragma unroll
    for (int j = 0; j < MT_NJ<LP>; j++) mt_step<LP, LS, PLS>(j, bw, bwb, toff, c...);
  };
  auto finish = [&](const f32x4 d, int T) { F::finish(d, orow, T, kq, r); };
  auto a_of_tile = [&](int T) { return F::a_of_tile(abase, T, n16); };
  // Every wave classifies ALL the step's M-tiles by itself, lane T tile T: no list to build, no barrier.  Bit T of the
  // mask: tile T has to run.  (A first version let a wave test its own four tiles one after the other with eight lanes each
  // and appended to a shared list behind a barrier: 4 500 cycles per step for the classification alone, stamps.)
  unsigned long long run_mask;
  bool run;
  {
    const int T = lane, P = 16 * T, rp = P / WD, x = P - rp * WD;
    run = T < NT;
    if (run && !(x < 1 || x + 15 > WD - 2 || P + 15 >= NPX || (top && rp == 0) || (bottom && rp == RP - 1))) {
      // window = bits x - 1 .. x + 16 of tile rows 2 rp .. 2 rp + 3: two words per row
      const int w0 = (x - 1) >> 5, lo = (x - 1) & 31;
      const unsigned m0 = 0x3FFFFu << lo, m1 = lo + 18 > 32 ? (1u << (lo + 18 - 32)) - 1u : 0u;
      unsigned any = 0u;
#pragma unroll
      for (int rr = 0; rr < 4; rr++) {
        const unsigned *rw = nz + (2 * rp + rr) * 8 + w0;
        any |= (rw[0] & m0) | (rw[1] & m1);
      }
      run = any != 0u;
    }
    run_mask = __builtin_amdgcn_ballot_w64(run);
  }
  // marks != null (k_trunk12; an LDS array): the step's OUTPUT marks for the next layer, RP pooled rows x (WD / 2 + 31) / 32
  // words, bit x of row y set <-> the pooled pixel (y, x) was written by a tile that ran (it may differ from k2).  Tile T
  // writes the pooled pixels 8 T .. 8 T + 7 of the step's flat RP x WD / 2 enumeration, so a word is five mask bits spread
  // to bytes and shifted to the word's start; one lane per word of the last wave.  The caller stores them behind the
  // step's barrier (a global pointer kept alive through this phase spilled k_trunk12<0, true>: 118 -> 128 VGPRs + scratch).
  if (marks != nullptr && wv == 15) {
    constexpr int W2 = WD / 2, WPR = (W2 + 31) / 32;
    static_assert(RP * WPR <= 64, "one lane per word");
    if (lane < RP * WPR) {
      const int y = lane / WPR, w = lane - y * WPR;
      const int f0 = y * W2 + 32 * w, t0 = f0 >> 3;                // flat pooled pixel of bit 0, its tile
      const unsigned b5 = (unsigned)(run_mask >> t0);              // tiles t0 .. t0 + 4 (t0 < 64; no tile past NT is set)
      const unsigned lo = (((b5 & 15u) * 0x00204081u) & 0x01010101u) * 0xFFu, hi = ((b5 >> 4) & 1u) * 0xFFu;  // a bit -> a byte
      unsigned word = __funnelshift_r(lo, hi, (unsigned)(f0 & 7));
      const int nb = W2 - 32 * w;                                  // columns of the row in this word
      if (nb < 32) word &= (1u << nb) - 1u;
      marks[lane] = word;
    }
  }
  auto store_const = [&](int T) {                                          // the constant tile: the dense result, stored
    F::template store<true>(orow, T, kq, r, k2, k2);
  };
  auto run1 = [&](int T0) {
    f32x4 d0 = binit;
    mm(MtAcc{a_of_tile(T0), d0});
    finish(d0, T0);
  };
  // the wave's own four tiles: the constant ones are stored; then the RUN tiles are dealt out over all 16 waves - wave w
  // takes the w-th, (w + 16)-th, ... set bit of the mask (a tile's result does not depend on who computes it)
#pragma unroll 1
  for (int T = wv; T < NT; T += 16)
    if (!((run_mask >> T) & 1ull)) store_const(T);
  if (wv == 0) { n_all += (unsigned)NT; n_exec += (unsigned)__builtin_popcountll(run_mask); }
  TSG_STAMP(0);
  // lane T knows its tile's rank among the run tiles (the set bits below it); one more ballot gives the wave ITS tiles,
  // four at most.  (Walking the mask bit by bit to the w-th, (w + 16)-th, ... set bit was ~700 scalar instructions per wave
  // and step with three tiles per wave, k_conv3_stream: more than the skipped tiles saved.)
  const unsigned rank = __builtin_amdgcn_mbcnt_hi((unsigned)(run_mask >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)run_mask, 0u));
  unsigned long long m = __builtin_amdgcn_ballot_w64(run && (rank & 15u) == (unsigned)wv);
#pragma unroll 1
  while (m) {
    const int T0 = __builtin_ctzll(m);
    m &= m - 1;
    if (m) {                                                                // two accumulator chains
      const int T1 = __builtin_ctzll(m);
      m &= m - 1;
      f32x4 d0 = binit, d1 = binit;
      mm(MtAcc{a_of_tile(T0), d0}, MtAcc{a_of_tile(T1), d1});
      finish(d0, T0);
      finish(d1, T1);
    } else run1(T0);
  }
  TSG_STAMP(2);
}

// ---- conv1 -> conv2 fused: the 5.2 GB pooled conv1 activation never exists -----------------------------------------
// One 1024-thread workgroup walks ONE image top to bottom in 20 steps of F12_TH = 10 conv2 rows.  Per step:
//   phase A (all threads, VALU + LDS): the table form of conv1 (see k_conv1_lut) for the 10 NEW rows of p1 = pool(relu(
//            bn(conv1))) - a thread owns two adjacent p1 pixels, 1000 of the 1024 threads busy - written straight into
//            the planar LDS tile the GEMM reads (rows R0 - 1 .. R0 + 10 of p1, zero outside the image);
//   phase B (MFMA): conv2 as k_convm's banded GEMM on that tile, M-tiles of 16 pixels enumerated FLAT over the 5 row
//            pairs x 200 columns (62.5 M-tiles: no masked columns), 4 per wave as four accumulator chains; the global loads of
//            the next step's bit rows are in flight meanwhile;
//            (the step's last two p1 rows are also kept aside: they are the first two tile rows of the next step).
// Separating the phases in time costs little as long as each phase has its four waves per SIMD busy; one workgroup per CU.
// (r03: a form with two half-workgroups in anti-phase, 8 table waves beside 8 GEMM waves on two images, took 3.19 ms
// against 2.83 ms - measured on the chip and removed again, DESIGN.md section 3.  MFMA and VALU instructions share one
// issue port per SIMD and a matrix wave with MFMAs queued starves the vector instructions of the waves beside it
// (tools/ubench_coexec.hip, fixed-window form); the table phase is also one chain of LDS latencies of ~8 400 cycles
// per WAVE whatever the number of waves, so halving the table waves halves the table throughput.)
// Output = k_convm's: planar [img][8][100][100].
constexpr int F12_TH = 10, F12_LS = 216, F12_ROWS = F12_TH + 2;
constexpr int F12_PLS = (F12_ROWS * F12_LS + 63) / 64 * 64 + 16;  // plane stride = 16 mod 64, as k_convm
constexpr int F12_WR = 14, F12_BR = 2 * (F12_TH + 1) + 2;         // words per staged bit row; bit rows of the first step
constexpr int F12_THREADS = 1024;
constexpr int C3_MW = 4;                                          // words of a p2 row's marks (100 bits): ConvParams::marks
static_assert(F12_PLS % 64 == 16 && F12_PLS % 4 == 0 && F12_LS % 4 == 0, "tile layout");
static_assert(2 * F12_BR * F12_WR <= F12_THREADS, "one staged word per thread");
static_assert((F12_TH + 1) * 100 <= 2 * F12_THREADS && F12_TH * 100 <= F12_THREADS, "pixel pairs per step");

// SPARSE (OFX_OPT_TRUNK_SPARSE: exact, the default): the two input planes are ~1 % set bits (lib/observation.py:79-95), so
// most of conv1's output is ONE value per channel - K1[c] = relu(bn(conv1(empty window))), table pattern 0 - and most
// of conv2's M-tiles multiply that constant.  Exact: a wave whose 64 pixel pairs all see empty 4 x 6 bit windows writes
// K1 instead of reading its 16 table rows per pixel (the same sum of the same two table entries), every other pixel
// pair marks its two columns in a per-row bit map, and the GEMM phase skips M-tiles whose whole window is unmarked and
// away from the padding (ts_gemm_phase_sparse).  Bit-identical to the dense kernel (tests/test_gpu_policy.py).
template <int LP, bool SPARSE = false>
__global__ __launch_bounds__(F12_THREADS) void k_trunk12(ConvParams p, const float *lut) {
  constexpr bool BF16 = LP != 0;
  constexpr int W = PS, H = PS, H1 = PS / 2, H2 = PS / 4, LS = F12_LS, PLS = F12_PLS, NK = 24;
  __shared__ __align__(16) float slut[2 * 512 * 8];
  __shared__ __align__(16) float tile[8 * F12_PLS];
  __shared__ unsigned rows[2][2][F12_BR][F12_WR];  // [buffer][channel][bit row][word]
  __shared__ __align__(16) float halo[2][8][2][F12_LS];  // the last two p1 rows of a step = the first two of the next
  __shared__ unsigned nz[SPARSE ? 2 : 1][F12_ROWS][8];   // SPARSE: [buffer][tile row]: bit x <-> column x may differ from K1
  __shared__ __align__(16) float k1s[8], k2s[8];         // SPARSE: the constants of an empty neighbourhood
  __shared__ unsigned mk2[SPARSE ? (F12_TH / 2) * C3_MW : 1];  // SPARSE: the step's p2 marks for k_conv3_stream (ConvParams::marks)
  // SPARSE (fp32): the 24 B operands of a lane are re-read from here in every phase B instead of living in registers
  // through phase A - with them the loop spilled, and every spill reload is an s_waitcnt vmcnt(0), i.e. a wait for the bit
  // rows in flight and for the stores' acknowledgements (stamps: 3 400 of a step's 13 700 cycles in front of phase A's
  // barrier, 5 000 behind the last M-tile)
  __shared__ float wbs[(SPARSE && !BF16) ? 24 * 64 : 1];
  [[maybe_unused]] unsigned n_exec = 0, n_all = 0, t_exec = 0, t_all = 0; // SPARSE: the wave's counts (M-tiles run / all, table passes run / all; not read out by the stamps build)
#if OFX_TRUNK_STAMPS
  unsigned long long st_a = 0, st_b = 0, st_last = __builtin_amdgcn_s_memtime(), st_g[3] = {0, 0, 0};
#define T12_STAMP(acc) do { const unsigned long long t_ = __builtin_amdgcn_s_memtime(); acc += t_ - st_last; st_last = t_; } while (0)
#else
#define T12_STAMP(acc) do { } while (0)
#endif
  const int tid = threadIdx.x, lane = tid & 63;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int n16 = lane & 15, kq = lane >> 4, co = n16 >> 1, r = n16 & 1;

  // bit rows of the p1 rows [pa, pb): image rows 2 pa - 1 .. 2 pb, re-aligned like k_conv1_lut (bit x + 1 of a staged
  // row <-> image column x; bit 0 and the bits past column W - 1 are the zero padding).  One word per thread.
  auto bits_fetch = [&](int img, int pa, int pb) -> unsigned {
    const int nrows = 2 * (pb - pa) + 2;
    unsigned out = 0u;
    if (tid < 2 * nrows * F12_WR) {
      const int w = tid % F12_WR, rr = (tid / F12_WR) % nrows, ci = tid / (F12_WR * nrows);
      const int gy = 2 * pa - 1 + rr;
      if (gy >= 0 && gy < H) {
        const long long s0 = (long long)gy * W + 32 * w - 1;      // cell of output bit 0 (-1 only for gy = 0, w = 0)
        const unsigned *bits = p.bits[ci] + (size_t)img * p.bits_stride;
        const long long sw = s0 >> 5;                             // arithmetic shift: -1 -> word -1
        const unsigned lo = (sw >= 0 && sw < (PS * PS) >> 5) ? bits[sw] : 0u;
        const unsigned hi = (sw + 1 < (PS * PS) >> 5) ? bits[sw + 1] : 0u;
        out = __funnelshift_r(lo, hi, (unsigned)(s0 & 31));
        const int xlo = 32 * w - 1;
        if (xlo < 0) out &= ~1u;
        const int over = xlo + 32 - W;                            // bits past the last column
        if (over > 0) out = over >= 32 ? 0u : (out & (0xFFFFFFFFu >> over));
      }
    }
    return out;
  };
  auto bits_commit = [&](int buf, int pa, int pb, unsigned word) {
    const int nrows = 2 * (pb - pa) + 2;
    if (tid < 2 * nrows * F12_WR) {
      const int w = tid % F12_WR, rr = (tid / F12_WR) % nrows, ci = tid / (F12_WR * nrows);
      rows[buf][ci][rr][w] = word;
    }
  };

  // ---- prologue: table, weights, zeroed tile (halo columns and the row above the image stay zero), first bit rows ----
  for (int e = tid; e < 2 * 512 * 8 / 4; e += F12_THREADS)
    reinterpret_cast<f32x4 *>(slut)[e] = reinterpret_cast<const f32x4 *>(lut)[e];
  for (int e = tid; e < 8 * PLS / 4; e += F12_THREADS) reinterpret_cast<f32x4 *>(tile)[e] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int e = tid; e < 2 * 8 * 2 * LS / 4; e += F12_THREADS) reinterpret_cast<f32x4 *>(&halo[0][0][0][0])[e] = f32x4{0.f, 0.f, 0.f, 0.f};
  float bw[(BF16 || SPARSE) ? 1 : NK];
  lp_x4 bwb[6];
  if constexpr (BF16) ts_bw_lp<LP ? LP : 1>(p.wbm, n16, kq, bwb);
  else if constexpr (SPARSE) {
    for (int e = tid; e < NK * 64; e += F12_THREADS) wbs[e] = p.wbm[e];
  } else {
#pragma unroll
    for (int j = 0; j < NK; j++) bw[j] = p.wbm[j * 64 + lane];   // per-lane B operand of k_convm (PrepLayout::wbm)
  }
  const float bias = p.b[co];
  const f32x4 binit = {bias, bias, bias, bias};
  const float *abase = &tile[kq * PLS + 3];
  if constexpr (SPARSE) {
    // K1: the table form's value for pattern 0 in both channels (the max of four equal sums and 0); K2: conv2 + pool + ReLU
    // of a window of K1 planes, through the kernel's own MFMA sequence on a tile filled with them
    __syncthreads();                                               // slut stands
    if (tid < 8) k1s[tid] = fmaxf(slut[tid] + slut[512 * 8 + tid], 0.f);
    for (int e = tid; e < 2 * F12_ROWS * 8; e += F12_THREADS) (&nz[0][0][0])[e] = 0u;
    __syncthreads();
    for (int e = tid; e < 8 * PLS; e += F12_THREADS) tile[e] = k1s[min(e / PLS, 7)];
    __syncthreads();
    if (wv == 0) {
      // any interior M-tile: row pair 1, columns 16 .. 31; fp32: the lane's B operands straight out of wbs [24][64]
      const float q0 = mt_const<LP, LS, PLS, 64>(abase + 2 * LS + 16 + n16, wbs + lane, bwb, kq, binit);
      if (r == 0 && kq == 0) {
        k2s[co] = q0;
        if (blockIdx.x == 0 && p.k2) p.k2[co] = q0;               // for k_conv3_stream<., true>: every workgroup has the same bits
      }
    }
    __syncthreads();
    for (int e = tid; e < 8 * PLS / 4; e += F12_THREADS) reinterpret_cast<f32x4 *>(tile)[e] = f32x4{0.f, 0.f, 0.f, 0.f};
  }
  bits_commit(0, 0, F12_TH + 1, bits_fetch((int)blockIdx.x, 0, F12_TH + 1));
  unsigned w_ahead = 0u;                                // SPARSE: the bit rows of the step after next, in flight
  if constexpr (SPARSE) { if ((int)blockIdx.x < p.images) w_ahead = bits_fetch((int)blockIdx.x, F12_TH + 1, 2 * F12_TH + 1); }
  __syncthreads();
  const float k2 = SPARSE ? k2s[co] : 0.f;

  // persistent: a workgroup takes images blockIdx.x, blockIdx.x + gridDim.x, ... (table, weights and the zero frame of
  // the tile are set up once; the first bit rows of the next image are fetched under the last step of this one)
#pragma unroll 1
  for (int img = (int)blockIdx.x; img < p.images; img += (int)gridDim.x)
#pragma unroll 1
  for (int step = 0; step < H1 / F12_TH; step++) {
    const int R0 = step * F12_TH;                                  // first conv2 row of the step
    // new p1 rows [pa, pb) -> tile rows pa - (R0 - 1) ..; the first step also makes row 0 (its row -1 is the zero row),
    // the last one leaves row 200 zero
    const int pa = step ? R0 + 1 : 0, pb = min(R0 + F12_TH + 1, H1);
    const int buf = step & 1;
    // the next step's bit rows (of the workgroup's next image behind the last step)
    const bool last = step + 1 == H1 / F12_TH;
    const int nimg = last ? img + (int)gridDim.x : img;
    const bool more = nimg < p.images;
    const int na = last ? 0 : R0 + F12_TH + 1, nb = last ? F12_TH + 1 : min(R0 + 2 * F12_TH + 1, H1);
    unsigned nextw = 0u;
    T12_STAMP(st_b);
    // ---- phase A: conv1 table look-up + pool + ReLU, two adjacent p1 pixels per thread ----
    if (step && pb - pa < F12_TH)  // last step: p1 row 200 does not exist - the tile row behind the image is zero
      for (int e = tid; e < 8 * LS; e += F12_THREADS) tile[(e / LS) * PLS + (F12_TH + 1) * LS + e % LS] = 0.f;
    if (!step)  // the row above the image
      for (int e = tid; e < 8 * LS; e += F12_THREADS) tile[(e / LS) * PLS + e % LS] = 0.f;
    if (step && tid < 8 * 2 * (LS / 4)) {  // rows R0 - 1, R0: kept by the previous step (nobody reads the tile in phase A)
      const int c4 = tid % (LS / 4), rr = (tid / (LS / 4)) & 1, ci = tid / (2 * (LS / 4));
      reinterpret_cast<f32x4 *>(&tile[ci * PLS + rr * LS])[c4] = reinterpret_cast<const f32x4 *>(&halo[buf][ci][rr][0])[c4];
    }
    if constexpr (SPARSE) {  // ... and their column marks (the rows this step writes start at tile row 2: no overlap)
      if (step && tid < 16) nz[buf][tid >> 3][tid & 7] = nz[buf ^ 1][F12_TH + (tid >> 3)][tid & 7];
    }
    for (int q = tid; q < (pb - pa) * 100; q += F12_THREADS) {
      const int py = q / 100, pp = q - py * 100;
      const int x0 = 4 * pp;                                       // window = staged bits x0 .. x0 + 5 of rows 2 py .. 2 py + 3
      unsigned f[2][4];
#pragma unroll
      for (int ci = 0; ci < 2; ci++)
#pragma unroll
        for (int rr = 0; rr < 4; rr++) f[ci][rr] = c1_window<6>(rows[buf][ci][2 * py + rr], x0);
      float m2[8][2];
      bool dense_pass = true;
      if constexpr (SPARSE) {
        const unsigned any = (f[0][0] | f[0][1] | f[0][2] | f[0][3]) | (f[1][0] | f[1][1] | f[1][2] | f[1][3]);
        dense_pass = __builtin_amdgcn_ballot_w64(any != 0u) != 0;  // wave-uniform
        t_all++;
        if (dense_pass) {
          t_exec++;
          if (any != 0u) atomicOr(&nz[buf][pa + py - (R0 - 1)][(2 * pp) >> 5], 3u << ((2 * pp) & 31));  // columns 2 pp, 2 pp + 1: an even bit and its neighbour
        } else {
          const f32x4 ka = *reinterpret_cast<const f32x4 *>(&k1s[0]), kb = *reinterpret_cast<const f32x4 *>(&k1s[4]);
#pragma unroll
          for (int c = 0; c < 8; c++) m2[c][0] = m2[c][1] = c < 4 ? ka[c & 3] : kb[c & 3];
        }
      }
      if (dense_pass) {
#pragma unroll
      for (int j = 0; j < 2; j++) {
        f32x4 acc[4][2];                                           // [2x2 pixel][channels 0-3 | 4-7]
#pragma unroll
        for (int ci = 0; ci < 2; ci++)
#pragma unroll
          for (int qq = 0; qq < 4; qq++) {
            const int dy = qq >> 1, sh = 2 * j + (qq & 1);
            const unsigned pat = ((f[ci][dy] >> sh) & 7u) | (((f[ci][dy + 1] >> sh) & 7u) << 3) | (((f[ci][dy + 2] >> sh) & 7u) << 6);
            const f32x4 *e = reinterpret_cast<const f32x4 *>(&slut[(ci * 512 + pat) * 8]);
            if (ci == 0) { acc[qq][0] = e[0]; acc[qq][1] = e[1]; }  // the table of channel 0 carries the bias
            else { acc[qq][0] += e[0]; acc[qq][1] += e[1]; }
          }
#pragma unroll
        for (int c = 0; c < 8; c++) {
          float m;  // the operands are ordinary VALU results (interlocked), not MFMA results: asm is safe here
          asm("v_max3_f32 %0, %1, %2, 0" : "=v"(m) : "v"(acc[0][c >> 2][c & 3]), "v"(acc[1][c >> 2][c & 3]));
          asm("v_max3_f32 %0, %1, %2, %3" : "=v"(m) : "v"(acc[2][c >> 2][c & 3]), "v"(acc[3][c >> 2][c & 3]), "v"(m));
          m2[c][j] = m;
        }
      }
      }  // dense_pass
      const int trow = pa + py - (R0 - 1);
      float *dst = &tile[trow * LS + 4 + 2 * pp];
#pragma unroll
      for (int c = 0; c < 8; c++) *reinterpret_cast<float2 *>(dst + c * PLS) = make_float2(m2[c][0], m2[c][1]);
      if (trow >= F12_TH) {  // also the next step's first two rows
#pragma unroll
        for (int c = 0; c < 8; c++)
          *reinterpret_cast<float2 *>(&halo[buf ^ 1][c][trow - F12_TH][4 + 2 * pp]) = make_float2(m2[c][0], m2[c][1]);
      }
    }
    __syncthreads();

    T12_STAMP(st_a);
    // ---- phase B: conv2 on the tile; the next step's bit rows are fetched meanwhile ----
    if constexpr (!SPARSE) { if (more) nextw = bits_fetch(nimg, na, nb); }
    // SPARSE: the bit rows travel TWO steps ahead.  The dense GEMM phase hides the ~2 us of a fetch issued at its start;
    // the sparse step is over before the word lands.  Here, BETWEEN the two phases, the word fetched a whole step ago is
    // committed (the next step's rows) and the step after that is requested: the wait for the word is a vmcnt(0), which
    // also waits for every p2 store in flight - at the top of the step those are the stores the previous GEMM phase has
    // just issued (stamps: 5 000 of a step's 12 700 cycles went there), behind phase A they are a table phase old.
    if constexpr (SPARSE) {
      if (more) bits_commit(buf ^ 1, na, nb, w_ahead);
      int i2 = nimg, s2 = last ? 0 : step + 1;
      if (++s2 == H1 / F12_TH) { s2 = 0; i2 += (int)gridDim.x; }
      const int r2 = s2 * F12_TH;
      w_ahead = i2 < p.images ? bits_fetch(i2, s2 ? r2 + 1 : 0, min(r2 + F12_TH + 1, H1)) : 0u;
    }

    if constexpr (SPARSE) {
      float bwl[BF16 ? 1 : NK];
      if constexpr (!BF16) {
        int zoff;                                   // an offset the compiler cannot see through: the reads stay in the loop
        asm volatile("s_mov_b32 %0, 0" : "=s"(zoff));
#pragma unroll
        for (int j = 0; j < NK; j++) bwl[j] = wbs[j * 64 + lane + zoff];
      }
      ts_gemm_phase_sparse<200, F12_TH / 2, F12_LS, F12_PLS, LP>(abase, bwl, bwb, binit, wv, lane, n16, kq, r,
                                                                  p.out + (((size_t)img * 8 + co) * H2 + (R0 >> 1)) * H2,
                                                                  &nz[buf][0][0], k2, step == 0, last, n_exec, n_all, mk2
#if OFX_TRUNK_STAMPS
                                                                  , st_g
#endif
                                                                  );
      // the other buffer's marks are last step's: cleared for the next step (its first two rows are copied in there)
      for (int e = tid; e < F12_ROWS * 8; e += F12_THREADS) (&nz[buf ^ 1][0][0])[e] = 0u;
    } else
      ts_gemm_phase<200, F12_TH / 2, F12_LS, F12_PLS, LP>(abase, bw, bwb, binit, wv, n16, kq, r,
                                                           p.out + (((size_t)img * 8 + co) * H2 + (R0 >> 1)) * H2);
    if constexpr (!SPARSE) { if (more) bits_commit(buf ^ 1, na, nb, nextw); }  // the other buffer: phase A of this step is behind every wave
    __syncthreads();
    // the step's p2 marks: 5 rows x 4 words, one plain store (the next GEMM phase, which rewrites mk2, is a barrier away)
    if constexpr (SPARSE) { if (tid < (F12_TH / 2) * C3_MW) p.marks[((size_t)img * H2 + (R0 >> 1)) * C3_MW + tid] = mk2[tid]; }
  }
  if constexpr (SPARSE) {
#if OFX_TRUNK_STAMPS
    T12_STAMP(st_b);
    if (p.stat && tid == 0) {   // diagnostic: cycles of wave 0 in phase A (up to its barrier) / phase B / whole kernel / blocks
      atomicAdd(&p.stat[0], st_a); atomicAdd(&p.stat[1], st_b);          // phase A (with its barrier) / the rest of the step
      atomicAdd(&p.stat[2], st_g[0]); atomicAdd(&p.stat[3], st_g[2]);    // of that: classification + constant stores / the run tiles
    }
#else
    if (p.stat && lane == 0) {
      atomicAdd(&p.stat[0], (unsigned long long)n_exec); atomicAdd(&p.stat[1], (unsigned long long)n_all);
      atomicAdd(&p.stat[2], (unsigned long long)t_exec); atomicAdd(&p.stat[3], (unsigned long long)t_all);
    }
#endif
  }
}

// ---- conv3 as a streaming kernel: k_trunk12's GEMM phase on tiles that arrive by LDS-direct loads --------------------
// Planar f32 input [img][8][100][100] -> planar [img][8][50][50].  One persistent 1024-thread workgroup per CU walks an
// image in 5 steps of 20 rows over TWO tiles (8 planes x 22 rows x 108 floats each, 157 KB): while the GEMM phase
// (ts_gemm_phase: 10 row pairs x 100 columns = 62.5 M-tiles, four chains per wave) runs on one, the 22 rows of the next
// step land in the other by global_load_lds_dwordx4 - no staging registers (a register prefetch of 20 rows spills next
// to four accumulator chains), no LDS store instructions.  An LDS-direct load writes lane l's 16 bytes at base + 16 l, so a
// plane is filled front to back in pieces of 64 float4: lane q of a plane -> (row q / 27, float4 q % 27); float4 0 and
// 26 of a row (the halo columns) and the rows outside the image read 16 zero bytes instead (PrepLayout::zero16).
constexpr int C3_W = 100, C3_TH = 20, C3_LS = 108, C3_ROWS = C3_TH + 2, C3_F4 = C3_LS / 4;
constexpr int C3_PLS = (C3_ROWS * C3_LS + 63) / 64 * 64 + 16;
constexpr int C3_PF4 = C3_ROWS * C3_F4, C3_NI = (C3_PF4 + 63) / 64;  // float4 of a plane, wave-instructions per plane
static_assert(C3_PLS % 64 == 16 && C3_W % C3_TH == 0 && C3_W / 4 + 2 == C3_F4 && 64 * C3_NI * 4 <= C3_PLS + 64 * 4, "tile layout");
static_assert(2 * 8 * C3_PLS * 4 <= 160 * 1024, "two tiles in LDS");

//
// SPARSE (exact; runs exactly when k_trunk12<., true> made this launch's p2): most of p2 is conv2's constant K2[ci], and
// k_trunk12 leaves a bit map of the pixels that may differ from it (ConvParams::marks, from the run mask of its own GEMM
// phase) and K2 itself (ConvParams::k2).  The marks of a step's 22 tile rows arrive with the tile - LDS-direct, 4 bytes
// per lane, rows of 8 words of which 4 are zeros: the nz array of ts_gemm_phase_sparse - and an M-tile whose 4 x 18
// window is unmarked and off the zero padding stores K3[co] instead of running: K3 = this kernel's own matrix sequence
// (the 16-bit one for LP != 0) on a tile of K2 planes, pooled, once per workgroup.  Bit-identical to the dense form.
template <int LP, bool SPARSE = false>
__global__ __launch_bounds__(F12_THREADS) void k_conv3_stream(ConvParams p, const float *zero16) {
  constexpr bool BF16 = LP != 0;
  constexpr int W = C3_W, H = C3_W, H2 = C3_W / 2, PLS = C3_PLS, NK = 24, STEPS = H / C3_TH;
  __shared__ __align__(16) float tiles[2][8 * C3_PLS];
  __shared__ __align__(16) unsigned nzs[SPARSE ? 2 : 1][SPARSE ? C3_ROWS : 1][8];  // SPARSE: [buffer][tile row]: bit x <-> column x may differ from K2
  __shared__ float k3s[8];
  static_assert((2 * 8 * C3_PLS + 2 * C3_ROWS * 8 + 8) * 4 <= 160 * 1024, "tiles, marks and K3 in LDS");
  unsigned n_exec = 0, n_all = 0;                        // SPARSE: wave 0's counts of M-tiles run / all
  const int tid = threadIdx.x, lane = tid & 63;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int n16 = lane & 15, kq = lane >> 4, co = n16 >> 1, r = n16 & 1;

  // rows R0 - 1 .. R0 + C3_TH of image img -> tiles[buf]; 80 wave-instructions spread over the 16 waves
  auto stage = [&](int buf, int img, int R0) {
#pragma unroll 1
    for (int i = wv; i < 8 * C3_NI; i += F12_THREADS / 64) {
      const int ci = i / C3_NI, k = i - ci * C3_NI;
      const int q = 64 * k + lane;
      if (q < C3_PF4) {
        const int row = q / C3_F4, c4 = q - row * C3_F4, gy = R0 - 1 + row;
        const float *src = zero16;
        if (c4 >= 1 && c4 <= W / 4 && gy >= 0 && gy < H) src = p.in + (((size_t)img * 8 + ci) * H + gy) * W + 4 * (c4 - 1);
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)src,
                                         (__attribute__((address_space(3))) void *)&tiles[buf][ci * PLS + 256 * k], 16, 0, 0);
      }
    }
    if constexpr (SPARSE) {  // the marks of the same 22 rows: word q -> (row q / 8, word q % 8), three wave-instructions
      constexpr int NM = (C3_ROWS * 8 + 63) / 64;
      const int k = F12_THREADS / 64 - 1 - wv;             // the last waves take them
      const int q = 64 * k + lane;
      if (k < NM && q < C3_ROWS * 8) {
        const int row = q >> 3, w = q & 7, gy = R0 - 1 + row;
        const unsigned *src = reinterpret_cast<const unsigned *>(zero16);
        if (w < C3_MW && gy >= 0 && gy < H) src = p.marks + ((size_t)img * H + gy) * C3_MW + w;
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)src,
                                         (__attribute__((address_space(3))) void *)(&nzs[buf][0][0] + 64 * k), 4, 0, 0);
      }
    }
  };

  float bw[BF16 ? 1 : NK];
  lp_x4 bwb[6];
  if constexpr (BF16) ts_bw_lp<LP ? LP : 1>(p.wbm, n16, kq, bwb);
  else {
#pragma unroll
    for (int j = 0; j < NK; j++) bw[j] = p.wbm[j * 64 + lane];
  }
  const float bias = p.b[co];
  const f32x4 binit = {bias, bias, bias, bias};
  if ((int)blockIdx.x < p.images) stage(0, (int)blockIdx.x, 0);
  if constexpr (SPARSE) {
    // K3 while the first tile is in flight: the first four rows of the OTHER tile's planes hold K2 (read from where
    // k_trunk12 left it), wave 0 runs the M-tile at row pair 0, columns 16 .. 31 on them
    for (int e = tid; e < 8 * 4 * C3_LS; e += F12_THREADS) tiles[1][(e / (4 * C3_LS)) * PLS + e % (4 * C3_LS)] = p.k2[e / (4 * C3_LS)];
    __syncthreads();
    if (wv == 0) {
      const float q0 = mt_const<LP, C3_LS, C3_PLS>(&tiles[1][kq * PLS + 3] + 16 + n16, bw, bwb, kq, binit);
      if (r == 0 && kq == 0) k3s[co] = q0;
    }
  }
  // the LDS-direct loads are published to the other waves by vmcnt(0) BEFORE the barrier: the memory model only
  // promises lgkmcnt(0) at a workgroup fence, so the wait is written out rather than left to the compiler
  __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0)
  __syncthreads();
  const float k3 = SPARSE ? k3s[co] : 0.f;
  int buf = 0;
#pragma unroll 1
  for (int img = (int)blockIdx.x; img < p.images; img += (int)gridDim.x)
#pragma unroll 1
  for (int step = 0; step < STEPS; step++) {
    const int R0 = step * C3_TH;
    const bool last = step + 1 == STEPS;
    const int nimg = last ? img + (int)gridDim.x : img;
    if (nimg < p.images) stage(buf ^ 1, nimg, last ? 0 : R0 + C3_TH);
    if constexpr (SPARSE) {
#if OFX_TRUNK_STAMPS
      unsigned long long st_g[3] = {0, 0, 0};
#endif
      ts_gemm_phase_sparse<W, C3_TH / 2, C3_LS, C3_PLS, LP>(&tiles[buf][kq * PLS + 3], bw, bwb, binit, wv, lane, n16, kq, r,
                                                            p.out + (((size_t)img * 8 + co) * H2 + (R0 >> 1)) * H2,
                                                            &nzs[buf][0][0], k3, step == 0, last, n_exec, n_all, nullptr
#if OFX_TRUNK_STAMPS
                                                            , st_g
#endif
                                                            );
    } else
      ts_gemm_phase<W, C3_TH / 2, C3_LS, C3_PLS, LP>(&tiles[buf][kq * PLS + 3], bw, bwb, binit, wv, n16, kq, r,
                                                     p.out + (((size_t)img * 8 + co) * H2 + (R0 >> 1)) * H2);
    __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0): the next tile's LDS-direct loads have landed (see above)
    __syncthreads();
    buf ^= 1;
  }
  if constexpr (SPARSE) {
#if !OFX_TRUNK_STAMPS
    if (p.stat && tid == 0) { atomicAdd(&p.stat[4], (unsigned long long)n_exec); atomicAdd(&p.stat[5], (unsigned long long)n_all); }
#endif
  }
}

// ---- launchers -----------------------------------------------------------------------
// conv1 -> conv2 fused (k_trunk12, one persistent workgroup per CU) once the images fill the CUs a few times over;
// below that the two-kernel form has the shorter critical path (OFX_OPT_TRUNK_FUSE: 1 always, 2 never)
bool ofx_trunk_fused(const ofx_handle *h, size_t N) {
  if (h->opt_trunk_plain) return false;
  return h->opt_trunk_fuse == 1 || (h->opt_trunk_fuse == 0 && N >= 4 * (size_t)h->n_cus);
}

template <int CIN, int COUT, int TH, int TW, int MODE, bool POOL, bool OUT_HWC>
static int launch_conv(ofx_handle *h, ConvParams p, int images, int H) {
  p.H = H; p.W = H;
  p.tiles_x = H / TW;
  p.tiles = p.tiles_x * (H / TH);
  constexpr int NTB = ((TH / 2) * (TW / 2) + 63) / 64 * 64;
  hipLaunchKernelGGL((k_conv<CIN, COUT, TH, TW, MODE, POOL, OUT_HWC>), dim3((unsigned)(images * p.tiles)), dim3(NTB), 0,
                     h->stream, p);
  OFX_HIP(hipGetLastError());
  return OFX_OK;
}

static int launch_conv1_lut(ofx_handle *h, ConvParams cp, const float *lut) {
  cp.H = PS; cp.W = PS;
  hipLaunchKernelGGL(k_conv1_lut<40>, dim3((unsigned)(cp.images * (PS / 40))), dim3(256), 0, h->stream, cp, lut);
  OFX_HIP(hipGetLastError());
  return OFX_OK;
}

int ofx_launch_conv1_lut(ofx_handle *h, const void *bits, int n, const float *lut, float *out) {  // ofx_trunk.h
  ConvParams cp{};
  cp.bits[0] = reinterpret_cast<const unsigned *>(bits);
  cp.bits[1] = cp.bits[0] + (PS * PS) / 32;
  cp.bits_stride = 2 * (size_t)((PS * PS) / 32);
  cp.out = out; cp.images = n;
  return launch_conv1_lut(h, cp, lut);
}

// the kernels' argument for layer i (0-based): conv(in) -> out with the layer's folded weights
static void trunk_layer(ConvParams &cp, const TrunkParams &p, int i, const float *in, float *out) {
  cp.in = in; cp.w = p.tw[i]; cp.b = p.tb[i]; cp.out = out;
  if (i > 0) cp.wbm = p.wbm[i - 1];
}

// large batches: conv1 -> conv2 fused and conv3 streaming, one persistent workgroup per CU; LP = the operand format
template <int LP>
static int trunk_streaming(ofx_handle *h, ConvParams cp, const TrunkParams &p) {
  const dim3 grid((unsigned)(p.images < h->n_cus ? p.images : h->n_cus));
  cp.w = p.tw[0]; cp.b = p.tb[1]; cp.out = p.p2; cp.wbm = p.wbm[0]; cp.stat = p.stat;
  if (p.sparse && !(p.nz2 && p.k2)) { ofx_set_error("trunk_streaming: the sparse form needs the marks buffer"); return OFX_ERR_STATE; }
  cp.marks = p.nz2; cp.k2 = p.k2;
  if (p.sparse) hipLaunchKernelGGL((k_trunk12<LP, true>), grid, dim3(F12_THREADS), 0, h->stream, cp, p.lut1);
  else hipLaunchKernelGGL((k_trunk12<LP, false>), grid, dim3(F12_THREADS), 0, h->stream, cp, p.lut1);
  OFX_HIP(hipGetLastError());
  trunk_layer(cp, p, 2, p.p2, p.p3);
  // the sparse conv3 reads the marks and K2 the sparse k_trunk12 has just written for these very images; the dense pair otherwise
  if (p.sparse) hipLaunchKernelGGL((k_conv3_stream<LP, true>), grid, dim3(F12_THREADS), 0, h->stream, cp, p.zero16);
  else hipLaunchKernelGGL((k_conv3_stream<LP, false>), grid, dim3(F12_THREADS), 0, h->stream, cp, p.zero16);
  OFX_HIP(hipGetLastError());
  trunk_layer(cp, p, 3, p.p3, p.p4);
  return launch_convm<10, 4, true, 1, LP>(h, cp, p.images, 50);
}

int ofx_launch_trunk(ofx_handle *h, const TrunkParams &p) {
  ConvParams cp{};
  cp.bits[0] = p.bits[0]; cp.bits[1] = p.bits[1]; cp.bits_stride = p.bits_stride; cp.images = p.images;
  const bool plain = h->opt_trunk_plain;  // OFX_OPT_TRUNK_PLAIN: every layer through the plain VALU kernel
  if (ofx_trunk_fused(h, (size_t)p.images))
    return p.lowp == 1 ? trunk_streaming<1>(h, cp, p) : p.lowp == 2 ? trunk_streaming<2>(h, cp, p) : trunk_streaming<0>(h, cp, p);
  // small batches: one kernel per layer, fp32.  k_convm tile shapes from an A/B on the chip (conv2: 2 row pairs x 208
  // columns, 29 KB of LDS, five workgroups per CU)
  const int N = p.images;
  int rc;
  trunk_layer(cp, p, 0, nullptr, p.p1);
  if ((rc = plain ? launch_conv<2, 8, 10, 100, 1, true, false>(h, cp, N, 400) : launch_conv1_lut(h, cp, p.lut1))) return rc;
  trunk_layer(cp, p, 1, p.p1, p.p2);
  if ((rc = plain ? launch_conv<8, 8, 10, 100, 0, true, false>(h, cp, N, 200) : launch_convm<2, 13, false, 1>(h, cp, N, 200))) return rc;
  trunk_layer(cp, p, 2, p.p2, p.p3);
  if ((rc = plain ? launch_conv<8, 8, 10, 100, 0, true, false>(h, cp, N, 100) : launch_convm<4, 7, false, 1>(h, cp, N, 100))) return rc;
  trunk_layer(cp, p, 3, p.p3, p.p4);  // writes (h,w,c) = Flatten order
  return plain ? launch_conv<8, 8, 10, 50, 0, true, true>(h, cp, N, 50) : launch_convm<10, 4, true, 1>(h, cp, N, 50);
}

// the sparse form's counters (ConvParams::stat): slots first .. first + count - 1 read into dst and reset; dst stays as it
// is when the handle has none
static int trunk_stat_take(ofx_handle *h, int first, int count, void *dst) {
  if (!h->trunk_stat) return OFX_OK;
  OFX_HIP(hipSetDevice(h->cfg.device));
  OFX_HIP(hipMemcpyAsync(dst, h->trunk_stat + first, count * sizeof(unsigned long long), hipMemcpyDeviceToHost, h->stream));
  OFX_HIP(hipMemsetAsync(h->trunk_stat + first, 0, count * sizeof(unsigned long long), h->stream));
  OFX_HIP(hipStreamSynchronize(h->stream));
  return OFX_OK;
}

extern "C" int ofx_policy_trunk_stats(ofx_handle *h, int64_t *counts_host) {
  if (!h || !counts_host) { ofx_set_error("ofx_policy_trunk_stats: null argument"); return OFX_ERR_INVALID; }
  for (int i = 0; i < 4; i++) counts_host[i] = 0;
  return trunk_stat_take(h, 0, 4, counts_host);
}

// conv3's M-tiles (k_conv3_stream<., true>): slots 4 and 5 of the same counters, read and reset on their own
extern "C" int ofx_policy_trunk_stats3(ofx_handle *h, int64_t *run_host, int64_t *total_host) {
  if (!h || !run_host || !total_host) { ofx_set_error("ofx_policy_trunk_stats3: null argument"); return OFX_ERR_INVALID; }
  int64_t v[2] = {0, 0};
  const int rc = trunk_stat_take(h, 4, 2, v);
  *run_host = v[0]; *total_host = v[1];
  return rc;
}

// the trunk's output of the last forward of n_images images x m ships on this handle: p4 [n_images][5000] in (h, w, c) order,
// read out of the forward's workspace (same sizes -> same layout; valid until the next user of the scratch block)
extern "C" int ofx_policy_trunk_features(ofx_handle *h, int32_t n_images, int32_t m, float *out_host) {
  if (!h || !out_host || n_images <= 0 || m <= 0) { ofx_set_error("ofx_policy_trunk_features: bad argument"); return OFX_ERR_INVALID; }
  const float *p4 = ofx_policy_ws_p4(h, (size_t)n_images, (size_t)n_images * (size_t)m);
  if (!p4) { ofx_set_error("ofx_policy_trunk_features: no forward of these sizes has run"); return OFX_ERR_STATE; }
  OFX_HIP(hipSetDevice(h->cfg.device));
  OFX_HIP(hipMemcpyAsync(out_host, p4, (size_t)n_images * 5000 * sizeof(float), hipMemcpyDeviceToHost, h->stream));
  OFX_HIP(hipStreamSynchronize(h->stream));
  return OFX_OK;
}
