// ofx_train.hip - one DQN fit step of the bi-head pointer_model: the model.fit call of
// Trainer.replay (agents/qlearnIA_V2.py:284; model.compile(loss='mse', optimizer=Adam(lr)) :190).
//
// Two forms of the same step.  The default is the LEAN form (dqn_fit_lean below + the kernels of ofx_fit.hip): only the
// pre-activation tensor of every convolution is kept in HBM, the rest is recomputed inside fused tiles (9.4 MB of
// workspace per minibatch row; 4096 rows in 42 ms, 65 ms with the reference's dense targets).  The PLAIN form (OFX_OPT_FIT_PLAIN, dqn_fit_impl) is the layer-by-layer
// original - one fp32 VALU kernel per layer and pass, every tensor of the graph in HBM (37 MB per row) - kept as the
// reference of the lean form.  Both: fixed-order reductions (no atomics: a fit is reproducible to the bit), the dense
// forwards on the f32 MFMA GEMM of the forward, every gradient tensor checked against torch autograd in float64 and the
// two forms against each other (tests/test_train.py).  Keras semantics assumed (parity unpinned: no keras in the image):
//   * fit runs the graph in training mode: BatchNorm normalises with the batch mean / biased variance (eps 1e-3) and
//     moves the stored statistics: moving = 0.99 moving + 0.01 batch;
//   * loss = mse(output1) + mse(output2), each the mean over the batch and the output elements;
//   * the targets equal the current predictions except target[iaction] = y_act and ptr_target[pointer] = y_ptr
//     (qlearnIA_V2.py:279-280), i.e. one non-zero error per head and sample.  The pointer addresses heat[y][x] and
//     the inputs are the transitions' `state` observations (the reference's [x][y] indexing and its use of
//     next_state as input, :280-283, are stated in include/ofx.h, not reproduced);
//   * Adam: beta1 0.9, beta2 0.999, eps 1e-7, bias-corrected step size.
#include "ofx_internal.h"
#include "ofx_arena.h"
#include "ofx_blob.h"
#include "ofx_fit.h"
#include <float.h>
#include <string.h>

#define TPS 400

// ---------------------------------------------------------------- elementwise / layout kernels
__global__ void t_bits_to_f32(int n, const uint32_t *bits, float *x) {  // bits [n][2][5000] -> x [n][2][400][400]
  const size_t total = (size_t)n * 2 * TPS * TPS;
  for (size_t e = blockIdx.x * (size_t)blockDim.x + threadIdx.x; e < total; e += (size_t)gridDim.x * blockDim.x) {
    const size_t img = e / (TPS * TPS), p = e - img * (TPS * TPS);
    x[e] = (float)((bits[img * ((TPS * TPS) >> 5) + (p >> 5)] >> (p & 31)) & 1u);
  }
}

// z[n][co][H][W] = conv3x3(x[n][ci][H][W], w HWIO [3][3][ci][co]) + b[co], zero padding.  One thread per PIXEL with all
// CO outputs in registers: an input value is loaded once for the CO channels (the weights are wave-uniform reads); per
// output the terms are added in the order (ci, ky, kx), one rounding per operation (-ffp-contract=off).
template <int CO>
__global__ void t_conv_fwd(int n, int ci_n, int H, int W, const float *x, const float *w, const float *b, float *z) {
  const size_t per = (size_t)H * W, total = (size_t)n * per;
  for (size_t e = blockIdx.x * (size_t)blockDim.x + threadIdx.x; e < total; e += (size_t)gridDim.x * blockDim.x) {
    const int xx = e % W, yy = (e / W) % H;
    const size_t s = e / per;
    float acc[CO];
#pragma unroll
    for (int co = 0; co < CO; co++) acc[co] = b[co];
    for (int ci = 0; ci < ci_n; ci++) {
      const float *xp = x + (s * ci_n + ci) * per;
#pragma unroll
      for (int ky = 0; ky < 3; ky++) {
        const int y = yy + ky - 1;
        if (y < 0 || y >= H) continue;
#pragma unroll
        for (int kx = 0; kx < 3; kx++) {
          const int xq = xx + kx - 1;
          if (xq < 0 || xq >= W) continue;
          const float v = xp[(size_t)y * W + xq];
          const float *wp = w + ((ky * 3 + kx) * ci_n + ci) * CO;
#pragma unroll
          for (int co = 0; co < CO; co++) acc[co] += v * wp[co];
        }
      }
    }
#pragma unroll
    for (int co = 0; co < CO; co++) z[(s * CO + co) * per + (size_t)yy * W + xx] = acc[co];
  }
}

// dx[n][ci][H][W] = sum_co conv3x3_transposed(dz[n][co], w): one thread per pixel with all CI inputs in registers
template <int CI>
__global__ void t_conv_bwd_data(int n, int co_n, int H, int W, const float *dz, const float *w, float *dx) {
  const size_t per = (size_t)H * W, total = (size_t)n * per;
  for (size_t e = blockIdx.x * (size_t)blockDim.x + threadIdx.x; e < total; e += (size_t)gridDim.x * blockDim.x) {
    const int xx = e % W, yy = (e / W) % H;
    const size_t s = e / per;
    float acc[CI];
#pragma unroll
    for (int ci = 0; ci < CI; ci++) acc[ci] = 0.f;
    for (int co = 0; co < co_n; co++) {
      const float *dp = dz + (s * co_n + co) * per;
#pragma unroll
      for (int ky = 0; ky < 3; ky++) {
        const int y = yy - (ky - 1);  // output pixel that read this input through tap ky
        if (y < 0 || y >= H) continue;
#pragma unroll
        for (int kx = 0; kx < 3; kx++) {
          const int xq = xx - (kx - 1);
          if (xq < 0 || xq >= W) continue;
          const float v = dp[(size_t)y * W + xq];
          const float *wp = w + (size_t)(ky * 3 + kx) * CI * co_n + co;
#pragma unroll
          for (int ci = 0; ci < CI; ci++) acc[ci] += v * wp[ci * co_n];
        }
      }
    }
#pragma unroll
    for (int ci = 0; ci < CI; ci++) dx[(s * CI + ci) * per + (size_t)yy * W + xx] = acc[ci];
  }
}

// dw[(ky,kx,ci,co)] = sum_{n,y,x} x[n][ci][y+ky-1][x+kx-1] dz[n][co][y][x] (double accumulators: up to 10^7 terms).
// block = a block of CIB input channels x a block of COB output channels x one of gridDim.y slices of the (n, H, W) sum:
// a pixel's input taps and output gradients are loaded once for the CIB x COB weight columns; db[co] = sum dz comes from
// the blocks of input-channel block 0.  part[slice][wid], combined in slice order by t_conv_bwd_finish.
template <int CIB, int COB>
__global__ __launch_bounds__(256) void t_conv_bwd_weight(int n, int ci_n, int co_n, int H, int W, const float *x,
                                                         const float *dz, double *part) {
  constexpr int NV = CIB * COB * 9 + COB;
  __shared__ double red[4][NV];
  const int cob = co_n / COB;                                      // co_n is a multiple of COB, ci_n of CIB
  const int co0 = (blockIdx.x % cob) * COB, ci0 = (blockIdx.x / cob) * CIB, nw = 9 * ci_n * co_n;
  const size_t per = (size_t)H * W, total = (size_t)n * per, stride = (size_t)gridDim.y * 256;
  double acc[NV];
#pragma unroll
  for (int k = 0; k < NV; k++) acc[k] = 0.0;
  for (size_t e = (size_t)blockIdx.y * 256 + threadIdx.x; e < total; e += stride) {
    const int s = e / per, yy = (e - (size_t)s * per) / W, xx = e % W;
    double g[COB];
#pragma unroll
    for (int c = 0; c < COB; c++) {
      g[c] = dz[((size_t)s * co_n + co0 + c) * per + (size_t)yy * W + xx];
      acc[CIB * COB * 9 + c] += g[c];
    }
#pragma unroll
    for (int i = 0; i < CIB; i++) {
      const float *xs = x + ((size_t)s * ci_n + ci0 + i) * per;
#pragma unroll
      for (int ky = 0; ky < 3; ky++) {
        const int y = yy + ky - 1;
        if (y < 0 || y >= H) continue;
#pragma unroll
        for (int kx = 0; kx < 3; kx++) {
          const int xq = xx + kx - 1;
          if (xq < 0 || xq >= W) continue;
          const double v = (double)xs[(size_t)y * W + xq];
#pragma unroll
          for (int c = 0; c < COB; c++) acc[(i * COB + c) * 9 + ky * 3 + kx] += v * g[c];
        }
      }
    }
  }
#pragma unroll
  for (int k = 0; k < NV; k++) {
    double v = acc[k];
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6][k] = v;
  }
  __syncthreads();
  if (threadIdx.x < NV) {
    const int k = threadIdx.x;
    const double v = red[0][k] + red[1][k] + red[2][k] + red[3][k];
    double *row = part + (size_t)blockIdx.y * (nw + co_n);
    if (k < CIB * COB * 9) {
      const int t = k % 9, ic = k / 9, i = ic / COB, c = ic % COB;
      row[(t * ci_n + ci0 + i) * co_n + co0 + c] = v;
    } else if (ci0 == 0) {
      row[nw + co0 + (k - CIB * COB * 9)] = v;
    }
  }
}

__global__ void t_conv_bwd_finish(int nw, int nb, int slices, const double *part, float *dw, float *db) {
  const int wid = blockIdx.x * blockDim.x + threadIdx.x;
  if (wid >= nw + nb) return;
  double acc = 0.0;
  for (int k = 0; k < slices; k++) acc += part[(size_t)k * (nw + nb) + wid];
  if (wid < nw) dw[wid] = (float)acc;
  else db[wid - nw] = (float)acc;
}

// per-channel sums over (n, H, W): out[c] = {sum a, sum a*b} (b may be null -> sum a*a); double accumulation,
// gridDim.y slices per channel written to part[c][slice][2] and combined IN SLICE ORDER by t_chan_sums_finish: the same
// bits every run (the fit is reproducible)
__global__ __launch_bounds__(256) void t_chan_sums(int n, int c_n, size_t per, const float *a, const float *b, double *part) {
  __shared__ double r0[256], r1[256];
  const int c = blockIdx.x;
  double s0 = 0.0, s1 = 0.0;
  for (int s = 0; s < n; s++) {                                    // the channel's plane of every sample, slice by slice
    const float *pa = a + ((size_t)s * c_n + c) * per, *pb = b ? b + ((size_t)s * c_n + c) * per : pa;
    for (size_t i = (size_t)blockIdx.y * 256 + threadIdx.x; i < per; i += (size_t)gridDim.y * 256) {
      const double va = pa[i], vb = pb[i];
      s0 += va;
      s1 += va * vb;
    }
  }
  r0[threadIdx.x] = s0; r1[threadIdx.x] = s1;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) { r0[threadIdx.x] += r0[threadIdx.x + o]; r1[threadIdx.x] += r1[threadIdx.x + o]; }
    __syncthreads();
  }
  if (threadIdx.x == 0) { part[((size_t)c * gridDim.y + blockIdx.y) * 2] = r0[0]; part[((size_t)c * gridDim.y + blockIdx.y) * 2 + 1] = r1[0]; }
}
__global__ void t_chan_sums_finish(int c_n, int slices, const double *part, double *out) {
  const int c = threadIdx.x;
  if (c >= c_n) return;
  double s0 = 0.0, s1 = 0.0;
  for (int k = 0; k < slices; k++) { s0 += part[((size_t)c * slices + k) * 2]; s1 += part[((size_t)c * slices + k) * 2 + 1]; }
  out[2 * c] = s0; out[2 * c + 1] = s1;
}

// batch statistics from the sums: mean, biased variance (stat[c] = {mean, var})
__global__ void t_bn_finish_stats(int c_n, double count, const double *sums, float *stat) {
  const int c = threadIdx.x;
  if (c >= c_n) return;
  const double m = sums[2 * c] / count, v = sums[2 * c + 1] / count - m * m;
  stat[2 * c] = (float)m;
  stat[2 * c + 1] = (float)(v > 0.0 ? v : 0.0);
}

// The three BatchNorm element-wise kernels: blockIdx.y = plane (sample s, channel c) of `per` elements - the channel is
// block-uniform, no division per element.
// a = relu(gamma * (z - mean) / sqrt(var + eps) + beta)
__global__ void t_bn_relu_fwd(int c_n, size_t per, const float *z, const float *stat, const float *gamma, const float *beta,
                              float *a) {
  const int c = blockIdx.y % c_n;
  const size_t base = (size_t)blockIdx.y * per;
  const float mean = stat[2 * c], rs = rsqrtf(stat[2 * c + 1] + 1e-3f), g = gamma[c], bt = beta[c];
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < per; i += (size_t)gridDim.x * blockDim.x) {
    const float xh = (z[base + i] - mean) * rs;
    a[base + i] = fmaxf(g * xh + bt, 0.f);
  }
}

// dy (w.r.t. the BN output, ReLU mask applied) and xhat, in place over da / into xh
__global__ void t_bn_relu_bwd_pre(int c_n, size_t per, const float *z, const float *a, const float *stat, float *da, float *xh) {
  const int c = blockIdx.y % c_n;
  const size_t base = (size_t)blockIdx.y * per;
  const float mean = stat[2 * c], rs = rsqrtf(stat[2 * c + 1] + 1e-3f);
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < per; i += (size_t)gridDim.x * blockDim.x) {
    xh[base + i] = (z[base + i] - mean) * rs;
    if (!(a[base + i] > 0.f)) da[base + i] = 0.f;
  }
}

// dz = gamma / sqrt(var+eps) * (dy - mean(dy) - xhat * mean(dy * xhat)) ; sums[c] = {sum dy, sum dy*xhat}
__global__ void t_bn_bwd(int c_n, size_t per, double count, const float *dy, const float *xh, const float *stat,
                         const float *gamma, const double *sums, float *dz, float *dgamma, float *dbeta) {
  const int c = blockIdx.y % c_n;
  const size_t base = (size_t)blockIdx.y * per;
  const float m0 = (float)(sums[2 * c] / count), m1 = (float)(sums[2 * c + 1] / count);
  const float k = gamma[c] * rsqrtf(stat[2 * c + 1] + 1e-3f);
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < per; i += (size_t)gridDim.x * blockDim.x)
    dz[base + i] = k * (dy[base + i] - m0 - xh[base + i] * m1);
  if (blockIdx.x == 0 && blockIdx.y < (unsigned)c_n && threadIdx.x == 0) {
    dbeta[blockIdx.y] = (float)sums[2 * blockIdx.y];
    dgamma[blockIdx.y] = (float)sums[2 * blockIdx.y + 1];
  }
}

__global__ void t_pool_fwd(int nc, int H, int W, const float *a, float *p) {  // [nc][H][W] -> [nc][H/2][W/2]
  const int H2 = H / 2, W2 = W / 2;
  const size_t total = (size_t)nc * H2 * W2;
  for (size_t e = blockIdx.x * (size_t)blockDim.x + threadIdx.x; e < total; e += (size_t)gridDim.x * blockDim.x) {
    const int x = e % W2, y = (e / W2) % H2;
    const size_t c = e / ((size_t)W2 * H2);
    const float *q = a + (c * H + 2 * y) * W + 2 * x;
    p[e] = fmaxf(fmaxf(q[0], q[1]), fmaxf(q[W], q[W + 1]));
  }
}

// routes dp to the first maximum of each window (row-major), zero elsewhere
__global__ void t_pool_bwd(int nc, int H, int W, const float *a, const float *dp, float *da) {
  const int H2 = H / 2, W2 = W / 2;
  const size_t total = (size_t)nc * H2 * W2;
  for (size_t e = blockIdx.x * (size_t)blockDim.x + threadIdx.x; e < total; e += (size_t)gridDim.x * blockDim.x) {
    const int x = e % W2, y = (e / W2) % H2;
    const size_t c = e / ((size_t)W2 * H2), base = (c * H + 2 * y) * W + 2 * x;
    const float v[4] = {a[base], a[base + 1], a[base + W], a[base + W + 1]};
    int k = 0;
    for (int i = 1; i < 4; i++) if (v[i] > v[k]) k = i;
    const size_t off[4] = {base, base + 1, base + W, base + W + 1};
    for (int i = 0; i < 4; i++) da[off[i]] = i == k ? dp[e] : 0.f;
  }
}

// x2 bilinear, edge clamp: u[nc][2H][2W]; half-pixel centres, or (legacy, OFX_OPT_BILINEAR_LEGACY) src = dst / 2
__device__ inline void up_taps(int u, int n, int &i0, int &i1, float &w1, int legacy) {
  const int k = u >> 1;
  if (legacy) { i0 = k; i1 = min(k + 1, n - 1); w1 = (u & 1) ? 0.5f : 0.f; }
  else if (u & 1) { i0 = k; i1 = min(k + 1, n - 1); w1 = 0.25f; }
  else { i0 = max(k - 1, 0); i1 = k; w1 = 0.75f; }
}
__global__ void t_up_fwd(int nc, int H, int W, const float *x, float *u, int legacy) {
  const int H2 = 2 * H, W2 = 2 * W;
  const size_t total = (size_t)nc * H2 * W2;
  for (size_t e = blockIdx.x * (size_t)blockDim.x + threadIdx.x; e < total; e += (size_t)gridDim.x * blockDim.x) {
    const int ux = e % W2, uy = (e / W2) % H2;
    const size_t c = e / ((size_t)W2 * H2);
    int y0, y1, x0, x1; float wy, wx;
    up_taps(uy, H, y0, y1, wy, legacy); up_taps(ux, W, x0, x1, wx, legacy);
    const float *q = x + c * H * W;
    const float top = q[(size_t)y0 * W + x0] * (1.f - wx) + q[(size_t)y0 * W + x1] * wx;
    const float bot = q[(size_t)y1 * W + x0] * (1.f - wx) + q[(size_t)y1 * W + x1] * wx;
    u[e] = top * (1.f - wy) + bot * wy;
  }
}
// gather form: dx[y][x] = sum over the up-res cells whose two taps per axis include (y, x), in a fixed order (every run
// gives the same bits; the scatter form needed float atomics).  A source row y is a tap of up-res rows 2y-2 .. 2y+2 only.
__global__ void t_up_bwd(int nc, int H, int W, const float *du, float *dx, int legacy) {
  const int H2 = 2 * H, W2 = 2 * W;
  const size_t total = (size_t)nc * H * W;
  for (size_t e = blockIdx.x * (size_t)blockDim.x + threadIdx.x; e < total; e += (size_t)gridDim.x * blockDim.x) {
    const int x = e % W, y = (e / W) % H;
    const size_t c = e / ((size_t)W * H);
    const float *q = du + c * H2 * W2;
    float cy[5], cx[5];
#pragma unroll
    for (int k = 0; k < 5; k++) {
      const int uy = 2 * y - 2 + k, ux = 2 * x - 2 + k;
      int a0, a1; float w;
      cy[k] = 0.f; cx[k] = 0.f;
      if (uy >= 0 && uy < H2) { up_taps(uy, H, a0, a1, w, legacy); cy[k] = (a0 == y ? 1.f - w : 0.f) + (a1 == y ? w : 0.f); }
      if (ux >= 0 && ux < W2) { up_taps(ux, W, a0, a1, w, legacy); cx[k] = (a0 == x ? 1.f - w : 0.f) + (a1 == x ? w : 0.f); }
    }
    float acc = 0.f;
#pragma unroll
    for (int ky = 0; ky < 5; ky++) {
      if (cy[ky] == 0.f) continue;
      const int uy = 2 * y - 2 + ky;
      float row = 0.f;
#pragma unroll
      for (int kx = 0; kx < 5; kx++)
        if (cx[kx] != 0.f) row += cx[kx] * q[(size_t)uy * W2 + 2 * x - 2 + kx];
      acc += cy[ky] * row;
    }
    dx[e] = acc;
  }
}

// dy masked by the ReLU of y (in place) when relu
__global__ void t_relu_mask(size_t total, const float *y, float *dy) {
  for (size_t e = blockIdx.x * (size_t)blockDim.x + threadIdx.x; e < total; e += (size_t)gridDim.x * blockDim.x)
    if (!(y[e] > 0.f)) dy[e] = 0.f;
}
// dw[k][o] = sum_s x[s][k] dy[s][o], db[o] = sum_s dy[s][o] (row k = in_n).  A thread owns 4 rows x 4 columns (8 loads per
// 16 FMAs instead of 2 per FMA) of one of 8 interleaved shares of the samples; the 8 shares of a tile are added in share
// order through LDS: the same bits every run.  Block = 32 tiles x 8 shares.
__global__ __launch_bounds__(256) void t_dense_bwd_w(int n, int in_n, int out_n, const float *x, const float *dy, float *dw, float *db) {
  __shared__ float red[8][32][17];
  const int oq = (out_n + 3) / 4, kq = (in_n + 1 + 3) / 4;
  const int tl = threadIdx.x & 31, share = threadIdx.x >> 5;
  const int e = blockIdx.x * 32 + tl;
  const bool live = e < oq * kq;
  const int o0 = live ? (e % oq) * 4 : 0, k0 = live ? (e / oq) * 4 : 0;
  float acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; i++)
#pragma unroll
    for (int j = 0; j < 4; j++) acc[i][j] = 0.f;
  if (live)
    for (int s = share; s < n; s += 8) {
      float xv[4], dv[4];
#pragma unroll
      for (int i = 0; i < 4; i++) xv[i] = k0 + i < in_n ? x[(size_t)s * in_n + k0 + i] : (k0 + i == in_n ? 1.f : 0.f);
#pragma unroll
      for (int j = 0; j < 4; j++) dv[j] = o0 + j < out_n ? dy[(size_t)s * out_n + o0 + j] : 0.f;
#pragma unroll
      for (int i = 0; i < 4; i++)
#pragma unroll
        for (int j = 0; j < 4; j++) acc[i][j] += xv[i] * dv[j];
    }
#pragma unroll
  for (int i = 0; i < 4; i++)
#pragma unroll
    for (int j = 0; j < 4; j++) red[share][tl][4 * i + j] = acc[i][j];
  __syncthreads();
  if (share != 0 || !live) return;
#pragma unroll
  for (int i = 0; i < 4; i++)
#pragma unroll
    for (int j = 0; j < 4; j++) {
      float t = 0.f;
#pragma unroll
      for (int q = 0; q < 8; q++) t += red[q][tl][4 * i + j];
      if (o0 + j >= out_n) continue;
      if (k0 + i < in_n) dw[(size_t)(k0 + i) * out_n + o0 + j] = t;
      else if (k0 + i == in_n) db[o0 + j] = t;
    }
}
// dx[s][k] = sum_o dy[s][o] w[k][o] (+ dx when accumulate): 4 samples x 4 inputs per thread
__global__ __launch_bounds__(256) void t_dense_bwd_x(int n, int in_n, int out_n, const float *dy, const float *w, float *dx, int accumulate) {
  const int kq = (in_n + 3) / 4, sq = (n + 3) / 4;
  const size_t e = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
  if (e >= (size_t)kq * sq) return;
  const int k0 = (int)(e % kq) * 4, s0 = (int)(e / kq) * 4;
  float acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; i++)
#pragma unroll
    for (int j = 0; j < 4; j++) acc[i][j] = 0.f;
  for (int o = 0; o < out_n; o++) {
    float dv[4], wv[4];
#pragma unroll
    for (int i = 0; i < 4; i++) dv[i] = s0 + i < n ? dy[(size_t)(s0 + i) * out_n + o] : 0.f;
#pragma unroll
    for (int j = 0; j < 4; j++) wv[j] = k0 + j < in_n ? w[(size_t)(k0 + j) * out_n + o] : 0.f;
#pragma unroll
    for (int i = 0; i < 4; i++)
#pragma unroll
      for (int j = 0; j < 4; j++) acc[i][j] += dv[i] * wv[j];
  }
#pragma unroll
  for (int i = 0; i < 4; i++)
#pragma unroll
    for (int j = 0; j < 4; j++) {
      if (s0 + i >= n || k0 + j >= in_n) continue;
      const size_t at = (size_t)(s0 + i) * in_n + k0 + j;
      dx[at] = accumulate ? dx[at] + acc[i][j] : acc[i][j];
    }
}

// out[c][r] = in[r][c] (a weight matrix or a batch of activations for the MFMA GEMM's row-major operands)
__global__ void t_transpose(int rows, int cols, const float *in, float *out) {
  __shared__ float tile[32][33];
  const int r0 = blockIdx.y * 32, c0 = blockIdx.x * 32, tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  for (int i = ty; i < 32; i += 8)
    if (r0 + i < rows && c0 + tx < cols) tile[i][tx] = in[(size_t)(r0 + i) * cols + c0 + tx];
  __syncthreads();
  for (int i = ty; i < 32; i += 8)
    if (c0 + i < cols && r0 + tx < rows) out[(size_t)(c0 + i) * rows + r0 + tx] = tile[tx][i];
}

// f[n][5008] = concat(vec8, flatten_hwc(x4 [n][8][25][25])) and its transpose for the gradient
__global__ void t_concat_fwd(int n, const ofx_transition *rows, const float *x4, float *f, int next_head) {
  const size_t total = (size_t)n * 5008;
  for (size_t e = blockIdx.x * (size_t)blockDim.x + threadIdx.x; e < total; e += (size_t)gridDim.x * blockDim.x) {
    const int k = e % 5008, s = e / 5008;
    if (k < 8) f[e] = next_head ? rows[s].head_next[k] : rows[s].head_prev[k];
    else { const int j = k - 8, c = j % 8, p = j / 8; f[e] = x4[((size_t)s * 8 + c) * 625 + p]; }
  }
}
__global__ void t_concat_bwd(int n, const float *df, float *dx4) {
  const size_t total = (size_t)n * 5000;
  for (size_t e = blockIdx.x * (size_t)blockDim.x + threadIdx.x; e < total; e += (size_t)gridDim.x * blockDim.x) {
    const int j = e % 5000, s = e / 5000, c = j % 8, p = j / 8;
    dx4[((size_t)s * 8 + c) * 625 + p] = df[(size_t)s * 5008 + 8 + j];
  }
}

// loss seeds: one non-zero error per head and sample; loss[0] += mse(out1) share, loss[1] += mse(out2) share.
// rw (may be null = 1): per-row loss weights; td (may be null): the raw errors (e1, e2); delta: ofx_loss_seed's - 0 the
// squared error, > 0 Huber(delta) (ofx_dqn_fit_robust)
__global__ void t_loss_seed(int n, const ofx_transition *rows, const float *o1, const float *o2, const float *y_act,
                            const float *y_ptr, float *do1, float *do2, float *lpart, const float *rw, float *td, float delta) {
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= n) return;
  const ofx_transition r = rows[s];
  if (r.ship < 0) { lpart[2 * s] = lpart[2 * s + 1] = 0.f; return; }  // padding row: no error
  const int a = r.iaction ? 1 : 0, px = min(max(r.px, 0), TPS - 1), py = min(max(r.py, 0), TPS - 1);
  const float e1 = o1[2 * s + a] - y_act[s];
  const size_t k = (size_t)s * TPS * TPS + (size_t)py * TPS + px;
  const float e2 = o2[k] - y_ptr[s];
  const float w = rw ? rw[s] : 1.f;
  lpart[2 * s] = ofx_loss_seed(e1, w, 2.f * n, delta, &do1[2 * s + a]);      // summed in sample order by t_sum_ordered
  lpart[2 * s + 1] = ofx_loss_seed(e2, w, (float)(TPS * TPS) * n, delta, &do2[k]);
  if (td) { td[2 * s] = e1; td[2 * s + 1] = e2; }
}
// out[j] = sum_i part[i * stride + j] for j < stride, in index order (one thread per j: tiny)
__global__ void t_sum_ordered(int count, int stride, const float *part, float *out) {
  const int j = threadIdx.x;
  if (j >= stride) return;
  double acc = 0.0;
  for (int i = 0; i < count; i++) acc += (double)part[(size_t)i * stride + j];
  out[j] = (float)acc;
}

// ---- global gradient norm (ofx_dqn_fit_robust): sum g^2 over the whole blob, the same bits on every run ----
// A fixed grid of kNormBlocks x 256; each thread sums its grid-stride share in double, the four wave64s of a block
// combine in LDS by a fixed tree, part[block] goes to t_clip_scale.
static const int kNormBlocks = 256;
__global__ __launch_bounds__(256) void t_sqnorm_part(size_t cnt, const float *g, double *part) {
  __shared__ double red[256];
  double acc = 0.0;
  for (size_t e = blockIdx.x * (size_t)blockDim.x + threadIdx.x; e < cnt; e += (size_t)gridDim.x * blockDim.x) {
    const double v = (double)g[e];
    acc += v * v;
  }
  red[threadIdx.x] = acc;
  __syncthreads();
  for (int k = 128; k > 0; k >>= 1) {
    if ((int)threadIdx.x < k) red[threadIdx.x] += red[threadIdx.x + k];
    __syncthreads();
  }
  if (threadIdx.x == 0) part[blockIdx.x] = red[0];
}
// one thread, like t_sum_ordered: the block partials in index order (count == 0: no norm asked for), then
// loss[2] = scale * norm and loss[3] = the one factor Adam multiplies the gradient by, the factor of
// torch.nn.utils.clip_grad_norm_, min(1, clip / (norm + 1e-6)) in fp32 (clip == 0: no clipping, 1), times scale - the two
// multiplied once.  tail null (a fit's own gradient): scale is 1 - both products by 1.0f are exact - and the losses are
// left alone; else (ofx_dqn_apply: tail = the accumulator's last OFX_ACC_TAIL floats) loss[0..1] = scale * its two losses.
__global__ void t_clip_scale(int count, const double *part, float clip, float scale, const float *tail, float *loss) {
  if (threadIdx.x || blockIdx.x) return;
  double acc = 0.0;
  for (int i = 0; i < count; i++) acc += part[i];
  const float sc = tail ? scale : 1.f, norm = (float)sqrt(acc) * sc;
  if (tail) {
    loss[0] = sc * tail[OFX_ACC_LOSS];
    loss[1] = sc * tail[OFX_ACC_LOSS + 1];
  }
  loss[2] = norm;
  loss[3] = (clip > 0.f ? fminf(1.f, clip / (norm + 1e-6f)) : 1.f) * sc;
}

// Trainer.replay as written (ofx_dqn_fit_reference): the targets are whole predictions of `state` with one entry
// replaced per head, so every output carries an error.  t1 [n][2], t2 [n][TPS][TPS].
__global__ void t_reference_targets(int n, const ofx_transition *rows, float gamma, const float *act_next,
                                    const float *max_next, float *t1, float *t2) {
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= n) return;
  const ofx_transition r = rows[s];
  const float live = r.done ? 0.f : 1.f;                                     // int(not done)
  const int px = min(max(r.px, 0), TPS - 1), py = min(max(r.py, 0), TPS - 1);
  t1[2 * s + (r.iaction ? 1 : 0)] = (float)r.reward + gamma * fmaxf(act_next[2 * s], act_next[2 * s + 1]) * live;  // :279
  // ptr_target[ipointer] with ipointer = (x, y) on the (400, 400, 1) prediction = [row][col][0]: row x, column y (:280)
  t2[(size_t)s * TPS * TPS + (size_t)px * TPS + py] = (float)r.reward + gamma * max_next[s] * live;
}

// ---- TD targets of Trainer.replay (agents/qlearnIA_V2.py:251-270): the four ofx_dqn_targets* entries below ----
// The TD arithmetic (the forwards run in ofx_policy.hip).  It lives in this
// -ffp-contract=off file because the n-step form must round the product and the sum on their own, and under
// -ffp-contract=fast the backend fuses them whatever `#pragma clang fp contract` says.  The one-step form gives the
// bits it gave there as fma(live, gamma * m, reward): live is 0 or 1, so that fma rounds once, like the add here.
//
// The entries differ only in where the two bootstrap values of next_state come from:
//   v_act = the value of act [n][2]: act[2 i + sel[i]] when sel is given (Double DQN: the online forward's iaction - the
//           first maximum - picks among the target network's values), else the two-action soft value at tau_act, which
//           at tau_act == 0 is np.max(prediction);
//   v_ptr = ptr[i]: the heat map's maximum (max_next), the target network's map probed at the online forward's ipointer
//           (probe_tgt), or the forward's soft value (soft_next = ptr_soft of ofx_policy_forward_obs_soft).
struct Bootstrap {
  const float *act;     // [n][2]
  const int32_t *sel;   // [n] or null
  const float *ptr;     // [n]
  float tau_act;
};
// the Munchausen bonus (ofx_dqn_targets_soft, one-step form only): alpha > 0 adds the scaled, clipped T ln pi(a | s) of the
// action taken to the reward; soft_prev [n] is ptr_soft of `state`
struct Munchausen { float alpha, clip; const float *soft_prev; };

__device__ __forceinline__ float soft_act_value(float a0, float a1, float tau) {
  const float m = fmaxf(a0, a1);  // np.max(prediction)
  if (tau == 0.f) return m;
  return m + tau * log1pf(expf(-fabsf(a0 - a1) / tau));
}
// ret / disc null: the one-step form, y = reward + gamma * v * int(not done); else n-step, y = ret + disc * v.  Every
// operation is rounded on its own.  q_sa / p_sp (may be null): the forward on `state` was run (act_prev / probe_prev).
__global__ void k_dqn_targets(int n, const ofx_transition *rows, float gamma, const float *act_prev, const float *probe_prev,
                              Bootstrap B, Munchausen M, float *q_sa, float *p_sp, float *y_act, float *y_ptr,
                              const float *ret, const float *disc) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const ofx_transition r = rows[i];
  if (r.ship < 0) {
    if (q_sa) q_sa[i] = p_sp[i] = 0.f;
    y_act[i] = y_ptr[i] = 0.f;
    return;
  }
  const int a = r.iaction ? 1 : 0;
  if (q_sa) {
    q_sa[i] = act_prev[2 * i + a];
    p_sp[i] = probe_prev[i];
  }
  const float v_act = B.sel ? B.act[2 * i + (B.sel[i] ? 1 : 0)] : soft_act_value(B.act[2 * i], B.act[2 * i + 1], B.tau_act);
  const float v_ptr = B.ptr[i];
  if (ret) {
    y_act[i] = ret[i] + disc[i] * v_act;
    y_ptr[i] = ret[i] + disc[i] * v_ptr;
    return;
  }
  const float live = r.done ? 0.f : 1.f;  // int(not done)
  float r_act = (float)r.reward, r_ptr = (float)r.reward;
  if (M.alpha > 0.f) {
    const float l_act = act_prev[2 * i + a] - soft_act_value(act_prev[2 * i], act_prev[2 * i + 1], B.tau_act);
    const float l_ptr = probe_prev[i] - M.soft_prev[i];
    r_act = r_act + M.alpha * fminf(fmaxf(l_act, M.clip), 0.f);
    r_ptr = r_ptr + M.alpha * fminf(fmaxf(l_ptr, M.clip), 0.f);
  }
  y_act[i] = r_act + gamma * v_act * live;
  y_ptr[i] = r_ptr + gamma * v_ptr * live;
}

// ofx_policy_blend_weights: dst = c * dst + tau * src with c = 1 - tau formed once by the caller; both products are
// rounded, then the sum (this file is compiled with -ffp-contract=off)
__global__ void k_blend_weights(size_t cnt, float *dst, const float *src, float c, float tau) {
  for (size_t e = blockIdx.x * (size_t)blockDim.x + threadIdx.x; e < cnt; e += (size_t)gridDim.x * blockDim.x)
    dst[e] = c * dst[e] + tau * src[e];
}

// the rows' observation heads [n][8] and (probe, may be null) clamped pointers [n][2]; zeros for a padding row
__global__ void k_dqn_unpack(int n, const ofx_transition *rows, float *vec_prev, float *vec_next, int32_t *probe) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const ofx_transition r = rows[i];
  const bool pad = r.ship < 0;
#pragma unroll
  for (int k = 0; k < 8; k++) {
    vec_prev[(size_t)i * 8 + k] = pad ? 0.f : r.head_prev[k];
    vec_next[(size_t)i * 8 + k] = pad ? 0.f : r.head_next[k];
  }
  if (!probe) return;
  probe[2 * i] = pad ? 0 : min(max(r.px, 0), TPS - 1);
  probe[2 * i + 1] = pad ? 0 : min(max(r.py, 0), TPS - 1);
}

// dense targets: d = 2 (o - t) scale; block b's share of the loss goes to lpart[b] (summed in block order afterwards)
__global__ __launch_bounds__(256) void t_loss_dense(size_t total, float scale, const float *o, const float *t, float *d, float *lpart) {
  __shared__ float red[256];
  float acc = 0.f;
  for (size_t e = blockIdx.x * (size_t)blockDim.x + threadIdx.x; e < total; e += (size_t)gridDim.x * blockDim.x) {
    const float err = o[e] - t[e];
    d[e] = 2.f * err * scale;
    acc += err * err * scale;
  }
  red[threadIdx.x] = acc;
  __syncthreads();
  for (int k = 128; k > 0; k >>= 1) {
    if ((int)threadIdx.x < k) red[threadIdx.x] += red[threadIdx.x + k];
    __syncthreads();
  }
  if (threadIdx.x == 0) lpart[blockIdx.x] = red[0];
}

// c1 = 1 - beta1 and c2 = 1 - beta2 arrive rounded from their decimal values (0.1, 0.001): formed in fp32 from the rounded
// betas, 1.f - 0.999f is 0.000999987 - 1.3e-5 off the constant of the recurrence, 27 times what the format asks for.
// scale (may be null = 1): Adam on scale[0] * g, the factor t_clip_scale left in device memory (no host round trip between
// the gradient and the update); a factor of exactly 1 - the clip inactive - gives the bits of the null form
__global__ void t_adam(size_t cnt, float *w, const float *g, float *m, float *v, float lr_t, float b1, float b2, float c1,
                       float c2, float eps, const float *scale) {
  const float sc = scale ? scale[0] : 1.f;
  for (size_t e = blockIdx.x * (size_t)blockDim.x + threadIdx.x; e < cnt; e += (size_t)gridDim.x * blockDim.x) {
    const float gi = scale ? sc * g[e] : g[e];
    const float mi = b1 * m[e] + c1 * gi, vi = b2 * v[e] + c2 * gi * gi;
    m[e] = mi; v[e] = vi;
    w[e] -= lr_t * mi / (sqrtf(vi) + eps);
  }
}

// ---- the split fit (ofx_dqn_grad / ofx_dqn_apply): the accumulator is [n_floats gradient][OFX_ACC_TAIL] (include/ofx.h) ----
// One micro-batch into the accumulator, element by element in a fixed order: the gradient blob, the {mean, var} pairs
// t_moving_scaled reads from the 7 stat slots, the two losses, a count of 1 and zeros.  reset: acc = value, else acc += value - a
// plain fp32 add (this file is compiled with -ffp-contract=off), no scale.
struct AccSrc {
  const float *stat[7];   // trunk 0-3, head-2 0-2
  int stat_n[7];          // floats that hold data in each slot: 2 x channels
  const float *loss;      // {loss1, loss2}
};
__global__ void t_accumulate(size_t n_floats, const float *grad, AccSrc S, float *acc, int reset) {
  const size_t total = n_floats + OFX_ACC_TAIL;
  for (size_t e = blockIdx.x * (size_t)blockDim.x + threadIdx.x; e < total; e += (size_t)gridDim.x * blockDim.x) {
    float v = 0.f;
    if (e < n_floats) v = grad[e];
    else {
      const int k = (int)(e - n_floats), slot = k / OFX_ACC_STAT_FLOATS, i = k % OFX_ACC_STAT_FLOATS;
      if (slot < 7) v = i < S.stat_n[slot] ? S.stat[slot][i] : 0.f;
      else if (k == OFX_ACC_LOSS) v = S.loss[0];
      else if (k == OFX_ACC_LOSS + 1) v = S.loss[1];
      else if (k == OFX_ACC_COUNT) v = 1.f;
    }
    acc[e] = reset ? v : acc[e] + v;
  }
}
// moving = 0.99 moving + 0.01 (scale * stat): stat holds the batch statistics {mean, var} per channel - a fit's own at
// scale 1 (the product by 1.0f is exact and nothing here is contracted: the bits of the unscaled expression), or the
// accumulator's summed ones (ofx_dqn_apply)
__global__ void t_moving_scaled(int c_n, float *mean, float *var, const float *stat, float scale) {
  const int c = threadIdx.x;
  if (c >= c_n) return;
  mean[c] = 0.99f * mean[c] + 0.01f * (scale * stat[2 * c]);
  var[c] = 0.99f * var[c] + 0.01f * (scale * stat[2 * c + 1]);
}

// ---------------------------------------------------------------- host orchestration
#define GRID(total) dim3((unsigned)(((total) + 255) / 256 > 65535 * 16 ? 65535 * 16 : ((total) + 255) / 256)), dim3(256)
#define K(kern, total, ...) do { hipLaunchKernelGGL(kern, GRID(total), 0, st, __VA_ARGS__); OFX_HIP(hipGetLastError()); } while (0)

static const int kWSlices = 128;

static void conv_bwd_weight(hipStream_t st, int n, int ci, int co, int H, int W, const float *x, const float *dz,
                            double *part, float *dw, float *db) {
  const int nw = 9 * ci * co;
  // few weights over many pixels (out2, upconv3) need the slices to fill the chip; small maps do not
  const size_t total = (size_t)n * H * W;
  // the partial-sum buffer holds kWSlices * 600 doubles: a layer with few weights can afford more, shorter slices
  const int cap = (int)((size_t)kWSlices * 600 / (size_t)(nw + co));
  int slices = (int)((total + 8191) / 8192);
  slices = slices < 1 ? 1 : slices > cap ? cap : slices;
  if (slices > 1024) slices = 1024;
#define BWW(CIB, COB) hipLaunchKernelGGL((t_conv_bwd_weight<CIB, COB>), dim3((ci / CIB) * (co / COB), slices), dim3(256), 0, st, n, ci, co, H, W, x, dz, part)
  if (co % 4 == 0) BWW(1, 4);
  else if (co % 2 == 0 && ci % 2 == 0) BWW(2, 2);
  else if (co % 2 == 0) BWW(1, 2);
  else if (ci % 4 == 0) BWW(4, 1);
  else BWW(1, 1);
#undef BWW
  hipLaunchKernelGGL(t_conv_bwd_finish, dim3((nw + co + 255) / 256), dim3(256), 0, st, nw, co, slices, part, dw, db);
}

// one blockIdx.y per (sample, channel) plane of `per` elements, up to 64 blocks of 256 threads along it
#define PLANES(per, planes) dim3((unsigned)(((per) + 255) / 256 > 64 ? 64 : ((per) + 255) / 256), (unsigned)(planes)), dim3(256)
static int conv_fwd(hipStream_t st, int n, int ci, int co, int H, int W, const float *x, const float *w, const float *b, float *z) {
  const size_t px = (size_t)n * H * W;
  switch (co) {
    case 8: hipLaunchKernelGGL(t_conv_fwd<8>, GRID(px), 0, st, n, ci, H, W, x, w, b, z); break;
    case 4: hipLaunchKernelGGL(t_conv_fwd<4>, GRID(px), 0, st, n, ci, H, W, x, w, b, z); break;
    case 2: hipLaunchKernelGGL(t_conv_fwd<2>, GRID(px), 0, st, n, ci, H, W, x, w, b, z); break;
    case 1: hipLaunchKernelGGL(t_conv_fwd<1>, GRID(px), 0, st, n, ci, H, W, x, w, b, z); break;
    default: ofx_set_error("ofx_dqn_fit: no conv kernel for %d output channels", co); return OFX_ERR_STATE;
  }
  OFX_HIP(hipGetLastError());
  return OFX_OK;
}
static int conv_bwd_data(hipStream_t st, int n, int ci, int co, int H, int W, const float *dz, const float *w, float *dx) {
  const size_t px = (size_t)n * H * W;
  switch (ci) {
    case 8: hipLaunchKernelGGL(t_conv_bwd_data<8>, GRID(px), 0, st, n, co, H, W, dz, w, dx); break;
    case 4: hipLaunchKernelGGL(t_conv_bwd_data<4>, GRID(px), 0, st, n, co, H, W, dz, w, dx); break;
    case 2: hipLaunchKernelGGL(t_conv_bwd_data<2>, GRID(px), 0, st, n, co, H, W, dz, w, dx); break;
    case 1: hipLaunchKernelGGL(t_conv_bwd_data<1>, GRID(px), 0, st, n, co, H, W, dz, w, dx); break;
    default: ofx_set_error("ofx_dqn_fit: no conv kernel for %d input channels", ci); return OFX_ERR_STATE;
  }
  OFX_HIP(hipGetLastError());
  return OFX_OK;
}

__global__ void t_count_pads(int n, const ofx_transition *rows, int32_t *out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n && rows[i].ship < 0) atomicAdd(out, 1);
}

// a workspace the handle keeps between calls: grown on demand, given back when a call needs less than a quarter of it (one
// 4096-row fit leaves 40 GB behind - a handle that then trains on 256 rows should not hold them), freed by ofx_destroy
static int keep_workspace(ofx_handle *h, void **buf, size_t *have, size_t need) {
  if (*have / 4 > need) *have = 0;   // given back: allocated anew at `need`
  return ofx_ensure_buffer(h, buf, have, need);
}

// A workspace (ofx_arena.h): `layout`, the one statement of its buffers, measures; the handle's block is ensured (keep: under
// keep_workspace's give-back rule); `layout` hands out the pointers; ok() is checked before the caller's first launch
template <class Layout>
static int carve(ofx_handle *h, void **buf, size_t *have, bool keep, const char *who, Layout layout) {
  Arena measure;
  layout(measure);
  const int rc = keep ? keep_workspace(h, buf, have, measure.used) : ofx_ensure_buffer(h, buf, have, measure.used);
  if (rc) return rc;
  Arena A(*buf, measure.used);
  layout(A);
  if (!A.ok()) { ofx_set_error("%s: internal workspace sized too small", who); return OFX_ERR_STATE; }
  return OFX_OK;
}

// padding rows (ship < 0) would enter the BatchNorm batch statistics and the loss scale: refused before any work is done
static int refuse_pads(ofx_handle *h, int n, const ofx_transition *rows, const char *who) {
  hipStream_t st = h->stream;
  int32_t *counter, pads = 0;
  int rc = ofx_counter(h, OFX_COUNTER_PADS, &counter);
  if (rc) return rc;
  OFX_HIP(hipMemsetAsync(counter, 0, sizeof(int32_t), st));
  hipLaunchKernelGGL(t_count_pads, dim3((n + 255) / 256), dim3(256), 0, st, n, rows, counter);
  OFX_HIP(hipMemcpyAsync(&pads, counter, sizeof(pads), hipMemcpyDeviceToHost, st));
  OFX_HIP(hipStreamSynchronize(st));
  if (pads) {
    ofx_set_error("%s: %d of %d rows are padding (ship < 0); gather with ofx_replay_gather_valid", who, pads, n);
    return OFX_ERR_INVALID;
  }
  return OFX_OK;
}

// ofx_dqn_targets (ret == disc == null) and ofx_dqn_targets_nstep: the same two forwards, then the one k_dqn_targets launch
// every form ends in.
// ofx_dqn_targets_double (dbl; `weights` is the online blob): the forward on next_state runs twice - online for
// (iaction, ipointer), then `target` probed at that pointer - and the bootstrap is the target's values at that selection.
// ofx_dqn_targets_soft (soft): the forwards are ofx_policy_forward_obs_soft's - max_next then holds ptr_soft of next_state,
// and with the Munchausen term the forward on `state` runs whether or not q_sa / p_sp are wanted and adds soft_prev.
// What one forward hands to the next lives in the aux arena: the forward's scratch block is laid out anew by each.
struct SoftArgs { float tau_act, tau_ptr, m_alpha, m_clip; };   // checked by ofx_dqn_targets_soft
struct TargetsWs {
  float *vec_prev, *vec_next, *act_prev, *act_next, *probe_prev, *max_next, *act_tgt, *probe_tgt, *soft_prev;
  int32_t *probe, *sel_action, *sel_pointer;   // sel_*, *_tgt: the double form only, soft_prev: the soft form only (null otherwise)
};
static void targets_layout(Arena &A, size_t n, bool dbl, bool soft, TargetsWs &W) {
  W.vec_prev = A.f(8 * n); W.vec_next = A.f(8 * n);
  W.probe = A.n<int32_t>(2 * n);
  W.act_prev = A.f(2 * n); W.act_next = A.f(2 * n); W.probe_prev = A.f(n); W.max_next = A.f(n);
  W.sel_action = dbl ? A.n<int32_t>(n) : nullptr; W.sel_pointer = dbl ? A.n<int32_t>(2 * n) : nullptr;
  W.act_tgt = dbl ? A.f(2 * n) : nullptr; W.probe_tgt = dbl ? A.f(n) : nullptr;
  W.soft_prev = soft ? A.f(n) : nullptr;
}
static int dqn_targets_impl(ofx_handle *h, const char *who, const float *weights, const float *target, bool dbl, int32_t n,
                            const ofx_transition *rows, const void *bits_prev, const void *bits_next, float gamma,
                            const float *ret, const float *disc, float *q_sa, float *p_sp, float *y_act, float *y_ptr,
                            const SoftArgs *soft = nullptr) {
  if (!h || !weights || (dbl && !target) || !rows || !bits_prev || !bits_next || (!q_sa) != (!p_sp) || !y_act || !y_ptr ||
      n < 1) {
    ofx_set_error("%s: bad argument", who);
    return OFX_ERR_INVALID;
  }
  OFX_HIP(hipSetDevice(h->cfg.device));
  TargetsWs W;
  int rc = carve(h, &h->aux, &h->aux_bytes, false, who, [&](Arena &A) { targets_layout(A, (size_t)n, dbl, soft != nullptr, W); });
  if (rc) return rc;
  hipLaunchKernelGGL(k_dqn_unpack, dim3((n + 255) / 256), dim3(256), 0, h->stream, n, rows, W.vec_prev, W.vec_next, W.probe);
  OFX_HIP(hipGetLastError());
  // q_sa = p_sp = NULL: the caller only wants the targets (ofx_dqn_fit's own forward gives the current values) - the forward
  // on `state` is skipped
  if (soft && soft->m_alpha > 0.f) {   // Munchausen: always, with the soft value of `state` next to the probe
    if ((rc = ofx_policy_forward_obs_soft(h, weights, n, bits_prev, W.vec_prev, soft->tau_ptr, W.act_prev, nullptr, nullptr, nullptr,
                                          W.probe, W.probe_prev, W.soft_prev, nullptr, nullptr)))
      return rc;
  } else if (q_sa && (rc = ofx_policy_forward_obs(h, weights, n, bits_prev, W.vec_prev, W.act_prev, nullptr, nullptr, nullptr, W.probe, W.probe_prev)))
    return rc;
  Bootstrap B = {W.act_next, nullptr, W.max_next, 0.f};   // two-action value at tau_act, the pointer head's from the forward
  Munchausen M = {0.f, 0.f, nullptr};
  if (soft) {
    rc = ofx_policy_forward_obs_soft(h, weights, n, bits_next, W.vec_next, soft->tau_ptr, W.act_next, nullptr, nullptr, nullptr,
                                     nullptr, nullptr, W.max_next, nullptr, nullptr);
    B.tau_act = soft->tau_act;
    M = {soft->m_alpha, soft->m_clip, W.soft_prev};
  } else if (dbl) {
    // online first (the pinned slot when `weights` is the pinned blob), then the target through prep_tmp
    if ((rc = ofx_policy_forward_obs(h, weights, n, bits_next, W.vec_next, nullptr, W.sel_action, W.sel_pointer, nullptr, nullptr, nullptr)))
      return rc;
    rc = ofx_policy_forward_obs(h, target, n, bits_next, W.vec_next, W.act_tgt, nullptr, nullptr, nullptr, W.sel_pointer, W.probe_tgt);
    B = {W.act_tgt, W.sel_action, W.probe_tgt, 0.f};
  } else {
    rc = ofx_policy_forward_obs(h, weights, n, bits_next, W.vec_next, W.act_next, nullptr, nullptr, W.max_next, nullptr, nullptr);
  }
  if (rc) return rc;
  hipLaunchKernelGGL(k_dqn_targets, dim3((n + 255) / 256), dim3(256), 0, h->stream, n, rows, gamma, W.act_prev, W.probe_prev, B, M,
                     q_sa, p_sp, y_act, y_ptr, ret, disc);
  OFX_HIP(hipGetLastError());
  return OFX_OK;
}

extern "C" int ofx_dqn_targets(ofx_handle *h, const float *weights, int32_t n, const ofx_transition *rows,
                               const void *bits_prev, const void *bits_next, float gamma, float *q_sa, float *p_sp,
                               float *y_act, float *y_ptr) {
  return dqn_targets_impl(h, "ofx_dqn_targets", weights, nullptr, false, n, rows, bits_prev, bits_next, gamma, nullptr,
                          nullptr, q_sa, p_sp, y_act, y_ptr);
}

extern "C" int ofx_dqn_targets_nstep(ofx_handle *h, const float *weights, int32_t n, const ofx_transition *rows,
                                     const void *bits_prev, const void *bits_next, const float *ret, const float *disc,
                                     float *q_sa, float *p_sp, float *y_act, float *y_ptr) {
  if (!ret || !disc) { ofx_set_error("ofx_dqn_targets_nstep: ret and disc must be given"); return OFX_ERR_INVALID; }
  return dqn_targets_impl(h, "ofx_dqn_targets_nstep", weights, nullptr, false, n, rows, bits_prev, bits_next, 0.f, ret,
                          disc, q_sa, p_sp, y_act, y_ptr);
}

extern "C" int ofx_dqn_targets_double(ofx_handle *h, const float *online, const float *target, int32_t n,
                                      const ofx_transition *rows, const void *bits_prev, const void *bits_next,
                                      float gamma, const float *ret, const float *disc, float *q_sa, float *p_sp,
                                      float *y_act, float *y_ptr) {
  if ((!ret) != (!disc)) { ofx_set_error("ofx_dqn_targets_double: pass ret and disc together"); return OFX_ERR_INVALID; }
  return dqn_targets_impl(h, "ofx_dqn_targets_double", online, target, true, n, rows, bits_prev, bits_next,
                          ret ? 0.f : gamma, ret, disc, q_sa, p_sp, y_act, y_ptr);
}

static bool soft_tau_ok(float tau) { return tau == 0.f || (tau >= 1e-6f && tau <= 1e30f); }   // NaN fails every comparison

extern "C" int ofx_dqn_targets_soft(ofx_handle *h, const float *weights, int32_t n, const ofx_transition *rows,
                                    const void *bits_prev, const void *bits_next, float gamma, const float *ret,
                                    const float *disc, float tau_act, float tau_ptr, float m_alpha, float m_clip, float *q_sa,
                                    float *p_sp, float *y_act, float *y_ptr) {
  const char *who = "ofx_dqn_targets_soft";
  if ((!ret) != (!disc)) { ofx_set_error("%s: pass ret and disc together", who); return OFX_ERR_INVALID; }
  if (!soft_tau_ok(tau_act) || !soft_tau_ok(tau_ptr)) {
    ofx_set_error("%s: tau_act = %g, tau_ptr = %g; each must be 0 or lie in [1e-6, 1e30]", who, (double)tau_act, (double)tau_ptr);
    return OFX_ERR_INVALID;
  }
  if (!(m_alpha >= 0.f && m_alpha <= 1.f)) { ofx_set_error("%s: m_alpha = %g; it must lie in [0, 1]", who, (double)m_alpha); return OFX_ERR_INVALID; }
  if (m_alpha > 0.f && (ret || tau_act == 0.f || tau_ptr == 0.f || !(m_clip <= 0.f && m_clip > -INFINITY))) {
    ofx_set_error("%s: the Munchausen term (m_alpha > 0) takes the one-step form, both taus > 0 and a finite m_clip <= 0 (got %g)", who,
                  (double)m_clip);
    return OFX_ERR_INVALID;
  }
  const SoftArgs soft = {tau_act, tau_ptr, m_alpha, m_clip};
  return dqn_targets_impl(h, who, weights, nullptr, false, n, rows, bits_prev, bits_next, ret ? 0.f : gamma, ret, disc, q_sa, p_sp,
                          y_act, y_ptr, &soft);
}

// Soft / hard update of a target network: the whole blob, BatchNorm moving statistics included.  tau == 1 is a copy (a
// NaN in dst must not survive 0 * NaN), tau == 0 is nothing at all.
extern "C" int ofx_policy_blend_weights(ofx_handle *h, float *dst, const float *src, float tau) {
  if (!h || !dst || !src || dst == src) {
    ofx_set_error("ofx_policy_blend_weights: bad argument (null, or dst == src)");
    return OFX_ERR_INVALID;
  }
  if (!(tau >= 0.f && tau <= 1.f)) {   // NaN fails both comparisons
    ofx_set_error("ofx_policy_blend_weights: tau must lie in [0, 1], got %g", (double)tau);
    return OFX_ERR_INVALID;
  }
  OFX_HIP(hipSetDevice(h->cfg.device));
  hipStream_t st = h->stream;
  ofx_policy_desc L;
  int rc = ofx_policy_layout(h, &L);
  if (rc) return rc;
  if (tau == 0.f) return OFX_OK;
  const size_t cnt = (size_t)L.n_floats;
  if (tau == 1.f) OFX_HIP(hipMemcpyAsync(dst, src, sizeof(float) * cnt, hipMemcpyDeviceToDevice, st));
  else K(k_blend_weights, cnt, cnt, dst, src, 1.0f - tau, tau);
  return ofx_policy_weights_updated(h, dst);
}

// One fit step, as the extern "C" entries hand it to the drivers.  Two forms of the targets: the sparse one of ofx_dqn_fit
// (one error per head and sample: y_act / y_ptr, inputs = `state`) and the dense one of ofx_dqn_fit_reference (t1 [n][2] /
// t2 [n][400][400] whole target tensors, inputs = next_state's maps + the rows' next_state head).  Everything from
// row_weight on belongs to the sparse form and is off by default.
struct FitCall {
  float *weights = nullptr, *adam_m = nullptr, *adam_v = nullptr;
  int32_t step = 1, n = 0;
  float lr = 0.f;
  const ofx_transition *rows = nullptr;
  const void *bits = nullptr;                                            // the input maps [n][2][5000] words
  const float *y_act = nullptr, *y_ptr = nullptr, *t1 = nullptr, *t2 = nullptr;   // sparse / dense targets
  float *grad_out = nullptr, *loss_host = nullptr;                       // either may be null
  const float *row_weight = nullptr;                                     // per-row loss weights and the rows' errors
  float *td_out = nullptr, *grad_norm_host = nullptr;                    // (ofx_dqn_fit_weighted); the norm's read-back
  float huber_delta = 0.f, clip_norm = 0.f, scale = 1.f;                 // ofx_dqn_fit_robust; tail's factor
  // the split fit.  acc (ofx_dqn_grad): the drivers stop after the gradient and hand it to fit_accumulate instead of the
  // update.  tail (ofx_dqn_apply): the gradient is an accumulator, tail its last OFX_ACC_TAIL floats, scale its factor.
  float *acc = nullptr;
  const float *tail = nullptr;
  int acc_reset = 0;
  bool norm() const { return clip_norm > 0.f || grad_norm_host; }
};

// The tail of a fit step, after the gradients: Adam on the trained tensors, the moving BatchNorm statistics from the batch
// statistics (tstat / ustat: trunk / head-2 layers), the loss read back (a synchronisation), a pinned blob prepared again.
// ofx_dqn_fit_robust (C.clip_norm > 0 or C.grad_norm_host given): the gradient's global norm and the clip factor go to
// loss[2] / loss[3] - the slot is 64 floats - so the copy that fetches the loss fetches the norm too; with a clip, Adam
// reads the factor from there.  npart: kNormBlocks doubles.
static int fit_apply_update(ofx_handle *h, const ofx_policy_desc &L, const FitCall &C, const float *grad,
                            const float *const *tstat, const float *const *ustat, float *loss, double *npart) {
  hipStream_t st = h->stream;
  float *weights = C.weights;
  const float b1 = 0.9f, b2 = 0.999f;
  const float lr_t = C.lr * sqrtf(1.f - powf(b2, (float)C.step)) / (1.f - powf(b1, (float)C.step));
  const bool scaled = C.clip_norm > 0.f || (C.tail && C.scale != 1.f);   // Adam reads its factor from loss[3]
  // the norm pass (untrained slots of the gradient blob are zero: one pass over all of it), then the norm, the factor
  // and - an accumulator's (C.tail) - the losses times scale; neither asked for: nothing is launched
  if (C.norm()) hipLaunchKernelGGL(t_sqnorm_part, dim3(kNormBlocks), dim3(256), 0, st, (size_t)L.n_floats, grad, npart);
  if (C.norm() || C.tail)
    hipLaunchKernelGGL(t_clip_scale, dim3(1), dim3(64), 0, st, C.norm() ? kNormBlocks : 0, npart, C.clip_norm, C.scale, C.tail, loss);
  OFX_HIP(hipGetLastError());
  for (int t = 0; t < L.n_tensors; t++) {
    if (!ofx_blob_trained(t)) continue;  // moving mean / variance
    K(t_adam, (size_t)L.count[t], (size_t)L.count[t], weights + L.offset[t], grad + L.offset[t], C.adam_m + L.offset[t],
      C.adam_v + L.offset[t], lr_t, b1, b2, 0.1f, 0.001f, 1e-7f, scaled ? loss + 3 : (const float *)nullptr);
  }
  // (a fit's own statistics: scale 1, the bits of the unscaled expression)
  for (int i = 0; i < 4; i++)
    hipLaunchKernelGGL(t_moving_scaled, dim3(1), dim3(64), 0, st, 8, weights + L.offset[ofx_t_trunk(i, OFX_T_MEAN)],
                       weights + L.offset[ofx_t_trunk(i, OFX_T_VAR)], tstat[i], C.scale);
  for (int j = 0; j < 3; j++)
    hipLaunchKernelGGL(t_moving_scaled, dim3(1), dim3(64), 0, st, kUpCout[j], weights + L.offset[ofx_t_up(j, OFX_T_MEAN)],
                       weights + L.offset[ofx_t_up(j, OFX_T_VAR)], ustat[j], C.scale);
  OFX_HIP(hipGetLastError());
  float lh[4] = {0.f, 0.f, 0.f, 0.f};   // {loss1, loss2, norm, clip factor}
  OFX_HIP(hipMemcpyAsync(lh, loss, sizeof(float) * (C.norm() ? 4 : 2), hipMemcpyDeviceToHost, st));
  OFX_HIP(hipStreamSynchronize(st));
  if (C.loss_host) { C.loss_host[0] = lh[0]; C.loss_host[1] = lh[1]; }
  if (C.grad_norm_host) *C.grad_norm_host = lh[2];
  return ofx_policy_weights_updated(h, weights);
}

// The tail of ofx_dqn_grad, in place of fit_apply_update: this micro-batch's gradient, batch statistics and losses into
// the accumulator (t_accumulate).  Nothing of the weights, the Adam moments or a pinned blob's preparation is touched.
static int fit_accumulate(ofx_handle *h, const ofx_policy_desc &L, const FitCall &C, const float *grad,
                          const float *const *tstat, const float *const *ustat, const float *loss) {
  hipStream_t st = h->stream;
  AccSrc S;
  for (int i = 0; i < 4; i++) { S.stat[i] = tstat[i]; S.stat_n[i] = 2 * 8; }
  for (int j = 0; j < 3; j++) { S.stat[4 + j] = ustat[j]; S.stat_n[4 + j] = 2 * kUpCout[j]; }
  S.loss = loss;
  const size_t total = (size_t)L.n_floats + OFX_ACC_TAIL;
  K(t_accumulate, total, (size_t)L.n_floats, grad, S, C.acc, C.acc_reset);
  if (C.loss_host) {
    OFX_HIP(hipMemcpyAsync(C.loss_host, loss, sizeof(float) * 2, hipMemcpyDeviceToHost, st));
    OFX_HIP(hipStreamSynchronize(st));
  }
  return OFX_OK;
}

// ---- what the two drivers below run alike, kernel for kernel ----
// dense forward: f = concat(head vector, flattened p3) (next_head: the rows' next_state head - the dense targets), then the
// four dense layers on the f32 MFMA (k_gemm_f32: exact fp32 products, fp32 accumulation in MFMA order)
static int fit_dense_fwd(ofx_handle *h, const ofx_policy_desc &L, const float *w, int n, const ofx_transition *rows, int next_head,
                         const float *p3, float *f, float *d1, float *d2, float *o1, float *u0) {
  hipStream_t st = h->stream;
  auto T = [&](int t) { return w + L.offset[t]; };
  int rc;
  K(t_concat_fwd, (size_t)n * 5008, n, rows, p3, f, next_head);
  if ((rc = ofx_launch_gemm(h, f, 5008, T(OFX_T_DENSE1), 100, T(OFX_T_DENSE1 + 1), d1, 100, n, 100, 5008, 1))) return rc;
  if ((rc = ofx_launch_gemm(h, d1, 100, T(OFX_T_DENSE2), 50, T(OFX_T_DENSE2 + 1), d2, 50, n, 50, 100, 1))) return rc;
  if ((rc = ofx_launch_gemm(h, d2, 50, T(OFX_T_OUT1), 2, T(OFX_T_OUT1 + 1), o1, 2, n, 2, 50, 0))) return rc;
  return ofx_launch_gemm(h, d1, 100, T(OFX_T_UPDENSE), 625, T(OFX_T_UPDENSE + 1), u0, 625, n, 625, 100, 1);
}
// the loss of the dense targets (ofx_dqn_fit_reference): both heads' seeds, loss[0] / loss[1] from the block shares in lpart
static int fit_dense_loss(hipStream_t st, int n, const float *o1, const float *o2, const float *t1, const float *t2, float *do1,
                          float *do2, float *lpart, float *loss) {
  const size_t N = (size_t)n;
  const int nb1 = (int)((N * 2 + 255) / 256), nb2 = (int)(N * 160000 / 256 > 2048 ? 2048 : (N * 160000 + 255) / 256);
  hipLaunchKernelGGL(t_loss_dense, dim3(nb1), dim3(256), 0, st, N * 2, 1.f / (2.f * n), o1, t1, do1, lpart);
  hipLaunchKernelGGL(t_sum_ordered, dim3(1), dim3(64), 0, st, nb1, 1, lpart, loss);
  hipLaunchKernelGGL(t_loss_dense, dim3(nb2), dim3(256), 0, st, N * 160000, 1.f / (160000.f * n), o2, t2, do2, lpart + 2048);
  hipLaunchKernelGGL(t_sum_ordered, dim3(1), dim3(64), 0, st, nb2, 1, lpart + 2048, loss + 1);
  OFX_HIP(hipGetLastError());
  return OFX_OK;
}
// backward of updense (du0 = d u0 [n][625], behind u0's ReLU mask), of head 1 from its seeds do1, and of dense2, down to
// dense1's weight gradient; dd1 = d d1 is left behind its mask for the caller's d f.  g: the gradient blob
static int fit_dense_bwd(hipStream_t st, const ofx_policy_desc &L, const float *w, float *g, int n, const float *du0,
                         const float *f, const float *d1, const float *d2, const float *do1, float *dd1, float *dd2) {
  const size_t N = (size_t)n;
  auto T = [&](int t) { return w + L.offset[t]; };
  auto G = [&](int t) { return g + L.offset[t]; };
  K(t_dense_bwd_w, (size_t)26 * 157 * 8, n, 100, 625, d1, du0, G(OFX_T_UPDENSE), G(OFX_T_UPDENSE + 1));
  K(t_dense_bwd_x, ((N + 3) / 4) * 25, n, 100, 625, du0, T(OFX_T_UPDENSE), dd1, 0);
  // ---- head 1 ----
  K(t_dense_bwd_w, (size_t)32 * 8, n, 50, 2, d2, do1, G(OFX_T_OUT1), G(OFX_T_OUT1 + 1));
  K(t_dense_bwd_x, ((N + 3) / 4) * 13, n, 50, 2, do1, T(OFX_T_OUT1), dd2, 0);
  K(t_relu_mask, N * 50, N * 50, d2, dd2);
  K(t_dense_bwd_w, (size_t)26 * 13 * 8 + 255, n, 100, 50, d1, dd2, G(OFX_T_DENSE2), G(OFX_T_DENSE2 + 1));
  K(t_dense_bwd_x, ((N + 3) / 4) * 25, n, 100, 50, dd2, T(OFX_T_DENSE2), dd1, 1);
  // ---- dense1 ----
  K(t_relu_mask, N * 100, N * 100, d1, dd1);
  K(t_dense_bwd_w, (size_t)1253 * 25 * 8, n, 5008, 100, f, dd1, G(OFX_T_DENSE1), G(OFX_T_DENSE1 + 1));
  return OFX_OK;
}
// after the backward pass: ofx_dqn_grad (C.acc) stops at the gradient; else the gradient is copied out when asked for, then
// the update
static int fit_finish(ofx_handle *h, const ofx_policy_desc &L, const FitCall &C, const float *grad, const float *const *tstat,
                      const float *const *ustat, float *loss, double *npart) {
  if (C.acc) return fit_accumulate(h, L, C, grad, tstat, ustat, loss);
  if (C.grad_out) OFX_HIP(hipMemcpyAsync(C.grad_out, grad, sizeof(float) * L.n_floats, hipMemcpyDeviceToDevice, h->stream));
  return fit_apply_update(h, L, C, grad, tstat, ustat, loss, npart);
}

// The lean form of one fit step (default; ofx_fit.hip): the same graph, loss and update as dqn_fit_impl below with only
// z of every convolution in HBM.  The dense layers, the loss and Adam are the plain form's kernels.
static const int tS[4] = {400, 200, 100, 50}, uS[3] = {50, 100, 200};   // map sizes of the trunk / head-2 layers
struct LeanWs {
  float *grad, *loss, *zero, *wtr, *lpart, *weff, *gpatch, *luts, *w1t;
  double *part, *sums, *fpart, *pscratch, *cpart, *fpart2, *npart;
  float *tp[3], *tz[4], *tg[4], *tstat[4], *tact[4], *uz[3], *ug[3], *ustat[3], *uact[3];
  float *o2, *do2, *p3, *f, *d1, *d2, *o1, *u0, *gu0, *do1, *dd1, *dd2, *df, *dp3;
};
static void lean_layout(Arena &A, int n, size_t n_floats, LeanWs &W) {
  const size_t N = (size_t)n;
  W.grad = A.f(n_floats); W.loss = A.f(64); W.zero = A.f(64); W.wtr = A.f(576);   // loss, zero: adjacent, one memset clears both
  W.lpart = A.f(2 * N + 4096); W.part = A.d(ofx_fit_part_doubles()); W.sums = A.d(32); W.weff = A.f(ofx_fit_out_floats());
  W.fpart = A.d(ofx_fit_out_doubles(n)); W.pscratch = A.d(ofx_fit_point_doubles(n));
  W.gpatch = A.f(N * 128);   // textbook targets: all of the last head layer's g that is not zero
  for (int i = 0; i < 3; i++) W.tp[i] = A.f(N * 8 * tS[i + 1] * tS[i + 1]);   // pooled activation
  for (int i = 0; i < 4; i++) {   // z, g (layer 0 has neither), stat (+ the mean's low parts), act
    W.tz[i] = i ? A.f(N * 8 * tS[i] * tS[i]) : nullptr; W.tg[i] = i ? A.f(N * 8 * tS[i] * tS[i]) : nullptr; W.tstat[i] = A.f(32); W.tact[i] = A.f(16);
  }
  W.luts = A.f(ofx_fit_first_floats()); W.w1t = A.f(5008 * 100);
  W.cpart = A.d(ofx_fit_first_doubles(n)); W.fpart2 = A.d(ofx_fit_first_part_doubles(n));   // correlation, first-layers backward
  for (int j = 0; j < 3; j++) { W.uz[j] = A.f(N * kUpCout[j] * uS[j] * uS[j]); W.ug[j] = A.f(N * kUpCout[j] * uS[j] * uS[j]); W.ustat[j] = A.f(32); W.uact[j] = A.f(16); }
  W.o2 = A.f(N * 160000); W.do2 = A.f(N * 160000);
  W.p3 = A.f(N * 5000); W.f = A.f(N * 5008); W.d1 = A.f(N * 100); W.d2 = A.f(N * 50); W.o1 = A.f(N * 2); W.u0 = A.f(N * 625);
  W.gu0 = A.f(N * 625); W.do1 = A.f(N * 2); W.dd1 = A.f(N * 100); W.dd2 = A.f(N * 50); W.df = A.f(N * 5008); W.dp3 = A.f(N * 5000);
  W.npart = A.d(kNormBlocks);   // gradient-norm partials
}
static int dqn_fit_lean(ofx_handle *h, const FitCall &C) {
  const bool dense = C.t1 != nullptr;
  OFX_HIP(hipSetDevice(h->cfg.device));
  hipStream_t st = h->stream;
  ofx_policy_desc L;
  int rc = ofx_policy_layout(h, &L);
  if (rc) return rc;
  const int n = C.n;
  const ofx_transition *rows = C.rows;
  const void *bits_prev = C.bits;   // (the maps of `state`; dense targets: of next_state)
  if (!dense && (rc = refuse_pads(h, n, rows, "ofx_dqn_fit"))) return rc;   // (dense targets: ofx_dqn_fit_reference has checked)
  const size_t N = (size_t)n;
  const int legacy = h->opt_bilinear_legacy;
  LeanWs W;
  if ((rc = carve(h, &h->fitws, &h->fitws_bytes, true, "ofx_dqn_fit", [&](Arena &A) { lean_layout(A, n, (size_t)L.n_floats, W); })))
    return rc;
  auto T = [&](int t) { return C.weights + L.offset[t]; };
  auto G = [&](int t) { return W.grad + L.offset[t]; };
  OFX_HIP(hipMemsetAsync(W.grad, 0, sizeof(float) * L.n_floats, st));
  OFX_HIP(hipMemsetAsync(W.loss, 0, 2 * 256, st));   // loss and zero
  int nb = 0;
  // input of trunk layer i: the forward pools the previous layer's z on the fly and KEEPS the pooled activation (a quarter
  // of z's bytes); the weight gradient reads that plane back instead of pooling z a second time
  auto trunk_src = [&](int i, bool backward) {
    if (i == 0) return ofx_fit_src{OFX_FIT_SRC_BITS, nullptr, bits_prev, nullptr, 400, 400, legacy};
    if (backward || i == 1) return ofx_fit_src{OFX_FIT_SRC_PLANE, nullptr, W.tp[i - 1], W.zero, tS[i], tS[i], legacy};
    return ofx_fit_src{OFX_FIT_SRC_POOL, W.tp[i - 1], W.tz[i - 1], W.tact[i - 1], tS[i - 1], tS[i - 1], legacy};
  };
  auto head_src = [&](int j) {   // input of head-2 layer j (3 = the output convolution)
    return j == 0 ? ofx_fit_src{OFX_FIT_SRC_UPRAW, nullptr, W.u0, nullptr, 25, 25, legacy}
                  : ofx_fit_src{OFX_FIT_SRC_UP, nullptr, W.uz[j - 1], W.uact[j - 1], uS[j - 1], uS[j - 1], legacy};
  };

  // ---- forward (training mode) ----
  // the first layer is never materialised: statistics from the autocorrelation of the bit maps, p0 through the table kernel
  if ((rc = ofx_fit_first_fwd(h, n, bits_prev, T(ofx_t_trunk(0)), T(ofx_t_trunk(0, OFX_T_BIAS)), T(ofx_t_trunk(0, OFX_T_GAMMA)), T(ofx_t_trunk(0, OFX_T_BETA)), W.cpart, W.tstat[0], W.tact[0], W.luts, W.tp[0]))) return rc;
  for (int i = 1; i < 4; i++) {
    const int s = tS[i];
    if ((rc = ofx_fit_conv_fwd(st, n, kTrunkCin[i], 8, s, s, trunk_src(i, false), T(ofx_t_trunk(i)), T(ofx_t_trunk(i, OFX_T_BIAS)), W.tz[i], W.part, &nb))) return rc;
    if ((rc = ofx_fit_finish(st, nb, 8, (double)N * s * s, W.part, T(ofx_t_trunk(i, OFX_T_GAMMA)), T(ofx_t_trunk(i, OFX_T_BETA)), nullptr, W.tstat[i], W.tact[i]))) return rc;
  }
  if ((rc = ofx_fit_pool_act(st, n, 8, 50, 50, W.tz[3], W.tact[3], W.p3))) return rc;
  if ((rc = fit_dense_fwd(h, L, C.weights, n, rows, dense ? 1 : 0, W.p3, W.f, W.d1, W.d2, W.o1, W.u0))) return rc;
  for (int j = 0; j < 3; j++) {
    const int s = uS[j];
    if ((rc = ofx_fit_conv_fwd(st, n, kUpCin[j], kUpCout[j], s, s, head_src(j), T(ofx_t_up(j)), T(ofx_t_up(j, OFX_T_BIAS)), W.uz[j], W.part, &nb))) return rc;
    if ((rc = ofx_fit_finish(st, nb, kUpCout[j], (double)N * s * s, W.part, T(ofx_t_up(j, OFX_T_GAMMA)), T(ofx_t_up(j, OFX_T_BETA)), nullptr, W.ustat[j], W.uact[j]))) return rc;
  }
  if (dense && (rc = ofx_fit_out_fwd(st, n, head_src(3), T(OFX_T_OUT2), T(OFX_T_OUT2 + 1), W.o2, W.weff))) return rc;

  // ---- loss seeds ----
  OFX_HIP(hipMemsetAsync(W.do1, 0, N * 2 * 4, st));
  if (!dense) {
    // one error per sample on the heat map: the output convolution at the pointer only, its gradients and the last head
    // layer's g from that one pixel (ofx_fit.hip, "the top of head 2 for the textbook targets")
    float *o2p = W.o2, *d2p = W.o2 + N;                      // [n] each: the dense planes are not used on this path
    if ((rc = ofx_fit_top_point(st, n, rows, head_src(3), T(OFX_T_OUT2), T(OFX_T_OUT2 + 1), W.o1, C.y_act, C.y_ptr, W.ustat[2], o2p, W.do1, d2p, W.lpart, W.gpatch,
                                W.pscratch, W.sums, G(OFX_T_OUT2), G(OFX_T_OUT2 + 1), C.row_weight, C.td_out, C.huber_delta))) return rc;
    hipLaunchKernelGGL(t_sum_ordered, dim3(1), dim3(64), 0, st, n, 2, W.lpart, W.loss);
    OFX_HIP(hipGetLastError());
  } else if ((rc = fit_dense_loss(st, n, W.o1, W.o2, C.t1, C.t2, W.do1, W.do2, W.lpart, W.loss))) return rc;

  // ---- backward: head 2 ----
  if (dense && (rc = ofx_fit_out_bw(st, n, head_src(3), W.do2, W.part, W.fpart, G(OFX_T_OUT2), G(OFX_T_OUT2 + 1)))) return rc;
  const float *dzn = W.do2;
  for (int j = 2; j >= 0; j--) {
    const int s = uS[j];
    if (j < 2 || dense) {   // (the textbook path has the last layer's g and its sums already)
      if ((rc = ofx_fit_b1_up(st, n, kUpCout[j], kUpCout[j + 1], s, s, 1, dzn, T(ofx_t_up(j + 1)), W.uz[j], W.ustat[j], W.uact[j], legacy, W.ug[j], W.part, &nb, W.zero, W.wtr))) return rc;
      if ((rc = ofx_fit_finish(st, nb, kUpCout[j], 1.0, W.part, nullptr, nullptr, W.sums, nullptr, nullptr))) return rc;
    }
    const bool patch = j == 2 && !dense;   // (g of the last layer is a 4 x 4 patch per sample there: not read, dz written)
    if ((rc = ofx_fit_bw(st, n, kUpCin[j], kUpCout[j], s, s, head_src(j), 1, W.ug[j], W.uz[j], W.ustat[j], T(ofx_t_up(j, OFX_T_GAMMA)), W.sums, W.part,
                         G(ofx_t_up(j)), G(ofx_t_up(j, OFX_T_BIAS)), G(ofx_t_up(j, OFX_T_GAMMA)), G(ofx_t_up(j, OFX_T_BETA)), patch ? W.gpatch : nullptr,
                         patch ? rows : nullptr))) return rc;
    dzn = W.ug[j];
  }
  if ((rc = ofx_fit_b1_up(st, n, 1, 2, 25, 25, 0, dzn, T(ofx_t_up(0)), W.u0, nullptr, nullptr, legacy, W.gu0, W.part, &nb, W.zero, W.wtr))) return rc;
  // gu0 = d u0 [n][625], already behind u0's ReLU mask
  // ---- backward: updense, head 1, dense2, dense1's weights; then d f and the trunk ----
  if ((rc = fit_dense_bwd(st, L, C.weights, W.grad, n, W.gu0, W.f, W.d1, W.d2, W.do1, W.dd1, W.dd2))) return rc;
  // d f = dd1 x W1^T on the f32 MFMA GEMM (the 5008 x 100 kernel transposed first): 2 x 5008 x 100 FLOP per row
  hipLaunchKernelGGL(t_transpose, dim3((100 + 31) / 32, (5008 + 31) / 32), dim3(256), 0, st, 5008, 100, T(OFX_T_DENSE1), W.w1t);
  OFX_HIP(hipGetLastError());
  if ((rc = ofx_launch_gemm(h, W.dd1, 100, W.w1t, 5008, nullptr, W.df, 5008, n, 5008, 100, 0))) return rc;
  K(t_concat_bwd, N * 5000, n, W.df, W.dp3);
  dzn = W.dp3;
  for (int i = 3; i >= 0; i--) {
    const int s = tS[i];
    if ((rc = ofx_fit_b1_pool(st, n, s, s, i < 3, dzn, i < 3 ? T(ofx_t_trunk(i + 1)) : nullptr, W.tz[i], W.tstat[i], W.tact[i], W.tg[i], W.part, &nb, W.wtr, W.zero))) return rc;
    if ((rc = ofx_fit_finish(st, nb, 8, 1.0, W.part, nullptr, nullptr, W.sums, nullptr, nullptr))) return rc;
    if (i == 1) {
      // the first two layers: the first has neither z, g nor dz, the second's dz is never stored - only the windows that see
      // a set bit are visited (ofx_fit.hip, f_first_bwd)
      if ((rc = ofx_fit_first_bwd(st, n, bits_prev, W.tg[1], W.tz[1], W.tstat[1], T(ofx_t_trunk(1, OFX_T_GAMMA)), W.sums, T(ofx_t_trunk(1)), W.tp[0], W.luts, T(ofx_t_trunk(0)), T(ofx_t_trunk(0, OFX_T_BIAS)), W.tstat[0],
                                  T(ofx_t_trunk(0, OFX_T_GAMMA)), T(ofx_t_trunk(0, OFX_T_BETA)), W.fpart2, W.cpart, G(ofx_t_trunk(0)), G(ofx_t_trunk(0, OFX_T_BIAS)), G(ofx_t_trunk(0, OFX_T_GAMMA)), G(ofx_t_trunk(0, OFX_T_BETA)), G(ofx_t_trunk(1)), G(ofx_t_trunk(1, OFX_T_BIAS)), G(ofx_t_trunk(1, OFX_T_GAMMA)), G(ofx_t_trunk(1, OFX_T_BETA))))) return rc;
      break;
    }
    if ((rc = ofx_fit_bw(st, n, kTrunkCin[i], 8, s, s, trunk_src(i, true), 1, W.tg[i], W.tz[i], W.tstat[i], T(ofx_t_trunk(i, OFX_T_GAMMA)), W.sums, W.part,
                         G(ofx_t_trunk(i)), G(ofx_t_trunk(i, OFX_T_BIAS)), G(ofx_t_trunk(i, OFX_T_GAMMA)), G(ofx_t_trunk(i, OFX_T_BETA))))) return rc;
    dzn = W.tg[i];
  }
  return fit_finish(h, L, C, W.grad, W.tstat, W.ustat, W.loss, W.npart);
}

// The plain form of one fit step (OFX_OPT_FIT_PLAIN): every tensor of the graph in HBM, one kernel per layer and pass.
// gA / gB: two gradient scratch planes of the largest size, reused down the backward pass (as are up4 and the
// activations, once dead).
struct PlainWs {
  float *grad, *loss, *lpart;           // lpart: per-sample / per-block loss shares, summed in order
  double *sums, *spart, *wpart, *npart; // spart: t_chan_sums partials [channel][slice][2]
  float *x0, *tz[4], *ta[4], *tp[4], *tstat[4], *f, *d1, *d2, *o1, *u0, *uu[3], *uz[3], *ua[3], *ustat[3], *up4, *o2;
  float *do1, *do2, *gA, *gB, *dd1, *dd2, *df;
};
static void plain_layout(Arena &A, size_t N, size_t n_floats, PlainWs &W) {
  W.grad = A.f(n_floats); W.loss = A.f(64); W.lpart = A.f(2 * N + 4096);
  W.sums = A.d(16 * 16); W.spart = A.d(16 * 64 * 2); W.wpart = A.d((size_t)kWSlices * 600);
  W.x0 = A.f(N * 2 * 160000);
  for (int i = 0; i < 4; i++) {   // trunk: z, activation, pooled activation, batch statistics
    const size_t per = (size_t)tS[i] * tS[i];
    W.tz[i] = A.f(N * 8 * per); W.ta[i] = A.f(N * 8 * per); W.tp[i] = A.f(N * 8 * per / 4); W.tstat[i] = A.f(16);
  }
  W.f = A.f(N * 5008); W.d1 = A.f(N * 100); W.d2 = A.f(N * 50); W.o1 = A.f(N * 2); W.u0 = A.f(N * 625);
  for (int j = 0; j < 3; j++) {   // head 2: up-sampled input, z, activation, batch statistics
    const size_t per = (size_t)uS[j] * uS[j];
    W.uu[j] = A.f(N * kUpCin[j] * per); W.uz[j] = A.f(N * kUpCout[j] * per); W.ua[j] = A.f(N * kUpCout[j] * per); W.ustat[j] = A.f(16);
  }
  W.up4 = A.f(N * 8 * 160000); W.o2 = A.f(N * 160000); W.do1 = A.f(N * 2); W.do2 = A.f(N * 160000);
  W.gA = A.f(N * 8 * 160000); W.gB = A.f(N * 8 * 160000);   // gradient scratch (largest tensors)
  W.dd1 = A.f(N * 100); W.dd2 = A.f(N * 50); W.df = A.f(N * 5008); W.npart = A.d(kNormBlocks);
}
static int dqn_fit_impl(ofx_handle *h, const FitCall &C) {
  if (!h->opt_fit_plain) return dqn_fit_lean(h, C);
  const bool dense = C.t1 != nullptr;
  OFX_HIP(hipSetDevice(h->cfg.device));
  hipStream_t st = h->stream;
  ofx_policy_desc L;
  int rc = ofx_policy_layout(h, &L);
  if (rc) return rc;
  const int n = C.n;
  const ofx_transition *rows = C.rows;
  if (!dense && (rc = refuse_pads(h, n, rows, "ofx_dqn_fit"))) return rc;   // (dense targets: ofx_dqn_fit_reference has checked)
  const size_t N = (size_t)n;
  const int legacy = h->opt_bilinear_legacy;
  PlainWs W;
  if ((rc = carve(h, &h->fitws, &h->fitws_bytes, true, "ofx_dqn_fit", [&](Arena &A) { plain_layout(A, N, (size_t)L.n_floats, W); })))
    return rc;
  auto T = [&](int t) { return C.weights + L.offset[t]; };
  auto G = [&](int t) { return W.grad + L.offset[t]; };
  OFX_HIP(hipMemsetAsync(W.grad, 0, sizeof(float) * L.n_floats, st));
  OFX_HIP(hipMemsetAsync(W.loss, 0, 64 * sizeof(float), st));

  // ---- forward (training mode) ----
  K(t_bits_to_f32, N * 2 * 160000, n, (const uint32_t *)C.bits, W.x0);
  const float *tin = W.x0;
  for (int i = 0, s = 400; i < 4; i++, s /= 2) {
    const size_t per = (size_t)s * s;
    if ((rc = conv_fwd(st, n, kTrunkCin[i], 8, s, s, tin, T(ofx_t_trunk(i)), T(ofx_t_trunk(i, OFX_T_BIAS)), W.tz[i]))) return rc;
    hipLaunchKernelGGL(t_chan_sums, dim3(8, 64), dim3(256), 0, st, n, 8, per, W.tz[i], (const float *)nullptr, W.spart);
    hipLaunchKernelGGL(t_chan_sums_finish, dim3(1), dim3(64), 0, st, 8, 64, W.spart, W.sums);
    hipLaunchKernelGGL(t_bn_finish_stats, dim3(1), dim3(64), 0, st, 8, (double)N * (double)per, W.sums, W.tstat[i]);
    hipLaunchKernelGGL(t_bn_relu_fwd, PLANES(per, n * 8), 0, st, 8, per, W.tz[i], W.tstat[i], T(ofx_t_trunk(i, OFX_T_GAMMA)), T(ofx_t_trunk(i, OFX_T_BETA)), W.ta[i]);
    K(t_pool_fwd, N * 8 * per / 4, n * 8, s, s, W.ta[i], W.tp[i]);
    tin = W.tp[i];
  }
  if ((rc = fit_dense_fwd(h, L, C.weights, n, rows, dense ? 1 : 0, W.tp[3], W.f, W.d1, W.d2, W.o1, W.u0))) return rc;
  const float *uin = W.u0;
  for (int j = 0, s = 50; j < 3; j++, s *= 2) {
    const size_t per = (size_t)s * s;
    K(t_up_fwd, N * kUpCin[j] * per, n * kUpCin[j], s / 2, s / 2, uin, W.uu[j], legacy);
    if ((rc = conv_fwd(st, n, kUpCin[j], kUpCout[j], s, s, W.uu[j], T(ofx_t_up(j)), T(ofx_t_up(j, OFX_T_BIAS)), W.uz[j]))) return rc;
    hipLaunchKernelGGL(t_chan_sums, dim3(kUpCout[j], 64), dim3(256), 0, st, n, kUpCout[j], per, W.uz[j], (const float *)nullptr, W.spart);
    hipLaunchKernelGGL(t_chan_sums_finish, dim3(1), dim3(64), 0, st, kUpCout[j], 64, W.spart, W.sums);
    hipLaunchKernelGGL(t_bn_finish_stats, dim3(1), dim3(64), 0, st, kUpCout[j], (double)N * (double)per, W.sums, W.ustat[j]);
    hipLaunchKernelGGL(t_bn_relu_fwd, PLANES(per, n * kUpCout[j]), 0, st, kUpCout[j], per, W.uz[j], W.ustat[j], T(ofx_t_up(j, OFX_T_GAMMA)), T(ofx_t_up(j, OFX_T_BETA)), W.ua[j]);
    uin = W.ua[j];
  }
  K(t_up_fwd, N * 8 * 160000, n * 8, 200, 200, W.ua[2], W.up4, legacy);
  if ((rc = conv_fwd(st, n, 8, 1, 400, 400, W.up4, T(OFX_T_OUT2), T(OFX_T_OUT2 + 1), W.o2))) return rc;

  // ---- loss seeds ----
  OFX_HIP(hipMemsetAsync(W.do1, 0, N * 2 * 4, st));
  OFX_HIP(hipMemsetAsync(W.do2, 0, N * 160000 * 4, st));
  if (dense) {
    if ((rc = fit_dense_loss(st, n, W.o1, W.o2, C.t1, C.t2, W.do1, W.do2, W.lpart, W.loss))) return rc;
  } else {
    K(t_loss_seed, N, n, rows, W.o1, W.o2, C.y_act, C.y_ptr, W.do1, W.do2, W.lpart, C.row_weight, C.td_out, C.huber_delta);
    hipLaunchKernelGGL(t_sum_ordered, dim3(1), dim3(64), 0, st, n, 2, W.lpart, W.loss);
  }

  // ---- backward: head 2 ----
  conv_bwd_weight(st, n, 8, 1, 400, 400, W.up4, W.do2, W.wpart, G(OFX_T_OUT2), G(OFX_T_OUT2 + 1));
  if ((rc = conv_bwd_data(st, n, 8, 1, 400, 400, W.do2, T(OFX_T_OUT2), W.gA))) return rc;   // d up4
  float *dcur = W.gB;                                                          // d W.ua[2]
  K(t_up_bwd, N * 8 * 40000, n * 8, 200, 200, W.gA, dcur, legacy);
  for (int j = 2, s = 200; j >= 0; j--, s /= 2) {
    const size_t per = (size_t)s * s;
    float *xh = W.gA;                                                          // reuse as xhat
    hipLaunchKernelGGL(t_bn_relu_bwd_pre, PLANES(per, n * kUpCout[j]), 0, st, kUpCout[j], per, W.uz[j], W.ua[j], W.ustat[j], dcur, xh);
    hipLaunchKernelGGL(t_chan_sums, dim3(kUpCout[j], 64), dim3(256), 0, st, n, kUpCout[j], per, dcur, xh, W.spart);
    hipLaunchKernelGGL(t_chan_sums_finish, dim3(1), dim3(64), 0, st, kUpCout[j], 64, W.spart, W.sums);
    float *dz = W.ua[j];                                                       // the activation is dead now: holds dz
    hipLaunchKernelGGL(t_bn_bwd, PLANES(per, n * kUpCout[j]), 0, st, kUpCout[j], per, (double)N * (double)per, dcur, xh, W.ustat[j], T(ofx_t_up(j, OFX_T_GAMMA)), W.sums, dz, G(ofx_t_up(j, OFX_T_GAMMA)), G(ofx_t_up(j, OFX_T_BETA)));
    conv_bwd_weight(st, n, kUpCin[j], kUpCout[j], s, s, W.uu[j], dz, W.wpart, G(ofx_t_up(j)), G(ofx_t_up(j, OFX_T_BIAS)));
    float *duu = W.gA;                                                         // d (upsampled input)
    if ((rc = conv_bwd_data(st, n, kUpCin[j], kUpCout[j], s, s, dz, T(ofx_t_up(j)), duu))) return rc;
    float *dprev = W.gB;                                                       // d (previous activation / u0)
    K(t_up_bwd, N * kUpCin[j] * per / 4, n * kUpCin[j], s / 2, s / 2, duu, dprev, legacy);
    dcur = dprev;
  }
  // dcur = d u0 [n][625] (pre-mask)
  K(t_relu_mask, N * 625, N * 625, W.u0, dcur);
  // ---- backward: updense, head 1, dense2, dense1's weights; then d f and the trunk ----
  if ((rc = fit_dense_bwd(st, L, C.weights, W.grad, n, dcur, W.f, W.d1, W.d2, W.do1, W.dd1, W.dd2))) return rc;
  K(t_dense_bwd_x, ((N + 3) / 4) * 1252, n, 5008, 100, W.dd1, T(OFX_T_DENSE1), W.df, 0);
  float *dp = W.gB;
  K(t_concat_bwd, N * 5000, n, W.df, dp);                                    // d W.tp[3] [n][8][25][25]
  for (int i = 3, s = 50; i >= 0; i--, s *= 2) {
    const size_t per = (size_t)s * s, tot = N * 8 * per;
    float *da = W.gA;
    K(t_pool_bwd, tot / 4, n * 8, s, s, W.ta[i], dp, da);
    float *xh = W.gB + N * 8 * 40000;                                          // second half of W.gB (>= N*8*per for s <= 200)
    if (s == 400) xh = W.up4;                                                // the 400^2 layer: up4 (8 x 400^2) is dead by now
    hipLaunchKernelGGL(t_bn_relu_bwd_pre, PLANES(per, n * 8), 0, st, 8, per, W.tz[i], W.ta[i], W.tstat[i], da, xh);
    hipLaunchKernelGGL(t_chan_sums, dim3(8, 64), dim3(256), 0, st, n, 8, per, da, xh, W.spart);
    hipLaunchKernelGGL(t_chan_sums_finish, dim3(1), dim3(64), 0, st, 8, 64, W.spart, W.sums);
    float *dz = W.ta[i];
    hipLaunchKernelGGL(t_bn_bwd, PLANES(per, n * 8), 0, st, 8, per, (double)N * (double)per, da, xh, W.tstat[i], T(ofx_t_trunk(i, OFX_T_GAMMA)), W.sums, dz, G(ofx_t_trunk(i, OFX_T_GAMMA)), G(ofx_t_trunk(i, OFX_T_BETA)));
    const float *xin = i == 0 ? W.x0 : W.tp[i - 1];
    conv_bwd_weight(st, n, kTrunkCin[i], 8, s, s, xin, dz, W.wpart, G(ofx_t_trunk(i)), G(ofx_t_trunk(i, OFX_T_BIAS)));
    if (i > 0) {
      dp = W.gB;                                                               // d W.tp[i-1] [n][8][s][s]
      if ((rc = conv_bwd_data(st, n, 8, 8, s, s, dz, T(ofx_t_trunk(i)), dp))) return rc;
    }
  }
  return fit_finish(h, L, C, W.grad, W.tstat, W.ustat, W.loss, W.npart);
}

// The null / range checks the five fit entries share.  `update`: the call ends in the Adam update (moments and a step
// number are needed); `sparse`: it takes y_act / y_ptr; `own`: the entry's further pointers are all there.
static int fit_check(const ofx_handle *h, const FitCall &C, const char *who, bool update, bool sparse, bool own = true) {
  if (!h || !C.weights || !C.rows || !C.bits || C.n < 1 || !own || (update && (!C.adam_m || !C.adam_v || C.step < 1)) ||
      (sparse && (!C.y_act || !C.y_ptr))) { ofx_set_error("%s: bad argument", who); return OFX_ERR_INVALID; }
  return OFX_OK;
}
static bool finite_nonneg(float x) { return x >= 0.f && x <= FLT_MAX; }   // NaN fails the first comparison, infinity the second

// The sparse-target call of ofx_dqn_fit, _weighted, _robust and ofx_dqn_grad: what the four take in common; an entry adds
// what is its own
static FitCall sparse_call(float *weights, float *adam_m, float *adam_v, int32_t step, float lr, int32_t n,
                           const ofx_transition *rows, const void *bits_prev, const float *y_act, const float *y_ptr,
                           float *grad_out, float *loss_host, const float *row_weight = nullptr, float *td_out = nullptr,
                           float huber_delta = 0.f) {
  FitCall C;
  C.weights = weights; C.adam_m = adam_m; C.adam_v = adam_v; C.step = step; C.lr = lr; C.n = n; C.rows = rows;
  C.bits = bits_prev; C.y_act = y_act; C.y_ptr = y_ptr; C.grad_out = grad_out; C.loss_host = loss_host;
  C.row_weight = row_weight; C.td_out = td_out; C.huber_delta = huber_delta;
  return C;
}

extern "C" int ofx_dqn_fit(ofx_handle *h, float *weights, float *adam_m, float *adam_v, int32_t step, float lr, int32_t n,
                           const ofx_transition *rows, const void *bits_prev, const float *y_act, const float *y_ptr,
                           float *grad_out, float *loss_host) {
  const FitCall C = sparse_call(weights, adam_m, adam_v, step, lr, n, rows, bits_prev, y_act, y_ptr, grad_out, loss_host);
  const int rc = fit_check(h, C, "ofx_dqn_fit", true, true);
  return rc ? rc : dqn_fit_impl(h, C);
}

// ofx_dqn_fit with Keras sample_weight semantics (prioritized replay's importance-sampling weights): the loss is
// sum w e1^2 / (2 n) + sum w e2^2 / (160000 n); row_weight null = ofx_dqn_fit bit for bit (so is a weight of 1.0).
extern "C" int ofx_dqn_fit_weighted(ofx_handle *h, float *weights, float *adam_m, float *adam_v, int32_t step, float lr,
                                    int32_t n, const ofx_transition *rows, const void *bits_prev, const float *y_act,
                                    const float *y_ptr, float *grad_out, float *loss_host, const float *row_weight,
                                    float *td_out) {
  const FitCall C = sparse_call(weights, adam_m, adam_v, step, lr, n, rows, bits_prev, y_act, y_ptr, grad_out, loss_host,
                                row_weight, td_out);
  const int rc = fit_check(h, C, "ofx_dqn_fit_weighted", true, true);
  return rc ? rc : dqn_fit_impl(h, C);
}

// ofx_dqn_fit_weighted with the error bounded by Huber(huber_delta) and the gradient clipped to a global norm of
// clip_norm before Adam; 0 switches either off, and with both off and no grad_norm_host this is ofx_dqn_fit_weighted.
extern "C" int ofx_dqn_fit_robust(ofx_handle *h, float *weights, float *adam_m, float *adam_v, int32_t step, float lr,
                                  int32_t n, const ofx_transition *rows, const void *bits_prev, const float *y_act,
                                  const float *y_ptr, float *grad_out, float *loss_host, const float *row_weight,
                                  float *td_out, float huber_delta, float clip_norm, float *grad_norm_host) {
  FitCall C = sparse_call(weights, adam_m, adam_v, step, lr, n, rows, bits_prev, y_act, y_ptr, grad_out, loss_host, row_weight,
                          td_out, huber_delta);
  C.clip_norm = clip_norm; C.grad_norm_host = grad_norm_host;
  const int rc = fit_check(h, C, "ofx_dqn_fit_robust", true, true);
  if (rc) return rc;
  if (!finite_nonneg(huber_delta) || !finite_nonneg(clip_norm)) {
    ofx_set_error("ofx_dqn_fit_robust: huber_delta and clip_norm must be finite and >= 0 (0 = off), got %g and %g",
                  (double)huber_delta, (double)clip_norm);
    return OFX_ERR_INVALID;
  }
  return dqn_fit_impl(h, C);
}

// The split fit.  ofx_dqn_grad is ofx_dqn_fit_robust up to and including the backward pass - the same driver in its
// gradient-only mode (C.acc) - and ofx_dqn_apply is fit_apply_update on an accumulator (C.tail): include/ofx.h.
extern "C" int32_t ofx_dqn_acc_floats(const ofx_handle *h) {
  ofx_policy_desc L;
  if (!h || ofx_policy_layout(h, &L)) return -1;
  return L.n_floats + OFX_ACC_TAIL;
}

extern "C" int ofx_dqn_grad(ofx_handle *h, const float *weights, int32_t n, const ofx_transition *rows,
                            const void *bits_prev, const float *y_act, const float *y_ptr, const float *row_weight,
                            float *td_out, float huber_delta, float *acc, int32_t reset, float *loss_host) {
  // (the drivers read the blob and hand it on to fit_apply_update alone, which this mode never reaches: no moments, step
  // and rate at FitCall's defaults)
  FitCall C = sparse_call(const_cast<float *>(weights), nullptr, nullptr, 1, 0.f, n, rows, bits_prev, y_act, y_ptr, nullptr,
                          loss_host, row_weight, td_out, huber_delta);
  C.acc = acc; C.acc_reset = reset != 0;
  const int rc = fit_check(h, C, "ofx_dqn_grad", false, true, acc != nullptr);
  if (rc) return rc;
  if (!finite_nonneg(huber_delta)) {
    ofx_set_error("ofx_dqn_grad: huber_delta must be finite and >= 0 (0 = off), got %g", (double)huber_delta);
    return OFX_ERR_INVALID;
  }
  return dqn_fit_impl(h, C);
}

struct ApplyWs { float *loss; double *npart; };   // {loss1, loss2, norm, factor} and the norm's block partials
static void apply_layout(Arena &A, ApplyWs &W) { W.loss = A.f(64); W.npart = A.d(kNormBlocks); }

extern "C" int ofx_dqn_apply(ofx_handle *h, float *weights, float *adam_m, float *adam_v, int32_t step, float lr,
                             const float *acc, float scale, float clip_norm, float *loss_host, float *grad_norm_host) {
  if (!h || !weights || !adam_m || !adam_v || !acc || step < 1) {
    ofx_set_error("ofx_dqn_apply: bad argument");
    return OFX_ERR_INVALID;
  }
  if (!(scale > 0.f && scale <= FLT_MAX) || !finite_nonneg(clip_norm)) {
    ofx_set_error("ofx_dqn_apply: scale must be finite and > 0, clip_norm finite and >= 0 (0 = off), got %g and %g",
                  (double)scale, (double)clip_norm);
    return OFX_ERR_INVALID;
  }
  OFX_HIP(hipSetDevice(h->cfg.device));
  ofx_policy_desc L;
  int rc = ofx_policy_layout(h, &L);
  if (rc) return rc;
  // a block of its own, so the fit's workspace stays as the last ofx_dqn_grad sized it
  ApplyWs W;
  if ((rc = carve(h, &h->applyws, &h->applyws_bytes, false, "ofx_dqn_apply", [&](Arena &A) { apply_layout(A, W); }))) return rc;
  const float *tail = acc + L.n_floats, *tstat[4], *ustat[3];
  for (int i = 0; i < 4; i++) tstat[i] = tail + OFX_ACC_STAT_FLOATS * i;
  for (int j = 0; j < 3; j++) ustat[j] = tail + OFX_ACC_STAT_FLOATS * (4 + j);
  FitCall C;
  C.weights = weights; C.adam_m = adam_m; C.adam_v = adam_v; C.step = step; C.lr = lr; C.loss_host = loss_host;
  C.clip_norm = clip_norm; C.grad_norm_host = grad_norm_host; C.tail = tail; C.scale = scale;
  return fit_apply_update(h, L, C, acc, tstat, ustat, W.loss, W.npart);
}

// Trainer.replay's loop body and fit exactly as written (agents/qlearnIA_V2.py:251-285), quirks included:
//   [target, ptr_target]         = predict(state)                                   (:266, inference-mode BatchNorm)
//   [prediction, ptr_prediction] = predict(next_state)                              (:274)
//   target[iaction]      = reward + gamma max(prediction)     int(not done)         (:279)
//   ptr_target[ipointer] = reward + gamma max(ptr_prediction) int(not done)         (:280) - ipointer = (x, y) indexes
//                          the (400, 400, 1) prediction as [x][y]: row x, column y, the transpose of the pixel that
//                          get_best_action's unravel_index(order='F') named
//   inputs1[i] = img_input (re-bound to NEXT_state's maps at :273), inputs2[i] = next_obs.vector[:8]     (:282-283)
//   fit(x = inputs, y = [target, ptr_target]): training-mode forward on next_state against targets built from state
// so every output element carries an error, not one per head.
struct RefWs { float *vec_prev, *vec_next, *act_next, *max_next, *t1, *t2; };
static void ref_layout(Arena &A, size_t N, RefWs &W) {
  W.vec_prev = A.f(8 * N); W.vec_next = A.f(8 * N); W.act_next = A.f(2 * N); W.max_next = A.f(N);
  W.t1 = A.f(2 * N); W.t2 = A.f(N * TPS * TPS);
}
extern "C" int ofx_dqn_fit_reference(ofx_handle *h, float *weights, float *adam_m, float *adam_v, int32_t step, float lr,
                                     int32_t n, const ofx_transition *rows, const void *bits_prev, const void *bits_next,
                                     float gamma, float *grad_out, float *loss_host) {
  FitCall C;
  C.weights = weights; C.adam_m = adam_m; C.adam_v = adam_v; C.step = step; C.lr = lr;
  C.n = n; C.rows = rows; C.bits = bits_next; C.grad_out = grad_out; C.loss_host = loss_host;
  int rc = fit_check(h, C, "ofx_dqn_fit_reference", true, false, bits_prev != nullptr);
  if (rc) return rc;
  OFX_HIP(hipSetDevice(h->cfg.device));
  hipStream_t st = h->stream;
  if ((rc = refuse_pads(h, n, rows, "ofx_dqn_fit_reference"))) return rc;  // before the two predict passes
  const size_t N = (size_t)n;
  RefWs W;
  if ((rc = carve(h, &h->fitws2, &h->fitws2_bytes, true, "ofx_dqn_fit_reference", [&](Arena &A) { ref_layout(A, N, W); }))) return rc;
  K(k_dqn_unpack, N, n, rows, W.vec_prev, W.vec_next, (int32_t *)nullptr);   // (padding rows were refused above)
  if ((rc = ofx_policy_predict_obs(h, weights, n, bits_prev, W.vec_prev, W.t1, W.t2, nullptr))) return rc;
  if ((rc = ofx_policy_predict_obs(h, weights, n, bits_next, W.vec_next, W.act_next, nullptr, W.max_next))) return rc;
  K(t_reference_targets, N, n, rows, gamma, W.act_next, W.max_next, W.t1, W.t2);
  C.t1 = W.t1; C.t2 = W.t2;
  return dqn_fit_impl(h, C);
}
