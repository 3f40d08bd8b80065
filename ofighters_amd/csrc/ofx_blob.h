// ofx_blob.h - the user's weight blob of the bi-head policy, described once (host only): the order of its 52 tensors,
// the channel tables and the offsets (identical to oracle/policy_oracle.c and agents/policy_weights.py layout()).
#pragma once
#include <stdint.h>

// a conv + BatchNorm layer is six consecutive tensors; dense layers and the output convolution are a kernel and a bias
enum { OFX_T_KERNEL, OFX_T_BIAS, OFX_T_GAMMA, OFX_T_BETA, OFX_T_MEAN, OFX_T_VAR, OFX_T_PER_CONV };
constexpr int OFX_T_DENSE1 = 24, OFX_T_DENSE2 = 26, OFX_T_OUT1 = 28, OFX_T_UPDENSE = 30, OFX_T_UP = 32, OFX_T_OUT2 = 50,
              OFX_T_COUNT = 52;
constexpr int ofx_t_trunk(int i, int part = OFX_T_KERNEL) { return OFX_T_PER_CONV * i + part; }       // conv1..4: i = 0..3
constexpr int ofx_t_up(int j, int part = OFX_T_KERNEL) { return OFX_T_UP + OFX_T_PER_CONV * j + part; }  // upconv1..3: j = 0..2
static_assert(ofx_t_trunk(4) == OFX_T_DENSE1 && OFX_T_DENSE2 == OFX_T_DENSE1 + 2 && OFX_T_OUT1 == OFX_T_DENSE2 + 2 &&
              OFX_T_UPDENSE == OFX_T_OUT1 + 2 && OFX_T_UP == OFX_T_UPDENSE + 2 && ofx_t_up(3) == OFX_T_OUT2 &&
              OFX_T_OUT2 + 2 == OFX_T_COUNT, "tensor order of the blob");

// false for the moving mean / variance of the BatchNorm layers: Adam leaves them alone, the fit moves them itself
constexpr bool ofx_blob_trained(int t) {
  const int part = t < OFX_T_DENSE1 ? t % OFX_T_PER_CONV : t >= OFX_T_UP && t < OFX_T_OUT2 ? (t - OFX_T_UP) % OFX_T_PER_CONV : 0;
  return part != OFX_T_MEAN && part != OFX_T_VAR;
}

static const int kTrunkCin[4] = {2, 8, 8, 8};  // every trunk layer has 8 output channels
static const int kUpCin[4] = {1, 2, 4, 8};     // upconv1..3 and the output convolution
static const int kUpCout[4] = {2, 4, 8, 1};

// offset[t], count[t] of tensor t in floats, offset[n] = the blob's size; returns n = OFX_T_COUNT
static inline int policy_layout(int32_t *offset, int32_t *count) {
  int n = 0, off = 0;
#define T(c) do { offset[n] = off; count[n] = (c); off += (c); n++; } while (0)
  for (int i = 0; i < 4; i++) { T(9 * kTrunkCin[i] * 8); T(8); T(8); T(8); T(8); T(8); }
  T(5008 * 100); T(100);
  T(100 * 50); T(50);
  T(50 * 2); T(2);
  T(100 * 625); T(625);
  for (int i = 0; i < 3; i++) { int co = kUpCout[i]; T(9 * kUpCin[i] * co); T(co); T(co); T(co); T(co); T(co); }
  T(9 * 8 * 1); T(1);
#undef T
  offset[n] = off;
  return n;
}
