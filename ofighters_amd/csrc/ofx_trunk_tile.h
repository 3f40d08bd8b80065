// ofx_trunk_tile.h - the M-tile of the trunk's banded GEMM (ofx_trunk.hip: k_convm, k_trunk12, k_conv3_stream), each
// piece stated once: where a lane's A operands sit in the LDS tile (taps), the matrix sequence over one, two or four
// interleaved accumulators (chain), the 2x2 pool + ReLU of the result (pool), the flat enumeration of M-tiles of the
// streaming kernels (MtFlat) and the value all of that gives on a constant window (mt_const).  The forms that must agree
// bit for bit (sparse == dense, streaming == per-layer, K2 / K3 == a tile that ran) agree because they call these.
#pragma once
#include "ofx_lowp.h"

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));

// max without the canonicalising v_max(x, x) the compiler puts in front of fmaxf() in IEEE mode (x is an MFMA
// result here, never a signalling NaN): med3(x, floor, +inf).  NOT inline assembly: the compiler's hazard recogniser
// does not look inside an asm statement, so an asm v_max placed right behind the MFMA that produces x reads the
// register before the matrix pipe has written it (seen as wrong cells under one scheduling variant).
// The +inf comes out of an opaque scalar move: with a literal the optimiser folds med3 back into the canonicalising max.
__device__ __forceinline__ float max_raw(float x, float floor) {
  float pinf;
  asm("s_mov_b32 %0, 0x7f800000" : "=s"(pinf));
  return __builtin_amdgcn_fmed3f(x, floor, pinf);
}

// ---- taps: the LDS offsets of a lane's A operands relative to a = abase + the M-tile's origin, in a tile of 8 channel
// planes PLS apart with rows LS apart.  abase = the lane's k-quarter plane (+ kq * PLS) at column -1 of tile row 0.
// fp32 (24 MFMAs of K = 4; MFMA j, lane kq: k = 4 j + kq): the (row, dx) of step j is a compile-time constant and the
// channel is 4 (j & 1) + kq, so every LDS read is base + immediate.
template <int LS, int PLS>
__device__ __forceinline__ constexpr int mt_aof(int j) {
  return (4 * (j & 1)) * PLS + ((j >> 1) / 3) * LS + ((j >> 1) % 3);
}
// 16-bit (6 MFMAs of K = 16; MFMA J, lane kq, element i: tap 2 J + (kq >> 1), channel 4 (kq & 1) + i): one address per J,
// lane-constant tap offset, the four planes by immediate.  abase carries the fp32 form's + kq * PLS: taken out again.
template <int LS, int PLS>
__device__ __forceinline__ void mt_toff(int kq, int (&toff)[6]) {
#pragma unroll
  for (int J = 0; J < 6; J++) {
    const int tap = 2 * J + (kq >> 1);
    toff[J] = (4 * (kq & 1) - kq) * PLS + (tap / 3) * LS + tap % 3;
  }
}

// ---- chain: the M-tile's matrix sequence for one, two or four interleaved accumulators (independent chains keep the
// matrix pipe busy): the MFMA index is the outer loop, the chain the inner one.  LP 0: fp32 operands, the lane's B operand
// of MFMA j at bw[j * BS] (24 registers, or BS = 64: straight out of a [24][64] array); LP 1 / 2: bf16 / fp16 operands
// rounded on the way in (ofx_lowp.h), B in bwb[6], taps in toff (mt_toff; not read for LP 0).
// mt_step is MFMA j of every chain; the loop over j stands at the call site,
//   #pragma unroll
//   for (int j = 0; j < MT_NJ<LP>; j++) mt_step<LP, LS, PLS>(j, bw, bwb, toff, MtAcc{a0, d0}, MtAcc{a1, d1});
// because with the loop inside a function the compiler's early passes meet a call where the kernels had a loop, and
// k_convm's code comes out different (the forms are compared instruction by instruction when this file changes).
struct MtAcc {      // one chain:
  const float *a;   // the lane's A row at the M-tile's origin
  f32x4 &d;         // the caller's accumulator, bias in
};
template <int LP>
constexpr int MT_NJ = LP ? 6 : 24;  // MFMAs of an M-tile
template <int LP, int LS, int PLS, int BS = 1, typename... Acc>
__device__ __forceinline__ void mt_step(int j, const float *bw, const lp_x4 (&bwb)[6], const int (&toff)[6], Acc... t) {
  static_assert(sizeof...(Acc) == 1 || sizeof...(Acc) == 2 || sizeof...(Acc) == 4, "one, two or four accumulator chains");
  if constexpr (LP != 0) {
    auto pk = [&](const float *q) { return lp_pk4<LP ? LP : 1>(q[0], q[PLS], q[2 * PLS], q[3 * PLS]); };
    const lp_x4 A[] = {pk(t.a + toff[j])...};
    int c = 0;
    ((t.d = lp_mfma16<LP ? LP : 1>(A[c++], bwb[j], t.d)), ...);
  } else {
    ((t.d = __builtin_amdgcn_mfma_f32_16x16x4f32(t.a[mt_aof<LS, PLS>(j)], bw[LP ? 0 : j * BS], t.d, 0, 0, 0)), ...);
  }
}

// ---- pool: the epilogue of an M-tile.  Lane (n = (co, r), kq) holds pixels 4 kq .. 4 kq + 3 of conv row r: x-pool +
// ReLU (two v_med3: compiler-visible reads of the MFMA result, see max_raw), y-pool = max with the DPP quad swap
// [1,0,3,2] (rows r = 0 / 1 sit in lanes n, n ^ 1).  Returns the lane's two pooled pixels; the r = 0 lanes store them.
__device__ __forceinline__ f32x2 mt_pool(const f32x4 d) {
  float q0, q1;
  q0 = max_raw(max_raw(d[0], 0.f), d[1]);
  q1 = max_raw(max_raw(d[2], 0.f), d[3]);
  q0 = max_raw(q0, __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, q0), 0xB1, 0xF, 0xF, true)));
  q1 = max_raw(q1, __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, q1), 0xB1, 0xF, 0xF, true)));
  return (f32x2){q0, q1};
}

// ---- the constant of a constant window: the pooled value the kernel's own sequence gives on an M-tile whose whole
// window holds constant planes.  a = the lane's A row of any interior M-tile of a tile filled with them; every lane
// of a channel returns the same value.  The same sequence as a tile that runs, hence the same bits.
template <int LP, int LS, int PLS, int BS = 1>
__device__ __forceinline__ float mt_const(const float *a, const float *bw, const lp_x4 (&bwb)[6], int kq, const f32x4 binit) {
  int toff[6];
  mt_toff<LS, PLS>(kq, toff);
  f32x4 d = binit;
#pragma unroll
  for (int j = 0; j < MT_NJ<LP>; j++) mt_step<LP, LS, PLS, BS>(j, bw, bwb, toff, MtAcc{a, d});
  return mt_pool(d)[0];
}

// ---- flat M-tiles of the streaming kernels: an LDS tile of RP row pairs x WD columns, M-tiles of 16 pixels enumerated
// FLAT over (row pair, column): NT = RP * WD / 16 of them, no masked columns.  Output: planar rows of WD / 2 pooled
// pixels, orow = the lane's channel plane at the step's first pooled row.
template <int WD, int RP, int LS>
struct MtFlat {
  static constexpr int NPX = RP * WD, NT = (NPX + 15) / 16;
  static_assert(WD % 4 == 0 && NT <= 64, "four M-tiles per wave at most");
  // the lane's A row: pixel 16 T + n16 (clamped past the end)
  static __device__ __forceinline__ const float *a_of_tile(const float *abase, int T, int n16) {
    const int P = min(16 * T + n16, NPX - 1);
    const int rp = P / WD, x = P - rp * WD;
    return abase + 2 * rp * LS + x;
  }
  // one 8-byte store from the r = 0 lanes: the lane's two pooled pixels of tile T (its four pixels P .. P + 3 sit in one
  // row pair).  INSIDE: the tile is known to end inside the step (a constant tile does)
  template <bool INSIDE = false>
  static __device__ __forceinline__ void store(float *orow, int T, int kq, int r, float q0, float q1) {
    const int P = 16 * T + 4 * kq;
    const int rp = P / WD, x = P - rp * WD;
    if (r == 0 && (INSIDE || P < NPX)) *reinterpret_cast<float2 *>(orow + rp * (WD / 2) + (x >> 1)) = make_float2(q0, q1);
  }
  // epilogue of a tile that ran: pool + ReLU, store
  static __device__ __forceinline__ void finish(const f32x4 d, float *orow, int T, int kq, int r) {
    const f32x2 q = mt_pool(d);
    store(orow, T, kq, r, q[0], q[1]);
  }
};
