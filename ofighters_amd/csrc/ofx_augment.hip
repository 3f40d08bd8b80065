// ofx_augment.hip - symmetry augmentation of stored observations (include/ofx.h, "symmetry augmentation (opt-in)"):
// the eight isometries of the square applied in place to 1-bit maps, observation heads and pointers.
//
// One workgroup per observation.  The two maps (2 * words uint32, 40 KB at 400 x 400) are staged in LDS with 16-byte
// loads, a barrier follows, and every output word is then formed from LDS and written back over the input with 16-byte
// stores: nothing outside the observation's 2 * words words is read or written, and no other workgroup touches them.
//  - Without the transpose bit an output word is a run of source pixels of one or more source rows (one row boundary
//    at the most while W >= 32): per row segment a forward run, or a bit-reversed one under FLIP_X, taken with a funnel
//    shift over two neighbouring LDS words.  A row is W / 32 = 12.5 words at W = 400: no run is word-aligned.
//  - With the transpose bit the 32 pixels of an output word come from 32 source rows: the plain 32-read gather.  Read in
//    output order, neighbouring lanes would be 128 output pixels = 128 source rows = 1600 LDS words apart - one bank for
//    the whole wave.  So the lanes walk the uint4s in a permuted order: S = W / gcd(W, 128) uint4s are a whole number of
//    output rows (25 uint4s = 8 rows at W = 400), and lane l takes uint4 l * S + c: the lanes of a wave then read the
//    same source row at source columns 8 apart, four lanes per LDS word (a broadcast) and consecutive words beyond.
// The head and pointer arithmetic is lane 0's.
#include "ofx_internal.h"
#include <string.h>

#define OFX_LDS_LIMIT (64 * 1024) /* the budget of the packed readers (ofx_replay.hip): a frame's two maps in LDS */

struct AugmentParams {
  int W, H, words;
  uint32_t *bits[2];     // [n][2][words]: prev / next of ofx_replay_augment; [0] alone for ofx_obs_transform
  ofx_transition *rows;  // DRAW: [n]
  float *vec8;           // !DRAW: [n][8] or null
  int32_t *pointer;      // !DRAW: [n][2] or null
  const uint8_t *op;     // !DRAW: [n]
  uint8_t *op_out;       // DRAW: [n] or null
  ofx_rng_key key;
  uint32_t draw, first, arena_base, mask;
  int perm_s, perm_g;    // the transposed walk's permutation (uint4s per map = perm_s * perm_g), perm_s == 0: none
};

// pixels p .. p + len - 1 of a map (1 <= len <= 32, all inside it) in bits 0 .. len - 1
__device__ __forceinline__ uint32_t sym_run(const uint32_t *map, int words, int p, int len) {
  const int w = p >> 5;
  const uint32_t lo = map[w], hi = w + 1 < words ? map[w + 1] : 0u;
  const uint32_t v = (uint32_t)((((uint64_t)hi << 32) | lo) >> (p & 31));
  return len == 32 ? v : v & ((1u << len) - 1u);
}

// output word k of a map under element g without the transpose bit
__device__ __forceinline__ uint32_t sym_word_flip(const uint32_t *map, int W, int H, int words, int g, int k) {
  int y = (32 * k) / W, x = 32 * k - y * W;
  uint32_t out = 0u;
  for (int pos = 0; pos < 32;) {
    const int len = min(32 - pos, W - x);
    const int sy = (g & OFX_SYM_FLIP_Y) ? H - 1 - y : y;
    uint32_t v;
    if (g & OFX_SYM_FLIP_X) v = __brev(sym_run(map, words, sy * W + (W - x - len), len)) >> (32 - len);
    else v = sym_run(map, words, sy * W + x, len);
    out |= v << pos;
    pos += len;
    x = 0;
    y++;
  }
  return out;
}

// output word k of a map under element g with the transpose bit (W == H): out[y'][x'] = in[x1][y1], (x1, y1) = the
// output position with the flips undone
__device__ __forceinline__ uint32_t sym_word_transpose(const uint32_t *map, int W, int g, int k) {
  int y = (32 * k) / W, x = 32 * k - y * W;
  const int dp = (g & OFX_SYM_FLIP_X) ? -W : W;  // one output pixel further along a row is one source row further
  uint32_t out = 0u;
  for (int pos = 0; pos < 32;) {  // per output row the word touches, as in sym_word_flip
    const int len = min(32 - pos, W - x);
    int p = ((g & OFX_SYM_FLIP_X) ? W - 1 - x : x) * W + ((g & OFX_SYM_FLIP_Y) ? W - 1 - y : y);
    uint32_t acc = 0u;  // the segment's bits enter at bit 31 and move down: one funnel shift per pixel
#pragma unroll 8
    for (int i = 0; i < len; i++, p += dp) acc = __builtin_amdgcn_alignbit(map[p >> 5] >> (p & 31), acc, 1u);
    out |= (acc >> (32 - len)) << pos;
    pos += len;
    x = 0;
    y++;
  }
  return out;
}

__device__ __forceinline__ void sym_pair_f(float *v, int W, int H, int g) {
  float x = v[0], y = v[1];
  if (g & OFX_SYM_TRANSPOSE) { const float t = x; x = y; y = t; }
  if (g & OFX_SYM_FLIP_X) x = (float)(W - 1) - x;
  if (g & OFX_SYM_FLIP_Y) y = (float)(H - 1) - y;
  v[0] = x; v[1] = y;
}

__device__ __forceinline__ void sym_pair_i(int32_t *v, int W, int H, int g) {
  int32_t x = v[0], y = v[1];
  if (g & OFX_SYM_TRANSPOSE) { const int32_t t = x; x = y; y = t; }
  if (g & OFX_SYM_FLIP_X) x = W - 1 - x;
  if (g & OFX_SYM_FLIP_Y) y = H - 1 - y;
  v[0] = x; v[1] = y;
}

// grid (n, DRAW ? 2 : 1): observation blockIdx.y (prev / next) of row blockIdx.x.  Every exit is block-uniform.
template <bool DRAW>
__global__ __launch_bounds__(256) void k_obs_transform(AugmentParams p) {
  extern __shared__ uint4 sym_lds[];
  const int d = blockIdx.x, which = blockIdx.y;
  int g;
  if constexpr (DRAW) {
    const bool pad = p.rows[d].ship < 0;  // read by both workgroups of the row; neither writes it
    g = 0;
    if (!pad) {
      uint32_t rr[4];
      ofx_philox4x32_10(p.arena_base, p.first + (uint32_t)d, p.draw, OFX_STREAM_AUGMENT, p.key, rr);
      int nth = ofx_draw_int(rr[0], __popc(p.mask) - 1);
      for (uint32_t m = p.mask; m; m &= m - 1u, nth--)
        if (nth == 0) { g = __ffs((int)m) - 1; break; }
    }
    if (which == 0 && threadIdx.x == 0 && p.op_out) p.op_out[d] = (uint8_t)g;
    if (pad) return;
  } else {
    g = p.op[d];
    if (g > 7 || ((g & OFX_SYM_TRANSPOSE) && p.W != p.H)) return;  // no-ops: the host cannot see op
  }
  if (g == 0) return;
  if (threadIdx.x == 0) {
    if constexpr (DRAW) {
      ofx_transition *row = p.rows + d;
      float *head = which ? row->head_next : row->head_prev;
      sym_pair_f(head + 2, p.W, p.H, g);
      sym_pair_f(head + 6, p.W, p.H, g);
      if (which == 0) sym_pair_i(&row->px, p.W, p.H, g);  // px, py are adjacent int32 fields
    } else {
      if (p.vec8) { sym_pair_f(p.vec8 + 8 * (size_t)d + 2, p.W, p.H, g); sym_pair_f(p.vec8 + 8 * (size_t)d + 6, p.W, p.H, g); }
      if (p.pointer) sym_pair_i(p.pointer + 2 * (size_t)d, p.W, p.H, g);
    }
  }
  const int words = p.words, n4 = words >> 2;
  uint4 *io = reinterpret_cast<uint4 *>(p.bits[which] + (size_t)d * 2 * words);
  for (int k = threadIdx.x; k < 2 * n4; k += 256) sym_lds[k] = io[k];
  __syncthreads();
  const uint32_t *lds = reinterpret_cast<const uint32_t *>(sym_lds);
  const bool tr = g & OFX_SYM_TRANSPOSE;
  for (int idx = threadIdx.x; idx < 2 * n4; idx += 256) {
    const int m = idx >= n4 ? 1 : 0;
    int j = idx - m * n4;
    if (tr && p.perm_s) j = (j % p.perm_g) * p.perm_s + j / p.perm_g;  // a bijection on [0, perm_s * perm_g) = [0, n4)
    const uint32_t *map = lds + m * words;
    uint32_t w4[4];
#pragma unroll
    for (int c = 0; c < 4; c++)
      w4[c] = tr ? sym_word_transpose(map, p.W, g, 4 * j + c) : sym_word_flip(map, p.W, p.H, words, g, 4 * j + c);
    io[m * n4 + j] = make_uint4(w4[0], w4[1], w4[2], w4[3]);
  }
}

// what both entries refuse about the frame: its two maps must fit the LDS budget and be whole uint4s
static int augment_frame_check(const ofx_handle *h, const char *who) {
  const size_t px = (size_t)h->cfg.width * h->cfg.height;
  if (px % 128) { ofx_set_error("%s: width*height must be a multiple of 128", who); return OFX_ERR_INVALID; }
  if (px / 4 > OFX_LDS_LIMIT) {
    ofx_set_error("%s: the two maps of a frame (%zu bytes) exceed the %d bytes of LDS they are transformed in", who, px / 4,
                  OFX_LDS_LIMIT);
    return OFX_ERR_INVALID;
  }
  return OFX_OK;
}

static void augment_params(const ofx_handle *h, AugmentParams *p) {
  memset(p, 0, sizeof(*p));
  p->W = h->cfg.width; p->H = h->cfg.height;
  p->words = (int)(((size_t)p->W * p->H) >> 5);
  if (p->W == p->H) {  // the transposed walk: S uint4s = a whole number of rows, when they tile the map
    int a = p->W, b = 128;
    while (b) { const int t = a % b; a = b; b = t; }
    const int S = p->W / a, n4 = p->words >> 2;
    if (n4 % S == 0) { p->perm_s = S; p->perm_g = n4 / S; }
  }
}

extern "C" int ofx_obs_transform(ofx_handle *h, int32_t n_obs, const uint8_t *op, void *bits, float *vec8, int32_t *pointer) {
  if (!h || !op || !bits) { ofx_set_error("ofx_obs_transform: null handle, op or bits"); return OFX_ERR_INVALID; }
  if (n_obs < 1) { ofx_set_error("ofx_obs_transform: n_obs must be >= 1, got %d", n_obs); return OFX_ERR_INVALID; }
  int rc;
  if ((rc = augment_frame_check(h, "ofx_obs_transform"))) return rc;
  OFX_HIP(hipSetDevice(h->cfg.device));
  AugmentParams p;
  augment_params(h, &p);
  p.bits[0] = (uint32_t *)bits; p.vec8 = vec8; p.pointer = pointer; p.op = op;
  hipLaunchKernelGGL(k_obs_transform<false>, dim3((unsigned)n_obs), dim3(256), (size_t)p.words * 8, h->stream, p);
  OFX_HIP(hipGetLastError());
  return OFX_OK;
}

extern "C" int ofx_replay_augment(ofx_handle *h, uint64_t seed, uint32_t draw, int32_t first, int32_t n, uint32_t op_mask,
                                  ofx_transition *rows, void *bits_prev, void *bits_next, uint8_t *op_out) {
  if (!h || !rows || !bits_prev || !bits_next) { ofx_set_error("ofx_replay_augment: null handle, rows or bits"); return OFX_ERR_INVALID; }
  if (n < 1 || first < 0 || first > INT32_MAX - n) {
    ofx_set_error("ofx_replay_augment: n must be >= 1, first >= 0 and first + n < 2^31, got first %d, n %d", first, n);
    return OFX_ERR_INVALID;
  }
  if (!(op_mask & 0xFFu) || (op_mask & ~0xFFu)) {
    ofx_set_error("ofx_replay_augment: op_mask must allow an element of 0 .. 7 and nothing else, got 0x%X", op_mask);
    return OFX_ERR_INVALID;
  }
  if ((op_mask & 0xAAu) && h->cfg.width != h->cfg.height) {
    ofx_set_error("ofx_replay_augment: op_mask 0x%X allows a transposing element, which needs width == height (%d x %d)",
                  op_mask, h->cfg.width, h->cfg.height);
    return OFX_ERR_INVALID;
  }
  int rc;
  if ((rc = augment_frame_check(h, "ofx_replay_augment"))) return rc;
  OFX_HIP(hipSetDevice(h->cfg.device));
  if (op_mask == 1u) {  // the identity alone: no kernel
    if (op_out) OFX_HIP(hipMemsetAsync(op_out, 0, (size_t)n, h->stream));
    return OFX_OK;
  }
  AugmentParams p;
  augment_params(h, &p);
  p.bits[0] = (uint32_t *)bits_prev; p.bits[1] = (uint32_t *)bits_next; p.rows = rows; p.op_out = op_out;
  p.key = ofx_key(seed); p.draw = draw; p.first = (uint32_t)first;
  p.arena_base = (uint32_t)h->cfg.arena_base; p.mask = op_mask;
  hipLaunchKernelGGL(k_obs_transform<true>, dim3((unsigned)n, 2u), dim3(256), (size_t)p.words * 8, h->stream, p);
  OFX_HIP(hipGetLastError());
  return OFX_OK;
}
