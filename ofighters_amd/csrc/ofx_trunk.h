// ofx_trunk.h - the convolutional trunk of the bi-head policy (4 x [conv3x3 + BN + ReLU + maxpool2], once per image) as
// one launcher (ofx_trunk.hip); called by policy_forward_impl (ofx_policy.hip) with pointers into the prepared weights.
#pragma once
#include "ofx_internal.h"

#define PS 400 /* the model's fixed input side: Input((DEFAULT_WIDTH, DEFAULT_HEIGHT, 2)) */

// argument of the convolution kernels (the trunk's and k_upconv1 of ofx_policy.hip)
struct ConvParams {
  const float *in;                 // MODE 0: planar [img][CIN][H][W]; k_upconv1: [img][625]
  const unsigned *bits[2];         // MODE 1: word bits[ci][img * bits_stride + w], LSB-first (ch0 ship, ch1 laser)
  size_t bits_stride;              // words between consecutive images (PS*PS/32, or twice that for interleaved maps)
  const float *w, *b;              // folded [9][CIN][COUT], [COUT]
  float *out;                      // planar [img][COUT][Ho][Wo] or HWC [img][Ho][Wo][COUT]
  const uint8_t *mask;             // per image, may be null
  const float *wbm;                // k_convm, CIN = 8: per-lane B operand [24][64] (PrepLayout::wbm)
  int H, W;                        // conv domain (input after any upsampling) = conv output size
  int tiles_x, tiles;              // tiles per row / per image
  int legacy;                      // k_upconv1: TF1 legacy source mapping (src = dst / 2) instead of half-pixel centres
  int images;                      // k_convm: number of images (the grid is padded to a multiple of 8 of them)
  const int32_t *live;             // k_upconv1 with a mask: ordered list of the selected images (live[0] = count), else null
  unsigned long long *stat;        // k_trunk12<., true>: [4] M-tiles executed / all, table waves executed / all;
                                   // k_conv3_stream<., true>: [4], [5] M-tiles executed / all (may be null)
  unsigned *marks;                 // k_trunk12<., true> writes, k_conv3_stream<., true> reads: [img][100][4] words, bit x of
                                   // row y set <-> p2(y, x) may differ from K2 (written by an M-tile that ran)
  float *k2;                       // likewise: [8] conv2's constant K2[co], as k_trunk12<., true> derived it
};

struct TrunkParams {
  const unsigned *bits[2];         // the two 1-bit maps, as ConvParams::bits
  size_t bits_stride;
  int images;
  const float *tw[4], *tb[4], *wbm[3], *lut1, *zero16;  // into the prepared weights (PrepLayout, ofx_policy.hip)
  float *p1, *p2, *p3, *p4;        // pooled activations [img][8][200][200] (absent in the streaming form), [8][100][100],
                                   // [8][50][50] planar, [25][25][8] (h,w,c) = Flatten order
  int lowp;                        // OFX_OPT_POLICY_BF16: 0 fp32, 1 bf16 / 2 fp16 operands (streaming form only)
  bool sparse;                     // the streaming conv1 -> conv2 and conv3 skip constant windows (exact)
  unsigned long long *stat;        // counters of the sparse form [6] or null
  unsigned *nz2;                   // streaming form: the p2 marks [img][100][4] and K2 [8] (ConvParams::marks, ::k2)
  float *k2;
};

// the streaming form (k_trunk12 + k_conv3_stream) for this many images?  Otherwise one kernel per layer, and p1 exists.
bool ofx_trunk_fused(const ofx_handle *h, size_t images);
// the four layers on the handle's stream: plain (OFX_OPT_TRUNK_PLAIN) / streaming / per-layer form
int ofx_launch_trunk(ofx_handle *h, const TrunkParams &p);
// p4 inside the handle's scratch block as the forward of N images, S samples laid it out; null when the block is smaller
// (ofx_policy.hip, which owns the workspace layout; for ofx_policy_trunk_features)
const float *ofx_policy_ws_p4(ofx_handle *h, size_t N, size_t S);
// conv1 + BatchNorm + ReLU + pool of n stored observations (bits [n][2][5000]) through a caller-built table [2][512][8]
// (channel 0 carries the bias): out [n][8][200][200].  The fit's first layer (ofx_fit.hip): its table folds the BATCH statistics.
int ofx_launch_conv1_lut(ofx_handle *h, const void *bits, int n, const float *lut, float *out);
