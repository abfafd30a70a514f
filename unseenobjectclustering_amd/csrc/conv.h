// Internal interface of the conv / pooling / head kernels (csrc/conv.hip, csrc/head.hip).
#pragma once
#include "common.h"

namespace uoc {

// One convolution over G independent groups (= the RGB and the XYZ branch, which have their
// own weights).  Activations are NHWC fp32; weights are [G][taps][Cout][Kc] with BatchNorm
// already folded in (Kc = Cin, or 32 for the stem's 8-pixel x 4-channel rows).
struct ConvParams {
  const float *in;    // [G][B][H][W][Cin]
  const float *w;     // [G][T][Cout][Kc]
  const float *bias;  // [G][Cout]; nullptr = no bias (the Winograd F(4x4) plane GEMMs)
  const float *res;   // [G][B][Ho][Wo][Cout] or nullptr
  float *out;         // [G][B][Ho][Wo][Cout]
  int G, B, H, W, Cin, Ho, Wo, Cout;
  int KH, KW, stride, dil, pad, relu;
  int stem;           // 1: 7x7 s2 p3 conv over NHWC4 input, K-chunk = one kernel row
  int tune = 1;       // 0: never autotune for this call (generic C entry: the tuner re-launches into `out` and syncs)
  // profiling overrides (csrc/prof.h): a caller that uses this convolution as a building block books it under its own
  // kernel class, algorithmic flop count and shape tag
  int prof_kc = -1;
  double prof_flops = 0.0;
  int prof_tag[4] = {0, 0, 0, 0};
};

int launch_conv(const ConvParams &p, hipStream_t st);
// Tile-level entries of the direct kernel (tests): the (family, height) pairs of every non-stem instantiation (returns their
// number, writes at most `cap` pairs), the static model's choice for a shape (fam_bm: the height of each of the 4 families,
// 0 where Cout does not admit it), and a launch of exactly one instantiation (never touches the tuner's table).
int conv_tile_list(int *out_pairs, int cap);
int conv_tile_choice(const ConvParams &p, int *cfg, int *bm, int *fam_bm);
int launch_conv_tile(const ConvParams &p, hipStream_t st, int cfg, int bm);

// A plane-GEMM tile of the Winograd F(4x4) path named by a caller (tests): BM tiles x BN output channels.
struct W4Tile {
  int bm, bn;
};
// (BN, BM) pairs of the fp32 plane GEMM (split = false) or of the split-precision one; what the static model picks
int wino4_tile_list(bool split, int *out_pairs, int cap);
// (dense: for the dense plan instead of the skipping one the network runs; the split-precision GEMM is always dense)
void wino4_tile_choice(bool split, bool dense, int B, int H, int W, int d, int Cout, int G, int *bn, int *bm);
int wino4_split_tile_list(int *out_pairs, int cap);
void wino4_split_tile_choice(int NT, int Cout, int planes, int *bn, int *bm);
// the shared cost model over a tile list {BM, BN} (the first of equal costs wins; bm / bn keep their value if no tile admits
// Cout) and the grid of a plane GEMM with a given tile.  Work items are counted over the rows each plane covers (Wino4Rows,
// csrc/wino4_math.h); the forms that take NT alone are the dense plan's: every one of `planes` planes covers all NT rows.
struct Wino4Rows;
void wino4_pick_tile(const int (*tiles)[2], int n, const Wino4Rows &rows, int Cout, int G, int &bm, int &bn);
int wino4_plane_grid(const Wino4Rows &rows, int Cout, int G, int bm, int bn);
void wino4_pick_tile(const int (*tiles)[2], int n, int NT, int Cout, int planes, int &bm, int &bn);
int wino4_plane_grid(int NT, int Cout, int planes, int bm, int bn);

// Winograd F(4x4,3x3) path (csrc/wino4.hip): U = transformed weights [G*36][Cout][Cin] (launch_wino4_weights, computed
// in double), ws = scratch of wino4_ws_floats() floats (the V and M frequency planes).
bool wino4_eligible(const ConvParams &p);
bool wino4_channels_ok(int Cin, int Cout);
size_t wino4_ws_floats(int G, int B, int H, int W, int d, int Cin, int Cout);
int wino4_num_tiles(int B, int H, int W, int d);   // NT of the layer's geometry
int launch_wino4_weights(const float *w, float *U, int G, int Cout, int Cin, hipStream_t st);
// U3 != nullptr: the split-precision ("bf16x3") plane GEMM of csrc/wino4_split.hip with the weights split by
// launch_wino4_split_weights ([G*36][3][Cout][Cin] bf16) — an experiment, never the default
// tile != nullptr: the plane GEMM runs exactly that instantiation (UOC_EINVAL if there is none or Cout % bn != 0) instead of
// the static model's choice; pair loop and grid follow the library's own rules for the tile
// dense: the dense plan (natural tile order, every plane covers every tile) instead of the skipping plan; same kernels, same bits
int launch_wino4_conv(const ConvParams &p, const float *U, float *ws, hipStream_t st, const unsigned short *U3 = nullptr,
                      const W4Tile *tile = nullptr, bool dense = false);
int launch_wino4_split_weights(const float *U, unsigned short *U3, int G, int Cout, int Cin, hipStream_t st);
int launch_wino4_slice_split(const ConvParams &p0, int Bg, int b0, const unsigned short *U3, float *ws, hipStream_t st,
                             const W4Tile *tile = nullptr);
struct Wino4Geom;
int w4_stage_output(const ConvParams &p, const Wino4Geom &geo, const float *Mw, hipStream_t st);
long wino4_elem_blocks(long items);
// NCHW [B][3][H][W] -> NHWC4 [B][H][W][4] (4th channel = 0)
int launch_nchw3_to_nhwc4(const float *in, float *out, int B, int H, int W, hipStream_t st);
// 3x3 s2 p1 max pooling, NHWC, C % 4 == 0; `n_img` images
int launch_maxpool3x3s2(const float *in, float *out, int n_img, int H, int W, int C, int Ho, int Wo, hipStream_t st);
// embed[b][p][:] = normalize(bilinear_up(a[b] + c[b]))  (align_corners=True), a,c: [B][h][w][64]; c may be null
// cat != 0: no sum; embed [B][2][H*W][64] = the two branches as planes, normalised over all 128 channels
int launch_head(const float *fa, const float *fb, float *embed, int B, int h, int w, int H, int W, int cat,
                hipStream_t st);

}  // namespace uoc
