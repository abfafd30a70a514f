/*
 * uoc_hip.h — C ABI of libuoc_hip.so, the MI355X (gfx950) native library behind the
 * reference's Python call surface for the inference hot path
 * (the reference has no FFI layer — these entry points are what a ctypes
 * binding for that path binds).
 *
 * Conventions
 *   - every pointer named d_* is a DEVICE pointer into caller-owned memory (a torch tensor);
 *     the library allocates nothing across the boundary except the opaque net handle.
 *   - every function returns 0 on success or a negative errno-style code; it never throws.
 *     uoc_last_error() returns a thread-local message for the last failure.
 *   - `stream` is a hipStream_t passed as void*; all work is enqueued on it, nothing
 *     synchronises unless documented.
 *   - embeddings ("X") are PIXEL-MAJOR: [batch][n][64] fp32, one 256-byte row per pixel.
 *     This is the layout the fused backbone head writes and the clustering kernels read.
 */
#ifndef UOC_HIP_H
#define UOC_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define UOC_OK 0
#define UOC_EINVAL (-22)
#define UOC_ENOMEM (-12)
#define UOC_EHIP (-5)
#define UOC_ENOENT (-2)
#define UOC_ETIMEDOUT (-110)

#define UOC_EMBED_DIM 64   /* channel count C the kernels are specialised for */
#define UOC_MAX_SEEDS 128  /* num_seeds upper bound (reference default 100)   */
#define UOC_METRIC_COSINE 0     /* embedding metric of the *_ex clustering calls: cfg.TRAIN.EMBEDDING_METRIC 'cosine' */
#define UOC_METRIC_EUCLIDEAN 1  /* ... and 'euclidean' (the reference's code default)                                */

int uoc_version(void);
/* Always 0 since round 6: every kernel choice that affects rounding is a compile-time constant and the library holds one
 * implementation per step (rounds 3-5 had a -DUOC_DEV build with the measured-and-rejected alternates).  Kept for ABI stability. */
int uoc_is_dev_build(void);
/* Hash of everything that could make two processes compute different bits (the library version).  The frame-parallel runner all-reduces it next to its error flag: ranks that disagree
 * fail before the gather instead of silently breaking sharding independence. */
unsigned long long uoc_config_fingerprint(void);
/* Releases process-wide helper objects (the per-device events that order the persistent sampling kernels of
 * different streams).  Optional; call it before process exit while the HIP runtime is still up.  Idempotent. */
int uoc_shutdown(void);
const char *uoc_last_error(void);
/* The library reads its (speed-only) UOC_* environment variables once and caches them; a process that changes one
 * afterwards (tests, micro-benchmarks) calls this to have them read again at their next use. */
int uoc_reload_env(void);

/* ------------------------------------------------------------------------------------------
 * Mean-shift clustering  — replaces lib/utils/mean_shift.py:128-229 (cosine metric; the *_ex calls below also euclidean)
 * ---------------------------------------------------------------------------------------- */

/* Seed selection runs as ONE persistent cooperative launch with X resident on chip when the batch
 * fits the device (default); 0 forces the streaming one-launch-per-step kernel.  Same results. */
int uoc_ms_set_persistent_fps(int on);
/* A caller that launches clustering from SEVERAL streams of one device (frames in flight) must switch this on: the
 * persistent sampling grids of different streams are then ordered through a per-device event, because two of them
 * partially resident at the same time would each wait for blocks the other keeps off the chip.  Off by default
 * (single-stream callers pay nothing). */
int uoc_ms_set_stream_ordering(int on);
/* Number of seed-selection calls since process start in which fields that the on-chip kernel should have handled
 * went to the streaming kernel instead (does not fit on chip / cooperative launch refused).  The two kernels sum the
 * dot product in different orders; a caller that needs placement-independent results checks that this stays 0. */
int uoc_ms_fps_fallbacks(void);
/* The persistent kernel's grid-wide exchange spins with a bound; a block that gives up raises a sticky device
 * flag and the call's outputs are then meaningless.  uoc_ms_check synchronises `stream`, reads and clears the
 * flag: 0, or UOC_ETIMEDOUT.  The host mirrors call it at the points where they synchronise anyway. */
int uoc_ms_check(void *stream);

/* Scratch bytes the clustering entry points need for (batch, n, m).  d_ws of every uoc_ms_* call that takes one is
 * 256-byte aligned: any other alignment is UOC_EINVAL before any device work. */
size_t uoc_ms_workspace_bytes(int batch, int n, int m);

/* Farthest-point seed selection — select_smart_seeds, mean_shift.py:128-189.
 * d_first_index [batch] int32: the index the reference draws with np.random.randint (:155).
 * d_seeds [batch][m][64], d_indices [batch][m] int32. */
int uoc_ms_select_seeds(const float *d_X, int batch, int n, int m, const int32_t *d_first_index,
                        float *d_seeds, int32_t *d_indices, void *d_ws, size_t ws_bytes, void *stream);

/* The same with the first num_init rows of every d_seeds[b] already chosen by the caller — the init_seeds /
 * num_init_seeds continuation of select_smart_seeds, mean_shift.py:142-170 (`seeds = init_seeds` there too: the
 * selection is written into the caller's matrix).  The given rows need not be rows of X; their d_indices stay -1
 * like the reference's selected_indices.  num_init = 0 is uoc_ms_select_seeds (d_first_index is then required;
 * otherwise it is not read).  num_init > 0 always runs the one-launch-per-step kernel. */
int uoc_ms_select_seeds_from(const float *d_X, int batch, int n, int m, int num_init, const int32_t *d_first_index,
                             float *d_seeds, int32_t *d_indices, void *d_ws, size_t ws_bytes, void *stream);

/* iters x { W = exp(kappa Z X^T); Z = normalize(W X) } — seed_hill_climbing_ball,
 * mean_shift.py:79-109 with ball_kernel :26.  d_Z [batch][m][64] is updated in place. */
int uoc_ms_hill_climb(const float *d_X, int batch, int n, float *d_Z, int m, float kappa, int iters,
                      void *d_ws, size_t ws_bytes, void *stream);

/* Sequential epsilon-ball labelling of the seeds — connected_components, mean_shift.py:41-76.
 * d_seed_labels [batch][m] int32; d_num_unique [batch] int32 = len(unique(seed labels)). */
int uoc_ms_seed_components(const float *d_Z, int batch, int m, float epsilon, int32_t *d_seed_labels,
                           int32_t *d_num_unique, void *stream);

/* Nearest-seed assignment + "largest cluster becomes label 0" — mean_shift.py:211-227.
 * d_labels [batch][n] int32; d_closest (nullable) [batch][n] int32 = argmin seed.
 * A pixel no seed wins (a non-finite row of d_X or only non-finite seeds: no distance compares below +inf) gets label 0,
 * is counted under label 0 for the swap, and closest = INT_MAX.  A seed label outside 0..127 is written to d_labels as
 * it is and left out of the counts.  The same holds for uoc_ms_assign_ex with either metric. */
int uoc_ms_assign(const float *d_X, int batch, int n, const float *d_Z, const int32_t *d_seed_labels,
                  const int32_t *d_num_unique, int m, int32_t *d_labels, int32_t *d_closest,
                  void *d_ws, size_t ws_bytes, void *stream);

/* The four stages above back to back — mean_shift_smart_init, mean_shift.py:192-229.
 * d_Z_out (nullable) receives the converged seeds, d_seed_labels_out (nullable) their labels. */
int uoc_ms_cluster(const float *d_X, int batch, int n, int m, float kappa, int iters, float epsilon,
                   const int32_t *d_first_index, int32_t *d_labels, int32_t *d_indices,
                   float *d_Z_out, int32_t *d_seed_labels_out, void *d_ws, size_t ws_bytes, void *stream);

/* 128-d embeddings (cfg.TRAIN.FUSION_TYPE = 'cat', SEG.py:109-110): the field is stored as `halves` = 2 planes of 64
 * channels, d_X [batch][halves][n][64] (plane 0 = channels 0..63), and so are the converged seeds d_Z_out
 * [batch][halves][m][64]; every dot product runs over both planes.  halves = 1 is exactly uoc_ms_cluster. */
size_t uoc_ms_workspace_bytes_wide(int batch, int n, int m, int halves);
int uoc_ms_cluster_wide(const float *d_X, int halves, int batch, int n, int m, float kappa, int iters, float epsilon,
                        const int32_t *d_first_index, int32_t *d_labels, int32_t *d_indices, float *d_Z_out,
                        int32_t *d_seed_labels_out, void *d_ws, size_t ws_bytes, void *stream);

/* The calls above with the embedding metric as an argument (the reference's metric=, mean_shift.py): UOC_METRIC_COSINE
 * is exactly the call without _ex; UOC_METRIC_EUCLIDEAN clusters with
 *   seed selection  d = ||x - s||_2                                 (farthest point, first index on ties)
 *   hill climbing   W = exp(-kappa ||z - x||^2), Z = W X / max(rowsum(W), 1)   (no renormalisation)
 *   seed components ||z_j - z_i||_2 <= epsilon
 *   assignment      argmin ||x - z||_2                               (first index on ties)
 * Any other metric returns UOC_EINVAL (uoc_last_error says why) and launches nothing.  Same workspace, determinism and
 * batch independence as the cosine calls. */
int uoc_ms_select_seeds_ex(const float *d_X, int batch, int n, int m, int num_init, const int32_t *d_first_index,
                           float *d_seeds, int32_t *d_indices, int metric, void *d_ws, size_t ws_bytes, void *stream);
int uoc_ms_hill_climb_ex(const float *d_X, int batch, int n, float *d_Z, int m, float kappa, int iters, int metric,
                         void *d_ws, size_t ws_bytes, void *stream);
int uoc_ms_seed_components_ex(const float *d_Z, int batch, int m, float epsilon, int metric, int32_t *d_seed_labels,
                              int32_t *d_num_unique, void *stream);
int uoc_ms_assign_ex(const float *d_X, int batch, int n, const float *d_Z, const int32_t *d_seed_labels,
                     const int32_t *d_num_unique, int m, int metric, int32_t *d_labels, int32_t *d_closest, void *d_ws,
                     size_t ws_bytes, void *stream);
int uoc_ms_cluster_ex(const float *d_X, int batch, int n, int m, float kappa, int iters, float epsilon, int metric,
                      const int32_t *d_first_index, int32_t *d_labels, int32_t *d_indices, float *d_Z_out,
                      int32_t *d_seed_labels_out, void *d_ws, size_t ws_bytes, void *stream);
int uoc_ms_cluster_wide_ex(const float *d_X, int halves, int batch, int n, int m, float kappa, int iters, float epsilon,
                           int metric, const int32_t *d_first_index, int32_t *d_labels, int32_t *d_indices, float *d_Z_out,
                           int32_t *d_seed_labels_out, void *d_ws, size_t ws_bytes, void *stream);


/* ------------------------------------------------------------------------------------------
 * RGB-D ResNet34-8s embedding network — replaces SEGNET.forward (lib/networks/SEG.py:88-119,
 * RGBD/'add' branch) with its two Resnet34_8s backbones (resnet_dilated.py:287-327,
 * resnet.py:116-270).  Activations NHWC fp32, convolutions on fp32 MFMA, BatchNorm folded.
 * ---------------------------------------------------------------------------------------- */
typedef struct uoc_net uoc_net;

/* Input modality / fusion of SEGNET (SEG.py:69-71 construction, :97-110 forward):
 *   RGBD_ADD   cfg.INPUT='RGBD', FUSION_TYPE='add'   : fcn(img) + fcn_depth(xyz)          (two backbones)
 *   COLOR      cfg.INPUT='COLOR'                     : fcn(img)
 *   DEPTH      cfg.INPUT='DEPTH'                     : fcn(xyz)   (the weights still live under "fcn.")
 *   RGBD_EARLY cfg.INPUT='RGBD', FUSION_TYPE='early' : fcn(cat(img, xyz)), a 6-channel stem (SEG.py:178-181)
 *   RGBD_CAT   cfg.INPUT='RGBD', FUSION_TYPE='cat'   : cat(fcn(img), fcn_depth(xyz)) -> 128-d embeddings (:109-110) */
enum { UOC_NET_RGBD_ADD = 0, UOC_NET_COLOR = 1, UOC_NET_DEPTH = 2, UOC_NET_RGBD_EARLY = 3, UOC_NET_RGBD_CAT = 4 };

int uoc_net_create(uoc_net **out);                   /* = uoc_net_create_mode(out, UOC_NET_RGBD_ADD) */
int uoc_net_create_mode(uoc_net **out, int mode);
int uoc_net_embed_dim(const uoc_net *net);           /* 64, or 128 for RGBD_CAT */
int uoc_net_destroy(uoc_net *net);
/* One state-dict entry by its reference key ("fcn.resnet34_8s.layer1.0.conv1.weight", ...;
 * SEG.py:130-159 contract), HOST fp32 memory, copied. */
int uoc_net_load_param(uoc_net *net, const char *name, const float *host_data, size_t numel);
/* Checks that every parameter is present, folds BN (eps 1e-5), re-lays weights out as
 * [tap][cout][cin] and uploads them to the CURRENT device. */
int uoc_net_finalize(uoc_net *net);
size_t uoc_net_workspace_bytes(const uoc_net *net, int B, int H, int W);
/* d_rgb, d_xyz: [B][3][H][W] fp32 NCHW (what test_sample hands the network, test_dataset.py:247);
 * the one the mode does not read (d_xyz for COLOR, d_rgb for DEPTH) may be NULL.
 * d_embed: [B][H*W][64] pixel-major unit-norm embeddings; RGBD_CAT: [B][2][H*W][64], plane 0 = the image
 * branch's 64 channels, plane 1 = the XYZ branch's, normalised over all 128 (the layout uoc_ms_cluster_wide reads). */
/* EXPERIMENT (round 6), off by default and never part of the headline measurement: the plane GEMMs of the Winograd layers in
 * split precision — every fp32 operand as three bf16 terms (3 x 8 = 24 significand bits), six bf16 MFMA products with fp32
 * accumulation, 2.67x the fp32 matrix rate (csrc/wino4_split.hip).  Embeddings stay within the fp32 path's distance of an
 * fp64 evaluation, but they are NOT bit-identical to it.  Call after uoc_net_finalize; on = 1 splits the transformed
 * weights once (hipMalloc + a synchronisation). */
int uoc_net_set_split_precision(uoc_net *net, int on);
/* d_ws: uoc_net_workspace_bytes(net, B, H, W) bytes, 256-byte aligned: any other alignment is UOC_EINVAL. */
int uoc_net_forward(uoc_net *net, const float *d_rgb, const float *d_xyz, int B, int H, int W, float *d_embed,
                    void *d_ws, size_t ws_bytes, void *stream);

/* Single fused conv (+bias +residual +ReLU), NHWC, over G independent groups stacked on the leading
 * dimension (in [G][B][H][W][Cin], weights [G][K*K][Cout][Cin], bias [G][Cout], ...); K in {1,3}.
 * Cin % 32 == 0, Cout % 64 == 0.  Exposed for unit tests / micro-benchmarks of the conv kernels.
 * uoc_conv2d_nhwc runs the direct implicit-GEMM kernel.  uoc_conv2d_nhwc_algo names the algorithm explicitly (no
 * environment variable decides it): UOC_CONV_DIRECT, or UOC_CONV_WINOGRAD4 = F(4x4,3x3) as the network runs its 3x3
 * stride-1 layers from 64 channels up (UOC_EINVAL if the shape is not eligible).  The Winograd path keeps its transformed weights and
 * scratch in buffers owned by this entry: one caller thread at a time.
 * UOC_CONV_WINOGRAD4 runs, as the network does, the plan in which a tile whose fourth output row / column lies outside the
 * image skips the frequency planes that only those outputs read; UOC_CONV_WINOGRAD4_DENSE runs the same kernels with every
 * plane over every tile.  The two give the same bits; the tile entries below take either (same list, cfg = BN, bm). */
#define UOC_CONV_DIRECT 0
#define UOC_CONV_WINOGRAD4 4
#define UOC_CONV_WINOGRAD4_BF16X3 5   /* EXPERIMENT: the same with the split-precision plane GEMM (see uoc_net_set_split_precision) */
#define UOC_CONV_WINOGRAD4_DENSE 6    /* tests: UOC_CONV_WINOGRAD4's kernels on the dense plan, where every frequency plane covers every tile; the same bits */
int uoc_conv2d_nhwc(const float *d_in, const float *d_w, const float *d_bias, const float *d_res, float *d_out,
                    int G, int B, int H, int W, int Cin, int Cout, int K, int stride, int dil, int pad, int relu,
                    void *stream);
int uoc_conv2d_nhwc_algo(const float *d_in, const float *d_w, const float *d_bias, const float *d_res, float *d_out,
                         int G, int B, int H, int W, int Cin, int Cout, int K, int stride, int dil, int pad, int relu,
                         int algo, void *stream);

/* Test entries of the convolution kernels: every tile instantiation, and the stem, the pooling and the head on their own.
 * The conv kernels are families of template instantiations chosen at run time (by a static cost model, and in the network
 * by a tuner that times them); all instantiations of one algorithm sum every output in the same order and are
 * bit-identical, which tests/test_conv_tiles_gpu.py asserts through these entries.
 * uoc_conv2d_tile_list writes min(cap, n) pairs (cfg, bm) to out_pairs and returns n, the number of instantiations of
 *   `algo` (generated from the table that drives the dispatch).  UOC_CONV_DIRECT: cfg = tile family 0..3 (0: 2x4 waves
 *   x 128 output channels, 1: 1x8 x 128, 2: 2x4 x 64, 3: 1x4 x 64), bm = pixels per tile.  UOC_CONV_WINOGRAD4 and
 *   UOC_CONV_WINOGRAD4_BF16X3: cfg = BN, the plane GEMM's output channels per tile (64 or 128), bm = its tiles per block
 *   tile; the fp32 plane GEMM has each pair with and without its pair loop, which follows from Cin (an even number, four or
 *   more, of 32-channel chunks) as in the network.
 * uoc_conv2d_nhwc_tile is uoc_conv2d_nhwc_algo running exactly the instantiation (cfg, bm), on the grid the library uses
 *   for that tile.  UOC_EINVAL if the list has no such pair or the shape does not admit it (Cout % BN != 0, a shape the
 *   algorithm refuses, a group above 2 GB).  It neither reads nor writes the tuner's table and launches nothing to time.
 * uoc_conv2d_tile_choice: the pair the static model picks for a shape (pad = dil for K = 3, 0 for K = 1), host arithmetic
 *   (the Winograd model reads the device's CU count, 256 without a device).  UOC_CONV_DIRECT also fills family_bm[4] (unless
 *   NULL) with the height each family would run at, 0 where Cout does not admit the family: the network's tuner may
 *   take any of them.
 * uoc_net_stem: d_nchw [G][B][3][H][W] -> d_out [G][B][H1][W1][64], H1 = (H-1)/2 + 1: the NCHW -> NHWC4 kernel and the
 *   7x7 stride-2 pad-3 instantiation.  h_w [G][64][3][7][7] and h_bias [G][64] are HOST memory (as uoc_net_load_param
 *   takes them; re-laid out by the function uoc_net_finalize uses); h_bias NULL = zero, as in the first pass of the
 *   early-fusion stem, whose second pass takes the first as d_res [G][B][H1][W1][64].  Allocates, synchronises, frees.
 * uoc_maxpool3x3s2_nhwc: [n_img][H][W][C] -> [n_img][(H-1)/2+1][(W-1)/2+1][C], kernel 3, stride 2, padding 1 (taps outside
 *   the image are skipped), C % 4 == 0.
 * uoc_head: d_fa, d_fb [B][h][w][64] -> unit-norm d_embed [B][H*W][64] = normalize(bilinear(fa + fb), align_corners) (d_fb
 *   may be NULL), or with cat != 0 [B][2][H*W][64], the two upsampled branches normalised over all 128 channels. */
int uoc_conv2d_tile_list(int algo, int32_t *out_pairs, int cap);
int uoc_conv2d_nhwc_tile(const float *d_in, const float *d_w, const float *d_bias, const float *d_res, float *d_out,
                         int G, int B, int H, int W, int Cin, int Cout, int K, int stride, int dil, int pad, int relu,
                         int algo, void *stream, int cfg, int bm);
int uoc_conv2d_tile_choice(int G, int B, int H, int W, int Cin, int Cout, int K, int stride, int dil, int algo,
                           int32_t *cfg, int32_t *bm, int32_t *family_bm);
int uoc_net_stem(const float *d_nchw, const float *h_w, const float *h_bias, const float *d_res, int G, int B, int H,
                 int W, int relu, float *d_out, void *stream);
int uoc_maxpool3x3s2_nhwc(const float *d_in, float *d_out, int n_img, int H, int W, int C, void *stream);
int uoc_head(const float *d_fa, const float *d_fb, float *d_embed, int B, int h, int w, int H, int W, int cat,
             void *stream);


/* ------------------------------------------------------------------------------------------
 * Two-stage glue — replaces lib/fcn/test_dataset.py:62-198 (filter_labels_depth, crop_rois,
 * match_label_crop) with batched device kernels.  Label maps are int32 with ids < 128.
 * ---------------------------------------------------------------------------------------- */
typedef struct uoc_roi_table {
  int32_t K;            /* number of ROIs = non-zero labels present, ascending label order    */
  int32_t label[128];   /* stage-1 label id of ROI k                                          */
  int32_t box[128][4];  /* x0, y0, x1, y1 inclusive, padded 25 % and clamped (:83-93)         */
} uoc_roi_table;

/* The one workspace of the ROI entry points below (the size does not depend on the frame).  d_ws 16-byte aligned: every
 * region holds 4-byte words and starts at a multiple of 256 bytes from d_ws. */
size_t uoc_roi_workspace_bytes(void);

/* Input preparation (read_sample / compute_xyz, tools/test_images.py:96-133) on the device:
 * d_bgr [H][W][3] uint8 (cv2.imread order), d_depth_mm [H][W] uint16 millimetres ->
 * d_image [3][H][W] = bgr/255 - mean (mean_* = PIXEL_MEANS/255 as float32), d_xyz [3][H][W] metres. */
int uoc_prep_rgbd(const uint8_t *d_bgr, const uint16_t *d_depth_mm, int H, int W, float fx, float fy, float px,
                  float py, float mean_b, float mean_g, float mean_r, float *d_image, float *d_xyz, void *stream);

/* filter_labels_depth (:183-198): per batch item, a non-zero label whose fraction of pixels with
 * z > 0 is < threshold becomes 0.  d_z: the Z plane of item 0; items are z_batch_stride floats apart. */
int uoc_filter_labels_depth(int32_t *d_labels, const float *d_z, long z_batch_stride, int B, int H, int W,
                            float threshold, void *d_ws, size_t ws_bytes, void *stream);

/* One pass that (optionally, d_z != NULL) applies the depth filter in place and builds the ROI
 * table of crop_rois (:68-93; mask.py:180-187 tight box, round-half-even padding, clamping). */
int uoc_roi_build(int32_t *d_labels, const float *d_z, int H, int W, float threshold, float pad_fraction,
                  uoc_roi_table *d_table, void *d_ws, size_t ws_bytes, void *stream);

/* crop_rois (:95-110): crops of the [3][H][W] image / XYZ planes resized to SxS with bilinear
 * align_corners=True, object mask with nearest.  Outputs NCHW [K][3][S][S] and [K][S][S].
 * COLOR input (depth is None, :73-76): d_xyz = d_xyz_crops = NULL. */
int uoc_roi_crop(const float *d_rgb, const float *d_xyz, const int32_t *d_labels, int H, int W,
                 const uoc_roi_table *d_table, int K, int S, float *d_rgb_crops, float *d_xyz_crops,
                 float *d_mask_crops, void *stream);

/* match_label_crop part 1 (:118-136): d_keep[k][c] = 1 iff crop cluster c of ROI k overlaps the
 * stage-1 mask by >= 50 %; d_meanz[k] = mean z (>0) over kept pixels (all pixels if none kept).
 * Without depth (d_xyz_crops = NULL) d_meanz is not written: ROIs are ordered by box area (:138-146). */
int uoc_roi_match_stats(const int32_t *d_labels_crop, const float *d_mask_crops, const float *d_xyz_crops, int K,
                        int S, int32_t *d_keep, float *d_meanz, void *d_ws, size_t ws_bytes, void *stream);

/* match_label_crop part 2 (:156-177): d_map[k][c] = global id of kept cluster c (0 = dropped),
 * d_order = ROI paint order (far to near); nearest-resize each crop back to its box and paste
 * non-zeros, later ROIs overwrite earlier ones.  d_refined [H*W] is fully written.  K in 1..127, S, H, W >= 1:
 * UOC_EINVAL before any launch otherwise, like the other ROI calls. */
int uoc_roi_paste(const int32_t *d_labels_crop, const uoc_roi_table *d_table, const int32_t *d_map,
                  const int32_t *d_order, int K, int S, int H, int W, int32_t *d_refined, void *stream);

/* match_label_crop (:116-179) entirely on the device (round 6): the statistics of uoc_roi_match_stats, then the ROI paint
 * order — sorted(key = mean depth | box area, reverse=True) with Python's stable-sort semantics, NaN keys included for
 * K < 64 (csrc/roi.hip restates CPython's list.sort for short lists) — the running renumbering of kept clusters, and the
 * paste of uoc_roi_paste.  No host round trip.  d_keep (nullable) [K][128] receives the keep table, d_plan (nullable)
 * [K + K*128] the paint order followed by the id map.  d_status (nullable): bit 0 is OR-ed in when some key is NaN and
 * K >= 64 — the one case not restated here; d_refined is then painted in index order and the caller re-does the ordering
 * on the host (uoc_roi_match_stats + uoc_roi_paste). */
int uoc_roi_match(const int32_t *d_labels_crop, const float *d_mask_crops, const float *d_xyz_crops,
                  const uoc_roi_table *d_table, int K, int S, int H, int W, int32_t *d_refined, int32_t *d_keep,
                  int32_t *d_plan, int32_t *d_status, void *d_ws, size_t ws_bytes, void *stream);

/* Frame-parallel runner (no reference counterpart; SURVEY 8(e): the gathered block is uint8 like the ROS consumer's cast,
 * ros/test_images_segmentation.py:165): d_out[i] = (uint8) d_labels[i] for i < n, *d_top = max(*d_top, max_i d_labels[i])
 * (the caller checks once per block that no id exceeded 255). */
int uoc_labels_to_u8(const int32_t *d_labels, long n, uint8_t *d_out, int32_t *d_top, void *stream);


/* ------------------------------------------------------------------------------------------
 * Evaluation — the integer statistics of multilabel_metrics (lib/utils/evaluation.py:109-257; overlap and
 * boundary precision / recall of a predicted against a ground-truth label map).  The host mirror
 * unseenobjectclustering_amd/utils/evaluation.py turns them into the reference's metric dictionary.
 * ---------------------------------------------------------------------------------------- */
typedef struct uoc_eval_tables {
  int32_t cont[128 * 128];     /* [gt][pred] pixels with that label pair (:188-190)                          */
  int32_t prec_tp[128 * 128];  /* [gt][pred] boundary pixels of pred inside the dilated boundary of gt (:103)  */
  int32_t rec_tp[128 * 128];   /* [gt][pred] boundary pixels of gt inside the dilated boundary of pred (:104)  */
  int32_t bnd_pred[128];       /* boundary pixels (seg2bmap, :15-73) of every predicted mask (:212-215)        */
  int32_t bnd_gt[128];         /* ... of every ground-truth mask (:216-219)                                    */
  int32_t bad_label;           /* != 0: a label id outside [0, 128) was seen (such pixels are skipped)         */
} uoc_eval_tables;

/* d_ws 256-byte aligned (UOC_EINVAL otherwise; the two regions hold 4-byte words). */
size_t uoc_eval_workspace_bytes(int H, int W);
/* d_pred, d_gt: [H][W] int32 label maps (0 = background); radius = bound_pix of boundary_overlap (:88-89),
 * the dilation structuring element is the disk x^2 + y^2 <= radius^2 (:94-98). */
int uoc_eval_pair_stats(const int32_t *d_pred, const int32_t *d_gt, int H, int W, int radius, uoc_eval_tables *d_tables,
                        void *d_ws, size_t ws_bytes, void *stream);


/* ------------------------------------------------------------------------------------------
 * Per-object point clouds and 3D statistics from label maps (no reference counterpart: the step every consumer of
 * the label map takes next).  A pixel of object l has label l in [1, 127]; other ids, negative ones included, are
 * background.  A valid point is a pixel of an object whose x, y, z are finite and whose z > 0.
 * One record per (frame, id), all 128 ids; id 0 and absent ids are all zeros (box -1).  Float fields are 0 when
 * count == 0.  Sums run in fp64 in a fixed order: every output is bitwise reproducible, and frame b's outputs do not
 * depend on the other frames of the batch.
 * ---------------------------------------------------------------------------------------- */
#define UOC_OBJECTS_MAX_ATTR 8
typedef struct uoc_object {
  int32_t pixels;         /* pixels with the id                                                                  */
  int32_t count;          /* valid points                                                                        */
  int32_t box[4];         /* pixel box x0, y0, x1, y1 inclusive over the id's pixels; -1 when pixels == 0       */
  float centroid[3];      /* mean of the valid points                                                            */
  float cov[6];           /* population covariance (1/n) sum (p-c)(p-c)^T: xx, xy, xz, yy, yz, zz               */
  float aabb_min[3];
  float aabb_max[3];
  float eig[3];           /* eigenvalues of cov, descending, never negative (clamped at 0)                       */
  float axes[9];          /* row-major 3x3, column k = unit eigenvector e_k; e0, e1 have their largest-magnitude
                             component positive (ties: lowest index), e2 = e0 x e1                                 */
  float obb_center[3];    /* c + sum_k e_k (min d_k + max d_k) / 2,  d_k = (p - c) . e_k over the valid points     */
  float obb_half[3];      /* (max d_k - min d_k) / 2                                                             */
  int32_t offset;         /* first row of the object's points in the packed cloud                                */
  int32_t kept;           /* rows of the object in the packed cloud                                              */
} uoc_object;

/* d_ws 16-byte aligned: its regions hold 8-byte keys and fp64 sums and start at multiples of 256 bytes from d_ws. */
size_t uoc_objects_workspace_bytes(int B, int H, int W);
/* d_labels [B][H][W] int32, d_xyz [B][3][H][W] fp32 metres, d_attr (nullable) [B][attr_ch][H][W] fp32 with
 * attr_ch <= UOC_OBJECTS_MAX_ATTR.  d_objects [B][128].
 * Packed cloud (d_points == NULL: records only): rows ordered by frame, id, raster index y*W + x; d_points [P][3],
 * d_point_attr (nullable) [P][attr_ch], d_point_pixel (nullable) [P] raster index within the frame.  With
 * max_points_per_object = M > 0 an object of count > M keeps the points of in-object rank floor(j*count/M),
 * j = 0..M-1 (64-bit arithmetic); M <= 0 keeps all.  *d_total receives P; no row at or past `capacity` is written
 * (capacity B*H*W always suffices). */
int uoc_objects(const int32_t *d_labels, const float *d_xyz, const float *d_attr, int attr_ch, int B, int H, int W,
                int max_points_per_object, uoc_object *d_objects, float *d_points, float *d_point_attr,
                int32_t *d_point_pixel, long capacity, int32_t *d_total, void *d_ws, size_t ws_bytes, void *stream);


/* ------------------------------------------------------------------------------------------
 * Object tracking across the frames of a stream (no reference counterpart): each raw label map
 * becomes a tracked label map whose ids are track slots 1..127.  An object keeps its slot while it is in view and gets
 * it back after an occlusion of at most max_age frames.  Object ids are 1..127, every other value is background.
 * All arithmetic is integer: the result is defined exactly and does not depend on launch order or batch.
 *
 * State per stream (caller-owned device memory, uoc_track_state_bytes(B, H, W) / B bytes each, stream b at byte offset
 * b * that; 16-byte aligned): int32 [1024] header = the slot table uoc_track[128] (slot 0 unused), then at word 640 the
 * number of uids handed out (next uid = that + 1), the step counter and the sticky count of dropped objects;
 * int32 [128*128] contingency scratch (all zero between steps); int32 [H*W] memory map (for every live track the
 * pixels of its last sighting that no later object has covered).  An all-zero state is a reset stream.
 *
 * One step with the raw map L: cont[t][c] = #pixels with mem == t and L == c; candidates are pairs of a live track t
 * and a present id c with inter = cont[t][c] > 0 and inter * 65536 >= q * union, union = area_mem[t] + area_cur[c] -
 * inter; greedy matching takes the candidate of largest IoU among unmatched t and c (exact comparison by 64-bit cross
 * multiplication; ties: larger inter, lower t, lower c) until none is left; a matched track gets age 0, hits + 1, the
 * id's area; an unmatched one age + 1 and is retired (record zeroed) when age > max_age; unmatched ids in ascending
 * order take the free slots in ascending order (a slot retired in this step included) with uid = next uid, hits 1,
 * born = step; without a free slot the object becomes background and `dropped` grows.  out = slot of L (0 = background);
 * mem' = out where out != 0, else mem where its track was live, is unmatched and was not retired, else 0.
 * ---------------------------------------------------------------------------------------- */
typedef struct uoc_track {
  int32_t uid;    /* 0 = free slot; else the stream's running object number 1, 2, 3, ..., never reused */
  int32_t age;    /* frames since the last match (0 = matched in the last step)                         */
  int32_t hits;   /* frames in which the track was matched (the birth included)                         */
  int32_t area;   /* pixels at the last match                                                           */
  int32_t born;   /* step index of the birth                                                            */
} uoc_track;
#define UOC_TRACK_SLOTS 128            /* slot 0 is never a track */
#define UOC_TRACK_HEADER_WORDS 1024    /* int32 words of a stream's state before its contingency scratch */
#define UOC_TRACK_META_WORD 640        /* words 640, 641, 642 = uids handed out, step, dropped */
#define UOC_TRACK_CONT_WORDS (128 * 128)

size_t uoc_track_state_bytes(int B, int H, int W);
size_t uoc_track_workspace_bytes(int B);
/* Zeroes the state of stream `which`, or of all B streams when which = -1. */
int uoc_track_reset(void *d_state, int B, int H, int W, int which, void *stream);
/* d_labels, d_out [B][H*W] int32 (distinct buffers); q = round(min_iou * 65536) in [1, 65536]; max_age >= 0;
 * d_lut (nullable) [B][128]: raw id -> slot of this step; d_tracks (nullable) [B][128]: the slot table after the step.
 * H*W must be below 2^31.  Where d_lut / d_tracks are given, every word of them is written (rows of absent ids and of free
 * slots are zero): they need no initialisation.  d_state and d_ws 16-byte aligned.  Three launches on `stream`, nothing
 * synchronises. */
int uoc_track_step(const int32_t *d_labels, int B, int H, int W, int q, int max_age, void *d_state, int32_t *d_out,
                   int32_t *d_lut, uoc_track *d_tracks, void *d_ws, size_t ws_bytes, void *stream);


/* ------------------------------------------------------------------------------------------
 * Spatially connected components of a label map (no reference counterpart): the clustering never
 * asks whether the pixels of one id touch each other; this step does.  L is [B][H][W] int32 with H*W below 2^31.
 *
 * A pixel is foreground when 1 <= L <= 127; every other value (negative ids, 128, 255) is background.  connectivity is
 * 4 or 8.  A component is a maximal set of foreground pixels of ONE frame that carry the SAME id and are connected
 * through neighbours of that id; pixels of different ids or frames never join.  Of a component: root = its smallest
 * raster index y*W + x, area = its pixel count, src = its raw id.  siblings(b, i) = the number of components of raw id
 * i in frame b, the small ones included.  A component is small when area < min_area (min_area >= 1); small components
 * become background.
 *
 * Mode ALL: the non-small components of a frame, in ascending root order, get the new ids 1, 2, ..., 127; those beyond
 * the 127th become background and count as dropped.  table[b][k] = {src, area, root, siblings(b, src)} for new id k.
 * Mode LARGEST: per raw id the non-small component of largest area (ties: the smaller root) keeps the raw id; the id's
 * other non-small components become background and count as dropped.  table[b][i] = {i, area, root, siblings(b, i)}
 * for raw id i.
 * Both: unused table rows and row 0 are zero; counts[b] = {found, small, kept, dropped}, found = small + kept +
 * dropped; out is int32 in 0..127 and must not alias L.  All arithmetic is integer and every choice is over a strict
 * total order: the result is defined exactly and does not depend on launch order or batch.
 * ---------------------------------------------------------------------------------------- */
#define UOC_CC_ALL 0
#define UOC_CC_LARGEST 1

/* 0 for a bad shape. */
size_t uoc_cc_workspace_bytes(int B, int H, int W);
/* d_labels, d_out [B][H*W] int32 (distinct buffers); d_table [B][128][4] and d_ws 16-byte aligned; d_counts [B][4].
 * Returns UOC_EINVAL before any device work for null pointers, d_out == d_labels, a connectivity other than 4 or 8,
 * min_area < 1, an unknown mode, a bad shape or a workspace below uoc_cc_workspace_bytes(B, H, W).  Six (LARGEST) or
 * seven (ALL) launches on `stream`, one fewer when the frame is a single 32x32 tile; no host read, nothing
 * synchronises, no state is kept between calls. */
int uoc_cc_split(const int32_t *d_labels, int B, int H, int W, int connectivity, int min_area, int mode, int32_t *d_out,
                 int32_t *d_table, int32_t *d_counts, void *d_ws, size_t ws_bytes, void *stream);


/* ------------------------------------------------------------------------------------------
 * Support plane and object heights above it (no reference counterpart): the dominant plane of
 * the background pixels of a frame, and every object measured against it.  d_labels [B][H][W] int32 and d_xyz
 * [B][3][H][W] fp32 metres as for uoc_objects; H*W below 2^31.
 *
 * A. Candidates (integers, exact).  A pixel is a candidate when its label is NOT in 1..127, x, y, z are finite, z > 0
 * and q_c = (int) rintf(c * 1000.0f) (fp32 product, round half to even) has |q_c| <= 32767 for c = x, y, z.  M = the
 * candidates of the frame, listed in raster order.  M < 3: no plane.
 * B. Hypotheses (integers, exact).  mix(x): x ^= x >> 16; x *= 0x7feb352d; x ^= x >> 15; x *= 0x846ca68b; x ^= x >> 16
 * in uint32.  For h = 0..num_hyp-1 and k = 0, 1, 2: i_k = (uint64(mix(seed ^ ((3h+k) * 0x9E3779B9))) * M) >> 32 (the
 * frame index is not hashed), p_k = q of candidate i_k, n = (p1-p0) x (p2-p0) in int64, g = max |n_c|,
 * s = max(0, bitlength(g) - 30), n'_c = sign(n_c) * (|n_c| >> s).  n' = 0: score(h) = -1.  Else L = floor(sqrt(n'.n'))
 * exactly and score(h) = #candidates q with |n'.(q - p0)| <= tau_mm * L.  Winner: largest score, ties to the lowest h;
 * every score -1: no plane.
 * C. Refinement (fp64, fixed summation order, one round).  Over the winner's inliers (the integer test of B) and their
 * original fp32 points: centroid c, population covariance, eigen-decomposition; normal = the unit eigenvector of the
 * smallest eigenvalue, d = -normal.c, both negated when d < 0 (the camera is on the positive side); d == 0: the
 * component of normal of largest magnitude is positive (ties: lowest index).  u = the normalised projection of (1,0,0)
 * onto the plane ((0,1,0) when that projection is shorter than 1e-6), v = normal x u.
 * D. Objects.  For every id 1..127 over its valid points (uoc_objects' rule), t = normal.p + d, (a, b) =
 * ((p-c).u, (p-c).v) in fp64: see uoc_plane_object.  Without a plane every field below but `candidates` is 0.
 * Bitwise reproducible; frame b's outputs do not depend on the other frames of the batch.
 * ---------------------------------------------------------------------------------------- */
typedef struct uoc_plane {
  int32_t found;       /* 1 when a plane was fitted                                                              */
  int32_t candidates;  /* M                                                                                      */
  int32_t inliers;     /* the winner's score                                                                     */
  int32_t hyp;         /* the winning h                                                                          */
  float normal[3];     /* refined unit normal                                                                    */
  float d;             /* refined offset: normal.p + d = 0                                                       */
  float centroid[3];   /* centroid c of the inliers                                                              */
  float eig[3];        /* eigenvalues of the inliers' covariance, descending, never negative (clamped at 0)      */
  float rms;           /* sqrt(eig[2]): rms distance of the inliers from the plane                               */
  float u[3];          /* in-plane axes                                                                          */
  float v[3];
} uoc_plane;

typedef struct uoc_plane_object {
  int32_t count;       /* valid points of the id; 0: every other field is 0                                      */
  float height_min;    /* min t                                                                                  */
  float height_max;    /* max t                                                                                  */
  float foot[2];       /* mean of (a, b)                                                                         */
  float cov2[3];       /* population covariance of (a, b): aa, ab, bb                                            */
  float axis[2];       /* unit major axis e of cov2 in the (u, v) frame (closed-form 2x2 eigen-solve, fp64); its
                          component of larger magnitude is positive (ties: index 0); eigen-gap 0: (1, 0)           */
  float half[3];       /* half extents (max - min) / 2 of r.e, r.e' and t, r = (a, b) - foot, e' = (-e[1], e[0])  */
  float center[3];     /* upright box centre: c + (foot + m0 e + m1 e') in (u, v) + m2 normal, m = (max + min) / 2 */
} uoc_plane_object;
#define UOC_PLANE_MAX_HYP 1024      /* num_hyp in 1..1024 */
#define UOC_PLANE_MAX_TAU_MM 1000   /* tau_mm (and rem_mm) in 1..1000 */

/* 0 for a bad shape or num_hyp outside 1..1024. */
size_t uoc_plane_workspace_bytes(int B, int H, int W, int num_hyp);
/* num_hyp in 1..1024, tau_mm in 1..1000.  d_planes [B], d_objs [B][128], d_height (nullable) [B][H][W]: t as fp32 at
 * every pixel with a valid point (object or background), NaN elsewhere and in a frame without a plane.  d_ws 16-byte
 * aligned.  Returns UOC_EINVAL before any device work for null pointers, bad ranges, a bad shape or a workspace below
 * uoc_plane_workspace_bytes(B, H, W, num_hyp).  Launches on `stream`; no host read, nothing synchronises, no state is
 * kept between calls. */
int uoc_support_plane(const int32_t *d_labels, const float *d_xyz, int B, int H, int W, int num_hyp, int tau_mm,
                      uint32_t seed, uoc_plane *d_planes, uoc_plane_object *d_objs, float *d_height, void *d_ws,
                      size_t ws_bytes, void *stream);


/* ------------------------------------------------------------------------------------------
 * Several planes of a frame's background: shelves, walls and the plane the objects stand on (no reference counterpart;
 * DESIGN.md section 22).  Sequential extraction: rules A, B and C of uoc_support_plane repeated on what the earlier
 * planes left.  K = max_planes in 1..8, tau_mm in 1..1000, rem_mm in tau_mm..1000, min_inliers >= 3, num_hyp in
 * 1..1024, B * K <= 65535.
 *
 * R. Rounds (integers, exact).  C_0 = the candidates of rule A in raster order.  Round r = 0..K-1 works on C_r,
 * M_r = |C_r|: its hypotheses follow rule B on C_r with the seed (seed + r) mod 2^32, the ranks i_k being ranks in C_r,
 * and its winner W_r = (n', p0, L) follows the same argmax and the same tie rule.
 * S. Stop.  Extraction stops before round r when M_r < 3, when every score of the round is -1 or when the winning score
 * is below min_inliers.  count = the rounds that produced a plane.
 * I. Inliers I_r = {q in C_r : |n'.(q - p0)| <= tau_mm * L}; removed R_r = {q in C_r : |n'.(q - p0)| <= rem_mm * L}.
 * The fringe R_r \ I_r belongs to no plane, but cannot seed a duplicate of plane r.  The survivors
 * C_{r+1} = C_r \ R_r keep their raster order.
 * C'. Refinement.  Rule C per plane over I_r and the original fp32 points, with the same fixed summation order: a
 * uoc_plane per (frame, r), d_planes [B][K].  `candidates` of slot r is M_r.  Slot `count` (the round that stopped, when
 * count < K) holds zeros but for candidates = M_count, as a frame without a plane does in uoc_support_plane; the slots
 * after it are all zero.
 * D'. Objects.  Rule D against every found plane, d_objs [B][K][128] (nullable); slots past count hold zeros.
 *
 * d_index [B][H][W] int32: -2 not a candidate; r in I_r; 16 + r in R_r \ I_r; -1 a candidate that survived every round.
 * d_count [B] int32.  d_info [B][K]: see uoc_plane_info; zeros past count but for round_candidates of slot `count`.
 * Round 0 is uoc_support_plane bit for bit: with the same num_hyp, tau_mm and seed, d_planes[b][0] and d_objs[b][0][*]
 * equal what uoc_support_plane writes, for any K and rem_mm and any min_inliers <= that plane's inliers.
 * Bitwise reproducible; frame b's outputs do not depend on the other frames of the batch.
 * ---------------------------------------------------------------------------------------- */
typedef struct uoc_plane_info {
  int32_t round_candidates;  /* M_r                                                                              */
  int32_t removed;           /* |R_r|                                                                            */
  float cos0;                /* normal_r . normal_0, fp64 from the fp64 refinement                               */
  float offset0;             /* normal_0 . centroid_r + d_0: signed distance of plane r's centroid from plane 0  */
  float extent[4];           /* min a, max a, min b, max b of I_r, (a, b) = ((p - c_r).u_r, (p - c_r).v_r), fp64 */
} uoc_plane_info;
#define UOC_PLANES_MAX 8            /* max_planes in 1..8 */
#define UOC_PLANES_FRINGE 16        /* d_index: 16 + r marks the removal band of plane r outside its inliers */

/* 0 for a bad shape, num_hyp outside 1..1024, max_planes outside 1..8 or B * max_planes above 65535. */
size_t uoc_planes_workspace_bytes(int B, int H, int W, int num_hyp, int max_planes);
/* d_ws 16-byte aligned.  Returns UOC_EINVAL before any device work for null pointers (d_objs alone may be null), bad
 * ranges, a bad shape or a workspace below uoc_planes_workspace_bytes(B, H, W, num_hyp, max_planes).  Launches on
 * `stream`; no host read, nothing synchronises, no state is kept between calls. */
int uoc_support_planes(const int32_t *d_labels, const float *d_xyz, int B, int H, int W, int max_planes, int num_hyp,
                       int tau_mm, int rem_mm, int min_inliers, uint32_t seed, int32_t *d_count, uoc_plane *d_planes,
                       uoc_plane_info *d_info, int32_t *d_index, uoc_plane_object *d_objs, void *d_ws, size_t ws_bytes,
                       void *stream);


/* ------------------------------------------------------------------------------------------
 * Object relations of a frame: contact, occlusion and pick order (no reference counterpart).
 * d_labels [B][H][W] int32 and d_xyz [B][3][H][W] fp32 metres as for uoc_objects, of which only channel 2 (z) is read;
 * H*W below 2^29.  Integers only.
 *
 * Ids.  id(p) = L when 1 <= L <= 127, else 0 (the background rule of uoc_objects, uoc_track_step and uoc_cc_split).
 * Id 0 takes part in the pair tables.
 * Depth.  valid(p) when z is finite and 0 < z <= 65.0f; then zq(p) = (int) rintf(z * 1000.0f) (fp32 product, round
 * half to even).
 * Neighbour pairs.  connectivity 4: for every pixel p = (x, y) the pairs (p, (x+1, y)) and (p, (x, y+1)) that lie
 * inside the frame; connectivity 8: also (p, (x+1, y+1)) and (p, (x-1, y+1)).  Every unordered pair of neighbouring
 * pixels is visited once; pairs never cross frames.
 * Tables.  For a pair (p, r) with a = id(p), b = id(r), a != b: border[a][b] += 1 and border[b][a] += 1.  When both
 * pixels are valid and |zq(p) - zq(r)| < gap_mm: touch[a][b] += 1 and touch[b][a] += 1.  When both are valid and the
 * gap is >= gap_mm: front[n][f] += 1 with n the id of the pixel of smaller zq and f the other id.  A pair with an
 * invalid pixel counts in border only.  d_pairs [B][3][128][128] int32 holds the planes UOC_REL_BORDER, UOC_REL_TOUCH
 * and UOC_REL_FRONT; the diagonals are 0.
 * Relations, ids 1..127 only.  An id is present when it has at least one pixel.  a occludes b when front[a][b] >=
 * min_pairs and front[a][b] > front[b][a]; a touches b when touch[a][b] >= min_pairs.
 * Layers.  Round r = 1, 2, ... gives layer r to every present id that has no layer yet and whose occluders all have a
 * layer below r; the first round that layers nothing ends the peeling, and the ids left over (occlusion cycles and
 * what lies below them) get layer -1.
 * Every count is a sum of ones and every choice is over a strict total order: the result is defined exactly and does
 * not depend on launch order or batch.
 * ---------------------------------------------------------------------------------------- */
#define UOC_REL_BORDER 0
#define UOC_REL_TOUCH 1
#define UOC_REL_FRONT 2
#define UOC_REL_MAX_GAP_MM 65535   /* gap_mm in 1..65535 */

typedef struct uoc_relation_object {   /* one per (frame, id); all zero for id 0 and for an absent id */
  int32_t pixels;     /* pixels with the id                                                                      */
  int32_t edge;       /* of which in row 0, row H-1, column 0 or column W-1, each counted once                    */
  int32_t border;     /* sum over b != a of border[a][b], b = 0 included                                          */
  int32_t border_bg;  /* border[a][0]                                                                             */
  int32_t hidden;     /* front[0][a]: unlabelled matter in front of the object                                    */
  int32_t n_touch;    /* ids in 1..127 that touch a                                                               */
  int32_t n_above;    /* ids in 1..127 that occlude a                                                             */
  int32_t n_below;    /* ids in 1..127 that a occludes                                                            */
  int32_t layer;      /* peeling round, or -1                                                                     */
  int32_t free;       /* 1 when present, n_above == 0, hidden < min_pairs and edge == 0                           */
  int32_t order;      /* 1-based rank among the present ids by (layer, -1 after every positive layer; then id)    */
} uoc_relation_object;

/* 0 for a bad shape. */
size_t uoc_relations_workspace_bytes(int B, int H, int W);
/* connectivity 4 or 8, gap_mm in 1..65535, min_pairs >= 1.  d_pairs [B][3][128][128] int32, d_objs [B][128]; d_ws
 * 16-byte aligned.  Returns UOC_EINVAL before any device work for null pointers, bad ranges, a bad shape (B outside
 * 1..65535, H*W not below 2^29) or a workspace below uoc_relations_workspace_bytes(B, H, W).  Two memsets and two
 * launches on `stream`; no host read, nothing synchronises, no state is kept between calls. */
int uoc_relations(const int32_t *d_labels, const float *d_xyz, int B, int H, int W, int connectivity, int gap_mm,
                  int min_pairs, int32_t *d_pairs, uoc_relation_object *d_objs, void *d_ws, size_t ws_bytes, void *stream);


/* ------------------------------------------------------------------------------------------
 * Table occupancy and placement: free space on the support plane (no reference counterpart).
 * d_labels [B][H][W] int32 and d_xyz [B][3][H][W] fp32 metres as for uoc_objects; d_planes [B] as uoc_support_plane
 * writes them, or filled in by the caller; H*W below 2^31.  Every output is an integer.
 *
 * F. The frame in integers, S = 16384.  A plane record is used when found == 1, every component of normal, u, v is
 * finite with magnitude <= 2, d is finite with |d| <= 1000 and qc_c = (int) rintf(centroid[c] * 1000.0f) (fp32 product)
 * has |qc_c| <= 32767; any other record is a frame without a plane.  N_c = (int) rint((double) normal[c] * 16384.0),
 * U_c, V_c likewise from u, v, D = (int64) rint((double) d * 16384000.0): each one correctly rounded operation (the
 * double products are exact).  d_frame [B][16] int64 = N[3], D, U[3], V[3], qc[3], 1, 0, 0.  A frame without a plane has
 * a zero frame record, all-zero state / owner / dist2 / counts, and every query answered (-1, -1, 0, 0).
 * P. Points.  A pixel takes part when x, y, z are finite, z > 0 and q_c = (int) rintf(c * 1000.0f) has |q_c| <= 32767
 * for c = x, y, z (uoc_support_plane's rule A without its label condition).  id(p) = L when 1 <= L <= 127, else 0.
 * In int64: T = N.q + D (height above the plane in mm * 2^14), A = U.(q - qc), Bv = V.(q - qc).  Bound: |N_c|, |U_c|,
 * |V_c| <= 32768 and |q_c - qc_c| <= 65534, so |A|, |Bv|, |N.q| <= 3 * 32768 * 65534 < 2^33, and |D| < 2^34.
 * i = floor(A / (cell_mm * S)) + G/2 and j = floor(Bv / (cell_mm * S)) + G/2, floor towards minus infinity.  A point
 * with i or j outside [0, G) adds one to `outside` and is otherwise ignored.  Else, with id = id(p):
 *   T < -tau_mm*S: ignored;  else id != 0 or T > h_obs_mm*S: obstacle, n_obs[i][j] += 1, owner[i][j] = max(owner, id);
 *   else T <= tau_mm*S: table, n_table[i][j] += 1;  else ignored.
 * C. Cells.  state = 2 (obstacle) when n_obs >= min_pts, else 1 (table) when n_table >= min_pts, else 0 (unknown).
 * owner is 0 unless state is 2.  cells[a], a = 1..127: the obstacle cells whose owner is a.
 * E. Clearance.  A cell is blocking when its state is 2, or 0 with unknown_blocks set; every cell outside the grid is
 * blocking.  dist2[i][j] = the smallest (i-i')^2 + (j-j')^2 over the blocking cells (i', j'), the outside ones
 * included: the exact squared Euclidean distance transform, 0 on blocking cells, at most (G/2)^2.
 * Q. Queries (need2, ai, aj, mode), the same for every frame; the candidates are the cells of state 1.  mode 0
 * (widest): the candidate of largest dist2, ties to the lowest i*G + j; answer (i, j, dist2, dist2 >= need2).  mode 1
 * (nearest): among the candidates with dist2 >= need2 the smallest (i-ai)^2 + (j-aj)^2, ties to the larger dist2, then
 * to the lowest i*G + j; answer (i, j, dist2, 1).  No candidate: (-1, -1, 0, 0).
 * Every count is a sum of ones and every choice is over a strict total order: the result is defined exactly and does
 * not depend on launch order or batch.
 * ---------------------------------------------------------------------------------------- */
#define UOC_PLACE_MAX_QUERIES 16
#define UOC_PLACE_WIDEST 0
#define UOC_PLACE_NEAREST 1
#define UOC_PLACE_MAX_GRID 512      /* G: a multiple of 8 in 8..512 (every table-grid call) */
#define UOC_PLACE_MAX_MM 1000       /* cell_mm, tau_mm in 1..1000, h_obs_mm in 0..1000 */
#define UOC_PLACE_MAX_MIN_PTS 65535
#define UOC_PLACE_MAX_ANCHOR 4096   /* a query's anchor cell lies in -4096..4095 */
#define UOC_PLACE_SCALE 16384       /* S of the integer frame */

/* 0 for a bad shape (B outside 1..65535, H*W not below 2^31) or a bad G. */
size_t uoc_placement_workspace_bytes(int B, int H, int W, int G);
/* G a multiple of 8 in 8..512; cell_mm, tau_mm in 1..1000; h_obs_mm in 0..1000; min_pts in 1..65535; unknown_blocks 0
 * or 1; Q in 0..16.  h_queries: a HOST array [Q][4] int32 (nullable when Q == 0), read before the call returns:
 * need2 in 0..2^30, ai and aj in -4096..4095, mode 0 or 1.  d_state, d_owner, d_dist2 [B][G][G] int32; d_counts
 * [B][128] int32, word 0 = outside, words 1..127 = cells; d_frame [B][16] int64; d_answers [B][Q][4] int32 (nullable
 * when Q == 0); d_ws 16-byte aligned.  Returns UOC_EINVAL before any device work for null pointers, bad ranges, a bad
 * shape or a workspace below uoc_placement_workspace_bytes(B, H, W, G); a rejected call writes nothing.  Three
 * memsets and three launches on `stream`, a fourth when Q > 0; no host read of device memory, nothing synchronises,
 * no state is kept between calls. */
int uoc_placement(const int32_t *d_labels, const float *d_xyz, const uoc_plane *d_planes, int B, int H, int W, int G,
                  int cell_mm, int h_obs_mm, int tau_mm, int min_pts, int unknown_blocks, const int32_t *h_queries, int Q,
                  int32_t *d_state, int32_t *d_owner, int32_t *d_dist2, int32_t *d_counts, int64_t *d_frame,
                  int32_t *d_answers, void *d_ws, size_t ws_bytes, void *stream);


/* ------------------------------------------------------------------------------------------
 * Grasp candidates: a parallel-jaw fit on the table grid (no reference counterpart).
 * d_state, d_owner [B][G][G] int32 as uoc_placement writes them, G a multiple of 8 in 8..512.  Top-down grasps only:
 * the gripper closes along a direction in the plane, the fingers come down on the table.  Every output is an integer.
 *
 * D. Directions, S = 16384.  h_dirs: a HOST array [A][2] int32 of closing directions (Cx_k, Cy_k) in units of 1/S, every
 * component in [-S, S]; the Python wrapper fills it with rint(cos(pi k / A) S), rint(sin(pi k / A) S) in float64.  No
 * kernel calls a trigonometric function.  Parameters, in cells: A in 1..32 directions; M in 0..8, the lateral offsets
 * m = -M..M; Wmax in 1..64, the largest opening; gap in 0..4, the clearance between a finger and the object; F in 1..8,
 * the finger thickness; Hp in 0..4, the pad half-length; unknown_blocks 0 or 1.
 * K. Cells.  A cell whose state is outside 0..2, or whose state is 2 with an owner outside 1..127, counts as unknown.
 * A. Anchor.  For id a in 1..127: n_a = the cells with state == 2 and owner == a, Si, Sj the sums of their indices.
 * n_a == 0: the id is absent.  Else, in int64, ax = (S (2 Si + n_a)) / (2 n_a) and ay likewise from Sj, floor division:
 * the centroid of the cell centres in units of 1/S cell.
 * S. Samples.  X = ax + t Cx_k - l Cy_k, Y = ay + t Cy_k + l Cx_k, cell (X >> 14, Y >> 14) with arithmetic shifts
 * (floor).  Class of a sample relative to a: OUT when the cell is outside [0, G)^2; OWN: state 2 and owner a; OTHER:
 * state 2 and another owner in 1..127; FREE: state 1, or state 0 when unknown_blocks == 0; UNKNOWN: everything else.
 * C. Candidate (k, m).  The pad strip is the lines l = m-Hp .. m+Hp; the search range is t = -R..R, R = 2 Wmax.  The
 * first code that applies:
 *   -1 (MISS)     no OWN sample in the strip over the search range; tlo = 0
 *   -2 (WIDE)     tlo / thi = the smallest / largest t of an OWN sample over the whole strip, w = thi - tlo + 1 > Wmax
 *   -3 (PINCHED)  an OTHER or OUT sample in the strip for t in [tlo, thi]
 *   -4 (BLOCKED)  a sample that is not FREE in the strip for t in [tlo-gap-F, tlo-1] or [thi+1, thi+gap+F] (these t may
 *                 lie beyond -R..R; the sample formula applies there, too)
 *   w  (>= 1)     otherwise
 * d_cand [B][128][A][2M+1][2] int32 = (code, tlo); the rows of id 0 and of absent ids are all zero.
 * B. Best.  d_best [B][128][8] int32 = (ok, k, m, tlo, w, ax, ay, n_ok), n_ok = the candidates with a positive code.
 * The winner is the maximum of the 32-bit key 1 + (((M-|m|) << 24) | ((Wmax-w) << 16) | ((A-1-k) << 8) | (m >= 0)):
 * nearest to the centroid, then narrowest, then lowest k, then +m before -m; a strict total order over (k, m).
 * Without a candidate of positive code: (0, -1, 0, 0, 0, ax, ay, 0).  Absent id and id 0: all zero.  A frame whose
 * state is all zero (a frame without a plane) has all-zero outputs.
 * Every count is a sum of ones and every choice is over a strict total order: the result is defined exactly and does
 * not depend on launch order or batch.
 * ---------------------------------------------------------------------------------------- */
#define UOC_GRASP_MAX_DIRS 32
#define UOC_GRASP_MISS (-1)
#define UOC_GRASP_WIDE (-2)
#define UOC_GRASP_PINCHED (-3)
#define UOC_GRASP_BLOCKED (-4)
#define UOC_GRASP_SCALE 16384       /* S of the direction table and of the anchor */
#define UOC_GRASP_MAX_OFFSETS 8     /* M in 0..8 */
#define UOC_GRASP_MAX_OPEN 64       /* Wmax in 1..64 cells */
#define UOC_GRASP_MAX_GAP 4         /* gap in 0..4 cells */
#define UOC_GRASP_MAX_FINGER 8      /* F in 1..8 cells */
#define UOC_GRASP_MAX_PAD 4         /* Hp in 0..4 cells */

/* 0 for B outside 1..65535, a bad G, A outside 1..32 or M outside 0..8. */
size_t uoc_grasp_workspace_bytes(int B, int G, int A, int M);
/* Ranges as in D above.  h_dirs is read before the call returns.  d_ws 16-byte aligned.  Returns UOC_EINVAL before any
 * device work for null pointers, bad ranges or a workspace below uoc_grasp_workspace_bytes(B, G, A, M); a rejected call
 * writes nothing, the workspace included.  One memset and two launches on `stream`; no host read of device memory,
 * nothing synchronises, no state is kept between calls. */
int uoc_grasp(const int32_t *d_state, const int32_t *d_owner, int B, int G, const int32_t *h_dirs, int A, int M, int Wmax,
              int gap, int F, int Hp, int unknown_blocks, int32_t *d_cand, int32_t *d_best, void *d_ws, size_t ws_bytes,
              void *stream);


/* ------------------------------------------------------------------------------------------
 * Elevation map: object tops and stacking spots on the table grid (no reference counterpart).
 * d_labels [B][H][W] int32 and d_xyz [B][3][H][W] fp32 metres as for uoc_placement; d_frame [B][16] int64 exactly as
 * uoc_placement wrote it, or filled in by the caller; G, cell_mm and tau_mm as given to uoc_placement make the two grids
 * coincide cell for cell.  H*W below 2^31.  S = 16384.  Every output is an integer.
 *
 * F. Frame.  A record is used when word 13 is 1, words 0..2 (N) and 4..9 (U, V) have magnitude <= 32768, |word 3| (D)
 * <= 2^34 and words 10..12 (qc) have magnitude <= 32767, which keeps the int64 bounds of uoc_placement's step P for
 * caller-supplied records; any other record is a frame without a plane: elev all UOC_ELEV_NONE; owner, pts, near, dist2,
 * info all zero; every row of tops (0, 0, -1, -1, 0, 0, 0, 0); every answer (-1, -1, 0, 0).
 * P. Points.  uoc_placement's rule P unchanged: participation, q, T, A, Bv, i, j with floor division, id(p).  A point
 * outside the grid adds 1 to `outside`; a point with T < -tau_mm*S is ignored.  A kept point has hq = min(T >> 14, 32767)
 * (arithmetic shift: a floor, T = -1 gives -1), key = hq + 1024 (in 24..33791) and word = (key << 7) | id.
 * H. Cells, first pass.  pts[c] = the kept points of cell c, top[c] = their largest word: the highest point, ties to the
 * larger id.  pts > 0: elev[c] = (top >> 7) - 1024, owner[c] = top & 127; else elev[c] = UOC_ELEV_NONE, owner[c] = 0.
 * N. Cells, second pass over the same points.  near[c] = the kept points with key >= (top[c] >> 7) - step_mm; a cell is
 * solid when near >= min_pts (a lone mixed pixel above a surface makes its cell not solid, not a false top).
 * L. Level.  Cells outside the grid are not solid.  A cell c is blocking when it is not solid, or when one of its four
 * edge neighbours c' is not solid, has owner(c') != owner(c) or |elev(c) - elev(c')| > step_mm: a level region has one
 * owner and climbs at most step_mm per cell.  The cells on the grid's border are always blocking.
 * E. Clearance.  dist2 = the exact squared Euclidean distance transform to the nearest blocking cell, the cells outside
 * the grid included, as uoc_placement's step E: 0 on blocking cells, at most (G/2)^2.
 * T. d_tops [B][128][8] int32, id a = 0..127 (0: the table and whatever is unlabelled) = (cells, level, i, j, dist2,
 * elev_at, elev_max, elev_mean): cells = the solid cells owned by a; level = those that are not blocking; (i, j) = the
 * level cell of largest dist2, ties to the lowest i*G + j, elev_at its elev ((-1, -1), dist2 = elev_at = 0 when level ==
 * 0); elev_max = the largest elev over the solid cells (0 when cells == 0); elev_mean = floor(sum / level) towards minus
 * infinity of the int64 sum of elev over the level cells (0 when level == 0).
 * Q. Queries (need2, id, hmin_mm, hmax_mm), the same for every frame.  The candidates are the cells that are not
 * blocking with hmin <= elev <= hmax and owner == id (id in 0..127), or owner >= 1 (id == -1: any object, never the
 * table).  Answer (i, j, dist2, dist2 >= need2) of the candidate of largest dist2, ties to the lowest i*G + j; without a
 * candidate (-1, -1, 0, 0).
 * I. d_info [B][4] int32 = (found, outside, the cells with pts > 0, the solid cells).
 * Every count is a sum of ones and every choice is over a strict total order: the result is defined exactly and does
 * not depend on launch order or batch.
 * ---------------------------------------------------------------------------------------- */
#define UOC_ELEV_MAX_QUERIES 16
#define UOC_ELEV_NONE (-32768)

/* 0 for a bad shape (B outside 1..65535, H*W not below 2^31) or a bad G. */
size_t uoc_elevation_workspace_bytes(int B, int H, int W, int G);
/* G a multiple of 8 in 8..512; cell_mm, tau_mm, step_mm in 1..1000; min_pts in 1..65535; Q in 0..16.  h_queries: a HOST
 * array [Q][4] int32 (nullable when Q == 0), read before the call returns: need2 in 0..2^30, id in -1..127, hmin_mm and
 * hmax_mm in -32768..32767.  d_elev, d_owner, d_pts, d_near, d_dist2 [B][G][G] int32; d_tops [B][128][8] int32; d_info
 * [B][4] int32; d_answers [B][Q][4] int32 (nullable when Q == 0); d_ws 16-byte aligned.  Returns UOC_EINVAL before any
 * device work for null pointers, bad ranges, a bad shape, a workspace below uoc_elevation_workspace_bytes(B, H, W, G) or
 * one that is not 16-byte aligned; a rejected call writes nothing, the workspace included.  Four memsets and five
 * launches on `stream`; no host read of device memory, nothing synchronises, no state is kept between calls. */
int uoc_elevation(const int32_t *d_labels, const float *d_xyz, const int64_t *d_frame, int B, int H, int W, int G,
                  int cell_mm, int tau_mm, int step_mm, int min_pts, const int32_t *h_queries, int Q, int32_t *d_elev,
                  int32_t *d_owner, int32_t *d_pts, int32_t *d_near, int32_t *d_dist2, int32_t *d_tops, int32_t *d_info,
                  int32_t *d_answers, void *d_ws, size_t ws_bytes, void *stream);


/* ------------------------------------------------------------------------------------------
 * Footprint fitting: oriented put-down poses on the table grid (no reference counterpart).
 * d_state, d_owner, d_dist2 [B][G][G] int32 as uoc_placement writes them, cell index i*G + j, G a multiple of 8 in
 * 8..512; d_frame [B][16] int64 as uoc_placement writes it, nullable.  For up to 8 rectangles and up to 32 orientations
 * over half a turn: in which orientations the rectangle, centred on a cell, lies wholly on free cells.  Every output is
 * an integer.
 *
 * D. Directions: exactly D of uoc_grasp.  S = 16384; h_dirs: a HOST array [A][2] int32 of directions (Cx_k, Cy_k), the
 * rectangle's long axis, every component in [-S, S]; A in 1..32.  No kernel calls a trigonometric function.
 * R. Rectangles.  h_rects: a HOST array [F][8] int32, F in 1..8, record f = (HL, HW, ignore, mode, ai, aj, 0, 0): HL, HW
 * the half length and half width in units of 1/256 cell, each in 0..16384 with HL^2 + HW^2 <= 16384^2; ignore in 0..127
 * (0: none); mode UOC_FOOT_ROOMIEST or UOC_FOOT_NEAREST; the anchor ai, aj in -4096..4095; words 6 and 7 are 0.  R_f is
 * the smallest integer with (256 R_f)^2 >= HL^2 + HW^2, at most 64.
 * K. Cells.  A cell whose state is outside 0..2, or whose state is 2 with an owner outside 1..127, counts as unknown
 * (K of uoc_grasp).  Cell c is FREE for rectangle f when its state is 1; when it is unknown (state 0 included) and
 * unknown_blocks == 0; or when its state is 2, ignore >= 1 and owner == ignore (the object being moved does not block
 * itself).  A cell outside the grid is never FREE.
 * M. Mask.  M(f,k) = the offsets (di, dj) with |di|, |dj| <= R_f + 1, |di Cx_k + dj Cy_k| <= 64 HL and
 * |-di Cy_k + dj Cx_k| <= 64 HW: the cells whose centre lies inside the rectangle turned to direction k (64 = S/256;
 * every product stays below 2^22).  (0,0) is in it, it is symmetric about the centre, and as the intersection of four
 * half planes with the lattice every row di of it is one span dj_lo..dj_hi or empty.
 * X. Fit.  d_fits [B][F][G][G] int32: bit k of fits[b][f][i][j] is set iff every cell (i+di, j+dj), (di, dj) in M(f,k),
 * lies inside the grid and is FREE for f; bits A..31 are 0.  d_count [B][F][32] int32: count[b][f][k] = the cells with
 * bit k; words A..31 are 0.
 * B. Best.  d_best [B][F][8] int32 = (ok, i, j, k, dist2, da, poses, cells): poses = the set bits over the frame, cells =
 * the cells with a non-zero word.  The winner over all set (cell, k) is the maximum of one 64-bit key, with
 * d = min(max(dist2[cell], 0), 65536), idx = i*G + j, da = (i-ai)^2 + (j-aj)^2 (below 2^26):
 *   UOC_FOOT_ROOMIEST  ((d + 1) << 23) | ((0x3FFFF - idx) << 5) | (31 - k)
 *   UOC_FOOT_NEAREST   ((2^27 - 1 - da) << 23) | ((0x3FFFF - idx) << 5) | (31 - k)
 * both strict total orders: ties to the lowest idx, then the lowest k.  Without a pose (0, -1, -1, -1, 0, 0, 0, 0); with
 * one ok = 1, dist2 = d of the winning cell and da as above, in both modes.
 * F. Frames.  With d_frame given, a frame whose word 13 is not 1 is a frame without a plane: all-zero fits and count, the
 * no-pose best.  With d_frame == NULL every frame is evaluated as it stands.
 * Every count is a sum of ones and every choice is over a strict total order: the result is defined exactly and does
 * not depend on launch order or batch.
 * ---------------------------------------------------------------------------------------- */
#define UOC_FOOT_MAX_RECTS 8
#define UOC_FOOT_MAX_HALF 16384
#define UOC_FOOT_ROOMIEST 0
#define UOC_FOOT_NEAREST 1

/* 0 for a bad shape: B outside 1..65535, a bad G, A outside 1..32 or F outside 1..8. */
size_t uoc_footprint_workspace_bytes(int B, int G, int A, int F);
/* Ranges as in D and R above; unknown_blocks 0 or 1.  h_dirs and h_rects are read before the call returns and travel as
 * kernel arguments (256 bytes each): no copy.  d_ws 16-byte aligned.  Returns UOC_EINVAL before any device work for null
 * pointers other than d_frame, bad ranges, a workspace below uoc_footprint_workspace_bytes(B, G, A, F) or one that is not
 * 16-byte aligned; uoc_last_error names the argument; a rejected call writes nothing, the workspace included.  Two
 * memsets (the accumulators, d_count) and four launches on `stream`; no host read of device memory, nothing
 * synchronises, no state is kept between calls. */
int uoc_footprint(const int32_t *d_state, const int32_t *d_owner, const int32_t *d_dist2, const int64_t *d_frame, int B, int G,
                  const int32_t *h_dirs, int A, const int32_t *h_rects, int F, int unknown_blocks, int32_t *d_fits,
                  int32_t *d_count, int32_t *d_best, void *d_ws, size_t ws_bytes, void *stream);


/* ------------------------------------------------------------------------------------------
 * Routes: reachability and slide paths on the table grid (no reference counterpart).
 * d_state, d_owner [B][G][G] int32 as uoc_placement writes them, cell index i*G + j, G a multiple of 8 in 8..512; d_frame
 * [B][16] int64 as uoc_placement writes it, nullable.  dist2 is not an input: the stage derives clearance itself, so that
 * an ignored object really is gone.  For up to 8 queries: can a disc get from a source cell to a target cell without
 * being lifted over anything, at what cost, and along which cells.  Every output is an integer.
 *
 * Q. Queries.  h_queries: a HOST array [Q][8] int32, Q in 1..8, record q = (need2, si, sj, ti, tj, ignore, 0, 0): need2 in
 * 0..4096 the squared radius, in cells, of the disc that travels (the need2 of a placement query); the source (si, sj) in
 * [0, G); the target (ti, tj) in [0, G), or (-1, -1) for none; ignore in 0..127, the object being moved (0: none); words 6
 * and 7 are 0.
 * K. Cells.  A cell whose state is outside 0..2, or whose state is 2 with an owner outside 1..127, counts as unknown (K of
 * uoc_grasp and uoc_footprint).  Cell c is FREE for query q when its state is 1; when it is unknown (state 0 included)
 * and unknown_blocks == 0; or when its state is 2, ignore >= 1 and owner == ignore.  A cell outside the grid is never FREE.
 * P. Passable.  Cell c is PASSABLE for q when c is FREE and every offset (di, dj) with di^2 + dj^2 < need2 lands inside the
 * grid on a FREE cell.  need2 == 0 has no offset: PASSABLE = FREE.  Every row of the disc is one span.  With ignore == 0
 * this is "c is not blocking and dist2[c] >= need2" of uoc_placement's step E.
 * M. Moves.  Eight neighbours in this fixed order: (-1,0), (0,-1), (0,1), (1,0), (-1,-1), (-1,1), (1,-1), (1,1).  An
 * orthogonal move costs 5, a diagonal move 7.  A move needs both ends PASSABLE; a diagonal move (di, dj) from (i, j) also
 * needs (i+di, j) and (i, j+dj) PASSABLE (no corner cutting).  A cost is a chamfer length, not a Euclidean one: on an
 * empty grid cost / 5 lies between 0.98995 and 1.07704 times the Euclidean distance in cells.
 * C. Cost.  d_cost [B][Q][G][G] int32: the least total cost of moves from the source, 0 at the source; -1 where the cell is
 * not PASSABLE or not reachable.  A source that is not PASSABLE: -1 everywhere.  cost <= 7 G^2 < 2^21.
 * A. Closest approach.  With a target, over the reached cells (cost >= 0), the maximum of the 64-bit key
 *   ((2^19 - 1 - da) << 39) | ((2^21 - 1 - cost) << 18) | (0x3FFFF - idx),  da = (i-ti)^2 + (j-tj)^2 < 2^19, idx = i*G + j:
 * nearest to the target, then cheapest, then the lowest index; a strict total order.  A reached target wins with da = 0.
 * W. Path.  d_path [B][Q][P][2] int32, P = max_path in 1..4096.  From the closest-approach cell c, step to the first
 * neighbour n in M's order for which the move n -> c is allowed and cost[n] + w == cost[c], until the source.  path[0] is
 * the closest-approach cell; entries up to min(steps, P-1) are written, the rest are (-1, -1); steps is the full number
 * of moves even when the path is cut short.
 * I. d_info [B][Q][8] int32 = (src_ok, ok, ci, cj, cost, steps, reached, passable): src_ok = the source is PASSABLE; ok =
 * the target is given and reached; (ci, cj, cost) the closest-approach cell and its cost; reached and passable count
 * cells.  Without a target, or with src_ok == 0: (src_ok, 0, -1, -1, 0, 0, reached, passable) and a path of (-1, -1).
 * F. Frames.  With d_frame given, a frame whose word 13 is not 1 is a frame without a plane: cost all -1, every info
 * record (0, 0, -1, -1, 0, 0, 0, 0), paths all (-1, -1).  With d_frame == NULL every frame is evaluated as it stands.
 * The cost field is the unique fixpoint of integer relaxations, the key is a strict total order and the walk back follows
 * a fixed order: the result is defined exactly and does not depend on launch order or batch.
 * ---------------------------------------------------------------------------------------- */
#define UOC_ROUTES_MAX_QUERIES 8
#define UOC_ROUTES_MAX_NEED2 4096
#define UOC_ROUTES_MAX_PATH 4096

/* 0 for a bad shape: B outside 1..65535, a bad G or Q outside 1..8. */
size_t uoc_routes_workspace_bytes(int B, int G, int Q);
/* Ranges as in Q above; unknown_blocks 0 or 1; max_path in 1..4096.  h_queries is read before the call returns and travels
 * as a kernel argument: no copy.  d_ws 16-byte aligned.  Returns UOC_EINVAL before any device work for null pointers other
 * than d_frame, bad ranges, non-zero words 6 or 7, a bad shape, a workspace below uoc_routes_workspace_bytes(B, G, Q) or
 * one that is not 16-byte aligned; uoc_last_error names the argument; a rejected call writes nothing, the workspace
 * included.  One memset and three launches on `stream`; no host read of device memory, nothing synchronises, no state is
 * kept between calls.  After the call the first B*Q int32 words of the workspace hold the relaxation sweeps each (frame,
 * query) took: a diagnostic for measurements, not a result. */
int uoc_routes(const int32_t *d_state, const int32_t *d_owner, const int64_t *d_frame, int B, int G, const int32_t *h_queries,
               int Q, int unknown_blocks, int max_path, int32_t *d_cost, int32_t *d_info, int32_t *d_path, void *d_ws,
               size_t ws_bytes, void *stream);


/* ------------------------------------------------------------------------------------------
 * Label confidence: assignment margins per pixel and per object (no reference counterpart).
 * The nearest-seed assignment (uoc_ms_assign) picks per pixel the seed of smallest cosine distance; how far the nearest
 * seed of ANOTHER seed component lies behind it is how close the pixel came to carrying another label.
 *
 * M. uoc_ms_confidence.  Layouts of uoc_ms_assign / uoc_ms_cluster_wide: d_X [batch][halves][n][64], d_Z
 * [batch][halves][m][64], d_seed_labels [batch][m], d_num_unique [batch]; halves 1 or 2, 1 <= m <= 128, 1 <= n <= 2^30.
 * Per pixel p, with S(p, s) the fp32 MFMA dot product of uoc_ms_assign (same staging, same order):
 *   d(p, s)  = 0.5f * (1.0f - S(p, s))
 *   best(p)  = argmin_s d, ties to the lowest s;  c1 = seed_labels[best]
 *   rival(p) = argmin of d over the seeds with seed_labels[s] != c1, ties to the lowest s; -1 when every seed carries c1
 *   margin(p) = d(p, rival) - d(p, best) in fp32, >= 0 by construction; 1.0f without a rival (the largest value a
 *               difference of cosine distances can take)
 *   labels(p) = seed_labels[best] after the "largest cluster becomes label 0" swap of uoc_ms_assign (only labels in
 *               range(num_unique) are counted, the first maximum wins, 0 and that label change places)
 *   second(p) = the same swap applied to seed_labels[rival], or -1
 *   closest(p) = best(p)
 * d_labels [batch][n] int32 and d_margin [batch][n] float are required; d_second, d_closest, d_rival [batch][n] int32 are
 * nullable.  d_labels and d_closest are bit-identical to what uoc_ms_assign writes for the same inputs (the two
 * kernels share the code that computes and stores them).  A pixel no seed wins (a NaN row) gets label 0 and closest = INT_MAX as there, and margin = 1.0f,
 * second = rival = -1; labels outside 0..127 are left out of the histogram.  Minima over a fixed set with index
 * tie-breaks: the result does not depend on launch order or batch.
 * metric must be UOC_METRIC_COSINE; UOC_METRIC_EUCLIDEAN is not built (the square root near zero needs its own error
 * analysis) and returns UOC_EINVAL saying so.
 * Returns UOC_EINVAL before any device work for null required pointers, bad ranges, d_X or d_Z not 16-byte aligned, a
 * workspace below uoc_ms_confidence_workspace_bytes or not 16-byte aligned, an output that overlaps an input (d_labels
 * aliasing d_X, ...) or another output; uoc_last_error names the argument; a rejected call writes nothing.  One memset
 * and two or three launches on `stream`; no host read of device memory, nothing synchronises, no state is kept between
 * calls.
 *
 * P. uoc_conf_paste carries crop-level values into the frame along the paint plan of uoc_roi_match.  d_values_crop
 * [K][S*S] float; d_labels_crop [K][S*S] int32 and d_table as given to uoc_roi_match; d_plan [K + K*128] int32, the
 * paint order followed by the id map, exactly as uoc_roi_match writes it; d_out [H*W] float.  A frame pixel gets the
 * value of the crop pixel whose (mapped, non-zero) label uoc_roi_paste leaves there: the same nearest-resize source
 * index, and a later ROI of the order overwrites an earlier one.  A pixel that nothing paints is LEFT UNTOUCHED: the
 * caller pre-fills d_out.  K in 1..127, S in 1..4096, H*W in 1..2^30.  UOC_EINVAL before any device work for null
 * pointers, bad ranges or a d_out [H*W] that overlaps d_values_crop, d_labels_crop, d_table or d_plan anywhere (the kernel
 * reads them while it writes); uoc_last_error names the argument.  One launch.
 *
 * O. uoc_conf_objects summarises any (label map, value map) pair per id, in integers.  d_labels [B][H*W] int32, d_conf
 * [B][H*W] float, weak_q in 0..65535.  Per pixel q = 0 when conf is NaN or negative, else min(65535, (int)(conf *
 * 65536.0f)): the product is exact, the conversion truncates.  d_stats [B][128][4] int64 = (pixels, sum_q, min_q, weak)
 * for label l in 0..127 (row 0: the background); labels outside 0..127 are ignored; weak counts the pixels with q <
 * weak_q; min_q = 0 when pixels == 0.  Sums of integers and a minimum: defined exactly, independent of launch order and
 * batch.  B in 1..65535, H*W in 1..2^30, d_stats 8-byte aligned.  UOC_EINVAL before any device work for null pointers or
 * bad ranges.  One memset and two launches.
 * ---------------------------------------------------------------------------------------- */
#define UOC_CONF_MAX_N (1 << 30)
#define UOC_CONF_ONE 65536          /* the fixed-point unit of uoc_conf_objects' q */

/* 0 for a bad shape: batch outside 1..65535, n outside 1..2^30, m outside 1..128, halves not 1 or 2. */
size_t uoc_ms_confidence_workspace_bytes(int batch, int n, int m, int halves);
int uoc_ms_confidence(const float *d_X, int halves, int batch, int n, const float *d_Z, const int32_t *d_seed_labels,
                      const int32_t *d_num_unique, int m, int metric, int32_t *d_labels, float *d_margin,
                      int32_t *d_second, int32_t *d_closest, int32_t *d_rival, void *d_ws, size_t ws_bytes, void *stream);
int uoc_conf_paste(const float *d_values_crop, const int32_t *d_labels_crop, const uoc_roi_table *d_table,
                   const int32_t *d_plan, int K, int S, int H, int W, float *d_out, void *stream);
int uoc_conf_objects(const int32_t *d_labels, const float *d_conf, int B, int H, int W, int weak_q, int64_t *d_stats,
                     void *stream);


/* ------------------------------------------------------------------------------------------
 * Surface normals: per-pixel normals and object faces (no reference counterpart).
 * d_xyz [B][3][H][W] fp32 metres; d_labels [B][H][W] int32, nullable; d_planes [B] as uoc_support_plane writes them or
 * filled in by the caller, nullable.  H*W below 2^31.  Pixels are (row, column).  Everything but d_unit is an integer.
 *
 * P. Points.  A pixel is valid when x, y, z are finite, z > 0 and q_c = (int) rintf(c * 16000.0f) (fp32 product, round
 * half to even) has |q_c| <= 524287 for c = x, y, z: the unit is 1/16 mm, a depth in whole millimetres is represented
 * exactly.  id(p) = L when 1 <= L <= 127, else 0; without labels every id is 0.
 * D. Pairs, r = step.  The horizontal pair at pixel m has the ends a = m - (0, r) and b = m + (0, r); it exists when both
 * ends lie inside the image and are valid, id(a) == id(b), and d = q(b) - q(a) has |d_z| <= 16 jump_mm and |d_x|, |d_y| <=
 * 16383.  The vertical pair is the same with (r, 0).
 * T. Tangents, s = window.  For pixel p: TX = the sum of d over the horizontal pairs at the (2s+1)^2 pixels m with
 * |m - p| <= s in both coordinates whose id(a) == id(p), nX their number; TY, nY likewise over the vertical pairs.
 * |T_c| <= 81 * 16383 < 2^21.
 * N. Normal.  p has a normal when it is valid, nX >= min_pairs, nY >= min_pairs and n' != 0, where N = TY x TX in int64
 * (|N_c| < 2^43; a visible surface of an organised cloud then faces the camera, there is no sign search), k = max(0,
 * bitlength(max_c |N_c|) - 30) and n'_c = N_c >> k, an arithmetic shift (|n'_c| <= 2^30).  grazing = (n' . (q >> 4) >= 0),
 * again an arithmetic shift; the sum stays below 2^48.
 * C. Class, only with a plane record that rule F of uoc_placement accepts; Pq, Uq, Vq are its N, U, V (units of 2^-14,
 * magnitude <= 32768).  c = n' . Pq (below 2^47), L = floor(sqrt(n' . n')), exact (n' . n' < 2^62).  The first rule that
 * applies: UOC_NORMAL_UP when c * 16384 >= c_up * L; UOC_NORMAL_DOWN when -c * 16384 >= c_up * L; UOC_NORMAL_SIDE when
 * |c| * 16384 <= s_side * L; else UOC_NORMAL_OBLIQUE.  Every product stays below 2^61.  Without a plane (d_planes NULL,
 * or a record that rule F rejects) the class is 0.
 * Z. Azimuth of a SIDE pixel.  a = n' . Uq, b = n' . Vq; the bin is the k in 0..A-1 with the largest a Cx_k + b Cy_k
 * (below 2^62), ties to the lowest k.  h_dirs: a HOST array [A][2] int32 of (Cx_k, Cy_k), each component in
 * [-16384, 16384], A in 1..32.  The bin of any other pixel is 0.  No kernel calls a trigonometric function.
 * Outputs.  d_n [B][H][W][4] int32 = (n'_x, n'_y, n'_z, info), info = class | grazing << 3 | bin << 8 | nX << 16 |
 * nY << 24; all zero without a normal.  d_unit [B][3][H][W] fp32, nullable = (float)((double) n'_c / sqrt((double)(n' . n'))),
 * NaN without a normal.  d_faces [B][128][40] int32, row a = id 0..127 (row 0: the background) = (pixels, with_normal,
 * up, side, oblique, down, grazing, peak) and the histogram [32] of the azimuth bins of the id's SIDE pixels: pixels
 * counts every pixel of the id, valid or not, the others count pixels with a normal; peak = the fullest bin, ties to the
 * lowest, -1 when side == 0.
 * Every count is a sum of ones and every choice is over a strict total order: the result is defined exactly and does
 * not depend on launch order or batch.
 * ---------------------------------------------------------------------------------------- */
#define UOC_NORMAL_UP 1
#define UOC_NORMAL_SIDE 2
#define UOC_NORMAL_OBLIQUE 3
#define UOC_NORMAL_DOWN 4
#define UOC_NORMALS_MAX_DIRS 32
#define UOC_NORMALS_FACE_WORDS 40

/* 0 for a bad shape (B outside 1..65535, H*W not below 2^31). */
size_t uoc_normals_workspace_bytes(int B, int H, int W);
/* step in 1..8, window in 0..4, jump_mm in 1..1000, min_pairs in 1..(2 window + 1)^2, A in 1..32, c_up and s_side in
 * 0..2^28 with c_up > s_side (the wrapper: c_up = rint(cos(up_deg) 2^28), s_side = rint(sin(side_deg) 2^28)).  h_dirs is
 * read before the call returns and travels as a kernel argument.  d_n and d_ws 16-byte aligned.  Returns UOC_EINVAL
 * before any device work for null d_xyz / d_n / d_faces / h_dirs / d_ws, bad ranges, a bad shape, a d_n that is not
 * 16-byte aligned, a workspace below uoc_normals_workspace_bytes(B, H, W) or one that is not 16-byte aligned;
 * uoc_last_error names the argument; a rejected call writes nothing, the workspace included.  One memset (the face
 * accumulators in the workspace) and two launches on `stream`; no host read of device memory, nothing synchronises, no
 * state is kept between calls. */
int uoc_normals(const float *d_xyz, const int32_t *d_labels, const uoc_plane *d_planes, int B, int H, int W, int step,
                int window, int jump_mm, int min_pairs, const int32_t *h_dirs, int A, int c_up, int s_side, int32_t *d_n,
                float *d_unit, int32_t *d_faces, void *d_ws, size_t ws_bytes, void *stream);


/* ------------------------------------------------------------------------------------------
 * Re-identification: appearance signatures and identities (no reference counterpart).  The
 * tracker keeps an id while masks overlap; this layer gives an object the same id again after a jump with IoU 0 or an
 * occlusion longer than max_age, by what it looks like.  Integers only; the result is defined exactly and does not
 * depend on launch order or batch.  id(p) = L when 1 <= L <= 127, else 0 (background).
 *
 * S. Signature of an id: UOC_SIG_WORDS = 104 int32.  Word 0 pixels n; word 1 valid = its pixels with z_mm >= 0, where
 * z_mm = (int) rintf(z * 1000.0f) when z > 0 && z <= 65, else -1 (NaN: -1), 0 without d_xyz; words 2, 3 the low and
 * high word of the unsigned 64-bit sum over the valid pixels of (z_mm * z_mm) >> 10, a visible metric area up to a
 * constant; words 4..7 zero; words 8..88 the chromaticity histogram, 9 x 9, bin 8 + iu * 9 + iv; word 89 =
 * UOC_SIG_DARK the dark bin; words 90..98 the intensity histogram; words 99..103 zero.  Row 0 and the rows of absent
 * ids are all zero.
 * Votes of a pixel with the bytes (b, g, r) and s = b + g + r.  Chroma when s >= 48: u = (64 b) / s, v = (64 g) / s,
 * ul = u >> 3, uf = u & 7, vl = v >> 3, vf = v & 7; bin (ul + du, vl + dv), du, dv in {0, 1}, gets the weight
 * (du ? uf : 8 - uf) * (dv ? vf : 8 - vf); a zero weight is no vote, so ul == 8 never reaches a row 9.  Dark when s < 48:
 * 64 into the dark bin.  Intensity always: y = s / 3, yl = y >> 5, yf = (y & 31) >> 2; 8 (8 - yf) into bin yl and, when
 * yf != 0, 8 yf into bin yl + 1.  Every pixel adds 64 to the chroma / dark part and 64 to the intensity part.
 * Stored: q = (h * 768) / n for the chroma and dark bins, (h * 256) / n for the intensity bins, h the raw 32-bit counter,
 * the product in 64 bits: a signature sums to at most 65536.  A counter holds at most 64 n, hence H*W <= UOC_SIG_MAX_N.
 * M. Similarity.  sim(a, b) = the sum over the words 8..98 of min(qa, qb), 0 when either pixels is 0; in 0..65536.
 * I. Identities.  State per stream (caller-owned device memory, uoc_ident_state_bytes(B) / B bytes each, 16-byte
 * aligned): int32 [1024] header = the table [128][5] = pid, uid, seen, hits, pixels (entry 0 unused; pid 0 = free, all
 * zero), then at word 640 the pids handed out, the step counter and `evicted`; then the entries' last signatures
 * [128][104].  An all-zero state is a reset stream.  One step with the tracker's table T (after its step) and the
 * signatures S of the TRACKED map, so both keyed by track slot; the uids of T's slots are distinct:
 *  1. step += 1; an entry with pid != 0 and step - seen > max_lost is zeroed.
 *  2. Slot s is visible when T[s].uid != 0, T[s].age == 0 and S[s].pixels > 0.  A visible slot whose uid is an entry's
 *     uid is bound to it; the other visible slots are newcomers; entries with pid != 0 bound to no slot are lost.
 *  3. Candidates: (newcomer s, lost e) with sim(S[s], sig[e]) >= q and, when r > 0, both areas non-zero and
 *     min(As, Ae) * 256 >= r * max(As, Ae) in 64 bits.
 *  4. Greedy matching: the candidate of largest sim among unmatched s and e; ties: larger seen, lower e, lower s.  A
 *     match binds s to e and sets e.uid = T[s].uid.
 *  5. The newcomers left, in ascending s, take the free entries in ascending order (those freed in 1 included); with
 *     none free, the lost entry left with the smallest seen (ties: lower e), and `evicted` grows.  Such an entry gets
 *     pid = ++pids, hits = 0 and the newcomer's uid.
 *  6. Every bound pair: seen = step, hits += 1, pixels and the signature are S[s]'s, lut[s] = e; every other lut word
 *     is 0.  out = lut[id(tracked)].
 * Out of scope: position or motion costs, telling two look-alike objects apart (the tie rule decides), blending
 * signatures over time.
 * ---------------------------------------------------------------------------------------- */
#define UOC_SIG_WORDS 104
#define UOC_SIG_MAX_N (1 << 24)
#define UOC_SIG_PIXELS 0
#define UOC_SIG_VALID 1
#define UOC_SIG_AREA 2                 /* words 2, 3 */
#define UOC_SIG_HIST 8                 /* words 8..88: chroma bin 8 + iu * 9 + iv */
#define UOC_SIG_DARK 89
#define UOC_SIG_INTENSITY 90           /* words 90..98 */
#define UOC_IDENT_WORDS 5              /* an entry of the table: pid, uid, seen, hits, pixels */
#define UOC_IDENT_HEADER_WORDS 1024    /* int32 words of a stream's state before its signatures */
#define UOC_IDENT_META_WORD 640        /* words 640, 641, 642 = pids handed out, step, evicted */

/* 0 for B outside 1..65535. */
size_t uoc_signature_workspace_bytes(int B);
/* d_labels [B][H*W] int32; d_image [B][H*W][3] uint8, BGR; d_xyz [B][3][H*W] fp32, nullable; d_sig [B][128][104].  The
 * workspace holds the vote accumulators: it must be ALL ZERO before the first call that uses it and every call leaves
 * it all zero, so it is zeroed once, not per call.  d_sig and d_ws 16-byte aligned.  Returns UOC_EINVAL before any
 * device work for null d_labels / d_image / d_sig / d_ws, a bad shape, H*W above UOC_SIG_MAX_N, a short workspace.
 * Two launches on `stream`, nothing synchronises. */
int uoc_signature(const int32_t *d_labels, const uint8_t *d_image, const float *d_xyz, int B, int H, int W, int32_t *d_sig,
                  void *d_ws, size_t ws_bytes, void *stream);
/* d_sim [B][128][128]: d_sim[b][i][j] = sim(d_sig_a[b][i], d_sig_b[b][j]).  Signatures 16-byte aligned. */
int uoc_sig_similarity(const int32_t *d_sig_a, const int32_t *d_sig_b, int B, int32_t *d_sim, void *stream);
size_t uoc_ident_state_bytes(int B);
size_t uoc_ident_workspace_bytes(int B);
/* Zeroes the state of stream `which`, or of all B streams when which = -1. */
int uoc_ident_reset(void *d_state, int B, int which, void *stream);
/* d_tracked, d_out [B][H*W] int32 (distinct buffers), H*W below 2^31; d_tracks [B][128]; d_sig [B][128][104]; q = round(min_sim * 65536) in [1, 65536]; r = round(min_size *
 * 256) in [0, 256]; max_lost >= 0; d_lut (nullable) [B][128]: slot -> entry of this step; d_ident (nullable)
 * [B][128][5]: the table after the step.  Where d_lut / d_ident are given, every word of them is written (row 0, invisible
 * slots and free entries are zero): they need no initialisation.  d_state, d_ws and d_sig 16-byte aligned.  Two launches on
 * `stream`, nothing synchronises. */
int uoc_ident_step(const int32_t *d_tracked, const uoc_track *d_tracks, const int32_t *d_sig, int B, int H, int W, int q, int r,
                   int max_lost, void *d_state, int32_t *d_out, int32_t *d_lut, int32_t *d_ident, void *d_ws, size_t ws_bytes,
                   void *stream);

/* ------------------------------------------------------------------------------------------
 * Object motion: planar registration on the table grid.  How an object that stays on the table
 * moved between two frames: a rotation about the plane normal and an in-plane shift, found by an exhaustive integer
 * search over both.  Inputs are the state / owner grids of uoc_placement for the same B frames "before" (x = a) and
 * "after" (x = b), rasterised in ONE plane frame, a host table of A rotations, a radius R and P host pairs (id_a, id_b).
 *  C. Cell (i, j) of grid x belongs to id `a` iff its state is 2 and its owner is exactly `a`.  n_a, n_b: the counts;
 *     still = n_a + n_b - 2 |A n B|, the cost of "did not move".
 *  P. The pivots p = (floor_div(2 sum(i) + n_a, 2 n_a), floor_div(2 sum(j) + n_a, 2 n_a)) over A's cells, q the same
 *     over B's.
 *  T. S = 16384.  h_rot[k] = (Cx_k, Cy_k) = (rint(cos(2 pi k / A) S), rint(sin(2 pi k / A) S)), a full turn; every word
 *     in -S..S.  rd(x) = floor_div(2 x + S, 2 S).  Forward F_k(di, dj) = (rd(di Cx - dj Cy), rd(di Cy + dj Cx)); inverse
 *     I_k(ei, ej) = (rd(ei Cx + ej Cy), rd(-ei Cy + ej Cx)).  Every product stays below 2^24.
 *  X. For k in 0..A-1 and a shift s = (si, sj), |si|, |sj| <= R:
 *       cost(k, s) = #{c in A : q + s + F_k(c - p) not in B} + #{c' in B : p + I_k(c' - q - s) not in A}.
 *     A cell outside the grid is in neither set.
 *  K. The answer is the minimum of the key (cost << 33) | (s2 << 23) | (kk << 17) | (k << 11) | sidx with s2 = si^2 +
 *     sj^2, kk = min(k, A - k), sidx = (si + R)(2R + 1) + (sj + R): least cost, then least shift, then least turn, then
 *     lowest k, then lowest shift index.  A strict total order.
 *  O. d_rot[b][p][k] = (cost, si, sj, 0), the key's minimum over s for that k; rows k >= A are (-1, 0, 0, 0).
 *     d_best[b][p] = 16 words (status, k, si, sj, cost, n_a, n_b, still, pi, pj, qi, qj, ti, tj, second, 0) with
 *     t = q + s - p, the pivot's travel in cells, and second = the least d_rot cost over the rotations at circular
 *     distance >= 2 from k, -1 when there is none.
 *  S. status 1: evaluated.  0: no common frame (frame records given, and word 13 of either is not 1 or the 16 words of
 *     the two differ).  2: n_a = 0 or n_b = 0.  3: n_a or n_b above UOC_MOTION_MAX_CELLS.  For a status other than 1,
 *     d_best is (status, -1, 0, 0, 0, n_a, n_b, 0, 0...) and every d_rot row is (-1, 0, 0, 0); n_a = n_b = 0 for status
 *     0.  With both frame pointers NULL every frame is evaluated as it stands.
 * Out of scope: heights, out-of-plane motion, objects leaving the plane, partial occlusion, sub-cell refinement, more
 * than 64 rotations.
 * ---------------------------------------------------------------------------------------- */
#define UOC_MOTION_MAX_ROT 64
#define UOC_MOTION_MAX_RADIUS 16
#define UOC_MOTION_MAX_PAIRS 16
#define UOC_MOTION_MAX_CELLS 4096
#define UOC_MOTION_SCALE 16384
#define UOC_MOTION_ROT_WORDS 4
#define UOC_MOTION_BEST_WORDS 16

/* 0 for B outside 1..65535, G not a multiple of 8 in 8..512, A outside 1..64, P outside 1..16. */
size_t uoc_motion_workspace_bytes(int B, int G, int A, int P);
/* d_state_x, d_owner_x [B][G][G] int32; d_frame_a, d_frame_b [B][16] int64 or both NULL; h_rot [A][2] and h_pairs [P][2]
 * on the host, read before the call returns; d_rot [B][P][64][4], d_best [B][P][16] int32.  Returns UOC_EINVAL before any
 * device work, outputs and workspace untouched, for null pointers other than the two frame pointers, one frame pointer
 * NULL and one not, B / G / A / R / P out of range, a table word outside -S..S, an id outside 1..127, a workspace below
 * uoc_motion_workspace_bytes(B, G, A, P) or one that is not 16-byte aligned.  One memset and three launches on `stream`,
 * nothing synchronises. */
int uoc_motion(const int32_t *d_state_a, const int32_t *d_owner_a, const int64_t *d_frame_a, const int32_t *d_state_b,
               const int32_t *d_owner_b, const int64_t *d_frame_b, int B, int G, const int32_t *h_rot, int A, int R,
               const int32_t *h_pairs, int P, int32_t *d_rot, int32_t *d_best, void *d_ws, size_t ws_bytes, void *stream);

/* ------------------------------------------------------------------------------------------
 * Scene memory: the table grid fused over time.  A per-stream memory of the state / owner grids
 * of uoc_placement: cells observed in this frame overwrite it, cells not observed keep what was last seen there for at
 * most max_age steps, and a cell whose observation contradicts the memory is flagged.  The fused grids have the
 * meaning of uoc_placement's, so every stage that takes those takes these.  Integers only.
 * State.  Caller-owned, 16-byte aligned, uoc_scene_state_bytes(B, G) bytes; stream b at b * (that / B).  Per stream:
 *     int64 [16]   the lattice record: the frame record (uoc_placement's d_frame) of the grid the memory lives on
 *     int32 [16]   meta: word 0 = steps taken, word 1 = restarts, the rest 0
 *     int32 [G*G]  memory words  state | owner << 8 | age << 16,  state 0..2, owner 0..127, age 0..32767: never negative
 *   In int32 words: the meta at UOC_SCENE_META_WORD, the memory at UOC_SCENE_MEM_WORD.  All zero is a reset stream.
 *  L. The lattice, per frame.  With d_frame given and word 13 (found) of the frame's record not 1: status 0, the
 *     stream's state is untouched, state / owner / dist2 / change / ids / answers are those of a frame without a plane
 *     in uoc_placement (zeros, (-1, -1, 0, 0) per query), age is -1 everywhere and info = (0, steps, 0, ...).  With a
 *     record given and steps > 0, if the stored record differs from it in any of the 16 words: a restart, every memory
 *     word counts as 0 for this step, restarts goes up by 1 and the status is 2.  Otherwise the status is 1.  The given
 *     record is stored on the first step (steps = 0) and on a restart.  d_frame == NULL: the lattice is the caller's
 *     word, nothing is compared or stored, status 1.  With status 1 and 2 steps goes up by 1.
 *  N. The current cell: s = state_cur when that is 1 or 2, else 0; o = owner_cur when s == 2 and 1 <= owner_cur <= 127,
 *     else 0 (an obstacle without an id keeps owner 0 and is a real obstacle).
 *  U. The update, with the memory word (ms, mo, ma).
 *     Observed, s != 0: the new word is (s, o, 0); the change code against the old word is APPEARED (1) when ms == 1
 *     and s == 2, VANISHED (2) when ms == 2 and s == 1, REOWNED (3) when ms == 2, s == 2 and mo != o, else SAME (0),
 *     also when ms == 0.
 *     Not observed, s == 0: kept as (ms, mo, ma + 1) when ms != 0, ma < max_age and not (ms == 2 and bit mo of the
 *     frame's drop mask is set); the drop mask is 128 bits, bit a = bit (a & 31) of word d_drop[b][a >> 5], no bits
 *     with d_drop == NULL.  Otherwise forgotten: the word becomes 0.  The change code is 0.
 *     Per cell: state and owner come from the new word; age is 0 where observed, ma + 1 where kept, -1 where the new
 *     word is 0; change is the change code.
 *  E. Clearance on the fused grid, rule E of uoc_placement: a cell is blocking when its fused state is 2, or 0 with
 *     unknown_blocks; every cell outside the grid is blocking; dist2 is the exact squared Euclidean distance, in cells,
 *     to the nearest blocking cell.
 *  Q. Queries on the fused grid, rule Q of uoc_placement: the candidates are the cells of fused state 1, the same keys
 *     and ties.
 *  T. ids[b][a][8] for a = 0..127 (row 0: the obstacles without an id):
 *       0 cells_now     observed obstacle cells with o == a          4 vanished     VANISHED cells with mo == a
 *       1 cells_kept    kept obstacle cells with mo == a             5 reowned_in   REOWNED cells with o == a
 *       2 oldest        the largest age among them, 0 without one    6 reowned_out  REOWNED cells with mo == a
 *       3 appeared      APPEARED cells with o == a                   7 forgotten    memory obstacle cells with mo == a
 *                                                                                   forgotten in this step, by age or drop
 *     info[b][8] = (status, steps after this step, observed cells, kept cells, forgotten cells of any state, appeared,
 *     vanished, reowned).  Every count is a sum of ones and oldest a maximum: no result depends on launch order or on
 *     the other frames of the batch.
 * Out of scope: a moving camera (a new plane is a restart), deciding that a remembered object has moved away (the
 * caller says so through d_drop), heights, blending or voting over several sightings, image-space label smoothing.
 * ---------------------------------------------------------------------------------------- */
#define UOC_SCENE_META_WORD 32         /* int32 words of a stream's state before its meta words */
#define UOC_SCENE_MEM_WORD 48          /* ... and before its memory words */
#define UOC_SCENE_MAX_AGE 32767
#define UOC_SCENE_ID_WORDS 8
#define UOC_SCENE_INFO_WORDS 8
#define UOC_SCENE_SAME 0
#define UOC_SCENE_APPEARED 1
#define UOC_SCENE_VANISHED 2
#define UOC_SCENE_REOWNED 3

/* B * (192 + 4 G G); 0 for B outside 1..65535 or G not a multiple of 8 in 8..512. */
size_t uoc_scene_state_bytes(int B, int G);
size_t uoc_scene_workspace_bytes(int B, int G);
/* Zeroes the state of stream `which`, or of all B streams when which = -1.  UOC_EINVAL for a null or misaligned state,
 * a bad B or G, which outside -1..B-1. */
int uoc_scene_reset(void *d_state, int B, int G, int which, void *stream);
/* d_state_cur, d_owner_cur [B][G][G] int32; d_frame (nullable) [B][16] int64; d_drop (nullable) [B][4] int32; h_queries
 * [Q][4] on the host as for uoc_placement, read before the call returns; d_mem: the state; d_state, d_owner, d_dist2,
 * d_age, d_change [B][G][G], d_ids [B][128][8], d_info [B][8], d_answers [B][Q][4] int32.  Returns UOC_EINVAL before any
 * device work, outputs, state and workspace untouched, for null pointers other than d_frame, d_drop and, with Q = 0,
 * h_queries and d_answers; B outside 1..65535; G not a multiple of 8 in 8..512; max_age outside 0..32767;
 * unknown_blocks neither 0 nor 1; Q outside 0..16 or a query out of uoc_placement's ranges; a workspace below
 * uoc_scene_workspace_bytes(B, G); a state or workspace that is not 16-byte aligned.  One memset and two launches on
 * `stream`, a third with queries; nothing synchronises. */
int uoc_scene_step(const int32_t *d_state_cur, const int32_t *d_owner_cur, const int64_t *d_frame, const int32_t *d_drop,
                   int B, int G, int max_age, int unknown_blocks, const int32_t *h_queries, int Q, void *d_mem,
                   int32_t *d_state, int32_t *d_owner, int32_t *d_dist2, int32_t *d_age, int32_t *d_change,
                   int32_t *d_ids, int32_t *d_info, int32_t *d_answers, void *d_ws, size_t ws_bytes, void *stream);


/* ------------------------------------------------------------------------------------------
 * Host-side data formats (no device work) — what the dataset loaders need in place of python-pcl
 * (lib/datasets/ocid_object.py:105, osd_object.py:92): LZF decoder for `DATA binary_compressed` PCD files.
 * `in`/`out` are HOST pointers.  Returns the number of bytes written or a negative code.
 * ---------------------------------------------------------------------------------------- */
long uoc_lzf_decompress(const uint8_t *in, size_t in_len, uint8_t *out, size_t out_cap);

/* ------------------------------------------------------------------------------------------
 * Opt-in per-kernel timing (HIP events on the launch stream).  Single-threaded use.
 * uoc_prof_report writes a JSON array [{kernel, launches, total_ms, flops, bytes}, ...] where
 * flops/bytes are the ALGORITHMIC totals of the recorded launches.
 * ---------------------------------------------------------------------------------------- */
int uoc_prof_enable(int on);
int uoc_prof_reset(void);
int uoc_prof_report(char *buf, size_t cap);

#ifdef __cplusplus
/* The record sizes a binding's struct mirrors are held to. */
static_assert(sizeof(uoc_roi_table) == 2564, "uoc_roi_table");
static_assert(sizeof(uoc_object) == 164, "uoc_object");
static_assert(sizeof(uoc_track) == 20, "uoc_track");
static_assert(sizeof(uoc_plane) == 84, "uoc_plane");
static_assert(sizeof(uoc_plane_object) == 64, "uoc_plane_object");
static_assert(sizeof(uoc_plane_info) == 32, "uoc_plane_info");
static_assert(sizeof(uoc_relation_object) == 44, "uoc_relation_object");
#endif

#ifdef __cplusplus
}
#endif
#endif /* UOC_HIP_H */
