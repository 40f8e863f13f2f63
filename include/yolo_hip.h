/*
 * yolo_hip.h -- C ABI of libyolo_hip.so, the MI355X (gfx950) implementation of the YOLOv1 hot path.
 *
 * The reference (mattiaskvist/yolo-v1) is pure Python with no FFI layer; its hot path is the
 * arithmetic behind the `src/yolo` module surface.  This header is the boundary a
 * maintainer binds instead of the torch ops those modules call: every entry point names the
 * reference lines it replaces.  INTEGRATION.md shows the ctypes binding.
 *
 * Conventions
 *   - extern "C", plain pointers and sizes, no torch types.  All pointers are DEVICE pointers
 *     unless a parameter is called host_*.
 *   - `stream` is a hipStream_t passed as void* (NULL = the null stream).  Calls only enqueue
 *     work; nothing here synchronises, allocates or frees device memory, so every call can be
 *     captured in a hipGraph.  Workspaces are caller-allocated.
 *   - return value: 0 = ok, <0 = YOLO_E_* argument error, >0 = hipError_t.  No exceptions cross
 *     the ABI.  yolo_hip_last_error() gives a human-readable string for the calling thread.
 *   - activations inside the network are "padded NHWC bf16": [N][H+2*halo][W+2*halo][C] with a
 *     zero border of `halo` pixels that producers never write (so 3x3/pad-1 consumers need no
 *     bounds checks).  The caller zeroes a buffer once at allocation.
 */
#ifndef YOLO_HIP_H
#define YOLO_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 2: yolo_igemm_desc gained tile_px / split_slabs, yolo_wgrad_desc gained dw_sumsq / slabs / slab_floats, the multi-tensor Adam entries
 *    gained skip_flag.  A binding must refuse a library whose version differs from the header it was
 *    written against (yolo/_hip.py does): the descriptors are passed by pointer and a shorter struct would be read past its end. */
#define YOLO_HIP_ABI_VERSION 2

#define YOLO_E_ARG (-1)         /* bad argument (null pointer, size out of range)              */
#define YOLO_E_UNSUPPORTED (-2) /* shape not supported by the kernels (see each function)      */

typedef void *yolo_stream_t;

int yolo_hip_abi_version(void);
const char *yolo_hip_last_error(void);
/* Diagnostics (libyolo_hip_diag.so, `make diag`, -DIGEMM_STAMPS): the staggered yolo_igemm configurations write eight
 * s_memtime stamps of K iteration `k_iter` per wave of the first 512 workgroups to buf[(workgroup * 8 + wave) * 8 + i]
 * (int64, device memory of 512 * 64 entries; NULL switches it off).  The product library compiles no stamps and returns
 * YOLO_E_UNSUPPORTED for a non-NULL buffer.  tools/stamps_igemm.py reads them. */
int yolo_debug_stamps(void *buf, int k_iter);
/* A non-blocking HIP stream on the current device: of the lowest scheduling priority the device offers (low != 0) or of the
 * default one.  For work off the critical path (weight gradients beside the data-gradient chain, a deferred optimizer pass):
 * the dispatcher then prefers the main chain's workgroups.  The stream lives until the process ends. */
int yolo_stream_create(int low, yolo_stream_t *out);

/* ---------------------------------------------------------------------------------------------
 * Post-processing: S x S x B box decode, pairwise IoU, per-image NMS.  fp64 arithmetic on fp32
 * inputs in the reference's operation order -> bit-exact records, class ids and kept indices.
 * ------------------------------------------------------------------------------------------- */

/* Replaces YOLOInference.parse_predictions (src/yolo/inference.py:170-210) and
 * mAPMetric._parse_predictions (src/yolo/metrics.py:185-218) for a whole batch.
 *   pred    [N][S][S][5B+C] fp32
 *   rec     [N][S*S*B][6] f64 = {class_id, conf*prob, x, y, w, h}; per image the first counts[n]
 *           rows are valid, in (row i, col j, box b) scan order
 *   counts  [N] int32
 * Limits: S*S*B <= 1024, B <= 8. */
int yolo_decode(const float *pred, int N, int S, int B, int C, double conf_thr,
                double *rec, int32_t *counts, yolo_stream_t stream);

/* Class-specific scores (YOLOv1 paper section 2; Darknet get_detection_boxes): every box b of every cell is a candidate
 * of EVERY class c with score (double)conf_b * (double)prob_c, kept iff score > conf_thr.  One launch, one workgroup per
 * (image, class).
 *   pred    [N][S][S][5B+C] fp32
 *   rec     [N][C][S*S*B][6] f64 = {c, score, x, y, w, h} (x, y, w, h as yolo_decode); of group (n, c) the first
 *           counts[n][c] rows are valid, in (row i, col j, box b) scan order; the rows behind them are not written
 *   counts  [N][C] int32
 * rec viewed as N*C images of S*S*B records is what yolo_nms and yolo_map_match take (all records of a group share one class).
 * Limits: S*S*B <= 1024, B <= 8 (those of yolo_decode).  YOLO_E_ARG on a null pointer, N < 0 or C < 1; N == 0 succeeds. */
int yolo_decode_classes(const float *pred, int N, int S, int B, int C, double conf_thr,
                        double *rec /*[N][C][S*S*B][6]*/, int32_t *counts /*[N][C]*/, yolo_stream_t stream);

/* Replaces mAPMetric._parse_ground_truth (src/yolo/metrics.py:232-256).
 *   rec [N][S*S][5] f64 = {class_id, x, y, w, h}; counts [N]. */
int yolo_decode_gt(const float *tgt, int N, int S, int B, int C,
                   double *rec, int32_t *counts, yolo_stream_t stream);

#define YOLO_NMS_INFERENCE 0 /* inference.py:212-249,298-317: IoU has +1e-6, output in confidence order   */
#define YOLO_NMS_METRICS 1   /* metrics.py:258-341: union==0 -> 0, no eps, output grouped by class         */

/* Replaces YOLOInference.non_max_suppression (src/yolo/inference.py:298-317, variant 0) and
 * mAPMetric._apply_nms (src/yolo/metrics.py:270-296, variant 1), one 4-wave workgroup per image (ballot-built
 * suppression matrix, bit-mask greedy sweep).
 *   rec [N][max_per_img][6] f64 as written by yolo_decode; counts [N]
 *   keep [N][max_per_img] int32: indices into the image's records in the reference's OUTPUT order;
 *   keep_counts [N].
 * A later box survives a kept one iff class differs or IoU < thr (IoU == thr suppresses).
 * Limit: max_per_img <= 1024 (<= 128: suppression matrix by ballots in one pass; above, e.g. S = 14, B = 3 -> 588 boxes:
 * row-by-row sweep with a 1024-bit mask -- same comparisons, same result). */
int yolo_nms(const double *rec, const int32_t *counts, int N, int max_per_img, double thr, int variant,
             int32_t *keep, int32_t *keep_counts, yolo_stream_t stream);

/* Pairwise IoU matrix out[na][nb] between boxes a[na][4], b[nb][4] (x,y,w,h f64); the scalar
 * formulas of YOLOInference.iou (inference.py:229-249, variant 0) and mAPMetric._calculate_iou
 * (metrics.py:313-341, variant 1). */
int yolo_pairwise_iou(const double *a, int na, const double *b, int nb, int variant,
                      double *out, yolo_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Loss.  Replaces YOLOLoss.forward + compute_iou (src/yolo/loss.py:87-212) AND its autograd
 * backward in one pass: responsible-box selection by IoU, the five partial sums, dL/dpred
 * including the gradient that flows through the (non-detached) IoU target.
 *   pred,tgt [N][S][S][5B+C] fp32
 *   out      [8] fp32 : {total, coord, conf_obj, conf_noobj, class} each already / N, then
 *            out[5] = error flag (1.0 if some object cell selects a target slot >= B; the
 *            reference raises IndexError there), out[6..7] unused
 *   dpred    [N][S][S][5B+C] fp32 = d total / d pred, or NULL (forward only)
 *   work     [8*N] f64 caller workspace (per-image partial sums; deterministic reduction order)
 * Limits: B <= 8, S*S <= 1024. */
int yolo_loss_fwd_bwd(const float *pred, const float *tgt, int N, int S, int B, int C,
                      float lambda_coord, float lambda_noobj,
                      float *out, float *dpred, double *work, yolo_stream_t stream);

/* YOLOLoss.compute_iou (src/yolo/loss.py:174-212) for n box pairs, fp32. */
int yolo_loss_iou(const float *boxes1, const float *boxes2, long n, float *out, yolo_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Network layers.  bf16 storage, fp32 MFMA accumulation.  These replace the aten kernels behind
 * nn.Conv2d + nn.LeakyReLU(0.1), nn.MaxPool2d(2,2), nn.Linear as instantiated by
 * YOLOv1Backbone (src/yolo/models.py:47-84), the FC head (models.py:239-245) and DetectionHead
 * (models.py:313-332).
 * ------------------------------------------------------------------------------------------- */

/* One implicit-GEMM problem:  out[px][co] = epi( sum_{tap,c} in[row(px) + tapoff(tap) + c] * w[co][tap][c] )
 * It covers conv forward, conv data-gradient (weights packed transposed+flipped), and Linear
 * forward / data-gradient (a 1x1 conv on a 1x1 image).  All "elements" are bf16 elements. */
typedef struct yolo_igemm_desc {
    /* output pixel grid */
    int32_t N, Ho, Wo;
    /* input addressing: row(px=(n,oy,ox)) = n*in_img_stride + oy*in_row_stride*sy + ox*in_px_stride*sx ... */
    int64_t in_img_stride;  /* elements between images of the (padded) input                       */
    int32_t in_row_stride;  /* elements between input rows                                         */
    int32_t in_px_stride;   /* elements between input pixels (= channel count of the buffer)       */
    int32_t in_off;         /* element offset of (row 0, px 0, tap 0) inside an image              */
    int32_t stride;         /* conv stride (1 or 2)                                                */
    int32_t KH, KW;         /* taps                                                                */
    int32_t tap_len;        /* contiguous input elements per tap (= Cin; multiple of BK)           */
    int32_t Cout;           /* output channels (rows of w)                                         */
    /* output addressing (padded NHWC): out[(n*out_img_stride) + (oy*out_row_stride) + ox*out_px_stride + out_off + co] */
    int64_t out_img_stride;
    int32_t out_row_stride, out_px_stride, out_off;
    /* epilogue */
    int32_t epilogue;       /* YOLO_EPI_*                                                          */
    float slope;            /* LeakyReLU negative slope                                            */
    int32_t out_fp32;       /* 1: out is fp32, 0: bf16                                             */
    int32_t split_k;        /* >1: K split over blockIdx.y, fp32 atomicAdd into out (out_fp32=1,
                               epilogue NONE; caller zero-fills out and applies bias afterwards)   */
    /* aux addressing for YOLO_EPI_MUL_DLRELU (same form as the output addressing) */
    int64_t aux_img_stride;
    int32_t aux_row_stride, aux_px_stride, aux_off;
    int32_t pool2;          /* 1: fuse MaxPool2d(2,2) into the epilogue (conv -> LeakyReLU -> pool, models.py:49-55):
                               Ho/Wo stay the CONV output size, out_* address the pooled map [Ho/2][Wo/2];
                               2: as 1, and the UN-pooled activation is also written, to `aux` with the aux_* strides
                               (training keeps it for the backward pass);
                               3: as 1, and `aux` receives the ARG-MAX CODES instead: uint16 per (pooled pixel, 8 channels)
                               at index (pooled element address + channel) / 8 -- a buffer of the pooled map's geometry
                               with an eighth of its elements -- 2 bits per channel = window position 2*dy + dx of the
                               first maximum of the activations as stored.  With the pooled map that is all the backward
                               pass needs (yolo_maxpool2_bwd_codes): the un-pooled activation is never written       */
    int32_t w_blocked;      /* 1: w is in the panel layout of yolo_pack_fc_weight_blocked (Linear layers)      */
    int32_t tile_order;     /* 0 = heuristic; 1 = channel tiles fastest; 2 = pixel tiles fastest inside an XCD's range   */
    int32_t tile_hint;      /* 0 = let the library pick the tile configuration; 1: 128x128, 2: 256x128
                               (8 waves, 3 stages), 3: 128x64, 4: 64x128, 5/6: 1/2 on the 16x16x32
                               MFMA shape, 11: 256x128x64 and 12: 256x256x32 / 13: 256x128x32 with the staggered
                               two-phase schedule (8 waves), 14: 256 x 208 x 32 staggered with an uneven 7 / 6 column
                               split between the wave groups (see tile_px), 15: the same tile with the register-pipelined
                               one-barrier loop (even number >= 4 of 32-deep K steps per split; no pool2 / bn_stats /
                               atomics), 7-10: BK = 32 variants of 64x128, 19: streaming 1x1 convolution of the thin-K pointwise
                               layers (1x1, tap_len 64 / 128 / 192 / 256 / 512, Cout % 64 == 0, bf16 out, N*Ho*Wo % 16 == 0: the weight
                               panel sits in LDS, every wave walks 16-pixel groups with the next group's activation fragments and
                               the residual vectors in flight; igemm_stream.hip), 20 / 21: the persistent kernels (igemm_persist.hip: one software
                               pipeline over all tiles of a workgroup, tiles of 256 x 208 / 224 drawn from per-XCD queues, epilogue out of the
                               accumulator registers), 22: 3x3 / stride-1 conv of 64 -> 64 channels on maps of (16k) x (16k) pixels with the weight
                               panel resident in LDS and the input patch of a 16 x 16 tile staged once (conv_c64.hip; epilogue NONE / BIAS /
                               BIAS_LRELU, bf16 out, bn_stats allowed, no pool2 / split_k)  (tuning / tests;
                               a caller that wants the best plan times them per problem, as engine.igemm_call does) */
    int64_t px_begin, px_end; /* compute only output pixels [px_begin, px_end) of the flattened (n, oy, ox) index
                               (0, 0 = all).  Lets a caller run the bulk of a layer with a large tile in whole
                               rounds of the 256 CUs and the remainder with a small tile in one short round,
                               instead of a last round that keeps a few CUs busy for a full large-tile time */
    int32_t skew_phases;    /* > 1 (8-wave configurations, launches of more than 256 workgroups): the first-round
                               workgroups start (slot % skew_phases) * skew_step shader cycles late, so that the CUs
                               do not all reach their output stores at the same moment (0 = off)                  */
    int32_t skew_step;
    void *bn_stats;         /* != NULL (bf16 output, no split_k / pool2 / pixel range): YOLO_BN_ACC_REPLICAS * 2*Cout doubles into
                               which the launch adds, per output channel, the sum and the sum of squares of the values it
                               stored -- the statistics pass of a following yolo_batchnorm_train_fwd (stats_ready = 1) */
    int32_t tile_px;        /* > 0: a workgroup's tile covers only tile_px pixels of the flattened (n, oy, ox) index (at most the
                               configuration's pixel-tile edge; its remaining slots idle).  The layers of this network have
                               N * 49 * 4^k output pixels, which never divide into whole rounds of 256 CUs with 128- or 256-pixel
                               tiles; tile_hint 14 (256 channels x 208 pixel slots, uneven staggered split) with tile_px = 196
                               gives 64 * 4^k tiles per channel tile -- whole rounds at batch 64.  0 = all slots         */
    int32_t split_slabs;    /* split_k > 1 only.  1: split s STORES its partial tile into slab s of `out` = fp32
                               [split_k][N*Ho*Wo][Cout] (no zero fill, no atomics) and yolo_igemm_finish adds the slabs in
                               the fixed order 0, 1, .. -- bit-reproducible for any split count.  0: fp32 atomics into one
                               zero-filled [N*Ho*Wo][Cout] buffer                                                       */
} yolo_igemm_desc;

#define YOLO_EPI_NONE 0        /* out = acc                                                        */
#define YOLO_EPI_BIAS 1        /* out = acc + bias[co]                                             */
#define YOLO_EPI_BIAS_LRELU 2  /* out = lrelu(acc + bias[co])            (Conv2d/Linear + LeakyReLU) */
#define YOLO_EPI_MUL_DLRELU 3  /* out = acc * (aux[px][co] > 0 ? 1 : slope)  (dgrad through the
                                  previous layer's LeakyReLU; aux = that layer's output, bf16,
                                  addressed by the aux_* strides)                                                        */

#define YOLO_EPI_BIAS_ADD_LRELU 4 /* out = lrelu(acc + bias[co] + aux[px][co])  (residual add of a ResNet bottleneck,
                                    slope 0 = ReLU; aux = identity / downsample branch, bf16, aux_* strides)  */

int yolo_igemm(const yolo_igemm_desc *d, const void *in_bf16, const void *w_bf16 /*[Cout][KH*KW*tap_len]*/,
               const float *bias, const void *aux_bf16, void *out, yolo_stream_t stream);
/* Finishing pass of a split-K convolution.  Few-pixel, deep-K layers (the 7x7x1024 ones: 3136 pixels at batch 64,
 * K = 9216) have too few output tiles to fill 256 CUs; the caller runs yolo_igemm with split_k > 1, out_fp32 = 1,
 * YOLO_EPI_NONE into a zero-filled dense fp32 [N*Ho*Wo][Cout] buffer (or, with split_slabs = 1, into split_k slabs of
 * that shape) and then this pass, with the layer's REAL descriptor (epilogue, out_* / aux_* strides; split_k = the number
 * of slabs to add in fixed order when split_slabs = 1, else ignored), applies bias / LeakyReLU / LeakyReLU'(aux) and
 * writes bf16. */
int yolo_igemm_finish(const yolo_igemm_desc *d, const float *acc, const float *bias, const void *aux_bf16,
                      void *out_bf16, yolo_stream_t stream);

/* Weight-gradient of a conv / Linear, "flat" pixel indexing:
 *     dw[co][tap][ci] (+)= sum_{p < P} dy[p*dy_px_stride + co] * x[p*x_px_stride + tapoff(tap) + ci]
 *     tapoff(ky,kx) = (ky - pad)*x_row_stride + (kx - pad)*x_px_stride
 * p runs over EVERY pixel slot of the zero-haloed dy buffer (halo slots hold zeros and add nothing),
 * so dy and x must share one padded geometry (stride-1 convs; a stride-2 conv passes a zero-stuffed
 * dy of the input's geometry).  x needs a guard band of finite values (zeros) of at least
 * |tapoff| elements before and after the buffer.  dw is fp32 in the packed layout
 * [Cout][KH*KW][Cin]; with split > 1 or accumulate != 0 it is accumulated with fp32 atomics
 * (caller zero-fills / owns the previous value).  db[co] += sum_p dy[p][co] if db != NULL
 * (always accumulated: caller zero-fills).  dw == NULL: the bias gradient alone, flat indexing only
 * (with a pixel geometry: YOLO_E_UNSUPPORTED).  Replaces the weight / bias gradient of aten
 * convolution_backward and addmm backward. */
typedef struct yolo_wgrad_desc {
    int64_t P;                       /* dy pixel slots                                            */
    int32_t dy_px_stride, x_px_stride; /* elements between pixel slots (multiples of 8)           */
    int32_t Cout, Cin;
    int32_t KH, KW, pad;
    int64_t x_row_stride;            /* elements between input rows (multiple of 8)               */
    int32_t split;                   /* pixel-range split (uniform, 2-D grid).  0: the library's two-segment
                                        schedule -- whole rounds of the chip's workgroup slots plus a finer-split
                                        tail round; the caller zero-fills dw (tiles that are split over
                                        several workgroups are accumulated with atomics, the others stored) */
    int32_t accumulate;              /* 1: add into dw even when split == 1                       */
    int32_t variant;                 /* 0: choose; 1: 128x128 tile, 4 waves, 2 stages; 2: 256x128 tile, 8 waves, 3 stages;
                                        3: 2 + staggered two-phase schedule; 4: 128x128 tile, 8 waves; 5: 256x256 tile, wave
                                        tile 128x64, four 32-pixel stages, register-pipelined one-barrier loop
                                        (wgrad_pipe.hip; Cin in {8, 16, 32, 64, 128} with KH * KW > 1: 256 / Cin taps per tile, any other
                                        Cin one tap per tile; flat indexing with pad 0 needs P % 32 == 0, else YOLO_E_UNSUPPORTED: rows past
                                        the range re-read slot 0, which must be a zero halo slot of dy); 6: the tiles and schedule of
                                        5 with FOUR waves of 128x128, one per SIMD, 256 accumulator registers in AGPRs
                                        (wgrad_wide.hip)  (tests / tuning; all agree bit for bit with one pixel range per tile)  */
    /* Pixel geometry (geo_W == 0: "flat" indexing, p IS the slot).  Otherwise the reduction runs over the P = N*geo_H*geo_W
     * pixels p = (n*geo_H + oy)*geo_W + ox only, and pixel p lives in slot
     *     n*geo_img_slots + oy*geo_row_slots + ox*geo_px_slots + geo_slot0
     * of BOTH buffers (dy at slot*dy_px_stride, x at slot*x_px_stride + tap offset): the interior of a zero-haloed buffer
     * (geo_px_slots = 1) skips the halo slots -- 1.04x .. 1.65x fewer K steps -- and geo_px_slots = 2 with
     * geo_row_slots = 2 * row pitch visits only the non-zero slots of a stride-2 conv's zero-stuffed gradient (4x fewer). */
    int32_t geo_W, geo_H, geo_img_slots, geo_row_slots, geo_px_slots, geo_slot0;
    double *dw_sumsq;                /* optional (device double, NULL = off): += sum of squares of the dw this launch stores -- the
                                        global gradient norm of clip_grad_norm_ (trainer.py:79) then needs no pass over the 822 MB
                                        gradient of the Linear behind nn.Flatten.  Only with every tile stored by one workgroup
                                        (split = 1, accumulate = 0, variant 0 / 1, Cin % 4 == 0); otherwise YOLO_E_UNSUPPORTED */
    float *slabs;                    /* optional (variant 5 / 6, accumulate = 0, Cin % 4 == 0): scratch of slab_floats floats.  Every workgroup then
                                        STORES its 256 x 256 partial tile there and a second kernel adds the partials of a tile in pixel-range
                                        order into dw -- no fp32 atomics on dw (1.5 TB/s chip-wide, 60-90 k cycles per workgroup), dw need not
                                        be zero-filled, and dw is bit-reproducible.  yolo_wgrad_slab_floats gives the size a launch needs.
                                        Variants 0 / 1 / 4 (the 128 x 128 kernels; uniform split and split = 0, pair_taps, pixel geometry): only
                                        the workgroups of a tile that IS split over pixel ranges store a dense 128 x 128 partial; a tile owned by
                                        one workgroup keeps its direct store.  This replaces the atomicAdd epilogue of wgrad_kernel
                                        (4 and 8 waves).  With slabs in use, db is order-fixed too: the bias sums of the pixel ranges are stored
                                        ([co][range]: behind the tile partials for variants 0 / 1 / 4; in row co of dw, which is free until the
                                        slab sum runs, for 5 / 6 -- KH * KW * Cin must hold the ranges) and added in range order into db by a
                                        plain store, so db need not be zero-filled.  A launch of variant 0 / 1 / 4 without a split tile needs
                                        no slabs (yolo_wgrad_slab_floats gives 0) and runs as without them: db += one sum per channel.
                                        Variants 2 / 3 and accumulate != 0 are refused (YOLO_E_UNSUPPORTED) */
    int64_t slab_floats;
} yolo_wgrad_desc;

/* floats of yolo_wgrad_desc.slabs the launch described by d would use (0: variants 2 / 3; variants 0 / 1 / 4 when no tile is split);
 * host arithmetic only, launches nothing */
int yolo_wgrad_slab_floats(const yolo_wgrad_desc *d, long *floats);
int yolo_wgrad(const yolo_wgrad_desc *d, const void *x_bf16, const void *dy_bf16,
               float *dw_packed, float *db, yolo_stream_t stream);

/* MaxPool2d(2,2) on padded NHWC bf16 (models.py:51,55,65,72) and its backward fused with the
 * backward of the LeakyReLU that precedes the pool:
 *   dz[n][y][x][c] = (y,x is the arg-max of its 2x2 window, first in scan order on ties)
 *                    ? dpool[n][y/2][x/2][c] * (yfull > 0 ? 1 : slope) : 0 */
typedef struct yolo_pool_desc {
    int32_t N, H, W, C;       /* un-pooled logical size                                          */
    int32_t in_halo, out_halo;
} yolo_pool_desc;
/* MaxPool2d(3, stride 2, pad 1) forward (ResNet stem).  The input must be >= 0 (it follows a ReLU), so
 * the zero halo of the buffer is equivalent to the -inf padding of the operator.  H, W = input size. */
int yolo_maxpool3s2_fwd(const yolo_pool_desc *d, const void *x_bf16, void *y_bf16, yolo_stream_t stream);
/* its backward (aten max_pool2d_with_indices_backward): dx[n][h][w][c] = sum of dy over the windows whose arg-max
 * (first maximum in row-major order, recomputed from x) is (h, w).  d->out_halo = halo of dy, dx_halo = halo of dx. */
int yolo_maxpool3s2_bwd(const yolo_pool_desc *d, const void *x_bf16, const void *dy_bf16, void *dx_bf16, int dx_halo,
                        yolo_stream_t stream);
/* yolo_maxpool2_fwd and yolo_maxpool2_bwd_lrelu take an odd H or W with MaxPool2d's floor rule: the pooled map is [H/2][W/2], the last
 * row / column belongs to no window, and the backward does not write it (dz must hold zeros there: a fresh workspace buffer does). */
int yolo_maxpool2_fwd(const yolo_pool_desc *d, const void *x_bf16, void *y_bf16, yolo_stream_t stream);
int yolo_maxpool2_bwd_lrelu(const yolo_pool_desc *d, const void *yfull_bf16, const void *dpool_bf16,
                            float slope, void *dz_bf16, yolo_stream_t stream);
/* The same gradient from the POOLED activation (geometry of dpool) and the arg-max codes a fused conv + pool epilogue left
 * (yolo_igemm pool2 = 3, yolo_conv_stem7_fwd codes): codes[(pooled element address) / 8] = uint16, 2 bits per channel.  The
 * un-pooled activation is not read -- training never stores it (models.py:49-55: conv -> LeakyReLU -> MaxPool2d). */
int yolo_maxpool2_bwd_codes(const yolo_pool_desc *d, const void *ypool_bf16, const void *codes_u16, const void *dpool_bf16,
                            float slope, void *dz_bf16, yolo_stream_t stream);

/* ---- layout / precision conversion at the boundary to PyTorch-layout fp32 tensors ------------- */

/* NCHW fp32 -> padded NHWC bf16 with Cpad >= C channels (extra channels zero). */
int yolo_nchw_f32_to_nhwc_bf16(const float *x, int N, int C, int H, int W, void *y, int Cpad,
                               int halo_lo, int halo_hi, yolo_stream_t stream);
/* padded NHWC bf16 -> NCHW fp32 (module boundary, e.g. YOLOv1Backbone.forward's return value). */
int yolo_nhwc_bf16_to_nchw_f32(const void *x, int N, int C, int H, int W, int halo, float *y, yolo_stream_t stream);
/* padded NHWC bf16 -> NCHW bf16: nn.Flatten order (c*H*W + h*W + w) in front of the FC head
 * (src/yolo/models.py:240), so that Linear weights keep their state_dict column order. */
int yolo_nhwc_bf16_to_nchw_bf16(const void *x, int N, int C, int H, int W, int halo, void *y, yolo_stream_t stream);

/* OIHW fp32 -> packed bf16 [Cout][KH][KWp][Cinp] (forward operand) and, if wt != NULL,
 * [Cin][KH][KW][Cout] with taps flipped (data-gradient operand).  KWp/Cinp >= KW/Cin pad with zeros. */
int yolo_pack_conv_weight(const float *w_oihw, int Cout, int Cin, int KH, int KW, int Cinp, int KWp,
                          void *w_fwd_bf16, void *w_dgrad_bf16, yolo_stream_t stream);
/* Linear weight [O][K] fp32 -> bf16 [O][K'] with the K axis permuted from (c, hw) to (hw, c) order
 * (HW = 1: plain cast) and, if wt != NULL, the transposed copy [K'][O] for the data-gradient. */
int yolo_pack_fc_weight(const float *w, int O, int C, int HW, void *w_fwd_bf16, void *w_t_bf16, yolo_stream_t stream);
/* Linear weight [O][K] fp32 (K % 64 == 0) -> bf16 panels [ceil(O/128)][K/64][128][64], rows >= O zero.
 * With yolo_igemm_desc.w_blocked = 1 each LDS stage of the weight stream is one contiguous 16-KB read
 * (a Linear layer at batch 64 is HBM-bound on its 822 MB / 411 MB weight). */
int yolo_pack_fc_weight_blocked(const float *w, int O, long K, void *w_panels_bf16, yolo_stream_t stream);
/* The same panels with the K axis permuted from (c, hw) -- nn.Flatten of an NCHW map (models.py:239) -- to (hw, c): the Linear layer
 * then reads a dense NHWC conv output as it lies in memory and the flatten pass disappears (inference). */
int yolo_pack_fc_weight_blocked_hwc(const float *w, int O, int C, int HW, void *w_panels_bf16, yolo_stream_t stream);
/* packed fp32 gradient [Cout][KH][KWp][Cinp] -> OIHW fp32 (accumulate=0: overwrite, 1: add). */
int yolo_unpack_conv_wgrad(const float *dw_packed, int Cout, int Cin, int KH, int KW, int Cinp, int KWp,
                           float *dw_oihw, int accumulate, yolo_stream_t stream);
/* Forward of the 7x7 / stride-2 / pad-3 stem conv (models.py:49-51): x = NHWC4 bf16 with halo 3, w = the packed
 * [64][7][8][4] bf16 panel of yolo_pack_conv_weight(Cinp = 4, KWp = 8), out = NHWC bf16 with 64 channels
 * (out_off = element offset of output pixel (0,0), pixel stride 64).  y = lrelu(conv + bias, slope); pool2 = 1 also
 * applies MaxPool2d(2,2) and out_* then address the POOLED map.  The raw input patch of an 8 x 16 output tile is staged
 * once in LDS and the 4x overlap of neighbouring pixels' 7 x 8 windows is resolved by the MFMA operand read addresses
 * (the generic yolo_igemm gathers every window from L2: 448 B per output pixel).  Ho % 8 == 0, Wo % 16 == 0.
 * out_full (pool2 = 1 only, may be NULL): the un-pooled activation is written as well -- training needs it for the
 * backward of the pool and of the LeakyReLU -- so that the separate pooling pass disappears there too.
 * pool2 = 3: out_full receives the ARG-MAX CODES instead (uint16 per pooled pixel and 8 channels at (pooled element address) / 8,
 * 2 bits per channel, as yolo_igemm pool2 = 3; full_* unused): with the pooled map that is all the backward pass needs. */
int yolo_conv_stem7_fwd(const void *x_nhwc4_bf16, const void *w_packed_bf16, const float *bias, int N, int Ho, int Wo,
                        long x_img_stride, int x_row_stride, float slope, int pool2, void *out_bf16,
                        long out_img_stride, int out_row_stride, int out_off, void *out_full_bf16,
                        long full_img_stride, int full_row_stride, int full_off, yolo_stream_t stream);
/* The same from the caller's NCHW fp32 image batch [N][3][H][W] (H, W even; Ho = H/2, Wo = W/2): the input patch of a tile is
 * converted to NHWC4 bf16 on its way into LDS (same rounding as yolo_nchw_f32_to_nhwc_bf16), so the separate layout pass and its
 * 103 MB intermediate (batch 64) disappear.  Same results bit for bit. */
int yolo_conv_stem7_fwd_f32(const float *x_nchw_f32, const void *w_packed_bf16, const float *bias, int N, int H, int W, float slope,
                            int pool2, void *out_bf16, long out_img_stride, int out_row_stride, int out_off, void *out_full_bf16,
                            long full_img_stride, int full_row_stride, int full_off, yolo_stream_t stream);
/* Weight + bias gradient of the 7x7 / stride-2 / pad-3 stem conv (models.py:49; 3 input channels stored
 * NHWC4 with halo 3, Cout = 64) WITHOUT the unfolded copy: the unfolding happens in the LDS read addresses of
 * the MFMA operands.  dy: NHWC bf16 with 64 channels, dy_off = element offset of output pixel (0,0).
 * Ho % 8 == 0 and Wo % 16 == 0 required (otherwise: yolo_im2col_rows + yolo_wgrad).  Writes (does not
 * accumulate) dw in OIHW fp32 [64][3][7][7] and db[64] (NULL: skipped); deterministic: per-workgroup
 * partials in `scratch` (>= 14400 floats; 768 * 14400 for full speed) are summed in a fixed order. */
int yolo_wgrad_stem7(const void *x_nhwc4_bf16, const void *dy_bf16, int N, int Ho, int Wo, long x_img_stride,
                     int x_row_stride, long dy_img_stride, int dy_row_stride, int dy_off, float *dw_oihw,
                     float *db, float *scratch, long scratch_elems, yolo_stream_t stream);
/* The same with the backward of the MaxPool2d(2,2) + LeakyReLU that follow the stem fused in: y_full = the stem's
 * un-pooled activation (64 channels), dpool = gradient of the pooled map [Ho/2][Wo/2]; the gradient tile
 * (arg-max of every window gets dpool * LeakyReLU', the rest 0 -- what yolo_maxpool2_bwd_lrelu writes) is rebuilt in
 * registers per tile, so that 411 MB gradient buffer (batch 64) is neither written nor read.  Same results bit for bit. */
int yolo_wgrad_stem7_pooled(const void *x_nhwc4_bf16, const void *y_full_bf16, int N, int Ho, int Wo, long x_img_stride,
                            int x_row_stride, long y_img_stride, int y_row_stride, int y_off, const void *dpool_bf16,
                            long dp_img_stride, int dp_row_stride, int dp_off, float slope, float *dw_oihw, float *db,
                            float *scratch, long scratch_elems, yolo_stream_t stream);
/* ... and from what a stem forward with pool2 = 3 left instead of the un-pooled activation: y_pooled (geometry of dpool: the
 * dp_* strides address both) and the arg-max codes (uint16 at (pooled element address) / 8).  Reads 154 MB instead of 514 MB at
 * batch 64; same results bit for bit. */
int yolo_wgrad_stem7_codes(const void *x_nhwc4_bf16, const void *y_pooled_bf16, const void *codes_u16, int N, int Ho, int Wo,
                           long x_img_stride, int x_row_stride, const void *dpool_bf16, long dp_img_stride, int dp_row_stride,
                           int dp_off, float slope, float *dw_oihw, float *db, float *scratch, long scratch_elems,
                           yolo_stream_t stream);
/* Whole-model forms of the two calls above: every conv layer of the model in ONE launch (LDS-tiled,
 * all HBM accesses in runs of >= 128 B).  Layers need Cout % 64 == 0 (unpack: % 4), Cin % 64 == 0,
 * KH*KW <= 9 and no padding (Cinp = Cin, KWp = KW); either output of a pack item may be NULL. */
#define YOLO_PACK_MAX 32
typedef struct yolo_conv_pack_item {
    const float *w;            /* OIHW fp32 */
    void *w_fwd_bf16;          /* [Cout][KH][KW][Cin] */
    void *w_dgrad_bf16;        /* [Cin][KH][KW][Cout], taps flipped */
    int Cout, Cin, KH, KW;
} yolo_conv_pack_item;
typedef struct yolo_conv_unpack_item {
    const float *dw_packed;    /* [Cout][KH][KW][Cin] fp32 */
    float *dw_oihw;
    int Cout, Cin, KH, KW;
} yolo_conv_unpack_item;
int yolo_pack_conv_weights_multi(const yolo_conv_pack_item *items, int count, yolo_stream_t stream);
int yolo_unpack_conv_wgrads_multi(const yolo_conv_unpack_item *items, int count, yolo_stream_t stream);
/* Row-segment unfold for the 7x7/stride-2 first layer's WEIGHT GRADIENT only (Cin=3 gives no
 * channel-contiguous K axis): xcol[n][oy+h][ox+h][ky*seg + j] = x[n][oy*stride+ky][(ox*stride)*px + j],
 * written in the zero-haloed geometry of the layer's output so that yolo_wgrad's flat indexing
 * applies with one tap.  (models.py:49; the forward conv of that layer is im2col-free.) */
int yolo_im2col_rows(const void *x_bf16, long x_img_stride, int x_row_stride, int x_px_stride, int stride,
                     int KH, int seg, int N, int Ho, int Wo, int out_halo, void *xcol_bf16, yolo_stream_t stream);
/* fp32 [R][Ccols] -> bf16 transposed y[c*ld + r] (ld >= R; columns R..ld-1 are not written: the
 * caller zero-fills once).  Data-gradient operand of a Linear layer ([K][O] from [O][K]). */
int yolo_transpose_f32_to_bf16(const float *x, int R, int Ccols, void *y_bf16, int ld, yolo_stream_t stream);
/* bf16 [R][ldx] -> bf16 transposed y[c*ldy + r] (columns R..ldy-1 of y are not written). */
int yolo_transpose_bf16(const void *x_bf16, int R, int Ccols, int ldx, void *y_bf16, int ldy, yolo_stream_t stream);
/* Data-gradient of the Linear layer behind nn.Flatten (models.py:240-241), computed TRANSPOSED by
 * yolo_wgrad -- dxT[k][n] = sum_o W[o][k] * g[n][o] with the forward bf16 copy of W as the "dy" operand, so
 * that no [K][O] transposed copy of the 205 M-element weight is ever written -- and finished here:
 * k = c*H*W + h*W + w  ->  zero-haloed NHWC bf16 gradient, times LeakyReLU'(y_act) (y_act NULL: none). */
int yolo_fc_dgrad_to_nhwc(const float *dxT, int N, int C, int H, int W, int halo, const void *y_act_bf16,
                          float slope, void *g_bf16, yolo_stream_t stream);
int yolo_cast_f32_to_bf16(const float *x, long n, void *y_bf16, yolo_stream_t stream);
int yolo_cast_bf16_to_f32(const void *x_bf16, long n, float *y, yolo_stream_t stream);
/* y = lrelu(x + bias[col]) over [R][Ccols] fp32, bf16 and/or fp32 outputs (finishes a split-K Linear). */
int yolo_bias_lrelu_rows(const float *x, const float *bias, int R, int Ccols, float slope,
                         void *y_bf16, float *y_f32, yolo_stream_t stream);
/* the same finishing pass for a Linear layer whose split_k workgroups STORED their partial results as slabs
 * (yolo_igemm_desc.split_slabs): x = fp32 [slabs][R][Ccols], added in the fixed order 0, 1, .. -> bit-reproducible forward. */
int yolo_bias_lrelu_rows_slabs(const float *x, int slabs, const float *bias, int R, int Ccols, float slope,
                               void *y_bf16, float *y_f32, yolo_stream_t stream);

/* y[r][0..ld) = bf16( x[r][c] * (mask ? (mask[r][c] ? scale : 0) : 1) * (act ? (act[r][c] > 0 ? 1 : slope) : 1) ),
 * columns Cc..ld-1 zero.  x fp32 [R][Cc], mask u8 [R][Cc], act bf16 [R][Cc].  Backward of
 * Dropout(0.5) + LeakyReLU(0.1) of the FC head (models.py:242-243) and the fp32->bf16 hand-over of
 * dL/dpred (row padding to a multiple of 8 columns). */
int yolo_scale_rows_to_bf16(const float *x, const unsigned char *mask, float scale, const void *act_bf16, float slope,
                            int R, int Cc, int ld, void *y_bf16, yolo_stream_t stream);
/* nn.Dropout forward on bf16: y = mask ? x * scale : 0 (mask u8 drawn by the caller's RNG). */
int yolo_dropout_bf16(const void *x_bf16, const unsigned char *mask, float scale, long n, void *y_bf16, yolo_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Optimizer step (HBM-bound).  Replaces clip_grad_norm_(max_norm=10) + optim.Adam(lr, weight_decay)
 * of the reference's train step (src/yolo/training/trainer.py:79-95, src/train.py:177-179).
 * ------------------------------------------------------------------------------------------- */
/* *acc += sum(g[i]^2)  (device double, caller zero-fills once per step; one call per tensor). */
int yolo_sumsq_f32(const float *g, long n, double *acc, yolo_stream_t stream);
/* One tensor of torch.optim.Adam (amsgrad=False, L2 weight decay) in a single pass; `step` is the
 * 1-based step count.  If norm_sq != NULL the gradient is first scaled by
 * min(1, max_norm / (sqrt(*norm_sq) + 1e-6)) exactly as clip_grad_norm_ would have.  If p_bf16 != NULL
 * the updated parameter is also written as bf16 (same layout; 8-B aligned, p / g / exp_avg / exp_avg_sq 16-B aligned -- the same holds
 * for every tensor of the multi-tensor forms -- else YOLO_E_UNSUPPORTED). */
int yolo_adam_step(float *p, const float *g, float *exp_avg, float *exp_avg_sq, long n, float lr, float beta1,
                   float beta2, float eps, float weight_decay, long step, const double *norm_sq,
                   float max_norm, void *p_bf16, yolo_stream_t stream);
/* Multi-tensor forms: ONE launch for a whole parameter list (the reference's optimizer is torch's
 * multi-tensor `_foreach` Adam; 48 of this model's 52 tensors are too small to fill the chip alone).
 * Tables are host arrays; they are copied into the kernel arguments, YOLO_MT_MAX tensors per launch.
 * All tensors of one yolo_adam_step_multi call share `step` and the hyper-parameters.
 * skip_flag (device float, NULL: none): when *skip_flag != 0 the launch updates NOTHING -- the reference raises IndexError inside
 * YOLOLoss.forward for a target that selects a box slot >= B (src/yolo/loss.py:112-118), i.e. before any parameter update; here the
 * loss kernel's error word (out[5] of yolo_loss_fwd_bwd) is read by the host only after the step was enqueued, so the update
 * kernels test it on the device. */
#define YOLO_MT_MAX 48
typedef struct yolo_adam_tensor {
    float *p;            /* parameter, updated in place */
    const float *g;      /* gradient */
    float *m, *v;        /* exp_avg, exp_avg_sq */
    void *p_bf16;        /* optional bf16 shadow of p in the same layout (NULL: none) */
    long n;              /* elements */
} yolo_adam_tensor;
/* *acc += the sum of squares of every g[i] (n[i] elements; empty tensors are legal): one launch per YOLO_MT_MAX tensors.
 * YOLO_E_ARG: a null pointer, count < 0, n[i] < 0.  YOLO_E_UNSUPPORTED: a g[i] not 16-B aligned.  Every tensor is checked before the first
 * launch.  Either way nothing is launched. */
int yolo_sumsq_f32_multi(const float *const *g, const long *n, int count, double *acc, yolo_stream_t stream);
/* Order-fixed forms of yolo_sumsq_f32 / yolo_sumsq_f32_multi (norm_fixed.hip; EngineConfig.DETERMINISTIC).  They replace the one fp64
 * atomicAdd per workgroup in which sumsq_kernel / sumsq_multi_kernel end: a workgroup owns one 65536-element slice of one tensor (the
 * table layout of yolo_sumsq_f32_multi) and STORES its fp64 partial in scratch slot = its index; a last one-workgroup stage adds the slots
 * in a fixed order onto *acc (caller zero-fills, as before).  The double is then a function of the gradients and the tensor list alone,
 * and with it the clip coefficient of every parameter.  scratch: scratch_slots >= yolo_sumsq_fixed_slots doubles, 8-B aligned, not shared
 * with a launch in flight on another stream.  Everything is checked before the first launch. */
int yolo_sumsq_fixed_slots(const long *n, int count, long *slots);
int yolo_sumsq_f32_fixed(const float *g, long n, double *scratch, long scratch_slots, double *acc, yolo_stream_t stream);
int yolo_sumsq_f32_multi_fixed(const float *const *g, const long *n, int count, double *scratch, long scratch_slots, double *acc,
                               yolo_stream_t stream);
/* yolo_adam_step for a whole parameter list: one launch per YOLO_MT_MAX tensors; empty tensors are legal.
 * YOLO_E_ARG: a null pointer, count < 0, step < 1, n < 0.  YOLO_E_UNSUPPORTED: p / g / m / v not 16-B aligned, p_bf16 not 8-B aligned.
 * Every tensor is checked before the first launch.  Either way nothing is launched. */
int yolo_adam_step_multi(const yolo_adam_tensor *t, int count, float lr, float beta1, float beta2, float eps,
                         float weight_decay, long step, const double *norm_sq, float max_norm, const float *skip_flag,
                         yolo_stream_t stream);
/* The same update as a BACKGROUND pass: `workgroups` (1 .. 256) persistent workgroups of 1024 threads, each holding one CU to itself
 * (they reserve LDS they do not use), walk the elements.  An HBM-bound pass that occupies exactly that many CUs: launched on a
 * second stream it runs beside MFMA-bound kernels on the other CUs -- e.g. the update of the Linear layers (76 % of this model's
 * optimizer bytes, first used at the END of the next forward) beside the next forward's conv stack.  At most YOLO_MT_MAX tensors. */
int yolo_adam_step_multi_bg(const yolo_adam_tensor *t, int count, float lr, float beta1, float beta2, float eps,
                            float weight_decay, long step, const double *norm_sq, float max_norm, const float *skip_flag,
                            int workgroups, yolo_stream_t stream);

/* torch.optim.SGD (maximize=False) with the same folded clip_grad_norm_, skip flag and bf16 shadow as the Adam entries -- the YOLOv1
 * paper's recipe (momentum 0.9, weight decay 5e-4) in the optimizer slot of the reference's train step
 * (src/yolo/training/trainer.py:79-95).  Per element, in fp32, every a * b + c one fused multiply-add (all three forms: the same bits):
 *     g = grad * clip                   clip = min(1, max_norm / (sqrt(*norm_sq) + 1e-6)), 1 when norm_sq == NULL
 *     g = g + weight_decay * p          (weight_decay != 0)
 *     buf = first_step ? g : momentum * buf + (1 - dampening) * g ;  g = nesterov ? g + momentum * buf : buf      (momentum != 0)
 *     p = p - lr * g ;  p_bf16 = bf16(p)
 * first_step != 0: the momentum buffers are only written (torch creates them as a copy of the gradient).  momentum == 0: buf is not
 * touched and may be NULL.  *skip_flag != 0 updates nothing: not p, not buf, not the shadow.
 * YOLO_E_ARG: a null pointer, a negative size / lr / momentum / weight_decay, nesterov with momentum <= 0 or dampening != 0 (the
 * ValueErrors of torch.optim.SGD), workgroups outside 1 .. 256, more than YOLO_MT_MAX tensors in the background form.
 * YOLO_E_UNSUPPORTED: p / g / buf not 16-B aligned, p_bf16 not 8-B aligned.  Either way nothing is launched. */
typedef struct yolo_sgd_tensor {
    float *p;            /* parameter, updated in place */
    const float *g;      /* gradient */
    float *buf;          /* momentum_buffer */
    void *p_bf16;        /* optional bf16 shadow of p in the same layout (NULL: none) */
    long n;              /* elements */
} yolo_sgd_tensor;
/* One tensor (trainer.py:79-95, the optimizer.step() of one parameter). */
int yolo_sgd_step(float *p, const float *g, float *buf, long n, float lr, float momentum, float dampening, float weight_decay,
                  int nesterov, int first_step, const double *norm_sq, float max_norm, void *p_bf16, const float *skip_flag,
                  yolo_stream_t stream);
/* A whole parameter list (trainer.py:79-95, optimizer.step() as torch's multi-tensor `_foreach` SGD does it): one launch per
 * YOLO_MT_MAX tensors, the host table copied into the kernel arguments; empty tensors are legal.  All tensors share first_step and
 * the hyper-parameters. */
int yolo_sgd_step_multi(const yolo_sgd_tensor *t, int count, float lr, float momentum, float dampening, float weight_decay,
                        int nesterov, int first_step, const double *norm_sq, float max_norm, const float *skip_flag,
                        yolo_stream_t stream);
/* The same update (trainer.py:79-95) as a BACKGROUND pass for a second stream, like yolo_adam_step_multi_bg: `workgroups` (1 .. 256)
 * persistent workgroups of 1024 threads, each holding one CU to itself.  At most YOLO_MT_MAX tensors. */
int yolo_sgd_step_multi_bg(const yolo_sgd_tensor *t, int count, float lr, float momentum, float dampening, float weight_decay,
                           int nesterov, int first_step, const double *norm_sq, float max_norm, const float *skip_flag,
                           int workgroups, yolo_stream_t stream);

/* LARS (You, Gitman, Ginsburg 2017: layer-wise adaptive rate scaling) in the optimizer slot of the reference's train step
 * (src/yolo/training/trainer.py:79-95), for the large effective batches of accumulation x ranks; the reference has no such optimizer, the
 * entries stand beside its clip_grad_norm_ + optimizer.step().  Two passes (lars.hip).
 *
 * Per-tensor sums of squares, order-fixed, no atomics (the structure of yolo_sumsq_f32_multi_fixed): a workgroup owns one 65536-element
 * slice of one tensor and stores sum p^2 and sum g^2 of it in scratch slots 2k, 2k + 1 (k = its index); one workgroup per tensor adds the
 * tensor's slots in a fixed order and STORES norms[2i] = sum p[i]^2, norms[2i+1] = sum g[i]^2 (doubles; not accumulated, empty tensors
 * give 0, 0); lists longer than YOLO_MT_MAX take several launches, each reusing the scratch from slot 0.  g_total (NULL: none):
 * *g_total = norms[1] + norms[3] + .. in rising order, the global squared gradient norm for the folded clip (trainer.py:79-95), stored.
 * Two calls on the same inputs give the same bits, so EngineConfig.DETERMINISTIC needs no second path.  scratch: scratch_slots >=
 * yolo_lars_norm_slots doubles, 8-B aligned, not shared with a launch in flight on another stream; norms: 2 * count doubles.
 * YOLO_E_ARG: a null pointer, count < 0, n[i] < 0, scratch too small.  YOLO_E_UNSUPPORTED: a p[i] or g[i] not 16-B aligned, norms or
 * g_total not 8-B aligned.  Every tensor is checked before the first launch: a refused call launches nothing. */
int yolo_lars_norm_slots(const long *n, int count, long *slots);
int yolo_lars_norms_multi(const float *const *p, const float *const *g, const long *n, int count, double *scratch, long scratch_slots,
                          double *norms, double *g_total, yolo_stream_t stream);
/* The step, with the folded clip_grad_norm_, skip flag and bf16 shadow of the SGD entries (trainer.py:79-95).  Per tensor, in fp64, from
 * the two doubles of yolo_lars_norms_multi:
 *     wn = sqrt(norms[0]) ;  gn = (double)clip * sqrt(norms[1])          clip = min(1, max_norm / (sqrt(*norm_sq) + 1e-6)) in fp32, 1 when NULL
 *     trust = (adapt && wn > 0 && gn > 0) ? (float)((double)eta * wn / (gn + (double)weight_decay * wn + (double)eps)) : 1
 * Per element, in fp32, every a * b + c one fused multiply-add (all three forms: the same bits):
 *     g = grad * clip ;  g = g + weight_decay * p (weight_decay != 0) ;  g = g * trust
 *     buf = first_step ? g : momentum * buf + g  (momentum != 0; else buf is not touched, may be NULL, and g is used) ;  p = p - lr * buf
 *     p_bf16 = bf16(p)
 * -- the regularised gradient scaled by the trust ratio, then torch.optim.SGD(weight_decay=0); no dampening, no Nesterov.  adapt == 0: the
 * plain clipped SGD step, bit for bit.  *skip_flag != 0 updates nothing.
 * YOLO_E_ARG: a null pointer, a negative size / lr / momentum / weight_decay / eta / eps, adapt != 0 with norms == NULL, workgroups outside
 * 1 .. 256, more than YOLO_MT_MAX tensors in the background form.  YOLO_E_UNSUPPORTED: p / g / buf not 16-B aligned, p_bf16 or norms not
 * 8-B aligned.  Either way nothing is launched. */
typedef struct yolo_lars_tensor {
    float *p;            /* parameter, updated in place */
    const float *g;      /* gradient */
    float *buf;          /* momentum_buffer */
    void *p_bf16;        /* optional bf16 shadow of p in the same layout (NULL: none) */
    const double *norms; /* the 2 doubles of this tensor: sum p^2, sum g^2 (NULL when adapt == 0) */
    long n;              /* elements */
    int adapt;           /* 0: trust ratio 1 (biases, BatchNorm gamma / beta) */
} yolo_lars_tensor;
/* One tensor (trainer.py:79-95, the optimizer.step() of one parameter). */
int yolo_lars_step(float *p, const float *g, float *buf, long n, const double *norms, int adapt, float lr, float momentum, float weight_decay,
                   float eta, float eps, int first_step, const double *norm_sq, float max_norm, void *p_bf16, const float *skip_flag,
                   yolo_stream_t stream);
/* A whole parameter list (trainer.py:79-95): one launch per YOLO_MT_MAX tensors, the host table copied into the kernel arguments; empty
 * tensors are legal.  All tensors share first_step and the hyper-parameters; adapt is per tensor. */
int yolo_lars_step_multi(const yolo_lars_tensor *t, int count, float lr, float momentum, float weight_decay, float eta, float eps,
                         int first_step, const double *norm_sq, float max_norm, const float *skip_flag, yolo_stream_t stream);
/* The same update (trainer.py:79-95) as a BACKGROUND pass for a second stream, like yolo_sgd_step_multi_bg: `workgroups` (1 .. 256)
 * persistent workgroups of 1024 threads, each holding one CU to itself.  At most YOLO_MT_MAX tensors. */
int yolo_lars_step_multi_bg(const yolo_lars_tensor *t, int count, float lr, float momentum, float weight_decay, float eta, float eps,
                            int first_step, const double *norm_sq, float max_norm, const float *skip_flag, int workgroups,
                            yolo_stream_t stream);

/* Exponential moving average of the weights, the copy a detector validates and ships: replaces
 * torch.optim.swa_utils.get_ema_multi_avg_fn / torch._foreach_lerp_(ema, params, 1 - decay) (the reference keeps no EMA; its
 * train step is src/yolo/training/trainer.py:79-95, and the average follows optimizer.step()).  Per element, in fp32:
 *     e = fmaf(w, p - e, e)             w = (float)(1.0 - decay), formed by the host in double
 * -- one rounding for the difference, one for the fused multiply-add (torch.lerp's form for weights below 0.5); all three forms
 * compute the same bits.  p is only read.  *skip_flag != 0 (device float, NULL: none) updates nothing: a step the optimizer
 * skipped is no EMA step.
 * YOLO_E_ARG: a null pointer, n < 0, w outside [0, 1] or NaN, workgroups outside 1 .. 256, more than YOLO_MT_MAX tensors in the
 * background form.  YOLO_E_UNSUPPORTED: ema or p not 16-B aligned, ema overlapping p.  Either way nothing is launched. */
typedef struct yolo_ema_tensor {
    float *ema;          /* average, updated in place */
    const float *p;      /* parameter or buffer of the trained model */
    long n;              /* elements */
} yolo_ema_tensor;
/* One tensor. */
int yolo_ema_update(float *ema, const float *p, long n, float w, const float *skip_flag, yolo_stream_t stream);
/* A whole list (torch._foreach_lerp_): one launch per YOLO_MT_MAX tensors, the host table copied into the kernel arguments; empty
 * tensors are legal. */
int yolo_ema_update_multi(const yolo_ema_tensor *t, int count, float w, const float *skip_flag, yolo_stream_t stream);
/* The same update as a BACKGROUND pass for a second stream, like yolo_sgd_step_multi_bg: `workgroups` (1 .. 256) persistent
 * workgroups of 1024 threads, each holding one CU to itself.  At most YOLO_MT_MAX tensors. */
int yolo_ema_update_multi_bg(const yolo_ema_tensor *t, int count, float w, const float *skip_flag, int workgroups,
                             yolo_stream_t stream);

/* Gradient accumulation, K micro-batches per optimizer step: replaces what autograd's AccumulateGrad does when backward() runs again
 * without zero_grad (one stock add per tensor, no 1/K), and torch._foreach_mul_ / torch._foreach_add_(acc, grads, alpha=1/K) (the
 * reference has no accumulation: src/yolo/training/trainer.py:64 clears the gradients in front of every backward).  Per element, in fp32:
 *     dst = fmaf(alpha, x, y)           y != NULL;      alpha = (float)(1.0 / K), formed by the host in double
 *     dst = alpha * x                   y == NULL
 * -- one rounding either way (the product inside the fma is exact); both forms compute the same bits.  x and y are only read, unless dst IS
 * one of them: dst == x or dst == y exactly is the in-place use (acc = fmaf(alpha, g, acc); the fold g = fmaf(alpha, g, acc)), every element
 * read before it is written by the same lane.  *skip_flag != 0 (device float, NULL: none) writes nothing.
 * YOLO_E_ARG: null dst or x, n < 0, count < 0, alpha not finite.  YOLO_E_UNSUPPORTED: a pointer not 16-B aligned, dst overlapping x or y
 * without being it.  Every tensor is checked before the first launch: a refused call launches nothing. */
typedef struct yolo_accum_tensor {
    float *dst;          /* written; may be x or y */
    const float *x;      /* the micro-batch's gradient */
    const float *y;      /* the accumulator so far, or NULL */
    long n;              /* elements */
} yolo_accum_tensor;
/* One tensor. */
int yolo_grad_accum(float *dst, const float *x, const float *y, long n, float alpha, const float *skip_flag, yolo_stream_t stream);
/* A whole list: one launch per YOLO_MT_MAX tensors, the host table copied into the kernel arguments; empty tensors are legal. */
int yolo_grad_accum_multi(const yolo_accum_tensor *t, int count, float alpha, const float *skip_flag, yolo_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Factored gradient of a Linear layer (fc_factored.hip / fc_factored.h).  The weight gradient of nn.Linear is the product of two thin
 * batch factors, G = scale * dy^T x (addmm backward, the FC head of src/yolo/models.py:239-245); for the Linear(50176, 4096) behind
 * nn.Flatten the factors are 6.9 MB at batch 64 and G is 822 MB.  These entries take the FACTORS in the optimizer slot of the reference's
 * train step (src/yolo/training/trainer.py:79-95): the norm for clip_grad_norm_ comes from two rows x rows Gram matrices, and the step
 * kernels rebuild G tile by tile on the matrix cores (v_mfma_f32_32x32x16_bf16, `rows` on the K axis, zero-padded in LDS to the K step of
 * 16) and apply the element op of yolo_adam_step_multi / yolo_sgd_step_multi to p / m / v straight out of the accumulator registers.  G
 * never touches memory.  One device function forms the tile product for the gradient entry and both step entries, one multiply applies
 * `scale`: G is the same bits in all three, for any `workgroups`.  No atomics anywhere: every entry is a function of its inputs alone.
 * A workgroup owns tiles of 64 x 64 weights; the input-feature index lies on the MFMA column (lane & 31), so that one accumulator
 * register is two 128-B row segments of p / m / v.  O and I need not be multiples of the tile, rows need not be a multiple of 16.
 * Every entry: YOLO_E_ARG for a null pointer, rows / O / I < 1, ld_dy < O, ld_x < I, a negative `workgroups`, scratch too small;
 * YOLO_E_UNSUPPORTED for I % 8 != 0, ld_dy or ld_x not a multiple of 8, dy / x / p / m / v / buf / g_out not 16-B aligned, p_bf16 or the
 * doubles not 8-B aligned, rows > YOLO_FC_MAX_ROWS (the two K panels of a tile, 128 x (rows + 8) bf16, must fit the 160 KB of LDS).
 * Everything is checked before the first launch: a refused call launches nothing. */
#define YOLO_FC_MAX_ROWS 512
/* Longest fp32 accumulation chain of one Gram entry in yolo_fc_factored_sumsq: the Gram matrices are formed in chunks of this many
 * columns on the matrix cores, the chunk partials are added in fp64. */
#define YOLO_FC_GRAM_CHAIN 256
typedef struct yolo_fc_factors {
    const void *dy;   /* bf16 [rows][ld_dy], columns 0..O-1 used  */
    const void *x;    /* bf16 [rows][ld_x],  columns 0..I-1 used  */
    int32_t rows;     /* factor rows = images (x ranks); any value >= 1, need not be a multiple of the MFMA K step */
    int32_t O, I;     /* the weight is fp32 [O][I], row-major (the master's layout) */
    int32_t ld_dy, ld_x;   /* multiples of 8 */
    float scale;      /* G = scale * dy^T x   (1 / world size under data parallelism) */
} yolo_fc_factors;
/* g_out [O][I] fp32 = G: the gradient on request (what autograd's addmm backward would have stored, times scale). */
int yolo_fc_factored_grad(const yolo_fc_factors *f, float *g_out, yolo_stream_t stream);
/* *acc += |G|^2 without forming G: |G|^2 = scale^2 * sum_{n,m} (dy_n . dy_m)(x_n . x_m).  Three order-fixed stages, as norm_fixed.hip: one
 * wave per (factor, 32 x 32 Gram tile, column range) adds its chunks' fp32 MFMA partials in fp64 and stores the tile; the tiles' ranges
 * are added in rising order per entry, the two Gram entries multiplied and summed per workgroup into a slot; one workgroup adds the slots
 * in a fixed order, multiplies by scale^2 (double) and adds onto *acc.  scratch: scratch_doubles >= yolo_fc_factored_sumsq_slots doubles,
 * 8-B aligned, not shared with a launch in flight on another stream. */
int yolo_fc_factored_sumsq_slots(const yolo_fc_factors *f, long *doubles);
int yolo_fc_factored_sumsq(const yolo_fc_factors *f, double *scratch, long scratch_doubles, double *acc, yolo_stream_t stream);
/* yolo_adam_step_multi / yolo_sgd_step_multi for ONE [O][I] parameter whose gradient is given by its factors (same scalars, same folded
 * clip, skip flag and bf16 shadow; first_step etc. as there).  workgroups > 0: a persistent grid of that many workgroups walks the tiles
 * (the background form for a second stream); 0: the whole chip.  The result does not depend on `workgroups`. */
int yolo_adam_step_factored(const yolo_fc_factors *f, float *p, float *exp_avg, float *exp_avg_sq, void *p_bf16, float lr, float beta1,
                            float beta2, float eps, float weight_decay, long step, const double *norm_sq, float max_norm,
                            const float *skip_flag, int workgroups, yolo_stream_t stream);
int yolo_sgd_step_factored(const yolo_fc_factors *f, float *p, float *buf, void *p_bf16, float lr, float momentum, float dampening,
                           float weight_decay, int nesterov, int first_step, const double *norm_sq, float max_norm,
                           const float *skip_flag, int workgroups, yolo_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Classification pretraining of the YOLOv1 trunk (the paper's first stage: 20 convolutions, an average pool and one Linear layer
 * at 224 x 224).  These three entries EXTEND the reference surface -- mattiaskvist/yolo-v1 has no classifier stage, it downloads
 * torchvision's ImageNet weights -- so each names the stock-torch operation it replaces instead of a reference line.
 * Nothing here uses atomics: two calls on the same inputs give the same bits (EngineConfig.DETERMINISTIC needs no second path).
 * ------------------------------------------------------------------------------------------- */

/* Replaces torch.nn.functional.adaptive_avg_pool2d(x, 1) / x.mean((2, 3)) on the NCHW fp32 features a conv-terminated plan returns.
 *   x [N][C][HW] fp32 -> y [N][C] fp32, y[n][c] = (sum of the row) * (float)(1.0 / HW)
 * The sum is formed in fp32 in one fixed order that depends on HW only: a group of L lanes owns a row (L = the smallest power of two
 * with 4 L >= HW, at most 64; several rows per wave when HW is small), a lane adds its elements j, j + L, .. in that order, the
 * group folds its L partial sums with an xor butterfly.  Rows need no alignment (HW = 49).
 * YOLO_E_ARG: a null pointer, N < 0, C < 1, HW < 1.  N = 0 launches nothing. */
int yolo_gap_fwd(const float *x, int N, int C, int HW, float *y, yolo_stream_t stream);
/* Its backward (autograd's mean_backward: expand + div): dx[n][c][i] = dy[n][c] * (float)(1.0 / HW), one fp32 multiply per element.
 * 16-B stores when dx is 16-B aligned, 4-B stores otherwise.  Errors as yolo_gap_fwd. */
int yolo_gap_bwd(const float *dy, int N, int C, int HW, float *dx, yolo_stream_t stream);

/* Replaces torch.nn.functional.cross_entropy(logits, labels, label_smoothing = e, reduction = "mean"), its autograd backward and
 * torch.topk(logits, 5) + the membership test of a top-1 / top-5 accuracy, in one pass: one workgroup per row, strided (any K >= 1).
 *   logits  [N][K] fp32, labels [N] int64
 *   per row: m = max, s = sum exp(x - m) (fp32 exp, fp64 sum), lse = m + log s;
 *            loss = (1 - e) (lse - x[label]) + e (lse - mean x)                      (fp64)
 *   out     [2] fp32: out[0] = the mean of the row losses, added in row order in fp64 by a one-workgroup last stage;
 *           out[1] = error flag, 1.0 if some label lies outside [0, K).  Such a row contributes zero loss, a zero gradient row and
 *           no hits, and nothing is read or written out of bounds for it (torch raises / asserts on the device there); the flag is a
 *           device float an optimizer's skip_flag can take, like out[5] of yolo_loss_fwd_bwd
 *   dlogits [N][K] fp32 = (softmax - ((1 - e) onehot + e / K)) / N, or NULL (forward only: the same out and hits)
 *   hits    [N][2] int32: hits[n][0] = top-1, hits[n][1] = top-5.  A hit at k: fewer than k logits of the row are STRICTLY greater than
 *           the label's -- independent of any sort, and a tie with the label's logit never costs the hit
 *   work    [N] f64 caller workspace: the row losses
 * YOLO_E_ARG: a null pointer (dlogits excepted), N < 0, K < 1, label_smoothing outside [0, 1) or NaN.  N = 0: out[0] = NaN, as torch. */
int yolo_softmax_xent_fwd_bwd(const float *logits, const int64_t *labels, int N, int K, float label_smoothing, float *out,
                              float *dlogits, int32_t *hits, double *work, yolo_stream_t stream);

/* g *= min(1, max_norm / (sqrt(*norm_sq) + 1e-6))  (stand-alone clip_grad_norm_ for other optimizers). */
int yolo_clip_scale_f32(float *g, long n, const double *norm_sq, float max_norm, yolo_stream_t stream);

/* BatchNorm2d forward in TRAINING mode (batch statistics) + optional residual add + optional ReLU, in place on a
 * zero-haloed NHWC bf16 conv output z [N][H+2h][W+2h][C] (C % 8 == 0).  The reference's default model trains with a
 * frozen ResNet-50 backbone whose BatchNorm layers still run in training mode (trainer.py:49): they normalise with
 * the batch mean / biased variance and update running_mean / running_var (unbiased) with `momentum`, as aten
 * batch_norm(training=True) does.  acc2c: YOLO_BN_ACC_REPLICAS * 2*C doubles, zero on entry and on return (scratch shared
 * by all layers; the workgroups' partial sums are spread over the replicas because same-address fp64 atomics serialise);
 * scale_shift: 2*C floats of scratch; residual: NHWC bf16 of the same H, W, C (NULL: none).  Forward only. */
#define YOLO_BN_ACC_REPLICAS 16
int yolo_batchnorm_train_fwd(void *z_bf16, int N, int H, int W, int C, int halo, const float *gamma, const float *beta,
                             double eps, double momentum, float *running_mean, float *running_var,
                             const void *residual_bf16, int residual_halo, int relu, double *acc2c,
                             float *scale_shift, void *out_bf16, int out_halo, float *save_mean_invstd,
                             int stats_ready, yolo_stream_t stream);
/* (stats_ready = 1: acc2c already holds the sums -- the producing yolo_igemm accumulated them (yolo_igemm_desc.bn_stats) --
 *  and the statistics pass over z is skipped; stats_ready = 2: z is normalised with running_mean / running_var as they are
 *  (aten batch_norm(training=False): eval() mode of the reference's trunk, src/yolo/models.py:131-176, when gradients flow
 *  through it); nothing is accumulated or updated, save_mean_invstd receives the running mean and 1/sqrt(running_var + eps);
 *  out_bf16 != NULL: the result goes to that buffer [N][H+2*out_halo][W+2*out_halo][C] and z is kept -- a trainable
 *  trunk needs z for the backward pass; save_mean_invstd != NULL: 4*C floats -- batch mean, 1/sqrt(var + eps), and the
 *  scale / shift the forward applied, y = fma(z, scale, shift).)
 *
 * BatchNorm2d backward (training mode) for a conv -> BN [-> + residual] [-> ReLU] unit of a TRAINABLE ResNet trunk
 * (the reference's default run: ResNetBackbone(pretrained=True, freeze=False), src/train.py:144; aten
 * native_batch_norm_backward + threshold_backward).  dy: gradient wrt the unit's output; y: that output (ReLU mask,
 * NULL when the unit has no ReLU, or with relu_from_z = 1: the unit is conv -> BN -> ReLU without a residual and the mask is
 * recomputed as fma(z, scale, shift) > 0, the forward's own expression, which saves reading y twice);
 * z: the conv output the forward normalised; mean_invstd: the 4*C floats saved by the forward.
 *   dy' = dy * [y > 0];  dbeta = sum dy';  dgamma = sum dy' * xhat;  dz = gamma * invstd * (dy' - dbeta/M - xhat * dgamma/M)
 * dz is written at dz[n*dz_img_stride + y*dz_row_stride + x*dz_px_stride + dz_off + c] (doubled strides put it
 * zero-stuffed on the input grid of a stride-2 conv, the form yolo_wgrad / the data gradient read); store_masked_dy: dy'
 * replaces dy in place (the identity branch of a bottleneck receives it).  relu_from_z bit 1 (value 2 or 3): the forward ran
 * with stats_ready = 2 (running statistics): dgamma / dbeta as above with the saved mean / invstd, dz = gamma * invstd * dy'.  acc2c: as above (YOLO_BN_ACC_REPLICAS * 2*C
 * doubles, zero on entry and on return); coef3c: 3*C floats of scratch. */
int yolo_batchnorm_bwd(void *dy_bf16, int dy_halo, const void *y_bf16, int y_halo, const void *z_bf16, int z_halo,
                       int N, int H, int W, int C, const float *gamma, const float *mean_invstd, void *dz_bf16,
                       long dz_img_stride, long dz_row_stride, long dz_px_stride, long dz_off, int store_masked_dy,
                       int relu_from_z, float *dgamma, float *dbeta, double *acc2c, float *coef3c, yolo_stream_t stream);

/* conv -> BatchNorm2d -> LeakyReLU(slope) [-> MaxPool2d(2,2)] units of the BatchNorm variant of the YOLOv1 network (Darknet's
 * yolov1.cfg: batch_normalize=1 on every convolution).  Replaces aten batch_norm(training=True / False) + leaky_relu
 * [+ max_pool2d(2, 2)] and, backward, max_pool2d_with_indices_backward + leaky_relu_backward + native_batch_norm_backward.
 * Statistics, finalisation, running statistics, stats_ready 0 / 1 / 2 and save_mean_invstd exactly as yolo_batchnorm_train_fwd.
 *   y = t > 0 ? t : slope * t,  t = fma(z, scale, shift),  one bf16 rounding.
 * z is never written (always kept), `out` is required.  pool2 = 1: `out` is the pooled map [N][H/2 + 2*out_halo][W/2 + 2*out_halo][C],
 * the maximum over the bf16-ROUNDED y of each 2x2 window (what yolo_maxpool2_fwd over a stored y gives, bit for bit); the un-pooled y
 * is never written.  H and W must be even then (YOLO_E_UNSUPPORTED otherwise: run pool2 = 0 and yolo_maxpool2_fwd). */
int yolo_batchnorm_train_fwd_lrelu(const void *z_bf16, int N, int H, int W, int C, int halo, const float *gamma,
                                   const float *beta, double eps, double momentum, float *running_mean,
                                   float *running_var, float slope, int pool2, double *acc2c, float *scale_shift,
                                   void *out_bf16, int out_halo, float *save_mean_invstd, int stats_ready,
                                   yolo_stream_t stream);
/* Its backward.  The activation mask is recomputed from z with the forward's own fma(z, scale, shift) > 0 (mean_invstd = the 4*C floats the
 * forward saved); no y is read.  dy' = dy * (t > 0 ? 1 : slope).  pool2 = 1: dy is the gradient of the POOLED map, in pooled geometry
 * [N][H/2 + 2*dy_halo][W/2 + 2*dy_halo][C]; the four bf16-rounded y of a window are rebuilt from z, the gradient goes to the first
 * maximum in scan order (the rule of yolo_maxpool2_bwd_lrelu and of aten), the other three elements have dy' = 0.  dbeta, dgamma, dz,
 * the dz strides (zero-stuffed for a stride-2 conv), acc2c and coef3c as yolo_batchnorm_bwd; frozen = 1: the forward ran with
 * stats_ready = 2 and the two batch terms drop out.  H, W = un-pooled size of z. */
int yolo_batchnorm_bwd_lrelu(const void *dy_bf16, int dy_halo, const void *z_bf16, int z_halo, int N, int H, int W, int C,
                             const float *gamma, const float *mean_invstd, float slope, int pool2, void *dz_bf16,
                             long dz_img_stride, long dz_row_stride, long dz_px_stride, long dz_off, int frozen,
                             float *dgamma, float *dbeta, double *acc2c, float *coef3c, yolo_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * TP / FP matching of mAPMetric on the device.  Replaces the per-class greedy matching loops of
 * src/yolo/metrics.py:343-442 (AP per class and threshold), :444-491 (overall precision / recall) and :568-651 (size
 * buckets), which walk every prediction in Python.  Inputs are the device outputs of yolo_decode + yolo_nms (metrics
 * variant) and yolo_decode_gt of the same batch.  Per kept prediction k of image n (NMS output order):
 *   tp_bits[n*max_per_img + k], bit v*(T+1) + t = 1 iff the prediction is a true positive at thresholds[t] against
 *   ground-truth set v (0 all, 1 small, 2 medium, 3 large: area < small_area / < medium_area / else); t == T is
 *   `extra_threshold` (the reference's overall precision / recall use 0.5 whatever the threshold list is).
 * gt_bucket[n*max_gt + g] = 1 / 2 / 3.  thresholds is a HOST array.  T <= 15, max_per_img <= 128, max_gt <= 64. */
int yolo_map_match(const double *rec, const int32_t *keep, const int32_t *keep_counts, int N, int max_per_img,
                   const double *gt_rec, const int32_t *gt_counts, int max_gt, const double *thresholds, int T,
                   double extra_threshold, double small_area, double medium_area, unsigned long long *tp_bits,
                   int32_t *gt_bucket, yolo_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * PASCAL VOC devkit matching ("VOC devkit evaluation"; not in the reference): the kept detections of
 * yolo_decode / yolo_decode_classes + yolo_nms (metrics variant) against the ANNOTATED ground truth of their images, with
 * `difficult` flags, on clamped pixel boxes with the devkit's + 1 overlap, and the compaction of the result, in one launch
 * (one single-wave workgroup per group).
 *   rec, keep, keep_counts   as yolo_nms takes and leaves them: n_groups groups of max_per_group records
 *   groups_per_image         C behind yolo_decode_classes, 1 behind yolo_decode; group g belongs to image g / groups_per_image
 *   gt_box [G][4] f64 pixel {xmin, ymin, xmax, ymax}, gt_cls [G], gt_difficult [G] (0 / 1), gt_off [images + 1]: image n owns
 *   rows gt_off[n] .. gt_off[n+1] - 1; img_wh [images][2] f64 = {W, H} in pixels.  All in device memory.
 *   max_gt                   the largest number of ground truths of one image of the batch (the caller knows its table)
 *   thresholds               HOST array of T IoU thresholds
 * A ground truth of another class than the detection's never takes part.  Output rows are dense: group order, inside a
 * group NMS order; row r of a group starts at the sum of keep_counts of the groups in front of it, out_total[0] = number of
 * rows, rows behind it are not written:
 *   out_score [.] f64, out_cls_img [.][2] = {class, image_base + image}, out_box [.][4] = the clamped pixel corners,
 *   out_status [.] : bits 2t, 2t+1 = 0 FP, 1 TP, 2 ignored (best match is difficult) at thresholds[t].
 * The outputs hold n_groups * max_per_group rows at most.
 * Limits (YOLO_E_ARG, like null pointers and negative sizes, before any launch): 1 <= T <= 16, max_gt <= 256,
 * 1 <= max_per_group <= 1024, n_groups a multiple of groups_per_image.  n_groups == 0 succeeds with out_total[0] = 0. */
int yolo_voc_match(const double *rec, const int32_t *keep, const int32_t *keep_counts, int n_groups, int max_per_group,
                   int groups_per_image, const double *gt_box, const int32_t *gt_cls, const unsigned char *gt_difficult,
                   const int32_t *gt_off, const double *img_wh, int max_gt, int image_base, const double *thresholds, int T,
                   double *out_score, int32_t *out_cls_img, uint32_t *out_status, double *out_box, int32_t *out_total,
                   yolo_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * The final answer of batched detection ("Batched detection"; not in the reference): the kept detections of
 * yolo_decode / yolo_decode_classes + yolo_nms (variant YOLO_NMS_INFERENCE) as one dense list per image in result order, in
 * one launch (one workgroup per image), so that the copy to the host is the detections and nothing else.
 *   rec, keep, keep_counts   as yolo_nms takes and leaves them: n_groups groups of max_per_group records
 *   groups_per_image         C behind yolo_decode_classes, 1 behind yolo_decode; group g belongs to image g / groups_per_image
 *   img_wh [images][2] f64 = {W, H} in pixels, device memory, or NULL
 * Result order of image n: the kept entries of its groups, groups ascending, each group in its keep order; with
 * groups_per_image > 1 that list by score descending, equal scores in list order (numpy's stable argsort of -score, what
 * yolo/ops.py: classes_to_images does on the host).  A merge by rank: every keep list of the inference variant is in that order
 * already, which the kernel relies on.
 *   out_det [total][6] f64 = {class, score, b0, b1, b2, b3}: with img_wh the pixel corners {xmin, ymin, xmax, ymax} clamped to
 *           the image (fp64, the operations of yolo/_post_cpu.py: voc_pixel_boxes in their order), with img_wh == NULL the
 *           record's x, y, w, h bit for bit
 *   out_image [total] int32  the image of each row
 *   out_off [images + 1] int32: image n owns rows out_off[n] .. out_off[n+1] - 1; out_off[images] = total
 * Rows behind total are not written; the outputs hold n_groups * max_per_group rows at most.  No atomics: the same input gives
 * the same bits.  The scores of an image are ranked out of LDS while groups_per_image * max_per_group <= 4096 (the default model:
 * 20 x 98 = 1960); beyond that the same ranking reads them from global memory -- slower, the same result, no shape is refused.
 * YOLO_E_ARG, before any HIP call: a null pointer (img_wh excepted), n_groups < 0, max_per_group < 1, groups_per_image < 1,
 * n_groups not a multiple of groups_per_image.  YOLO_E_UNSUPPORTED: n_groups * max_per_group beyond int32.  n_groups == 0
 * succeeds with out_off[0] = 0. */
int yolo_detect_finish(const double *rec, const int32_t *keep, const int32_t *keep_counts, int n_groups, int max_per_group,
                       int groups_per_image, const double *img_wh, double *out_det, int32_t *out_image, int32_t *out_off,
                       yolo_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Image preprocessing.  Replaces YOLOInference.transform / the eval transform of the reference
 * (src/yolo/inference.py:58-66, src/yolo/dataset.py:224-233): Resize((Ho,Wo)) = PIL.Image.resize(BILINEAR) ->
 * ToTensor (/255) -> Normalize(mean, std), from decoded uint8 RGB [N][Hs][Ws][3] in device memory.
 * Resize is Pillow's two-pass 8-bit resampling, bit-exact: hbounds/vbounds = int32 [out][2] (first input index,
 * count), hcoef/vcoef = int32 [out][k] 22-bit fixed-point weights, computed by the host exactly as Pillow's
 * precompute_coeffs + normalize_coeffs_8bpc do (yolo/preprocess.py); tables may be NULL for an axis whose size does
 * not change; tmp = uint8 [N][Hs][Wo][3] scratch for the horizontal pass.  mean3 / std3 are HOST pointers.
 * Outputs (either may be NULL): out_nhwc4 = zero-haloed NHWC4 bf16 [N][Ho+2h][Wo+2h][4] (interior written, channel 3 = 0:
 * the stem's input, = yolo_nchw_f32_to_nhwc_bf16 of the fp32 result), out_nchw = fp32 [N][3][Ho][Wo] (what the
 * reference's transform returns). */
int yolo_preprocess_u8(const unsigned char *src_u8, int N, int Hs, int Ws, int Ho, int Wo, const int32_t *hbounds,
                       const int32_t *hcoef, int hk, const int32_t *vbounds, const int32_t *vcoef, int vk,
                       unsigned char *tmp_u8, const float *mean3, const float *std3, void *out_nhwc4_bf16, int halo,
                       float *out_nchw, yolo_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Training / validation input path on the device.  Replaces the per-sample host transforms of the reference
 * (src/yolo/dataset.py:288-319 RandomResizedCrop + ColorJitter, 325-409 __getitem__'s transform calls): the host decodes
 * the file and draws the random parameters; crop -> Resize (Pillow BILINEAR, bit-exact) -> ColorJitter operations in the
 * sampled order (Pillow's ImageEnhance.Brightness / ImageEnhance.Color and an H-byte shift through its HSV conversion,
 * bit-exact) -> ToTensor -> Normalize run here for a whole batch of images of DIFFERENT sizes.
 * The Darknet recipe (yolo.dataset._DarknetAugment) goes the same way: a window that may leave the image (YOLO_AUG_F_EDGE:
 * row and column are clamped to the image, i.e. the border pixels are replicated), a mirror of the output columns
 * (YOLO_AUG_F_FLIP) and YOLO_AUG_HSV, one round trip through Pillow's 8-bit HSV with the H byte shifted and the S and V
 * bytes scaled.
 * One descriptor per image; the images lie packed in one uint8 buffer (HWC RGB). */
typedef struct yolo_augment_desc {
    int64_t src_off;            /* byte offset of the image in the packed buffer */
    int64_t tmp_off;            /* byte offset of its [ch][Wo][3] slice in tmp_u8 (used when cw != Wo) */
    int32_t Hs, Ws;             /* decoded size */
    int32_t top, left, ch, cw;  /* crop (the whole image for validation); with YOLO_AUG_F_EDGE a window that may leave the image */
    /* Pillow's tables for cw -> Wo and ch -> Ho in DEVICE memory: int32 [out][2 + k] rows of (first input index, count,
       k 22-bit fixed-point weights); NULL / k = 0 for an axis whose size does not change */
    const int32_t *htab;
    const int32_t *vtab;
    int32_t hk, vk;
    int32_t n_ops;              /* 0..3 colour operations, applied in the order of ops[] */
    int32_t ops[3];             /* YOLO_AUG_BRIGHTNESS / _SATURATION / _HUE, or YOLO_AUG_HSV alone */
    float brightness;           /* ImageEnhance.Brightness factor; YOLO_AUG_HSV: the factor of the V byte */
    float saturation;           /* ImageEnhance.Color factor; YOLO_AUG_HSV: the factor of the S byte */
    int32_t hue_shift;          /* int(delta * 255), added to the H byte modulo 256 */
    int32_t flags;              /* YOLO_AUG_F_*; 0: the crop lies inside the image and is not mirrored */
} yolo_augment_desc;
#define YOLO_AUG_BRIGHTNESS 0
#define YOLO_AUG_SATURATION 1
#define YOLO_AUG_HUE 2
/* (3 is not assigned) */
#define YOLO_AUG_HSV 4          /* H := (H + hue_shift) mod 256, S := min(255, trunc(S * saturation)), V := min(255, trunc(V * brightness)),
                                   fp32 products; shares the factor fields, so it is the only entry of ops[]; factors finite and >= 0 */
#define YOLO_AUG_F_FLIP 1       /* mirror the output columns (after the resize, before the colour operations) */
#define YOLO_AUG_F_EDGE 2       /* the window may leave the image: reads are clamped to the image (edge replication); it must still
                                   intersect the image, and |top|, |left|, ch, cw <= 32768 */

/* descs_host is validated before any HIP call (known flags, crop inside its image -- with YOLO_AUG_F_EDGE: intersecting it -- and
 * the image inside src_bytes, tables present where a size changes, tmp slice inside tmp_bytes, n_ops <= 3, known operations,
 * YOLO_AUG_HSV alone and with finite factors >= 0); descs_dev is the same array in device memory, which
 * the kernels read.  Two launches for the whole batch: a horizontal pass over the crop rows of every image that needs
 * one into tmp_u8, then a vertical pass that finishes each output pixel in registers.  mean3 / std3 are HOST pointers.
 * Outputs (each may be NULL, not all): out_nhwc4 = zero-haloed NHWC4 bf16 [N][Ho+2h][Wo+2h][4] (interior written, channel
 * 3 = 0, exactly as yolo_preprocess_u8 leaves it), out_nchw = fp32 [N][3][Ho][Wo], out_u8 = the augmented image
 * [N][Ho][Wo][3] before ToTensor. */
int yolo_augment_u8(const unsigned char *src_u8, int64_t src_bytes, const yolo_augment_desc *descs_host,
                    const yolo_augment_desc *descs_dev, int N, int Ho, int Wo, unsigned char *tmp_u8, int64_t tmp_bytes,
                    const float *mean3, const float *std3, void *out_nhwc4_bf16, int halo, float *out_nchw,
                    unsigned char *out_u8, yolo_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* YOLO_HIP_H */
