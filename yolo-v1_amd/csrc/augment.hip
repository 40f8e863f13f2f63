// Training / validation input path on the device for gfx950: a batch of decoded uint8 HWC RGB images of DIFFERENT sizes ->
// per-image crop -> Resize (Pillow BILINEAR, bit-exact) -> ColorJitter operations in the sampled order (Pillow's
// ImageEnhance.Brightness / .Color and the HSV hue shift, bit-exact: augment_math.h) -> ToTensor -> Normalize -> the stem's
// input format (zero-haloed NHWC4 bf16), NCHW fp32 and / or the augmented uint8 image.
// The Darknet recipe uses the descriptor's flags: YOLO_AUG_F_EDGE, a window that may leave the image (row and column clamped
// to it), YOLO_AUG_F_FLIP, mirrored output columns (the vertical pass reads the mirrored column of stage 1), and the
// YOLO_AUG_HSV operation.  flags == 0 takes the unclamped loops, as before the flags existed.
// Replaces the per-sample host transforms of the reference (src/yolo/dataset.py:288-319 RandomResizedCrop + ColorJitter,
// 325-409 the transform calls of __getitem__), which run one PIL image at a time on the host and ship 2.4 MB of fp32 per
// image; here the host decodes the file and draws the random parameters (yolo/augment.py, yolo/dataset.py).
//
// Two launches for the whole batch, as in preprocess.hip: the horizontal pass over the crop rows only, into a ragged
// uint8 scratch (per-image offset), then the vertical pass, which finishes the pixel in registers.  blockIdx.y is the
// image, so the descriptor reads are wave-uniform.  Integer arithmetic for the resize; the colour operations and the
// normalisation are correctly rounded IEEE operations without contraction (this file is built with -ffp-contract=off and
// uses the _rn intrinsics).  Byte work bound by memory latency: one thread per output pixel (3 channels).
#include <float.h>
#include "common.h"
#include "augment_math.h"

namespace yolo {

constexpr int AUG_BITS = 32 - 8 - 2;

__device__ __forceinline__ int aug_clip8(int acc)
{
    const int v = acc >> AUG_BITS;
    return v < 0 ? 0 : (v > 255 ? 255 : v);
}

// image n: src crop rows [ch][cw][3] -> tmp + tmp_off [ch][Wo][3]   (images whose crop is Wo wide are skipped)
__global__ void __launch_bounds__(256) augment_h_u8_kernel(const unsigned char *__restrict__ src, const yolo_augment_desc *__restrict__ descs, int Wo,
                                                           unsigned char *__restrict__ tmp)
{
    const yolo_augment_desc &d = descs[blockIdx.y];
    const int hk = d.hk;
    if (hk <= 0) return;
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= d.ch * Wo) return;
    const int xx = idx % Wo, y = idx / Wo;
    const int *row = d.htab + (long)xx * (2 + hk);
    const int x0 = row[0], cnt = row[1];
    const int *k = row + 2;
    const int flags = d.flags;                                  // wave-uniform: blockIdx.y is the image
    int a0 = 1 << (AUG_BITS - 1), a1 = a0, a2 = a0;
    if (flags & YOLO_AUG_F_EDGE) {
        const unsigned char *s = src + d.src_off + (long)yolo_aug::src_row(d.top, y, d.Hs, flags) * d.Ws * 3;
        for (int x = 0; x < cnt; ++x) {
            const int w = k[x];
            const unsigned char *px = s + yolo_aug::src_col(d.left, x0 + x, d.Ws, flags) * 3;
            a0 += (int)px[0] * w;
            a1 += (int)px[1] * w;
            a2 += (int)px[2] * w;
        }
    } else {
        const unsigned char *s = src + d.src_off + ((long)(d.top + y) * d.Ws + d.left + x0) * 3;
        for (int x = 0; x < cnt; ++x) {
            const int w = k[x];
            a0 += (int)s[3 * x] * w;
            a1 += (int)s[3 * x + 1] * w;
            a2 += (int)s[3 * x + 2] * w;
        }
    }
    unsigned char *o = tmp + d.tmp_off + (long)idx * 3;
    o[0] = (unsigned char)aug_clip8(a0); o[1] = (unsigned char)aug_clip8(a1); o[2] = (unsigned char)aug_clip8(a2);
}

// image n: (tmp slice | src crop) [ch][Wo][3] -(optional vertical pass)-> [Ho][Wo][3] -> colour operations -> outputs
__global__ void __launch_bounds__(256) augment_v_color_norm_kernel(const unsigned char *__restrict__ src, const unsigned char *__restrict__ tmp,
                                                                   const yolo_augment_desc *__restrict__ descs, int Ho, int Wo, float m0, float m1, float m2,
                                                                   float s0, float s1, float s2, bf16_t *__restrict__ out4, int halo,
                                                                   float *__restrict__ out_nchw, unsigned char *__restrict__ out_u8)
{
    const int n = blockIdx.y;
    const yolo_augment_desc &d = descs[n];
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= Ho * Wo) return;
    const int xx = idx % Wo, yy = idx / Wo;
    const int flags = d.flags;                                  // wave-uniform: blockIdx.y is the image
    const int sx = yolo_aug::stage1_col(xx, Wo, flags);         // the output position stays (yy, xx)
    // stage 1 of this image: its slice of tmp (rows of Wo pixels), or the crop inside the source (rows of Ws pixels)
    const unsigned char *in;
    long row_bytes;
    if (d.hk > 0) {
        in = tmp + d.tmp_off + (long)sx * 3;
        row_bytes = (long)Wo * 3;
    } else {
        in = src + d.src_off + ((long)d.top * d.Ws + d.left + sx) * 3;
        row_bytes = (long)d.Ws * 3;
    }
    int r, g, b;
    const int vk = d.vk;
    if ((flags & YOLO_AUG_F_EDGE) && d.hk == 0) {
        // the window may leave the image and stage 1 is the source itself: every row and the column are clamped to it
        const unsigned char *col = src + d.src_off + (long)yolo_aug::src_col(d.left, sx, d.Ws, flags) * 3;
        row_bytes = (long)d.Ws * 3;
        if (vk > 0) {
            const int *row = d.vtab + (long)yy * (2 + vk);
            const int y0 = row[0], cnt = row[1];
            const int *k = row + 2;
            int a0 = 1 << (AUG_BITS - 1), a1 = a0, a2 = a0;
            for (int y = 0; y < cnt; ++y) {
                const int w = k[y];
                const unsigned char *s = col + (long)yolo_aug::src_row(d.top, y0 + y, d.Hs, flags) * row_bytes;
                a0 += (int)s[0] * w; a1 += (int)s[1] * w; a2 += (int)s[2] * w;
            }
            r = aug_clip8(a0); g = aug_clip8(a1); b = aug_clip8(a2);
        } else {
            const unsigned char *s = col + (long)yolo_aug::src_row(d.top, yy, d.Hs, flags) * row_bytes;
            r = s[0]; g = s[1]; b = s[2];
        }
    } else if (vk > 0) {
        const int *row = d.vtab + (long)yy * (2 + vk);
        const int y0 = row[0], cnt = row[1];
        const int *k = row + 2;
        const unsigned char *s = in + (long)y0 * row_bytes;
        int a0 = 1 << (AUG_BITS - 1), a1 = a0, a2 = a0;
        for (int y = 0; y < cnt; ++y) {
            const int w = k[y];
            a0 += (int)s[0] * w; a1 += (int)s[1] * w; a2 += (int)s[2] * w;
            s += row_bytes;
        }
        r = aug_clip8(a0); g = aug_clip8(a1); b = aug_clip8(a2);
    } else {
        const unsigned char *s = in + (long)yy * row_bytes;
        r = s[0]; g = s[1]; b = s[2];
    }
    const int n_ops = d.n_ops;
    for (int i = 0; i < n_ops; ++i) yolo_aug::color_op(d.ops[i], r, g, b, d.brightness, d.saturation, d.hue_shift);
    if (out_u8) {
        unsigned char *o = out_u8 + ((long)n * Ho * Wo + idx) * 3;
        o[0] = (unsigned char)r; o[1] = (unsigned char)g; o[2] = (unsigned char)b;
    }
    if (!out4 && !out_nchw) return;
    // ToTensor: uint8 -> fp32 / 255 ; Normalize: (x - mean) / std  (each operation correctly rounded, no contraction)
    const float f0 = __fdiv_rn(__fsub_rn(__fdiv_rn((float)r, 255.0f), m0), s0);
    const float f1 = __fdiv_rn(__fsub_rn(__fdiv_rn((float)g, 255.0f), m1), s1);
    const float f2 = __fdiv_rn(__fsub_rn(__fdiv_rn((float)b, 255.0f), m2), s2);
    if (out4) {
        const int Hp = Ho + 2 * halo, Wp = Wo + 2 * halo;
        uint2 o;
        o.x = (unsigned)f32_to_bf16(f0) | ((unsigned)f32_to_bf16(f1) << 16);
        o.y = (unsigned)f32_to_bf16(f2);
        *reinterpret_cast<uint2 *>(out4 + (((long)n * Hp + yy + halo) * Wp + xx + halo) * 4) = o;
    }
    if (out_nchw) {
        const long plane = (long)Ho * Wo;
        float *o = out_nchw + (long)n * 3 * plane + idx;
        o[0] = f0; o[plane] = f1; o[2 * plane] = f2;
    }
}

}  // namespace yolo

using namespace yolo;

YOLO_API int yolo_augment_u8(const unsigned char *src, int64_t src_bytes, const yolo_augment_desc *descs_host, const yolo_augment_desc *descs_dev, int N, int Ho,
                             int Wo, unsigned char *tmp, int64_t tmp_bytes, const float *mean3, const float *std3, void *out_nhwc4, int halo, float *out_nchw,
                             unsigned char *out_u8, yolo_stream_t stream)
{
    if (!src || !descs_host || !descs_dev || !mean3 || !std3 || (!out_nhwc4 && !out_nchw && !out_u8) || N <= 0 || N > 65535 || Ho <= 0 || Wo <= 0 || halo < 0
        || src_bytes <= 0 || tmp_bytes < 0 || Ho > 32768 || Wo > 32768)
        return fail(YOLO_E_ARG, "yolo_augment_u8: bad argument");
    if (std3[0] == 0.0f || std3[1] == 0.0f || std3[2] == 0.0f) return fail(YOLO_E_ARG, "yolo_augment_u8: zero std");
    int max_rows = 0;      // crop rows of the tallest image that needs the horizontal pass
    for (int n = 0; n < N; ++n) {
        const yolo_augment_desc &d = descs_host[n];
        if (d.Hs <= 0 || d.Ws <= 0 || d.Hs > 32768 || d.Ws > 32768 || d.src_off < 0 || d.src_off + (int64_t)d.Hs * d.Ws * 3 > src_bytes)
            return fail(YOLO_E_ARG, "yolo_augment_u8: image %d (%d x %d at byte %lld) lies outside the %lld-byte buffer", n, d.Hs, d.Ws, (long long)d.src_off,
                        (long long)src_bytes);
        if (d.flags & ~(YOLO_AUG_F_FLIP | YOLO_AUG_F_EDGE)) return fail(YOLO_E_ARG, "yolo_augment_u8: image %d: unknown flag bits 0x%x", n, (unsigned)d.flags);
        if (d.flags & YOLO_AUG_F_EDGE) {
            if (d.ch <= 0 || d.cw <= 0 || d.ch > 32768 || d.cw > 32768 || d.top < -32768 || d.top > 32768 || d.left < -32768 || d.left > 32768)
                return fail(YOLO_E_ARG, "yolo_augment_u8: image %d: window (top %d, left %d, %d x %d) out of range", n, d.top, d.left, d.ch, d.cw);
            if (d.top >= d.Hs || d.top + d.ch <= 0 || d.left >= d.Ws || d.left + d.cw <= 0)
                return fail(YOLO_E_ARG, "yolo_augment_u8: image %d: window (top %d, left %d, %d x %d) misses its %d x %d image", n, d.top, d.left, d.ch, d.cw, d.Hs,
                            d.Ws);
        } else if (d.top < 0 || d.left < 0 || d.ch <= 0 || d.cw <= 0 || d.top > d.Hs - d.ch || d.left > d.Ws - d.cw)
            return fail(YOLO_E_ARG, "yolo_augment_u8: image %d: crop (top %d, left %d, %d x %d) outside its %d x %d image", n, d.top, d.left, d.ch, d.cw, d.Hs, d.Ws);
        if (d.cw != Wo) {
            if (!d.htab || d.hk <= 0) return fail(YOLO_E_ARG, "yolo_augment_u8: image %d: width %d -> %d needs the horizontal table", n, d.cw, Wo);
            if (!tmp || d.tmp_off < 0 || d.tmp_off + (int64_t)d.ch * Wo * 3 > tmp_bytes)
                return fail(YOLO_E_ARG, "yolo_augment_u8: image %d: its horizontal-pass slice lies outside the %lld-byte scratch", n, (long long)tmp_bytes);
            if (d.ch > max_rows) max_rows = d.ch;
        } else if (d.hk != 0) {
            return fail(YOLO_E_ARG, "yolo_augment_u8: image %d: a horizontal table for an unchanged width", n);
        }
        if (d.ch != Ho ? (!d.vtab || d.vk <= 0) : d.vk != 0) return fail(YOLO_E_ARG, "yolo_augment_u8: image %d: height %d -> %d and the vertical table disagree", n, d.ch, Ho);
        if (d.n_ops < 0 || d.n_ops > 3) return fail(YOLO_E_ARG, "yolo_augment_u8: image %d: %d colour operations (0..3)", n, d.n_ops);
        for (int i = 0; i < d.n_ops; ++i) {
            if (d.ops[i] == YOLO_AUG_HSV) {
                if (d.n_ops != 1) return fail(YOLO_E_ARG, "yolo_augment_u8: image %d: YOLO_AUG_HSV shares the factor fields and has to be the only operation", n);
                if (!(d.saturation >= 0.0f && d.saturation <= FLT_MAX && d.brightness >= 0.0f && d.brightness <= FLT_MAX))
                    return fail(YOLO_E_ARG, "yolo_augment_u8: image %d: YOLO_AUG_HSV factors (S %g, V %g) must be finite and >= 0", n, (double)d.saturation,
                                (double)d.brightness);
            } else if (d.ops[i] < YOLO_AUG_BRIGHTNESS || d.ops[i] > YOLO_AUG_HUE) {
                return fail(YOLO_E_ARG, "yolo_augment_u8: image %d: unknown colour operation %d", n, d.ops[i]);
            }
        }
    }
    hipStream_t s = STRM(stream);
    if (max_rows > 0) {
        const long per = (long)max_rows * Wo;
        hipLaunchKernelGGL(augment_h_u8_kernel, dim3((unsigned)((per + 255) / 256), (unsigned)N), dim3(256), 0, s, src, descs_dev, Wo, tmp);
        if (int rc = check_launch("yolo_augment_u8(horizontal)")) return rc;
    }
    const long per = (long)Ho * Wo;
    hipLaunchKernelGGL(augment_v_color_norm_kernel, dim3((unsigned)((per + 255) / 256), (unsigned)N), dim3(256), 0, s, src, tmp, descs_dev, Ho, Wo, mean3[0], mean3[1],
                       mean3[2], std3[0], std3[1], std3[2], (bf16_t *)out_nhwc4, halo, out_nchw, out_u8);
    return check_launch("yolo_augment_u8");
}
