// Gradient accumulation for gfx950, next to the optimizer passes of optim.hip / sgd.hip and the weight EMA of ema.hip: K micro-batches per
// optimizer step (DDP's no_sync, Darknet's subdivisions) as one multi-tensor HBM pass per micro-batch.  Per element, in fp32:
//   dst = fmaf(alpha, x, y)        y != NULL
//   dst = alpha * x                y == NULL   (one rounding)
// alpha = (float)(1.0 / K), formed by the host in double.  The product inside the fma is exact, so either form rounds once; the fma is explicit
// and contraction is off, so the single and the multi-tensor form compute the same bits.
// dst may be exactly x or exactly y (the in-place uses: acc = fmaf(alpha, g, acc) and the fold g = fmaf(alpha, g, acc)): a lane reads its
// elements before it writes them and no other lane touches them.  8 B per element without y, 12 B with it.
// Foreground launch shape of multi_tensor.h: a workgroup owns one MT_CHUNK slice of one tensor of the table in the kernel arguments.
#include "multi_tensor.h"

#include <cmath>

namespace yolo {

__device__ __forceinline__ float accum1(float x, float y, float alpha)
{
#pragma clang fp contract(off)
    return __builtin_fmaf(alpha, x, y);
}

__device__ __forceinline__ float scale1(float x, float alpha)
{
#pragma clang fp contract(off)
    return alpha * x;
}

__device__ __forceinline__ float4 accum4(const float4 &x, const float4 &y, float alpha)
{
    return make_float4(accum1(x.x, y.x, alpha), accum1(x.y, y.y, alpha), accum1(x.z, y.z, alpha), accum1(x.w, y.w, alpha));
}

__device__ __forceinline__ float4 scale4(const float4 &x, float alpha)
{
    return make_float4(scale1(x.x, alpha), scale1(x.y, alpha), scale1(x.z, alpha), scale1(x.w, alpha));
}

__global__ void __launch_bounds__(256) accum_multi_kernel(const MtTable<yolo_accum_tensor> tab, float alpha, const float *skip_flag)
{
    if (mt_skipped(skip_flag)) return;
    long beg, end;
    const yolo_accum_tensor &t = mt_slice<MT_CHUNK>(tab, beg, end);
    const bool has_y = t.y != nullptr;                  // uniform over the workgroup
    if (beg + MT_CHUNK <= t.n) {
        // a whole chunk: all 16-B loads of a lane (sixteen with y, eight without) are issued before the first store
        float4 xv[8], yv[8];
        if (has_y) {
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const long i = beg + (long)(u * 256 + threadIdx.x) * 4;
                xv[u] = *reinterpret_cast<const float4 *>(t.x + i);
                yv[u] = *reinterpret_cast<const float4 *>(t.y + i);
            }
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const long i = beg + (long)(u * 256 + threadIdx.x) * 4;
                *reinterpret_cast<float4 *>(t.dst + i) = accum4(xv[u], yv[u], alpha);
            }
        } else {
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const long i = beg + (long)(u * 256 + threadIdx.x) * 4;
                xv[u] = *reinterpret_cast<const float4 *>(t.x + i);
            }
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const long i = beg + (long)(u * 256 + threadIdx.x) * 4;
                *reinterpret_cast<float4 *>(t.dst + i) = scale4(xv[u], alpha);
            }
        }
        return;
    }
    for (long i = beg + threadIdx.x * 4; i < end; i += 1024) {
        if (i + 4 <= end) {
            const float4 xv = *reinterpret_cast<const float4 *>(t.x + i);
            if (has_y) {
                const float4 yv = *reinterpret_cast<const float4 *>(t.y + i);
                *reinterpret_cast<float4 *>(t.dst + i) = accum4(xv, yv, alpha);
            } else {
                *reinterpret_cast<float4 *>(t.dst + i) = scale4(xv, alpha);
            }
        } else {
            for (long k = i; k < end; ++k) t.dst[k] = has_y ? accum1(t.x[k], t.y[k], alpha) : scale1(t.x[k], alpha);     // behind the last float4
        }
    }
}

}  // namespace yolo

using namespace yolo;

static int accum_tensor_ok(const char *who, const yolo_accum_tensor &a, int idx)
{
    if (!a.dst || !a.x || a.n < 0) return fail(YOLO_E_ARG, "%s: tensor %d: null pointer or negative size", who, idx);
    if (((uintptr_t)a.dst | (uintptr_t)a.x | (uintptr_t)a.y) & 15) return fail(YOLO_E_UNSUPPORTED, "%s: tensor %d is not 16-B aligned", who, idx);
    // dst == x or dst == y: every element is read and written by one lane.  Any other overlap: a workgroup would read where another may
    // already have written, and the result would depend on the order they ran in
    const uintptr_t d = (uintptr_t)a.dst, bytes = (uintptr_t)a.n * sizeof(float);
    for (const float *src : {a.x, a.y}) {
        const uintptr_t s = (uintptr_t)src;
        if (src && a.n > 0 && s != d && d < s + bytes && s < d + bytes)
            return fail(YOLO_E_UNSUPPORTED, "%s: tensor %d: dst overlaps %s without being it", who, idx, src == a.x ? "x" : "y");
    }
    return 0;
}

static int accum_launch(const char *who, const yolo_accum_tensor *t, int count, float alpha, const float *skip_flag, yolo_stream_t stream)
{
    if (!std::isfinite(alpha)) return fail(YOLO_E_ARG, "%s: alpha %g is not finite", who, (double)alpha);
    return mt_foreground<MT_CHUNK>(who, t, count, accum_tensor_ok, [&](const MtTable<yolo_accum_tensor> &tab, long chunks) {
        hipLaunchKernelGGL(accum_multi_kernel, dim3((unsigned)chunks), dim3(256), 0, STRM(stream), tab, alpha, skip_flag);
        return check_launch(who);
    });
}

YOLO_API int yolo_grad_accum(float *dst, const float *x, const float *y, long n, float alpha, const float *skip_flag, yolo_stream_t stream)
{
    const yolo_accum_tensor t = {dst, x, y, n};
    return accum_launch("yolo_grad_accum", &t, 1, alpha, skip_flag, stream);
}

YOLO_API int yolo_grad_accum_multi(const yolo_accum_tensor *t, int count, float alpha, const float *skip_flag, yolo_stream_t stream)
{
    if (!t || count < 0) return fail(YOLO_E_ARG, "yolo_grad_accum_multi: bad argument");
    return accum_launch("yolo_grad_accum_multi", t, count, alpha, skip_flag, stream);
}
