// Exponential moving average of the weights for gfx950, next to the optimizer passes of optim.hip and sgd.hip: what
// torch.optim.swa_utils.get_ema_multi_avg_fn does with torch._foreach_lerp_(ema, params, 1 - decay), as one multi-tensor HBM pass.
// Per element, in fp32:
//   e = fmaf(w, p - e, e)          w = (float)(1.0 - decay), formed by the host in double
// -- one rounding for the difference and one for the fused multiply-add, torch.lerp's form for weights below 0.5.  The difference is a
// single operation and the product feeds an explicit fma, so nothing is left to contraction and the three launch forms compute the
// same bits.  w = 0 leaves e as it is, w = 1 gives fmaf(1, p - e, e), which is p up to one rounding.
// 12 B per element: read e and p, write e.  p is never written.
// Same launch shapes as the SGD entries: a workgroup owns one MT_CHUNK slice of one tensor of the table in the kernel arguments
// (yolo_ema_update, yolo_ema_update_multi), or `workgroups` persistent 1024-thread workgroups walk the chunk list (yolo_ema_update_multi_bg).
#include "multi_tensor.h"

namespace yolo {

__device__ __forceinline__ float ema1(float e, float p, float w)
{
#pragma clang fp contract(off)
    const float d = p - e;
    return __builtin_fmaf(w, d, e);
}

__device__ __forceinline__ float4 ema4(const float4 &e, const float4 &p, float w)
{
    return make_float4(ema1(e.x, p.x, w), ema1(e.y, p.y, w), ema1(e.z, p.z, w), ema1(e.w, p.w, w));
}

// The element op of the background kernel (multi_tensor.h: mt_walk_bg); the foreground kernel shares its tail
struct EmaOp {
    float w;
    struct Vals {
        float4 e[2], p[2];
    };
    __device__ __forceinline__ void load(const yolo_ema_tensor &t, long i, int u, Vals &x) const
    {
        x.e[u] = *reinterpret_cast<const float4 *>(t.ema + i);
        x.p[u] = *reinterpret_cast<const float4 *>(t.p + i);
    }
    __device__ __forceinline__ void full(const yolo_ema_tensor &t, long i, int u, Vals &x) const
    {
        *reinterpret_cast<float4 *>(t.ema + i) = ema4(x.e[u], x.p[u], w);
    }
    __device__ __forceinline__ void tail(const yolo_ema_tensor &t, long k0, long end, long step) const
    {
        for (long k = k0; k < end; k += step) t.ema[k] = ema1(t.ema[k], t.p[k], w);
    }
};

// a skipped optimizer step (skip_flag) is no EMA step either
__global__ void __launch_bounds__(256) ema_multi_kernel(const MtTable<yolo_ema_tensor> tab, float w, const float *skip_flag)
{
    if (mt_skipped(skip_flag)) return;
    long beg, end;
    const yolo_ema_tensor &t = mt_slice<MT_CHUNK>(tab, beg, end);
    if (beg + MT_CHUNK <= t.n) {
        // a whole chunk: all sixteen 16-B loads of a lane are issued before the first result is used (64 KB in flight per workgroup)
        float4 ev[8], pv[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const long i = beg + (long)(u * 256 + threadIdx.x) * 4;
            ev[u] = *reinterpret_cast<const float4 *>(t.ema + i);
            pv[u] = *reinterpret_cast<const float4 *>(t.p + i);
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const long i = beg + (long)(u * 256 + threadIdx.x) * 4;
            *reinterpret_cast<float4 *>(t.ema + i) = ema4(ev[u], pv[u], w);
        }
        return;
    }
    for (long i = beg + threadIdx.x * 4; i < end; i += 1024) {
        if (i + 4 <= end) {
            const float4 ev = *reinterpret_cast<const float4 *>(t.ema + i);
            const float4 pv = *reinterpret_cast<const float4 *>(t.p + i);
            *reinterpret_cast<float4 *>(t.ema + i) = ema4(ev, pv, w);
        } else {
            EmaOp{w}.tail(t, i, end, 1);
        }
    }
}

__global__ void __launch_bounds__(1024) ema_multi_bg_kernel(const MtTable<yolo_ema_tensor> tab, int chunks, float w, const float *skip_flag)
{
    if (mt_skipped(skip_flag)) return;
    mt_walk_bg(tab, chunks, EmaOp{w});
}

}  // namespace yolo

using namespace yolo;

static int ema_weight_ok(const char *who, float w)
{
    if (!(w >= 0.0f && w <= 1.0f)) return fail(YOLO_E_ARG, "%s: weight %g is not in [0, 1]", who, (double)w);      // NaN fails both comparisons
    return 0;
}

static int ema_tensor_ok(const char *who, const yolo_ema_tensor &e, int idx)
{
    if (!e.ema || !e.p || e.n < 0) return fail(YOLO_E_ARG, "%s: tensor %d: null pointer or negative size", who, idx);
    if (((uintptr_t)e.ema | (uintptr_t)e.p) & 15) return fail(YOLO_E_UNSUPPORTED, "%s: tensor %d is not 16-B aligned", who, idx);
    // a workgroup reads p where another may already have written ema: the result would depend on the order they ran in
    const uintptr_t a = (uintptr_t)e.ema, b = (uintptr_t)e.p, bytes = (uintptr_t)e.n * sizeof(float);
    if (e.n > 0 && a < b + bytes && b < a + bytes) return fail(YOLO_E_UNSUPPORTED, "%s: tensor %d: ema overlaps p", who, idx);
    return 0;
}

static int ema_foreground(const char *who, const yolo_ema_tensor *t, int count, float w, const float *skip_flag, yolo_stream_t stream)
{
    if (int rc = ema_weight_ok(who, w)) return rc;
    return mt_foreground<MT_CHUNK>(who, t, count, ema_tensor_ok, [&](const MtTable<yolo_ema_tensor> &tab, long chunks) {
        hipLaunchKernelGGL(ema_multi_kernel, dim3((unsigned)chunks), dim3(256), 0, STRM(stream), tab, w, skip_flag);
        return check_launch(who);
    });
}

YOLO_API int yolo_ema_update(float *ema, const float *p, long n, float w, const float *skip_flag, yolo_stream_t stream)
{
    const yolo_ema_tensor t = {ema, p, n};
    return ema_foreground("yolo_ema_update", &t, 1, w, skip_flag, stream);
}

YOLO_API int yolo_ema_update_multi(const yolo_ema_tensor *t, int count, float w, const float *skip_flag, yolo_stream_t stream)
{
    if (!t || count < 0) return fail(YOLO_E_ARG, "yolo_ema_update_multi: bad argument");
    return ema_foreground("yolo_ema_update_multi", t, count, w, skip_flag, stream);
}

YOLO_API int yolo_ema_update_multi_bg(const yolo_ema_tensor *t, int count, float w, const float *skip_flag, int workgroups, yolo_stream_t stream)
{
    const char *who = "yolo_ema_update_multi_bg";
    if (int rc = ema_weight_ok(who, w)) return rc;
    static bool lds_done[64] = {};
    MtBackground<yolo_ema_tensor> bg;
    if (int rc = mt_background(who, t, count, workgroups, true, ema_tensor_ok, (const void *)ema_multi_bg_kernel, lds_done, bg)) return rc;
    if (bg.grid == 0) return 0;
    hipLaunchKernelGGL(ema_multi_bg_kernel, dim3(bg.grid), dim3(1024), BG_LDS, STRM(stream), bg.tab, bg.chunks, w, skip_flag);
    return check_launch(who);
}
