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
#include "optim_common.h"

#include <algorithm>

namespace yolo {

struct EmaTable {
    yolo_ema_tensor t[YOLO_MT_MAX];
    int first[YOLO_MT_MAX + 1];       // first chunk of every tensor
    int count;
};

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

// false: the optimizer skipped this step on the device, and a skipped step is no EMA step either
__device__ __forceinline__ bool ema_begin(const float *skip_flag)
{
    return !(skip_flag && *skip_flag != 0.0f);
}

// elements [k0, end) of one tensor, one per thread and trip: the partial chunk behind a tensor's last float4 / last full chunk
__device__ __forceinline__ void ema_scalar(const yolo_ema_tensor &t, long k0, long end, long step, float w)
{
    for (long k = k0; k < end; k += step) t.ema[k] = ema1(t.ema[k], t.p[k], w);
}

__global__ void __launch_bounds__(256) ema_multi_kernel(const EmaTable tab, float w, const float *skip_flag)
{
    if (!ema_begin(skip_flag)) return;
    const int ti = find_tensor(tab.first, tab.count, blockIdx.x);
    const yolo_ema_tensor &t = tab.t[ti];
    const long beg = (long)(blockIdx.x - tab.first[ti]) * MT_CHUNK;
    const long end = min(t.n, beg + MT_CHUNK);
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
            ema_scalar(t, i, end, 1, w);
        }
    }
}

// Background form: the structure of sgd_multi_bg_kernel (sgd.hip) -- gridDim.x persistent workgroups of 1024 threads, each alone on its CU
// because of the dynamic LDS it reserves and does not use; the loads of the NEXT chunk are issued before the current one is computed and
// stored.
__global__ void __launch_bounds__(1024) ema_multi_bg_kernel(const EmaTable tab, int chunks, float w, const float *skip_flag)
{
    if (!ema_begin(skip_flag)) return;
    struct Vals {
        float4 e[2], p[2];
    };
    auto where = [&](int b, int &ti, long &beg, bool &full) {
        ti = find_tensor(tab.first, tab.count, b);
        beg = (long)(b - tab.first[ti]) * MT_CHUNK;
        full = beg + MT_CHUNK <= tab.t[ti].n;
    };
    auto load = [&](int ti, long beg, Vals &x) {
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const long i = beg + (long)(u * 1024 + threadIdx.x) * 4;
            x.e[u] = *reinterpret_cast<const float4 *>(tab.t[ti].ema + i);
            x.p[u] = *reinterpret_cast<const float4 *>(tab.t[ti].p + i);
        }
    };
    int b = blockIdx.x;
    int ti = 0, nti = 0;
    long beg = 0, nbeg = 0;
    bool full = false, nfull = false;
    Vals cur = {}, nxt = {};
    if (b < chunks) {
        where(b, ti, beg, full);
        if (full) load(ti, beg, cur);
    }
    while (b < chunks) {
        const int nb = b + (int)gridDim.x;
        if (nb < chunks) {
            where(nb, nti, nbeg, nfull);
            if (nfull) load(nti, nbeg, nxt);
        }
        const yolo_ema_tensor &t = tab.t[ti];
        if (full) {
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                const long i = beg + (long)(u * 1024 + threadIdx.x) * 4;
                *reinterpret_cast<float4 *>(t.ema + i) = ema4(cur.e[u], cur.p[u], w);
            }
        } else {
            ema_scalar(t, beg + threadIdx.x, min(t.n, beg + MT_CHUNK), 1024, w);     // last, partial chunk of a tensor
        }
        b = nb; ti = nti; beg = nbeg; full = nfull;
        cur = nxt;
    }
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

// every tensor of the call is checked before the first launch: a refused call launches nothing
static int ema_foreground(const char *who, const yolo_ema_tensor *t, int count, float w, const float *skip_flag, yolo_stream_t stream)
{
    if (int rc = ema_weight_ok(who, w)) return rc;
    for (int i = 0; i < count; ++i) {
        if (int rc = ema_tensor_ok(who, t[i], i)) return rc;
        if ((t[i].n + MT_CHUNK - 1) / MT_CHUNK > 0x7fffffffL) return fail(YOLO_E_UNSUPPORTED, "%s: tensor %d is too large", who, i);
    }
    for (int base = 0; base < count;) {
        EmaTable tab{};
        long chunks = 0;
        int k = 0;
        for (; base + k < count && k < YOLO_MT_MAX; ++k) {
            const long c = (t[base + k].n + MT_CHUNK - 1) / MT_CHUNK;
            if (chunks + c > 0x7fffffffL) break;
            tab.t[k] = t[base + k]; tab.first[k] = (int)chunks;
            chunks += c;
        }
        tab.first[k] = (int)chunks;
        tab.count = k;
        if (chunks > 0) {
            hipLaunchKernelGGL(ema_multi_kernel, dim3((unsigned)chunks), dim3(256), 0, STRM(stream), tab, w, skip_flag);
            if (int rc = check_launch(who)) return rc;
        }
        base += k;
    }
    return 0;
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
    if (!t || count < 0 || count > YOLO_MT_MAX || workgroups < 1 || workgroups > 256)
        return fail(YOLO_E_ARG, "%s: bad argument (at most %d tensors, 1 .. 256 workgroups)", who, YOLO_MT_MAX);
    if (int rc = ema_weight_ok(who, w)) return rc;
    EmaTable tab{};
    long chunks = 0;
    for (int k = 0; k < count; ++k) {
        if (int rc = ema_tensor_ok(who, t[k], k)) return rc;
        tab.t[k] = t[k]; tab.first[k] = (int)chunks;
        chunks += (t[k].n + MT_CHUNK - 1) / MT_CHUNK;
        if (chunks > 0x7fffffffL) return fail(YOLO_E_UNSUPPORTED, "%s: too many elements", who);
    }
    tab.first[count] = (int)chunks;
    tab.count = count;
    if (chunks == 0) return 0;
    constexpr int BG_LDS = 96 * 1024;       // with 1024 threads: one such workgroup per CU, and no 128-KB conv workgroup beside it
    static bool attr_done[64] = {};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) dev = 0;
    if (!attr_done[dev]) {
        hipError_t e = hipFuncSetAttribute((const void *)ema_multi_bg_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, BG_LDS);
        if (e != hipSuccess) return fail((int)e, "%s: hipFuncSetAttribute(%d B LDS): %s", who, BG_LDS, hipGetErrorString(e));
        attr_done[dev] = true;
    }
    const dim3 grid((unsigned)std::min<long>(workgroups, chunks)), block(1024);
    hipLaunchKernelGGL(ema_multi_bg_kernel, grid, block, BG_LDS, STRM(stream), tab, (int)chunks, w, skip_flag);
    return check_launch(who);
}
