// Fused SGD step for gfx950, next to the Adam pass of optim.hip: global-gradient-norm clipping + torch.optim.SGD (momentum, dampening,
// L2 weight decay, Nesterov; maximize=False) in one HBM pass -- the YOLOv1 paper's recipe on the reference's train step
// (src/yolo/training/trainer.py:79-95: clip_grad_norm_(max_norm=10), optimizer.step()).  Per element, in fp32:
//   g = grad * clip ; g += wd * p ; buf = first_step ? g : momentum * buf + (1 - dampening) * g ; g = nesterov ? g + momentum * buf : buf ;
//   p -= lr * g ; p_bf16 = bf16(p)
// One state tensor where Adam keeps two: 22 B per element with the bf16 shadow (read p, g, buf; write p, buf, shadow) against 30 B,
// 18 B on the first step (buf is only written), 12 B without momentum (buf is not touched).
// Same launch shapes as the Adam entries: a workgroup owns one MT_CHUNK slice of one tensor of the table in the kernel arguments
// (yolo_sgd_step, yolo_sgd_step_multi), or `workgroups` persistent 1024-thread workgroups walk the chunk list (yolo_sgd_step_multi_bg).
#include "optim_common.h"

#include <algorithm>

namespace yolo {

enum { MOM_NONE = 0, MOM_FIRST = 1, MOM_NEXT = 2 };   // no momentum (buf untouched) / buf = g (written only) / buf = momentum * buf + omd * g

struct SgdArgs {
    float lr, momentum, omd, wd;      // omd = 1 - dampening
    int nesterov;
    const double *norm_sq;
    float max_norm;
    const float *skip_flag;
};
struct SgdTable {
    yolo_sgd_tensor t[YOLO_MT_MAX];
    int first[YOLO_MT_MAX + 1];       // first chunk of every tensor
    int count;
};

// Every product that feeds a sum is an explicit fma and nothing else may contract: the three launch forms then compute the same bits
// (the Adam kernels leave contraction to the compiler and differ in the last bit between forms).
template <int MODE>
__device__ __forceinline__ void sgd1(float &p, float g, float &buf, float clip, const SgdArgs &a)
{
#pragma clang fp contract(off)
    g = g * clip;
    if (a.wd != 0.0f) g = __builtin_fmaf(a.wd, p, g);                           // grad.add(param, alpha=weight_decay)
    if (MODE == MOM_FIRST) buf = g;                                             // torch.clone(grad).detach()
    if (MODE == MOM_NEXT) buf = __builtin_fmaf(a.momentum, buf, a.omd * g);     // buf.mul_(momentum).add_(grad, alpha=1 - dampening)
    if (MODE != MOM_NONE) g = a.nesterov ? __builtin_fmaf(a.momentum, buf, g) : buf;
    p = __builtin_fmaf(-a.lr, g, p);                                            // param.add_(grad, alpha=-lr)
}

// false: the producer of the gradients flagged this step as invalid, nothing is updated
__device__ __forceinline__ bool sgd_begin(const SgdArgs &a, float &clip)
{
    if (a.skip_flag && *a.skip_flag != 0.0f) return false;
    clip = 1.0f;
    if (a.norm_sq) {
        const float total = (float)sqrt(*a.norm_sq);
        const float c = a.max_norm / (total + 1e-6f);
        clip = c < 1.0f ? c : 1.0f;
    }
    return true;
}

__device__ __forceinline__ uint2 pack_bf16x4(const float4 &v)
{
    uint2 o;
    o.x = (unsigned)f32_to_bf16(v.x) | ((unsigned)f32_to_bf16(v.y) << 16);
    o.y = (unsigned)f32_to_bf16(v.z) | ((unsigned)f32_to_bf16(v.w) << 16);
    return o;
}

template <int MODE>
__device__ __forceinline__ void sgd4(float4 &p, const float4 &g, float4 &b, float clip, const SgdArgs &a)
{
    sgd1<MODE>(p.x, g.x, b.x, clip, a);
    sgd1<MODE>(p.y, g.y, b.y, clip, a);
    sgd1<MODE>(p.z, g.z, b.z, clip, a);
    sgd1<MODE>(p.w, g.w, b.w, clip, a);
}

// elements [k0, end) of one tensor, one per thread and trip: the partial chunk behind a tensor's last float4 / last full chunk
template <int MODE>
__device__ __forceinline__ void sgd_scalar(const yolo_sgd_tensor &t, long k0, long end, long step, float clip, const SgdArgs &a)
{
    bf16_t *pb = (bf16_t *)t.p_bf16;
    for (long k = k0; k < end; k += step) {
        float pk = t.p[k], bk = MODE == MOM_NEXT ? t.buf[k] : 0.0f;
        sgd1<MODE>(pk, t.g[k], bk, clip, a);
        t.p[k] = pk;
        if (MODE != MOM_NONE) t.buf[k] = bk;
        if (pb) pb[k] = f32_to_bf16(pk);
    }
}

template <int MODE>
__global__ void __launch_bounds__(256) sgd_multi_kernel(const SgdTable tab, const SgdArgs a)
{
    float clip;
    if (!sgd_begin(a, clip)) return;
    const int ti = find_tensor(tab.first, tab.count, blockIdx.x);
    const yolo_sgd_tensor &t = tab.t[ti];
    const long beg = (long)(blockIdx.x - tab.first[ti]) * MT_CHUNK;
    const long end = min(t.n, beg + MT_CHUNK);
    for (long i = beg + threadIdx.x * 4; i < end; i += 1024) {
        if (i + 4 <= end) {
            float4 pv = *reinterpret_cast<const float4 *>(t.p + i);
            const float4 gv = *reinterpret_cast<const float4 *>(t.g + i);
            float4 bv = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            if (MODE == MOM_NEXT) bv = *reinterpret_cast<const float4 *>(t.buf + i);
            sgd4<MODE>(pv, gv, bv, clip, a);
            *reinterpret_cast<float4 *>(t.p + i) = pv;
            if (MODE != MOM_NONE) *reinterpret_cast<float4 *>(t.buf + i) = bv;
            if (t.p_bf16) *reinterpret_cast<uint2 *>((bf16_t *)t.p_bf16 + i) = pack_bf16x4(pv);
        } else {
            sgd_scalar<MODE>(t, i, end, 1, clip, a);
        }
    }
}

// Background form: the structure of adam_multi_bg_kernel (optim.hip) -- gridDim.x persistent workgroups of 1024 threads, each alone on its CU
// because of the dynamic LDS it reserves and does not use; the loads of the NEXT chunk are issued before the current one is computed and
// stored, so that a CU keeps 100-200 KB in flight.
template <int MODE>
__global__ void __launch_bounds__(1024) sgd_multi_bg_kernel(const SgdTable tab, int chunks, const SgdArgs a)
{
    float clip;
    if (!sgd_begin(a, clip)) return;
    struct Vals {
        float4 p[2], g[2], b[2];
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
            x.p[u] = *reinterpret_cast<const float4 *>(tab.t[ti].p + i);
            x.g[u] = *reinterpret_cast<const float4 *>(tab.t[ti].g + i);
            if (MODE == MOM_NEXT) x.b[u] = *reinterpret_cast<const float4 *>(tab.t[ti].buf + i);
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
        const yolo_sgd_tensor &t = tab.t[ti];
        if (full) {
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                const long i = beg + (long)(u * 1024 + threadIdx.x) * 4;
                sgd4<MODE>(cur.p[u], cur.g[u], cur.b[u], clip, a);
                *reinterpret_cast<float4 *>(t.p + i) = cur.p[u];
                if (MODE != MOM_NONE) *reinterpret_cast<float4 *>(t.buf + i) = cur.b[u];
                if (t.p_bf16) *reinterpret_cast<uint2 *>((bf16_t *)t.p_bf16 + i) = pack_bf16x4(cur.p[u]);
            }
        } else {
            sgd_scalar<MODE>(t, beg + threadIdx.x, min(t.n, beg + MT_CHUNK), 1024, clip, a);     // last, partial chunk of a tensor
        }
        b = nb; ti = nti; beg = nbeg; full = nfull;
        cur = nxt;
    }
}

}  // namespace yolo

using namespace yolo;

// torch.optim.SGD's constructor checks; -> the kernel arguments and the momentum mode
static int sgd_args(const char *who, float lr, float momentum, float dampening, float weight_decay, int nesterov, int first_step, const double *norm_sq,
                    float max_norm, const float *skip_flag, SgdArgs &a, int &mode)
{
    if (lr < 0.0f || momentum < 0.0f || weight_decay < 0.0f) return fail(YOLO_E_ARG, "%s: negative lr, momentum or weight_decay", who);
    if (nesterov && (momentum <= 0.0f || dampening != 0.0f)) return fail(YOLO_E_ARG, "%s: Nesterov momentum requires a momentum and zero dampening", who);
    a.lr = lr; a.momentum = momentum; a.omd = (float)(1.0 - (double)dampening); a.wd = weight_decay;
    a.nesterov = nesterov != 0;
    a.norm_sq = norm_sq; a.max_norm = max_norm; a.skip_flag = skip_flag;
    mode = momentum == 0.0f ? MOM_NONE : first_step ? MOM_FIRST : MOM_NEXT;
    return 0;
}

static int sgd_tensor_ok(const char *who, const yolo_sgd_tensor &e, int idx, int mode)
{
    if (!e.p || !e.g || (mode != MOM_NONE && !e.buf) || e.n < 0) return fail(YOLO_E_ARG, "%s: tensor %d: null pointer or negative size", who, idx);
    const uintptr_t bp = mode != MOM_NONE ? (uintptr_t)e.buf : 0;       // without momentum the kernels never form an address from buf
    if (((uintptr_t)e.p | (uintptr_t)e.g | bp) & 15) return fail(YOLO_E_UNSUPPORTED, "%s: tensor %d is not 16-B aligned", who, idx);
    if ((uintptr_t)e.p_bf16 & 7) return fail(YOLO_E_UNSUPPORTED, "%s: bf16 shadow %d is not 8-B aligned", who, idx);
    return 0;
}

// every tensor of the call is checked before the first launch: a refused call launches nothing
static int sgd_foreground(const char *who, const yolo_sgd_tensor *t, int count, const SgdArgs &a, int mode, yolo_stream_t stream)
{
    for (int i = 0; i < count; ++i) {
        if (int rc = sgd_tensor_ok(who, t[i], i, mode)) return rc;
        if ((t[i].n + MT_CHUNK - 1) / MT_CHUNK > 0x7fffffffL) return fail(YOLO_E_UNSUPPORTED, "%s: tensor %d is too large", who, i);
    }
    for (int base = 0; base < count;) {
        SgdTable tab{};
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
            const dim3 grid((unsigned)chunks), block(256);
            if (mode == MOM_NONE) hipLaunchKernelGGL(sgd_multi_kernel<MOM_NONE>, grid, block, 0, STRM(stream), tab, a);
            else if (mode == MOM_FIRST) hipLaunchKernelGGL(sgd_multi_kernel<MOM_FIRST>, grid, block, 0, STRM(stream), tab, a);
            else hipLaunchKernelGGL(sgd_multi_kernel<MOM_NEXT>, grid, block, 0, STRM(stream), tab, a);
            if (int rc = check_launch(who)) return rc;
        }
        base += k;
    }
    return 0;
}

YOLO_API int yolo_sgd_step(float *p, const float *g, float *buf, long n, float lr, float momentum, float dampening, float weight_decay, int nesterov,
                           int first_step, const double *norm_sq, float max_norm, void *p_bf16, const float *skip_flag, yolo_stream_t stream)
{
    SgdArgs a;
    int mode;
    if (int rc = sgd_args("yolo_sgd_step", lr, momentum, dampening, weight_decay, nesterov, first_step, norm_sq, max_norm, skip_flag, a, mode)) return rc;
    const yolo_sgd_tensor t = {p, g, buf, p_bf16, n};
    return sgd_foreground("yolo_sgd_step", &t, 1, a, mode, stream);
}

YOLO_API int yolo_sgd_step_multi(const yolo_sgd_tensor *t, int count, float lr, float momentum, float dampening, float weight_decay, int nesterov,
                                 int first_step, const double *norm_sq, float max_norm, const float *skip_flag, yolo_stream_t stream)
{
    if (!t || count < 0) return fail(YOLO_E_ARG, "yolo_sgd_step_multi: bad argument");
    SgdArgs a;
    int mode;
    if (int rc = sgd_args("yolo_sgd_step_multi", lr, momentum, dampening, weight_decay, nesterov, first_step, norm_sq, max_norm, skip_flag, a, mode)) return rc;
    return sgd_foreground("yolo_sgd_step_multi", t, count, a, mode, stream);
}

YOLO_API int yolo_sgd_step_multi_bg(const yolo_sgd_tensor *t, int count, float lr, float momentum, float dampening, float weight_decay, int nesterov,
                                    int first_step, const double *norm_sq, float max_norm, const float *skip_flag, int workgroups, yolo_stream_t stream)
{
    const char *who = "yolo_sgd_step_multi_bg";
    if (!t || count < 0 || count > YOLO_MT_MAX || workgroups < 1 || workgroups > 256)
        return fail(YOLO_E_ARG, "%s: bad argument (at most %d tensors, 1 .. 256 workgroups)", who, YOLO_MT_MAX);
    SgdArgs a;
    int mode;
    if (int rc = sgd_args(who, lr, momentum, dampening, weight_decay, nesterov, first_step, norm_sq, max_norm, skip_flag, a, mode)) return rc;
    SgdTable tab{};
    long chunks = 0;
    for (int k = 0; k < count; ++k) {
        if (int rc = sgd_tensor_ok(who, t[k], k, mode)) return rc;
        tab.t[k] = t[k]; tab.first[k] = (int)chunks;
        chunks += (t[k].n + MT_CHUNK - 1) / MT_CHUNK;
        if (chunks > 0x7fffffffL) return fail(YOLO_E_UNSUPPORTED, "%s: too many elements", who);
    }
    tab.first[count] = (int)chunks;
    tab.count = count;
    if (chunks == 0) return 0;
    constexpr int BG_LDS = 96 * 1024;       // with 1024 threads: one such workgroup per CU, and no 128-KB conv workgroup beside it
    const void *fn = mode == MOM_NONE ? (const void *)sgd_multi_bg_kernel<MOM_NONE>
                   : mode == MOM_FIRST ? (const void *)sgd_multi_bg_kernel<MOM_FIRST> : (const void *)sgd_multi_bg_kernel<MOM_NEXT>;
    static bool attr_done[3][64] = {};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) dev = 0;
    if (!attr_done[mode][dev]) {
        hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, BG_LDS);
        if (e != hipSuccess) return fail((int)e, "%s: hipFuncSetAttribute(%d B LDS): %s", who, BG_LDS, hipGetErrorString(e));
        attr_done[mode][dev] = true;
    }
    const dim3 grid((unsigned)std::min<long>(workgroups, chunks)), block(1024);
    const int nchunks = (int)chunks;
    if (mode == MOM_NONE) hipLaunchKernelGGL(sgd_multi_bg_kernel<MOM_NONE>, grid, block, BG_LDS, STRM(stream), tab, nchunks, a);
    else if (mode == MOM_FIRST) hipLaunchKernelGGL(sgd_multi_bg_kernel<MOM_FIRST>, grid, block, BG_LDS, STRM(stream), tab, nchunks, a);
    else hipLaunchKernelGGL(sgd_multi_bg_kernel<MOM_NEXT>, grid, block, BG_LDS, STRM(stream), tab, nchunks, a);
    return check_launch(who);
}
