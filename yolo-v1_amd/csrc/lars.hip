// LARS (You, Gitman, Ginsburg 2017: layer-wise adaptive rate scaling) for gfx950, next to the SGD pass of sgd.hip: what a large-batch run
// (--accum-steps x ranks x batch 64) needs beyond SGD with momentum, as two multi-tensor HBM passes on multi_tensor.h.
//
// 1. Per-tensor norms, order-fixed, no atomics (the structure of norm_fixed.hip): a 256-thread workgroup owns one SQ_CHUNK slice of one
//    tensor and STORES two fp64 partials, sum p^2 in scratch slot 2 * blockIdx.x and sum g^2 in slot 2 * blockIdx.x + 1 (wg_sumsq's
//    grouping for both); a finish kernel with one workgroup per tensor adds that tensor's slots first[i] .. first[i+1] in a fixed order
//    (thread t: slots t, t + 256, .. in rising order; then the 256 thread sums in rising order) and stores norms[2i], norms[2i+1].  A last
//    one-thread stage stores *g_total = norms[1] + norms[3] + .. in rising order: the global squared gradient norm of the folded clip, so
//    a LARS step reads the gradients twice (norms, step), never a third time.  8 B per element.
// 2. The step, in the three forms of SGD.  Per tensor, in fp64, wave-uniform (once per workgroup, once per chunk in the background form):
//      wn = sqrt(norms[0]) ; gn = (double)clip * sqrt(norms[1])
//      trust = (adapt && wn > 0 && gn > 0) ? (float)((double)eta * wn / (gn + (double)wd * wn + (double)eps)) : 1.0f
//    Per element, in fp32, every a * b + c an explicit fma and nothing else contracted (the three forms: the same bits, as sgd1):
//      g = grad * clip ; g = fma(wd, p, g) (wd != 0) ; g = g * trust ; buf = first_step ? g : fma(momentum, buf, g) ; p = fma(-lr, buf, p)
//    i.e. the regularised gradient scaled by the trust ratio, then torch.optim.SGD(weight_decay=0): no dampening, no Nesterov.  With
//    adapt == 0 the element op is sgd1's with dampening 0 (g * 1.0f is g).  22 B per element with the bf16 shadow, as SGD.
#include "multi_tensor.h"

#include <vector>

namespace yolo {

// ---- norms ----

struct LarsNormTensor {
    const float *p, *g;
    long n;
};

__global__ void __launch_bounds__(256) lars_norm_part_kernel(const MtTable<LarsNormTensor> tab, double *__restrict__ slots)
{
    long beg, end;
    const LarsNormTensor &t = mt_slice<SQ_CHUNK>(tab, beg, end);
    const long s = 2 * (long)blockIdx.x;
    wg_sumsq(t.p, beg + threadIdx.x * 4, end, 1024, [&](double v) { slots[s] = v; });
    __syncthreads();
    wg_sumsq(t.g, beg + threadIdx.x * 4, end, 1024, [&](double v) { slots[s + 1] = v; });
}

// workgroup i: tensor i of the launch's table -> norms[2i], norms[2i+1] (norms already at the launch's tensor offset); an empty tensor: 0, 0
__global__ void __launch_bounds__(256) lars_norm_finish_kernel(const MtTable<LarsNormTensor> tab, const double *__restrict__ slots, double *__restrict__ norms)
{
    const int lo = tab.first[blockIdx.x], hi = tab.first[blockIdx.x + 1];
    double sp = 0.0, sg = 0.0;
    for (int i = lo + (int)threadIdx.x; i < hi; i += 256) {
        sp += slots[2 * (long)i];
        sg += slots[2 * (long)i + 1];
    }
    __shared__ double redp[256], redg[256];
    redp[threadIdx.x] = sp;
    redg[threadIdx.x] = sg;
    __syncthreads();
    if (threadIdx.x == 0) {
        double tp = redp[0], tg = redg[0];
        for (int k = 1; k < 256; ++k) {
            tp += redp[k];
            tg += redg[k];
        }
        norms[2 * (long)blockIdx.x] = tp;
        norms[2 * (long)blockIdx.x + 1] = tg;
    }
}

__global__ void __launch_bounds__(64) lars_norm_total_kernel(const double *__restrict__ norms, int count, double *__restrict__ g_total)
{
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    double t = 0.0;
    for (int i = 0; i < count; ++i) t += norms[2 * (long)i + 1];
    *g_total = t;
}

// ---- step ----

enum { MOM_NONE = 0, MOM_FIRST = 1, MOM_NEXT = 2 };   // as sgd.hip: buf untouched / buf = g (written only) / buf = fma(momentum, buf, g)

struct LarsArgs {
    float lr, momentum, wd, eta, eps;
    const double *norm_sq;
    float max_norm;
    const float *skip_flag;
};

// the trust ratio of one tensor: fp64 from the two stored sums, narrowed once (tests/lars_ref.py::trust_ref restates it)
__device__ __forceinline__ float lars_trust(const yolo_lars_tensor &t, float clip, const LarsArgs &a)
{
#pragma clang fp contract(off)
    if (!t.adapt || !t.norms) return 1.0f;
    const double wn = sqrt(t.norms[0]);
    const double gn = (double)clip * sqrt(t.norms[1]);
    if (!(wn > 0.0 && gn > 0.0)) return 1.0f;
    const double den = (gn + (double)a.wd * wn) + (double)a.eps;
    return (float)((double)a.eta * wn / den);
}

template <int MODE>
__device__ __forceinline__ void lars1(float &p, float g, float &buf, float clip, float trust, const LarsArgs &a)
{
#pragma clang fp contract(off)
    g = g * clip;
    if (a.wd != 0.0f) g = __builtin_fmaf(a.wd, p, g);
    g = g * trust;
    if (MODE == MOM_FIRST) buf = g;
    if (MODE == MOM_NEXT) buf = __builtin_fmaf(a.momentum, buf, g);
    if (MODE != MOM_NONE) g = buf;
    p = __builtin_fmaf(-a.lr, g, p);
}

// The element op of both step kernels (multi_tensor.h: mt_walk_bg).  The background walk hands every call its tensor; the trust ratio of a
// full chunk is taken with the loads of the chunk (load, u == 0) and travels with the chunk's values.  It is FORMED only when the walk
// enters another tensor (trust_of): the two doubles come through a vector load, and the s_waitcnt vmcnt(0) in front of the fp64
// arithmetic also waits for the chunk prefetched before -- formed per chunk, it left one chunk in flight instead of two (the Linear
// layers' pass alone on 128 CUs: 1.088 ms per chunk-wise trust, 1.056 ms this way; yolo_sgd_step_multi_bg 1.036 ms).
template <int MODE>
struct LarsOp {
    float clip;
    const LarsArgs &a;
    mutable const float *last_p = nullptr;      // the tensor last_trust belongs to (p is never NULL)
    mutable float last_trust = 1.0f;
    struct Vals {
        float4 p[2], g[2], b[2];
        float trust;
    };
    __device__ __forceinline__ float trust_of(const yolo_lars_tensor &t) const
    {
        if (t.p != last_p) {        // wave-uniform: the table lies in the kernel arguments
            last_trust = lars_trust(t, clip, a);
            last_p = t.p;
        }
        return last_trust;
    }
    __device__ __forceinline__ void vec(const yolo_lars_tensor &t, long i, float4 &p, const float4 &g, float4 &b, float trust) const
    {
        lars1<MODE>(p.x, g.x, b.x, clip, trust, a);
        lars1<MODE>(p.y, g.y, b.y, clip, trust, a);
        lars1<MODE>(p.z, g.z, b.z, clip, trust, a);
        lars1<MODE>(p.w, g.w, b.w, clip, trust, a);
        *reinterpret_cast<float4 *>(t.p + i) = p;
        if (MODE != MOM_NONE) *reinterpret_cast<float4 *>(t.buf + i) = b;
        if (t.p_bf16) *reinterpret_cast<uint2 *>((bf16_t *)t.p_bf16 + i) = pack_bf16x4(p);
    }
    __device__ __forceinline__ void load(const yolo_lars_tensor &t, long i, int u, Vals &x) const
    {
        if (u == 0) x.trust = trust_of(t);
        x.p[u] = *reinterpret_cast<const float4 *>(t.p + i);
        x.g[u] = *reinterpret_cast<const float4 *>(t.g + i);
        if (MODE == MOM_NEXT) x.b[u] = *reinterpret_cast<const float4 *>(t.buf + i);
    }
    __device__ __forceinline__ void full(const yolo_lars_tensor &t, long i, int u, Vals &x) const { vec(t, i, x.p[u], x.g[u], x.b[u], x.trust); }
    __device__ __forceinline__ void tail(const yolo_lars_tensor &t, long k0, long end, long step, float trust) const
    {
        bf16_t *pb = (bf16_t *)t.p_bf16;
        for (long k = k0; k < end; k += step) {
            float pk = t.p[k], bk = MODE == MOM_NEXT ? t.buf[k] : 0.0f;
            lars1<MODE>(pk, t.g[k], bk, clip, trust, a);
            t.p[k] = pk;
            if (MODE != MOM_NONE) t.buf[k] = bk;
            if (pb) pb[k] = f32_to_bf16(pk);
        }
    }
    __device__ __forceinline__ void tail(const yolo_lars_tensor &t, long k0, long end, long step) const
    {
        tail(t, k0, end, step, trust_of(t));
    }
};

template <int MODE>
__global__ void __launch_bounds__(256) lars_multi_kernel(const MtTable<yolo_lars_tensor> tab, const LarsArgs a)
{
    if (mt_skipped(a.skip_flag)) return;
    const LarsOp<MODE> op{clip_coefficient(a.norm_sq, a.max_norm), a};
    long beg, end;
    const yolo_lars_tensor &t = mt_slice<MT_CHUNK>(tab, beg, end);
    const float trust = lars_trust(t, op.clip, a);
    for (long i = beg + threadIdx.x * 4; i < end; i += 1024) {
        if (i + 4 <= end) {
            float4 pv = *reinterpret_cast<const float4 *>(t.p + i);
            const float4 gv = *reinterpret_cast<const float4 *>(t.g + i);
            float4 bv = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            if (MODE == MOM_NEXT) bv = *reinterpret_cast<const float4 *>(t.buf + i);
            op.vec(t, i, pv, gv, bv, trust);
        } else {
            op.tail(t, i, end, 1, trust);
        }
    }
}

template <int MODE>
__global__ void __launch_bounds__(1024) lars_multi_bg_kernel(const MtTable<yolo_lars_tensor> tab, int chunks, const LarsArgs a)
{
    if (mt_skipped(a.skip_flag)) return;
    mt_walk_bg(tab, chunks, LarsOp<MODE>{clip_coefficient(a.norm_sq, a.max_norm), a});
}

}  // namespace yolo

using namespace yolo;

// ---- norms: host ----

YOLO_API int yolo_lars_norm_slots(const long *n, int count, long *slots)
{
    if (!n || !slots || count < 0) return fail(YOLO_E_ARG, "yolo_lars_norm_slots: bad argument");
    long tot = 0;
    for (int i = 0; i < count; ++i) {
        if (n[i] < 0) return fail(YOLO_E_ARG, "yolo_lars_norm_slots: tensor %d: negative size", i);
        tot += 2 * mt_chunks<SQ_CHUNK>(n[i]);
    }
    *slots = tot;
    return 0;
}

static int lars_norm_tensor_ok(const char *who, const LarsNormTensor &e, int idx)
{
    if (!e.p || !e.g || e.n < 0) return fail(YOLO_E_ARG, "%s: tensor %d: null pointer or negative size", who, idx);
    if (((uintptr_t)e.p | (uintptr_t)e.g) & 15) return fail(YOLO_E_UNSUPPORTED, "%s: tensor %d is not 16-B aligned", who, idx);
    return 0;
}

YOLO_API int yolo_lars_norms_multi(const float *const *p, const float *const *g, const long *n, int count, double *scratch, long scratch_slots,
                                   double *norms, double *g_total, yolo_stream_t stream)
{
    const char *who = "yolo_lars_norms_multi";
    if (!p || !g || !n || !norms || count < 0 || scratch_slots < 0) return fail(YOLO_E_ARG, "%s: bad argument", who);
    if (((uintptr_t)norms | (uintptr_t)g_total) & 7) return fail(YOLO_E_UNSUPPORTED, "%s: norms and g_total must be 8-B aligned", who);
    std::vector<LarsNormTensor> t(count);
    long total = 0;
    for (int i = 0; i < count; ++i) {
        t[i] = {p[i], g[i], n[i]};
        total += n[i] < 0 ? 0 : 2 * mt_chunks<SQ_CHUNK>(n[i]);
    }
    if (int rc = mt_check<SQ_CHUNK>(who, t.data(), count, lars_norm_tensor_ok)) return rc;
    if (total > 0 && (!scratch || ((uintptr_t)scratch & 7) || scratch_slots < total))
        return fail(YOLO_E_ARG, "%s: scratch holds %ld doubles, these tensors need %ld (yolo_lars_norm_slots)", who, scratch_slots, total);
    // not mt_launch: a table of empty tensors has no chunks, and its norms are still stored (0, 0)
    for (int base = 0; base < count;) {
        MtTable<LarsNormTensor> tab{};
        long chunks;
        const int took = mt_fill<SQ_CHUNK>(tab, t.data() + base, count - base, chunks);
        // the launches of one call run one after the other on the stream: each reuses the scratch from slot 0
        if (chunks > 0) {
            hipLaunchKernelGGL(lars_norm_part_kernel, dim3((unsigned)chunks), dim3(256), 0, STRM(stream), tab, scratch);
            if (int rc = check_launch(who)) return rc;
        }
        hipLaunchKernelGGL(lars_norm_finish_kernel, dim3((unsigned)took), dim3(256), 0, STRM(stream), tab, (const double *)scratch, norms + 2 * (long)base);
        if (int rc = check_launch("yolo_lars_norms_multi (finish)")) return rc;
        base += took;
    }
    if (g_total) {
        hipLaunchKernelGGL(lars_norm_total_kernel, dim3(1), dim3(64), 0, STRM(stream), (const double *)norms, count, g_total);
        return check_launch("yolo_lars_norms_multi (total)");
    }
    return 0;
}

// ---- step: host ----

static int lars_args(const char *who, float lr, float momentum, float weight_decay, float eta, float eps, int first_step, const double *norm_sq,
                     float max_norm, const float *skip_flag, LarsArgs &a, int &mode)
{
    if (lr < 0.0f || momentum < 0.0f || weight_decay < 0.0f) return fail(YOLO_E_ARG, "%s: negative lr, momentum or weight_decay", who);
    if (eta < 0.0f || eps < 0.0f) return fail(YOLO_E_ARG, "%s: negative eta or eps", who);
    a.lr = lr; a.momentum = momentum; a.wd = weight_decay; a.eta = eta; a.eps = eps;
    a.norm_sq = norm_sq; a.max_norm = max_norm; a.skip_flag = skip_flag;
    mode = momentum == 0.0f ? MOM_NONE : first_step ? MOM_FIRST : MOM_NEXT;
    return 0;
}

static int lars_tensor_ok(const char *who, const yolo_lars_tensor &e, int idx, int mode)
{
    if (!e.p || !e.g || (mode != MOM_NONE && !e.buf) || e.n < 0) return fail(YOLO_E_ARG, "%s: tensor %d: null pointer or negative size", who, idx);
    if (e.adapt && !e.norms) return fail(YOLO_E_ARG, "%s: tensor %d: adapt without norms", who, idx);
    const uintptr_t bp = mode != MOM_NONE ? (uintptr_t)e.buf : 0;       // without momentum the kernels never form an address from buf
    if (((uintptr_t)e.p | (uintptr_t)e.g | bp) & 15) return fail(YOLO_E_UNSUPPORTED, "%s: tensor %d is not 16-B aligned", who, idx);
    if ((uintptr_t)e.p_bf16 & 7) return fail(YOLO_E_UNSUPPORTED, "%s: bf16 shadow %d is not 8-B aligned", who, idx);
    if ((uintptr_t)e.norms & 7) return fail(YOLO_E_UNSUPPORTED, "%s: norms %d are not 8-B aligned", who, idx);
    return 0;
}

static int lars_foreground(const char *who, const yolo_lars_tensor *t, int count, const LarsArgs &a, int mode, yolo_stream_t stream)
{
    auto ok = [&](const char *w, const yolo_lars_tensor &e, int idx) { return lars_tensor_ok(w, e, idx, mode); };
    return mt_foreground<MT_CHUNK>(who, t, count, ok, [&](const MtTable<yolo_lars_tensor> &tab, long chunks) {
        const dim3 grid((unsigned)chunks), block(256);
        if (mode == MOM_NONE) hipLaunchKernelGGL(lars_multi_kernel<MOM_NONE>, grid, block, 0, STRM(stream), tab, a);
        else if (mode == MOM_FIRST) hipLaunchKernelGGL(lars_multi_kernel<MOM_FIRST>, grid, block, 0, STRM(stream), tab, a);
        else hipLaunchKernelGGL(lars_multi_kernel<MOM_NEXT>, grid, block, 0, STRM(stream), tab, a);
        return check_launch(who);
    });
}

YOLO_API int yolo_lars_step(float *p, const float *g, float *buf, long n, const double *norms, int adapt, float lr, float momentum, float weight_decay,
                            float eta, float eps, int first_step, const double *norm_sq, float max_norm, void *p_bf16, const float *skip_flag,
                            yolo_stream_t stream)
{
    LarsArgs a;
    int mode;
    if (int rc = lars_args("yolo_lars_step", lr, momentum, weight_decay, eta, eps, first_step, norm_sq, max_norm, skip_flag, a, mode)) return rc;
    const yolo_lars_tensor t = {p, g, buf, p_bf16, norms, n, adapt};
    return lars_foreground("yolo_lars_step", &t, 1, a, mode, stream);
}

YOLO_API int yolo_lars_step_multi(const yolo_lars_tensor *t, int count, float lr, float momentum, float weight_decay, float eta, float eps,
                                  int first_step, const double *norm_sq, float max_norm, const float *skip_flag, yolo_stream_t stream)
{
    if (!t || count < 0) return fail(YOLO_E_ARG, "yolo_lars_step_multi: bad argument");
    LarsArgs a;
    int mode;
    if (int rc = lars_args("yolo_lars_step_multi", lr, momentum, weight_decay, eta, eps, first_step, norm_sq, max_norm, skip_flag, a, mode)) return rc;
    return lars_foreground("yolo_lars_step_multi", t, count, a, mode, stream);
}

YOLO_API int yolo_lars_step_multi_bg(const yolo_lars_tensor *t, int count, float lr, float momentum, float weight_decay, float eta, float eps,
                                     int first_step, const double *norm_sq, float max_norm, const float *skip_flag, int workgroups, yolo_stream_t stream)
{
    const char *who = "yolo_lars_step_multi_bg";
    LarsArgs a;
    int mode;
    if (int rc = lars_args(who, lr, momentum, weight_decay, eta, eps, first_step, norm_sq, max_norm, skip_flag, a, mode)) return rc;
    const void *fn = mode == MOM_NONE ? (const void *)lars_multi_bg_kernel<MOM_NONE>
                   : mode == MOM_FIRST ? (const void *)lars_multi_bg_kernel<MOM_FIRST> : (const void *)lars_multi_bg_kernel<MOM_NEXT>;
    static bool lds_done[3][64] = {};
    auto ok = [&](const char *w, const yolo_lars_tensor &e, int idx) { return lars_tensor_ok(w, e, idx, mode); };
    MtBackground<yolo_lars_tensor> bg;
    if (int rc = mt_background(who, t, count, workgroups, true, ok, fn, lds_done[mode], bg)) return rc;
    if (bg.grid == 0) return 0;
    const dim3 grid(bg.grid), block(1024);
    if (mode == MOM_NONE) hipLaunchKernelGGL(lars_multi_bg_kernel<MOM_NONE>, grid, block, BG_LDS, STRM(stream), bg.tab, bg.chunks, a);
    else if (mode == MOM_FIRST) hipLaunchKernelGGL(lars_multi_bg_kernel<MOM_FIRST>, grid, block, BG_LDS, STRM(stream), bg.tab, bg.chunks, a);
    else hipLaunchKernelGGL(lars_multi_bg_kernel<MOM_NEXT>, grid, block, BG_LDS, STRM(stream), bg.tab, bg.chunks, a);
    return check_launch(who);
}
