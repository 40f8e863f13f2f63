// Fused SGD step for gfx950, next to the Adam pass of optim.hip: global-gradient-norm clipping + torch.optim.SGD (momentum, dampening,
// L2 weight decay, Nesterov; maximize=False) in one HBM pass -- the YOLOv1 paper's recipe on the reference's train step
// (src/yolo/training/trainer.py:79-95: clip_grad_norm_(max_norm=10), optimizer.step()).  Per element, in fp32:
//   g = grad * clip ; g += wd * p ; buf = first_step ? g : momentum * buf + (1 - dampening) * g ; g = nesterov ? g + momentum * buf : buf ;
//   p -= lr * g ; p_bf16 = bf16(p)
// One state tensor where Adam keeps two: 22 B per element with the bf16 shadow (read p, g, buf; write p, buf, shadow) against 30 B,
// 18 B on the first step (buf is only written), 12 B without momentum (buf is not touched).
// Same launch shapes as the Adam entries: a workgroup owns one MT_CHUNK slice of one tensor of the table in the kernel arguments
// (yolo_sgd_step, yolo_sgd_step_multi), or `workgroups` persistent 1024-thread workgroups walk the chunk list (yolo_sgd_step_multi_bg).
#include "fc_factored.h"
#include "multi_tensor.h"

namespace yolo {

enum { MOM_NONE = 0, MOM_FIRST = 1, MOM_NEXT = 2 };   // no momentum (buf untouched) / buf = g (written only) / buf = momentum * buf + omd * g

struct SgdArgs {
    float lr, momentum, omd, wd;      // omd = 1 - dampening
    int nesterov;
    const double *norm_sq;
    float max_norm;
    const float *skip_flag;
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

// The element op of both SGD kernels (multi_tensor.h: mt_walk_bg)
template <int MODE>
struct SgdOp {
    float clip;
    const SgdArgs &a;
    struct Vals {
        float4 p[2], g[2], b[2];
    };
    // one float4 of every array, already in registers: update, store at element i
    __device__ __forceinline__ void vec(const yolo_sgd_tensor &t, long i, float4 &p, const float4 &g, float4 &b) const
    {
        sgd1<MODE>(p.x, g.x, b.x, clip, a);
        sgd1<MODE>(p.y, g.y, b.y, clip, a);
        sgd1<MODE>(p.z, g.z, b.z, clip, a);
        sgd1<MODE>(p.w, g.w, b.w, clip, a);
        *reinterpret_cast<float4 *>(t.p + i) = p;
        if (MODE != MOM_NONE) *reinterpret_cast<float4 *>(t.buf + i) = b;
        if (t.p_bf16) *reinterpret_cast<uint2 *>((bf16_t *)t.p_bf16 + i) = pack_bf16x4(p);
    }
    __device__ __forceinline__ void load(const yolo_sgd_tensor &t, long i, int u, Vals &x) const
    {
        x.p[u] = *reinterpret_cast<const float4 *>(t.p + i);
        x.g[u] = *reinterpret_cast<const float4 *>(t.g + i);
        if (MODE == MOM_NEXT) x.b[u] = *reinterpret_cast<const float4 *>(t.buf + i);
    }
    __device__ __forceinline__ void full(const yolo_sgd_tensor &t, long i, int u, Vals &x) const { vec(t, i, x.p[u], x.g[u], x.b[u]); }
    __device__ __forceinline__ void tail(const yolo_sgd_tensor &t, long k0, long end, long step) const
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
};

template <int MODE>
__global__ void __launch_bounds__(256) sgd_multi_kernel(const MtTable<yolo_sgd_tensor> tab, const SgdArgs a)
{
    if (mt_skipped(a.skip_flag)) return;
    const SgdOp<MODE> op{clip_coefficient(a.norm_sq, a.max_norm), a};
    long beg, end;
    const yolo_sgd_tensor &t = mt_slice<MT_CHUNK>(tab, beg, end);
    for (long i = beg + threadIdx.x * 4; i < end; i += 1024) {
        if (i + 4 <= end) {
            float4 pv = *reinterpret_cast<const float4 *>(t.p + i);
            const float4 gv = *reinterpret_cast<const float4 *>(t.g + i);
            float4 bv = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            if (MODE == MOM_NEXT) bv = *reinterpret_cast<const float4 *>(t.buf + i);
            op.vec(t, i, pv, gv, bv);
        } else {
            op.tail(t, i, end, 1);
        }
    }
}

template <int MODE>
__global__ void __launch_bounds__(1024) sgd_multi_bg_kernel(const MtTable<yolo_sgd_tensor> tab, int chunks, const SgdArgs a)
{
    if (mt_skipped(a.skip_flag)) return;
    mt_walk_bg(tab, chunks, SgdOp<MODE>{clip_coefficient(a.norm_sq, a.max_norm), a});
}

// yolo_sgd_step_factored: the gradient of one [O][I] parameter arrives as its two batch factors (fc_factored.h); a lane applies sgd1 to the 16
// weights of its accumulator registers
template <int MODE>
struct SgdFcEpi {
    float clip;
    const SgdArgs &a;
    float *p, *buf;
    bf16_t *pb;
    struct Elem {
        float p, b;
    };
    __device__ __forceinline__ void load(long i, Elem &e) const
    {
        e.p = p[i];
        e.b = MODE == MOM_NEXT ? buf[i] : 0.0f;
    }
    __device__ __forceinline__ void finish(long i, float g, Elem &e) const
    {
        sgd1<MODE>(e.p, g, e.b, clip, a);
        p[i] = e.p;
        if (MODE != MOM_NONE) buf[i] = e.b;
        if (pb) pb[i] = f32_to_bf16(e.p);
    }
};

template <int MODE, int TEAMS>
__global__ void __launch_bounds__(256 * TEAMS) sgd_fc_kernel(const FcTiles f, float *p, float *buf, bf16_t *pb, const SgdArgs a)
{
    if (mt_skipped(a.skip_flag)) return;
    fc_walk_tiles<TEAMS>(f, SgdFcEpi<MODE>{clip_coefficient(a.norm_sq, a.max_norm), a, p, buf, pb});
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

static int sgd_foreground(const char *who, const yolo_sgd_tensor *t, int count, const SgdArgs &a, int mode, yolo_stream_t stream)
{
    auto ok = [&](const char *w, const yolo_sgd_tensor &e, int idx) { return sgd_tensor_ok(w, e, idx, mode); };
    return mt_foreground<MT_CHUNK>(who, t, count, ok, [&](const MtTable<yolo_sgd_tensor> &tab, long chunks) {
        const dim3 grid((unsigned)chunks), block(256);
        if (mode == MOM_NONE) hipLaunchKernelGGL(sgd_multi_kernel<MOM_NONE>, grid, block, 0, STRM(stream), tab, a);
        else if (mode == MOM_FIRST) hipLaunchKernelGGL(sgd_multi_kernel<MOM_FIRST>, grid, block, 0, STRM(stream), tab, a);
        else hipLaunchKernelGGL(sgd_multi_kernel<MOM_NEXT>, grid, block, 0, STRM(stream), tab, a);
        return check_launch(who);
    });
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
    SgdArgs a;
    int mode;
    if (int rc = sgd_args(who, lr, momentum, dampening, weight_decay, nesterov, first_step, norm_sq, max_norm, skip_flag, a, mode)) return rc;
    const void *fn = mode == MOM_NONE ? (const void *)sgd_multi_bg_kernel<MOM_NONE>
                   : mode == MOM_FIRST ? (const void *)sgd_multi_bg_kernel<MOM_FIRST> : (const void *)sgd_multi_bg_kernel<MOM_NEXT>;
    static bool lds_done[3][64] = {};
    auto ok = [&](const char *w, const yolo_sgd_tensor &e, int idx) { return sgd_tensor_ok(w, e, idx, mode); };
    MtBackground<yolo_sgd_tensor> bg;
    if (int rc = mt_background(who, t, count, workgroups, true, ok, fn, lds_done[mode], bg)) return rc;
    if (bg.grid == 0) return 0;
    const dim3 grid(bg.grid), block(1024);
    if (mode == MOM_NONE) hipLaunchKernelGGL(sgd_multi_bg_kernel<MOM_NONE>, grid, block, BG_LDS, STRM(stream), bg.tab, bg.chunks, a);
    else if (mode == MOM_FIRST) hipLaunchKernelGGL(sgd_multi_bg_kernel<MOM_FIRST>, grid, block, BG_LDS, STRM(stream), bg.tab, bg.chunks, a);
    else hipLaunchKernelGGL(sgd_multi_bg_kernel<MOM_NEXT>, grid, block, BG_LDS, STRM(stream), bg.tab, bg.chunks, a);
    return check_launch(who);
}

// yolo_sgd_step_factored (the entry stands with the other factored entries in fc_factored.hip; the kernel needs sgd1)
int yolo::sgd_step_factored(const yolo_fc_factors *d, float *p, float *buf, void *p_bf16, float lr, float momentum, float dampening, float weight_decay,
                            int nesterov, int first_step, const double *norm_sq, float max_norm, const float *skip_flag, int workgroups,
                            yolo_stream_t stream)
{
    const char *who = "yolo_sgd_step_factored";
    if (int rc = fc_check(who, d)) return rc;
    SgdArgs a;
    int mode;
    if (int rc = sgd_args(who, lr, momentum, dampening, weight_decay, nesterov, first_step, norm_sq, max_norm, skip_flag, a, mode)) return rc;
    if (!p || (mode != MOM_NONE && !buf)) return fail(YOLO_E_ARG, "%s: null pointer", who);
    if (fc_misaligned(p, 15) || (mode != MOM_NONE && fc_misaligned(buf, 15))) return fail(YOLO_E_UNSUPPORTED, "%s: p and buf must be 16-B aligned", who);
    if (fc_misaligned(p_bf16, 7)) return fail(YOLO_E_UNSUPPORTED, "%s: bf16 shadow is not 8-B aligned", who);
    if (fc_misaligned(norm_sq, 7)) return fail(YOLO_E_UNSUPPORTED, "%s: norm_sq is not 8-B aligned", who);
    FcLaunch L;
    if (int rc = fc_prepare(who, d, workgroups, L)) return rc;
    bf16_t *pb = (bf16_t *)p_bf16;
    static bool lds_done[3][3][64] = {};
    auto launch = [&](auto kernel, bool (&done)[64]) {
        if (int rc = fc_raise_lds(who, L, (const void *)kernel, done)) return rc;
        hipLaunchKernelGGL(kernel, dim3(L.grid), dim3(256 * L.teams), L.lds, STRM(stream), L.f, p, buf, pb, a);
        return check_launch(who);
    };
    auto teams = [&](auto k1, auto k2, auto k4) {
        return L.teams == 4 ? launch(k4, lds_done[mode][2]) : L.teams == 2 ? launch(k2, lds_done[mode][1]) : launch(k1, lds_done[mode][0]);
    };
    if (mode == MOM_NONE) return teams(sgd_fc_kernel<MOM_NONE, 1>, sgd_fc_kernel<MOM_NONE, 2>, sgd_fc_kernel<MOM_NONE, 4>);
    if (mode == MOM_FIRST) return teams(sgd_fc_kernel<MOM_FIRST, 1>, sgd_fc_kernel<MOM_FIRST, 2>, sgd_fc_kernel<MOM_FIRST, 4>);
    return teams(sgd_fc_kernel<MOM_NEXT, 1>, sgd_fc_kernel<MOM_NEXT, 2>, sgd_fc_kernel<MOM_NEXT, 4>);
}
