// Fused optimizer step for gfx950 (HBM-bound, one pass over the 271.7 M fp32 parameters):
// global-gradient-norm clipping + Adam with L2 weight decay, i.e. what the reference's train step
// does with torch.nn.utils.clip_grad_norm_(max_norm=10) followed by optim.Adam(lr, weight_decay)
// (src/yolo/training/trainer.py:79-95, src/train.py:177-179) in ~10 separate multi-tensor passes.
//   yolo_sumsq_f32 : accumulates sum(g^2) of one tensor into a device double (fp64 atomics)
//   yolo_adam_step : g' = g * clip + wd * p ; m,v update ; p -= lr/bc1 * m / (sqrt(v)/sqrt(bc2) + eps)
//                    clip = min(1, max_norm / (sqrt(norm_sq) + 1e-6)) is read from device memory, so the
//                    whole step needs no host synchronisation.  Optionally also writes bf16(p) (the
//                    forward operand of Linear layers has the master's layout).
// 16 B per lane on every stream (float4), grid-stride, <= 2048 workgroups.
//
// Multi-tensor forms (yolo_sumsq_f32_multi, yolo_adam_step_multi): the model has 52 parameter tensors,
// 48 of them small; one launch per tensor leaves most of the chip idle for most of the step.  The
// per-tensor table travels in the kernel arguments (<= YOLO_MT_MAX entries per launch), a workgroup
// owns one MT_CHUNK-element slice of one tensor and finds it by scanning the table's chunk prefix.
#include "fc_factored.h"
#include "multi_tensor.h"

#include <cmath>
#include <vector>

namespace yolo {

__global__ void __launch_bounds__(256) sumsq_kernel(const float *__restrict__ g, long n, double *__restrict__ acc)
{
    wg_sumsq(g, ((long)blockIdx.x * blockDim.x + threadIdx.x) * 4, n, (long)gridDim.x * blockDim.x * 4, [&](double s) { atomicAdd(acc, s); });
}

__device__ __forceinline__ void adam1(float &p, float g, float &m, float &v, float clip, float wd, float b1, float b2, float step_size, float inv_bc2_sqrt, float eps)
{
    g = g * clip;
    g = g + wd * p;                       // grad.add(param, alpha=weight_decay)
    m = m + (g - m) * (1.0f - b1);        // exp_avg.lerp_(grad, 1 - beta1)
    v = v * b2 + (1.0f - b2) * g * g;     // exp_avg_sq.mul_(beta2).addcmul_(grad, grad, value=1-beta2)
    const float denom = sqrtf(v) * inv_bc2_sqrt + eps;
    p = p - step_size * (m / denom);      // param.addcdiv_(exp_avg, denom, value=-step_size)
}

// The element op of the three Adam kernels.  They leave contraction to the compiler and may differ in the last bit between forms.
struct AdamOp {
    float clip, wd, b1, b2, step_size, inv_bc2_sqrt, eps;
    struct Vals {
        float4 p[2], g[2], m[2], v[2];
    };
    __device__ __forceinline__ void one(float &p, float g, float &m, float &v) const { adam1(p, g, m, v, clip, wd, b1, b2, step_size, inv_bc2_sqrt, eps); }
    // one float4 of every array, already in registers: update, store at element i
    __device__ __forceinline__ void vec(const yolo_adam_tensor &t, long i, float4 &pv, const float4 &gv, float4 &mv, float4 &vv) const
    {
        one(pv.x, gv.x, mv.x, vv.x);
        one(pv.y, gv.y, mv.y, vv.y);
        one(pv.z, gv.z, mv.z, vv.z);
        one(pv.w, gv.w, mv.w, vv.w);
        *reinterpret_cast<float4 *>(t.p + i) = pv;
        *reinterpret_cast<float4 *>(t.m + i) = mv;
        *reinterpret_cast<float4 *>(t.v + i) = vv;
        if (t.p_bf16) *reinterpret_cast<uint2 *>((bf16_t *)t.p_bf16 + i) = pack_bf16x4(pv);
    }
    __device__ __forceinline__ void load(const yolo_adam_tensor &t, long i, int u, Vals &x) const
    {
        x.p[u] = *reinterpret_cast<const float4 *>(t.p + i);
        x.g[u] = *reinterpret_cast<const float4 *>(t.g + i);
        x.m[u] = *reinterpret_cast<const float4 *>(t.m + i);
        x.v[u] = *reinterpret_cast<const float4 *>(t.v + i);
    }
    __device__ __forceinline__ void full(const yolo_adam_tensor &t, long i, int u, Vals &x) const { vec(t, i, x.p[u], x.g[u], x.m[u], x.v[u]); }
    __device__ __forceinline__ void tail(const yolo_adam_tensor &t, long k0, long end, long step) const
    {
        bf16_t *pb = (bf16_t *)t.p_bf16;
        for (long k = k0; k < end; k += step) {
            float pk = t.p[k], mk = t.m[k], vk = t.v[k];
            one(pk, t.g[k], mk, vk);
            t.p[k] = pk; t.m[k] = mk; t.v[k] = vk;
            if (pb) pb[k] = f32_to_bf16(pk);
        }
    }
    // the float4 groups i0, i0 + stride, .. < end of one tensor, and the 1-3 elements behind the last whole one
    __device__ __forceinline__ void span(const yolo_adam_tensor &t, long i0, long end, long stride) const
    {
        for (long i = i0; i < end; i += stride) {
            if (i + 4 <= end) {
                float4 pv = *reinterpret_cast<float4 *>(t.p + i);
                const float4 gv = *reinterpret_cast<const float4 *>(t.g + i);
                float4 mv = *reinterpret_cast<float4 *>(t.m + i), vv = *reinterpret_cast<float4 *>(t.v + i);
                vec(t, i, pv, gv, mv, vv);
            } else {
                tail(t, i, end, 1);
            }
        }
    }
};

__global__ void __launch_bounds__(256) adam_kernel(float *__restrict__ p, const float *__restrict__ g, float *__restrict__ m, float *__restrict__ v, long n,
                                                   float b1, float b2, float eps, float wd, float step_size, float inv_bc2_sqrt,
                                                   const double *__restrict__ norm_sq, float max_norm, bf16_t *__restrict__ pb)
{
    const AdamOp op{clip_coefficient(norm_sq, max_norm), wd, b1, b2, step_size, inv_bc2_sqrt, eps};
    const yolo_adam_tensor t = {p, g, m, v, pb, n};
    op.span(t, ((long)blockIdx.x * blockDim.x + threadIdx.x) * 4, n, (long)gridDim.x * blockDim.x * 4);
}

__global__ void __launch_bounds__(256) sumsq_multi_kernel(const MtTable<SumsqTensor> tab, double *__restrict__ acc)
{
    long beg, end;
    const SumsqTensor &t = mt_slice<SQ_CHUNK>(tab, beg, end);
    wg_sumsq(t.g, beg + threadIdx.x * 4, end, 1024, [&](double s) { atomicAdd(acc, s); });
}

__global__ void __launch_bounds__(256) adam_multi_kernel(const MtTable<yolo_adam_tensor> tab, float b1, float b2, float eps, float wd, float step_size, float inv_bc2_sqrt,
                                                         const double *__restrict__ norm_sq, float max_norm, const float *__restrict__ skip_flag)
{
    if (mt_skipped(skip_flag)) return;
    const AdamOp op{clip_coefficient(norm_sq, max_norm), wd, b1, b2, step_size, inv_bc2_sqrt, eps};
    long beg, end;
    const yolo_adam_tensor t = mt_slice<MT_CHUNK>(tab, beg, end);      // a copy: the pointers are read from the kernel arguments once, in front of the loop
    op.span(t, beg + threadIdx.x * 4, end, 1024);
}

// Background form (yolo_adam_step_multi_bg): mt_walk_bg.  Four float4 per array and thread are in flight: ~190 KB per CU, what
// ~100 GB/s per CU needs at HBM latency.
__global__ void __launch_bounds__(1024) adam_multi_bg_kernel(const MtTable<yolo_adam_tensor> tab, int chunks, float b1, float b2, float eps, float wd, float step_size,
                                                             float inv_bc2_sqrt, const double *__restrict__ norm_sq, float max_norm,
                                                             const float *__restrict__ skip_flag)
{
    if (mt_skipped(skip_flag)) return;
    mt_walk_bg(tab, chunks, AdamOp{clip_coefficient(norm_sq, max_norm), wd, b1, b2, step_size, inv_bc2_sqrt, eps});
}

// yolo_adam_step_factored: the gradient of one [O][I] parameter arrives as its two batch factors (fc_factored.h); a lane applies AdamOp::one to
// the 16 weights of its accumulator registers
struct AdamFcEpi {
    AdamOp op;
    float *p, *m, *v;
    bf16_t *pb;
    struct Elem {
        float p, m, v;
    };
    __device__ __forceinline__ void load(long i, Elem &e) const { e.p = p[i]; e.m = m[i]; e.v = v[i]; }
    __device__ __forceinline__ void finish(long i, float g, Elem &e) const
    {
        op.one(e.p, g, e.m, e.v);
        p[i] = e.p; m[i] = e.m; v[i] = e.v;
        if (pb) pb[i] = f32_to_bf16(e.p);
    }
};

template <int TEAMS>
__global__ void __launch_bounds__(256 * TEAMS) adam_fc_kernel(const FcTiles f, float *p, float *m, float *v, bf16_t *pb, float b1, float b2, float eps, float wd,
                                                      float step_size, float inv_bc2_sqrt, const double *__restrict__ norm_sq, float max_norm,
                                                      const float *__restrict__ skip_flag)
{
    if (mt_skipped(skip_flag)) return;
    fc_walk_tiles<TEAMS>(f, AdamFcEpi{AdamOp{clip_coefficient(norm_sq, max_norm), wd, b1, b2, step_size, inv_bc2_sqrt, eps}, p, m, v, pb});
}

__global__ void scale_by_clip_kernel(float *__restrict__ g, long n, const double *__restrict__ norm_sq, float max_norm)
{
    const float c = clip_ratio(norm_sq, max_norm);
    if (c >= 1.0f) return;
    const long stride = (long)gridDim.x * blockDim.x;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) g[i] *= c;
}

}  // namespace yolo

using namespace yolo;

// bias corrections of `step`, formed in double
struct AdamScalars {
    float step_size, inv_bc2_sqrt;
    AdamScalars(float lr, float beta1, float beta2, long step)
    {
        const double bc1 = 1.0 - pow((double)beta1, (double)step), bc2 = 1.0 - pow((double)beta2, (double)step);
        step_size = (float)((double)lr / bc1);
        inv_bc2_sqrt = (float)(1.0 / sqrt(bc2));
    }
};

static inline unsigned grid_for(long n, int per_thread)
{
    long b = (n + 256L * per_thread - 1) / (256L * per_thread);
    if (b > 2048) b = 2048;
    if (b < 1) b = 1;
    return (unsigned)b;
}

YOLO_API int yolo_sumsq_f32(const float *g, long n, double *acc, yolo_stream_t stream)
{
    if (!g || !acc || n < 0) return fail(YOLO_E_ARG, "yolo_sumsq_f32: bad argument");
    if (n == 0) return 0;
    if ((uintptr_t)g & 15) return fail(YOLO_E_UNSUPPORTED, "yolo_sumsq_f32: pointer must be 16-B aligned");
    hipLaunchKernelGGL(sumsq_kernel, dim3(grid_for(n, 16)), dim3(256), 0, STRM(stream), g, n, acc);
    return check_launch("yolo_sumsq_f32");
}

YOLO_API int yolo_adam_step(float *p, const float *g, float *m, float *v, long n, float lr, float beta1, float beta2, float eps, float weight_decay,
                            long step, const double *norm_sq, float max_norm, void *p_bf16, yolo_stream_t stream)
{
    if (!p || !g || !m || !v || n < 0 || step < 1) return fail(YOLO_E_ARG, "yolo_adam_step: bad argument");
    if (n == 0) return 0;
    if (((uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v) & 15) return fail(YOLO_E_UNSUPPORTED, "yolo_adam_step: pointers must be 16-B aligned");
    if ((uintptr_t)p_bf16 & 7) return fail(YOLO_E_UNSUPPORTED, "yolo_adam_step: bf16 shadow is not 8-B aligned");   // 8-B stores, as the multi-tensor entries
    const AdamScalars a(lr, beta1, beta2, step);
    hipLaunchKernelGGL(adam_kernel, dim3(grid_for(n, 8)), dim3(256), 0, STRM(stream), p, g, m, v, n, beta1, beta2, eps, weight_decay, a.step_size, a.inv_bc2_sqrt,
                       norm_sq, max_norm, (bf16_t *)p_bf16);
    return check_launch("yolo_adam_step");
}

static int sumsq_tensor_ok(const char *who, const SumsqTensor &e, int idx)
{
    if (!e.g || e.n < 0) return fail(YOLO_E_ARG, "%s: tensor %d: null pointer or negative size", who, idx);
    if ((uintptr_t)e.g & 15) return fail(YOLO_E_UNSUPPORTED, "%s: tensor %d is not 16-B aligned", who, idx);
    return 0;
}

YOLO_API int yolo_sumsq_f32_multi(const float *const *g, const long *n, int count, double *acc, yolo_stream_t stream)
{
    const char *who = "yolo_sumsq_f32_multi";
    if (!g || !n || !acc || count < 0) return fail(YOLO_E_ARG, "%s: bad argument", who);
    std::vector<SumsqTensor> t(count);
    for (int i = 0; i < count; ++i) t[i] = {g[i], n[i]};
    return mt_foreground<SQ_CHUNK>(who, t.data(), count, sumsq_tensor_ok, [&](const MtTable<SumsqTensor> &tab, long chunks) {
        hipLaunchKernelGGL(sumsq_multi_kernel, dim3((unsigned)chunks), dim3(256), 0, STRM(stream), tab, acc);
        return check_launch(who);
    });
}

static int adam_tensor_ok(const char *who, const yolo_adam_tensor &e, int idx)
{
    if (!e.p || !e.g || !e.m || !e.v || e.n < 0) return fail(YOLO_E_ARG, "%s: tensor %d: null pointer or negative size", who, idx);
    if (((uintptr_t)e.p | (uintptr_t)e.g | (uintptr_t)e.m | (uintptr_t)e.v) & 15) return fail(YOLO_E_UNSUPPORTED, "%s: tensor %d is not 16-B aligned", who, idx);
    if ((uintptr_t)e.p_bf16 & 7) return fail(YOLO_E_UNSUPPORTED, "%s: bf16 shadow %d is not 8-B aligned", who, idx);
    return 0;
}

YOLO_API int yolo_adam_step_multi(const yolo_adam_tensor *t, int count, float lr, float beta1, float beta2, float eps, float weight_decay, long step,
                                  const double *norm_sq, float max_norm, const float *skip_flag, yolo_stream_t stream)
{
    const char *who = "yolo_adam_step_multi";
    if (!t || count < 0 || step < 1) return fail(YOLO_E_ARG, "%s: bad argument", who);
    const AdamScalars a(lr, beta1, beta2, step);
    return mt_foreground<MT_CHUNK>(who, t, count, adam_tensor_ok, [&](const MtTable<yolo_adam_tensor> &tab, long chunks) {
        hipLaunchKernelGGL(adam_multi_kernel, dim3((unsigned)chunks), dim3(256), 0, STRM(stream), tab, beta1, beta2, eps, weight_decay, a.step_size,
                           a.inv_bc2_sqrt, norm_sq, max_norm, skip_flag);
        return check_launch(who);
    });
}

YOLO_API int yolo_adam_step_multi_bg(const yolo_adam_tensor *t, int count, float lr, float beta1, float beta2, float eps, float weight_decay, long step,
                                     const double *norm_sq, float max_norm, const float *skip_flag, int workgroups, yolo_stream_t stream)
{
    const char *who = "yolo_adam_step_multi_bg";
    static bool lds_done[64] = {};
    MtBackground<yolo_adam_tensor> bg;
    if (int rc = mt_background(who, t, count, workgroups, step >= 1, adam_tensor_ok, (const void *)adam_multi_bg_kernel, lds_done, bg)) return rc;
    if (bg.grid == 0) return 0;
    const AdamScalars a(lr, beta1, beta2, step);
    hipLaunchKernelGGL(adam_multi_bg_kernel, dim3(bg.grid), dim3(1024), BG_LDS, STRM(stream), bg.tab, bg.chunks, beta1, beta2, eps, weight_decay, a.step_size,
                       a.inv_bc2_sqrt, norm_sq, max_norm, skip_flag);
    return check_launch(who);
}

// yolo_adam_step_factored (the entry stands with the other factored entries in fc_factored.hip; the kernel needs AdamOp)
int yolo::adam_step_factored(const yolo_fc_factors *d, float *p, float *m, float *v, void *p_bf16, float lr, float beta1, float beta2, float eps,
                             float weight_decay, long step, const double *norm_sq, float max_norm, const float *skip_flag, int workgroups,
                             yolo_stream_t stream)
{
    const char *who = "yolo_adam_step_factored";
    if (int rc = fc_check(who, d)) return rc;
    if (!p || !m || !v || step < 1) return fail(YOLO_E_ARG, "%s: null pointer or step < 1", who);
    if (fc_misaligned(p, 15) || fc_misaligned(m, 15) || fc_misaligned(v, 15)) return fail(YOLO_E_UNSUPPORTED, "%s: p, exp_avg and exp_avg_sq must be 16-B aligned", who);
    if (fc_misaligned(p_bf16, 7)) return fail(YOLO_E_UNSUPPORTED, "%s: bf16 shadow is not 8-B aligned", who);
    if (fc_misaligned(norm_sq, 7)) return fail(YOLO_E_UNSUPPORTED, "%s: norm_sq is not 8-B aligned", who);
    static bool lds_done[3][64] = {};
    FcLaunch L;
    if (int rc = fc_prepare(who, d, workgroups, L)) return rc;
    const AdamScalars a(lr, beta1, beta2, step);
    auto launch = [&](auto kernel, bool (&done)[64]) {
        if (int rc = fc_raise_lds(who, L, (const void *)kernel, done)) return rc;
        hipLaunchKernelGGL(kernel, dim3(L.grid), dim3(256 * L.teams), L.lds, STRM(stream), L.f, p, m, v, (bf16_t *)p_bf16, beta1, beta2, eps, weight_decay,
                           a.step_size, a.inv_bc2_sqrt, norm_sq, max_norm, skip_flag);
        return check_launch(who);
    };
    return L.teams == 4 ? launch(adam_fc_kernel<4>, lds_done[2]) : L.teams == 2 ? launch(adam_fc_kernel<2>, lds_done[1]) : launch(adam_fc_kernel<1>, lds_done[0]);
}

YOLO_API int yolo_clip_scale_f32(float *g, long n, const double *norm_sq, float max_norm, yolo_stream_t stream)
{
    if (!g || !norm_sq || n < 0) return fail(YOLO_E_ARG, "yolo_clip_scale_f32: bad argument");
    if (n == 0) return 0;
    hipLaunchKernelGGL(scale_by_clip_kernel, dim3(grid_for(n, 4)), dim3(256), 0, STRM(stream), g, n, norm_sq, max_norm);
    return check_launch("yolo_clip_scale_f32");
}
