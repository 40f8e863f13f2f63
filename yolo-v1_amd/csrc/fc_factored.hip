// Factored gradient of a Linear layer for gfx950 (include/yolo_hip.h: yolo_fc_factors; tile code: fc_factored.h).
//   yolo_fc_factored_grad   G = scale * dy^T x stored as fp32 [O][I]: the gradient on request, and what the tests compare against.  The
//                           step entries (optim.hip: yolo_adam_step_factored, sgd.hip: yolo_sgd_step_factored) form the same bits and
//                           never store them.
//   yolo_adam_step_factored / yolo_sgd_step_factored: exported at the end of this file; their kernels in optim.hip / sgd.hip
//   yolo_fc_factored_sumsq  |G|^2 from the two rows x rows Gram matrices, A = dy dy^T over the O columns and B = x x^T over the I columns:
//                           |G|^2 = scale^2 sum_{n,m} A[n][m] B[n][m].  For the Gram matrices the batch axis is the MFMA's ROW and COLUMN
//                           and the factor's column its K: lane l takes eight consecutive columns of row l & 31 straight from memory,
//                           16 B, for both operands -- no LDS.  Three order-fixed stages (no atomics):
//                             part     one wave per (factor, 32 x 32 Gram tile, range of 256-column chunks): a chunk is 16 MFMAs in fp32
//                                      (chain YOLO_FC_GRAM_CHAIN), the chunks of the range are added in fp64; the tile is stored in the
//                                      accumulator's own (register, lane) order, the same for both factors
//                             combine  thread e adds the ranges of entry e in rising order for A and for B, multiplies, and a 256-thread
//                                      workgroup stores the sum of its products in a slot
//                             finish   one workgroup adds the slots in a fixed order, times scale^2, onto *acc
#include "fc_factored.h"

namespace yolo {

struct GradEpi {
    float *g;
    struct Elem {};
    __device__ __forceinline__ void load(long, Elem &) const {}
    __device__ __forceinline__ void finish(long idx, float gv, const Elem &) const { g[idx] = gv; }
};

__global__ void __launch_bounds__(256) fc_grad_kernel(const FcTiles f, float *__restrict__ g)
{
    fc_walk_tiles<1>(f, GradEpi{g});
}

constexpr int GRAM_CHUNK = YOLO_FC_GRAM_CHAIN;
constexpr long GRAM_WAVES = 1024;        // waves the part stage aims at per factor

struct GramPlan {
    const bf16_t *dy, *x;
    int rows, O, I, ld_dy, ld_x;
    int tr;                 // Gram tiles per side
    int T;                  // tr * tr
    int s_dy, cps_dy, s_x, cps_x;   // ranges per tile and chunks per range of each factor
};

// eight columns col .. col + 7 of row n, zero outside [0, rows) x [0, cols); col % 8 == 0
__device__ __forceinline__ fc_bf16x8 gram_load(const bf16_t *m, int ld, int rows, int cols, int n, int col)
{
    uint4 v = make_uint4(0u, 0u, 0u, 0u);
    if (n < rows && col < cols) {
        v = *reinterpret_cast<const uint4 *>(m + (long)n * ld + col);       // col + 8 <= ld: ld % 8 == 0 and col < cols <= ld
        const int left = cols - col;                                        // columns of this group inside the factor
        if (left < 8) {
            unsigned w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (2 * j >= left) w[j] = 0u;
                else if (2 * j + 1 >= left) w[j] &= 0xffffu;
            }
            v = make_uint4(w[0], w[1], w[2], w[3]);
        }
    }
    return __builtin_bit_cast(fc_bf16x8, v);
}

__global__ void __launch_bounds__(64) fc_gram_part_kernel(const GramPlan g, double *__restrict__ out)
{
    int u = blockIdx.x;
    const int units_dy = g.s_dy * g.T;
    const bool is_x = u >= units_dy;
    if (is_x) u -= units_dy;
    const bf16_t *m = is_x ? g.x : g.dy;
    const int ld = is_x ? g.ld_x : g.ld_dy, cols = is_x ? g.I : g.O, cps = is_x ? g.cps_x : g.cps_dy;
    const int s = u / g.T, tile = u % g.T;
    const int lane = threadIdx.x, r = lane & 31, h = lane >> 5;
    const int na = (tile / g.tr) * 32 + r, nb = (tile % g.tr) * 32 + r;
    const int nch = (cols + GRAM_CHUNK - 1) / GRAM_CHUNK;
    const int c_end = min(nch, (s + 1) * cps);
    double sum[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) sum[k] = 0.0;
    for (int c = s * cps; c < c_end; ++c) {
        const int col0 = c * GRAM_CHUNK + 8 * h;
        fc_f32x16 acc = {};
#pragma unroll 8
        for (int k = 0; k < GRAM_CHUNK; k += FC_KSTEP) {
            const fc_bf16x8 av = gram_load(m, ld, g.rows, cols, na, col0 + k);
            const fc_bf16x8 bv = gram_load(m, ld, g.rows, cols, nb, col0 + k);
            acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(av, bv, acc, 0, 0, 0);
        }
#pragma unroll
        for (int k = 0; k < 16; ++k) sum[k] += (double)acc[k];
    }
    double *dst = out + ((long)blockIdx.x * 16) * 64 + lane;      // blockIdx.x = (factor, range, tile): dy's ranges first
#pragma unroll
    for (int k = 0; k < 16; ++k) dst[k * 64] = sum[k];
}

__global__ void __launch_bounds__(256) fc_gram_combine_kernel(const double *__restrict__ part, int T, int s_dy, int s_x, double *__restrict__ slots)
{
    const long per = (long)T * 1024;                         // doubles of one range of one factor
    const long e = (long)blockIdx.x * 256 + threadIdx.x;     // < per: the grid is per / 256
    double a = 0.0, b = 0.0;
    for (int s = 0; s < s_dy; ++s) a += part[s * per + e];
    const double *px = part + s_dy * per;
    for (int s = 0; s < s_x; ++s) b += px[s * per + e];
    double v = a * b;
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    __shared__ double w[4];
    if ((threadIdx.x & 63) == 0) w[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) slots[blockIdx.x] = (w[0] + w[1]) + (w[2] + w[3]);
}

__global__ void __launch_bounds__(256) fc_gram_finish_kernel(const double *__restrict__ slots, int nslots, double scale_sq, double *__restrict__ acc)
{
    double s = 0.0;
    for (int i = threadIdx.x; i < nslots; i += 256) s += slots[i];
    __shared__ double red[256];
    red[threadIdx.x] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = red[0];
        for (int k = 1; k < 256; ++k) t += red[k];
        *acc = *acc + scale_sq * t;
    }
}

}  // namespace yolo

using namespace yolo;

YOLO_API int yolo_fc_factored_grad(const yolo_fc_factors *d, float *g_out, yolo_stream_t stream)
{
    const char *who = "yolo_fc_factored_grad";
    if (int rc = fc_check(who, d)) return rc;
    if (!g_out) return fail(YOLO_E_ARG, "%s: null output", who);
    if (fc_misaligned(g_out, 15)) return fail(YOLO_E_UNSUPPORTED, "%s: g_out must be 16-B aligned", who);
    static bool lds_done[64] = {};
    FcLaunch L;
    if (int rc = fc_prepare(who, d, 0, L)) return rc;
    if (int rc = fc_raise_lds(who, L, (const void *)fc_grad_kernel, lds_done)) return rc;
    hipLaunchKernelGGL(fc_grad_kernel, dim3(L.grid), dim3(256), L.lds, STRM(stream), L.f, g_out);
    return check_launch(who);
}

// ranges per Gram tile of a factor with `cols` columns: about GRAM_WAVES waves in all, a range a whole number of chunks
static void gram_split(int cols, int T, int &s, int &cps)
{
    const int nch = (cols + GRAM_CHUNK - 1) / GRAM_CHUNK;
    const long want = std::max<long>(1, GRAM_WAVES / T);
    cps = (int)((nch + want - 1) / want);
    s = (nch + cps - 1) / cps;
}

static GramPlan gram_plan(const yolo_fc_factors *d)
{
    GramPlan g;
    g.dy = (const bf16_t *)d->dy; g.x = (const bf16_t *)d->x;
    g.rows = d->rows; g.O = d->O; g.I = d->I; g.ld_dy = d->ld_dy; g.ld_x = d->ld_x;
    g.tr = (d->rows + 31) / 32;
    g.T = g.tr * g.tr;
    gram_split(d->O, g.T, g.s_dy, g.cps_dy);
    gram_split(d->I, g.T, g.s_x, g.cps_x);
    return g;
}

static long gram_doubles(const GramPlan &g) { return (long)(g.s_dy + g.s_x) * g.T * 1024 + (long)g.T * 4; }

YOLO_API int yolo_fc_factored_sumsq_slots(const yolo_fc_factors *d, long *doubles)
{
    const char *who = "yolo_fc_factored_sumsq_slots";
    if (!doubles) return fail(YOLO_E_ARG, "%s: null output", who);
    if (int rc = fc_check(who, d)) return rc;
    *doubles = gram_doubles(gram_plan(d));
    return 0;
}

YOLO_API int yolo_fc_factored_sumsq(const yolo_fc_factors *d, double *scratch, long scratch_doubles, double *acc, yolo_stream_t stream)
{
    const char *who = "yolo_fc_factored_sumsq";
    if (int rc = fc_check(who, d)) return rc;
    if (!acc || !scratch) return fail(YOLO_E_ARG, "%s: null scratch or accumulator", who);
    if (fc_misaligned(acc, 7) || fc_misaligned(scratch, 7)) return fail(YOLO_E_UNSUPPORTED, "%s: scratch and acc must be 8-B aligned", who);
    const GramPlan g = gram_plan(d);
    const long need = gram_doubles(g);
    if (scratch_doubles < need)
        return fail(YOLO_E_ARG, "%s: scratch holds %ld doubles, these factors need %ld (yolo_fc_factored_sumsq_slots)", who, scratch_doubles, need);
    const unsigned units = (unsigned)((g.s_dy + g.s_x) * g.T), nslots = (unsigned)g.T * 4;
    double *slots = scratch + (long)units * 1024;
    hipLaunchKernelGGL(fc_gram_part_kernel, dim3(units), dim3(64), 0, STRM(stream), g, scratch);
    if (int rc = check_launch(who)) return rc;
    hipLaunchKernelGGL(fc_gram_combine_kernel, dim3(nslots), dim3(256), 0, STRM(stream), (const double *)scratch, g.T, g.s_dy, g.s_x, slots);
    if (int rc = check_launch("yolo_fc_factored_sumsq (combine)")) return rc;
    hipLaunchKernelGGL(fc_gram_finish_kernel, dim3(1), dim3(256), 0, STRM(stream), (const double *)slots, (int)nslots, (double)d->scale * (double)d->scale, acc);
    return check_launch("yolo_fc_factored_sumsq (finish)");
}

// The step entries: the kernels stand beside the element ops they apply (optim.hip: AdamOp::one, sgd.hip: sgd1)
YOLO_API int yolo_adam_step_factored(const yolo_fc_factors *d, float *p, float *exp_avg, float *exp_avg_sq, void *p_bf16, float lr, float beta1, float beta2,
                                     float eps, float weight_decay, long step, const double *norm_sq, float max_norm, const float *skip_flag,
                                     int workgroups, yolo_stream_t stream)
{
    return adam_step_factored(d, p, exp_avg, exp_avg_sq, p_bf16, lr, beta1, beta2, eps, weight_decay, step, norm_sq, max_norm, skip_flag, workgroups, stream);
}

YOLO_API int yolo_sgd_step_factored(const yolo_fc_factors *d, float *p, float *buf, void *p_bf16, float lr, float momentum, float dampening,
                                    float weight_decay, int nesterov, int first_step, const double *norm_sq, float max_norm, const float *skip_flag,
                                    int workgroups, yolo_stream_t stream)
{
    return sgd_step_factored(d, p, buf, p_bf16, lr, momentum, dampening, weight_decay, nesterov, first_step, norm_sq, max_norm, skip_flag, workgroups, stream);
}
