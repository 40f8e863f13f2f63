// Order-fixed global gradient norm for gfx950 (EngineConfig.DETERMINISTIC): the same sum of squares as yolo_sumsq_f32 /
// yolo_sumsq_f32_multi (optim.hip), whose workgroups end in one fp64 atomicAdd each -- fp64 addition is not associative, so the
// double the optimizer kernels turn into the clip coefficient of EVERY parameter depended on the order in which the workgroups
// retired.  Here a workgroup owns one SQ_CHUNK-element slice of one tensor (the table layout and chunking of sumsq_multi_kernel)
// and STORES its fp64 partial in scratch slot blockIdx.x; a second one-workgroup kernel adds the slots in a fixed order
// (thread t: slots t, t + 256, .. in rising order; then the 256 thread sums in rising order) onto *acc.  No atomics; the result
// is a function of the inputs and the table alone.  HBM-bound like the original: one pass over the gradients + 8 B per 256 KB.
#include "optim_common.h"

namespace yolo {

constexpr int SQF_CHUNK = 65536;   // elements per workgroup (= SQ_CHUNK of optim.hip)

struct SumsqFixedTable {
    const float *g[YOLO_MT_MAX];
    long n[YOLO_MT_MAX];
    int first[YOLO_MT_MAX + 1];   // first chunk (= workgroup = scratch slot) of every tensor
    int count;
};

__global__ void __launch_bounds__(256) sumsq_fixed_part_kernel(const SumsqFixedTable tab, double *__restrict__ slots)
{
    const int ti = find_tensor(tab.first, tab.count, blockIdx.x);
    const float *__restrict__ g = tab.g[ti];
    const long n = tab.n[ti];
    const long beg = (long)(blockIdx.x - tab.first[ti]) * SQF_CHUNK;
    const long end = min(n, beg + SQF_CHUNK);
    double s = 0.0;
    for (long i = beg + threadIdx.x * 4; i < end; i += 1024) {
        if (i + 4 <= end) {
            const float4 v = *reinterpret_cast<const float4 *>(g + i);
            s += (double)(v.x * v.x + v.y * v.y) + (double)(v.z * v.z + v.w * v.w);
        } else {
            for (long k = i; k < end; ++k) s += (double)(g[k] * g[k]);
        }
    }
    for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off, 64);
    __shared__ double part[4];
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) slots[blockIdx.x] = part[0] + part[1] + part[2] + part[3];
}

__global__ void __launch_bounds__(256) sumsq_fixed_finish_kernel(const double *__restrict__ slots, int nslots, double *__restrict__ acc)
{
    double s = 0.0;
    for (int i = threadIdx.x; i < nslots; i += 256) s += slots[i];
    __shared__ double red[256];
    red[threadIdx.x] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = red[0];
        for (int k = 1; k < 256; ++k) t += red[k];
        *acc = *acc + t;
    }
}

}  // namespace yolo

using namespace yolo;

static long chunks_of(long n) { return (n + SQF_CHUNK - 1) / SQF_CHUNK; }

YOLO_API int yolo_sumsq_fixed_slots(const long *n, int count, long *slots)
{
    if (!n || !slots || count < 0) return fail(YOLO_E_ARG, "yolo_sumsq_fixed_slots: bad argument");
    long tot = 0;
    for (int i = 0; i < count; ++i) {
        if (n[i] < 0) return fail(YOLO_E_ARG, "yolo_sumsq_fixed_slots: tensor %d: negative size", i);
        tot += chunks_of(n[i]);
    }
    *slots = tot;
    return 0;
}

YOLO_API int yolo_sumsq_f32_multi_fixed(const float *const *g, const long *n, int count, double *scratch, long scratch_slots, double *acc, yolo_stream_t stream)
{
    if (!g || !n || !acc || count < 0 || scratch_slots < 0) return fail(YOLO_E_ARG, "yolo_sumsq_f32_multi_fixed: bad argument");
    // everything is checked before the first launch
    long total = 0;
    for (int i = 0; i < count; ++i) {
        if (!g[i] || n[i] < 0) return fail(YOLO_E_ARG, "yolo_sumsq_f32_multi_fixed: tensor %d: null pointer or negative size", i);
        if ((uintptr_t)g[i] & 15) return fail(YOLO_E_UNSUPPORTED, "yolo_sumsq_f32_multi_fixed: tensor %d is not 16-B aligned", i);
        if (chunks_of(n[i]) > 0x7fffffffL) return fail(YOLO_E_UNSUPPORTED, "yolo_sumsq_f32_multi_fixed: tensor %d is too large", i);
        total += chunks_of(n[i]);
    }
    if (total == 0) return 0;
    if (!scratch || ((uintptr_t)scratch & 7) || scratch_slots < total)
        return fail(YOLO_E_ARG, "yolo_sumsq_f32_multi_fixed: scratch holds %ld doubles, these tensors need %ld (yolo_sumsq_fixed_slots)", scratch_slots, total);
    for (int base = 0; base < count;) {
        SumsqFixedTable tab{};
        long chunks = 0;
        int k = 0;
        for (; base + k < count && k < YOLO_MT_MAX; ++k) {
            const long c = chunks_of(n[base + k]);
            if (chunks + c > 0x7fffffffL) break;
            tab.g[k] = g[base + k]; tab.n[k] = n[base + k]; tab.first[k] = (int)chunks;
            chunks += c;
        }
        tab.first[k] = (int)chunks;
        tab.count = k;
        if (chunks > 0) {
            // the launches of one call run one after the other on the stream: each reuses the scratch from slot 0
            hipLaunchKernelGGL(sumsq_fixed_part_kernel, dim3((unsigned)chunks), dim3(256), 0, STRM(stream), tab, scratch);
            if (int rc = check_launch("yolo_sumsq_f32_multi_fixed")) return rc;
            hipLaunchKernelGGL(sumsq_fixed_finish_kernel, dim3(1), dim3(256), 0, STRM(stream), (const double *)scratch, (int)chunks, acc);
            if (int rc = check_launch("yolo_sumsq_f32_multi_fixed (finish)")) return rc;
        }
        base += k;
    }
    return 0;
}

YOLO_API int yolo_sumsq_f32_fixed(const float *g, long n, double *scratch, long scratch_slots, double *acc, yolo_stream_t stream)
{
    if (!g || !acc || n < 0 || scratch_slots < 0) return fail(YOLO_E_ARG, "yolo_sumsq_f32_fixed: bad argument");
    if ((uintptr_t)g & 15) return fail(YOLO_E_UNSUPPORTED, "yolo_sumsq_f32_fixed: pointer must be 16-B aligned");
    return yolo_sumsq_f32_multi_fixed(&g, &n, 1, scratch, scratch_slots, acc, stream);
}
