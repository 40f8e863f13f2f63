// Order-fixed global gradient norm for gfx950 (EngineConfig.DETERMINISTIC): the same sum of squares as yolo_sumsq_f32 /
// yolo_sumsq_f32_multi (optim.hip), whose workgroups end in one fp64 atomicAdd each -- fp64 addition is not associative, so the
// double the optimizer kernels turn into the clip coefficient of EVERY parameter depended on the order in which the workgroups
// retired.  Here a workgroup owns one SQ_CHUNK-element slice of one tensor (the table and the workgroup sum of multi_tensor.h, as
// sumsq_multi_kernel) and STORES its fp64 partial in scratch slot blockIdx.x; a second one-workgroup kernel adds the slots in a fixed order
// (thread t: slots t, t + 256, .. in rising order; then the 256 thread sums in rising order) onto *acc.  No atomics; the result
// is a function of the inputs and the table alone.  HBM-bound like the original: one pass over the gradients + 8 B per 256 KB.
#include "multi_tensor.h"

#include <vector>

namespace yolo {

__global__ void __launch_bounds__(256) sumsq_fixed_part_kernel(const MtTable<SumsqTensor> tab, double *__restrict__ slots)
{
    long beg, end;
    const SumsqTensor &t = mt_slice<SQ_CHUNK>(tab, beg, end);
    wg_sumsq(t.g, beg + threadIdx.x * 4, end, 1024, [&](double s) { slots[blockIdx.x] = s; });
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

YOLO_API int yolo_sumsq_fixed_slots(const long *n, int count, long *slots)
{
    if (!n || !slots || count < 0) return fail(YOLO_E_ARG, "yolo_sumsq_fixed_slots: bad argument");
    long tot = 0;
    for (int i = 0; i < count; ++i) {
        if (n[i] < 0) return fail(YOLO_E_ARG, "yolo_sumsq_fixed_slots: tensor %d: negative size", i);
        tot += mt_chunks<SQ_CHUNK>(n[i]);
    }
    *slots = tot;
    return 0;
}

static int sumsq_tensor_ok(const char *who, const SumsqTensor &e, int idx)
{
    if (!e.g || e.n < 0) return fail(YOLO_E_ARG, "%s: tensor %d: null pointer or negative size", who, idx);
    if ((uintptr_t)e.g & 15) return fail(YOLO_E_UNSUPPORTED, "%s: tensor %d is not 16-B aligned", who, idx);
    return 0;
}

YOLO_API int yolo_sumsq_f32_multi_fixed(const float *const *g, const long *n, int count, double *scratch, long scratch_slots, double *acc, yolo_stream_t stream)
{
    const char *who = "yolo_sumsq_f32_multi_fixed";
    if (!g || !n || !acc || count < 0 || scratch_slots < 0) return fail(YOLO_E_ARG, "%s: bad argument", who);
    std::vector<SumsqTensor> t(count);
    long total = 0;
    for (int i = 0; i < count; ++i) {
        t[i] = {g[i], n[i]};
        total += n[i] < 0 ? 0 : mt_chunks<SQ_CHUNK>(n[i]);
    }
    if (int rc = mt_check<SQ_CHUNK>(who, t.data(), count, sumsq_tensor_ok)) return rc;
    if (total == 0) return 0;
    if (!scratch || ((uintptr_t)scratch & 7) || scratch_slots < total)
        return fail(YOLO_E_ARG, "%s: scratch holds %ld doubles, these tensors need %ld (yolo_sumsq_fixed_slots)", who, scratch_slots, total);
    return mt_launch<SQ_CHUNK>(t.data(), count, [&](const MtTable<SumsqTensor> &tab, long chunks) {
        // the launches of one call run one after the other on the stream: each reuses the scratch from slot 0
        hipLaunchKernelGGL(sumsq_fixed_part_kernel, dim3((unsigned)chunks), dim3(256), 0, STRM(stream), tab, scratch);
        if (int rc = check_launch(who)) return rc;
        hipLaunchKernelGGL(sumsq_fixed_finish_kernel, dim3(1), dim3(256), 0, STRM(stream), (const double *)scratch, (int)chunks, acc);
        return check_launch("yolo_sumsq_f32_multi_fixed (finish)");
    });
}

YOLO_API int yolo_sumsq_f32_fixed(const float *g, long n, double *scratch, long scratch_slots, double *acc, yolo_stream_t stream)
{
    if (!g || !acc || n < 0 || scratch_slots < 0) return fail(YOLO_E_ARG, "yolo_sumsq_f32_fixed: bad argument");
    if ((uintptr_t)g & 15) return fail(YOLO_E_UNSUPPORTED, "yolo_sumsq_f32_fixed: pointer must be 16-B aligned");
    return yolo_sumsq_f32_multi_fixed(&g, &n, 1, scratch, scratch_slots, acc, stream);
}
