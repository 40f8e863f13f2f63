// The multi-tensor HBM passes (optim.hip: Adam and the atomic norm, sgd.hip, ema.hip, accum.hip, norm_fixed.hip) in one place: the table
// that travels in the kernel arguments, the slice a foreground workgroup owns, the persistent double-buffered walk of the background
// forms, the clip coefficient / skip flag / bf16 pack / sum of squares every pass states the same way, and on the host the one loop that
// checks a whole call, fills tables YOLO_MT_MAX tensors at a time and launches.  A new pass writes its element op and a ten-line kernel:
//   foreground: __global__ k(const MtTable<T> tab, ..) { if (mt_skipped(flag)) return; const T &t = mt_slice<MT_CHUNK>(tab, beg, end); .. }
//               entry: mt_foreground<MT_CHUNK>(who, t, count, ok, launch)
//   background: __global__ k(const MtTable<T> tab, int chunks, ..) { if (mt_skipped(flag)) return; mt_walk_bg(tab, chunks, Op{..}); }
//               entry: mt_background(who, t, count, workgroups, .., bg) and one launch of bg.grid x 1024 threads with BG_LDS
// Every tensor of a call is checked before its first launch: a refused call launches nothing.
#pragma once
#include "common.h"

#include <algorithm>
#include <cstdint>

namespace yolo {

constexpr int MT_CHUNK = 8192;     // elements per workgroup: 256 lanes x float4 x 8
constexpr int SQ_CHUNK = 65536;    // of the norm kernels: the atomic form ends in ONE fp64 atomic per workgroup on one address, keep them few
constexpr int BG_LDS = 96 * 1024;  // with 1024 threads: one background workgroup per CU, and no 128-KB conv workgroup beside it
constexpr long MT_MAX_CHUNKS = 0x7fffffffL;   // chunk = workgroup index: an int in the table, gridDim.x of the launch

template <class T>                 // T: one tensor of the pass, with its element count in `long n`
struct MtTable {
    T t[YOLO_MT_MAX];
    int first[YOLO_MT_MAX + 1];    // first chunk of every tensor
    int count;
};

struct SumsqTensor {               // both norm forms (sumsq_multi_kernel, sumsq_fixed_part_kernel)
    const float *g;
    long n;
};

__device__ __forceinline__ int find_tensor(const int *first, int count, int b)
{
    int i = 0;
    while (i + 1 < count && first[i + 1] <= b) ++i;  // wave-uniform scalar scan of <= 48 entries
    return i;
}

// foreground: workgroup blockIdx.x owns elements [beg, end) of the tensor returned
template <int CHUNK, class T>
__device__ __forceinline__ const T &mt_slice(const MtTable<T> &tab, long &beg, long &end)
{
    const int ti = find_tensor(tab.first, tab.count, blockIdx.x);
    const T &t = tab.t[ti];
    beg = (long)(blockIdx.x - tab.first[ti]) * CHUNK;
    end = min(t.n, beg + CHUNK);
    return t;
}

// clip_grad_norm_'s max_norm / (total_norm + 1e-6) in fp32 (tests/elementwise_ref.py::clip_ref restates it bit for bit), and the
// coefficient the optimizer kernels fold into the gradient: min(1, that), 1 without a norm
__device__ __forceinline__ float clip_ratio(const double *norm_sq, float max_norm)
{
    const float total = (float)sqrt(*norm_sq);
    return max_norm / (total + 1e-6f);
}
__device__ __forceinline__ float clip_coefficient(const double *norm_sq, float max_norm)
{
    if (!norm_sq) return 1.0f;
    const float c = clip_ratio(norm_sq, max_norm);
    return c < 1.0f ? c : 1.0f;
}

// true: the producer of the gradients flagged this step as invalid on the device, the launch writes nothing
__device__ __forceinline__ bool mt_skipped(const float *skip_flag)
{
    return skip_flag && *skip_flag != 0.0f;
}

__device__ __forceinline__ uint2 pack_bf16x4(const float4 &v)
{
    uint2 o;
    o.x = (unsigned)f32_to_bf16(v.x) | ((unsigned)f32_to_bf16(v.y) << 16);
    o.y = (unsigned)f32_to_bf16(v.z) | ((unsigned)f32_to_bf16(v.w) << 16);
    return o;
}

// A 256-thread workgroup's sum of g[i]^2 over the float4 groups i = i0, i0 + stride, .. < end (the lane's own i0) in fp64, handed to
// done(sum) in thread 0.  The grouping of a float4, the shuffle order and part[0] + .. + part[3] are what elementwise_ref.sumsq_ref
// and the order-fixed norm restate: they do not change.
template <class Done>
__device__ __forceinline__ void wg_sumsq(const float *__restrict__ g, long i0, long end, long stride, Done done)
{
    double s = 0.0;
    for (long i = i0; i < end; i += stride) {
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
    if (threadIdx.x == 0) done(part[0] + part[1] + part[2] + part[3]);
}

// Background form: gridDim.x PERSISTENT workgroups of 1024 threads walk the chunk list; the dynamic LDS they reserve (BG_LDS, unused)
// keeps every other workgroup off their CU.  The pass then occupies exactly gridDim.x CUs -- HBM-bound work that runs beside the next
// forward's MFMA-bound conv stack on the remaining CUs instead of in front of it (a grid of 25 k small workgroups would starve, or be
// starved by, the conv kernels, whose workgroups need a whole CU each).  A chunk is 1024 threads x 2 x float4; the loads of the NEXT
// chunk are issued before the current one is computed and stored, so that a CU always has 100-250 KB in flight (without the prefetch
// an Adam pass on 48 CUs reached 44 GB/s per CU).  The element op supplies
//   Op::Vals                    what a lane holds of one chunk: two float4 per array it reads
//   op.load(t, i, u, x)         x[u] = the float4s at element i of tensor t
//   op.full(t, i, u, x)         compute on x[u] and store at element i        (u = 0, 1: the two float4 of a whole chunk)
//   op.tail(t, k0, end, step)   elements k0, k0 + step, .. < end one by one   (the last, partial chunk of a tensor)
template <class T, class Op>
__device__ __forceinline__ void mt_walk_bg(const MtTable<T> &tab, int chunks, const Op &op)
{
    using Vals = typename Op::Vals;
    auto where = [&](int b, int &ti, long &beg, bool &full) {
        ti = find_tensor(tab.first, tab.count, b);
        beg = (long)(b - tab.first[ti]) * MT_CHUNK;
        full = beg + MT_CHUNK <= tab.t[ti].n;
    };
    auto load = [&](int ti, long beg, Vals &x) {
#pragma unroll
        for (int u = 0; u < 2; ++u) op.load(tab.t[ti], beg + (long)(u * 1024 + threadIdx.x) * 4, u, x);
    };
    int b = blockIdx.x;
    int ti = 0, nti = 0;
    long beg = 0, nbeg = 0;
    bool full = false, nfull = false;
    Vals cur, nxt;      // not zeroed: a chunk's values are read only where `full` says they were loaded
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
        const T t = tab.t[ti];      // a copy: the pointers are read from the kernel arguments once per chunk
        if (full) {
#pragma unroll
            for (int u = 0; u < 2; ++u) op.full(t, beg + (long)(u * 1024 + threadIdx.x) * 4, u, cur);
        } else {
            op.tail(t, beg + threadIdx.x, min(t.n, beg + MT_CHUNK), 1024);
        }
        b = nb; ti = nti; beg = nbeg; full = nfull;
        cur = nxt;
    }
}

// ---- host side ----

template <int CHUNK>
inline long mt_chunks(long n) { return (n + CHUNK - 1) / CHUNK; }

// tab = the first tensors of t[0 .. count) that fit one launch; -> how many it took
template <int CHUNK, class T>
inline int mt_fill(MtTable<T> &tab, const T *t, int count, long &chunks)
{
    chunks = 0;
    tab.first[0] = 0;
    int k = 0;
    for (; k < count && k < YOLO_MT_MAX; ++k) {
        const long c = mt_chunks<CHUNK>(t[k].n);
        if (chunks + c > MT_MAX_CHUNKS) break;
        chunks += c;
        tab.t[k] = t[k]; tab.first[k + 1] = (int)chunks;
    }
    tab.count = k;
    return k;
}

// ok(who, t[i], i) -> 0 or the code of a fail() for every tensor of the call; then every tensor must fit a launch of its own
template <int CHUNK, class T, class Ok>
inline int mt_check(const char *who, const T *t, int count, Ok ok)
{
    for (int i = 0; i < count; ++i) {
        if (int rc = ok(who, t[i], i)) return rc;
        if (mt_chunks<CHUNK>(t[i].n) > MT_MAX_CHUNKS) return fail(YOLO_E_UNSUPPORTED, "%s: tensor %d is too large", who, i);
    }
    return 0;
}

// launch(tab, chunks) -> 0 or an error code, once per YOLO_MT_MAX checked tensors (chunks > 0: the grid of the launch)
template <int CHUNK, class T, class Launch>
inline int mt_launch(const T *t, int count, Launch launch)
{
    for (int base = 0; base < count;) {
        MtTable<T> tab{};
        long chunks;
        base += mt_fill<CHUNK>(tab, t + base, count - base, chunks);
        if (chunks > 0)
            if (int rc = launch(tab, chunks)) return rc;
    }
    return 0;
}

template <int CHUNK, class T, class Ok, class Launch>
inline int mt_foreground(const char *who, const T *t, int count, Ok ok, Launch launch)
{
    if (int rc = mt_check<CHUNK>(who, t, count, ok)) return rc;
    return mt_launch<CHUNK>(t, count, launch);
}

template <class T>
struct MtBackground {
    MtTable<T> tab;
    int chunks;
    unsigned grid;      // persistent workgroups to launch; 0: the tensors are all empty, nothing to do
};

// Everything in front of a background launch: the limits of the form (args_ok: what else the entry requires of its scalars), every
// tensor, the one table, and the LDS the kernel `fn` may reserve (lds_done: one flag per device for this kernel).
template <class T, class Ok>
inline int mt_background(const char *who, const T *t, int count, int workgroups, bool args_ok, Ok ok, const void *fn, bool (&lds_done)[64], MtBackground<T> &bg)
{
    if (!t || count < 0 || count > YOLO_MT_MAX || workgroups < 1 || workgroups > 256 || !args_ok)
        return fail(YOLO_E_ARG, "%s: bad argument (at most %d tensors, 1 .. 256 workgroups)", who, YOLO_MT_MAX);
    for (int k = 0; k < count; ++k)
        if (int rc = ok(who, t[k], k)) return rc;
    bg = {};
    long chunks;
    if (mt_fill<MT_CHUNK>(bg.tab, t, count, chunks) < count) return fail(YOLO_E_UNSUPPORTED, "%s: too many elements", who);
    if (chunks == 0) return 0;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) dev = 0;
    if (!lds_done[dev]) {
        hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, BG_LDS);
        if (e != hipSuccess) return fail((int)e, "%s: hipFuncSetAttribute(%d B LDS): %s", who, BG_LDS, hipGetErrorString(e));
        lds_done[dev] = true;
    }
    bg.chunks = (int)chunks;
    bg.grid = (unsigned)std::min<long>(workgroups, chunks);
    return 0;
}

}  // namespace yolo
