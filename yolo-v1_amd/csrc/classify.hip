// Classification pretraining of the YOLOv1 trunk for gfx950: global average pool (forward, backward) and a fused softmax cross-entropy
// (loss, gradient, top-1 / top-5 hits).  These entries extend the reference surface -- mattiaskvist/yolo-v1 has no classifier stage (it loads
// torchvision's ImageNet weights instead) -- so they name the stock-torch operation they replace, not a reference line.
//
//   gap_rows_kernel       x [R][HW] fp32 -> y [R] : a group of L lanes (L a power of two that depends on HW only) owns a row; a lane adds its
//                         elements j, j + L, .. in that order, the group folds the L partial sums with an xor butterfly.  No atomics; the order
//                         of the additions is a function of HW alone.  HW = 49: L = 16, four rows per wave, no alignment assumed per row.
//   gap_bwd_kernel        dx [R][HW] = dy [R] * inv_hw : one fp32 multiply per element, 16-B stores over the flat buffer.
//   xent_rows_kernel      one workgroup per row of logits [N][K], strided loops (any K >= 1): max, then sum of exp / sum of logits / logits
//                         above the label's (one pass), the row loss in fp64 into work[n], then the gradient row.
//   xent_finish_kernel    one workgroup: adds work[0 .. N) in row order, writes the mean loss and the error flag.
// Compiled with -ffp-contract=off (Makefile, SRCS_EXACT): every operation rounds as written.
#include "common.h"

#include <cmath>

namespace yolo {

#pragma clang fp contract(off)

// ---------------------------------------------------------------------------------------------- global average pool

// lanes per row: enough that a lane adds at most four elements, at most a wave
static int gap_lanes(int HW)
{
    int L = 1;
    while (L < 64 && L * 4 < HW) L <<= 1;
    return L;
}

// block = 256 threads = 256 / L rows
__global__ void __launch_bounds__(256) gap_rows_kernel(const float *__restrict__ x, long R, int HW, int L, float inv_hw, float *__restrict__ y)
{
    const int rows_per_block = 256 / L;
    const int j = threadIdx.x & (L - 1);
    const long row = (long)blockIdx.x * rows_per_block + (threadIdx.x / L);
    float acc = 0.0f;
    if (row < R) {
        const float *p = x + row * HW;
        for (int i = j; i < HW; i += L) acc += p[i];
    }
    // every lane of the wave takes part (rows past R carry zeros); the butterfly stays inside the aligned group of L lanes
    for (int off = L >> 1; off > 0; off >>= 1) acc += __shfl_xor(acc, off, 64);
    if (row < R && j == 0) y[row] = acc * inv_hw;
}

// thread t writes elements 4t .. 4t + 3 of the flat buffer
__global__ void __launch_bounds__(256) gap_bwd_kernel(const float *__restrict__ dy, long total, int HW, float inv_hw, float *__restrict__ dx)
{
    const long i = ((long)blockIdx.x * 256 + threadIdx.x) * 4;
    if (i >= total) return;
    long r = i / HW;
    int rem = (int)(i - r * HW);
    float v[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        v[k] = (i + k < total) ? dy[r] * inv_hw : 0.0f;
        if (++rem == HW) { rem = 0; ++r; }
    }
    if (i + 4 <= total) {
        *reinterpret_cast<float4 *>(dx + i) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
        for (int k = 0; i + k < total; ++k) dx[i + k] = v[k];       // behind the last float4
    }
}

// dx not 16-B aligned: one element per thread
__global__ void __launch_bounds__(256) gap_bwd_scalar_kernel(const float *__restrict__ dy, long total, int HW, float inv_hw, float *__restrict__ dx)
{
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i < total) dx[i] = dy[i / HW] * inv_hw;
}

// ---------------------------------------------------------------------------------------------- softmax cross-entropy

#define XENT_THREADS 256
#define XENT_WAVES (XENT_THREADS / 64)

// workgroup-wide folds: xor butterfly inside the wave, then the four wave results through LDS, added in wave order by every thread
__device__ __forceinline__ float block_max(float v, float *sm)
{
    for (int off = 32; off > 0; off >>= 1) v = fmaxf(v, __shfl_xor(v, off, 64));
    __syncthreads();                                   // sm may still be read from the previous fold
    if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = v;
    __syncthreads();
    float r = sm[0];
    for (int w = 1; w < XENT_WAVES; ++w) r = fmaxf(r, sm[w]);
    return r;
}

__device__ __forceinline__ double block_sum(double v, double *sm)
{
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = v;
    __syncthreads();
    double r = sm[0];
    for (int w = 1; w < XENT_WAVES; ++w) r += sm[w];
    return r;
}

__device__ __forceinline__ int block_sum_int(int v, int *sm)
{
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = v;
    __syncthreads();
    int r = sm[0];
    for (int w = 1; w < XENT_WAVES; ++w) r += sm[w];
    return r;
}

// grid = N, block = 256
__global__ void __launch_bounds__(XENT_THREADS) xent_rows_kernel(const float *__restrict__ logits, const int64_t *__restrict__ labels, int K, float eps,
                                                                 float inv_n, float *__restrict__ dlogits, int32_t *__restrict__ hits,
                                                                 double *__restrict__ work)
{
    __shared__ float smf[XENT_WAVES];
    __shared__ double smd[XENT_WAVES];
    __shared__ int smi[XENT_WAVES];
    const long n = blockIdx.x;
    const float *x = logits + n * K;
    float *g = dlogits ? dlogits + n * K : nullptr;
    const int64_t y = labels[n];
    if (y < 0 || y >= K) {
        // a label outside [0, K): no loss, no gradient, no hits; x[y] is never formed.  xent_finish_kernel raises the flag from the label itself
        if (g)
            for (int i = threadIdx.x; i < K; i += XENT_THREADS) g[i] = 0.0f;
        if (threadIdx.x == 0) {
            work[n] = 0.0;
            if (hits) { hits[2 * n] = 0; hits[2 * n + 1] = 0; }
        }
        return;
    }
    const float xy = x[y];
    float m = -INFINITY;
    double sumx = 0.0;
    int above = 0;
    for (int i = threadIdx.x; i < K; i += XENT_THREADS) {
        const float v = x[i];
        m = fmaxf(m, v);
        sumx += (double)v;
        above += v > xy ? 1 : 0;
    }
    m = block_max(m, smf);
    sumx = block_sum(sumx, smd);
    above = block_sum_int(above, smi);
    double s = 0.0;
    for (int i = threadIdx.x; i < K; i += XENT_THREADS) s += (double)expf(x[i] - m);
    s = block_sum(s, smd);                            // >= 1: the maximum itself contributes exp(0)
    if (threadIdx.x == 0) {
        const double lse = (double)m + log(s);
        const double hard = lse - (double)xy;
        const double soft = lse - sumx / (double)K;
        work[n] = (1.0 - (double)eps) * hard + (double)eps * soft;
        if (hits) { hits[2 * n] = above < 1 ? 1 : 0; hits[2 * n + 1] = above < 5 ? 1 : 0; }
    }
    if (g) {
        const float sf = (float)s;
        const float off = eps / (float)K;
        const float on = (1.0f - eps) + off;
        for (int i = threadIdx.x; i < K; i += XENT_THREADS) {
            const float p = expf(x[i] - m) / sf;
            g[i] = (p - (i == y ? on : off)) * inv_n;
        }
    }
}

// single workgroup: thread 0 adds the row losses in row order, a chunk of 256 at a time through LDS
__global__ void __launch_bounds__(XENT_THREADS) xent_finish_kernel(const double *__restrict__ work, const int64_t *__restrict__ labels, int N, int K,
                                                                   float *__restrict__ out)
{
    __shared__ double sm[XENT_THREADS];
    __shared__ int smi[XENT_WAVES];
    double total = 0.0;
    int bad = 0;
    for (int base = 0; base < N; base += XENT_THREADS) {
        const int n = base + threadIdx.x;
        if (n < N) {
            sm[threadIdx.x] = work[n];
            const int64_t y = labels[n];
            bad += (y < 0 || y >= K) ? 1 : 0;
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            const int cnt = min(XENT_THREADS, N - base);
            for (int k = 0; k < cnt; ++k) total += sm[k];
        }
        __syncthreads();
    }
    bad = block_sum_int(bad, smi);
    if (threadIdx.x == 0) {
        out[0] = (float)(total / (double)N);          // reduction="mean": an empty batch gives NaN, as torch does
        out[1] = bad > 0 ? 1.0f : 0.0f;
    }
}

}  // namespace yolo

using namespace yolo;

YOLO_API int yolo_gap_fwd(const float *x, int N, int C, int HW, float *y, yolo_stream_t stream)
{
    if (!x || !y || N < 0 || C < 1 || HW < 1) return fail(YOLO_E_ARG, "yolo_gap_fwd: bad argument");
    const long R = (long)N * C;
    if (R == 0) return 0;
    const int L = gap_lanes(HW);
    const long blocks = (R + (256 / L) - 1) / (256 / L);
    if (blocks > 0x7fffffffL) return fail(YOLO_E_UNSUPPORTED, "yolo_gap_fwd: N * C = %ld is too large", R);
    hipLaunchKernelGGL(gap_rows_kernel, dim3((unsigned)blocks), dim3(256), 0, STRM(stream), x, R, HW, L, (float)(1.0 / (double)HW), y);
    return check_launch("yolo_gap_fwd");
}

YOLO_API int yolo_gap_bwd(const float *dy, int N, int C, int HW, float *dx, yolo_stream_t stream)
{
    if (!dy || !dx || N < 0 || C < 1 || HW < 1) return fail(YOLO_E_ARG, "yolo_gap_bwd: bad argument");
    const long total = (long)N * C * HW;
    if (total == 0) return 0;
    const float inv_hw = (float)(1.0 / (double)HW);
    const bool vec = ((uintptr_t)dx & 15) == 0;
    const long threads = vec ? (total + 3) / 4 : total;
    const long blocks = (threads + 255) / 256;
    if (blocks > 0x7fffffffL) return fail(YOLO_E_UNSUPPORTED, "yolo_gap_bwd: N * C * HW = %ld is too large", total);
    if (vec)
        hipLaunchKernelGGL(gap_bwd_kernel, dim3((unsigned)blocks), dim3(256), 0, STRM(stream), dy, total, HW, inv_hw, dx);
    else
        hipLaunchKernelGGL(gap_bwd_scalar_kernel, dim3((unsigned)blocks), dim3(256), 0, STRM(stream), dy, total, HW, inv_hw, dx);
    return check_launch("yolo_gap_bwd");
}

YOLO_API int yolo_softmax_xent_fwd_bwd(const float *logits, const int64_t *labels, int N, int K, float label_smoothing, float *out, float *dlogits,
                                       int32_t *hits, double *work, yolo_stream_t stream)
{
    if (!logits || !labels || !out || !hits || !work || N < 0 || K < 1 || !(label_smoothing >= 0.0f && label_smoothing < 1.0f))
        return fail(YOLO_E_ARG, "yolo_softmax_xent_fwd_bwd: null pointer, N = %d < 0, K = %d < 1 or label_smoothing = %g outside [0, 1)", N, K,
                    (double)label_smoothing);
    if (N > 0)
        hipLaunchKernelGGL(xent_rows_kernel, dim3((unsigned)N), dim3(XENT_THREADS), 0, STRM(stream), logits, labels, K, label_smoothing,
                           (float)(1.0 / (double)N), dlogits, hits, work);
    hipLaunchKernelGGL(xent_finish_kernel, dim3(1), dim3(XENT_THREADS), 0, STRM(stream), work, labels, N, K, out);
    return check_launch("yolo_softmax_xent_fwd_bwd");
}
