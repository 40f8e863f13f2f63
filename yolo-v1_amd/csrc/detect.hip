// The last step of batched detection for gfx950: the kept detections of yolo_decode / yolo_decode_classes + yolo_nms (inference
// variant) as the final answer -- per image one dense list in result order, boxes in the pixels of the original image -- so that
// the copy to the host is the detections and nothing else (yolo/ops.py: detect / detect_host).  One launch behind yolo_nms, no
// atomics, every output word a function of the inputs alone.  This file MUST be compiled with -ffp-contract=off: the pixel
// corners ((x - w / 2) * W) are the fp64 operations of yolo/_post_cpu.py: voc_pixel_boxes, one rounding each.
//
// One 256-thread workgroup per image:
//   1. its first output row = the sum of the keep counts of all groups of the images in front of it, reduced by the workgroup
//      itself (a few thousand ints from L2) -> out_off; the last workgroup also writes out_off[images];
//   2. the image's list is its groups one behind the other, each in its keep order.  With one group per image that is the
//      result order.  With several (class-specific scoring) the result order is that list sorted by score descending, equal
//      scores in list order (numpy's stable argsort of -score).  Every group's keep list already is in that order (yolo_nms,
//      inference variant: confidence order, ties in scan order), so the place of entry k of group g is
//          k + sum over groups in front of g of #{score >= s} + sum over groups behind g of #{score > s},
//      each count one binary search over a sorted list: a merge by rank, no sorting network, no exchange between threads;
//   3. the thread that ranked an entry writes its row.
// The scores the searches read are staged in LDS when groups_per_image * max_per_group <= 4096 (the default model: 20 x 98);
// beyond that the same searches read them through the keep indices from global memory -- slower (two dependent loads a step),
// never wrong, and no shape is refused.
#include "common.h"

namespace yolo {

#pragma clang fp contract(off)

constexpr int DET_THREADS = 256;
constexpr int DET_STAGE = 4096;        // scores (and group counts) held in LDS

struct DetImage {
    const double *rec;                 // the image's first group
    const int *keep, *kcnt;
    int M, gpi;
    bool staged;
    const double *s_score;             // [gpi][M] when staged
    const int *s_kc;                   // the first min(gpi, DET_STAGE) clamped keep counts

    __device__ __forceinline__ int count(int g) const
    {
        if (g < DET_STAGE) return s_kc[g];
        const int c = kcnt[g];
        return c < 0 ? 0 : (c > M ? M : c);
    }
    __device__ __forceinline__ const double *row(int g, int k) const
    {
        int idx = keep[(size_t)g * M + k];
        idx = idx < 0 ? 0 : (idx >= M ? M - 1 : idx);
        return rec + ((size_t)g * M + idx) * 6;
    }
    __device__ __forceinline__ double score(int g, int k) const { return staged ? s_score[g * M + k] : row(g, k)[1]; }
    // entries of group g (n of them, scores descending) that go in front of score s: those above it, and the equal ones if `ties`
    __device__ __forceinline__ int in_front(int g, int n, double s, bool ties) const
    {
        int lo = 0, hi = n;
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            const double v = score(g, mid);
            if (v > s || (ties && v == s)) lo = mid + 1;
            else hi = mid;
        }
        return lo;
    }
};

__global__ void __launch_bounds__(DET_THREADS) detect_finish_kernel(const double *__restrict__ rec, const int *__restrict__ keep,
                                                                    const int *__restrict__ kcnt, int n_groups, int M, int gpi,
                                                                    const double *__restrict__ img_wh, double *__restrict__ out_det,
                                                                    int *__restrict__ out_image, int *__restrict__ out_off)
{
    __shared__ double s_score[DET_STAGE];
    __shared__ int s_kc[DET_STAGE];
    __shared__ int s_part[DET_THREADS / 64];
    const int img = blockIdx.x, tid = threadIdx.x;
    const long g0 = (long)img * gpi;

    // 1. first row of this image
    int part = 0;
    for (long g = tid; g < g0; g += DET_THREADS) {
        const int c = kcnt[g];
        part += c < 0 ? 0 : (c > M ? M : c);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) part += __shfl_xor(part, o);
    if ((tid & 63) == 0) s_part[tid >> 6] = part;
    const int n_kc = gpi < DET_STAGE ? gpi : DET_STAGE;
    for (int g = tid; g < n_kc; g += DET_THREADS) {
        const int c = kcnt[g0 + g];
        s_kc[g] = c < 0 ? 0 : (c > M ? M : c);
    }
    __syncthreads();
    int base = 0;
#pragma unroll
    for (int w = 0; w < DET_THREADS / 64; ++w) base += s_part[w];

    DetImage im{rec + (size_t)g0 * M * 6, keep + (size_t)g0 * M, kcnt + g0, M, gpi, (long)gpi * M <= DET_STAGE, s_score, s_kc};
    const long slots = (long)gpi * M;
    if (im.staged && gpi > 1) {
        for (int i = tid; i < (int)slots; i += DET_THREADS) {
            const int g = i / M, k = i - g * M;
            if (k < s_kc[g]) s_score[i] = im.row(g, k)[1];
        }
        __syncthreads();
    }
    if (tid == 0) {
        out_off[img] = base;
        if (g0 + gpi == n_groups) {
            int nk = 0;
            for (int g = 0; g < gpi; ++g) nk += im.count(g);
            out_off[img + 1] = base + nk;
        }
    }
    double W = 0.0, H = 0.0;
    if (img_wh) { W = img_wh[2 * (size_t)img]; H = img_wh[2 * (size_t)img + 1]; }

    // 2. + 3. one entry per thread and round: its place in the image's result order, then its row
    for (long i = tid; i < slots; i += DET_THREADS) {
        const int g = (int)(i / M), k = (int)(i - (long)g * M);
        if (k >= im.count(g)) continue;
        int rank = k;
        if (gpi > 1) {
            const double s = im.score(g, k);
            for (int o = 0; o < gpi; ++o) {
                const int n = im.count(o);
                if (n == 0 || o == g) continue;
                rank += im.in_front(o, n, s, o < g);
            }
        }
        const double *r = im.row(g, k);
        const size_t out = (size_t)base + rank;
        double *d = out_det + out * 6;
        d[0] = r[0];
        d[1] = r[1];
        if (img_wh) {
            const double x = r[2], y = r[3], w = r[4], h = r[5];
            double x1 = (x - w / 2) * W, y1 = (y - h / 2) * H, x2 = (x + w / 2) * W, y2 = (y + h / 2) * H;
            if (x1 < 0) x1 = 0.0;
            if (x1 > W) x1 = W;
            if (y1 < 0) y1 = 0.0;
            if (y1 > H) y1 = H;
            if (x2 < 0) x2 = 0.0;
            if (x2 > W) x2 = W;
            if (y2 < 0) y2 = 0.0;
            if (y2 > H) y2 = H;
            d[2] = x1; d[3] = y1; d[4] = x2; d[5] = y2;
        } else {
            d[2] = r[2]; d[3] = r[3]; d[4] = r[4]; d[5] = r[5];
        }
        out_image[out] = img;
    }
}

}  // namespace yolo

using namespace yolo;

YOLO_API int yolo_detect_finish(const double *rec, const int32_t *keep, const int32_t *keep_counts, int n_groups, int max_per_group, int groups_per_image,
                                const double *img_wh, double *out_det, int32_t *out_image, int32_t *out_off, yolo_stream_t stream)
{
    if (!rec || !keep || !keep_counts || !out_det || !out_image || !out_off) return fail(YOLO_E_ARG, "yolo_detect_finish: null pointer");
    if (n_groups < 0 || max_per_group < 1 || groups_per_image < 1 || n_groups % groups_per_image != 0)
        return fail(YOLO_E_ARG, "yolo_detect_finish: bad size (n_groups=%d, max_per_group=%d, groups_per_image=%d)", n_groups, max_per_group,
                    groups_per_image);
    if ((long)n_groups * max_per_group > 0x7fffffffL)
        return fail(YOLO_E_UNSUPPORTED, "yolo_detect_finish: %ld rows exceed the int32 offsets", (long)n_groups * max_per_group);
    if (n_groups == 0) {
        hipError_t e = hipMemsetAsync(out_off, 0, sizeof(int32_t), STRM(stream));
        if (e != hipSuccess) return fail((int)e, "yolo_detect_finish: %s", hipGetErrorString(e));
        return 0;
    }
    hipLaunchKernelGGL(detect_finish_kernel, dim3(n_groups / groups_per_image), dim3(DET_THREADS), 0, STRM(stream), rec, keep, keep_counts, n_groups,
                       max_per_group, groups_per_image, img_wh, out_det, out_image, out_off);
    return check_launch("yolo_detect_finish");
}
