// PASCAL VOC devkit matching of kept detections against the annotated ground truth, and the compaction of the result, for
// gfx950 -- one launch behind yolo_decode / yolo_decode_classes + yolo_nms (metrics variant).  fp64 in the operand order of
// DESIGN.md, "VOC devkit evaluation" (tests/voc_ref.py restates it); this file MUST be compiled with -ffp-contract=off: the
// union (a * b + c * d - e * f) and the pixel corners ((x - w / 2) * W) would otherwise be fused and the overlaps, which are
// compared with >= against the thresholds and with > against each other, would round differently.
//
// The devkit sorts ALL detections of a class by score and walks them; a detection only ever meets the ground truths of its own
// image, and an image's kept list (metrics NMS order: grouped by class, inside a class score-descending, ties in scan order)
// is that global order restricted to the image -- the argument yolo/metrics.py makes for yolo_map_match -- so the greedy
// matching is per group.  One single-wave workgroup per group ((image, class) under scoring "all", an image under "argmax"):
//   1. the group's output base = sum of the keep counts of the groups in front of it, reduced by the wave itself (a few
//      thousand ints from L2): dense rows in group order then NMS order, no atomics, no second launch, a fixed order;
//   2. lane l owns the image's ground truths l, l + 64, l + 128, l + 192 (<= 256 per image) in registers, with one
//      `taken` bit per threshold each;
//   3. the kept detections are staged 64 at a time (lane l converts detection k0 + l to clamped pixel corners and writes the
//      row's score, class, image and box), then walked one by one: every lane measures the overlap with its ground truths
//      of the detection's class, a 6-step butterfly finds the largest overlap and the lowest index among equal ones, the
//      owning lane decides TP / FP / ignored for all thresholds at once and the status word goes back by one __shfl.
#include "common.h"

namespace yolo {

#pragma clang fp contract(off)

constexpr int VOC_MAX_T = 16;
constexpr int VOC_MAX_GT = 256;
constexpr int VOC_GT_SLOTS = VOC_MAX_GT / 64;
constexpr int VOC_MAX_PER_GROUP = 1024;

struct VocMatchParams {
    double thr[VOC_MAX_T];
    int T;
};

__device__ __forceinline__ int wave_sum(int v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

__global__ void __launch_bounds__(64) voc_match_kernel(const double *__restrict__ rec, const int *__restrict__ keep, const int *__restrict__ kcnt,
                                                       int n_groups, int M, int groups_per_image, const double *__restrict__ gt_box,
                                                       const int *__restrict__ gt_cls, const unsigned char *__restrict__ gt_dif,
                                                       const int *__restrict__ gt_off, const double *__restrict__ img_wh, int max_gt, int image_base,
                                                       const VocMatchParams prm, double *__restrict__ out_score, int *__restrict__ out_cls_img,
                                                       unsigned int *__restrict__ out_status, double *__restrict__ out_box, int *__restrict__ out_total)
{
    __shared__ double s_box[64][4];
    __shared__ int s_cls[64];
    const int grp = blockIdx.x, lane = threadIdx.x;
    const int img = grp / groups_per_image;

    // 1. output base
    int part = 0;
    for (int g = lane; g < grp; g += 64) {
        const int c = kcnt[g];
        part += c < 0 ? 0 : (c > M ? M : c);
    }
    const long base = wave_sum(part);
    int nk = kcnt[grp];
    nk = nk < 0 ? 0 : (nk > M ? M : nk);
    if (grp == n_groups - 1 && lane == 0) out_total[0] = (int)(base + nk);
    if (nk == 0) return;                                   // wave-uniform

    // 2. this lane's ground truths
    const int g0 = gt_off[img];
    int ng = gt_off[img + 1] - g0;
    ng = ng < 0 ? 0 : (ng > max_gt ? max_gt : ng);          // max_gt <= VOC_MAX_GT (checked by the host entry)
    double gx1[VOC_GT_SLOTS], gy1[VOC_GT_SLOTS], gx2[VOC_GT_SLOTS], gy2[VOC_GT_SLOTS], garea[VOC_GT_SLOTS];
    int gcls[VOC_GT_SLOTS];
    bool gdif[VOC_GT_SLOTS];
    unsigned int taken[VOC_GT_SLOTS];
#pragma unroll
    for (int s = 0; s < VOC_GT_SLOTS; ++s) {
        const int j = lane + 64 * s;
        gcls[s] = -1; gdif[s] = false; taken[s] = 0u;
        gx1[s] = gy1[s] = gx2[s] = gy2[s] = garea[s] = 0.0;
        if (j < ng) {
            const double *b = gt_box + 4 * (size_t)(g0 + j);
            gx1[s] = b[0]; gy1[s] = b[1]; gx2[s] = b[2]; gy2[s] = b[3];
            garea[s] = (gx2[s] - gx1[s] + 1) * (gy2[s] - gy1[s] + 1);
            gcls[s] = gt_cls[g0 + j];
            gdif[s] = gt_dif[g0 + j] != 0;
        }
    }
    const double W = img_wh[2 * (size_t)img], H = img_wh[2 * (size_t)img + 1];
    const double *r_grp = rec + (size_t)grp * M * 6;
    const int *k_grp = keep + (size_t)grp * M;

    // 3. chunks of 64 kept detections
    for (int k0 = 0; k0 < nk; k0 += 64) {
        const int cnt = nk - k0 < 64 ? nk - k0 : 64;
        const long row = base + k0 + lane;
        if (lane < cnt) {
            int idx = k_grp[k0 + lane];
            idx = idx < 0 ? 0 : (idx >= M ? M - 1 : idx);
            const double *r = r_grp + (size_t)idx * 6;
            const double x = r[2], y = r[3], w = r[4], h = r[5];
            double x1 = (x - w / 2) * W, y1 = (y - h / 2) * H, x2 = (x + w / 2) * W, y2 = (y + h / 2) * H;
            if (x1 < 0) x1 = 0.0;
            if (x1 > W) x1 = W;
            if (x2 < 0) x2 = 0.0;
            if (x2 > W) x2 = W;
            if (y1 < 0) y1 = 0.0;
            if (y1 > H) y1 = H;
            if (y2 < 0) y2 = 0.0;
            if (y2 > H) y2 = H;
            const int c = (int)r[0];
            s_box[lane][0] = x1; s_box[lane][1] = y1; s_box[lane][2] = x2; s_box[lane][3] = y2;
            s_cls[lane] = c;
            out_score[row] = r[1];
            out_cls_img[2 * row] = c;
            out_cls_img[2 * row + 1] = image_base + img;
            double *ob = out_box + 4 * row;
            ob[0] = x1; ob[1] = y1; ob[2] = x2; ob[3] = y2;
        }
        __syncthreads();
        unsigned int my_status = 0u;
        for (int d = 0; d < cnt; ++d) {
            const double x1 = s_box[d][0], y1 = s_box[d][1], x2 = s_box[d][2], y2 = s_box[d][3];
            const int c = s_cls[d];
            const double darea = (x2 - x1 + 1) * (y2 - y1 + 1);
            double best = -__builtin_inf();
            int bj = 0x7fffffff;
#pragma unroll
            for (int s = 0; s < VOC_GT_SLOTS; ++s) {
                if (gcls[s] != c) continue;                 // other classes (and empty slots: -1) never take part
                const double iw = (gx2[s] < x2 ? gx2[s] : x2) - (gx1[s] > x1 ? gx1[s] : x1) + 1;
                const double ih = (gy2[s] < y2 ? gy2[s] : y2) - (gy1[s] > y1 ? gy1[s] : y1) + 1;
                if (iw > 0 && ih > 0) {
                    const double ua = darea + garea[s] - iw * ih;
                    const double ov = iw * ih / ua;
                    if (ov > best) { best = ov; bj = lane + 64 * s; }     // slots ascend: strict '>' keeps the lowest index
                }
            }
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                const double ob = __shfl_xor(best, o);
                const int oj = __shfl_xor(bj, o);
                if (ob > best || (ob == best && oj < bj)) { best = ob; bj = oj; }
            }
            // every lane now holds the same (best, bj); bj == 0x7fffffff: no candidate
            unsigned int st = 0u;
            const int owner = bj & 63;
            if (bj != 0x7fffffff && lane == owner) {
                const int slot = bj >> 6;
                bool dif = false;
                unsigned int tk = 0u;
#pragma unroll
                for (int s = 0; s < VOC_GT_SLOTS; ++s)
                    if (s == slot) { dif = gdif[s]; tk = taken[s]; }
                for (int t = 0; t < prm.T; ++t) {
                    if (!(best >= prm.thr[t])) continue;    // FP
                    if (dif) st |= 2u << (2 * t);            // ignored, consumes nothing
                    else if (!((tk >> t) & 1u)) { st |= 1u << (2 * t); tk |= 1u << t; }
                }
#pragma unroll
                for (int s = 0; s < VOC_GT_SLOTS; ++s)
                    if (s == slot) taken[s] = tk;
            }
            if (bj != 0x7fffffff) st = __shfl(st, owner);
            if (lane == d) my_status = st;
        }
        if (lane < cnt) out_status[row] = my_status;
        __syncthreads();                                    // the next chunk overwrites s_box / s_cls
    }
}

}  // namespace yolo

using namespace yolo;

YOLO_API int yolo_voc_match(const double *rec, const int32_t *keep, const int32_t *keep_counts, int n_groups, int max_per_group, int groups_per_image,
                            const double *gt_box, const int32_t *gt_cls, const unsigned char *gt_difficult, const int32_t *gt_off, const double *img_wh,
                            int max_gt, int image_base, const double *thresholds, int T, double *out_score, int32_t *out_cls_img, uint32_t *out_status,
                            double *out_box, int32_t *out_total, yolo_stream_t stream)
{
    if (!rec || !keep || !keep_counts || !gt_box || !gt_cls || !gt_difficult || !gt_off || !img_wh || !thresholds || !out_score || !out_cls_img ||
        !out_status || !out_box || !out_total)
        return fail(YOLO_E_ARG, "yolo_voc_match: null pointer");
    if (n_groups < 0 || groups_per_image < 1 || n_groups % groups_per_image != 0 || max_gt < 0 || image_base < 0)
        return fail(YOLO_E_ARG, "yolo_voc_match: bad size (n_groups=%d, groups_per_image=%d, max_gt=%d, image_base=%d)", n_groups, groups_per_image, max_gt,
                    image_base);
    if (T < 1 || T > VOC_MAX_T) return fail(YOLO_E_ARG, "yolo_voc_match: 1..%d thresholds (got %d)", VOC_MAX_T, T);
    if (max_gt > VOC_MAX_GT) return fail(YOLO_E_ARG, "yolo_voc_match: at most %d ground truths per image (got %d)", VOC_MAX_GT, max_gt);
    if (max_per_group < 1 || max_per_group > VOC_MAX_PER_GROUP)
        return fail(YOLO_E_ARG, "yolo_voc_match: max_per_group=%d outside 1..%d", max_per_group, VOC_MAX_PER_GROUP);
    if (n_groups == 0) {
        hipError_t e = hipMemsetAsync(out_total, 0, sizeof(int32_t), STRM(stream));
        if (e != hipSuccess) return fail((int)e, "yolo_voc_match: %s", hipGetErrorString(e));
        return 0;
    }
    VocMatchParams prm{};
    for (int t = 0; t < T; ++t) prm.thr[t] = thresholds[t];
    prm.T = T;
    hipLaunchKernelGGL(voc_match_kernel, dim3(n_groups), dim3(64), 0, STRM(stream), rec, keep, keep_counts, n_groups, max_per_group, groups_per_image, gt_box,
                       gt_cls, gt_difficult, gt_off, img_wh, max_gt, image_base, prm, out_score, out_cls_img, out_status, out_box, out_total);
    return check_launch("yolo_voc_match");
}
