// Tile code of the factored Linear gradient (include/yolo_hip.h: yolo_fc_factors): G = scale * dy^T x rebuilt per 64 x 64 weight tile on
// the matrix cores and handed, register by register, to an element op -- the store of yolo_fc_factored_grad (fc_factored.hip), AdamOp::one
// (optim.hip: yolo_adam_step_factored), sgd1 (sgd.hip: yolo_sgd_step_factored).  All three go through fc_tile_product and fc_scaled, so G is
// the same bits in each of them and for any grid.
//
// A team of four waves owns a tile of FC_T x FC_T weights; wave w owns the 32 x 32 quarter (w >> 1, w & 1).  With
// v_mfma_f32_32x32x16_bf16 as D[o][i] = sum_n A[o][n] B[n][i] lane l (r = l & 31, h = l >> 5) needs A = dy[n0 + 8h .. + 8][o0 + r] and
// B = x[n0 + 8h .. + 8][i0 + r]: eight values along the BATCH axis, which is the slow axis of both factors in memory.  So the two K panels
// of a tile are staged TRANSPOSED in LDS ([column][n], pitch kpad + 8 elements: 16-B reads, rows kpad .. pitch never read), zero-filled
// from `rows` up to kpad = rows rounded up to the K step of 16 and beyond the edges of the factors.  The accumulator then has the input
// feature on the lane (col = lane & 31) and the output feature in the register (row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)): one
// register of a wave is two 128-B row segments of p / m / v, the shape that stores at the full rate with no shuffle.
// Rows o >= O or columns i >= I of an edge tile are computed from zeros (or, inside ld_dy, from whatever the padding columns hold: an MFMA
// row depends on its own A row only) and never stored.
#pragma once
#include "multi_tensor.h"

namespace yolo {

typedef __attribute__((ext_vector_type(8))) __bf16 fc_bf16x8;
typedef __attribute__((ext_vector_type(16))) float fc_f32x16;

constexpr int FC_T = 64;          // tile edge, both ways
constexpr int FC_KSTEP = 16;      // K of the MFMA
constexpr int FC_PAD = 8;         // elements between LDS rows beyond kpad
constexpr unsigned FC_GRID_ALL = 2048;   // workgroups == 0: persistent workgroups of "the whole chip" (8 per CU at rows = 64)

struct FcTiles {                  // yolo_fc_factors as the kernels take it
    const bf16_t *dy, *x;
    int rows, O, I, ld_dy, ld_x;
    float scale;
    int kpad;                     // rows rounded up to FC_KSTEP
    int tiles_i;                  // tiles along I
    long tiles;
};

// Staging of both K panels of tile (o0, i0) into LDS, transposed, by the 256 threads of a team.  An item is one 16-B group of eight columns of one
// batch row, the eight groups of a panel's row (one 128-B line) on neighbouring lanes; a thread owns items tid, tid + 256, ..: kpad / 16 of them.
__device__ __forceinline__ uint4 fc_stage_load(const FcTiles &f, int o0, int i0, int item)
{
    const int per_panel = f.kpad * (FC_T / 8);
    const int which = item >= per_panel;                      // 0: dy, 1: x
    const int it = item - which * per_panel;
    const int grp = it & 7, n = it >> 3;
    const int col = (which ? i0 : o0) + grp * 8;
    const int lim = which ? f.I : f.ld_dy;                    // I % 8 == 0 and ld_dy % 8 == 0: a group is inside the row or outside
    uint4 v = make_uint4(0u, 0u, 0u, 0u);
    if (item < 2 * per_panel && n < f.rows && col < lim) {
        const bf16_t *src = which ? f.x + (long)n * f.ld_x + col : f.dy + (long)n * f.ld_dy + col;
        v = *reinterpret_cast<const uint4 *>(src);
    }
    return v;
}

__device__ __forceinline__ void fc_stage_store(const FcTiles &f, int item, const uint4 &v, bf16_t *lds)
{
    const int pitch = f.kpad + FC_PAD;
    const int per_panel = f.kpad * (FC_T / 8);
    if (item >= 2 * per_panel) return;
    const int which = item >= per_panel;
    const int it = item - which * per_panel;
    const int grp = it & 7, n = it >> 3;
    bf16_t *dst = lds + (which * FC_T + grp * 8) * pitch + n;
    dst[0 * pitch] = (bf16_t)(v.x & 0xffffu); dst[1 * pitch] = (bf16_t)(v.x >> 16);
    dst[2 * pitch] = (bf16_t)(v.y & 0xffffu); dst[3 * pitch] = (bf16_t)(v.y >> 16);
    dst[4 * pitch] = (bf16_t)(v.z & 0xffffu); dst[5 * pitch] = (bf16_t)(v.z >> 16);
    dst[6 * pitch] = (bf16_t)(v.w & 0xffffu); dst[7 * pitch] = (bf16_t)(v.w >> 16);
}

// THE tile product: the 32 x 32 quarter (wo, wi) of the staged tile, K steps in rising order.  Every entry that needs G calls this.
__device__ __forceinline__ fc_f32x16 fc_tile_product(const bf16_t *lds, int kpad, int wo, int wi)
{
    const int pitch = kpad + FC_PAD;
    const int lane = threadIdx.x & 63, r = lane & 31, h = lane >> 5;
    const bf16_t *a = lds + (wo * 32 + r) * pitch + 8 * h;
    const bf16_t *b = lds + (FC_T + wi * 32 + r) * pitch + 8 * h;
    fc_f32x16 acc = {};
    for (int k = 0; k < kpad; k += FC_KSTEP) {
        const fc_bf16x8 av = *reinterpret_cast<const fc_bf16x8 *>(a + k);
        const fc_bf16x8 bv = *reinterpret_cast<const fc_bf16x8 *>(b + k);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(av, bv, acc, 0, 0, 0);
    }
    return acc;
}

// G from the accumulator: one fp32 multiply, never contracted into what an element op does next
__device__ __forceinline__ float fc_scaled(float acc, float scale)
{
#pragma clang fp contract(off)
    const float g = acc * scale;
    return g;
}

// The walk of every factored kernel.  A workgroup is TEAMS teams of 256 threads, each with K panels of its own; workgroup b takes the tiles
// (b + k gridDim.x) TEAMS + team, k = 0, 1, ..; tile t = (t / tiles_i, t % tiles_i).  The element op supplies
//   Epi::Elem                 what a lane holds of one weight besides G
//   epi.load(idx, e)          e = the values at weight idx = o * I + i
//   epi.finish(idx, g, e)     compute and store
// Order inside a tile: the first FC_PRE staging loads (the factors: L2 hits), THEN the loads of the lane's 16 weights (HBM), then the LDS
// writes, the product and the element op -- loads return in order, so the HBM latency of p / m / v runs under the staging and the MFMAs
// instead of behind them.  (Factors of more than 16 * FC_PRE = 64 rows stage the rest behind the weights' loads.)
constexpr int FC_PRE = 4;

template <int TEAMS, class Epi>
__device__ __forceinline__ void fc_walk_tiles(const FcTiles &f, const Epi &epi)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char fc_lds_raw[];
    const int team = TEAMS > 1 ? (int)(threadIdx.x >> 8) : 0, tid = threadIdx.x & 255;
    bf16_t *lds = reinterpret_cast<bf16_t *>(fc_lds_raw) + team * (2 * FC_T * (f.kpad + FC_PAD));
    const int wave = tid >> 6, lane = tid & 63;
    const int wo = wave >> 1, wi = wave & 1;
    const int items = 2 * f.kpad * (FC_T / 8);
    for (long t0 = (long)blockIdx.x * TEAMS; t0 < f.tiles; t0 += (long)gridDim.x * TEAMS) {      // the same trip count for every team: barriers inside
        const long t = t0 + team;
        const bool live = t < f.tiles;
        const int o0 = live ? (int)(t / f.tiles_i) * FC_T : 0, i0 = live ? (int)(t % f.tiles_i) * FC_T : 0;
        uint4 pre[FC_PRE];
#pragma unroll
        for (int j = 0; j < FC_PRE; ++j) pre[j] = fc_stage_load(f, o0, i0, live ? tid + j * 256 : items);
        const int i = i0 + wi * 32 + (lane & 31);
        const int ob = o0 + wo * 32 + 4 * (lane >> 5);
        typename Epi::Elem e[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int o = ob + (r & 3) + 8 * (r >> 2);
            if (live && o < f.O && i < f.I) epi.load((long)o * f.I + i, e[r]);
        }
        __syncthreads();                                     // the previous tile's operand reads are done
#pragma unroll
        for (int j = 0; j < FC_PRE; ++j) fc_stage_store(f, tid + j * 256, pre[j], lds);
        for (int item = tid + FC_PRE * 256; item < items; item += 256) fc_stage_store(f, item, fc_stage_load(f, o0, i0, live ? item : items), lds);
        __syncthreads();
        const fc_f32x16 acc = fc_tile_product(lds, f.kpad, wo, wi);
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int o = ob + (r & 3) + 8 * (r >> 2);
            if (live && o < f.O && i < f.I) epi.finish((long)o * f.I + i, fc_scaled(acc[r], f.scale), e[r]);
        }
    }
}

// ---- host side ----

struct FcLaunch {
    FcTiles f;
    unsigned grid;
    unsigned lds;       // bytes of dynamic LDS of a workgroup (all its teams)
    int teams;          // 1, 2 or 4 teams of 256 threads per workgroup
};

constexpr unsigned FC_LDS_MOST = 2u * FC_T * (YOLO_FC_MAX_ROWS + FC_PAD) * (unsigned)sizeof(bf16_t);      // 133,120 B: one team at YOLO_FC_MAX_ROWS

inline bool fc_misaligned(const void *p, unsigned mask) { return ((uintptr_t)p & mask) != 0; }

// the checks every entry shares on its descriptor; -> 0 or the code of a fail()
inline int fc_check(const char *who, const yolo_fc_factors *d)
{
    if (!d) return fail(YOLO_E_ARG, "%s: null descriptor", who);
    if (!d->dy || !d->x) return fail(YOLO_E_ARG, "%s: null factor", who);
    if (d->rows < 1 || d->O < 1 || d->I < 1 || d->ld_dy < d->O || d->ld_x < d->I)
        return fail(YOLO_E_ARG, "%s: rows %d, O %d, I %d, ld_dy %d, ld_x %d: sizes must be >= 1 and the pitches cover the columns", who, d->rows, d->O,
                    d->I, d->ld_dy, d->ld_x);
    if (d->I % 8) return fail(YOLO_E_UNSUPPORTED, "%s: I = %d is not a multiple of 8", who, d->I);
    if (d->ld_dy % 8 || d->ld_x % 8) return fail(YOLO_E_UNSUPPORTED, "%s: ld_dy = %d, ld_x = %d must be multiples of 8", who, d->ld_dy, d->ld_x);
    if (fc_misaligned(d->dy, 15) || fc_misaligned(d->x, 15)) return fail(YOLO_E_UNSUPPORTED, "%s: dy and x must be 16-B aligned", who);
    if (d->rows > YOLO_FC_MAX_ROWS) return fail(YOLO_E_UNSUPPORTED, "%s: rows = %d, at most %d (YOLO_FC_MAX_ROWS)", who, d->rows, YOLO_FC_MAX_ROWS);
    return 0;
}

// Everything in front of a tile launch, after fc_check and the entry's own pointer checks: the kernel's view of the descriptor, the teams
// and the grid.  workgroups == 0: FC_GRID_ALL workgroups of one team (many per CU).  workgroups > 0, the background form: that many
// workgroups of as many teams as the LDS holds (4 up to 112 rows, 2 up to 240), so that a workgroup keeps a CU's memory pipeline busy alone.
inline int fc_prepare(const char *who, const yolo_fc_factors *d, int workgroups, FcLaunch &L)
{
    if (workgroups < 0) return fail(YOLO_E_ARG, "%s: workgroups = %d is negative", who, workgroups);
    FcTiles &f = L.f;
    f.dy = (const bf16_t *)d->dy; f.x = (const bf16_t *)d->x;
    f.rows = d->rows; f.O = d->O; f.I = d->I; f.ld_dy = d->ld_dy; f.ld_x = d->ld_x;
    f.scale = d->scale;
    f.kpad = (d->rows + FC_KSTEP - 1) / FC_KSTEP * FC_KSTEP;
    f.tiles_i = (d->I + FC_T - 1) / FC_T;
    f.tiles = (long)((d->O + FC_T - 1) / FC_T) * f.tiles_i;
    const unsigned one = 2u * FC_T * (unsigned)(f.kpad + FC_PAD) * (unsigned)sizeof(bf16_t);
    L.teams = workgroups == 0 ? 1 : 4 * one <= FC_LDS_MOST ? 4 : 2 * one <= FC_LDS_MOST ? 2 : 1;
    L.lds = one * (unsigned)L.teams;
    L.grid = (unsigned)std::min<long>(workgroups > 0 ? workgroups : FC_GRID_ALL, (f.tiles + L.teams - 1) / L.teams);
    return 0;
}

// the LDS the kernel `fn` may reserve (lds_done: one flag per device for this kernel)
inline int fc_raise_lds(const char *who, const FcLaunch &L, const void *fn, bool (&lds_done)[64])
{
    if (L.lds <= 48u * 1024u) return 0;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) dev = 0;
    if (!lds_done[dev]) {
        hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)FC_LDS_MOST);
        if (e != hipSuccess) return fail((int)e, "%s: hipFuncSetAttribute(%u B LDS): %s", who, FC_LDS_MOST, hipGetErrorString(e));
        lds_done[dev] = true;
    }
    return 0;
}

// The two step entries' bodies live beside the element ops they apply (optim.hip: AdamOp, sgd.hip: sgd1); fc_factored.hip exports them.
int adam_step_factored(const yolo_fc_factors *d, float *p, float *m, float *v, void *p_bf16, float lr, float beta1, float beta2, float eps,
                       float weight_decay, long step, const double *norm_sq, float max_norm, const float *skip_flag, int workgroups,
                       yolo_stream_t stream);
int sgd_step_factored(const yolo_fc_factors *d, float *p, float *buf, void *p_bf16, float lr, float momentum, float dampening, float weight_decay,
                      int nesterov, int first_step, const double *norm_sq, float max_norm, const float *skip_flag, int workgroups,
                      yolo_stream_t stream);

}  // namespace yolo
