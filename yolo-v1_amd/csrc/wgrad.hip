// Weight-gradient kernel for gfx950:  dw[co][tap][ci] (+)= sum_p dy[p][co] * x[p + tapoff(tap)][ci]
//
// Both operands are K-strided for this product (the reduction index is the pixel, the contiguous
// axis is the channel), so the tiles are staged pixel-major by LDS-DMA exactly as they lie in HBM
// and the MFMA fragments are fetched with gfx950's transposing LDS read (ds_read_b64_tr_b16): no
// transposed copy of an activation is ever written.
//
// "Flat" pixel indexing: p runs over EVERY pixel slot of the zero-haloed dy buffer (halo included).
// dy is exactly zero on its halo, so those slots add nothing, and for a stride-1 conv the matching
// input pixel of tap (ky,kx) is simply p + (ky-pad)*row_stride + (kx-pad): no div/mod, no bounds
// checks, perfectly contiguous 16-B loads.  The price is (H+2)(W+2)/(HW) extra pixels (1.04x at
// 112x112 .. 1.65x at 7x7).  A stride-2 conv runs on a zero-stuffed dy of the input's geometry.
// Callers keep a guard band of zeros (>= row_stride+1 pixels) in front of and behind every
// activation buffer so that shifted reads of halo slots stay inside the allocation.
//
// Tile: 128 co x 128 ci per (tap), 64 pixels per K step, 4 waves (2x2) or 8 (4x2), v_mfma_f32_32x32x16_bf16.
// Split over pixel ranges (blockIdx.y) with fp32 atomics into the packed gradient.
// Also here: the 256 x 128 kernel, the slab / bias sums of the 128 x 128 kernels, the bias-only column sum and
// the host side of yolo_wgrad.  The 7x7 stem has its own kernels (wgrad_stem.hip).
// Replaces the weight-gradient half of aten convolution_backward / addmm backward for
// src/yolo/models.py:47-84,239-245,313-332.
#include "wgrad_common.h"

namespace yolo {

__device__ uint4 g_zero_line[16];  // 256 B of zeros: source for out-of-range rows

// the same instruction from inline asm, invisible to the compiler's LDS alias / waitcnt tracking (wgrad256_kernel);
// lds = wave-uniform LDS byte address of the wave's 1-KB destination
#define DMA16(gptr, lds) \
    asm volatile("s_mov_b32 m0, %1\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, off" ::"v"(gptr), "s"(lds) : "memory", "m0")

constexpr int WG_T = 128;                 // tile edge (co and ci)
constexpr int WG_BP = 64;                 // pixels per K step
constexpr int WG_TILE_BYTES = WG_BP * WG_T * 2;   // 16 KB
constexpr int WG_STAGE_BYTES = 2 * WG_TILE_BYTES; // dy + x; double buffered: 64 KB per workgroup

typedef __attribute__((address_space(3))) s16x4 *lds_s16x4;

// MI = 32-row A (output-channel) fragments of a wave: 2 for a 64 x 64 wave tile, 1 for the 32 x 64 one of the 8-wave 128 x 128 kernel
template <int MI>
struct WFrag {
    bf16x8 a[MI], b[2];
};

// fragments of one 16-pixel sub-step: 2 * MI + 4 transposing reads (rows +4 lie `a_hi` / `b_hi` bytes further), all A pairs first
template <bool BIAS, int MI>
__device__ __forceinline__ void wave_load(const char *sb, const int (&a_rd)[2], const int (&b_rd)[2], int a_off, int a_hi, int b_off, int b_hi, WFrag<MI> &f,
                                          float (&bsum)[MI])
{
#pragma unroll
    for (int t = 0; t < MI; ++t) {
        const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4)(sb + a_rd[t] + a_off));
        const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4)(sb + a_rd[t] + a_off + a_hi));
        f.a[t] = __builtin_bit_cast(bf16x8, __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7));
        if (BIAS) {
#pragma unroll
            for (int e = 0; e < 4; ++e) bsum[t] += __uint_as_float(((unsigned)(unsigned short)lo[e]) << 16) + __uint_as_float(((unsigned)(unsigned short)hi[e]) << 16);
        }
    }
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4)(sb + b_rd[t] + b_off));
        const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4)(sb + b_rd[t] + b_off + b_hi));
        f.b[t] = __builtin_bit_cast(bf16x8, __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7));
    }
}

// one 64-pixel K step of a wave's (32 * MI) x 64 tile, software-pipelined: the reads of sub-step ks+1 are issued in front of
// the MFMAs of sub-step ks.  BIAS is a template flag and the caller branches ONCE per workgroup: a per-lane `if` inside
// this loop splits it into basic blocks and the compiler then waits lgkmcnt(0) in front of every MFMA group.
template <bool BIAS, int A_KS, int A_HI, int B_KS, int B_HI, int MI>
__device__ __forceinline__ void wave_step(const char *sb, const int (&a_rd)[2], const int (&b_rd)[2], f32x16 (&acc)[MI][2], float (&bsum)[MI])
{
    WFrag<MI> cur, nxt;
    wave_load<BIAS>(sb, a_rd, b_rd, 0, A_HI, 0, B_HI, cur, bsum);
#pragma unroll
    for (int ks = 0; ks < WG_BP / 16; ++ks) {
        if (ks + 1 < WG_BP / 16) wave_load<BIAS>(sb, a_rd, b_rd, (ks + 1) * A_KS, A_HI, (ks + 1) * B_KS, B_HI, nxt, bsum);
#pragma unroll
        for (int i = 0; i < MI; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(cur.a[i], cur.b[j], acc[i][j], 0, 0, 0);
        cur = nxt;
    }
}

// The 128 x 128 kernel with NW = 4 waves (2 x 2, a wave owns 64 co x 64 ci: yolo_wgrad_desc.variant 0 / 1) or NW = 8 (4 x 2, a wave owns
// 32 co x 64 ci, one A fragment and two B fragments per 16-pixel sub-step: variant 4).  The 8-wave form puts four waves on a SIMD with two
// resident workgroups -- more waves to cover the per-step LDS latency and barrier, at 1.5x the fragment reads per MFMA.
template <int NW>
__global__ void __launch_bounds__(64 * NW, 2) wgrad_kernel(const WgradParams p)
{
    constexpr int NTHR = 64 * NW;
    constexpr int NPC = 16 / NW;       // 1-KB LDS-DMA pieces per wave, operand and stage
    constexpr int ROWS = 256 / NW;     // output-channel rows per wave
    constexpr int MI = ROWS / 32;      // A fragments per sub-step
    constexpr int WPH = 64 / ROWS;     // waves (along co) that share one 64-row half of the epilogue
    // Two SEPARATE LDS objects, one per pipeline stage, and a K loop unrolled by two so that every
    // access names its stage statically: hipcc then knows the LDS-DMA writes of stage t+1 cannot alias
    // the transposing reads of stage t and does not drain vmcnt(0) in front of the first ds_read
    // (with one array and a runtime stage index it serialised load and compute).
    __shared__ __attribute__((aligned(16))) char bufA[WG_STAGE_BYTES];
    __shared__ __attribute__((aligned(16))) char bufB[WG_STAGE_BYTES];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wco = wave >> 1, wci = wave & 1;

    const int ntap_tiles = p.pair_taps ? (p.ntaps + 1) / 2 : p.ntaps;
    const int nwg = p.n_co_tiles * p.n_ci_tiles * ntap_tiles;
    int bid;
    long pbeg, pend;
    bool atomic;
    int part;
    wgrad_map(p, nwg, bid, pbeg, pend, atomic, part);
    if (pbeg >= pend) return;   // empty range of a rounded-up split (the whole workgroup leaves)
    // co-tile fastest, then ci-tile, then tap: neighbours share the x tile of one tap
    const int co_tile = bid % p.n_co_tiles;
    const int rest = bid / p.n_co_tiles;
    const int ci_tile = rest % p.n_ci_tiles;
    const int tap_tile = rest / p.n_ci_tiles;
    const int tap = p.pair_taps ? 2 * tap_tile : tap_tile;          // first (or only) tap of this tile
    const int ky = tap / p.KW, kx = tap - ky * p.KW;
    const long tap_off = (long)(ky - p.pad) * p.x_row_stride + (long)(kx - p.pad) * p.x_px_stride;
    const int ky2 = (tap + 1) / p.KW, kx2 = (tap + 1) - ky2 * p.KW;   // pair mode: the tap of tile columns 64..127
    const long tap_off2 = (long)(ky2 - p.pad) * p.x_row_stride + (long)(kx2 - p.pad) * p.x_px_stride;
    const bool tap2_ok = tap + 1 < p.ntaps;
    const int co0 = co_tile * WG_T, ci0 = ci_tile * WG_T;
    // columns of this tile that exist in dw[co][tap][ci]
    const int col_lim = p.pair_taps ? (tap2_ok ? 2 * p.Cin : p.Cin) : p.Cin - ci0;


    // ---- LDS-DMA sources.  A wave-instruction covers 4 pixel rows x 256 B.  Slot (row, c') holds
    // data chunk c = c' ^ ((row&3)<<2): the transposing reads of one 32-lane half then touch 16
    // distinct 16-B slots of the 256-B bank row (conflict-free).
    int row_of[NPC], a_coff[NPC], b_coff[NPC];
    bool b_second[NPC];
#pragma unroll
    for (int i = 0; i < NPC; ++i) {
        const int pos = (i * NW + wave) * 64 + lane;
        const int row = pos >> 4, cs = pos & 15;
        const int c = cs ^ ((row & 3) << 2);
        row_of[i] = row;
        int ca = co0 / 8 + c, cb = ci0 / 8 + c;
        if (ca >= p.Cout_ld / 8) ca = p.Cout_ld / 8 - 1;
        b_second[i] = false;
        if (p.pair_taps) {                      // chunks 0..7 -> tap, 8..15 -> tap + 1 (Cin == 64: 8 chunks per tap)
            b_second[i] = c >= 8;
            cb = c & 7;
        }
        if (cb >= p.Cin_ld / 8) cb = p.Cin_ld / 8 - 1;
        a_coff[i] = ca * 8;
        b_coff[i] = cb * 8;
    }
    const bf16_t *zline = reinterpret_cast<const bf16_t *>(g_zero_line) + (lane & 15) * 8;

    // slot[i]: buffer slot of the lane's i-th pixel row in the NEXT stage to be issued (-1: past the range -> zeros).
    // With a pixel index the lookups for stage t+1 are issued right behind the LDS-DMA of stage t and have a whole K
    // step to arrive.
    // (n0, oy0, ox0) = pixel coordinates of the first row of the NEXT stage to issue, carried in scalars; a lane's rows lie
    // < 64 pixels further, so their coordinates follow with two multiply-high "small divisions" each -- no index table, no
    // extra memory instruction (a table cost 7-17 % on the 56x56 / 112x112 layers, whichever way it was read).
    int n0 = 0, oy0 = 0, ox0 = 0;
    if (p.gW) {
        const long row = pbeg / p.gW;
        ox0 = (int)(pbeg - row * p.gW);
        n0 = (int)(row / p.gH);
        oy0 = (int)(row - (long)n0 * p.gH);
    }
    auto stage = [&](char *sb, long pb) {
#pragma unroll
        for (int i = 0; i < NPC; ++i) {
            const long pr = pb + row_of[i];
            long slot;
            if (p.gW) {
                const unsigned a = (unsigned)(ox0 + row_of[i]);
                const unsigned qx = __umulhi(a, p.mW);
                const unsigned b = (unsigned)oy0 + qx;
                const unsigned qy = __umulhi(b, p.mH);
                slot = (long)(n0 + (int)qy) * p.g_img + (int)(b - qy * p.gH) * p.g_row + (int)(a - qx * p.gW) * p.g_px + p.g_off;
            } else {
                slot = pr;
            }
            const bool ok = pr < pend;
            const bf16_t *sa = ok ? p.dy + slot * p.dy_px_stride + a_coff[i] : zline;
            const bf16_t *sx = (ok && !(b_second[i] && !tap2_ok)) ? p.x + slot * p.x_px_stride + (b_second[i] ? tap_off2 : tap_off) + b_coff[i] : zline;
            GLDS16(sa, sb + (i * NW + wave) * 1024);
            GLDS16(sx, sb + WG_TILE_BYTES + (i * NW + wave) * 1024);
        }
        if (p.gW) {   // advance the scalar coordinates by one stage (64 pixels)
            const unsigned a = (unsigned)(ox0 + WG_BP);
            const unsigned qx = __umulhi(a, p.mW);
            const unsigned b = (unsigned)oy0 + qx;
            const unsigned qy = __umulhi(b, p.mH);
            ox0 = (int)(a - qx * p.gW);
            oy0 = (int)(b - qy * p.gH);
            n0 += (int)qy;
        }
    };

    // ---- transposing fragment reads (see header): group g = lane>>4, q = (lane>>2)&3, pp = lane&3
    const int g = lane >> 4, q = (lane >> 2) & 3, pp = lane & 3;
    int a_rd[2], b_rd[2];     // a_rd[1] is unused with MI = 1
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        const int row = (g >> 1) * 8 + q;
        const int ca = (wco * ROWS + t * 32 + (g & 1) * 16 + 4 * pp) >> 3;
        const int cb = (wci * 64 + t * 32 + (g & 1) * 16 + 4 * pp) >> 3;
        a_rd[t] = row * 256 + ((ca ^ ((row & 3) << 2)) << 4) + (pp & 1) * 8;
        b_rd[t] = WG_TILE_BYTES + row * 256 + ((cb ^ ((row & 3) << 2)) << 4) + (pp & 1) * 8;
    }

    f32x16 acc[MI][2];
#pragma unroll
    for (int i = 0; i < MI; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.0f;

    // bias gradient rides along: the dy fragments of the (tap 0, ci-tile 0) workgroups cover every
    // (pixel, co) exactly once over the grid, so summing them costs no extra HBM pass
    const bool do_bias = p.db != nullptr && tap == 0 && ci_tile == 0 && wci == 0;
    float bsum[MI] = {};

    auto run = [&](auto bias_tag) {
        constexpr bool BIAS = decltype(bias_tag)::value;
        stage(bufA, pbeg);
        for (long pb = pbeg; pb < pend; pb += 2 * WG_BP) {
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __syncthreads();  // stage A landed for every wave; stage B is free
            if (pb + WG_BP < pend) stage(bufB, pb + WG_BP);
            wave_step<BIAS, 4096, 1024, 4096, 1024>(bufA, a_rd, b_rd, acc, bsum);
            if (pb + WG_BP >= pend) break;
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __syncthreads();
            if (pb + 2 * WG_BP < pend) stage(bufA, pb + 2 * WG_BP);
            wave_step<BIAS, 4096, 1024, 4096, 1024>(bufB, a_rd, b_rd, acc, bsum);
        }
    };
    if (do_bias) run(std::true_type{});
    else run(std::false_type{});

    if (do_bias) {
#pragma unroll
        for (int t = 0; t < MI; ++t) {
            const float tot = bsum[t] + __shfl_xor(bsum[t], 32, 64);  // the two k-halves of each co row
            const int co = co0 + wco * ROWS + t * 32 + (lane & 31);
            if (lane < 32 && co < p.Cout) {
                if (p.bias_part) p.bias_part[(long)co * p.bias_ld + wgrad_range(p, bid, part)] = tot;   // slab mode: summed in range order afterwards
                else atomicAdd(p.db + co, tot);
            }
        }
    }

    // ---- output through LDS, one half of the co rows at a time ([64 co][128 ci] fp32 = stage A): the accumulator layout
    // (row = (reg&3) + 8*(reg>>2) + 4*(lane>>5), col = lane&31) would give 4-B stores / atomics in 128-B pieces; from LDS
    // a wave-instruction covers 1 KB of one dw row as 16-B stores, or 256 contiguous bytes per atomic instruction.
    const long ldw = (long)p.ntaps * p.Cin;
    float *ot = reinterpret_cast<float *>(bufA);
    const bool vec_ok = !atomic && (p.Cin & 3) == 0 && ((uintptr_t)p.dw & 15) == 0;
    float *slab = (atomic && p.slabs) ? p.slabs + wgrad_slab_index(p, part) * (WG_T * WG_T) : nullptr;
    [[maybe_unused]] float ssq = 0.0f;   // p.sumsq (4 waves only): squares of the values this thread stores (the host requires the vector store path for it)
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        __syncthreads();   // (first pass: every wave is done reading the stage buffers)
        if (wco / WPH == h) {      // this wave's rows lie in half h, (wco % WPH) * ROWS rows down
#pragma unroll
            for (int i = 0; i < MI; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j)
#pragma unroll
                    for (int r = 0; r < 16; ++r)
                        ot[((wco % WPH) * ROWS + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5)) * WG_T + wci * 64 + j * 32 + (lane & 31)] = acc[i][j][r];
        }
        __syncthreads();
        if (slab) {
            // slab mode, split tile: the whole 128 x 128 partial, dense, as 16-B stores (wgrad_slab_sum128_kernel adds them in range order)
#pragma unroll
            for (int it = 0; it < 2048 / NTHR; ++it) {
                const int idx = it * NTHR + tid, row = idx >> 5, c4 = (idx & 31) * 4;
                *reinterpret_cast<float4 *>(slab + (h * 64 + row) * WG_T + c4) = *reinterpret_cast<const float4 *>(ot + row * WG_T + c4);
            }
        } else if (vec_ok) {
#pragma unroll
            for (int it = 0; it < 2048 / NTHR; ++it) {
                const int idx = it * NTHR + tid, row = idx >> 5, c4 = (idx & 31) * 4;
                const int co = co0 + h * 64 + row, ci = ci0 + c4;
                if (co < p.Cout && c4 < col_lim) {   // Cin % 4 == 0: a quad is inside or outside as a whole
                    const float4 v = *reinterpret_cast<const float4 *>(ot + row * WG_T + c4);
                    *reinterpret_cast<float4 *>(p.dw + (long)co * ldw + (long)tap * p.Cin + ci) = v;
                    if constexpr (NW == 4) ssq += (v.x * v.x + v.y * v.y) + (v.z * v.z + v.w * v.w);
                }
            }
        } else {
#pragma unroll 4
            for (int it = 0; it < 8192 / NTHR; ++it) {
                const int idx = it * NTHR + tid, row = idx >> 7, c = idx & 127;
                const int co = co0 + h * 64 + row, ci = ci0 + c;
                if (co < p.Cout && c < col_lim) {
                    float *o = p.dw + (long)co * ldw + (long)tap * p.Cin + ci;
                    const float v = ot[row * WG_T + c];
                    if (atomic) atomicAdd(o, v);
                    else *o = v;
                }
            }
        }
    }
    if constexpr (NW == 4) {
        if (p.sumsq) {       // wave-uniform branch; one fp64 atomic per workgroup
            double s = (double)ssq;
            for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off, 64);
            __syncthreads();
            double *wsum = reinterpret_cast<double *>(bufA);
            if (lane == 0) wsum[wave] = s;
            __syncthreads();
            if (tid == 0) atomicAdd(p.sumsq, wsum[0] + wsum[1] + wsum[2] + wsum[3]);
        }
    }
}

// ---------------------------------------------------------------------------------------------------
// 256 co x 128 ci variant, 8 waves (4 x 2, the same 64 x 64 wave tile), THREE 48-KB stages.
// The 128 x 128 kernel above keeps at most one 32-KB stage per workgroup in flight (two workgroups per
// CU): a K step computes for ~0.45 us while a stage takes 1.5-2 us to arrive, so the loop runs at the
// LDS-DMA latency, not at the MFMA rate (measured 31 % of peak on the 3x3 layers).  Here two stages
// (96 KB per CU) are in flight behind the one being consumed and every byte staged feeds twice the
// MFMA work; waits are counted (vmcnt(6) = "everything but the newest stage") and the barrier is the
// raw s_barrier, so a wave never drains the queue.  One static LDS array per stage + a loop unrolled by
// three keep every access's stage static (see the note in wgrad_kernel).
constexpr int W2_TCO = 256, W2_TCI = 128;
constexpr int W2_A_BYTES = WG_BP * W2_TCO * 2;     // 32 KB
constexpr int W2_B_BYTES = WG_BP * W2_TCI * 2;     // 16 KB
constexpr int W2_STAGE = W2_A_BYTES + W2_B_BYTES;  // 48 KB

template <bool STG>
__global__ void __launch_bounds__(512, 1) wgrad256_kernel(const WgradParams p)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];   // 3 stages x 48 KB
    const unsigned lds0 = (unsigned)(uintptr_t)(__attribute__((address_space(3))) char *)smem;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wco = wave >> 1, wci = wave & 1;

    const int nwg = p.n_co_tiles * p.n_ci_tiles * p.ntaps;
    int bid;
    long pbeg, pend;
    bool atomic;
    int part_unused;
    wgrad_map(p, nwg, bid, pbeg, pend, atomic, part_unused);
    if (pbeg >= pend) return;   // empty range of a rounded-up split (the whole workgroup leaves)
    const int co_tile = bid % p.n_co_tiles;
    const int rest = bid / p.n_co_tiles;
    const int ci_tile = rest % p.n_ci_tiles;
    const int tap = rest / p.n_ci_tiles;
    const int ky = tap / p.KW, kx = tap - ky * p.KW;
    const long tap_off = (long)(ky - p.pad) * p.x_row_stride + (long)(kx - p.pad) * p.x_px_stride;
    const int co0 = co_tile * W2_TCO, ci0 = ci_tile * W2_TCI;


    // ---- LDS-DMA sources: dy rows are 512 B (2 pixel rows per wave-instruction), x rows 256 B (4 per instruction);
    // slot (row, c') holds chunk c = c' ^ ((row&3)<<2) in both (see wgrad_kernel)
    int a_row[4], a_coff[4], b_row[2], b_coff[2];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int pos = (i * 8 + wave) * 64 + lane;
        const int row = pos >> 5, cs = pos & 31;
        int ca = co0 / 8 + (cs ^ ((row & 3) << 2));
        if (ca >= p.Cout_ld / 8) ca = p.Cout_ld / 8 - 1;
        a_row[i] = row;
        a_coff[i] = ca * 8;
    }
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int pos = (i * 8 + wave) * 64 + lane;
        const int row = pos >> 4, cs = pos & 15;
        int cb = ci0 / 8 + (cs ^ ((row & 3) << 2));
        if (cb >= p.Cin_ld / 8) cb = p.Cin_ld / 8 - 1;
        b_row[i] = row;
        b_coff[i] = cb * 8;
    }
    const bf16_t *zline = reinterpret_cast<const bf16_t *>(g_zero_line) + (lane & 15) * 8;

    auto stage = [&](int st, long pb) {
        const unsigned sb = lds0 + st * W2_STAGE;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const long pr = pb + a_row[i];
            const bf16_t *sa = pr < pend ? p.dy + pr * p.dy_px_stride + a_coff[i] : zline;
            DMA16(sa, sb + (i * 8 + wave) * 1024);
        }
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const long pr = pb + b_row[i];
            const bf16_t *sx = pr < pend ? p.x + pr * p.x_px_stride + tap_off + b_coff[i] : zline;
            DMA16(sx, sb + W2_A_BYTES + (i * 8 + wave) * 1024);
        }
    };

    const int g = lane >> 4, q = (lane >> 2) & 3, pp = lane & 3;
    int a_rd[2], b_rd[2];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        const int row = (g >> 1) * 8 + q;
        const int ca = (wco * 64 + t * 32 + (g & 1) * 16 + 4 * pp) >> 3;
        const int cb = (wci * 64 + t * 32 + (g & 1) * 16 + 4 * pp) >> 3;
        a_rd[t] = row * 512 + ((ca ^ ((row & 3) << 2)) << 4) + (pp & 1) * 8;
        b_rd[t] = W2_A_BYTES + row * 256 + ((cb ^ ((row & 3) << 2)) << 4) + (pp & 1) * 8;
    }

    f32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.0f;

    const bool do_bias = p.db != nullptr && tap == 0 && ci_tile == 0 && wci == 0;
    float bsum[2] = {0.0f, 0.0f};

    // The LDS-DMA is issued from inline asm (DMA16): hipcc's own waitcnt pass otherwise drains vmcnt(0) in front of the
    // first transposing read of every loop iteration (it cannot bound the age of the stage being read across the
    // back-edge), which empties the pipeline every third step.  So ordering is all explicit here: wait until only the
    // newest stage (6 instructions per wave) may still be in flight, meet the other waves, and fence the compiler.
#define W2_SYNC(more)                                                 \
    do {                                                              \
        if (more) asm volatile("s_waitcnt vmcnt(6)" ::: "memory");    \
        else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");         \
        __builtin_amdgcn_s_barrier();                                 \
        asm volatile("" ::: "memory");                                \
    } while (0)

    const long nsteps = pbeg < pend ? (pend - pbeg + WG_BP - 1) / WG_BP : 0;
    auto run = [&](auto bias_tag) {
        constexpr bool BIAS = decltype(bias_tag)::value;
        if constexpr (STG) {
            // ---- staggered two-phase schedule (the one of igemm.hip's MFMA_16x16x32_STAGGER): every K step is an L phase (all
            // 32 transposing reads of the step -> registers) and an M phase (its 16 MFMAs) between raw barriers; waves 0..3 and
            // 4..7 sit pairwise on the same SIMDs and run ONE PHASE APART, so one wave feeds the matrix pipe while its partner
            // reads LDS.  Stage s is issued by everybody in slot 2(s-2) and drained (counted vmcnt) at the end of slot 2s-1.
            auto read_all = [&](int st, WFrag<2> (&f)[4]) {
#pragma unroll
                for (int ks = 0; ks < 4; ++ks) wave_load<BIAS>(smem + st * W2_STAGE, a_rd, b_rd, ks * 8192, 2048, ks * 4096, 1024, f[ks], bsum);
            };
            auto mfma_all = [&](WFrag<2> (&f)[4]) {
#pragma unroll
                for (int ks = 0; ks < 4; ++ks)
#pragma unroll
                    for (int i = 0; i < 2; ++i)
#pragma unroll
                        for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(f[ks].a[i], f[ks].b[j], acc[i][j], 0, 0, 0);
            };
            auto wait_stage = [&](long newer) {   // newer = younger stages this wave has already issued
                if (newer >= 1) asm volatile("s_waitcnt vmcnt(6)" ::: "memory");
                else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            };
#define W2_BAR()                                   \
    do {                                           \
        __builtin_amdgcn_sched_barrier(0);         \
        __builtin_amdgcn_s_barrier();              \
        __builtin_amdgcn_sched_barrier(0);         \
    } while (0)
            const bool grpB = wave >= 4;
            const long nkk = nsteps;
            if (nkk > 0) stage(0, pbeg);
            if (nkk > 1) stage(1, pbeg + WG_BP);
            wait_stage(nkk - 1 < 1 ? nkk - 1 : 1);
            W2_BAR();
            WFrag<2> f[4];
            int rd = 0;
            if (!grpB) {
                int ld = 2;
                for (long it = 0; it < nkk; ++it) {
                    read_all(rd, f);                                                    // L(it)
                    if (it + 2 < nkk) stage(ld, pbeg + (it + 2) * WG_BP);
                    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                    W2_BAR();
                    __builtin_amdgcn_s_setprio(1);
                    mfma_all(f);                                                        // M(it)
                    __builtin_amdgcn_s_setprio(0);
                    { const long left = nkk - 2 - it; wait_stage(left < 0 ? 0 : left); }   // stage it+1 landed
                    W2_BAR();
                    rd = rd + 1 == 3 ? 0 : rd + 1;
                    ld = ld + 1 == 3 ? 0 : ld + 1;
                }
                __builtin_amdgcn_s_barrier();
            } else {
                if (2 < nkk) stage(2, pbeg + 2 * WG_BP);                                // slot 0
                W2_BAR();
                int ld = 0;
                for (long it = 0; it < nkk; ++it) {
                    read_all(rd, f);                                                    // L(it)
                    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                    { const long left = nkk - 2 - it; wait_stage(left < 0 ? 0 : left); }
                    W2_BAR();
                    if (it + 3 < nkk) stage(ld, pbeg + (it + 3) * WG_BP);               // M(it)
                    __builtin_amdgcn_s_setprio(1);
                    mfma_all(f);
                    __builtin_amdgcn_s_setprio(0);
                    W2_BAR();
                    rd = rd + 1 == 3 ? 0 : rd + 1;
                    ld = ld + 1 == 3 ? 0 : ld + 1;
                }
            }
#undef W2_BAR
        } else {
        if (nsteps > 0) stage(0, pbeg);
        if (nsteps > 1) stage(1, pbeg + WG_BP);
        for (long t = 0; t < nsteps; t += 3) {
            W2_SYNC(t + 1 < nsteps);
            if (t + 2 < nsteps) stage(2, pbeg + (t + 2) * WG_BP);
            wave_step<BIAS, 8192, 2048, 4096, 1024>(smem, a_rd, b_rd, acc, bsum);
            if (t + 1 >= nsteps) break;
            W2_SYNC(t + 2 < nsteps);
            if (t + 3 < nsteps) stage(0, pbeg + (t + 3) * WG_BP);
            wave_step<BIAS, 8192, 2048, 4096, 1024>(smem + W2_STAGE, a_rd, b_rd, acc, bsum);
            if (t + 2 >= nsteps) break;
            W2_SYNC(t + 3 < nsteps);
            if (t + 4 < nsteps) stage(1, pbeg + (t + 4) * WG_BP);
            wave_step<BIAS, 8192, 2048, 4096, 1024>(smem + 2 * W2_STAGE, a_rd, b_rd, acc, bsum);
        }
        }
    };
    if (do_bias) run(std::true_type{});
    else run(std::false_type{});
#undef W2_SYNC

    if (do_bias) {
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            const float tot = bsum[t] + __shfl_xor(bsum[t], 32, 64);
            const int co = co0 + wco * 64 + t * 32 + (lane & 31);
            if (lane < 32 && co < p.Cout) atomicAdd(p.db + co, tot);
        }
    }
    const long ldw = (long)p.ntaps * p.Cin;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int ci = ci0 + wci * 64 + j * 32 + (lane & 31);
            if (ci >= p.Cin) continue;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int co = co0 + wco * 64 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
                if (co >= p.Cout) continue;
                float *o = p.dw + (long)co * ldw + (long)tap * p.Cin + ci;
                if (atomic) atomicAdd(o, acc[i][j][r]);
                else *o = acc[i][j][r];
            }
        }
}

// Slab mode of the 128 x 128 kernels: sum of a split tile's dense partials into the packed gradient dw[co][tap][ci], in pixel-range order
// (fixed: the result does not depend on the order in which the workgroups ran).  One thread = 4 consecutive columns of one tile row;
// grid = (16, tiles).  A tile of an unsplit segment was stored by its one workgroup and is left alone.  `atomic` = WgradParams.atomic
// (bit 0 / 1: main / tail segment is split); uniform split: main_tiles = every tile, main_split = the ranges.
__global__ void __launch_bounds__(256) wgrad_slab_sum128_kernel(const float *__restrict__ slabs, float *__restrict__ dw, int Cout, int Cin, int ntaps, int n_co_tiles,
                                                                int n_ci_tiles, int pair_taps, int atomic, int main_tiles, int main_split, int tail_split,
                                                                int main_ranges, int tail_ranges)
{
    const int bid = blockIdx.y;
    const bool tail = bid >= main_tiles;
    if (!((atomic >> (tail ? 1 : 0)) & 1)) return;
    const int idx = blockIdx.x * 256 + threadIdx.x;               // float4 inside the tile: row = idx / 32
    const int row = idx >> 5, c4 = (idx & 31) * 4;
    const int co_tile = bid % n_co_tiles, rest = bid / n_co_tiles;
    const int ci_tile = rest % n_ci_tiles, tap_tile = rest / n_ci_tiles;
    const int tap = pair_taps ? 2 * tap_tile : tap_tile;
    const int ci0 = ci_tile * WG_T;
    const int col_lim = pair_taps ? (tap + 1 < ntaps ? 2 * Cin : Cin) : Cin - ci0;
    const int co = co_tile * WG_T + row;
    if (co >= Cout || c4 >= col_lim) return;
    const long first = tail ? ((atomic & 1) ? (long)main_tiles * main_split : 0L) + (long)(bid - main_tiles) * tail_split : (long)bid * main_split;
    const int n = tail ? tail_ranges : main_ranges;
    const float *src = slabs + first * (WG_T * WG_T) + row * WG_T + c4;
    float4 a = *reinterpret_cast<const float4 *>(src);
    for (int r = 1; r < n; ++r) {
        const float4 b = *reinterpret_cast<const float4 *>(src + (long)r * (WG_T * WG_T));
        a.x += b.x; a.y += b.y; a.z += b.z; a.w += b.w;
    }
    *reinterpret_cast<float4 *>(dw + (long)co * ntaps * Cin + (long)tap * Cin + ci0 + c4) = a;
}

// Slab mode, bias gradient: db[co] = sum over the pixel ranges r of part[co * ld + r], in range order (plain store: db need not be zero).
// The partials come from the (tap 0, ci-tile 0) workgroups, whose tile number is their co tile.
__global__ void __launch_bounds__(256) wgrad_bias_sum_kernel(const float *__restrict__ part, long ld, int Cout, int tile_co, int main_tiles, int main_ranges,
                                                             int tail_ranges, float *__restrict__ db)
{
    const int co = blockIdx.x * 256 + threadIdx.x;
    if (co >= Cout) return;
    const int n = co / tile_co >= main_tiles ? tail_ranges : main_ranges;
    const float *src = part + (long)co * ld;
    float s = src[0];
    for (int r = 1; r < n; ++r) s += src[r];
    db[co] = s;
}

// db[c] += sum_p dy[p][c]  (bias gradient).  HBM-bound column sum: a workgroup covers w <= 256
// 8-channel chunks (one 16-B load per thread) x R = 256/w pixel rows per pass, so every wave reads
// whole contiguous pixel rows whatever the channel count; LDS reduction over R, one fp32 atomic per
// channel per workgroup.
__global__ void __launch_bounds__(256) colsum_kernel(const bf16_t *__restrict__ dy, long P, int px_stride, int C, int w, long p_per_blk, float *__restrict__ db)
{
    const int nchunks = (C + 7) >> 3;
    const int R = 256 / w;
    const int col = threadIdx.x % w, r = threadIdx.x / w;
    const int c8 = blockIdx.x * w + col;
    // grid-stride over pixel rows: all workgroups sweep the buffer together (DRAM-page friendly),
    // 4 independent 16-B loads in flight per thread
    const long step = (long)gridDim.y * R;
    float s[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    auto acc8 = [&](const uint4 &v) {
        s[0] += __uint_as_float(v.x << 16); s[1] += __uint_as_float(v.x & 0xffff0000u);
        s[2] += __uint_as_float(v.y << 16); s[3] += __uint_as_float(v.y & 0xffff0000u);
        s[4] += __uint_as_float(v.z << 16); s[5] += __uint_as_float(v.z & 0xffff0000u);
        s[6] += __uint_as_float(v.w << 16); s[7] += __uint_as_float(v.w & 0xffff0000u);
    };
    if (r < R && c8 < nchunks) {
        const bf16_t *base = dy + c8 * 8;
        long pr = (long)blockIdx.y * R + r;
        for (; pr + 3 * step < P; pr += 4 * step) {
            const uint4 v0 = *reinterpret_cast<const uint4 *>(base + pr * px_stride);
            const uint4 v1 = *reinterpret_cast<const uint4 *>(base + (pr + step) * px_stride);
            const uint4 v2 = *reinterpret_cast<const uint4 *>(base + (pr + 2 * step) * px_stride);
            const uint4 v3 = *reinterpret_cast<const uint4 *>(base + (pr + 3 * step) * px_stride);
            acc8(v0); acc8(v1); acc8(v2); acc8(v3);
        }
        for (; pr < P; pr += step) acc8(*reinterpret_cast<const uint4 *>(base + pr * px_stride));
    }
    __shared__ float red[256][9];
#pragma unroll
    for (int k = 0; k < 8; ++k) red[threadIdx.x][k] = s[k];
    __syncthreads();
    if (r == 0 && c8 < nchunks) {
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            float t = 0.0f;
            for (int rr = 0; rr < R; ++rr) t += red[rr * w + col][k];
            if (c8 * 8 + k < C) atomicAdd(db + c8 * 8 + k, t);
        }
    }
}

int wgrad_bias_sum_launch(const WgradParams &p, int tile_co, int main_ranges, int tail_ranges, float *db, hipStream_t s)
{
    hipLaunchKernelGGL(wgrad_bias_sum_kernel, dim3((unsigned)((p.Cout + 255) / 256)), dim3(256), 0, s, (const float *)p.bias_part, p.bias_ld, p.Cout, tile_co,
                       p.main_tiles, main_ranges, tail_ranges, db);
    return check_launch("yolo_wgrad (bias sum)");
}

}  // namespace yolo

using namespace yolo;

// One yolo_wgrad launch with dw, as the host decides it.  wgrad_run fills it in four steps, in this order; a refusal never moves in front
// of one of an earlier step (tests/wgrad_cases.py states the order).
struct WgradLaunch {
    WgradParams p;
    // tile family.  big: 256 x 128 (variant 2; 3: + staggered two-phase schedule), 8 waves and 3 stages, only on request: measured no faster than
    // two co-resident 128 x 128 workgroups on any layer of the model.  pipe: 256 x 256, register-pipelined loop (variant 5, wgrad_pipe.hip: eight
    // waves of 128 x 64; 6, wgrad_wide.hip: four waves of 128 x 128).  Neither: 128 x 128 (variants 0 / 1: four waves, 4: eight)
    bool big, pipe;
    int tiles;
    dim3 grid;
    int main_ranges, tail_ranges;   // pixel ranges of a main / tail tile that hold pixels (uniform split: every tile is a main tile)
    long need;                      // slab mode: floats this launch needs (yolo_wgrad_slab_floats)
    long bias_at, bias_ld;          // 128 x 128 kernels: the [co][range] bias partials lie behind the tile partials, bias_ld ranges per row
};

// Step 1: validation of the descriptor, the tile family, its tile counts and taps per tile
static int wgrad_fill(const yolo_wgrad_desc *d, const void *x, const void *dy, float *dw, float *db, WgradLaunch &w)
{
    WgradParams &p = w.p;
    p.x = (const bf16_t *)x; p.dy = (const bf16_t *)dy; p.dw = dw; p.db = db;
    p.P = d->P;
    w.big = d->variant == 2 || d->variant == 3;
    w.pipe = d->variant == 5 || d->variant == 6;
    if (d->geo_W < 0 || d->geo_H < 0 || (d->geo_W > 0 && (d->geo_H <= 0 || d->geo_W > 65536 || d->geo_H > 65536)))
        return fail(YOLO_E_ARG, "yolo_wgrad: bad pixel geometry %d x %d", d->geo_W, d->geo_H);
    if (d->geo_W > 0) {
        if (w.big) return fail(YOLO_E_UNSUPPORTED, "yolo_wgrad: the 256x128 variants have no pixel-geometry mode");
        if (d->P % ((long)d->geo_W * d->geo_H)) return fail(YOLO_E_ARG, "yolo_wgrad: P = %ld is not a whole number of %d x %d images", (long)d->P, d->geo_W, d->geo_H);
        p.gW = d->geo_W; p.gH = d->geo_H;
        p.g_img = d->geo_img_slots; p.g_row = d->geo_row_slots; p.g_px = d->geo_px_slots; p.g_off = d->geo_slot0;
        p.mW = (unsigned)(((1ull << 32) + d->geo_W - 1) / d->geo_W);   // 2^32 for W = 1 wraps to 0: handled by W == 1 -> q = a
        p.mH = (unsigned)(((1ull << 32) + d->geo_H - 1) / d->geo_H);
        if (d->geo_W == 1 || d->geo_H == 1) return fail(YOLO_E_UNSUPPORTED, "yolo_wgrad: pixel geometry needs W, H >= 2 (use flat indexing)");
    }
    p.dy_px_stride = d->dy_px_stride; p.x_px_stride = d->x_px_stride;
    p.Cout = d->Cout; p.Cin = d->Cin;
    p.Cout_ld = (int)((std::min<long>(d->dy_px_stride, ((long)d->Cout + 7) & ~7L)));
    p.Cin_ld = (int)((std::min<long>(d->x_px_stride, ((long)d->Cin + 7) & ~7L)));
    p.KH = d->KH; p.KW = d->KW; p.pad = d->pad; p.x_row_stride = d->x_row_stride;
    p.ntaps = d->KH * d->KW;
    p.tile_taps = 1;
    if (w.pipe) {
        // 32-bit byte offsets from the operand bases, 24-bit slot arithmetic; a pixel range that ends inside a 32-pixel stage
        // reads halo slot 0 for the missing rows, which a Linear layer's operands (no halo) do not have
        const long max_slot = d->geo_W > 0 ? (d->P / ((long)d->geo_W * d->geo_H)) * (long)d->geo_img_slots + d->geo_slot0 : d->P;
        if (max_slot >= (1L << 24) || max_slot * (long)std::max(d->dy_px_stride, d->x_px_stride) * 2 + 4 * (long)d->pad * (d->x_row_stride + d->x_px_stride) >= (1L << 32)
            || d->dy_px_stride >= (1 << 23) || d->x_px_stride >= (1 << 23))
            return fail(YOLO_E_UNSUPPORTED, "yolo_wgrad: variant 5 addresses operands below 4 GB with fewer than 2^24 pixel slots");
        if (d->geo_W == 0 && d->pad == 0 && d->KH * d->KW == 1 && (d->P % 32))
            return fail(YOLO_E_UNSUPPORTED, "yolo_wgrad: variant 5 needs zero-haloed operands or P %% 32 == 0");
        // taps per tile: the kernels place a tap's columns as whole 16-B chunks (Cin / 8 per tap), so Cin must be a multiple of 8 --
        // Cin in {8, 16, 32, 64, 128}; Cin in {1, 2, 4} would divide by zero chunks per tap and takes one tap per tile like any other Cin
        p.tile_taps = (d->Cin < 256 && 256 % d->Cin == 0 && d->Cin % 8 == 0 && p.ntaps > 1 && d->x_px_stride >= d->Cin) ? 256 / d->Cin : 1;
        p.n_co_tiles = (d->Cout + 255) / 256;
        p.n_ci_tiles = p.tile_taps > 1 ? 1 : (d->Cin + 255) / 256;
        w.tiles = p.n_co_tiles * p.n_ci_tiles * ((p.ntaps + p.tile_taps - 1) / p.tile_taps);
    } else {
        // 128 x 128 kernels, Cin == 64 with several taps (the 64 -> 192 3x3 layer): two taps per 128-column tile instead of half-empty tiles
        p.pair_taps = ((d->variant <= 1 || d->variant == 4) && d->Cin == 64 && p.ntaps > 1 && d->x_px_stride >= 64) ? 1 : 0;
        p.n_co_tiles = w.big ? (d->Cout + W2_TCO - 1) / W2_TCO : (d->Cout + WG_T - 1) / WG_T;
        p.n_ci_tiles = (d->Cin + WG_T - 1) / WG_T;
        w.tiles = p.n_co_tiles * p.n_ci_tiles * (p.pair_taps ? (p.ntaps + 1) / 2 : p.ntaps);
    }
    return 0;
}

// Step 2: the split over pixel ranges -> grid and p.atomic
static void wgrad_schedule(const yolo_wgrad_desc *d, WgradLaunch &w)
{
    WgradParams &p = w.p;
    const int tiles = w.tiles;
    if (d->split > 0) {
        // uniform split, 2-D grid (tiles x ranges)
        long per = (d->P + d->split - 1) / d->split;
        per = (per + WG_BP - 1) / WG_BP * WG_BP;
        const int splits = (int)((d->P + per - 1) / per);
        p.p_per_split = per;
        // for the host code below: one main segment of every tile, no tail (the kernels read these fields only with seg = 1)
        p.main_tiles = tiles; p.main_split = splits; p.tail_split = 1; p.per_main = p.per_tail = per;
        p.atomic = (splits > 1 || d->accumulate) ? 1 : 0;
        w.grid = dim3((unsigned)tiles, (unsigned)splits);
        return;
    }
    // split == 0: two-segment schedule (see WgradParams), dw is accumulated.  Cost model in K steps: a round of
    // workgroups costs its K steps + ~30 steps' worth of prologue and atomic epilogue (fitted on the 3x3 layers).
    const long steps_total = (d->P + WG_BP - 1) / WG_BP;
    const int slots = (w.big || w.pipe) ? WG_SLOTS / 2 : WG_SLOTS;
    const double E = 30.0;
    double best = 1e30;
    int bs = 1, bt = 1;
    for (int sp = 1; sp <= slots; sp *= 2) {
        if (sp > 1 && steps_total / sp < 4) break;
        const int tpr = slots / sp;
        const int mt = tiles / tpr * tpr, tt = tiles - mt;
        long ts = 1;
        if (tt > 0) ts = std::max<long>(sp, std::min<long>(slots / tt, std::max<long>(1, steps_total / 4)));
        const double cost = (double)(mt / tpr) * ((double)((steps_total + sp - 1) / sp) + E) + (tt > 0 ? (double)((steps_total + ts - 1) / ts) + E : 0.0);
        if (cost < best) { best = cost; bs = sp; bt = (int)ts; }
    }
    const int tpr = slots / bs;
    p.seg = 1;
    p.slots = slots;
    p.main_split = bs;
    p.main_tiles = tiles / tpr * tpr;
    p.tail_tiles = tiles - p.main_tiles;
    p.tail_split = p.tail_tiles > 0 ? bt : 1;
    p.per_main = ((d->P + bs - 1) / bs + WG_BP - 1) / WG_BP * WG_BP;
    p.per_tail = ((d->P + p.tail_split - 1) / p.tail_split + WG_BP - 1) / WG_BP * WG_BP;
    // a segment whose tiles are reduced by ONE workgroup stores; only split tiles need atomics (dw arrives zero-filled
    // or holds the value to add to: accumulate forces atomics everywhere)
    p.atomic = d->accumulate ? 3 : ((bs > 1 ? 1 : 0) | (p.tail_split > 1 ? 2 : 0));
    const long nblk = (long)p.main_tiles * bs + (long)p.tail_tiles * p.tail_split;
    w.grid = dim3((unsigned)((nblk + slots - 1) / slots * slots));   // whole groups of `slots` ids for the XCD map
}

// Step 3: what slab mode would need for this schedule
static void wgrad_slab_layout(const yolo_wgrad_desc *d, WgradLaunch &w)
{
    const WgradParams &p = w.p;
    const long main_parts = (long)p.main_tiles * p.main_split, tail_parts = (long)p.tail_tiles * p.tail_split;
    w.main_ranges = (int)std::min<long>(p.main_split, (d->P + p.per_main - 1) / p.per_main);
    w.tail_ranges = (int)std::min<long>(p.tail_split, (d->P + p.per_tail - 1) / p.per_tail);
    if (w.pipe) {
        w.need = (main_parts + tail_parts) * 256 * 256;      // every workgroup's partial tile
    } else if (!w.big) {
        // 128 x 128 kernels: only the tiles of a SPLIT segment go through slabs (a tile owned by one workgroup keeps its direct store);
        // behind the tile partials, [co][range] bias partials of the widest segment
        const long nparts = (p.main_split > 1 ? main_parts : 0) + (p.tail_split > 1 ? tail_parts : 0);
        w.bias_ld = std::max(p.main_tiles > 0 ? p.main_split : 1, p.tail_tiles > 0 ? p.tail_split : 1);
        w.bias_at = nparts * WG_T * WG_T;
        w.need = nparts > 0 ? w.bias_at + (long)p.n_co_tiles * WG_T * w.bias_ld : 0;
    }
}

// Step 4: slab mode and dw_sumsq as asked for, the kernel of the family, the sums of slab mode behind it
static int wgrad_dispatch(const yolo_wgrad_desc *d, WgradLaunch &w, float *db, hipStream_t s)
{
    WgradParams &p = w.p;
    if (d->slabs) {
        // partial tiles as plain stores + a fixed-order sum instead of fp32 atomics
        if (w.big || d->accumulate || (d->Cin & 3) || (((uintptr_t)p.dw | (uintptr_t)d->slabs) & 15))
            return fail(YOLO_E_UNSUPPORTED, "yolo_wgrad: slabs need variant 0 / 1 / 4 / 5 / 6, accumulate = 0, Cin %% 4 == 0 and 16-B aligned dw / slabs");
        if (d->slab_floats < w.need) return fail(YOLO_E_ARG, "yolo_wgrad: slabs hold %ld floats, this launch needs %ld (yolo_wgrad_slab_floats)", (long)d->slab_floats, w.need);
        if (w.pipe) {
            p.slabs = d->slabs;
            p.atomic = 0;
            if (db) {
                // every tile goes through the slabs, so dw is free until the slab sum runs: row co holds the bias partials of its ranges
                if (std::max(w.main_ranges, w.tail_ranges) > (long)p.ntaps * p.Cin)
                    return fail(YOLO_E_UNSUPPORTED, "yolo_wgrad: slabs with db need KH * KW * Cin >= the pixel ranges of a tile");
                p.bias_part = p.dw;
                p.bias_ld = (long)p.ntaps * p.Cin;
            }
        } else if (w.need > 0) {
            p.slabs = d->slabs;          // p.atomic keeps saying which segment is split
            if (db) {
                p.bias_part = d->slabs + w.bias_at;
                p.bias_ld = w.bias_ld;
            }
        }
    }
    if (d->dw_sumsq && (w.pipe || w.big || d->variant == 4 || p.atomic || (d->Cin & 3) || ((uintptr_t)p.dw & 15)))
        return fail(YOLO_E_UNSUPPORTED, "yolo_wgrad: dw_sumsq needs the 128 x 128 kernel storing every tile from one workgroup (split 1, no accumulate, Cin %% 4 == 0)");
    if (w.pipe) {
        if (int rc = d->variant == 6 ? wgrad_wide_launch(p, w.grid, s) : wgrad_pipe_launch(p, w.grid, s)) return rc;
        if (p.bias_part) {            // (reads its partials out of dw: in front of the slab sum, which overwrites them)
            if (int rc = wgrad_bias_sum_launch(p, 256, w.main_ranges, w.tail_ranges, db, s)) return rc;
        }
        if (p.slabs) return wgrad_slab_sum_launch(p, w.tiles, w.main_ranges, w.tail_ranges, s);
        return 0;
    }
    if (w.big) {
        static bool lds_done[64] = {};
        if (int rc = wgrad_lds_attr(lds_done, (const void *)wgrad256_kernel<false>, (const void *)wgrad256_kernel<true>, 3 * W2_STAGE)) return rc;
        if (d->variant == 3) hipLaunchKernelGGL(wgrad256_kernel<true>, w.grid, dim3(512), 3 * W2_STAGE, s, p);
        else hipLaunchKernelGGL(wgrad256_kernel<false>, w.grid, dim3(512), 3 * W2_STAGE, s, p);
    } else if (d->variant == 4) {
        hipLaunchKernelGGL(wgrad_kernel<8>, w.grid, dim3(512), 0, s, p);
    } else {
        p.sumsq = d->dw_sumsq;
        hipLaunchKernelGGL(wgrad_kernel<4>, w.grid, dim3(256), 0, s, p);
    }
    if (int rc = check_launch("yolo_wgrad")) return rc;
    if (p.slabs) {
        hipLaunchKernelGGL(wgrad_slab_sum128_kernel, dim3(WG_T * WG_T / 4 / 256, (unsigned)w.tiles), dim3(256), 0, s, (const float *)p.slabs, p.dw, p.Cout, p.Cin,
                           p.ntaps, p.n_co_tiles, p.n_ci_tiles, p.pair_taps, p.atomic, p.main_tiles, p.main_split, p.tail_split,
                           w.main_ranges, w.tail_ranges);
        if (int rc = check_launch("yolo_wgrad (slab sum)")) return rc;
        if (p.bias_part) return wgrad_bias_sum_launch(p, WG_T, w.main_ranges, w.tail_ranges, db, s);
    }
    return 0;
}

// query: only the floats of slab space that this descriptor's launch needs (yolo_wgrad_slab_floats); nothing is launched
static int wgrad_run(const yolo_wgrad_desc *d, const void *x, const void *dy, float *dw, float *db, yolo_stream_t stream, long *query)
{
    if (!d || !x || !dy || (!dw && !db)) return fail(YOLO_E_ARG, "yolo_wgrad: null pointer");
    if (d->P <= 0 || d->Cout <= 0 || d->Cin <= 0 || d->KH <= 0 || d->KW <= 0 || d->split < 0) return fail(YOLO_E_ARG, "yolo_wgrad: bad descriptor");
    if ((d->dy_px_stride & 7) || (d->x_px_stride & 7) || (d->x_row_stride & 7) || d->dy_px_stride < d->Cout || d->x_px_stride < d->Cin)
        return fail(YOLO_E_UNSUPPORTED, "yolo_wgrad: pixel strides must be multiples of 8 elements and cover the channels");
    hipStream_t s = STRM(stream);
    if (dw) {
        WgradLaunch w{};
        if (int rc = wgrad_fill(d, x, dy, dw, db, w)) return rc;
        wgrad_schedule(d, w);
        wgrad_slab_layout(d, w);
        if (query) {
            *query = w.need;
            return 0;
        }
        return wgrad_dispatch(d, w, db, s);
    }
    // db alone: the column sum walks slots 0 .. P - 1: with a pixel geometry it would add other slots than the descriptor names
    if (d->geo_W != 0) return fail(YOLO_E_UNSUPPORTED, "yolo_wgrad: the bias-only launch (dw == NULL) has no pixel-geometry mode");
    const int nchunks = (d->Cout + 7) / 8;
    const int w = nchunks < 256 ? nchunks : 256;
    const int R = 256 / w;
    const int gx = (nchunks + w - 1) / w;
    long gy = d->P / ((long)R * 32);
    if (gy > 2048 / gx) gy = 2048 / gx;
    if (gy < 1) gy = 1;
    const long per = (d->P + gy - 1) / gy;
    hipLaunchKernelGGL(colsum_kernel, dim3(gx, (unsigned)gy), dim3(256), 0, s, (const bf16_t *)dy, (long)d->P, d->dy_px_stride, d->Cout, w, per, db);
    return check_launch("yolo_wgrad(bias)");
}

YOLO_API int yolo_wgrad(const yolo_wgrad_desc *d, const void *x, const void *dy, float *dw, float *db, yolo_stream_t stream)
{
    return wgrad_run(d, x, dy, dw, db, stream, nullptr);
}

YOLO_API int yolo_wgrad_slab_floats(const yolo_wgrad_desc *d, long *floats)
{
    if (!floats) return fail(YOLO_E_ARG, "yolo_wgrad_slab_floats: null pointer");
    *floats = 0;
    static float dummy[4];      // the schedule does not depend on the operand addresses; nothing is launched
    return wgrad_run(d, dummy, dummy, dummy, nullptr, nullptr, floats);
}
