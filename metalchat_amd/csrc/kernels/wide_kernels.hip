// Wide batches (mc_wide_batch_create, include/metalchat_hip.h Part 2h): the seven per-layer linears and the head of a batch of
// 17 .. MC_WIDE_BATCH_MAX rows, each in ONE pass over its weight matrix.
//
//   mc_wb_gemv_{i4,i8,w}_bfloat_e{0,1,2}     y[r][n] = epi(sum_k W[n][k] x[r][k]) for r < M <= 64: store, + residual, SiLU.mul
//   mc_wb_gemv_{i4,i8,w}_bfloat_e{0,1,2}_l   the same with a LoRA adaptor's term added in front of the epilogue
//
// Row r's bits are mc_b_gemv_*_eE's (batch_kernels.hip bgemv_body) for that activation row, because everything that fixes them
// is kept (the list is verify_kernels.hip's): each weight dequantised by bg_dequant (int8: bg_dequant8) with the scale of ITS group,
// (k0 + 32 g) / group; K cut into BG_WAVES equal contiguous slices,
// wave w of the workgroup taking slice w; per slice, 16-row weight tile and 16-column group ONE fp32 accumulator fed by
// v_mfma_f32_16x16x32_bf16 in ascending k, MFMA j of a 128-weight chunk contracting k = 32 g + 8 j + [0, 8) on both operands; the
// eight slice sums added in slice order; one rounding to T; then bgemv_body's epilogue on that T.  MFMA columns are independent,
// so an activation row's column index -- and what sits in the other columns -- does not reach its sums.
//
// The shape of the work is mc_v_head_*'s with WB_GROUPS = 4 column groups: a workgroup owns TILES 16-row weight tiles and all
// column groups, so a weight is dequantised once per call and a B fragment (16 activation rows x 8 k per lane group) is used for
// TILES weight tiles.  TILES is 1, 2, 4 or 8, taken from the grid: the launch that brings ceil(N / 16 / tiles) workgroups gets
// `tiles` per workgroup.  The host picks it per matrix (batch_plan.h wb_tiles): a matrix of few rows needs its workgroups to reach every
// compute unit, a matrix of many can spend them on fewer fetches of x.  The tile count does not reach the bits: the accumulators
// of two tiles never meet.  Column groups at or past M are skipped (wave-uniform), rows past M inside the last group are zero
// operands and are not stored.
//
// Adaptors (_l): the arguments (a, lda, lora_b, lora_cols, lora_scale) and the arithmetic are mc_b_gemv_*_l's (batch_kernels.hip),
// and so is THE ORDER OF p: bg_lora_sum -- one fp32 accumulator per output from +0, columns 0 .. lora_cols - 1 ascending, one
// addition per column.  The lane that folds (activation row n, weight rows r0 .. r0 + 3) loads the first 16 columns before the fold's barrier.
#include "common.h"

using namespace mc;

enum { WB_GROUPS = MC_WIDE_BATCH_MAX / 16 };
static_assert(WB_GROUPS * 16 == MC_WIDE_BATCH_MAX && WB_GROUPS <= BG_WAVES, "mc_wb_gemv: wave c folds column group c");

// part: the slice sums of one weight tile, [slice][column group][lane]
struct wb_lora {
    const bf16_t* a;
    uint32_t lda;
    const bf16_t* b;
    uint32_t cols;
    float scale;
};

template <int FMT, int EPI, bool LORA, int TILES>
__device__ __forceinline__ void
wbgemv_body(bg_f32x4 (*part)[WB_GROUPS][64], const uint8_t* __restrict__ w, const bf16_t* __restrict__ scales, const bf16_t* __restrict__ x,
            bf16_t* __restrict__ y, uint32_t K, uint32_t ngroups, uint32_t group, uint32_t M, uint32_t N, uint32_t ldy, const wb_lora& lo,
            const uint32_t tile0)
{
    constexpr bool Q4 = FMT == BFMT_I4, Q8 = FMT == BFMT_I8, QS = Q4 || Q8;
    constexpr int NWQ = Q8 ? 2 : 1;                                         // 16-byte loads of a lane's 32 quantised weights
    constexpr int U = (Q4 ? 4 : 2) / TILES > 0 ? (Q4 ? 4 : 2) / TILES : 1; // 128-weight chunks per round of weight loads
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t m = lane & 15, g = lane >> 4;
    const uint32_t ntiles = N / 16;
    if (tile0 >= ntiles) return; // (uniform over the workgroup: a grid rounded up)
    const size_t rowbytes = Q4 ? (size_t)K / 2 : (Q8 ? (size_t)K : (size_t)K * 2);
    const uint32_t kslice = K / BG_WAVES, kb = wave * kslice, ke = kb + kslice;
    // this lane's row of the workgroup's first tile; tile t lies tt(t) tiles behind it (wave-uniform: scalar arithmetic).  A tile
    // past N reads the last tile's rows: its sums are dropped
    const uint32_t row0 = tile0 * 16 + m;
    const uint8_t* wrow0 = w + (size_t)row0 * rowbytes + (Q4 ? 16 * g : (Q8 ? 32 * g : 64 * g));
    const bf16_t* srow0 = scales + (size_t)(row0 / 4) * ngroups * 4 + row0 % 4;
    const uint32_t tlast = ntiles - 1 - tile0, wtile = 16 * (uint32_t)rowbytes, stile = 16 * ngroups;
    auto tt = [&](int t) { return (uint32_t)t < tlast ? (uint32_t)t : tlast; };
    // lane (n, g) of column group c feeds activation row 16 c + n; a row at or past M is a zero operand
    const bf16_t* xlane = x + (size_t)(m < M ? m : 0) * K + 32 * g;
    bg_f32x4 acc[TILES][WB_GROUPS];
#pragma unroll
    for (int t = 0; t < TILES; t++)
#pragma unroll
        for (int c = 0; c < WB_GROUPS; c++) acc[t][c] = {0.f, 0.f, 0.f, 0.f};

    auto chunks = [&](uint32_t k0, auto uc) {
        constexpr int UU = decltype(uc)::value;
        uint4 wq[UU][TILES][NWQ];
        float s[UU][TILES], ms8[UU][TILES];
        if (QS) {
#pragma unroll
            for (int u = 0; u < UU; u++)
#pragma unroll
                for (int t = 0; t < TILES; t++) {
                    const uint32_t k = k0 + 128u * u;
#pragma unroll
                    for (int h = 0; h < NWQ; h++) wq[u][t][h] = *reinterpret_cast<const uint4*>(wrow0 + tt(t) * wtile + (Q4 ? k / 2 : k) + 16 * h);
                    s[u][t] = bf2f(srow0[tt(t) * stile + (size_t)(group ? (k + 32 * g) / group : 0) * 4]);
                    ms8[u][t] = -8.0f * s[u][t];
                }
        }
#pragma unroll
        for (int u = 0; u < UU; u++) {
            const uint32_t k = k0 + 128u * u;
#pragma unroll
            for (int j = 0; j < 4; j++) {
                uint4 a[TILES];
#pragma unroll
                for (int t = 0; t < TILES; t++) {
                    if (Q4) {
                        const uint4 q = wq[u][t][0];
                        const uint32_t d = j == 0 ? q.x : (j == 1 ? q.y : (j == 2 ? q.z : q.w));
                        a[t] = bg_dequant(d, s[u][t], ms8[u][t]);
                    } else if (Q8) {
                        const uint4 q = wq[u][t][j / 2];
                        a[t] = (j & 1) ? bg_dequant8(q.z, q.w, s[u][t]) : bg_dequant8(q.x, q.y, s[u][t]);
                    } else {
                        a[t] = *reinterpret_cast<const uint4*>(wrow0 + tt(t) * wtile + (size_t)(k + 8 * j) * 2);
                    }
                }
#pragma unroll
                for (int c = 0; c < WB_GROUPS; c++) {
                    if (16u * c >= M) continue; // wave-uniform
                    const bool has_x = 16u * c + m < M;
                    const uint4 xv = has_x ? *reinterpret_cast<const uint4*>(xlane + (size_t)16 * c * K + k + 8 * j) : make_uint4(0, 0, 0, 0);
#pragma unroll
                    for (int t = 0; t < TILES; t++)
                        acc[t][c] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bg_bf16x8, a[t]), __builtin_bit_cast(bg_bf16x8, xv),
                                                                            acc[t][c], 0, 0, 0);
                }
            }
        }
    };
    uint32_t k = kb;
    for (; k + 128u * U <= ke; k += 128u * U) chunks(k, std::integral_constant<int, U>{});
    for (; k < ke; k += 128u) chunks(k, std::integral_constant<int, 1>{});

    // per weight tile: the slice sums through LDS, then wave c adds column group c's in slice order and stores rows 16 c + n
#pragma unroll
    for (int t = 0; t < TILES; t++) {
        if (tile0 + t >= ntiles) break; // (uniform over the workgroup)
        // lane (n, g) of wave c < WB_GROUPS folds weight rows 16 (tile0 + t) + 4 g + i of activation row n = 16 c + m
        const uint32_t n = 16 * wave + m, r0 = (tile0 + t) * 16 + 4 * g;
        const bool folds = wave < WB_GROUPS && n < M;
        const bf16_t* arow = lo.a + (size_t)n * lo.lda;
        const bf16_t* brow = lo.b + (size_t)r0 * lo.cols;
        bg_lora_block first;
        if (LORA && folds) first = bg_lora_load(arow, brow, lo.cols, 0);
        if (t) __syncthreads();
#pragma unroll
        for (int c = 0; c < WB_GROUPS; c++)
            if (16u * c < M) part[wave][c][lane] = acc[t][c];
        __syncthreads();
        if (folds) {
            bg_f32x4 v = part[0][wave][lane];
#pragma unroll
            for (int w2 = 1; w2 < BG_WAVES; w2++) v += part[w2][wave][lane]; // slice order
            float p[4] = {0.f, 0.f, 0.f, 0.f};
            if (LORA) bg_lora_sum(p, first, arow, brow, lo.cols);
            bg_epilogue<EPI, LORA>(v, p, BF::rt(lo.scale), y + (size_t)n * ldy, r0);
        }
    }
}

// the tiles per workgroup of this launch, from its grid (at most 8: a grid below ceil(N / 128) leaves rows unwritten).  The int8 and
// the _l kernels hold at most 4 tiles' accumulators beside their wider weight registers / the adaptor's operands: 8 tiles are two
// passes of 4 there (the host does not ask for them: batch.cc wb_tiles)
template <int FMT, int EPI, bool LORA>
__device__ __forceinline__ void
wbgemv(const uint8_t* w, const bf16_t* scales, const bf16_t* x, bf16_t* y, uint32_t K, uint32_t ngroups, uint32_t group, uint32_t M, uint32_t N,
       uint32_t ldy, const wb_lora& lo = wb_lora{})
{
    __shared__ bg_f32x4 part[BG_WAVES][WB_GROUPS][64]; // 32 KB
    const uint32_t per = (N / 16 + gridDim.x - 1) / gridDim.x;
    if (per <= 1) wbgemv_body<FMT, EPI, LORA, 1>(part, w, scales, x, y, K, ngroups, group, M, N, ldy, lo, blockIdx.x);
    else if (per <= 2) wbgemv_body<FMT, EPI, LORA, 2>(part, w, scales, x, y, K, ngroups, group, M, N, ldy, lo, blockIdx.x * 2);
    else if (per <= 4) wbgemv_body<FMT, EPI, LORA, 4>(part, w, scales, x, y, K, ngroups, group, M, N, ldy, lo, blockIdx.x * 4);
    else if constexpr (FMT != BFMT_I8 && !LORA) wbgemv_body<FMT, EPI, LORA, 8>(part, w, scales, x, y, K, ngroups, group, M, N, ldy, lo, blockIdx.x * 8);
    else {
        wbgemv_body<FMT, EPI, LORA, 4>(part, w, scales, x, y, K, ngroups, group, M, N, ldy, lo, blockIdx.x * 8);
        __syncthreads(); // (the second pass writes the LDS the first one's fold read)
        wbgemv_body<FMT, EPI, LORA, 4>(part, w, scales, x, y, K, ngroups, group, M, N, ldy, lo, blockIdx.x * 8 + 4);
    }
}

// grid ceil(N / (16 tiles)), tiles in {1, 2, 4, 8}; 512 threads.  x [M][K], y [M] rows at stride ldy (e2: N / 2 columns of them);
// N % 16 == 0 (e2: N % 32 == 0), K % BG_K_UNIT == 0, 1 <= M <= MC_WIDE_BATCH_MAX
// _l: (a, lda, lora_b, lora_cols, lora_scale) behind them -- a [M] rows of lora_cols at stride lda, lora_b [N][lora_cols], lora_cols % 16 == 0
#define MC_WBGEMV(FMT, F, E)                                                                                                      \
    extern "C" __global__ void __launch_bounds__(64 * BG_WAVES)                                                                   \
    mc_wb_gemv_##FMT##_bfloat_e##E(const uint8_t* w, const bf16_t* scales, const bf16_t* x, bf16_t* y, uint32_t K,               \
                                   uint32_t ngroups, uint32_t group, uint32_t M, uint32_t N, uint32_t ldy)                        \
    {                                                                                                                             \
        wbgemv<F, E, false>(w, scales, x, y, K, ngroups, group, M, N, ldy);                                                       \
    }                                                                                                                             \
    extern "C" __global__ void __launch_bounds__(64 * BG_WAVES)                                                                   \
    mc_wb_gemv_##FMT##_bfloat_e##E##_l(const uint8_t* w, const bf16_t* scales, const bf16_t* x, bf16_t* y, uint32_t K,           \
                                       uint32_t ngroups, uint32_t group, uint32_t M, uint32_t N, uint32_t ldy, const bf16_t* a,   \
                                       uint32_t lda, const bf16_t* lora_b, uint32_t lora_cols, float lora_scale)                  \
    {                                                                                                                             \
        wbgemv<F, E, true>(w, scales, x, y, K, ngroups, group, M, N, ldy, wb_lora{a, lda, lora_b, lora_cols, lora_scale});        \
    }
MC_WBGEMV(i4, BFMT_I4, 0)
MC_WBGEMV(i4, BFMT_I4, 1)
MC_WBGEMV(i4, BFMT_I4, 2)
MC_WBGEMV(i8, BFMT_I8, 0)
MC_WBGEMV(i8, BFMT_I8, 1)
MC_WBGEMV(i8, BFMT_I8, 2)
MC_WBGEMV(w, BFMT_W, 0)
MC_WBGEMV(w, BFMT_W, 1)
MC_WBGEMV(w, BFMT_W, 2)
