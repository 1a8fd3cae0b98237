// Wide batches (mc_wide_batch_create, include/metalchat_hip.h Part 2h): the seven per-layer linears and the head of a batch of
// 17 .. MC_WIDE_BATCH_MAX rows, each in ONE pass over its weight matrix.
//
//   mc_wb_gemv_{i4,w}_bfloat_e{0,1,2}   y[r][n] = epi(sum_k W[n][k] x[r][k]) for r < M <= 64: store, + residual, SiLU.mul
//
// Row r's bits are mc_b_gemv_*_eE's (batch_kernels.hip bgemv_body) for that activation row, because everything that fixes them
// is kept (the list is verify_kernels.hip's): each weight dequantised by bg_dequant; K cut into BG_WAVES equal contiguous slices,
// wave w of the workgroup taking slice w; per slice, 16-row weight tile and 16-column group ONE fp32 accumulator fed by
// v_mfma_f32_16x16x32_bf16 in ascending k, MFMA j of a 128-weight chunk contracting k = 32 g + 8 j + [0, 8) on both operands; the
// eight slice sums added in slice order; one rounding to T; then bgemv_body's epilogue on that T.  MFMA columns are independent,
// so an activation row's column index -- and what sits in the other columns -- does not reach its sums.
//
// The shape of the work is mc_v_head_*'s with WB_GROUPS = 4 column groups: a workgroup owns TILES 16-row weight tiles and all
// column groups, so a weight is dequantised once per call and a B fragment (16 activation rows x 8 k per lane group) is used for
// TILES weight tiles.  TILES is 1, 2, 4 or 8, taken from the grid: the launch that brings ceil(N / 16 / tiles) workgroups gets
// `tiles` per workgroup.  The host picks it per matrix (batch.cc wb_tiles): a matrix of few rows needs its workgroups to reach every
// compute unit, a matrix of many can spend them on fewer fetches of x.  The tile count does not reach the bits: the accumulators
// of two tiles never meet.  Column groups at or past M are skipped (wave-uniform), rows past M inside the last group are zero
// operands and are not stored.
#include "common.h"

using namespace mc;

enum { WB_GROUPS = MC_WIDE_BATCH_MAX / 16 };
static_assert(WB_GROUPS * 16 == MC_WIDE_BATCH_MAX && WB_GROUPS <= BG_WAVES, "mc_wb_gemv: wave c folds column group c");

// part: the slice sums of one weight tile, [slice][column group][lane]
template <bool Q4, int EPI, int TILES>
__device__ __forceinline__ void
wbgemv_body(bg_f32x4 (*part)[WB_GROUPS][64], const uint8_t* __restrict__ w, const bf16_t* __restrict__ scales, const bf16_t* __restrict__ x,
            bf16_t* __restrict__ y, uint32_t K, uint32_t ngroups, uint32_t group, uint32_t M, uint32_t N, uint32_t ldy)
{
    constexpr int U = (Q4 ? 4 : 2) / TILES > 0 ? (Q4 ? 4 : 2) / TILES : 1; // 128-weight chunks per round of weight loads
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t m = lane & 15, g = lane >> 4;
    const uint32_t tile0 = blockIdx.x * TILES, ntiles = N / 16;
    if (tile0 >= ntiles) return; // (uniform over the workgroup: a grid rounded up)
    const size_t rowbytes = Q4 ? (size_t)K / 2 : (size_t)K * 2;
    const uint32_t kslice = K / BG_WAVES, kb = wave * kslice, ke = kb + kslice;
    // this lane's row of the workgroup's first tile; tile t lies tt(t) tiles behind it (wave-uniform: scalar arithmetic).  A tile
    // past N reads the last tile's rows: its sums are dropped
    const uint32_t row0 = tile0 * 16 + m;
    const uint8_t* wrow0 = w + (size_t)row0 * rowbytes + (Q4 ? 16 * g : 64 * g);
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
        uint4 wq[UU][TILES];
        float s[UU][TILES], ms8[UU][TILES];
        if (Q4) {
#pragma unroll
            for (int u = 0; u < UU; u++)
#pragma unroll
                for (int t = 0; t < TILES; t++) {
                    const uint32_t k = k0 + 128u * u;
                    wq[u][t] = *reinterpret_cast<const uint4*>(wrow0 + tt(t) * wtile + k / 2);
                    s[u][t] = bf2f(srow0[tt(t) * stile + (size_t)(group ? k / group : 0) * 4]);
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
                        const uint32_t d = j == 0 ? wq[u][t].x : (j == 1 ? wq[u][t].y : (j == 2 ? wq[u][t].z : wq[u][t].w));
                        a[t] = bg_dequant(d, s[u][t], ms8[u][t]);
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
        if (t) __syncthreads();
#pragma unroll
        for (int c = 0; c < WB_GROUPS; c++)
            if (16u * c < M) part[wave][c][lane] = acc[t][c];
        __syncthreads();
        const uint32_t n = 16 * wave + m;
        if (wave < WB_GROUPS && n < M) {
            bg_f32x4 v = part[0][wave][lane];
#pragma unroll
            for (int w2 = 1; w2 < BG_WAVES; w2++) v += part[w2][wave][lane]; // slice order
            // lane (n, g) holds weight rows 16 (tile0 + t) + 4 g + i of activation row n
            const uint32_t r0 = (tile0 + t) * 16 + 4 * g;
            bf16_t* yr = y + (size_t)n * ldy;
            if (EPI == BEPI_SILU_MUL) {
                // w1 | w3 rows interleaved (2j, 2j + 1): out[j] = T(silu(T(w1 x)) * T(w3 x))   (gemv.h EPI_SILU_MUL)
#pragma unroll
                for (int i = 0; i < 4; i += 2) {
                    const float ga = BF::rt(v[i]), gb = BF::rt(v[i + 1]);
                    yr[(r0 + i) / 2] = f2bf(mc::gemv::silu_T<BF>(ga) * gb);
                }
            } else {
#pragma unroll
                for (int i = 0; i < 4; i++) {
                    float o = BF::rt(v[i]);
                    if (EPI == BEPI_RESID) o = bf2f(yr[r0 + i]) + o; // residual added in T (gemv.h EPI_RESID)
                    yr[r0 + i] = f2bf(o);
                }
            }
        }
    }
}

// the tiles per workgroup of this launch, from its grid (at most 8: a grid below ceil(N / 128) leaves rows unwritten)
template <bool Q4, int EPI>
__device__ __forceinline__ void
wbgemv(const uint8_t* w, const bf16_t* scales, const bf16_t* x, bf16_t* y, uint32_t K, uint32_t ngroups, uint32_t group, uint32_t M, uint32_t N,
       uint32_t ldy)
{
    __shared__ bg_f32x4 part[BG_WAVES][WB_GROUPS][64]; // 32 KB
    const uint32_t per = (N / 16 + gridDim.x - 1) / gridDim.x;
    if (per <= 1) wbgemv_body<Q4, EPI, 1>(part, w, scales, x, y, K, ngroups, group, M, N, ldy);
    else if (per <= 2) wbgemv_body<Q4, EPI, 2>(part, w, scales, x, y, K, ngroups, group, M, N, ldy);
    else if (per <= 4) wbgemv_body<Q4, EPI, 4>(part, w, scales, x, y, K, ngroups, group, M, N, ldy);
    else wbgemv_body<Q4, EPI, 8>(part, w, scales, x, y, K, ngroups, group, M, N, ldy);
}

// grid ceil(N / (16 tiles)), tiles in {1, 2, 4, 8}; 512 threads.  x [M][K], y [M] rows at stride ldy (e2: N / 2 columns of them);
// N % 16 == 0 (e2: N % 32 == 0), K % BG_K_UNIT == 0, 1 <= M <= MC_WIDE_BATCH_MAX
#define MC_WBGEMV(FMT, Q4, E)                                                                                                     \
    extern "C" __global__ void __launch_bounds__(64 * BG_WAVES)                                                                   \
    mc_wb_gemv_##FMT##_bfloat_e##E(const uint8_t* w, const bf16_t* scales, const bf16_t* x, bf16_t* y, uint32_t K,               \
                                   uint32_t ngroups, uint32_t group, uint32_t M, uint32_t N, uint32_t ldy)                        \
    {                                                                                                                             \
        wbgemv<Q4, E>(w, scales, x, y, K, ngroups, group, M, N, ldy);                                                             \
    }
MC_WBGEMV(i4, true, 0)
MC_WBGEMV(i4, true, 1)
MC_WBGEMV(i4, true, 2)
MC_WBGEMV(w, false, 0)
MC_WBGEMV(w, false, 1)
MC_WBGEMV(w, false, 2)
