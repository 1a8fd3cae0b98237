// Speculative verify (mc_verify_rows, include/metalchat_hip.h Part 2f): after mc_extend_rows' layer pass every packed chunk row goes
// through the final norm (mc_b_rmsnorm_bfloat, grid y = M) and the head, and gets a greedy pick; then the acceptance per segment.
//
//   mc_v_head_{i4,w}_bfloat, mc_vhead_i8_bfloat (an int8 head; named outside the mc_v_ prefix, whose symbols tests/test_verify_rows_cpu.py lists)
//                            logits[M][N] for M <= 128 activation rows in ONE pass over the head's weights
//   mc_v_argmax_bfloat        picks[M]: argmax_row_body's rule (the first index of the maximum)
//   mc_v_accept               accepted / next_tokens per segment, and the accepted row's logits into the batch's [B][vocab]
//
// The head's bits are mc_b_gemv_*_e0's (batch_kernels.hip bgemv_body), row for row, because everything that fixes them is kept:
// each weight dequantised by bg_dequant; K cut into BG_WAVES equal contiguous slices, wave w of the workgroup taking slice w; per
// slice and 16-row weight tile ONE fp32 accumulator fed by v_mfma_f32_16x16x32_bf16 in ascending k, MFMA j of a 128-weight chunk
// contracting k = 32 g + 8 j + [0, 8) on both operands; the eight slice sums added in slice order; one rounding to T.  MFMA
// columns are independent, so an activation row's column index -- and what sits in the other columns -- does not reach its sums.
//
// What differs is the shape of the work.  A workgroup owns VH_TILES 16-row weight tiles and all VH_GROUPS 16-column groups: a
// dequantised A fragment is used for up to 128 activation rows (the dequantisation is paid once per weight and call), and a B
// fragment -- 16 activation rows x 8 k per lane group, one 16-byte load per lane -- for VH_TILES weight tiles, so the N / (16
// VH_TILES) workgroups fetch the M x K activations from L2 that many times and not N / 16 times.  Column groups at or past M are
// skipped (wave-uniform), rows past M inside the last group are zero operands and are not stored.
#include "common.h"

using namespace mc;

enum { VH_GROUPS = 8 }; // 16 x VH_GROUPS = MC_VERIFY_MAX_ROWS activation rows; VH_TILES (abi.h) x 16 weight rows per workgroup
static_assert(VH_GROUPS * 16 == MC_VERIFY_MAX_ROWS && VH_GROUPS == BG_WAVES, "mc_v_head: wave c folds column group c");

template <int FMT>
__device__ __forceinline__ void
vhead_body(const uint8_t* __restrict__ w, const bf16_t* __restrict__ scales, const bf16_t* __restrict__ x, bf16_t* __restrict__ y,
           uint32_t K, uint32_t ngroups, uint32_t group, uint32_t M, uint32_t N, uint32_t ldy)
{
    constexpr bool Q4 = FMT == BFMT_I4, Q8 = FMT == BFMT_I8, QS = Q4 || Q8;
    constexpr int NWQ = Q8 ? 2 : 1; // 16-byte loads of a lane's 32 quantised weights
    // the slice sums of one weight tile: [slice][column group][lane], 64 KB
    __shared__ bg_f32x4 part[BG_WAVES][VH_GROUPS][64];
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t m = lane & 15, g = lane >> 4;
    const uint32_t tile0 = blockIdx.x * VH_TILES, ntiles = N / 16;
    const size_t rowbytes = Q4 ? (size_t)K / 2 : (Q8 ? (size_t)K : (size_t)K * 2);
    const uint32_t kslice = K / BG_WAVES, kb = wave * kslice, ke = kb + kslice;
    const uint8_t* wrow[VH_TILES];
    const bf16_t* srow[VH_TILES];
#pragma unroll
    for (int t = 0; t < VH_TILES; t++) {
        // (a tile past N reads tile 0's rows of this workgroup: its sums are dropped)
        const uint32_t row = (tile0 + t < ntiles ? tile0 + t : tile0) * 16 + m;
        wrow[t] = w + (size_t)row * rowbytes + (Q4 ? 16 * g : (Q8 ? 32 * g : 64 * g));
        srow[t] = scales + (size_t)(row / 4) * ngroups * 4 + row % 4;
    }
    // lane (n, g) of column group c feeds activation row 16 c + n; a row at or past M is a zero operand
    const bf16_t* xlane = x + (size_t)(m < M ? m : 0) * K + 32 * g;
    bg_f32x4 acc[VH_TILES][VH_GROUPS];
#pragma unroll
    for (int t = 0; t < VH_TILES; t++)
#pragma unroll
        for (int c = 0; c < VH_GROUPS; c++) acc[t][c] = {0.f, 0.f, 0.f, 0.f};

    for (uint32_t k = kb; k < ke; k += 128u) {
        uint4 wq[VH_TILES][NWQ];
        float s[VH_TILES], ms8[VH_TILES];
        if (QS) {
#pragma unroll
            for (int t = 0; t < VH_TILES; t++) {
#pragma unroll
                for (int h = 0; h < NWQ; h++) wq[t][h] = *reinterpret_cast<const uint4*>(wrow[t] + (Q4 ? k / 2 : k) + 16 * h);
                s[t] = bf2f(srow[t][(size_t)(group ? (k + 32 * g) / group : 0) * 4]); // the group of this lane's 32 weights
                ms8[t] = -8.0f * s[t];
            }
        }
#pragma unroll
        for (int j = 0; j < 4; j++) {
            uint4 a[VH_TILES];
#pragma unroll
            for (int t = 0; t < VH_TILES; t++) {
                if (Q4) {
                    const uint4 q = wq[t][0];
                    const uint32_t d = j == 0 ? q.x : (j == 1 ? q.y : (j == 2 ? q.z : q.w));
                    a[t] = bg_dequant(d, s[t], ms8[t]);
                } else if (Q8) {
                    const uint4 q = wq[t][j / 2];
                    a[t] = (j & 1) ? bg_dequant8(q.z, q.w, s[t]) : bg_dequant8(q.x, q.y, s[t]);
                } else {
                    a[t] = *reinterpret_cast<const uint4*>(wrow[t] + (size_t)(k + 8 * j) * 2);
                }
            }
#pragma unroll
            for (int c = 0; c < VH_GROUPS; c++) {
                if (16u * c >= M) continue; // wave-uniform
                const bool has_x = 16u * c + m < M;
                const uint4 xv = has_x ? *reinterpret_cast<const uint4*>(xlane + (size_t)16 * c * K + k + 8 * j) : make_uint4(0, 0, 0, 0);
#pragma unroll
                for (int t = 0; t < VH_TILES; t++)
                    acc[t][c] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bg_bf16x8, a[t]), __builtin_bit_cast(bg_bf16x8, xv),
                                                                        acc[t][c], 0, 0, 0);
            }
        }
    }

    // per weight tile: the slice sums through LDS, then wave c adds column group c's in slice order and stores rows 16 c + n
#pragma unroll
    for (int t = 0; t < VH_TILES; t++) {
        if (tile0 + t >= ntiles) break; // (uniform over the workgroup)
        if (t) __syncthreads();
#pragma unroll
        for (int c = 0; c < VH_GROUPS; c++)
            if (16u * c < M) part[wave][c][lane] = acc[t][c];
        __syncthreads();
        const uint32_t n = 16 * wave + m;
        if (n >= M) continue;
        bg_f32x4 v = part[0][wave][lane];
#pragma unroll
        for (int w2 = 1; w2 < BG_WAVES; w2++) v += part[w2][wave][lane]; // slice order
        // lane (n, g) holds weight rows 16 (tile0 + t) + 4 g + i of activation row n
        bf16_t* yr = y + (size_t)n * ldy + (size_t)(tile0 + t) * 16 + 4 * g;
#pragma unroll
        for (int i = 0; i < 4; i++) yr[i] = f2bf(BF::rt(v[i]));
    }
}

// grid ceil(N / (16 VH_TILES)), 512 threads.  x [M][K], y [M] rows at stride ldy; N % 16 == 0, K % BG_K_UNIT == 0, 1 <= M <= 128
extern "C" __global__ void __launch_bounds__(64 * BG_WAVES)
mc_v_head_i4_bfloat(const uint8_t* w, const bf16_t* scales, const bf16_t* x, bf16_t* y, uint32_t K, uint32_t ngroups, uint32_t group,
                    uint32_t M, uint32_t N, uint32_t ldy)
{
    vhead_body<BFMT_I4>(w, scales, x, y, K, ngroups, group, M, N, ldy);
}
extern "C" __global__ void __launch_bounds__(64 * BG_WAVES)
mc_vhead_i8_bfloat(const uint8_t* w, const bf16_t* scales, const bf16_t* x, bf16_t* y, uint32_t K, uint32_t ngroups, uint32_t group,
                    uint32_t M, uint32_t N, uint32_t ldy)
{
    vhead_body<BFMT_I8>(w, scales, x, y, K, ngroups, group, M, N, ldy);
}
extern "C" __global__ void __launch_bounds__(64 * BG_WAVES)
mc_v_head_w_bfloat(const uint8_t* w, const bf16_t* scales, const bf16_t* x, bf16_t* y, uint32_t K, uint32_t ngroups, uint32_t group,
                   uint32_t M, uint32_t N, uint32_t ldy)
{
    vhead_body<BFMT_W>(w, scales, x, y, K, ngroups, group, M, N, ldy);
}

// grid (1, M), 1024 threads: picks[row] = the first index of the maximum of logits[row][0, n) (argmax_row_body's keys)
extern "C" __global__ void __launch_bounds__(1024)
mc_v_argmax_bfloat(const bf16_t* logits, uint32_t n, int32_t* picks)
{
    __shared__ unsigned long long wk[16];
    const bf16_t* lr = logits + (size_t)blockIdx.y * n;
    unsigned long long best = 0ull;
    for (uint32_t i = threadIdx.x; i < n; i += blockDim.x) best = max(best, (unsigned long long)make_key(bf2f(lr[i]), i));
    for (int off = 32; off >= 1; off >>= 1) best = max(best, (unsigned long long)__shfl_xor(best, off, 64));
    if ((threadIdx.x & 63) == 0) wk[threadIdx.x >> 6] = best;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (uint32_t w = 1; w < (blockDim.x + 63) / 64; w++) best = max(best, wk[w]);
        picks[blockIdx.y] = (int32_t)key_index(best);
    }
}

// grid (any, nseg): segment g = segs[blockIdx.y] holds the chunk c[0, len) = tokens[off ..] and the picks after each of its rows.
// a = the largest a <= len - 1 with c[i + 1] == pick[i] for all i < a (every thread walks the <= 15 drafts: no hand-off);
// accepted[row] = a, next_tokens[row] = pick[a] (either may be null), and logits row off + a into logits_out[row]
// (vocab % 8 == 0: rows are copied in 16-byte pieces).  Rows of the batch without a segment are not written.
extern "C" __global__ void __launch_bounds__(256)
mc_v_accept(const pp_seg* segs, const int32_t* tokens, const int32_t* picks, const bf16_t* logits, uint32_t vocab, int32_t* accepted,
            int32_t* next_tokens, bf16_t* logits_out)
{
    const pp_seg g = segs[blockIdx.y];
    int32_t a = 0;
    while (a < g.len - 1 && tokens[g.off + a + 1] == picks[g.off + a]) a++;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        if (accepted) accepted[g.row] = a;
        if (next_tokens) next_tokens[g.row] = picks[g.off + a];
    }
    const uint4* src = reinterpret_cast<const uint4*>(logits + (size_t)(g.off + a) * vocab);
    uint4* dst = reinterpret_cast<uint4*>(logits_out + (size_t)g.row * vocab);
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < vocab / 8; i += gridDim.x * blockDim.x) dst[i] = src[i];
}
