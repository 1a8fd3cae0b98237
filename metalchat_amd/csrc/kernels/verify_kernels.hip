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

// the first index of the maximum of lr[0, n) into *pick, by the whole workgroup (argmax_row_body's keys and order)
__device__ __forceinline__ void
v_argmax_row(const bf16_t* lr, uint32_t n, int32_t* pick)
{
    __shared__ unsigned long long wk[16];
    unsigned long long best = 0ull;
    for (uint32_t i = threadIdx.x; i < n; i += blockDim.x) best = max(best, (unsigned long long)make_key(bf2f(lr[i]), i));
    for (int off = 32; off >= 1; off >>= 1) best = max(best, (unsigned long long)__shfl_xor(best, off, 64));
    if ((threadIdx.x & 63) == 0) wk[threadIdx.x >> 6] = best;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (uint32_t w = 1; w < (blockDim.x + 63) / 64; w++) best = max(best, wk[w]);
        *pick = (int32_t)key_index(best);
    }
}

// grid (1, M), 1024 threads: picks[row] = the first index of the maximum of logits[row][0, n) (argmax_row_body's keys)
extern "C" __global__ void __launch_bounds__(1024)
mc_v_argmax_bfloat(const bf16_t* logits, uint32_t n, int32_t* picks)
{
    v_argmax_row(logits + (size_t)blockIdx.y * n, n, picks + blockIdx.y);
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

// ------------------------------------------------------------------------------------------
// Verify calls for sampling, masked and penalised rows (include/metalchat_hip.h Part 2m).  vrows[m] (abi.h verify_row, resolved on
// the host) carries packed row m's effective sampler and seed pair.  The two pick launches are the packed-row forms of the mixed
// launches of the row samplers (batch_kernels.hip): the branch on the row's kind is uniform per workgroup -- the packed row is a
// grid index -- so a greedy row computes mc_v_argmax_bfloat's pick, a default or drawing row sample_body's from its own logits
// row with pair vrows[m].seed, and the pick goes to picks[m].  (The names stand outside the mc_v_ prefix, whose symbols
// tests/test_verify_rows_cpu.py lists.)
//   mc_vs_topk_candidates_mixed_bfloat  grid (nlists, M), 64 threads: the candidate lists of the sampling packed rows with the
//                                       CALL's kpad into cand[m][nlists * kpad]; workgroups of greedy rows exit at once
//   mc_vs_pick_mixed_bfloat             grid (1, M), 1024 threads, dynamic LDS: cap keys
//   mc_vs_count_accepted                grid (nseg), after the accept launch: the counts of a penalised row gain the tokens fed
// ------------------------------------------------------------------------------------------
extern "C" __global__ void __launch_bounds__(64)
mc_vs_topk_candidates_mixed_bfloat(const bf16_t* logits, uint32_t n, uint32_t kpad, uint64_t* cand, uint32_t chunk, const verify_row* vrows)
{
    const uint32_t m = blockIdx.y;
    if (vrows[m].sampler.kind == ROW_SAMPLER_GREEDY) return; // (uniform)
    const bf16_t* lr = logits + (size_t)m * n;
    uint64_t* cr = cand + (size_t)m * gridDim.x * kpad;
    if (chunk == 512) topk_candidates_body<BF, 8>(lr, n, kpad, cr);
    else if (chunk == 1024) topk_candidates_body<BF, 16>(lr, n, kpad, cr);
    else if (chunk == 2048) topk_candidates_body<BF, 32>(lr, n, kpad, cr);
}

// sample_body finds its seed pair and its slot of tokens_out through a step state: the packed row's lives in LDS, step_index = m,
// and is handed ONE pair, the row's own -- so pair m % 1 = 0 of seeds + 2 seed is drawn from and the pick lands in picks[m].
// Nothing of the batch's rows[] is read or written.  n_seed_pairs == 0: no pair is read (sample_body's zero pair)
extern "C" __global__ void __launch_bounds__(1024)
mc_vs_pick_mixed_bfloat(const bf16_t* logits, uint32_t n, const uint64_t* cand, const verify_row* vrows, uint32_t nlists, uint32_t kpad,
                        uint32_t cap, const uint64_t* seeds, uint32_t n_seed_pairs, int32_t* picks)
{
    __shared__ step_state st;
    const uint32_t m = blockIdx.y;
    const verify_row v = vrows[m];
    if (v.sampler.kind == ROW_SAMPLER_GREEDY) { // (uniform)
        v_argmax_row(logits + (size_t)m * n, n, picks + m);
        return;
    }
    if (threadIdx.x == 0) st.step_index = (int32_t)m;
    __syncthreads();
    const sampler_params p{v.sampler.k, nlists * kpad, cap, v.sampler.inv_temp, v.sampler.top_p, nlists, kpad};
    sample_body<BF, SAMPLE_LAST_ROW>(cand + (size_t)m * p.ncand, p, seeds + 2 * (size_t)v.seed, n_seed_pairs ? 1u : 0u, &st, picks, nullptr,
                                     v.sampler.kind == ROW_SAMPLER_DRAW);
}

// grid (nseg), 64 threads: segment g = segs[blockIdx.x].  A row with penalties (table[row], the step's table) counts what was
// fed: chunk rows 0 .. accepted[row], for a tree (paths != null) the nodes paths[row][0 .. accepted[row]].  ONE thread walks them
// in order with plain loads and stores -- a token that occurs twice on the path is counted twice -- and no other word of counts is
// written.  Rows without penalties neither read nor write counts.  accepted <= len - 1 and the path's nodes lie below len
// (mc_v_accept / mc_tv_accept), the tokens inside the vocabulary (rows_check).
extern "C" __global__ void __launch_bounds__(64)
mc_vs_count_accepted(const pp_seg* segs, const int32_t* tokens, const int32_t* accepted, const int32_t* paths, const row_logits* table,
                     int32_t* counts, uint32_t vocab)
{
    const pp_seg g = segs[blockIdx.x];
    if (threadIdx.x != 0 || !(table[g.row].flags & ROW_LOGITS_PENALTY)) return;
    const int32_t a = min(accepted[g.row], g.len - 1);
    int32_t* cr = counts + (size_t)g.row * vocab;
    const int32_t* path = paths ? paths + (size_t)g.row * MC_VERIFY_MAX_LEN : nullptr;
    for (int32_t d = 0; d <= a; d++) {
        const int32_t node = path ? path[d] : d;
        if (node < 0 || node >= g.len) break;
        const int32_t t = tokens[g.off + node];
        cr[t] = cr[t] + 1;
    }
}
