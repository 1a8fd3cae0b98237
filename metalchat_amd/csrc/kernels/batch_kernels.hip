// Batched decode (mc_batch_*, include/metalchat_hip.h Part 2b): B <= 8 sequences in lockstep at ONE position over the decoder's
// weights -- what nn::attention::operator() does with input[bs, 1, dim] and a sink_cache of max_batch_size rows written at one
// start_pos (include/metalchat/nn/attention.h:163-206, nn/cache.h:154-215).
//
// Row independence is the invariant of every kernel here: batch row r is one grid index (or one MFMA column), and no sum mixes
// rows, so a row's bits do not depend on B or on what sits beside it.  The arithmetic per row is the batch-1 decoder's:
//   B-row GEMV    each weight dequantised ONCE as T(T(q) T(s)) (kernel/mul.metal:78-82), then used for every row as the A operand
//                 of v_mfma_f32_16x16x32_bf16 (16 weight rows x 32 k) against the rows' activations as B (16 columns, B used)
//   attention     attn_scores_bf / attn_pv_bf_body of decode_kernels.hip with the row on grid z: T(q.k), T(. scale), exp,
//                 p = T(e / sum), one rounding of the fp32 P.V sum
//   rope + cache  rope_kv_body per row, into the row's own cache at the batch's position
//   rmsnorm       rmsnorm_row_body per row; the embedding and the greedy / default sampler per row as well
#include "common.h"
#include "handoff.h"

using namespace mc;

// ------------------------------------------------------------------------------------------
// B-row GEMV: y[r][n] = epi(sum_k W[n][k] x[r][k]) for r < B.
// Workgroup = 16 consecutive weight rows x all of K; its BG_WAVES waves take K in contiguous equal slices, and their fp32
// partial tiles are added in wave order through LDS (fixed order, whatever B is).  Per 128-weight chunk lane (m, g) of a wave
// (m = lane % 16, g = lane / 16) loads row m's k [32 g, 32 g + 32) of the chunk (int4: one 16-byte load; bfloat: four); MFMA j
// of the chunk contracts k = 32 g + 8 j + [0, 8) on both operands: the B operand of lane (n, g) is batch row n's activations at
// those k (zero for n >= B).  The accumulator then holds C[4 g + i][n] in lane (n, g), element i.
// int4: a dword is 8 offset-binary nibbles, nibble p = weight {0,2,4,6,1,3,5,7}[p] of its 8-run; fma(n, s, -8 s) = (n - 8) s exactly (<= 12 significant bits), rounded once to bfloat by
// v_cvt_pk_bf16_f32 -- T(T(q) T(s)).  Scales: bfloat row quads [out/4][in/group][4]; group % 128 == 0 or 0 (one per row).
// ------------------------------------------------------------------------------------------
enum { BEPI_STORE = 0, BEPI_RESID = 1, BEPI_SILU_MUL = 2 };

typedef __bf16 bg_bf16x8 __attribute__((ext_vector_type(8)));
typedef float bg_f32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ uint4
bg_dequant(uint32_t d, float s, float ms8)
{
    // nibble p (bits 4p) is weight {0,2,4,6,1,3,5,7}[p]: the natural pair (2j, 2j + 1) is nibbles (j, j + 4) -- bytes j / 2
    // and j / 2 + 2 of the low (even j) or high (odd j) nibbles
    const uint32_t lo = d & 0x0F0F0F0Fu, hi = (d >> 4) & 0x0F0F0F0Fu;
    uint32_t o[4];
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const uint32_t v = (j & 1) ? hi : lo;
        const int b = j >> 1;
        const float a = __builtin_fmaf((float)((v >> (8 * b)) & 0xFFu), s, ms8);
        const float c = __builtin_fmaf((float)((v >> (8 * b + 16)) & 0xFFu), s, ms8);
        o[j] = pack_bf16x2(a, c);
    }
    return make_uint4(o[0], o[1], o[2], o[3]);
}

template <bool Q4, int EPI>
__device__ __forceinline__ void
bgemv_body(const uint8_t* __restrict__ w, const bf16_t* __restrict__ scales, const bf16_t* __restrict__ x,
           bf16_t* __restrict__ y, uint32_t K, uint32_t ngroups, uint32_t group, uint32_t B, uint32_t ldy)
{
    constexpr int U = Q4 ? 4 : 2; // 128-weight chunks per round of loads
    constexpr int NWD = Q4 ? 1 : 4;
    __shared__ bg_f32x4 part[BG_WAVES][64];
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t m = lane & 15, g = lane >> 4;
    const uint32_t row = blockIdx.x * 16 + m; // the weight row this lane loads
    const size_t rowbytes = Q4 ? (size_t)K / 2 : (size_t)K * 2;
    const uint8_t* wrow = w + (size_t)row * rowbytes;
    const bool has_x = m < B;
    const bf16_t* xrow = x + (size_t)(has_x ? m : 0) * K;
    const uint32_t kslice = K / BG_WAVES, kb = wave * kslice, ke = kb + kslice;
    const bf16_t* srow = scales + (size_t)(row / 4) * ngroups * 4 + row % 4;
    bg_f32x4 acc = {0.f, 0.f, 0.f, 0.f};

    auto chunks = [&](uint32_t k0, auto uc) {
        constexpr int UU = decltype(uc)::value;
        uint4 wv[UU][NWD], xv[UU][4];
        bf16_t sv[UU];
#pragma unroll
        for (int u = 0; u < UU; u++) {
            const uint32_t k = k0 + 128u * u;
            if (Q4) {
                wv[u][0] = *reinterpret_cast<const uint4*>(wrow + k / 2 + 16 * g);
                sv[u] = srow[(size_t)(group ? k / group : 0) * 4];
            } else {
#pragma unroll
                for (int j = 0; j < 4; j++) wv[u][j] = *reinterpret_cast<const uint4*>(wrow + (size_t)(k + 32 * g + 8 * j) * 2);
            }
        }
#pragma unroll
        for (int u = 0; u < UU; u++)
#pragma unroll
            for (int j = 0; j < 4; j++)
                xv[u][j] = has_x ? *reinterpret_cast<const uint4*>(xrow + k0 + 128u * u + 32 * g + 8 * j) : make_uint4(0, 0, 0, 0);
#pragma unroll
        for (int u = 0; u < UU; u++) {
            float s = 0.0f, ms8 = 0.0f;
            if (Q4) {
                s = bf2f(sv[u]);
                ms8 = -8.0f * s;
            }
#pragma unroll
            for (int j = 0; j < 4; j++) {
                uint4 a;
                if (Q4) {
                    const uint32_t d = j == 0 ? wv[u][0].x : (j == 1 ? wv[u][0].y : (j == 2 ? wv[u][0].z : wv[u][0].w));
                    a = bg_dequant(d, s, ms8);
                } else {
                    a = wv[u][Q4 ? 0 : j];
                }
                acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bg_bf16x8, a), __builtin_bit_cast(bg_bf16x8, xv[u][j]),
                                                              acc, 0, 0, 0);
            }
        }
    };
    uint32_t k = kb;
    for (; k + 128u * U <= ke; k += 128u * U) chunks(k, std::integral_constant<int, U>{});
    for (; k < ke; k += 128u) chunks(k, std::integral_constant<int, 1>{});

    part[wave][lane] = acc;
    __syncthreads();
    if (wave != 0 || m >= B) return;
    bg_f32x4 v = part[0][lane];
#pragma unroll
    for (int w2 = 1; w2 < BG_WAVES; w2++) v += part[w2][lane]; // wave order
    // lane (n = m, g) holds rows 16 blockIdx.x + 4 g + i of batch row n
    const uint32_t n = m, r0 = blockIdx.x * 16 + 4 * g;
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

#define MC_BGEMV(FMT, Q4, E)                                                                                                      \
    extern "C" __global__ void __launch_bounds__(64 * BG_WAVES)                                                                   \
    mc_b_gemv_##FMT##_bfloat_e##E(const uint8_t* w, const bf16_t* scales, const bf16_t* x, bf16_t* y, uint32_t K,                \
                                  uint32_t ngroups, uint32_t group, uint32_t B, uint32_t ldy)                                     \
    {                                                                                                                             \
        bgemv_body<Q4, E>(w, scales, x, y, K, ngroups, group, B, ldy);                                                            \
    }
MC_BGEMV(i4, true, 0)
MC_BGEMV(i4, true, 1)
MC_BGEMV(i4, true, 2)
MC_BGEMV(w, false, 0)
MC_BGEMV(w, false, 1)
MC_BGEMV(w, false, 2)

// ------------------------------------------------------------------------------------------
// Per-row state: rows[r] is batch row r's step_state -- .token (the input token of the step, overwritten by its pick) and
// .step_index (i * B + r for token i of a chained call: the seed pair and the slot of tokens_out the pick fills, exactly as the
// batch-1 sampler uses them).  grid y = batch row everywhere below.
// ------------------------------------------------------------------------------------------
// embedding rows (embed_body / embed_q8_body): advance = this launch starts a chained step -- row r's step_index moves by B
extern "C" __global__ void
mc_b_embed_bfloat(const bf16_t* table, const float* q8_scales, const int8_t* q8_table, bf16_t* out, step_state* rows,
                  uint32_t dim, int32_t advance, uint32_t B)
{
    const uint32_t r = blockIdx.y, k = blockIdx.x * blockDim.x + threadIdx.x;
    const int32_t token = rows[r].token;
    if (advance && k == 0) rows[r].step_index += (int32_t)B;
    if (k >= dim) return;
    bf16_t v;
    if (q8_table) v = f2bf(BF::rt((float)q8_table[(size_t)token * dim + k] * BF::rt(q8_scales[token])));
    else v = table[(size_t)token * dim + k];
    out[(size_t)r * dim + k] = v;
}

extern "C" __global__ void
mc_b_rmsnorm_bfloat(const bf16_t* x, const bf16_t* w, bf16_t* out, uint32_t dim, float eps)
{
    const size_t o = (size_t)blockIdx.y * dim;
    rmsnorm_row_body<BF>(x + o, w, nullptr, out + o, dim, eps, 0.0f);
}

// grid (H + 2 KV, B): row r's q heads rotated into q_out[r], its K / V rows into ITS cache (row stride `cache_stride`
// elements between the rows' caches of one layer) at the shared step's slot
extern "C" __global__ void
mc_b_rope_kv_bfloat(const bf16_t* qkv, bf16_t* q_out, bf16_t* kc, bf16_t* vt, const float* fcos, const float* fsin,
                    const step_state* st, uint32_t H, uint32_t KV, uint32_t hd, uint32_t max_seq, uint64_t cache_stride)
{
    const uint32_t r = blockIdx.y;
    rope_kv_body<BF>(qkv + (size_t)r * (H + 2 * KV) * hd, q_out + (size_t)r * H * hd, kc + r * cache_stride, vt + r * cache_stride,
                     fcos, fsin, nullptr, nullptr, st, H, KV, hd, max_seq, 0.0f, 0.0f);
}

// grid (nsplit, KV, B), 256 threads: mc_attn_scores_bfloat per row
extern "C" __global__ void __launch_bounds__(256)
mc_b_attn_scores_bfloat(const bf16_t* q, const bf16_t* kc, float* expv, float* psum, const step_state* st, uint32_t n_rep,
                        uint32_t hd, uint32_t max_seq, float scale, uint32_t nsplit, uint64_t cache_stride)
{
    const uint32_t r = blockIdx.z, H = gridDim.y * n_rep;
    const bf16_t* qr = q + (size_t)r * H * hd;
    const bf16_t* kr = kc + r * cache_stride;
    float* er = expv + (size_t)r * H * max_seq;
    float* pr = psum + (size_t)r * H * nsplit;
    if (hd == 128) attn_scores_bf<128>(qr, kr, er, pr, nullptr, st, n_rep, max_seq, scale, nsplit);
    else if (hd == 64) attn_scores_bf<64>(qr, kr, er, pr, nullptr, st, n_rep, max_seq, scale, nsplit);
}

// grid (hd / 16, KV, B), 1024 threads: mc_attn_pv_bfloat per row over the whole context (one range)
extern "C" __global__ void __launch_bounds__(1024)
mc_b_attn_pv_bfloat(const float* expv, const float* psum, const bf16_t* vt, bf16_t* out, const step_state* st, uint32_t n_rep,
                    uint32_t hd, uint32_t max_seq, uint32_t nsplit, uint64_t cache_stride)
{
    const uint32_t r = blockIdx.z, H = gridDim.y * n_rep;
    attn_pv_bf_body(expv + (size_t)r * H * max_seq, psum + (size_t)r * H * nsplit, vt + r * cache_stride, out + (size_t)r * H * hd,
                    st, n_rep, hd, max_seq, nsplit, nullptr, H, 0, 1);
}

// greedy pick per row: the first index of the maximum (make_key: value descending, then lower index), one workgroup per row
__device__ __forceinline__ void
argmax_row_body(const bf16_t* logits, uint32_t n, step_state* rows, int32_t* tokens_out)
{
    __shared__ unsigned long long wk[16];
    const uint32_t r = blockIdx.y;
    const bf16_t* lr = logits + (size_t)r * n;
    unsigned long long best = 0ull;
    for (uint32_t i = threadIdx.x; i < n; i += blockDim.x) best = max(best, (unsigned long long)make_key(bf2f(lr[i]), i));
    for (int off = 32; off >= 1; off >>= 1) best = max(best, (unsigned long long)__shfl_xor(best, off, 64));
    if ((threadIdx.x & 63) == 0) wk[threadIdx.x >> 6] = best;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (uint32_t w = 1; w < (blockDim.x + 63) / 64; w++) best = max(best, wk[w]);
        const int32_t token = (int32_t)key_index(best);
        rows[r].token = token;
        if (tokens_out) tokens_out[rows[r].step_index] = token;
    }
}
extern "C" __global__ void __launch_bounds__(1024)
mc_b_argmax_bfloat(const bf16_t* logits, uint32_t n, step_state* rows, int32_t* tokens_out)
{
    argmax_row_body(logits, n, rows, tokens_out);
}

// make_default_sampler per row: launch 1 (grid (lists, B)) and launch 2 (grid (1, B)) of sampler_kernels.hip
extern "C" __global__ void __launch_bounds__(64)
mc_b_topk_candidates_bfloat(const bf16_t* logits, uint32_t n, uint32_t kpad, uint64_t* cand, uint32_t chunk)
{
    const uint32_t r = blockIdx.y;
    const bf16_t* lr = logits + (size_t)r * n;
    uint64_t* cr = cand + (size_t)r * gridDim.x * kpad;
    if (chunk == 512) topk_candidates_body<BF, 8>(lr, n, kpad, cr);
    else if (chunk == 1024) topk_candidates_body<BF, 16>(lr, n, kpad, cr);
    else if (chunk == 2048) topk_candidates_body<BF, 32>(lr, n, kpad, cr);
}
extern "C" __global__ void
mc_b_sample_bfloat(const uint64_t* cand, sampler_params p, const uint64_t* seeds, uint32_t n_seed_pairs, step_state* rows,
                   int32_t* tokens_out)
{
    const uint32_t r = blockIdx.y;
    sample_body<BF>(cand + (size_t)r * p.ncand, p, seeds, n_seed_pairs, rows + r, tokens_out,
                    nullptr);
}

// ------------------------------------------------------------------------------------------
// Ragged rows (mc_ragged_*, Part 2c): every row at a position of its own.  rows[r] is then row r's whole step state -- pos,
// kv_len = pos + 1, write_slot = pos and rope_row = pos (a batch's cache never turns and its rope table starts at position 0)
// -- and rows[r].pos < 0 marks an IDLE row: no launch below reads its token, reads or writes its cache, or writes rows[r] or
// tokens_out for it.  The launches are thin wrappers over the lockstep kernels' bodies given rows + r for the shared state, so
// a row at position p computes the bits a lockstep batch computes at p.  The grids are the lockstep grids; an idle row's
// workgroups exit at once, and scores workgroups past a row's kv_len exit as they always do, so a row costs its own length.
// ------------------------------------------------------------------------------------------
__device__ __forceinline__ bool
row_idle(const step_state* rows, uint32_t r)
{
    return rows[r].pos < 0;
}

// starts a ragged step (in place of the lockstep mc_step_set), one thread per row.  advance = 0 (token 0 of a call): the host
// wrote .token, .pos and .step_index; the rest is derived.  advance = 1 (a chained step): .token holds the row's previous pick.
// The row turns idle if that pick is one of stop_ids[0, n_stop) or its last write was slot max_seq - 1; otherwise it moves to
// pos + 1 and its step_index by B, as the lockstep advance does.
extern "C" __global__ void __launch_bounds__(64)
mc_b_rows_begin(step_state* rows, const int32_t* stop_ids, int32_t n_stop, int32_t max_seq, int32_t B, int32_t advance)
{
    const int32_t r = (int32_t)threadIdx.x;
    if (r >= B || row_idle(rows, r)) return;
    int32_t pos = rows[r].pos;
    if (advance) {
        bool stop = pos >= max_seq - 1;
        const int32_t token = rows[r].token;
        for (int32_t i = 0; i < n_stop && !stop; i++) stop = token == stop_ids[i];
        if (stop) {
            rows[r].pos = -1;
            return;
        }
        pos += 1;
        rows[r].pos = pos;
        rows[r].step_index += B;
    }
    rows[r].kv_len = pos + 1;
    rows[r].write_slot = pos;
    rows[r].rope_row = pos;
}

// mc_b_embed_bfloat without the advance (mc_b_rows_begin did it); an idle row gets zeros and its token is never read
extern "C" __global__ void
mc_b_embed_rows_bfloat(const bf16_t* table, const float* q8_scales, const int8_t* q8_table, bf16_t* out, const step_state* rows,
                       uint32_t dim)
{
    const uint32_t r = blockIdx.y, k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= dim) return;
    bf16_t v = 0; // +0.0
    if (!row_idle(rows, r)) {
        const int32_t token = rows[r].token;
        if (q8_table) v = f2bf(BF::rt((float)q8_table[(size_t)token * dim + k] * BF::rt(q8_scales[token])));
        else v = table[(size_t)token * dim + k];
    }
    out[(size_t)r * dim + k] = v;
}

// mc_b_rope_kv_bfloat at row r's own slot and rope row
extern "C" __global__ void
mc_b_rope_kv_rows_bfloat(const bf16_t* qkv, bf16_t* q_out, bf16_t* kc, bf16_t* vt, const float* fcos, const float* fsin,
                         const step_state* rows, uint32_t H, uint32_t KV, uint32_t hd, uint32_t max_seq, uint64_t cache_stride)
{
    const uint32_t r = blockIdx.y;
    if (row_idle(rows, r)) return;
    rope_kv_body<BF>(qkv + (size_t)r * (H + 2 * KV) * hd, q_out + (size_t)r * H * hd, kc + r * cache_stride, vt + r * cache_stride,
                     fcos, fsin, nullptr, nullptr, rows + r, H, KV, hd, max_seq, 0.0f, 0.0f);
}

// mc_b_attn_scores_bfloat over row r's own kv_len
extern "C" __global__ void __launch_bounds__(256)
mc_b_attn_scores_rows_bfloat(const bf16_t* q, const bf16_t* kc, float* expv, float* psum, const step_state* rows, uint32_t n_rep,
                             uint32_t hd, uint32_t max_seq, float scale, uint32_t nsplit, uint64_t cache_stride)
{
    const uint32_t r = blockIdx.z, H = gridDim.y * n_rep;
    if (row_idle(rows, r)) return;
    const bf16_t* qr = q + (size_t)r * H * hd;
    const bf16_t* kr = kc + r * cache_stride;
    float* er = expv + (size_t)r * H * max_seq;
    float* pr = psum + (size_t)r * H * nsplit;
    if (hd == 128) attn_scores_bf<128>(qr, kr, er, pr, nullptr, rows + r, n_rep, max_seq, scale, nsplit);
    else if (hd == 64) attn_scores_bf<64>(qr, kr, er, pr, nullptr, rows + r, n_rep, max_seq, scale, nsplit);
}

// mc_b_attn_pv_bfloat over row r's own kv_len; an idle row's attention output is zeros (what Wo then reads for it)
extern "C" __global__ void __launch_bounds__(1024)
mc_b_attn_pv_rows_bfloat(const float* expv, const float* psum, const bf16_t* vt, bf16_t* out, const step_state* rows, uint32_t n_rep,
                         uint32_t hd, uint32_t max_seq, uint32_t nsplit, uint64_t cache_stride)
{
    const uint32_t r = blockIdx.z, H = gridDim.y * n_rep;
    if (row_idle(rows, r)) {
        // this workgroup's part of the output: heads kv * n_rep + [0, n_rep), dims 16 blockIdx.x + [0, 16)
        if (threadIdx.x < n_rep * 16)
            out[(size_t)r * H * hd + (size_t)(blockIdx.y * n_rep + threadIdx.x / 16) * hd + blockIdx.x * 16 + threadIdx.x % 16] = 0;
        return;
    }
    attn_pv_bf_body(expv + (size_t)r * H * max_seq, psum + (size_t)r * H * nsplit, vt + r * cache_stride, out + (size_t)r * H * hd,
                    rows + r, n_rep, hd, max_seq, nsplit, nullptr, H, 0, 1);
}

extern "C" __global__ void __launch_bounds__(1024)
mc_b_argmax_rows_bfloat(const bf16_t* logits, uint32_t n, step_state* rows, int32_t* tokens_out)
{
    if (row_idle(rows, blockIdx.y)) return;
    argmax_row_body(logits, n, rows, tokens_out);
}

// launch 2 of the default sampler; launch 1 (mc_b_topk_candidates_bfloat) runs for every row, an idle one on zero logits
extern "C" __global__ void
mc_b_sample_rows_bfloat(const uint64_t* cand, sampler_params p, const uint64_t* seeds, uint32_t n_seed_pairs, step_state* rows,
                        int32_t* tokens_out)
{
    const uint32_t r = blockIdx.y;
    if (row_idle(rows, r)) return;
    sample_body<BF>(cand + (size_t)r * p.ncand, p, seeds, n_seed_pairs, rows + r, tokens_out,
                    nullptr);
}
