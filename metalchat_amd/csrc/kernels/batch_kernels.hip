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
// v_cvt_pk_bf16_f32 -- T(T(q) T(s)).  Scales: bfloat row quads [out/4][in/group][4]; group % 32 == 0 or 0 (one per row).  A lane's 32
// weights of a chunk lie inside one group, so its scale is group (k0 + 32 g) / group: one bfloat load per lane and chunk (for
// group % 128 == 0 that is k0 / group for every g).
// int8 (mc_b_gemv_i8_*): int8 [out][in] row-major, the same scale quads.  Lane (m, g) loads row m's 32 bytes k0 + 32 g + [0, 32)
// (two 16-byte loads); MFMA j takes bytes 8 j .. 8 j + 7.  (float)q * s is exact in fp32 (8 x 8 significant bits), rounded once to
// bfloat by v_cvt_pk_bf16_f32 -- T(T(q) T(s)); no -8 s term.
// Adaptors (mc_b_gemv_*_l; quantization::lora_linear, quantization/lora.h:119-121; gemv.h finish_pair): behind the usual arguments
// (a, lda, lora_b, lora_cols, lora_scale) with a[n][c] = T(A x[n]) at row stride lda (an ordinary mc_b_gemv_w_bfloat_e0 over the stacked A
// wrote it) and lora_b [out][lora_cols] in fused row order, zeros outside a row's own adaptor columns; lora_cols % 16 == 0.  With v
// the fp32 sum of (activation row n, weight row r) after the slice fold,
//   o = T(T(v) + T(T(p) T(lora_scale))),  p = sum_c a[n][c] lora_b[r][c]
// and the e0 / e1 / e2 epilogue runs on o.  THE ORDER OF p: ONE fp32 accumulator per output, starting at +0, columns c = 0, 1, ..,
// lora_cols - 1 in ascending order, p = p + a_c b_c with the product exact in fp32 (8 x 8 significant bits) and one rounding per
// addition.  mc_wb_gemv_*_l (wide_kernels.hip) runs the same function (bg_lora_sum).  The first 16 columns are loaded before the
// barrier of the slice fold, the rest one 16-column block ahead of its use.
// ------------------------------------------------------------------------------------------
enum { BEPI_STORE = 0, BEPI_RESID = 1, BEPI_SILU_MUL = 2 };
enum { BFMT_W = 0, BFMT_I4 = 1, BFMT_I8 = 2 }; // the weight format of a batched GEMV kernel

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

// int8: dwords (d0, d1) are weights 8 j .. 8 j + 7 of a lane's 32 in natural order; T(T(q) T(s)) each
__device__ __forceinline__ uint4
bg_dequant8(uint32_t d0, uint32_t d1, float s)
{
    uint32_t o[4];
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const uint32_t d = j < 2 ? d0 : d1;
        const int sh = 16 * (j & 1);
        const float a = (float)(int32_t)(int8_t)(d >> sh) * s;
        const float c = (float)(int32_t)(int8_t)(d >> (sh + 8)) * s;
        o[j] = pack_bf16x2(a, c);
    }
    return make_uint4(o[0], o[1], o[2], o[3]);
}

// The adaptor term of one lane: activation row n's a[0, cols) against the four weight rows r0 .. r0 + 3 of lora_b, 16 columns
// a block.  p[i] takes columns in ascending order, one fp32 addition per column (the header states the order).
struct bg_lora_block {
    uint4 a[2], b[4][2];
};
__device__ __forceinline__ bg_lora_block
bg_lora_load(const bf16_t* __restrict__ arow, const bf16_t* __restrict__ brow, uint32_t cols, uint32_t c0)
{
    bg_lora_block k;
#pragma unroll
    for (int h = 0; h < 2; h++) {
        k.a[h] = *reinterpret_cast<const uint4*>(arow + c0 + 8 * h);
#pragma unroll
        for (int i = 0; i < 4; i++) k.b[i][h] = *reinterpret_cast<const uint4*>(brow + (size_t)i * cols + c0 + 8 * h);
    }
    return k;
}
__device__ __forceinline__ void
bg_lora_add(float (&p)[4], const bg_lora_block& k)
{
#pragma unroll
    for (int h = 0; h < 2; h++) {
        const uint32_t av[4] = {k.a[h].x, k.a[h].y, k.a[h].z, k.a[h].w};
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const uint32_t bv[4] = {k.b[i][h].x, k.b[i][h].y, k.b[i][h].z, k.b[i][h].w};
#pragma unroll
            for (int e = 0; e < 4; e++) {
                p[i] = p[i] + __uint_as_float(av[e] << 16) * __uint_as_float(bv[e] << 16);
                p[i] = p[i] + __uint_as_float(av[e] & 0xFFFF0000u) * __uint_as_float(bv[e] & 0xFFFF0000u);
            }
        }
    }
}
// first: columns [0, 16), loaded by the caller before its barrier
__device__ __forceinline__ void
bg_lora_sum(float (&p)[4], bg_lora_block first, const bf16_t* __restrict__ arow, const bf16_t* __restrict__ brow, uint32_t cols)
{
#pragma unroll
    for (int i = 0; i < 4; i++) p[i] = 0.0f;
    bg_lora_block cur = first;
    for (uint32_t c0 = 16; c0 < cols; c0 += 16) {
        const bg_lora_block next = bg_lora_load(arow, brow, cols, c0);
        bg_lora_add(p, cur);
        cur = next;
    }
    bg_lora_add(p, cur);
}

// The epilogue of the batched GEMVs on the four fp32 sums v of one lane: weight rows r0 .. r0 + 3 of the activation row whose
// output row is yr.  p: the adaptor sums (LORA), lscale_T = T(lora_scale)
template <int EPI, bool LORA>
__device__ __forceinline__ void
bg_epilogue(const bg_f32x4 v, const float (&p)[4], float lscale_T, bf16_t* __restrict__ yr, uint32_t r0)
{
    float o[4];
#pragma unroll
    for (int i = 0; i < 4; i++) {
        o[i] = BF::rt(v[i]);
        if (LORA) o[i] = BF::rt(o[i] + BF::rt(BF::rt(p[i]) * lscale_T)); // T(T(x Wd^T) + T(T(B (A x)) * scale))
    }
    if (EPI == BEPI_SILU_MUL) {
        // w1 | w3 rows interleaved (2j, 2j + 1): out[j] = T(silu(T(w1 x)) * T(w3 x))   (gemv.h EPI_SILU_MUL)
#pragma unroll
        for (int i = 0; i < 4; i += 2) yr[(r0 + i) / 2] = f2bf(mc::gemv::silu_T<BF>(o[i]) * o[i + 1]);
    } else {
#pragma unroll
        for (int i = 0; i < 4; i++) {
            if (EPI == BEPI_RESID) o[i] = bf2f(yr[r0 + i]) + o[i]; // residual added in T (gemv.h EPI_RESID)
            yr[r0 + i] = f2bf(o[i]);
        }
    }
}

template <int FMT, int EPI, bool LORA>
__device__ __forceinline__ void
bgemv_body(const uint8_t* __restrict__ w, const bf16_t* __restrict__ scales, const bf16_t* __restrict__ x,
           bf16_t* __restrict__ y, uint32_t K, uint32_t ngroups, uint32_t group, uint32_t B, uint32_t ldy,
           const bf16_t* __restrict__ la = nullptr, uint32_t lda = 0, const bf16_t* __restrict__ lb = nullptr, uint32_t lcols = 0,
           float lscale = 0.0f)
{
    constexpr bool Q4 = FMT == BFMT_I4, Q8 = FMT == BFMT_I8, QS = Q4 || Q8;
    constexpr int U = QS ? 4 : 2; // 128-weight chunks per round of loads
    constexpr int NWD = Q4 ? 1 : (Q8 ? 2 : 4);
    __shared__ bg_f32x4 part[BG_WAVES][64];
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t m = lane & 15, g = lane >> 4;
    const uint32_t row = blockIdx.x * 16 + m; // the weight row this lane loads
    const size_t rowbytes = Q4 ? (size_t)K / 2 : (Q8 ? (size_t)K : (size_t)K * 2);
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
            if (QS) sv[u] = srow[(size_t)(group ? (k + 32 * g) / group : 0) * 4];
            if (Q4) {
                wv[u][0] = *reinterpret_cast<const uint4*>(wrow + k / 2 + 16 * g);
            } else if (Q8) {
#pragma unroll
                for (int j = 0; j < 2; j++) wv[u][j] = *reinterpret_cast<const uint4*>(wrow + k + 32 * g + 16 * j);
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
            if (QS) s = bf2f(sv[u]);
            if (Q4) ms8 = -8.0f * s;
#pragma unroll
            for (int j = 0; j < 4; j++) {
                uint4 a;
                if (Q4) {
                    const uint32_t d = j == 0 ? wv[u][0].x : (j == 1 ? wv[u][0].y : (j == 2 ? wv[u][0].z : wv[u][0].w));
                    a = bg_dequant(d, s, ms8);
                } else if (Q8) {
                    const uint4 q = wv[u][j / 2];
                    a = (j & 1) ? bg_dequant8(q.z, q.w, s) : bg_dequant8(q.x, q.y, s);
                } else {
                    a = wv[u][j];
                }
                acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bg_bf16x8, a), __builtin_bit_cast(bg_bf16x8, xv[u][j]),
                                                              acc, 0, 0, 0);
            }
        }
    };
    uint32_t k = kb;
    for (; k + 128u * U <= ke; k += 128u * U) chunks(k, std::integral_constant<int, U>{});
    for (; k < ke; k += 128u) chunks(k, std::integral_constant<int, 1>{});

    // lane (n = m, g) of wave 0 holds rows 16 blockIdx.x + 4 g + i of batch row n
    const uint32_t n = m, r0 = blockIdx.x * 16 + 4 * g;
    const bool folds = wave == 0 && m < B;
    const bf16_t* arow = la + (size_t)n * lda;
    const bf16_t* brow = lb + (size_t)r0 * lcols;
    bg_lora_block first;
    if (LORA && folds) first = bg_lora_load(arow, brow, lcols, 0);
    part[wave][lane] = acc;
    __syncthreads();
    if (!folds) return;
    bg_f32x4 v = part[0][lane];
#pragma unroll
    for (int w2 = 1; w2 < BG_WAVES; w2++) v += part[w2][lane]; // wave order
    float p[4] = {0.f, 0.f, 0.f, 0.f};
    if (LORA) bg_lora_sum(p, first, arow, brow, lcols);
    bg_epilogue<EPI, LORA>(v, p, BF::rt(lscale), y + (size_t)n * ldy, r0);
}

#define MC_BGEMV(FMT, F, E)                                                                                                       \
    extern "C" __global__ void __launch_bounds__(64 * BG_WAVES)                                                                   \
    mc_b_gemv_##FMT##_bfloat_e##E(const uint8_t* w, const bf16_t* scales, const bf16_t* x, bf16_t* y, uint32_t K,                \
                                  uint32_t ngroups, uint32_t group, uint32_t B, uint32_t ldy)                                     \
    {                                                                                                                             \
        bgemv_body<F, E, false>(w, scales, x, y, K, ngroups, group, B, ldy);                                                      \
    }                                                                                                                             \
    extern "C" __global__ void __launch_bounds__(64 * BG_WAVES)                                                                   \
    mc_b_gemv_##FMT##_bfloat_e##E##_l(const uint8_t* w, const bf16_t* scales, const bf16_t* x, bf16_t* y, uint32_t K,            \
                                      uint32_t ngroups, uint32_t group, uint32_t B, uint32_t ldy, const bf16_t* a, uint32_t lda,  \
                                      const bf16_t* lora_b, uint32_t lora_cols, float lora_scale)                                 \
    {                                                                                                                             \
        bgemv_body<F, E, true>(w, scales, x, y, K, ngroups, group, B, ldy, a, lda, lora_b, lora_cols, lora_scale);                \
    }
MC_BGEMV(i4, BFMT_I4, 0)
MC_BGEMV(i4, BFMT_I4, 1)
MC_BGEMV(i4, BFMT_I4, 2)
MC_BGEMV(i8, BFMT_I8, 0)
MC_BGEMV(i8, BFMT_I8, 1)
MC_BGEMV(i8, BFMT_I8, 2)
MC_BGEMV(w, BFMT_W, 0)
MC_BGEMV(w, BFMT_W, 1)
MC_BGEMV(w, BFMT_W, 2)

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
// MC_SAMPLER_DRAW per row: mc_b_sample_bfloat with the drawing last phase (sampler_kernels.hip draw_position); named outside
// mc_b_* like its batch-1 form mc_draw_bfloat
extern "C" __global__ void
mc_draw_b_bfloat(const uint64_t* cand, sampler_params p, const uint64_t* seeds, uint32_t n_seed_pairs, step_state* rows,
                 int32_t* tokens_out)
{
    const uint32_t r = blockIdx.y;
    sample_body<BF, SAMPLE_LAST_DRAW>(cand + (size_t)r * p.ncand, p, seeds, n_seed_pairs, rows + r, tokens_out, nullptr);
}

// ------------------------------------------------------------------------------------------
// Ragged rows (mc_ragged_*, Part 2c): every row at a position of its own.  rows[r] is then row r's whole step state -- pos,
// kv_len = pos + 1, write_slot = pos and rope_row = pos (a batch's cache never turns and its rope table starts at position 0)
// -- and rows[r].pos < 0 marks an IDLE row: no launch below reads its token, reads or writes its cache, or writes rows[r] or
// tokens_out for it.  The launches are thin wrappers over the lockstep kernels' bodies given rows + r for the shared state, so
// a row at position p computes the bits a lockstep batch computes at p.  The grids are the lockstep grids; an idle row's
// workgroups exit at once, and scores workgroups past a row's kv_len exit as they always do, so a row costs its own length.
// A rolling batch (Part 2j) starts its steps with mc_b_rows_begin_rolling instead, which gives a row past the end the ring's
// write_slot and a rope row of its own; the launches behind it are these.
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

// Rolling rows (mc_rolling_set, Part 2j): mc_b_rows_begin for a batch whose rows decode past max_seq on nn::sink_cache's
// ring (nn/cache.h:187-204), one 64-thread workgroup per row (grid x = B).  Two differences:
//   * a row never stops for the end of its cache -- on its stop ids only -- and at pos >= max_seq it takes the state derive_state
//     (decode_kernels.hip) reaches after pos - max_seq + 1 single-step rolls from a linear cache: ring_base = (pos - max_seq + 1)
//     % post, write_slot = pre_len + (post - 1 + ring_base) % post, kv_len = max_seq.  Rows get past the end by single steps only,
//     so this is a function of pos alone and nothing is kept between calls; below max_seq the state is mc_b_rows_begin's.
//   * the rope row.  The batch's table ends at max_seq and the rows of one call can be any distance apart, so thread j < hd / 2
//     writes cos / sin of pair j at the row's absolute position into row r of rcos / rsin [B][hd / 2] -- rope_entry, the bits of
//     mc_rope_table's row for that position -- and rope_row = r: mc_b_rope_kv_rows_bfloat is given rcos / rsin for the table.
//     EVERY active row of a rolling batch takes this path, below max_seq as well: one path, and the same bits as the table's.
// Every thread reads the row's state before thread 0 rewrites it (the barrier); a chained step needs no host round trip.
extern "C" __global__ void __launch_bounds__(64)
mc_b_rows_begin_rolling(step_state* rows, const int32_t* stop_ids, int32_t n_stop, int32_t max_seq, int32_t pre_len, int32_t advance,
                        float* rcos, float* rsin, uint32_t hd, float theta)
{
    const uint32_t r = blockIdx.x, j = threadIdx.x, half = hd / 2;
    if (row_idle(rows, r)) return; // (uniform)
    int32_t pos = rows[r].pos;
    const int32_t token = rows[r].token, step_index = rows[r].step_index;
    bool stop = false;
    if (advance) {
        for (int32_t i = 0; i < n_stop && !stop; i++) stop = token == stop_ids[i];
        pos += 1;
    }
    __syncthreads();
    if (stop) {
        if (j == 0) rows[r].pos = -1;
        return;
    }
    if (j < half) rope_entry((uint32_t)pos, j, hd, theta, &rcos[(size_t)r * half + j], &rsin[(size_t)r * half + j]);
    if (j != 0) return;
    const int32_t post = max_seq - pre_len;
    int32_t ring_base = 0, write_slot = pos, kv_len = pos + 1;
    if (pos >= max_seq) {
        ring_base = (pos - max_seq + 1) % post;
        write_slot = pre_len + (post - 1 + ring_base) % post;
        kv_len = max_seq;
    }
    rows[r].pos = pos;
    if (advance) rows[r].step_index = step_index + (int32_t)gridDim.x;
    rows[r].kv_len = kv_len;
    rows[r].write_slot = write_slot;
    rows[r].ring_base = ring_base;
    rows[r].rope_row = (int32_t)r;
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
extern "C" __global__ void
mc_draw_b_rows_bfloat(const uint64_t* cand, sampler_params p, const uint64_t* seeds, uint32_t n_seed_pairs, step_state* rows,
                      int32_t* tokens_out)
{
    const uint32_t r = blockIdx.y;
    if (row_idle(rows, r)) return;
    sample_body<BF, SAMPLE_LAST_DRAW>(cand + (size_t)r * p.ncand, p, seeds, n_seed_pairs, rows + r, tokens_out, nullptr);
}

// ------------------------------------------------------------------------------------------
// Row samplers (mc_row_sampler_*, Part 2k): every row picks with settings of its own.  samplers[r] holds row r's EFFECTIVE
// settings (abi.h row_sampler, resolved on the host: greedy, the default sampler or the drawing one, never "inherit").  The two launches are the
// uniform ones with the branch on the row's kind in front -- uniform per workgroup, the row is a grid index -- so a greedy row
// computes mc_b_argmax_*'s pick, a default row mc_b_sample_*'s and a drawing row mc_draw_b_*'s (the chain is one, the last phase the row's):
//   launch 1  the candidate lists of the sampling rows with the CALL's kpad, the largest among its sampling rows.  The lists are
//             exact (list w = the kpad best keys of chunk w, best first), so a row's k best keys are among the first k of each
//             list whatever kpad >= k is: a larger kpad only appends keys that launch 2 drops.  Workgroups of greedy rows
//             (and, ragged, of idle rows) exit at once.
//   launch 2  one workgroup of 1024 threads per row -- the argmax's block size.  sample_body guards every phase by tid (its
//             strides take blockDim.x), and the k best of the keys it collects do not depend on how many threads collected them.
// ------------------------------------------------------------------------------------------
// ragged: rows[r].pos < 0 marks an idle row (the lockstep calls do not maintain .pos)
extern "C" __global__ void __launch_bounds__(64)
mc_b_topk_candidates_mixed_bfloat(const bf16_t* logits, uint32_t n, uint32_t kpad, uint64_t* cand, uint32_t chunk,
                                  const row_sampler* samplers, const step_state* rows, int32_t ragged)
{
    const uint32_t r = blockIdx.y;
    if (samplers[r].kind == ROW_SAMPLER_GREEDY || (ragged && row_idle(rows, r))) return;
    const bf16_t* lr = logits + (size_t)r * n;
    uint64_t* cr = cand + (size_t)r * gridDim.x * kpad;
    if (chunk == 512) topk_candidates_body<BF, 8>(lr, n, kpad, cr);
    else if (chunk == 1024) topk_candidates_body<BF, 16>(lr, n, kpad, cr);
    else if (chunk == 2048) topk_candidates_body<BF, 32>(lr, n, kpad, cr);
}

// nlists, kpad, cap: of the call (sampler_params' words of the same names); dynamic LDS: cap keys
__device__ __forceinline__ void
pick_mixed_body(const bf16_t* logits, uint32_t n, const uint64_t* cand, const row_sampler* samplers, uint32_t nlists, uint32_t kpad,
                uint32_t cap, const uint64_t* seeds, uint32_t n_seed_pairs, step_state* rows, int32_t* tokens_out)
{
    const uint32_t r = blockIdx.y;
    const row_sampler s = samplers[r];
    if (s.kind == ROW_SAMPLER_GREEDY) {
        argmax_row_body(logits, n, rows, tokens_out);
        return;
    }
    const sampler_params p{s.k, nlists * kpad, cap, s.inv_temp, s.top_p, nlists, kpad};
    sample_body<BF, SAMPLE_LAST_ROW>(cand + (size_t)r * p.ncand, p, seeds, n_seed_pairs, rows + r, tokens_out, nullptr, s.kind == ROW_SAMPLER_DRAW);
}
extern "C" __global__ void __launch_bounds__(1024)
mc_b_pick_mixed_bfloat(const bf16_t* logits, uint32_t n, const uint64_t* cand, const row_sampler* samplers, uint32_t nlists,
                       uint32_t kpad, uint32_t cap, const uint64_t* seeds, uint32_t n_seed_pairs, step_state* rows, int32_t* tokens_out)
{
    pick_mixed_body(logits, n, cand, samplers, nlists, kpad, cap, seeds, n_seed_pairs, rows, tokens_out);
}
// an idle row gets no pick: nothing of rows[r] or tokens_out is written for it
extern "C" __global__ void __launch_bounds__(1024)
mc_b_pick_mixed_rows_bfloat(const bf16_t* logits, uint32_t n, const uint64_t* cand, const row_sampler* samplers, uint32_t nlists,
                            uint32_t kpad, uint32_t cap, const uint64_t* seeds, uint32_t n_seed_pairs, step_state* rows,
                            int32_t* tokens_out)
{
    if (row_idle(rows, blockIdx.y)) return;
    pick_mixed_body(logits, n, cand, samplers, nlists, kpad, cap, seeds, n_seed_pairs, rows, tokens_out);
}
