// fp8 KV caches of batch rows (mc_kv_batch_create with MC_KV_FP8, include/metalchat_hip.h Part 2o): a row's cache holds OCP e4m3 bytes and
// one power-of-two exponent per cache vector in place of bfloat16 values -- hd + 1 bytes per vector instead of 2 hd.  bfloat16 decoders,
// head_dim 128 and 64.
//
// The format is a STORAGE format (the rule: tests/kv_fp8_rule.py).  For one cache vector x of hd bfloat16 values -- one kv head's K, or its V, at
// one slot, as rope_kv_body stores them:
//   amax    = max |x|
//   e       = the smallest integer with amax 2^-e <= 448, clamped to [-100, 119]; -100 for amax = 0
//   byte[i] = e4m3(x[i] 2^-e), nearest, ties to even, saturating at +-448 (reached only at e = 119); the scaling is exact in float32
//   deq[i]  = e4m3(byte[i]) 2^e: a normal bfloat16 or a zero, exactly
// and a row computes bit for bit what it would compute if its bfloat16 cache held deq: the attention kernels below turn bytes and exponents into
// the bfloat16 MFMA operands of attn_scores_bf / attn_pv_bf_body (decode_kernels.hip) in registers and keep everything behind the operands -- the
// MFMA k assignment, the 64-slot splits and their psum, the lane-strided denominator sum, the wave-interleaved 32-slot k-steps added in wave
// order, the rounding points -- by calling those kernels' own tails (scores_finish, softmax_inv, pv_finish_store).
//
// Per layer and row four planes, each with its own row stride:
//   K bytes  [kv][max_seq][hd]      V bytes  [kv][hd][max_seq] (transposed, as Vt)      kexp, vexp  [kv][max_seq] int8
// How the data moves:
//   write    one workgroup of hd / 2 threads per kv head (a single wave, a thread per rotation pair): amax by a shuffle tree over the active lanes,
//            two bytes per thread out of one v_cvt_pk_fp8_f32, thread 0 stores the exponent.  q leaves as bfloat16 through rope_kv_body itself.
//   scores   lane (col, c) of a wave loads slot col's bytes d = 32 ks + 8 c + [0, 8) -- 8 bytes where the bfloat16 kernel loads 16, a wave's 16 slots
//            are 16 hd contiguous bytes -- and the slot's exponent (one byte, 16 addresses a wave); 8 bytes and ONE scale are four
//            v_cvt_scalef32_pk_bf16_fp8, whose result IS deq.  A slot past kv_len is never loaded (the load is clamped to kv_len - 1, as there).
//   P.V      lane (col, c) loads 8 slots of Vt row 16 db + col (8 bytes) and the 8 exponents of those slots (8 bytes, the same address in the 16
//            lanes that share c: one request); the eight slots carry eight scales, so a pair goes through v_cvt_pk_f32_fp8, two exact fp32
//            multiplies and one v_cvt_pk_bf16_f32.  Bytes AND exponents of slots past kv_len are masked to zero before the conversion: a NaN byte
//            or a stray exponent there becomes +0, which p = 0 meets -- the bfloat16 kernel relies on 0 x finite garbage instead.
//            The exponents are not staged in LDS: a workgroup spans all max_seq slots, which no static array bounds, and the 8-byte loads hit
//            the cache lines the neighbouring k-steps fetched.
//   quant    (mc_batch_fork, mc_batch_import_kv) 64 slots of one kv head per workgroup.  K: hd / 8 lanes per slot, 16 bytes in and 8 bytes out a
//            lane.  Vt: a thread keeps the hd / 4 values of ITS slot whose rows are d = wave + 4 i -- a wave reads 64 consecutive slots of one row --,
//            the four partial maxima of a slot meet in LDS, and every thread converts what it holds.
//   dequant  (the export calls) mc_kv_export_bfloat's loop with deq in place of the copy.
// Non-finite K / V values are out of scope: their bytes are unspecified.
#include "common.h"

using namespace mc;

typedef float kv8_f32x2 __attribute__((ext_vector_type(2)));

constexpr int32_t KV8_E_MIN = -100, KV8_E_MAX = 119;

// |x| of a bfloat16 as an integer: for finite values the order of the integers is the order of the magnitudes
__device__ __forceinline__ uint32_t
kv8_abs(bf16_t v)
{
    return (uint32_t)v & 0x7FFFu;
}

// e of a vector whose amax has the bfloat16 magnitude bits `abits`: amax = m 2^E with 1 <= m < 2 needs e = E - 8 for m <= 1.75 (448 = 1.75 x 2^8)
// and E - 7 above it; a subnormal or zero amax lands below the clamp
__device__ __forceinline__ int32_t
kv8_exponent(uint32_t abits)
{
    const int32_t e = (int32_t)(abits >> 7) - 127 - 8 + ((abits & 0x7Fu) > 0x60u ? 1 : 0);
    return min(max(e, KV8_E_MIN), KV8_E_MAX);
}

__device__ __forceinline__ float
kv8_pow2(int32_t e) // 2^e for e in [-126, 127]
{
    return __uint_as_float((uint32_t)(e + 127) << 23);
}

// bytes (lo = a, hi = b) of two values of a vector with exponent e; inv = 2^-e
__device__ __forceinline__ uint32_t
kv8_quant2(float a, float b, float inv)
{
    a = fminf(fmaxf(a * inv, -448.0f), 448.0f);
    b = fminf(fmaxf(b * inv, -448.0f), 448.0f);
    return (uint32_t)__builtin_amdgcn_cvt_pk_fp8_f32(a, b, 0, false) & 0xFFFFu;
}

// deq of one byte (the low byte of `byte`)
__device__ __forceinline__ bf16_t
kv8_deq1(uint32_t byte, int32_t e)
{
    const kv8_f32x2 f = __builtin_amdgcn_cvt_pk_f32_fp8((int)byte, false);
    return f2bf(f.x * kv8_pow2(e));
}

// 8 bytes of ONE vector (scale = 2^e) as 8 bfloat16
__device__ __forceinline__ uint4
kv8_deq8(uint2 b, float scale)
{
    uint4 o;
    o.x = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8((int)b.x, scale, false));
    o.y = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8((int)b.x, scale, true));
    o.z = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8((int)b.y, scale, false));
    o.w = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8((int)b.y, scale, true));
    return o;
}

// 8 bytes of EIGHT vectors (byte i with exponent byte i of x) as 8 bfloat16
template <bool HI>
__device__ __forceinline__ uint32_t
kv8_deq2x2(uint32_t bw, uint32_t xw) // the low (HI: high) two bytes of bw, each with the exponent byte at its own place in xw
{
    const kv8_f32x2 f = __builtin_amdgcn_cvt_pk_f32_fp8((int)bw, HI);
    const int32_t e0 = (int32_t)(int8_t)(xw >> (HI ? 16 : 0)), e1 = (int32_t)(int8_t)(xw >> (HI ? 24 : 8));
    return pack_bf16x2(f.x * kv8_pow2(e0), f.y * kv8_pow2(e1)); // exact: deq is a bfloat16
}
__device__ __forceinline__ uint4
kv8_deq8x8(uint2 b, uint2 x)
{
    return make_uint4(kv8_deq2x2<false>(b.x, x.x), kv8_deq2x2<true>(b.x, x.x), kv8_deq2x2<false>(b.y, x.y), kv8_deq2x2<true>(b.y, x.y));
}

// ------------------------------------------------------------------------------------------
// RoPE + cache write.  grid (H + 2 KV, B), hd / 2 threads: rope_kv_body's values; q through rope_kv_body itself
// ------------------------------------------------------------------------------------------
__device__ __forceinline__ void
rope_kv_f8_body(const bf16_t* qkv, bf16_t* q_out, uint8_t* kq, uint8_t* vq, int8_t* kexp, int8_t* vexp, const float* fcos, const float* fsin,
                const step_state* st, uint32_t H, uint32_t KV, uint32_t hd, uint32_t max_seq)
{
    const uint32_t b = blockIdx.x, j = threadIdx.x, half = hd / 2;
    if (b < H) { // (uniform)
        rope_kv_body<BF>(qkv, q_out, nullptr, nullptr, fcos, fsin, nullptr, nullptr, st, H, KV, hd, max_seq, 0.0f, 0.0f);
        return;
    }
    const uint32_t slot = (uint32_t)st->write_slot;
    const bool is_k = b < H + KV;
    const uint32_t kv = is_k ? b - H : b - H - KV;
    const bf16_t* src = qkv + (size_t)b * hd;
    bf16_t o1, o2; // elements j and j + half of the vector
    if (is_k) {
        // rope_kv_body: the rotation partners lie side by side in the fused GEMV's output
        const float x1 = bf2f(src[2 * j]), x2 = bf2f(src[2 * j + 1]);
        const float c = fcos[(size_t)st->rope_row * half + j], s = fsin[(size_t)st->rope_row * half + j];
        o1 = f2bf(c * x1 - s * x2);
        o2 = f2bf(s * x1 + c * x2);
    } else {
        o1 = src[j];
        o2 = src[j + half];
    }
    uint32_t amax = max(kv8_abs(o1), kv8_abs(o2));
    for (uint32_t off = half / 2; off >= 1; off >>= 1) amax = max(amax, (uint32_t)__shfl_xor((int)amax, (int)off, 64)); // active lanes only
    const int32_t e = kv8_exponent(amax);
    const uint32_t q2 = kv8_quant2(bf2f(o1), bf2f(o2), kv8_pow2(-e));
    const size_t vec = (size_t)kv * max_seq + slot;
    if (is_k) {
        kq[vec * hd + j] = (uint8_t)q2;
        kq[vec * hd + j + half] = (uint8_t)(q2 >> 8);
        if (j == 0) kexp[vec] = (int8_t)e;
    } else {
        uint8_t* dst = vq + (size_t)kv * hd * max_seq + slot;
        dst[(size_t)j * max_seq] = (uint8_t)q2;
        dst[(size_t)(j + half) * max_seq] = (uint8_t)(q2 >> 8);
        if (j == 0) vexp[vec] = (int8_t)e;
    }
}

// cache_stride: bytes between the rows' K (and V) byte planes of one layer, exp_stride: between their exponent planes
extern "C" __global__ void __launch_bounds__(64)
mc_b_rope_kv_f8_bfloat(const bf16_t* qkv, bf16_t* q_out, uint8_t* kq, uint8_t* vq, int8_t* kexp, int8_t* vexp, const float* fcos, const float* fsin,
                       const step_state* st, uint32_t H, uint32_t KV, uint32_t hd, uint32_t max_seq, uint64_t cache_stride, uint64_t exp_stride)
{
    const uint32_t r = blockIdx.y;
    rope_kv_f8_body(qkv + (size_t)r * (H + 2 * KV) * hd, q_out + (size_t)r * H * hd, kq + r * cache_stride, vq + r * cache_stride, kexp + r * exp_stride,
                    vexp + r * exp_stride, fcos, fsin, st, H, KV, hd, max_seq);
}

// ... at row r's own slot and rope row; an idle row writes nothing
extern "C" __global__ void __launch_bounds__(64)
mc_b_rope_kv_f8_rows_bfloat(const bf16_t* qkv, bf16_t* q_out, uint8_t* kq, uint8_t* vq, int8_t* kexp, int8_t* vexp, const float* fcos,
                            const float* fsin, const step_state* rows, uint32_t H, uint32_t KV, uint32_t hd, uint32_t max_seq, uint64_t cache_stride,
                            uint64_t exp_stride)
{
    const uint32_t r = blockIdx.y;
    if (row_idle(rows, r)) return;
    rope_kv_f8_body(qkv + (size_t)r * (H + 2 * KV) * hd, q_out + (size_t)r * H * hd, kq + r * cache_stride, vq + r * cache_stride, kexp + r * exp_stride,
                    vexp + r * exp_stride, fcos, fsin, rows + r, H, KV, hd, max_seq);
}

// ------------------------------------------------------------------------------------------
// Scores.  grid (nsplit, KV, B), 256 threads: attn_scores_bf with the K operand made from bytes
// ------------------------------------------------------------------------------------------
template <int HD>
__device__ __forceinline__ void
attn_scores_f8(const bf16_t* __restrict__ q, const uint8_t* __restrict__ kq, const int8_t* __restrict__ kexp, float* __restrict__ expv,
               float* __restrict__ psum, const step_state* st, uint32_t n_rep, uint32_t max_seq, float scale, uint32_t nsplit)
{
    __shared__ float wsum[4][16];
    const uint32_t S = (uint32_t)st->kv_len;
    const uint32_t split = blockIdx.x, kv = blockIdx.y;
    const uint32_t p_begin = split * PB;
    if (p_begin >= S) return;
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t col = lane & 15, c = lane >> 4;
    constexpr int KS = HD / 32;

    // B fragments: K[slot = pos][d = ks*32 + c*8 + j] as bytes, and the slot's exponent
    const uint32_t pos = p_begin + wave * 16 + col;
    const uint32_t lp = pos < S ? pos : S - 1;
    const size_t vec = (size_t)kv * max_seq + lp;
    const uint8_t* kbase = kq + vec * HD;
    uint2 kb[KS];
#pragma unroll
    for (int ks = 0; ks < KS; ks++) kb[ks] = *reinterpret_cast<const uint2*>(kbase + ks * 32 + c * 8);
    const int32_t e = kexp[vec];
    uint4 qa[KS];
#pragma unroll
    for (int ks = 0; ks < KS; ks++) {
        qa[ks] = make_uint4(0, 0, 0, 0);
        if (col < n_rep) qa[ks] = *reinterpret_cast<const uint4*>(q + (size_t)(kv * n_rep + col) * HD + ks * 32 + c * 8);
    }
    const float kscale = kv8_pow2(e);
    f32x4_t acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ks = 0; ks < KS; ks++)
        acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, qa[ks]), __builtin_bit_cast(bf16x8_t, kv8_deq8(kb[ks], kscale)), acc, 0,
                                                      0, 0);
    scores_finish<BF>(acc, expv, psum, nullptr, wsum, S, pos, kv, n_rep, max_seq, scale, nsplit, split);
}

__device__ __forceinline__ void
b_attn_scores_f8(const bf16_t* q, const uint8_t* kq, const int8_t* kexp, float* expv, float* psum, const step_state* st, uint32_t n_rep, uint32_t hd,
                 uint32_t max_seq, float scale, uint32_t nsplit, uint64_t cache_stride, uint64_t exp_stride)
{
    const uint32_t r = blockIdx.z, H = gridDim.y * n_rep;
    const bf16_t* qr = q + (size_t)r * H * hd;
    const uint8_t* kr = kq + r * cache_stride;
    const int8_t* xr = kexp + r * exp_stride;
    float* er = expv + (size_t)r * H * max_seq;
    float* pr = psum + (size_t)r * H * nsplit;
    if (hd == 128) attn_scores_f8<128>(qr, kr, xr, er, pr, st, n_rep, max_seq, scale, nsplit);
    else if (hd == 64) attn_scores_f8<64>(qr, kr, xr, er, pr, st, n_rep, max_seq, scale, nsplit);
}

extern "C" __global__ void __launch_bounds__(256)
mc_b_attn_scores_f8_bfloat(const bf16_t* q, const uint8_t* kq, const int8_t* kexp, float* expv, float* psum, const step_state* st, uint32_t n_rep,
                           uint32_t hd, uint32_t max_seq, float scale, uint32_t nsplit, uint64_t cache_stride, uint64_t exp_stride)
{
    b_attn_scores_f8(q, kq, kexp, expv, psum, st, n_rep, hd, max_seq, scale, nsplit, cache_stride, exp_stride);
}

extern "C" __global__ void __launch_bounds__(256)
mc_b_attn_scores_f8_rows_bfloat(const bf16_t* q, const uint8_t* kq, const int8_t* kexp, float* expv, float* psum, const step_state* rows,
                                uint32_t n_rep, uint32_t hd, uint32_t max_seq, float scale, uint32_t nsplit, uint64_t cache_stride, uint64_t exp_stride)
{
    if (row_idle(rows, blockIdx.z)) return;
    b_attn_scores_f8(q, kq, kexp, expv, psum, rows + blockIdx.z, n_rep, hd, max_seq, scale, nsplit, cache_stride, exp_stride);
}

// ------------------------------------------------------------------------------------------
// Softmax + P.V.  grid (hd / 16, KV, B), 1024 threads: attn_pv_bf_body over one range with the Vt operand made from bytes
// ------------------------------------------------------------------------------------------
__device__ __forceinline__ void
attn_pv_f8_body(const float* __restrict__ expv, const float* __restrict__ psum, const uint8_t* __restrict__ vq, const int8_t* __restrict__ vexp,
                bf16_t* __restrict__ out, const step_state* st, uint32_t n_rep, uint32_t hd, uint32_t max_seq, uint32_t nsplit)
{
    __shared__ float part[16 * 16 * 16]; // up to 16 waves
    __shared__ float inv_s[16];
    const uint32_t S = (uint32_t)st->kv_len;
    const uint32_t db = blockIdx.x, kv = blockIdx.y;
    const uint32_t nact = (S + PB - 1) / PB;
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
    const uint32_t col = lane & 15, c = lane >> 4;
    const float* erow = expv + (size_t)(kv * n_rep + col) * max_seq;
    const uint8_t* vrow = vq + ((size_t)kv * hd + db * 16 + col) * max_seq;
    const int8_t* xrow = vexp + (size_t)kv * max_seq;
    const uint32_t nk = (S + 31) / 32;

    f32x4_t acc = {0.f, 0.f, 0.f, 0.f};
    // four k-steps of this wave per round, all loads first; the first round is requested before the denominators are reduced
    uint2 vb[4], xb[4];
    float4 e0[4], e1[4];
    auto request = [&](uint32_t t0) {
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const uint32_t p0 = (t0 + nw * u) * 32 + c * 8;
            const uint32_t pl = p0 + 8 <= max_seq ? p0 : max_seq - 8;
            vb[u] = *reinterpret_cast<const uint2*>(vrow + pl);
            xb[u] = *reinterpret_cast<const uint2*>(xrow + pl);
            e0[u] = make_float4(0.f, 0.f, 0.f, 0.f);
            e1[u] = e0[u];
            if (col < n_rep && p0 < S && t0 + nw * u < nk) {
                e0[u] = *reinterpret_cast<const float4*>(erow + p0);
                e1[u] = *reinterpret_cast<const float4*>(erow + p0 + 4);
            }
        }
    };
    uint32_t t0 = wave;
    if (t0 < nk) request(t0);
    const float inv = softmax_inv(psum, inv_s, kv, n_rep, nsplit, nact);
    while (t0 < nk) {
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const uint32_t p0 = (t0 + nw * u) * 32 + c * 8;
            const float e[8] = {e0[u].x, e0[u].y, e0[u].z, e0[u].w, e1[u].x, e1[u].y, e1[u].z, e1[u].w};
            uint32_t w[4];
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const float pa = (p0 + 2 * j < S) ? e[2 * j] * inv : 0.0f;
                const float pb = (p0 + 2 * j + 1 < S) ? e[2 * j + 1] * inv : 0.0f;
                w[j] = pack_bf16x2(pa, pb); // softmax output rounded to bf16
            }
            // the slots [p0, p0 + 8) below kv_len keep their bytes and exponents, the others read as byte 0 with exponent 0: +0.0
            const uint32_t nv = p0 < S ? min(S - p0, 8u) : 0u;
            const uint32_t mlo = nv >= 4 ? 0xFFFFFFFFu : (1u << (8 * nv)) - 1u;
            const uint32_t mhi = nv >= 8 ? 0xFFFFFFFFu : (nv > 4 ? (1u << (8 * (nv - 4))) - 1u : 0u);
            const uint2 vbytes = make_uint2(vb[u].x & mlo, vb[u].y & mhi), xbytes = make_uint2(xb[u].x & mlo, xb[u].y & mhi);
            const uint4 pa4 = make_uint4(w[0], w[1], w[2], w[3]);
            acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, pa4), __builtin_bit_cast(bf16x8_t, kv8_deq8x8(vbytes, xbytes)), acc,
                                                          0, 0, 0);
        }
        t0 += 4 * nw;
        if (t0 < nk) request(t0);
    }
    pv_finish_store(acc, part, out, 2, kv, n_rep, hd, db, nullptr, 0, 0, 1);
}

extern "C" __global__ void __launch_bounds__(1024)
mc_b_attn_pv_f8_bfloat(const float* expv, const float* psum, const uint8_t* vq, const int8_t* vexp, bf16_t* out, const step_state* st, uint32_t n_rep,
                       uint32_t hd, uint32_t max_seq, uint32_t nsplit, uint64_t cache_stride, uint64_t exp_stride)
{
    const uint32_t r = blockIdx.z, H = gridDim.y * n_rep;
    attn_pv_f8_body(expv + (size_t)r * H * max_seq, psum + (size_t)r * H * nsplit, vq + r * cache_stride, vexp + r * exp_stride, out + (size_t)r * H * hd, st,
                    n_rep, hd, max_seq, nsplit);
}

// ... over row r's own kv_len; an idle row's attention output is zeros (what Wo then reads for it)
extern "C" __global__ void __launch_bounds__(1024)
mc_b_attn_pv_f8_rows_bfloat(const float* expv, const float* psum, const uint8_t* vq, const int8_t* vexp, bf16_t* out, const step_state* rows,
                            uint32_t n_rep, uint32_t hd, uint32_t max_seq, uint32_t nsplit, uint64_t cache_stride, uint64_t exp_stride)
{
    const uint32_t r = blockIdx.z, H = gridDim.y * n_rep;
    if (row_idle(rows, r)) {
        if (threadIdx.x < n_rep * 16)
            out[(size_t)r * H * hd + (size_t)(blockIdx.y * n_rep + threadIdx.x / 16) * hd + blockIdx.x * 16 + threadIdx.x % 16] = 0;
        return;
    }
    attn_pv_f8_body(expv + (size_t)r * H * max_seq, psum + (size_t)r * H * nsplit, vq + r * cache_stride, vexp + r * exp_stride, out + (size_t)r * H * hd,
                    rows + r, n_rep, hd, max_seq, nsplit);
}

// ------------------------------------------------------------------------------------------
// mc_kv_quant_f8: bfloat16 K [kv][src_seq][hd] and Vt [kv * hd][src_seq] of one layer, positions [0, n), into one row's fp8 planes (slot = position).
// grid (ceil(n / 64), KV), 256 threads: 64 slots of one kv head
// ------------------------------------------------------------------------------------------
template <int HD>
__device__ __forceinline__ void
kv_quant_f8_body(const bf16_t* __restrict__ k_src, const bf16_t* __restrict__ vt_src, uint32_t src_seq, uint8_t* __restrict__ kq, uint8_t* __restrict__ vq,
                 int8_t* __restrict__ kexp, int8_t* __restrict__ vexp, uint32_t n, uint32_t max_seq)
{
    __shared__ uint32_t pmax[4][64];
    const uint32_t kv = blockIdx.y, s0 = blockIdx.x * 64;
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    // ---- K: LPS lanes per slot, 8 elements a lane; a wave takes its 16 slots 64 / LPS at a time
    constexpr uint32_t LPS = HD / 8, SPW = 64 / LPS;
    const uint32_t sub = lane / LPS, piece = lane % LPS;
#pragma unroll
    for (uint32_t i = 0; i < 16 / SPW; i++) {
        const uint32_t slot = s0 + wave * 16 + i * SPW + sub;
        const bool live = slot < n;
        uint4 v = make_uint4(0, 0, 0, 0);
        if (live) v = *reinterpret_cast<const uint4*>(k_src + ((size_t)kv * src_seq + slot) * HD + piece * 8);
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
        uint32_t amax = 0;
#pragma unroll
        for (int j = 0; j < 4; j++) amax = max(amax, max(w[j] & 0x7FFFu, (w[j] >> 16) & 0x7FFFu));
#pragma unroll
        for (uint32_t off = LPS / 2; off >= 1; off >>= 1) amax = max(amax, (uint32_t)__shfl_xor((int)amax, (int)off, 64));
        const int32_t e = kv8_exponent(amax);
        const float inv = kv8_pow2(-e);
        uint32_t q[4];
#pragma unroll
        for (int j = 0; j < 4; j++) q[j] = kv8_quant2(__uint_as_float(w[j] << 16), __uint_as_float(w[j] & 0xFFFF0000u), inv);
        if (live) {
            const size_t vec = (size_t)kv * max_seq + slot;
            *reinterpret_cast<uint2*>(kq + vec * HD + piece * 8) = make_uint2(q[0] | (q[1] << 16), q[2] | (q[3] << 16));
            if (piece == 0) kexp[vec] = (int8_t)e;
        }
    }
    // ---- Vt: thread (slot = lane, wave) holds rows d = wave + 4 i of its slot
    const uint32_t slot = s0 + lane;
    const bool live = slot < n;
    bf16_t v[HD / 4];
    uint32_t amax = 0;
#pragma unroll
    for (int i = 0; i < HD / 4; i++) {
        v[i] = live ? vt_src[((size_t)kv * HD + wave + 4 * i) * src_seq + slot] : (bf16_t)0;
        amax = max(amax, kv8_abs(v[i]));
    }
    pmax[wave][lane] = amax;
    __syncthreads();
    amax = max(max(pmax[0][lane], pmax[1][lane]), max(pmax[2][lane], pmax[3][lane]));
    if (!live) return;
    const int32_t e = kv8_exponent(amax);
    const float inv = kv8_pow2(-e);
#pragma unroll
    for (int i = 0; i < HD / 4; i += 2) {
        const uint32_t q2 = kv8_quant2(bf2f(v[i]), bf2f(v[i + 1]), inv);
        vq[((size_t)kv * HD + wave + 4 * i) * max_seq + slot] = (uint8_t)q2;
        vq[((size_t)kv * HD + wave + 4 * (i + 1)) * max_seq + slot] = (uint8_t)(q2 >> 8);
    }
    if (wave == 0) vexp[(size_t)kv * max_seq + slot] = (int8_t)e;
}

extern "C" __global__ void __launch_bounds__(256)
mc_kv_quant_f8(const bf16_t* k_src, const bf16_t* vt_src, uint32_t src_seq, uint8_t* kq, uint8_t* vq, int8_t* kexp, int8_t* vexp, uint32_t n, uint32_t hd,
               uint32_t max_seq)
{
    if (hd == 128) kv_quant_f8_body<128>(k_src, vt_src, src_seq, kq, vq, kexp, vexp, n, max_seq);
    else if (hd == 64) kv_quant_f8_body<64>(k_src, vt_src, src_seq, kq, vq, kexp, vexp, n, max_seq);
}

// ------------------------------------------------------------------------------------------
// mc_kv_dequant_f8: the logical view mc_kv_export_bfloat writes -- out[p][kv][d] for p in [0, kv_len), the ring unrolled -- as deq values
// ------------------------------------------------------------------------------------------
extern "C" __global__ void
mc_kv_dequant_f8(const uint8_t* kq, const uint8_t* vq, const int8_t* kexp, const int8_t* vexp, bf16_t* k_out, bf16_t* v_out, const step_state* st,
                 uint32_t KV, uint32_t hd, uint32_t max_seq, uint32_t pre_len)
{
    const uint32_t n = (uint32_t)st->kv_len;
    const uint32_t post = max_seq - pre_len;
    const size_t total = (size_t)n * KV * hd;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const uint32_t d = i % hd, kv = (i / hd) % KV, p = i / ((size_t)hd * KV);
        const uint32_t slot = p < pre_len ? p : pre_len + (p - pre_len + (uint32_t)st->ring_base) % post;
        const size_t vec = (size_t)kv * max_seq + slot;
        k_out[i] = kv8_deq1(kq[vec * hd + d], kexp[vec]);
        v_out[i] = kv8_deq1(vq[((size_t)kv * hd + d) * max_seq + slot], vexp[vec]);
    }
}
