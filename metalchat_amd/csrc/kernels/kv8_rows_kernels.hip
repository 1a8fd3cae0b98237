// The packed passes on fp8 KV caches (mc_kv_packed_set, include/metalchat_hip.h Part 2p): the rope + cache write, the causal attention of a chunk
// over its own columns and the extend attention over the range table of packed_kernels.hip / extend_kernels.hip, on the byte and exponent planes of
// kv8_kernels.hip.  The contract is Part 2o's (tests/kv_fp8_rule.py): every kernel here computes bit for bit what its bfloat16 counterpart computes on
// planes that hold deq(quant(K)), deq(quant(V)), and writes quant of what that counterpart would have stored.  Only what feeds the MFMA operands
// differs; the S^T = K Q^T operand order, load_k's 4-key deal, the exp window, s = T(T(q.k) scale), p = T(e / sum), the order in which lane groups,
// waves and ranges are added and the osum reduction are the bfloat16 bodies', restated addition for addition where they cannot be called
// (px_tile::score and mc_px_reduce_* are called as they are).
//
// How the data moves:
//   K        lane (l15, lg) loads the 8 bytes d = 32 ks + 8 lg + [0, 8) of ITS key per k-step -- 8 where the bfloat16 body loads 16 -- and the key's
//            exponent byte once; a fragment stays bytes while it is in flight (one tile ahead, as there) and becomes the operand in front of its
//            MFMAs: four v_cvt_scalef32_pk_bf16_fp8 per k-step, whose result IS deq.  The key index is clamped to the last visible key: an unwritten
//            slot is never loaded.
//   V        lane (l15, lg) holds the slots c = 32 b + 8 lg + [0, 8) of Vt row 16 t + l15: 8 bytes per tile t.  The eight slots carry eight
//            exponents, the same eight for every tile and both heads of the block: ONE 8-byte load (the same address in the 16 lanes of a lane
//            group) and eight 2^e built once per block; a tile is then four v_cvt_pk_f32_fp8, eight exact multiplies and four v_cvt_pk_bf16_f32.
//            Bytes and exponents of the first tiles are requested before the block's scores.
//   masks    bytes AND exponents of the slots at and past the tile's visible keys, and of a load clamped at max_seq, are zeroed before the
//            conversion: such a slot may hold a NaN byte (0x7f, 0xff) or a stray exponent (-128 would make 2^e an infinity), and byte 0 under
//            exponent 0 is +0.0, which p = 0 meets.  The bfloat16 extend body masks element-wise for the same reason; the packed body relies on
//            finite slots there, which bytes cannot promise.
//   write    K unit: the hd / 8 lanes of a head hold 4 + 4 elements behind the rotation; amax is the integer maximum of their magnitude bits over
//            a shuffle tree of those lanes, a lane stores 4 + 4 bytes, lane 0 the exponent.  V tile (16 rows of one kv head): thread (i, g) holds 8
//            elements of row r0 + i, the hd / 8 partial maxima of a row lie in different waves and meet in LDS, every thread stores its 8 bytes --
//            the 16 threads of a g write 16 consecutive slots of one d -- and thread g = 0 the exponent.
// No private segment, no spills, vector stores only.  bfloat16 decoders, head_dim 64 and 128.
// The names are mc_pp8_* / mc_px8_* beside mc_pp_* / mc_px_*, not those names with an _f8 in them: tests/test_rows_tables_cpu.py pins the set of
// mc_pp_* and mc_px_* names of the code object.

template <uint32_t HD>
struct kv8_kfrag {
    uint2 b[HD / 32]; // the bytes d = 32 ks + 8 lg + [0, 8) of one key
    int32_t e;        // its exponent
};

template <uint32_t HD>
__device__ __forceinline__ void
kv8_load_k(const uint8_t* __restrict__ kbase, const int8_t* __restrict__ xbase, uint32_t keyc, uint32_t kg, kv8_kfrag<HD>& k)
{
#pragma unroll
    for (uint32_t d = 0; d < HD / 32; d++) k.b[d] = *reinterpret_cast<const uint2*>(kbase + (size_t)keyc * HD + d * 32 + kg);
    k.e = xbase[keyc];
}

// the bfloat16 MFMA operand of a key's fragment: deq
template <uint32_t HD>
__device__ __forceinline__ void
kv8_k_operand(const kv8_kfrag<HD>& k, uint4 (&kb)[HD / 32])
{
    const float s = kv8_pow2(k.e);
#pragma unroll
    for (uint32_t d = 0; d < HD / 32; d++) kb[d] = kv8_deq8(k.b[d], s);
}

// byte masks of the eight slots c .. c + 7 of which those below `lim` are visible (none where the load was clamped at max_seq)
__device__ __forceinline__ void
kv8_slot_masks(uint32_t c, uint32_t lim, uint32_t max_seq, uint32_t& mlo, uint32_t& mhi)
{
    const uint32_t nv = (c + 8 <= max_seq && c < lim) ? min(lim - c, 8u) : 0u;
    mlo = nv >= 4 ? 0xFFFFFFFFu : (1u << (8 * nv)) - 1u;
    mhi = nv >= 8 ? 0xFFFFFFFFu : (nv > 4 ? (1u << (8 * (nv - 4))) - 1u : 0u);
}

// 2^e of eight (masked) exponent bytes
__device__ __forceinline__ void
kv8_scales8(uint2 x, float (&s)[8])
{
#pragma unroll
    for (int i = 0; i < 4; i++) {
        s[i] = kv8_pow2((int32_t)(int8_t)(x.x >> (8 * i)));
        s[4 + i] = kv8_pow2((int32_t)(int8_t)(x.y >> (8 * i)));
    }
}

// 8 (masked) bytes of eight vectors with their scales as 8 bfloat16: the products are exact, deq is a bfloat16
__device__ __forceinline__ uint4
kv8_deq8s(uint2 b, const float (&s)[8])
{
    const kv8_f32x2 f0 = __builtin_amdgcn_cvt_pk_f32_fp8((int)b.x, false), f1 = __builtin_amdgcn_cvt_pk_f32_fp8((int)b.x, true);
    const kv8_f32x2 f2 = __builtin_amdgcn_cvt_pk_f32_fp8((int)b.y, false), f3 = __builtin_amdgcn_cvt_pk_f32_fp8((int)b.y, true);
    return make_uint4(pack_bf16x2(f0.x * s[0], f0.y * s[1]), pack_bf16x2(f1.x * s[2], f1.y * s[3]), pack_bf16x2(f2.x * s[4], f2.y * s[5]),
                      pack_bf16x2(f3.x * s[6], f3.y * s[7]));
}

// ------------------------------------------------------------------------------------------
// Rope + cache write over the segment table: pf_rope_cache_v4_body's grid, units and values (no q / k norm: a batch's decoder has none), q rows as
// bfloat16; grid and block as mc_pp_rope_cache{,_parts}_bfloat
// ------------------------------------------------------------------------------------------
// TREE (kv8_tree_kernels.hip, mc_tree_verify on an fp8 batch): packed row r is node i of its segment's tree -- written to slot pos + i, rotated with rope
// row pos + depth(i) (tree_kernels.hip tv_rows::at); the one difference
template <bool SPLITS, bool TREE = false>
__device__ __forceinline__ void
pp8_rope_cache_body(const void* rows, uint32_t splits, uint32_t M, bf16_t* q_out, const pp_seg* segs, uint32_t nseg, uint8_t* kq, uint8_t* vq, int8_t* kexp,
                    int8_t* vexp, uint64_t cache_stride, uint64_t exp_stride, const float* fcos, const float* fsin, uint32_t H, uint32_t KV, uint32_t hd,
                    uint32_t max_seq, const tv_node* nodes = nullptr)
{
    __shared__ uint32_t pmax[16][16]; // [g][i]: a V tile's partial maxima
    const uint32_t half = hd / 2, lpu = hd / 8, nb = H + KV, NQ = (H + 2 * KV) * hd, per = blockDim.x / lpu;
    const uint32_t gq = (nb * M + per - 1) / per; // workgroups of q / k units; behind them KV * ceil(M / 16) of v tiles
    auto load8 = [&](size_t src, float (&x)[8]) {
        if (SPLITS) {
            pf_part_sum8(static_cast<const float*>(rows), splits, (size_t)M * NQ, src, x);
#pragma unroll
            for (int i = 0; i < 8; i++) x[i] = bf2f(f2bf(x[i]));
        } else {
            const uint4 v = *reinterpret_cast<const uint4*>(static_cast<const bf16_t*>(rows) + src);
            const uint32_t d[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int i = 0; i < 8; i++) x[i] = __uint_as_float((i & 1) ? (d[i >> 1] & 0xFFFF0000u) : (d[i >> 1] << 16));
        }
    };
    // pp_rows::at: packed row r -> (batch row, slot = rope row); TREE: tv_rows::at, rope row = pos + depth
    auto at = [&](uint32_t r, uint32_t& row, uint32_t& slot, uint32_t& rope_row) {
        uint32_t s = 0;
        while (s + 1 < nseg && r >= (uint32_t)segs[s + 1].off) s++;
        const pp_seg g = segs[s];
        row = (uint32_t)g.row;
        slot = (uint32_t)g.pos + (r - (uint32_t)g.off);
        rope_row = TREE ? (uint32_t)g.pos + (uint32_t)nodes[r].depth : slot;
    };
    auto mag = [](float v) { return __float_as_uint(v) >> 16 & 0x7FFFu; }; // (v is a bfloat16 value)
    if (blockIdx.x >= gq) { // (uniform)
        // a V tile: thread (i, g) holds elements 8 g .. 8 g + 7 of row r0 + i; rows past M and g >= hd / 8 hold nothing but reach the barrier
        const uint32_t vb = blockIdx.x - gq, kv = vb % KV, i = threadIdx.x & 15u, g = threadIdx.x >> 4, r = (vb / KV) * 16 + i;
        const bool live = r < M && g < lpu;
        float x[8];
        uint32_t amax = 0;
        if (live) {
            load8((size_t)r * NQ + (size_t)(nb + kv) * hd + 8 * g, x);
#pragma unroll
            for (int j = 0; j < 8; j++) amax = max(amax, mag(x[j]));
        }
        pmax[g][i] = amax;
        __syncthreads();
        if (!live) return;
        for (uint32_t gg = 0; gg < lpu; gg++) amax = max(amax, pmax[gg][i]);
        uint32_t row, slot, rope_row;
        at(r, row, slot, rope_row);
        const int32_t e = kv8_exponent(amax);
        const float inv = kv8_pow2(-e);
        uint8_t* dst = vq + row * cache_stride + ((size_t)kv * hd + 8 * g) * max_seq + slot;
#pragma unroll
        for (int j = 0; j < 8; j += 2) {
            const uint32_t q2 = kv8_quant2(x[j], x[j + 1], inv);
            dst[(size_t)j * max_seq] = (uint8_t)q2;
            dst[(size_t)(j + 1) * max_seq] = (uint8_t)(q2 >> 8);
        }
        if (g == 0) vexp[row * exp_stride + (size_t)kv * max_seq + slot] = (int8_t)e;
        return;
    }
    const uint32_t unit = blockIdx.x * per + threadIdx.x / lpu, l = threadIdx.x % lpu;
    if (unit >= nb * M) return;
    const uint32_t b = unit % nb, r = unit / nb;
    uint32_t row, slot, rope_row;
    at(r, row, slot, rope_row);
    float x[8];
    load8((size_t)r * NQ + (size_t)b * hd + 8 * l, x);
    const size_t tr = (size_t)rope_row * half + 4 * l;
    const float4 c4 = *reinterpret_cast<const float4*>(fcos + tr), s4 = *reinterpret_cast<const float4*>(fsin + tr);
    const float c[4] = {c4.x, c4.y, c4.z, c4.w}, s[4] = {s4.x, s4.y, s4.z, s4.w};
    float o1[4], o2[4];
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const float x1 = x[2 * i], x2 = x[2 * i + 1];
        o1[i] = BF::rt(c[i] * x1 - s[i] * x2);
        o2[i] = BF::rt(s[i] * x1 + c[i] * x2);
    }
    if (b < H) {
        bf16_t* dst = q_out + ((size_t)r * H + b) * hd + 4 * l;
        *reinterpret_cast<uint2*>(dst) = make_uint2(pack_bf16x2(o1[0], o1[1]), pack_bf16x2(o1[2], o1[3]));
        *reinterpret_cast<uint2*>(dst + half) = make_uint2(pack_bf16x2(o2[0], o2[1]), pack_bf16x2(o2[2], o2[3]));
        return;
    }
    // a K unit: the head's hd / 8 lanes are neighbours in one wave, all of them here
    uint32_t amax = 0;
#pragma unroll
    for (int i = 0; i < 4; i++) amax = max(amax, max(mag(o1[i]), mag(o2[i])));
    for (uint32_t off = lpu / 2; off >= 1; off >>= 1) amax = max(amax, (uint32_t)__shfl_xor((int)amax, (int)off, 64));
    const int32_t e = kv8_exponent(amax);
    const float inv = kv8_pow2(-e);
    const size_t vec = (size_t)(b - H) * max_seq + slot;
    uint8_t* dst = kq + row * cache_stride + vec * hd + 4 * l;
    *reinterpret_cast<uint32_t*>(dst) = kv8_quant2(o1[0], o1[1], inv) | (kv8_quant2(o1[2], o1[3], inv) << 16);
    *reinterpret_cast<uint32_t*>(dst + half) = kv8_quant2(o2[0], o2[1], inv) | (kv8_quant2(o2[2], o2[3], inv) << 16);
    if (l == 0) kexp[row * exp_stride + vec] = (int8_t)e;
}

// cache_stride: bytes between the rows' K (and V) byte planes of one layer, exp_stride: between their exponent planes
extern "C" __global__ void __launch_bounds__(256)
mc_pp8_rope_cache_bfloat(const bf16_t* qkv, uint32_t M, bf16_t* q_out, const pp_seg* segs, uint32_t nseg, uint8_t* kq, uint8_t* vq, int8_t* kexp,
                           int8_t* vexp, uint64_t cache_stride, uint64_t exp_stride, const float* fcos, const float* fsin, uint32_t H, uint32_t KV,
                           uint32_t hd, uint32_t max_seq)
{
    pp8_rope_cache_body<false>(qkv, 1, M, q_out, segs, nseg, kq, vq, kexp, vexp, cache_stride, exp_stride, fcos, fsin, H, KV, hd, max_seq);
}
extern "C" __global__ void __launch_bounds__(256)
mc_pp8_rope_cache_parts_bfloat(const float* part, uint32_t splits, uint32_t M, bf16_t* q_out, const pp_seg* segs, uint32_t nseg, uint8_t* kq,
                                 uint8_t* vq, int8_t* kexp, int8_t* vexp, uint64_t cache_stride, uint64_t exp_stride, const float* fcos,
                                 const float* fsin, uint32_t H, uint32_t KV, uint32_t hd, uint32_t max_seq)
{
    pp8_rope_cache_body<true>(part, splits, M, q_out, segs, nseg, kq, vq, kexp, vexp, cache_stride, exp_stride, fcos, fsin, H, KV, hd, max_seq);
}

// ------------------------------------------------------------------------------------------
// Causal attention of a chunk over its own columns, one query head per workgroup: pf_attn_body<HD, 1> (S = Q K^T, P through wave-private LDS, the
// inline exponential) at window 0, K and Vt operands made from bytes.  kq / vq / kexp / vexp: the row's planes
// IN LOCKSTEP with prefill_kernels.hip, by hand -- a change there to any of these must be made here too (tests/test_kv_fp8_rows_kernels_gpu.py
// holds the two to the same bits):
//   this body (one head)    pf_attn_body: b_lo / b_hi, the Q fragments, score_tile's operand order, rounding and mask, rsum and its shuffles over
//                           l15, wsum / inv_sum, p = T(e inv) through pl with its fences, the MFMA order over t, the osum reduction
//   pp8_attn_kt_body        pf_attn_kt_body: b_lo / b_hi, load_k's key deal, score_tile (`full` included), rsum's tree and its shuffles over lg,
//                           wsum / inv_sum, pa's packing order, the MFMA order over t and j, the osum reduction
//   px8_sums_body, _pv_body extend_kernels.hip px_sums_body / px_pv_body: the same list; px_tile::score itself is called
// What is NOT mirrored, on purpose: the loads (bytes, exponents, all V tiles before the scores) and the V masks (kv8_slot_masks).
// kv8_tree_kernels.hip instantiates pp8_rope_cache_body, px8_sums_body and px8_pv_body with TREE = true (mc_tv8_*): nothing is restated there, and the
// template parameter leaves the code of the kernels of this file as it was.
// ------------------------------------------------------------------------------------------
template <uint32_t HD>
__device__ __forceinline__ void
pp8_attn_body(const bf16_t* Q, const uint8_t* kq, const uint8_t* vq, const int8_t* kexp, const int8_t* vexp, bf16_t* out, uint32_t M, uint32_t S,
              uint32_t H, uint32_t n_rep, uint32_t max_seq, float scale, uint32_t r0)
{
    using T = BF;
    constexpr uint32_t DT = HD / 16, DK = HD / 32;
    __shared__ float wsum[4][16];
    __shared__ float inv_sum[16];
    __shared__ __attribute__((aligned(16))) bf16_t pl[4][16 * 40]; // 16 rows x 32 keys, rows padded to 80 bytes
    __shared__ float osum[4][16][HD + 1];
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t l15 = lane & 15, lg = lane >> 4, kg = lg * 8;
    const uint32_t h0 = blockIdx.y, kv = h0 / n_rep;
    const uint8_t* kbase = kq + (size_t)kv * max_seq * HD;
    const uint8_t* vbase = vq + (size_t)kv * HD * max_seq;
    const int8_t* kx = kexp + (size_t)kv * max_seq;
    const int8_t* vx = vexp + (size_t)kv * max_seq;
    const uint32_t sq = S - M, rlast = min(r0 + 15, M - 1);
    const uint32_t b_lo = sq / 32, b_hi = (sq + rlast) / 32;
    uint4 qa[DK];
    {
        const uint32_t qr = min(r0 + l15, M - 1);
#pragma unroll
        for (uint32_t d = 0; d < DK; d++) qa[d] = *reinterpret_cast<const uint4*>(Q + ((size_t)qr * H + h0) * HD + d * 32 + kg);
    }
    // masked, scaled score tile of the 16 keys from key0 on -> sv[i] for row lg * 4 + i, key key0 + l15
    auto score_tile = [&](uint32_t key0, float (&sv)[4]) {
        const uint32_t key = key0 + l15;
        kv8_kfrag<HD> k;
        kv8_load_k<HD>(kbase, kx, key < S ? key : S - 1, kg, k);
        uint4 kb[DK];
        kv8_k_operand<HD>(k, kb);
        pf_f32x4 acc = {0, 0, 0, 0};
#pragma unroll
        for (uint32_t d = 0; d < DK; d++)
            acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(pf_bf16x8, qa[d]), __builtin_bit_cast(pf_bf16x8, kb[d]), acc, 0, 0, 0);
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const uint32_t r = r0 + lg * 4 + i;
            const float sc = T::rt(T::rt(acc[i]) * scale);
            sv[i] = (r < M && key < S && pf_visible(r, key, S, M, 0u)) ? sc : -INFINITY;
        }
    };
    // ---- pass 1: exp row sums
    float rsum[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    for (uint32_t b = b_lo + wave; b <= b_hi; b += 4) {
        float sv[4];
        score_tile(b * 32, sv);
#pragma unroll
        for (int i = 0; i < 4; i++) rsum[i] += exp_precise(sv[i]);
        score_tile(b * 32 + 16, sv);
#pragma unroll
        for (int i = 0; i < 4; i++) rsum[i] += exp_precise(sv[i]);
    }
#pragma unroll
    for (int i = 0; i < 4; i++) {
        float e = rsum[i];
        e += __shfl_xor(e, 1, 64);
        e += __shfl_xor(e, 2, 64);
        e += __shfl_xor(e, 4, 64);
        e += __shfl_xor(e, 8, 64);
        if (l15 == 0) wsum[wave][lg * 4 + i] = e;
    }
    __syncthreads();
    if (threadIdx.x < 16) inv_sum[threadIdx.x] = 1.0f / ((wsum[0][threadIdx.x] + wsum[1][threadIdx.x]) + (wsum[2][threadIdx.x] + wsum[3][threadIdx.x]));
    __syncthreads();
    float inv[4];
#pragma unroll
    for (int i = 0; i < 4; i++) inv[i] = inv_sum[lg * 4 + i];
    // ---- pass 2: probabilities (T) x V
    pf_f32x4 oacc[DT];
#pragma unroll
    for (uint32_t t = 0; t < DT; t++) oacc[t] = pf_f32x4{0, 0, 0, 0};
    for (uint32_t b = b_lo + wave; b <= b_hi; b += 4) {
        // the block's V bytes and exponents, requested before its scores
        const uint32_t c = b * 32 + kg, cc = c + 8 <= max_seq ? c : max_seq - 8;
        const uint8_t* vp = vbase + (size_t)l15 * max_seq + cc;
        uint2 vbs[DT];
#pragma unroll
        for (uint32_t t = 0; t < DT; t++) vbs[t] = *reinterpret_cast<const uint2*>(vp + (size_t)t * 16 * max_seq);
        const uint2 xb = *reinterpret_cast<const uint2*>(vx + cc);
#pragma unroll
        for (uint32_t half = 0; half < 2; half++) {
            float sv[4];
            score_tile(b * 32 + half * 16, sv);
#pragma unroll
            for (int i = 0; i < 4; i++) {
                const float p = T::rt(exp_precise(sv[i]) * inv[i]); // (masked: exp(-inf) = 0, T(0 * inv) = 0)
                pl[wave][(lg * 4 + i) * 40 + half * 16 + l15] = T::st(p);
            }
        }
        // (the tile is private to this wave: pf_attn_body's wavefront fences)
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        const uint4 pa = *reinterpret_cast<const uint4*>(&pl[wave][l15 * 40 + kg]);
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        uint32_t mlo, mhi;
        kv8_slot_masks(c, S, max_seq, mlo, mhi);
        float vs[8];
        kv8_scales8(make_uint2(xb.x & mlo, xb.y & mhi), vs);
#pragma unroll
        for (uint32_t t = 0; t < DT; t++) {
            const uint4 vb = kv8_deq8s(make_uint2(vbs[t].x & mlo, vbs[t].y & mhi), vs);
            oacc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(pf_bf16x8, pa), __builtin_bit_cast(pf_bf16x8, vb), oacc[t], 0, 0, 0);
        }
    }
#pragma unroll
    for (uint32_t t = 0; t < DT; t++)
#pragma unroll
        for (int i = 0; i < 4; i++) osum[wave][lg * 4 + i][t * 16 + l15] = oacc[t][i];
    __syncthreads();
    for (uint32_t e = threadIdx.x; e < 16 * HD; e += blockDim.x) {
        const uint32_t rr = e / HD, d = e % HD, r = r0 + rr;
        if (r < M) out[((size_t)r * H + h0) * HD + d] = T::st((osum[0][rr][d] + osum[1][rr][d]) + (osum[2][rr][d] + osum[3][rr][d]));
    }
}

// ------------------------------------------------------------------------------------------
// ... two query heads of a kv head per workgroup: pf_attn_kt_body<HD, 2> (S^T = K Q^T, P in registers, the exp window) at window 0
// ------------------------------------------------------------------------------------------
template <uint32_t HD, int NH>
__device__ __forceinline__ void
pp8_attn_kt_body(const bf16_t* Q, const uint8_t* kq, const uint8_t* vq, const int8_t* kexp, const int8_t* vexp, bf16_t* out, uint32_t M, uint32_t S,
                 uint32_t H, uint32_t n_rep, uint32_t max_seq, float scale, const float* etab, uint32_t r0)
{
    using T = BF;
    constexpr uint32_t DT = HD / 16, DK = HD / 32;
    __shared__ float wsum[NH][4][16];
    __shared__ float inv_sum[NH][16];
    __shared__ __attribute__((aligned(16))) float ewin[2 * pf_exp_window::N];
    const pf_exp_window ew{ewin};
    ew.fill(etab);
    __shared__ float osum[4][16][HD + 1];
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t l15 = lane & 15, lg = lane >> 4, kg = lg * 8;
    const uint32_t h0 = blockIdx.y * NH, kv = h0 / n_rep;
    const uint8_t* kbase = kq + (size_t)kv * max_seq * HD;
    const uint8_t* vbase = vq + (size_t)kv * HD * max_seq;
    const int8_t* kx = kexp + (size_t)kv * max_seq;
    const int8_t* vx = vexp + (size_t)kv * max_seq;
    const uint32_t sq = S - M, rlast = min(r0 + 15, M - 1);
    const uint32_t b_lo = sq / 32, b_hi = (sq + rlast) / 32;
    const uint32_t r = r0 + l15; // this lane's row
    uint4 qa[NH][DK];
    {
        const uint32_t qr = min(r, M - 1);
#pragma unroll
        for (int j = 0; j < NH; j++)
#pragma unroll
            for (uint32_t d = 0; d < DK; d++) qa[j][d] = *reinterpret_cast<const uint4*>(Q + ((size_t)qr * H + h0 + j) * HD + d * 32 + kg);
    }
    // tile h of a 32-key block holds keys blk + 8 g + 4 h + (0..3) as its rows m = 4 g + (0..3) (pf_attn_kt_body load_k)
    auto load_k = [&](uint32_t blk, uint32_t h, kv8_kfrag<HD>& k) {
        const uint32_t key = blk + 8 * (l15 >> 2) + 4 * h + (l15 & 3);
        kv8_load_k<HD>(kbase, kx, key < S ? key : S - 1, kg, k);
    };
    // sv[j][i] = masked, scaled score of (row r, key blk + 8 lg + 4 h + i) for head j
    auto score_tile = [&](uint32_t blk, uint32_t h, const kv8_kfrag<HD>& k, float (&sv)[NH][4]) {
        const bool full = r0 + 15 < M && blk + 31 < S && blk >= sq && blk + 31 - sq <= r0;
        uint4 kb[DK];
        kv8_k_operand<HD>(k, kb);
#pragma unroll
        for (int j = 0; j < NH; j++) {
            pf_f32x4 acc = {0, 0, 0, 0};
#pragma unroll
            for (uint32_t d = 0; d < DK; d++)
                acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(pf_bf16x8, kb[d]), __builtin_bit_cast(pf_bf16x8, qa[j][d]), acc, 0, 0, 0);
#pragma unroll
            for (int i = 0; i < 4; i++) sv[j][i] = T::rt(T::rt(acc[i]) * scale);
        }
        if (!full) {
#pragma unroll
            for (int i = 0; i < 4; i++) {
                const uint32_t key = blk + lg * 8 + h * 4 + i;
                const bool vis = bool(int(r < M) & int(key < S) & int(pf_visible(r, key, S, M, 0u)));
#pragma unroll
                for (int j = 0; j < NH; j++) sv[j][i] = vis ? sv[j][i] : -INFINITY;
            }
        }
    };
    // ---- pass 1: exp row sums (one row per lane: its four keys of every tile, then the four lane groups, then the four waves)
    float rsum[NH];
#pragma unroll
    for (int j = 0; j < NH; j++) rsum[j] = 0.0f;
    kv8_kfrag<HD> k0, k1;
    load_k((b_lo + wave) * 32, 0, k0);
    __syncthreads(); // the exp window is filled
    for (uint32_t b = b_lo + wave; b <= b_hi; b += 4) {
        float sv[NH][4];
        load_k(b * 32, 1, k1);
        score_tile(b * 32, 0, k0, sv);
#pragma unroll
        for (int j = 0; j < NH; j++) rsum[j] += (ew(sv[j][0]) + ew(sv[j][1])) + (ew(sv[j][2]) + ew(sv[j][3]));
        load_k((b + 4) * 32, 0, k0); // (past the range: clamped to the last key, never used)
        score_tile(b * 32, 1, k1, sv);
#pragma unroll
        for (int j = 0; j < NH; j++) rsum[j] += (ew(sv[j][0]) + ew(sv[j][1])) + (ew(sv[j][2]) + ew(sv[j][3]));
    }
#pragma unroll
    for (int j = 0; j < NH; j++) {
        float e = rsum[j];
        e += __shfl_xor(e, 16, 64);
        e += __shfl_xor(e, 32, 64);
        if (lg == 0) wsum[j][wave][l15] = e;
    }
    __syncthreads();
    if (threadIdx.x < 16 * NH) {
        const uint32_t j = threadIdx.x / 16, rr = threadIdx.x % 16;
        inv_sum[j][rr] = 1.0f / ((wsum[j][0][rr] + wsum[j][1][rr]) + (wsum[j][2][rr] + wsum[j][3][rr]));
    }
    __syncthreads();
    float inv[NH];
#pragma unroll
    for (int j = 0; j < NH; j++) inv[j] = inv_sum[j][l15];
    // ---- pass 2: probabilities (T) x V
    pf_f32x4 oacc[NH][DT];
#pragma unroll
    for (int j = 0; j < NH; j++)
#pragma unroll
        for (uint32_t t = 0; t < DT; t++) oacc[j][t] = pf_f32x4{0, 0, 0, 0};
    load_k((b_lo + wave) * 32, 0, k0);
    for (uint32_t b = b_lo + wave; b <= b_hi; b += 4) {
        // the block's V bytes (every tile: 8 bytes each) and its eight exponents, requested before the scores
        const uint32_t c = b * 32 + kg, cc = c + 8 <= max_seq ? c : max_seq - 8;
        const uint8_t* vp = vbase + (size_t)l15 * max_seq + cc;
        uint2 vbs[DT];
#pragma unroll
        for (uint32_t t = 0; t < DT; t++) vbs[t] = *reinterpret_cast<const uint2*>(vp + (size_t)t * 16 * max_seq);
        const uint2 xb = *reinterpret_cast<const uint2*>(vx + cc);
        uint4 pa[NH];
        {
            float sv[NH][4];
            load_k(b * 32, 1, k1);
            score_tile(b * 32, 0, k0, sv);
#pragma unroll
            for (int j = 0; j < NH; j++) {
                pa[j].x = pack_bf16x2(T::rt(ew(sv[j][0]) * inv[j]), T::rt(ew(sv[j][1]) * inv[j]));
                pa[j].y = pack_bf16x2(T::rt(ew(sv[j][2]) * inv[j]), T::rt(ew(sv[j][3]) * inv[j]));
            }
            load_k((b + 4) * 32, 0, k0); // (past the range: clamped to the last key, never used)
            score_tile(b * 32, 1, k1, sv);
#pragma unroll
            for (int j = 0; j < NH; j++) {
                pa[j].z = pack_bf16x2(T::rt(ew(sv[j][0]) * inv[j]), T::rt(ew(sv[j][1]) * inv[j]));
                pa[j].w = pack_bf16x2(T::rt(ew(sv[j][2]) * inv[j]), T::rt(ew(sv[j][3]) * inv[j]));
            }
        }
        uint32_t mlo, mhi;
        kv8_slot_masks(c, S, max_seq, mlo, mhi);
        float vs[8];
        kv8_scales8(make_uint2(xb.x & mlo, xb.y & mhi), vs);
#pragma unroll
        for (uint32_t t = 0; t < DT; t++) {
            const uint4 vb = kv8_deq8s(make_uint2(vbs[t].x & mlo, vbs[t].y & mhi), vs);
#pragma unroll
            for (int j = 0; j < NH; j++)
                oacc[j][t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(pf_bf16x8, pa[j]), __builtin_bit_cast(pf_bf16x8, vb), oacc[j][t], 0, 0, 0);
        }
    }
#pragma unroll
    for (int j = 0; j < NH; j++) {
        if (j) __syncthreads();
#pragma unroll
        for (uint32_t t = 0; t < DT; t++)
#pragma unroll
            for (int i = 0; i < 4; i++) osum[wave][lg * 4 + i][t * 16 + l15] = oacc[j][t][i];
        __syncthreads();
        for (uint32_t e = threadIdx.x; e < 16 * HD; e += blockDim.x) {
            const uint32_t rr = e / HD, d = e % HD, ro = r0 + rr;
            if (ro < M) out[((size_t)ro * H + h0 + j) * HD + d] = T::st((osum[0][rr][d] + osum[1][rr][d]) + (osum[2][rr][d] + osum[3][rr][d]));
        }
    }
}

// grid (tiles, H / NH), 256 threads: the tile table and arguments of mc_pp_attn{,2}_bfloat_hd*, the four planes and two strides in place of kc / vt
#define MC_PP_ATTN_F8(HD)                                                                                                                             \
    extern "C" __global__ void __launch_bounds__(256)                                                                                                 \
    mc_pp8_attn_bfloat_hd##HD(const bf16_t* Q, const pp_seg* segs, const pp_tile* tiles, const uint8_t* kq, const uint8_t* vq, const int8_t* kexp,  \
                                const int8_t* vexp, uint64_t cache_stride, uint64_t exp_stride, bf16_t* out, uint32_t H, uint32_t n_rep,              \
                                uint32_t max_seq, float scale, const float* etab)                                                                     \
    {                                                                                                                                                 \
        const pp_tile t = tiles[blockIdx.x];                                                                                                          \
        const pp_seg g = segs[t.seg];                                                                                                                 \
        const size_t q0 = (size_t)g.off * H * HD;                                                                                                     \
        pp8_attn_body<HD>(Q + q0, kq + (size_t)g.row * cache_stride, vq + (size_t)g.row * cache_stride, kexp + (size_t)g.row * exp_stride,            \
                          vexp + (size_t)g.row * exp_stride, out + q0, (uint32_t)g.len, (uint32_t)(g.pos + g.len), H, n_rep, max_seq, scale,          \
                          (uint32_t)t.r0);                                                                                                            \
    }                                                                                                                                                 \
    extern "C" __global__ void __launch_bounds__(256)                                                                                                 \
    mc_pp8_attn2_bfloat_hd##HD(const bf16_t* Q, const pp_seg* segs, const pp_tile* tiles, const uint8_t* kq, const uint8_t* vq, const int8_t* kexp, \
                                 const int8_t* vexp, uint64_t cache_stride, uint64_t exp_stride, bf16_t* out, uint32_t H, uint32_t n_rep,             \
                                 uint32_t max_seq, float scale, const float* etab)                                                                    \
    {                                                                                                                                                 \
        const pp_tile t = tiles[blockIdx.x];                                                                                                          \
        const pp_seg g = segs[t.seg];                                                                                                                 \
        const size_t q0 = (size_t)g.off * H * HD;                                                                                                     \
        pp8_attn_kt_body<HD, 2>(Q + q0, kq + (size_t)g.row * cache_stride, vq + (size_t)g.row * cache_stride, kexp + (size_t)g.row * exp_stride,      \
                                vexp + (size_t)g.row * exp_stride, out + q0, (uint32_t)g.len, (uint32_t)(g.pos + g.len), H, n_rep, max_seq, scale,    \
                                etab, (uint32_t)t.r0);                                                                                                \
    }
MC_PP_ATTN_F8(64)
MC_PP_ATTN_F8(128)

// ------------------------------------------------------------------------------------------
// The extend attention over the range table: px_sums_body / px_pv_body with the operands made from bytes.  The rows, the mask, the Q fragments and
// the scores are px_tile's own (its kbase is not used); mc_px_reduce_* follows unchanged
// ------------------------------------------------------------------------------------------
// TREE: px_tile's tree select over the node table (kv8_tree_kernels.hip) -- the one difference, as in extend_kernels.hip
template <uint32_t HD, int NH, bool TREE = false>
struct px8_tile {
    px_tile<HD, NH, TREE> t;
    const uint8_t* kbase;
    const int8_t* kx;
    __device__ __forceinline__ void
    load_k(uint32_t blk, uint32_t h, kv8_kfrag<HD>& k) const
    {
        const uint32_t key = blk + 8 * (t.l15 >> 2) + 4 * h + (t.l15 & 3);
        kv8_load_k<HD>(kbase, kx, key < t.S ? key : t.S - 1, t.kg, k);
    }
    __device__ __forceinline__ void
    score(uint32_t blk, uint32_t h, const kv8_kfrag<HD>& k, float (&sv)[NH][4]) const
    {
        uint4 kb[HD / 32];
        kv8_k_operand<HD>(k, kb);
        t.score(blk, h, kb, sv);
    }
};

template <uint32_t HD, int NH, bool TREE = false>
__device__ __forceinline__ px8_tile<HD, NH, TREE>
px8_tile_of(const bf16_t* Q, const pp_seg& g, const px_range& e, const uint8_t* kq, const int8_t* kexp, uint64_t cache_stride, uint64_t exp_stride,
            uint32_t H, uint32_t n_rep, uint32_t max_seq, float scale, uint32_t h0, const tv_node* nodes = nullptr)
{
    px8_tile<HD, NH, TREE> t;
    t.t = px_tile_of<HD, NH, TREE>(Q, g, e, reinterpret_cast<const bf16_t*>(kq), 0, H, n_rep, max_seq, scale, h0, nodes);
    t.kbase = kq + (size_t)g.row * cache_stride + (size_t)(h0 / n_rep) * max_seq * HD;
    t.kx = kexp + (size_t)g.row * exp_stride + (size_t)(h0 / n_rep) * max_seq;
    return t;
}

// grid (H / NH, ranges of the launch), 256 threads
template <uint32_t HD, int NH, bool TREE = false>
__device__ __forceinline__ void
px8_sums_body(const bf16_t* Q, const pp_seg* segs, const px_range* tab, uint32_t ebase, const uint8_t* kq, const int8_t* kexp, uint64_t cache_stride,
              uint64_t exp_stride, float* sums, uint32_t H, uint32_t n_rep, uint32_t max_seq, float scale, const float* etab,
              const tv_node* nodes = nullptr)
{
    __shared__ float wsum[NH][4][16];
    __shared__ __attribute__((aligned(16))) float ewin[2 * pf_exp_window::N];
    const pf_exp_window ew{ewin};
    ew.fill(etab);
    const px_range e = tab[ebase + blockIdx.y];
    const pp_seg g = segs[e.seg];
    const uint32_t wave = threadIdx.x >> 6, h0 = blockIdx.x * NH;
    const px8_tile<HD, NH, TREE> t = px8_tile_of<HD, NH, TREE>(Q, g, e, kq, kexp, cache_stride, exp_stride, H, n_rep, max_seq, scale, h0, nodes);
    const uint32_t b_lo = (uint32_t)e.k_lo / 32, b_end = ((uint32_t)e.k_hi + 31) / 32;
    float rsum[NH];
#pragma unroll
    for (int j = 0; j < NH; j++) rsum[j] = 0.0f;
    kv8_kfrag<HD> k0, k1;
    t.load_k((b_lo + wave) * 32, 0, k0);
    __syncthreads(); // the exp window is filled
    for (uint32_t b = b_lo + wave; b < b_end; b += 4) {
        float sv[NH][4];
        t.load_k(b * 32, 1, k1);
        t.score(b * 32, 0, k0, sv);
#pragma unroll
        for (int j = 0; j < NH; j++) rsum[j] += (ew(sv[j][0]) + ew(sv[j][1])) + (ew(sv[j][2]) + ew(sv[j][3]));
        t.load_k((b + 4) * 32, 0, k0); // (past the range: clamped to the tile's last key, never used)
        t.score(b * 32, 1, k1, sv);
#pragma unroll
        for (int j = 0; j < NH; j++) rsum[j] += (ew(sv[j][0]) + ew(sv[j][1])) + (ew(sv[j][2]) + ew(sv[j][3]));
    }
#pragma unroll
    for (int j = 0; j < NH; j++) {
        float s = rsum[j];
        s += __shfl_xor(s, 16, 64);
        s += __shfl_xor(s, 32, 64);
        if (t.t.lg == 0) wsum[j][wave][t.t.l15] = s;
    }
    __syncthreads();
    if (threadIdx.x < 16 * NH) {
        const uint32_t j = threadIdx.x / 16, rr = threadIdx.x % 16;
        sums[((size_t)blockIdx.y * H + h0 + j) * 16 + rr] = (wsum[j][0][rr] + wsum[j][1][rr]) + (wsum[j][2][rr] + wsum[j][3][rr]);
    }
}

// grid (H / NH, ranges of the launch), 256 threads
template <uint32_t HD, int NH, bool TREE = false>
__device__ __forceinline__ void
px8_pv_body(const bf16_t* Q, const pp_seg* segs, const px_range* tab, uint32_t ebase, const uint8_t* kq, const uint8_t* vq, const int8_t* kexp,
            const int8_t* vexp, uint64_t cache_stride, uint64_t exp_stride, const float* sums, float* part, bf16_t* out, uint32_t H, uint32_t n_rep,
            uint32_t max_seq, float scale, const float* etab, const tv_node* nodes = nullptr)
{
    constexpr uint32_t DT = HD / 16;
    __shared__ float inv_sum[NH][16];
    // (the exp window and, behind the key loop, the waves' partial outputs share one buffer, as in px_pv_body)
    constexpr uint32_t NW = 2 * pf_exp_window::N, NO = 4 * 16 * (HD + 1);
    __shared__ __attribute__((aligned(16))) float lds[NW > NO ? NW : NO];
    const pf_exp_window ew{lds};
    ew.fill(etab);
    float (*osum)[16][HD + 1] = reinterpret_cast<float (*)[16][HD + 1]>(lds);
    const px_range e = tab[ebase + blockIdx.y];
    const pp_seg g = segs[e.seg];
    const uint32_t wave = threadIdx.x >> 6, h0 = blockIdx.x * NH;
    const px8_tile<HD, NH, TREE> t = px8_tile_of<HD, NH, TREE>(Q, g, e, kq, kexp, cache_stride, exp_stride, H, n_rep, max_seq, scale, h0, nodes);
    const uint32_t l15 = t.t.l15, lg = t.t.lg, kg = t.t.kg;
    const uint8_t* vbase = vq + (size_t)g.row * cache_stride + (size_t)(h0 / n_rep) * HD * max_seq;
    const int8_t* vx = vexp + (size_t)g.row * exp_stride + (size_t)(h0 / n_rep) * max_seq;
    const uint32_t b_lo = (uint32_t)e.k_lo / 32, b_end = ((uint32_t)e.k_hi + 31) / 32;
    if (threadIdx.x < 16 * NH) {
        // the row's sum: the tile's ranges first to last (px_pv_body)
        const uint32_t j = threadIdx.x / 16, rr = threadIdx.x % 16;
        float s = 0.0f;
        for (int32_t i = 0; i < e.n; i++) s += sums[((size_t)((uint32_t)(e.first + i) - ebase) * H + h0 + j) * 16 + rr];
        inv_sum[j][rr] = s == 0.0f ? 0.0f : 1.0f / s;
    }
    kv8_kfrag<HD> k0, k1;
    t.load_k((b_lo + wave) * 32, 0, k0);
    __syncthreads(); // the exp window is filled, the sums are there
    float inv[NH];
#pragma unroll
    for (int j = 0; j < NH; j++) inv[j] = inv_sum[j][l15];
    pf_f32x4 oacc[NH][DT];
#pragma unroll
    for (int j = 0; j < NH; j++)
#pragma unroll
        for (uint32_t d = 0; d < DT; d++) oacc[j][d] = pf_f32x4{0, 0, 0, 0};
    for (uint32_t b = b_lo + wave; b < b_end; b += 4) {
        // the block's V bytes (every tile: 8 bytes each) and its eight exponents, requested before the scores
        const uint32_t c = b * 32 + kg, cc = c + 8 <= max_seq ? c : max_seq - 8;
        const uint8_t* vp = vbase + (size_t)l15 * max_seq + cc;
        uint2 vbs[DT];
#pragma unroll
        for (uint32_t d = 0; d < DT; d++) vbs[d] = *reinterpret_cast<const uint2*>(vp + (size_t)d * 16 * max_seq);
        const uint2 xb = *reinterpret_cast<const uint2*>(vx + cc);
        uint4 pa[NH];
        {
            float sv[NH][4];
            t.load_k(b * 32, 1, k1);
            t.score(b * 32, 0, k0, sv);
#pragma unroll
            for (int j = 0; j < NH; j++) {
                pa[j].x = pack_bf16x2(BF::rt(ew(sv[j][0]) * inv[j]), BF::rt(ew(sv[j][1]) * inv[j]));
                pa[j].y = pack_bf16x2(BF::rt(ew(sv[j][2]) * inv[j]), BF::rt(ew(sv[j][3]) * inv[j]));
            }
            t.load_k((b + 4) * 32, 0, k0); // (past the range: clamped to the tile's last key, never used)
            t.score(b * 32, 1, k1, sv);
#pragma unroll
            for (int j = 0; j < NH; j++) {
                pa[j].z = pack_bf16x2(BF::rt(ew(sv[j][0]) * inv[j]), BF::rt(ew(sv[j][1]) * inv[j]));
                pa[j].w = pack_bf16x2(BF::rt(ew(sv[j][2]) * inv[j]), BF::rt(ew(sv[j][3]) * inv[j]));
            }
        }
        // a slot no row of the tile sees reads as byte 0 under exponent 0 (px_pv_body's element mask)
        uint32_t mlo, mhi;
        kv8_slot_masks(c, t.t.S, max_seq, mlo, mhi);
        float vs[8];
        kv8_scales8(make_uint2(xb.x & mlo, xb.y & mhi), vs);
#pragma unroll
        for (uint32_t d = 0; d < DT; d++) {
            const uint4 vb = kv8_deq8s(make_uint2(vbs[d].x & mlo, vbs[d].y & mhi), vs);
#pragma unroll
            for (int j = 0; j < NH; j++)
                oacc[j][d] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(pf_bf16x8, pa[j]), __builtin_bit_cast(pf_bf16x8, vb), oacc[j][d], 0, 0, 0);
        }
    }
    // the four waves' partial outputs, added in px_pv_body's order
#pragma unroll
    for (int j = 0; j < NH; j++) {
        __syncthreads(); // (the first: every wave is through with the exp window)
#pragma unroll
        for (uint32_t d = 0; d < DT; d++)
#pragma unroll
            for (int i = 0; i < 4; i++) osum[wave][lg * 4 + i][d * 16 + l15] = oacc[j][d][i];
        __syncthreads();
        float* po = part + ((size_t)blockIdx.y * H + h0 + j) * 16 * HD;
        for (uint32_t x = threadIdx.x; x < 16 * HD; x += blockDim.x) {
            const uint32_t rr = x / HD, d = x % HD, ro = (uint32_t)e.r0 + rr;
            const float o = (osum[0][rr][d] + osum[1][rr][d]) + (osum[2][rr][d] + osum[3][rr][d]);
            if (e.n > 1) po[rr * HD + d] = o;
            else if (ro < (uint32_t)g.len) out[((size_t)((uint32_t)g.off + ro) * H + h0 + j) * HD + d] = BF::st(o);
        }
    }
}

#define MC_PX_ATTN_F8(HD, NH, SFX)                                                                                                                  \
    extern "C" __global__ void __launch_bounds__(256)                                                                                               \
    mc_px8_sums##SFX##_bfloat_hd##HD(const bf16_t* Q, const pp_seg* segs, const px_range* tab, uint32_t ebase, const uint8_t* kq,                  \
                                       const int8_t* kexp, uint64_t cache_stride, uint64_t exp_stride, float* sums, uint32_t H, uint32_t n_rep,      \
                                       uint32_t max_seq, float scale, const float* etab)                                                            \
    {                                                                                                                                               \
        px8_sums_body<HD, NH>(Q, segs, tab, ebase, kq, kexp, cache_stride, exp_stride, sums, H, n_rep, max_seq, scale, etab);                        \
    }                                                                                                                                               \
    extern "C" __global__ void __launch_bounds__(256)                                                                                               \
    mc_px8_pv##SFX##_bfloat_hd##HD(const bf16_t* Q, const pp_seg* segs, const px_range* tab, uint32_t ebase, const uint8_t* kq, const uint8_t* vq, \
                                     const int8_t* kexp, const int8_t* vexp, uint64_t cache_stride, uint64_t exp_stride, const float* sums,          \
                                     float* part, bf16_t* out, uint32_t H, uint32_t n_rep, uint32_t max_seq, float scale, const float* etab)        \
    {                                                                                                                                               \
        px8_pv_body<HD, NH>(Q, segs, tab, ebase, kq, vq, kexp, vexp, cache_stride, exp_stride, sums, part, out, H, n_rep, max_seq, scale, etab);     \
    }
MC_PX_ATTN_F8(64, 1, )
MC_PX_ATTN_F8(64, 2, 2)
MC_PX_ATTN_F8(128, 1, )
MC_PX_ATTN_F8(128, 2, 2)
