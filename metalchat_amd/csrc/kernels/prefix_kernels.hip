// Shared-prefix rows (mc_prefix_*, include/metalchat_hip.h Part 2r): the attention of a ragged step on a batch whose rows may be ATTACHED to one
// shared prefix -- one more set of K / Vt planes per layer in a row's layout.  An attached row's slots [0, shared) are the prefix's (shared is a
// multiple of PB = 64), its slots [shared, kv_len) its own at the same absolute numbers; sp_len[r] = shared for an attached row, 0 for any other.
//
// What is shared is the cache operand of the MFMA.  attn_scores_bf / attn_pv_bf_body (decode_kernels.hip) put the n_rep query heads of one kv head
// on the 16 rows of v_mfma_f32_16x16x32_bf16 and leave 16 - n_rep rows zero; here G = 16 / n_rep batch rows sit against ONE K or V fragment:
// rows [gG, gG + G) are group g, and MFMA row i < G n_rep is (batch row gG + i / n_rep, head i % n_rep of the kv head).  MFMA rows are independent
// and everything behind the MFMA is those kernels' arithmetic restated for 16 live rows, so every (row, head) gets the bits of
// mc_b_attn_scores_rows_bfloat + mc_b_attn_pv_rows_bfloat on a row that holds a copy of the prefix.
//   scores  one launch, grid (nsplit, KV, 1 + B).  z = 0: the prefix's workgroup of (split, kv) loads its K fragments ONCE into registers and
//           loops over the groups (Q of the group as the A operand, the MFMA chain, T(acc), T(. scale), exp, the 16-slot shuffle sum, the four
//           wave sums as (w0 + w1) + (w2 + w3)).  z = 1 + r: attn_scores_bf over row r's own splits, the ones at or behind sp_len[r].
//   P.V     grid (hd / 16, KV, ceil(B / G)), 1024 threads.  Wave w takes k-steps w, w + 16, .. as attn_pv_bf_body does.  A k-step below
//           shared / 32 is ONE prefix V fragment against the P of all attached rows of the group; a k-step of a row's own slots is one MFMA per
//           row whose A rows outside that row are zero: exact +0 terms for the others (acc starts at +0.0 and never turns -0.0; caches are
//           finite behind kv_len, which attn_pv_bf_body relies on as well).  So every A row's accumulator receives its own k-steps in ascending
//           order, and the wave-order LDS sum and the single f2bf are pv_finish_store's.
// An idle row (rows[r].pos < 0) contributes zero operands and no stores but its attention output, +0.0.
#include "common.h"

using namespace mc;

// the prefix's workgroup of (split, kv): K fragments of slots [64 split, 64 split + 64) from the prefix planes, then every group that has a
// live attached row.  wsum is double-buffered by the groups run, so one barrier a group is enough
template <int HD>
__device__ __forceinline__ void
sp_scores_prefix(const bf16_t* __restrict__ q, const bf16_t* __restrict__ pkc, float* __restrict__ expv, float* __restrict__ psum,
                 const step_state* rows, const int32_t* __restrict__ sp_len, uint32_t n_rep, uint32_t max_seq, float scale, uint32_t nsplit,
                 uint32_t B, uint32_t G)
{
    __shared__ float wsum[2][4][16];
    const uint32_t split = blockIdx.x, kv = blockIdx.y, H = gridDim.y * n_rep;
    const uint32_t p_begin = split * PB;
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t col = lane & 15, c = lane >> 4;
    constexpr int KS = HD / 32;
    auto live = [&](uint32_t r) { return r < B && p_begin < (uint32_t)sp_len[r] && rows[r].pos >= 0; };

    // B fragments, once: K[slot = pos][d = ks*32 + c*8 + j]; every slot of the split lies in the prefix
    const uint32_t pos = p_begin + wave * 16 + col;
    const bf16_t* kbase = pkc + ((size_t)kv * max_seq + pos) * HD;
    uint4 kb[KS];
#pragma unroll
    for (int ks = 0; ks < KS; ks++) kb[ks] = *reinterpret_cast<const uint4*>(kbase + ks * 32 + c * 8);

    const uint32_t jr = col / n_rep, head = col % n_rep; // the A row this lane loads
    uint32_t par = 0;
    for (uint32_t r0 = 0; r0 < B; r0 += G) {
        bool any = false;
        for (uint32_t j = 0; j < G; j++) any = any || live(r0 + j);
        if (!any) continue; // (uniform)
        // A fragments: Q[(row, head) = col][d = ks*32 + c*8 + j], all G n_rep rows live
        const uint32_t r = r0 + jr;
        const bool mine = jr < G && live(r);
        uint4 qa[KS];
#pragma unroll
        for (int ks = 0; ks < KS; ks++) {
            qa[ks] = make_uint4(0, 0, 0, 0);
            if (mine) qa[ks] = *reinterpret_cast<const uint4*>(q + ((size_t)r * H + kv * n_rep + head) * HD + ks * 32 + c * 8);
        }
        f32x4_t acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ks = 0; ks < KS; ks++)
            acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, qa[ks]), __builtin_bit_cast(bf16x8_t, kb[ks]), acc, 0, 0, 0);
        // scores_finish for 16 live rows: lane (c, col) finishes MFMA row 4m + c of slot col
        float (*ws)[16] = wsum[par];
        par ^= 1;
#pragma unroll
        for (uint32_t m = 0; m < 4; m++) {
            const int src = (int)(m * 16 + col);
            const float v0 = __shfl(acc[0], src, 64), v1 = __shfl(acc[1], src, 64);
            const float v2 = __shfl(acc[2], src, 64), v3 = __shfl(acc[3], src, 64);
            const float own = c == 0 ? v0 : (c == 1 ? v1 : (c == 2 ? v2 : v3));
            const uint32_t a = 4 * m + c, ra = r0 + a / n_rep, ha = a % n_rep;
            float e = 0.0f;
            if (a / n_rep < G && live(ra)) {
                float s = BF::rt(own);
                s = BF::rt(s * scale);
                e = exp_precise(s);
                expv[((size_t)ra * H + kv * n_rep + ha) * max_seq + pos] = e;
            }
            e += __shfl_xor(e, 1, 64);
            e += __shfl_xor(e, 2, 64);
            e += __shfl_xor(e, 4, 64);
            e += __shfl_xor(e, 8, 64);
            if (col == 0) ws[wave][a] = e;
        }
        __syncthreads();
        if (threadIdx.x < 16) {
            const uint32_t a = threadIdx.x, ra = r0 + a / n_rep, ha = a % n_rep;
            if (a / n_rep < G && live(ra))
                psum[((size_t)ra * H + kv * n_rep + ha) * nsplit + split] = (ws[0][a] + ws[1][a]) + (ws[2][a] + ws[3][a]);
        }
    }
}

// grid (nsplit, KV, 1 + B), 256 threads.  z = 0: the prefix (kc of the prefix planes: pkc; shared: the slots it serves); z = 1 + r: row r's
// own splits through attn_scores_bf, an ordinary row (sp_len 0) all of its splits
extern "C" __global__ void __launch_bounds__(256)
mc_sp_attn_scores_bfloat(const bf16_t* q, const bf16_t* kc, const bf16_t* pkc, float* expv, float* psum, const step_state* rows,
                         const int32_t* sp_len, uint32_t n_rep, uint32_t hd, uint32_t max_seq, float scale, uint32_t nsplit,
                         uint64_t cache_stride, uint32_t B, uint32_t G, uint32_t shared)
{
    if (blockIdx.z == 0) {
        if (blockIdx.x * PB >= shared) return;
        if (hd == 128) sp_scores_prefix<128>(q, pkc, expv, psum, rows, sp_len, n_rep, max_seq, scale, nsplit, B, G);
        else if (hd == 64) sp_scores_prefix<64>(q, pkc, expv, psum, rows, sp_len, n_rep, max_seq, scale, nsplit, B, G);
        return;
    }
    const uint32_t r = blockIdx.z - 1, H = gridDim.y * n_rep;
    if (rows[r].pos < 0 || blockIdx.x * PB < (uint32_t)sp_len[r]) return;
    const bf16_t* qr = q + (size_t)r * H * hd;
    const bf16_t* kr = kc + r * cache_stride;
    float* er = expv + (size_t)r * H * max_seq;
    float* pr = psum + (size_t)r * H * nsplit;
    if (hd == 128) attn_scores_bf<128>(qr, kr, er, pr, nullptr, rows + r, n_rep, max_seq, scale, nsplit);
    else if (hd == 64) attn_scores_bf<64>(qr, kr, er, pr, nullptr, rows + r, n_rep, max_seq, scale, nsplit);
}

// One MFMA of the P.V kernel: k-step t of the V planes v, for the A rows `sel` names -- SP_ON_PREFIX: every row whose slots 32 t .. are the
// prefix's; j >= 0: row j of the group alone, in its own slots.  t = SP_NONE: nothing
enum : uint32_t { SP_NONE = 0xFFFFFFFFu };
enum { SP_ON_PREFIX = -1 };
struct sp_unit {
    uint32_t t = SP_NONE;
    const bf16_t* v = nullptr;
    int sel = SP_ON_PREFIX;
};

// grid (hd / 16, KV, ceil(B / G)), 1024 threads: group blockIdx.z.  vt: the rows' planes, pvt: the prefix's
extern "C" __global__ void __launch_bounds__(1024)
mc_sp_attn_pv_bfloat(const float* __restrict__ expv, const float* __restrict__ psum, const bf16_t* __restrict__ vt,
                     const bf16_t* __restrict__ pvt, bf16_t* __restrict__ out, const step_state* rows, const int32_t* __restrict__ sp_len,
                     uint32_t n_rep, uint32_t hd, uint32_t max_seq, uint32_t nsplit, uint64_t cache_stride, uint32_t B, uint32_t G)
{
    __shared__ float part[16 * 16 * 16];
    __shared__ float inv_s[16];
    const uint32_t db = blockIdx.x, kv = blockIdx.y, r0 = blockIdx.z * G, H = gridDim.y * n_rep;
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t col = lane & 15, c = lane >> 4;
    // row j of the group: its first own slot and its k-steps (0, 0: idle or past the batch)
    auto own_of = [&](uint32_t j) { return j < G && r0 + j < B && rows[r0 + j].pos >= 0 ? (uint32_t)sp_len[r0 + j] : 0u; };
    auto nk_of = [&](uint32_t j) { return j < G && r0 + j < B && rows[r0 + j].pos >= 0 ? ((uint32_t)rows[r0 + j].kv_len + 31) / 32 : 0u; };

    // this lane's A row: (row jr of the group, head); S = 0: not live
    const uint32_t jr = col / n_rep, head = col % n_rep;
    const uint32_t nk = nk_of(jr), own = own_of(jr);
    const uint32_t S = nk ? (uint32_t)rows[r0 + jr].kv_len : 0u;
    const float* erow = expv + ((size_t)(nk ? r0 + jr : 0) * H + kv * n_rep + head) * max_seq;
    const size_t vrow = ((size_t)kv * hd + db * 16 + col) * max_seq;

    f32x4_t acc = {0.f, 0.f, 0.f, 0.f};
    uint4 vb[4];
    float4 e0[4], e1[4];
    sp_unit un[4];
    // all loads of a round first (attn_pv_bf_body): the V fragment of each unit, and this lane's 8 numerators where the unit names its row
    auto request = [&]() {
#pragma unroll
        for (int u = 0; u < 4; u++) {
            e0[u] = make_float4(0.f, 0.f, 0.f, 0.f);
            e1[u] = e0[u];
            if (un[u].t == SP_NONE) continue;
            const uint32_t p0 = un[u].t * 32 + c * 8;
            const uint32_t pl = p0 + 8 <= max_seq ? p0 : max_seq - 8;
            vb[u] = *reinterpret_cast<const uint4*>(un[u].v + vrow + pl);
            const bool mine = un[u].sel == SP_ON_PREFIX ? un[u].t * 32 < own : ((int)jr == un[u].sel && un[u].t < nk);
            if (mine && p0 < S) {
                e0[u] = *reinterpret_cast<const float4*>(erow + p0);
                e1[u] = *reinterpret_cast<const float4*>(erow + p0 + 4);
            }
        }
    };
    auto consume = [&](float inv) {
#pragma unroll
        for (int u = 0; u < 4; u++) {
            if (un[u].t == SP_NONE) continue;
            const uint32_t p0 = un[u].t * 32 + c * 8;
            const float e[8] = {e0[u].x, e0[u].y, e0[u].z, e0[u].w, e1[u].x, e1[u].y, e1[u].z, e1[u].w};
            uint32_t w[4];
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const float pa = (p0 + 2 * j < S) ? e[2 * j] * inv : 0.0f;
                const float pb = (p0 + 2 * j + 1 < S) ? e[2 * j + 1] * inv : 0.0f;
                w[j] = pack_bf16x2(pa, pb); // softmax output rounded to bf16
            }
            const uint4 pa4 = make_uint4(w[0], w[1], w[2], w[3]);
            acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, pa4), __builtin_bit_cast(bf16x8_t, vb[u]), acc, 0, 0, 0);
        }
    };

    // the prefix's k-steps of this wave, four a round: [0, kpre), kpre = shared / 32 if the group has a live attached row
    uint32_t kpre = 0;
    for (uint32_t j = 0; j < G; j++) kpre = max(kpre, own_of(j) / 32);
    auto prefix_round = [&](uint32_t t0) {
#pragma unroll
        for (int u = 0; u < 4; u++) {
            un[u] = sp_unit{};
            if (t0 + 16 * u < kpre) un[u] = sp_unit{t0 + 16 * u, pvt, SP_ON_PREFIX};
        }
    };
    // the first round is requested BEFORE the denominators are reduced, as attn_pv_bf_body does
    uint32_t t0 = wave;
    prefix_round(t0);
    request();
    // softmax_inv per (row, head): the partials of a head added by a whole wave, lane-strided, then the shuffle tree
    { // (16 waves: A row `wave` each)
        const uint32_t a = wave, ja = a / n_rep, nka = nk_of(ja);
        float t = 0.0f;
        if (nka) {
            const float* prow = psum + ((size_t)(r0 + ja) * H + kv * n_rep + a % n_rep) * nsplit;
            const uint32_t nact = ((uint32_t)rows[r0 + ja].kv_len + PB - 1) / PB;
            for (uint32_t sp = lane; sp < nact; sp += 64) t += prow[sp];
            t = wave_sum(t);
        }
        if (lane == 0) inv_s[a] = nka ? 1.0f / t : 0.0f;
    }
    __syncthreads();
    const float inv = inv_s[col];
    while (t0 < kpre) {
        consume(inv);
        t0 += 64;
        prefix_round(t0);
        request();
    }
    // the rows' own k-steps, four rows a round: k-step t of wave t % 16, every row from its first own k-step to its last
    for (uint32_t j0 = 0; j0 < G; j0 += 4) {
        uint32_t tb = SP_NONE, te = 0;
        for (uint32_t j = j0; j < j0 + 4; j++) {
            if (!nk_of(j)) continue;
            tb = min(tb, own_of(j) / 32);
            te = max(te, nk_of(j));
        }
        if (tb == SP_NONE) continue;
        for (uint32_t t = tb + ((wave - tb) & 15u); t < te; t += 16) {
#pragma unroll
            for (int u = 0; u < 4; u++) {
                const uint32_t j = j0 + u;
                un[u] = sp_unit{};
                if (t >= own_of(j) / 32 && t < nk_of(j)) un[u] = sp_unit{t, vt + (r0 + j) * cache_stride, (int)j};
            }
            request();
            consume(inv);
        }
    }

    // pv_finish_store for 16 live rows: the waves' tiles added in wave order, one rounding; an idle row's output is +0.0
#pragma unroll
    for (int i = 0; i < 4; i++) part[(wave * 16 + c * 4 + i) * 16 + col] = acc[i];
    __syncthreads();
    if (threadIdx.x < 256) {
        const uint32_t a = threadIdx.x / 16, d = threadIdx.x % 16, ja = a / n_rep;
        if (ja >= G || r0 + ja >= B) return;
        float v = part[(0 * 16 + a) * 16 + d];
        for (uint32_t w = 1; w < 16; w++) v += part[(w * 16 + a) * 16 + d]; // wave order
        out[((size_t)(r0 + ja) * H + kv * n_rep + a % n_rep) * hd + db * 16 + d] = nk_of(ja) ? f2bf(v) : (bf16_t)0;
    }
}
