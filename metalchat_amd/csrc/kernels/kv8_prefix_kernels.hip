// Shared-prefix rows on an fp8 batch (mc_kv_prefix_set, include/metalchat_hip.h Part 2s): the attention of a ragged step whose rows may be attached
// to a shared prefix that is held, like a row, as four planes per layer -- K bytes [kv][max_seq][hd], V bytes [kv][hd][max_seq], kexp and vexp
// [kv][max_seq] (kv8_kernels.hip).  The groups are prefix_kernels.hip's: G = 16 / n_rep batch rows on the 16 MFMA rows against ONE K or V fragment
// of the prefix; sp_len[r] = shared (a multiple of PB = 64) for an attached row, 0 for any other.
//
// What is shared here is the CONVERTED operand.  The per-row fp8 kernels turn bytes and exponents into the bfloat16 MFMA operand once per row
// and k-step (P.V: about 32 VALU instructions in front of every MFMA); on the prefix the operand is made once and serves
//   scores  every group of the batch: the prefix's workgroup of (split, kv) loads hd / 32 x 8 bytes a lane and its slot's exponent, converts them
//           with four v_cvt_scalef32_pk_bf16_fp8 per k-step (kv8_deq8) into hd / 32 operands in registers, and loops over the groups as
//           sp_scores_prefix does.  Every slot of a prefix split lies below shared: no clamp, no mask.
//   P.V     the GW consecutive groups of a workgroup (grid z = ceil(ceil(B / G) / GW), GW = 1, 2 or 4, the plan's choice): a lane loads 8 V bytes
//           and the 8 exponents of its slots, makes the operand once (kv8_deq8x8, no masks) and issues one MFMA per group against it, each group
//           into its own 4-register accumulator.  A round keeps four (k-step, group) units in flight as 4 / GW k-steps x GW groups: the numerator
//           loads in flight are mc_sp_attn_pv_bfloat's, the V and exponent loads and the conversions fall by the factor GW.
// A row's own slots come from its own planes, one MFMA per row whose other A rows are zero, through kv8_deq8x8 with attn_pv_f8_body's byte and
// exponent masks at and past kv_len and its clamp at max_seq - 8.  The other rows' products are exact zeros: a byte of the rule is never NaN
// and the exponents lie in [-100, 119], so every operand is finite.  Each A row's accumulator therefore receives its own k-steps in ascending
// order, and every (row, head) gets the bits of mc_b_attn_scores_f8_rows_bfloat + mc_b_attn_pv_f8_rows_bfloat on a row whose planes hold a byte
// copy of the prefix in [0, shared): the tails of scores_finish, softmax_inv and pv_finish_store are restated for 16 live rows as in
// prefix_kernels.hip.
// LDS of the P.V kernel: ONE 16 KiB tile of wave partials, reused group after group (two barriers a group), and 16 denominators per group:
// 16 KiB + 256 bytes whatever GW is.
#include "common.h"

using namespace mc;

// sp_scores_prefix with the K operands made from the prefix's bytes, once for all groups
template <int HD>
__device__ __forceinline__ void
sp8_scores_prefix(const bf16_t* __restrict__ q, const uint8_t* __restrict__ pkq, const int8_t* __restrict__ pkexp, float* __restrict__ expv,
                  float* __restrict__ psum, const step_state* rows, const int32_t* __restrict__ sp_len, uint32_t n_rep, uint32_t max_seq, float scale,
                  uint32_t nsplit, uint32_t B, uint32_t G)
{
    __shared__ float wsum[2][4][16];
    const uint32_t split = blockIdx.x, kv = blockIdx.y, H = gridDim.y * n_rep;
    const uint32_t p_begin = split * PB;
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t col = lane & 15, c = lane >> 4;
    constexpr int KS = HD / 32;
    auto live = [&](uint32_t r) { return r < B && p_begin < (uint32_t)sp_len[r] && rows[r].pos >= 0; };

    // B fragments, once: K[slot = pos][d = ks*32 + c*8 + j] from 8 bytes and the slot's one scale; every slot of the split lies in the prefix
    const uint32_t pos = p_begin + wave * 16 + col;
    const size_t vec = (size_t)kv * max_seq + pos;
    const uint8_t* kbase = pkq + vec * HD;
    uint2 kbytes[KS];
#pragma unroll
    for (int ks = 0; ks < KS; ks++) kbytes[ks] = *reinterpret_cast<const uint2*>(kbase + ks * 32 + c * 8);
    const float kscale = kv8_pow2(pkexp[vec]);
    uint4 kb[KS];
#pragma unroll
    for (int ks = 0; ks < KS; ks++) kb[ks] = kv8_deq8(kbytes[ks], kscale);

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

// grid (nsplit, KV, 1 + B), 256 threads.  z = 0: the prefix (pkq, pkexp: its K planes; shared: the slots it serves); z = 1 + r: row r's own
// splits through attn_scores_f8, an ordinary row (sp_len 0) all of its splits.  cache_stride, exp_stride: between the rows' byte / exponent planes
extern "C" __global__ void __launch_bounds__(256)
mc_sp8_attn_scores_bfloat(const bf16_t* q, const uint8_t* kq, const int8_t* kexp, const uint8_t* pkq, const int8_t* pkexp, float* expv, float* psum,
                          const step_state* rows, const int32_t* sp_len, uint32_t n_rep, uint32_t hd, uint32_t max_seq, float scale, uint32_t nsplit,
                          uint64_t cache_stride, uint64_t exp_stride, uint32_t B, uint32_t G, uint32_t shared)
{
    if (blockIdx.z == 0) {
        if (blockIdx.x * PB >= shared) return;
        if (hd == 128) sp8_scores_prefix<128>(q, pkq, pkexp, expv, psum, rows, sp_len, n_rep, max_seq, scale, nsplit, B, G);
        else if (hd == 64) sp8_scores_prefix<64>(q, pkq, pkexp, expv, psum, rows, sp_len, n_rep, max_seq, scale, nsplit, B, G);
        return;
    }
    const uint32_t r = blockIdx.z - 1, H = gridDim.y * n_rep;
    if (rows[r].pos < 0 || blockIdx.x * PB < (uint32_t)sp_len[r]) return;
    const bf16_t* qr = q + (size_t)r * H * hd;
    const uint8_t* kr = kq + r * cache_stride;
    const int8_t* xr = kexp + r * exp_stride;
    float* er = expv + (size_t)r * H * max_seq;
    float* pr = psum + (size_t)r * H * nsplit;
    if (hd == 128) attn_scores_f8<128>(qr, kr, xr, er, pr, rows + r, n_rep, max_seq, scale, nsplit);
    else if (hd == 64) attn_scores_f8<64>(qr, kr, xr, er, pr, rows + r, n_rep, max_seq, scale, nsplit);
}


// LDS of the P.V kernel: one 16 KiB tile of wave partials per group -- a lane parks its accumulator of group g at the place the finish reads it --,
// the 16 denominators of each group and the table of the rows' first own slot and kv_len
struct sp8_pv_lds {
    float part[4][16 * 16 * 16];
    float inv_s[4][16];
    uint32_t lo[64], len[64]; // of row j of group g at [16 g + j]; len 0: idle or past the batch
};

// The prefix's k-steps of the P.V workgroup of GW consecutive groups, the first of them GW blockIdx.z; pvq, pvexp: the prefix's planes.  Leaves
// every lane's accumulator of group g in its tile, and the denominators and the rows' table for sp8_pv_own_finish
template <int GW>
__device__ __forceinline__ void
sp8_pv_prefix(const float* __restrict__ expv, const float* __restrict__ psum, const uint8_t* __restrict__ pvq, const int8_t* __restrict__ pvexp,
              const step_state* rows, const int32_t* __restrict__ sp_len, uint32_t n_rep, uint32_t hd, uint32_t max_seq, uint32_t nsplit, uint32_t B,
              uint32_t G, uint32_t shared, sp8_pv_lds& lds)
{
    constexpr int KR = 4 / GW; // k-steps of a round
    const uint32_t db = blockIdx.x, kv = blockIdx.y, g0 = blockIdx.z * GW, H = gridDim.y * n_rep;
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t col = lane & 15, c = lane >> 4;
    // row j of group g0 + g: the batch row, and whether it is in the step
    auto row_of = [&](uint32_t g, uint32_t j) { return (g0 + g) * G + j; };
    auto alive = [&](uint32_t g, uint32_t j) { return j < G && row_of(g, j) < B && rows[row_of(g, j)].pos >= 0; };
    if (threadIdx.x < GW * 16) {
        const uint32_t g = threadIdx.x / 16, j = threadIdx.x % 16;
        const bool is = alive(g, j);
        lds.lo[threadIdx.x] = is ? (uint32_t)sp_len[row_of(g, j)] : 0u;
        lds.len[threadIdx.x] = is ? (uint32_t)rows[row_of(g, j)].kv_len : 0u;
    }

    // this lane's A row in every group: (row jr, head).  eh: its (row, head) index into expv, row 0 where it is not live; amask bit g: it is
    // attached, its slots below `shared` are the prefix's; pmask bit g (uniform): the group has such a row
    const uint32_t jr = col / n_rep, head = col % n_rep;
    uint32_t eh[GW], amask = 0, pmask = 0;
#pragma unroll
    for (int g = 0; g < GW; g++) {
        const bool live = alive(g, jr), att = live && sp_len[row_of(g, jr)] > 0;
        eh[g] = (live ? row_of(g, jr) : 0u) * H + kv * n_rep + head;
        amask |= (att ? 1u : 0u) << g;
        pmask |= (__builtin_amdgcn_ballot_w64(att) != 0 ? 1u : 0u) << g; // the 16 columns of a wave cover the G rows of a group
    }
    const uint32_t kpre = pmask ? shared / 32 : 0u;
    const size_t vrow = ((size_t)kv * hd + db * 16 + col) * max_seq, xrow = (size_t)kv * max_seq;

    f32x4_t acc[GW];
#pragma unroll
    for (int g = 0; g < GW; g++) acc[g] = f32x4_t{0.f, 0.f, 0.f, 0.f};
    uint2 vb[KR], xb[KR];
    float4 e0[4], e1[4];
    // KR k-steps x GW groups a round; unit (i, g) is e0 / e1 [i GW + g], k-step i is vb / xb [i].  All loads of a round are requested before its
    // first conversion
    auto request = [&](uint32_t t0) {
#pragma unroll
        for (int i = 0; i < KR; i++) {
            const uint32_t t = t0 + 16 * i, p0 = t * 32 + c * 8;
            if (t >= kpre) continue;
            vb[i] = *reinterpret_cast<const uint2*>(pvq + vrow + p0); // p0 + 8 <= shared <= max_seq
            xb[i] = *reinterpret_cast<const uint2*>(pvexp + xrow + p0);
#pragma unroll
            for (int g = 0; g < GW; g++) {
                e0[i * GW + g] = make_float4(0.f, 0.f, 0.f, 0.f);
                e1[i * GW + g] = e0[i * GW + g];
                if (amask >> g & 1u) { // (shared < kv_len: an attached row stands behind the prefix)
                    const float* erow = expv + (size_t)eh[g] * max_seq + p0;
                    e0[i * GW + g] = *reinterpret_cast<const float4*>(erow);
                    e1[i * GW + g] = *reinterpret_cast<const float4*>(erow + 4);
                }
            }
        }
    };
    // the first round is requested BEFORE the denominators are reduced, as attn_pv_f8_body does
    uint32_t t0 = wave;
    request(t0);
    // softmax_inv per (row, head): the partials of a head added by a whole wave, lane-strided, then the shuffle tree (16 waves: A row `wave` each)
#pragma unroll 1
    for (uint32_t g = 0; g < (uint32_t)GW; g++) {
        const uint32_t a = wave, ja = a / n_rep;
        const bool is = alive(g, ja);
        float t = 0.0f;
        if (is) {
            const float* prow = psum + ((size_t)row_of(g, ja) * H + kv * n_rep + a % n_rep) * nsplit;
            const uint32_t nact = ((uint32_t)rows[row_of(g, ja)].kv_len + PB - 1) / PB;
            for (uint32_t sp = lane; sp < nact; sp += 64) t += prow[sp];
            t = wave_sum(t);
        }
        if (lane == 0) lds.inv_s[g][a] = is ? 1.0f / t : 0.0f;
    }
    __syncthreads();
    float inv[GW];
#pragma unroll
    for (int g = 0; g < GW; g++) inv[g] = lds.inv_s[g][col];
    while (t0 < kpre) {
#pragma unroll
        for (int i = 0; i < KR; i++) {
            if (t0 + 16 * i >= kpre) continue;
            const bf16x8_t v = __builtin_bit_cast(bf16x8_t, kv8_deq8x8(vb[i], xb[i])); // ONCE for the GW groups; no masks: every slot is below shared
#pragma unroll
            for (int g = 0; g < GW; g++) {
                if (!(pmask >> g & 1u)) continue; // (uniform)
                // the normalised P of the group's attached rows (the others' numerators are zeros); every slot lies below their kv_len
                const int u = i * GW + g;
                const uint4 pa = make_uint4(pack_bf16x2(e0[u].x * inv[g], e0[u].y * inv[g]), pack_bf16x2(e0[u].z * inv[g], e0[u].w * inv[g]),
                                            pack_bf16x2(e1[u].x * inv[g], e1[u].y * inv[g]), pack_bf16x2(e1[u].z * inv[g], e1[u].w * inv[g]));
                acc[g] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, pa), v, acc[g], 0, 0, 0);
            }
        }
        t0 += 16 * KR;
        request(t0);
    }
#pragma unroll
    for (int g = 0; g < GW; g++)
#pragma unroll
        for (int i = 0; i < 4; i++) lds.part[g][(wave * 16 + c * 4 + i) * 16 + col] = acc[g][i];
}

// ... then, group after group, the rows' own k-steps from their own planes vq, vexp on top of the parked accumulators, and the finish
__device__ __forceinline__ void
sp8_pv_own_finish(const float* __restrict__ expv, const uint8_t* __restrict__ vq, const int8_t* __restrict__ vexp, bf16_t* __restrict__ out, uint32_t n_rep,
                  uint32_t hd, uint32_t max_seq, uint64_t cache_stride, uint64_t exp_stride, uint32_t B, uint32_t G, uint32_t GW, sp8_pv_lds& lds)
{
    const uint32_t db = blockIdx.x, kv = blockIdx.y, g0 = blockIdx.z * GW, H = gridDim.y * n_rep;
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t col = lane & 15, c = lane >> 4;
    const uint32_t jr = col / n_rep, head = col % n_rep;
    const size_t vrow = ((size_t)kv * hd + db * 16 + col) * max_seq, xrow = (size_t)kv * max_seq;
    constexpr int R = 2; // rows of a round: four would need more scalar registers than there are (the per-row pointers, bounds and lane masks)
    uint2 vb[R], xb[R];
    float4 e0[R], e1[R];
#pragma unroll 1
    for (uint32_t g = 0; g < GW; g++) {
        const uint32_t r0 = (g0 + g) * G;
        if (r0 >= B) break; // (uniform)
        f32x4_t acc;
#pragma unroll
        for (int i = 0; i < 4; i++) acc[i] = lds.part[g][(wave * 16 + c * 4 + i) * 16 + col]; // (this lane's own words)
        const float inv = lds.inv_s[g][col];
        const uint32_t S = jr < G ? lds.len[16 * g + jr] : 0u; // this lane's row
        const float* erow = expv + ((size_t)(S ? r0 + jr : 0u) * H + kv * n_rep + head) * max_seq;
        // R rows a round: k-step t of wave t % 16, every row from its first own k-step to its last; one MFMA per row, whose other A rows are zero
        for (uint32_t j0 = 0; j0 < G; j0 += R) {
            uint32_t lo[R], Su[R], tb = SP_NONE, te = 0;
#pragma unroll
            for (int u = 0; u < R; u++) {
                lo[u] = __builtin_amdgcn_readfirstlane(lds.lo[16 * g + j0 + u]); // (uniform: into scalar registers)
                Su[u] = j0 + u < G ? __builtin_amdgcn_readfirstlane(lds.len[16 * g + j0 + u]) : 0u;
                if (!Su[u]) continue;
                tb = min(tb, lo[u] / 32);
                te = max(te, (Su[u] + 31) / 32);
            }
            if (tb == SP_NONE) continue;
            for (uint32_t t = tb + ((wave - tb) & 15u); t < te; t += 16) {
                const uint32_t p0 = t * 32 + c * 8;
                const uint32_t pl = p0 + 8 <= max_seq ? p0 : max_seq - 8;
                // slot p0 + k of this lane's row lies below its kv_len: all ones, else 0 -- `cond ? e inv : 0.0f` without a lane mask per slot
                uint32_t below[8];
#pragma unroll
                for (int k = 0; k < 8; k++) below[k] = (uint32_t)((int32_t)(p0 + k - S) >> 31);
                bool on[R];
#pragma unroll
                for (int u = 0; u < R; u++) { // all loads of the round first
                    on[u] = t * 32 >= lo[u] && t * 32 < Su[u];
                    if (!on[u]) continue;
                    const uint32_t r = r0 + j0 + u;
                    vb[u] = *reinterpret_cast<const uint2*>(vq + r * cache_stride + vrow + pl);
                    xb[u] = *reinterpret_cast<const uint2*>(vexp + r * exp_stride + xrow + pl);
                    e0[u] = make_float4(0.f, 0.f, 0.f, 0.f);
                    e1[u] = e0[u];
                    if (jr == j0 + u && p0 < S) {
                        e0[u] = *reinterpret_cast<const float4*>(erow + p0);
                        e1[u] = *reinterpret_cast<const float4*>(erow + p0 + 4);
                    }
                }
#pragma unroll
                for (int u = 0; u < R; u++) {
                    if (!on[u]) continue;
                    const float e[8] = {e0[u].x, e0[u].y, e0[u].z, e0[u].w, e1[u].x, e1[u].y, e1[u].z, e1[u].w};
                    uint32_t w[4];
#pragma unroll
                    for (int j = 0; j < 4; j++) {
                        const float pa = __uint_as_float(__float_as_uint(e[2 * j] * inv) & below[2 * j]);
                        const float pb = __uint_as_float(__float_as_uint(e[2 * j + 1] * inv) & below[2 * j + 1]);
                        w[j] = pack_bf16x2(pa, pb); // softmax output rounded to bf16
                    }
                    // attn_pv_f8_body's masks: the slots [p0, p0 + 8) below the unit row's kv_len keep their bytes and exponents, the others read as +0.0
                    const uint32_t nv = p0 < Su[u] ? min(Su[u] - p0, 8u) : 0u;
                    const uint32_t mlo = nv >= 4 ? 0xFFFFFFFFu : (1u << (8 * nv)) - 1u;
                    const uint32_t mhi = nv >= 8 ? 0xFFFFFFFFu : (nv > 4 ? (1u << (8 * (nv - 4))) - 1u : 0u);
                    const uint2 vbytes = make_uint2(vb[u].x & mlo, vb[u].y & mhi), xbytes = make_uint2(xb[u].x & mlo, xb[u].y & mhi);
                    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, make_uint4(w[0], w[1], w[2], w[3])),
                                                                  __builtin_bit_cast(bf16x8_t, kv8_deq8x8(vbytes, xbytes)), acc, 0, 0, 0);
                }
            }
        }
#pragma unroll
        for (int i = 0; i < 4; i++) lds.part[g][(wave * 16 + c * 4 + i) * 16 + col] = acc[i];
    }
    __syncthreads();
    // pv_finish_store for 16 live rows, a quarter of the workgroup per group: the waves' tiles added in wave order, one rounding; an idle
    // row's output is +0.0
    const uint32_t g = threadIdx.x / 256, a = threadIdx.x % 256 / 16, d = threadIdx.x % 16, ja = a / n_rep, r = (g0 + g) * G + ja;
    if (g < GW && ja < G && r < B) {
        float v = lds.part[g][(0 * 16 + a) * 16 + d];
        for (uint32_t w = 1; w < 16; w++) v += lds.part[g][(w * 16 + a) * 16 + d]; // wave order
        out[((size_t)r * H + kv * n_rep + a % n_rep) * hd + db * 16 + d] = lds.len[16 * g + ja] ? f2bf(v) : (bf16_t)0;
    }
}

// grid (hd / 16, KV, ceil(ceil(B / G) / GW)), 1024 threads: groups [GW blockIdx.z, GW blockIdx.z + GW).  GW: 1, 2 or 4; shared: the prefix's slots
extern "C" __global__ void __launch_bounds__(1024)
mc_sp8_attn_pv_bfloat(const float* expv, const float* psum, const uint8_t* vq, const int8_t* vexp, const uint8_t* pvq, const int8_t* pvexp, bf16_t* out,
                      const step_state* rows, const int32_t* sp_len, uint32_t n_rep, uint32_t hd, uint32_t max_seq, uint32_t nsplit,
                      uint64_t cache_stride, uint64_t exp_stride, uint32_t B, uint32_t G, uint32_t GW, uint32_t shared)
{
    __shared__ sp8_pv_lds lds;
    if (GW == 4) sp8_pv_prefix<4>(expv, psum, pvq, pvexp, rows, sp_len, n_rep, hd, max_seq, nsplit, B, G, shared, lds);
    else if (GW == 2) sp8_pv_prefix<2>(expv, psum, pvq, pvexp, rows, sp_len, n_rep, hd, max_seq, nsplit, B, G, shared, lds);
    else sp8_pv_prefix<1>(expv, psum, pvq, pvexp, rows, sp_len, n_rep, hd, max_seq, nsplit, B, G, shared, lds);
    sp8_pv_own_finish(expv, vq, vexp, out, n_rep, hd, max_seq, cache_stride, exp_stride, B, G, GW == 4 || GW == 2 ? GW : 1, lds);
}
