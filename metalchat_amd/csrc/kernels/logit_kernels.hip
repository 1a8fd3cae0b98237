// Row logit processors (mc_row_mask_*, mc_row_penalty_*, include/metalchat_hip.h Part 2l): ONE launch between the head GEMV and the
// pick that rewrites, in place, the logits of every row that has a token mask or penalties.  table[r] holds row r's settings (abi.h
// row_logits, resolved on the host); with T = bfloat16, x the float value of logit t and c the row's count of token t:
//   c  = counts[r][t]                          after this step's input token has been counted (below)
//   x1 = c > 0 ? (x > 0 ? x * inv_rep : x * rep) : x
//   x2 = c > 0 ? x1 - (freq * float(c) + pres) : x
//   y  = allowed(t) ? T(x2) : -inf             (an untouched x keeps its bits, -0.0 and NaNs included)
// every operation one float32 operation in the order written (the build sets -ffp-contract=off); no division: inv_rep comes from
// the host.  The pick launches then run on y unchanged.
//   grid      (ceil(n / LP_CHUNK), B): a workgroup of LP_THREADS threads streams LP_CHUNK logits of one row.  The row is a grid
//             index, so every branch on its settings is uniform per workgroup; workgroups of rows with nothing set (flags == 0)
//             exit at once, and in the _rows form those of idle rows.
//   memory    from the first 16-byte boundary of the chunk on, a thread owns 8 logits: one 16-byte load and store of logits, two
//             16-byte loads of counts, one mask dword (two where the 8 bits straddle words, which only a row whose base is not
//             16-byte aligned has).  Adjacent threads take adjacent pieces.  The elements in front of that boundary and behind the
//             last whole piece take the element path, as the whole chunk does where the counts are not aligned with the logits.
//             The logits of a batch ([B][vocab], vocab % 16 == 0) are all whole pieces.
//   counts    a row with penalties counts the step's input token rows[r].token before it penalises (`count` != 0; the packed passes
//             give 0): the ONE thread that owns element `token` adds 1, stores that one word and uses the new value -- no atomics,
//             no other word of counts is written.  Rows without penalties neither read nor write counts, rows without a mask do
//             not read masks: either table may be null then.
// No LDS, no atomics, nothing in private memory.
#include "common.h"

using namespace mc;
using namespace mc::abi;

constexpr bf16_t LP_NEG_INF = 0xFF80;

__device__ __forceinline__ bf16_t
logit_rule(bf16_t b, int32_t c, bool allowed, const row_logits& s)
{
    if (c > 0) {
        const float x = bf2f(b);
        const float x1 = x > 0.0f ? x * s.inv_rep : x * s.rep;
        b = f2bf(x1 - (s.freq * (float)c + s.pres));
    }
    return allowed ? b : LP_NEG_INF;
}

// element t of the row: its count (the input token's goes up by one first), its mask bit, the rule
__device__ __forceinline__ void
logit_element(bf16_t* lr, const uint32_t* mr, int32_t* cr, uint32_t t, int32_t input, bool masked, bool pen, const row_logits& s)
{
    int32_t c = 0;
    if (pen) {
        c = cr[t];
        if ((int32_t)t == input) {
            c += 1;
            cr[t] = c;
        }
    }
    const bool allowed = !masked || ((mr[t >> 5] >> (t & 31)) & 1u);
    lr[t] = logit_rule(lr[t], c, allowed, s);
}

__device__ __forceinline__ void
logits_process_body(bf16_t* logits, uint32_t n, const row_logits* table, const uint32_t* masks, int32_t* counts, const step_state* rows,
                    int32_t count)
{
    const uint32_t r = blockIdx.y, tid = threadIdx.x;
    const row_logits s = table[r];
    if (!s.flags) return; // (uniform)
    const bool masked = (s.flags & ROW_LOGITS_MASK) != 0, pen = (s.flags & ROW_LOGITS_PENALTY) != 0;
    bf16_t* lr = logits + (size_t)r * n;
    const uint32_t* mr = masks + (size_t)r * ((n + 31) / 32);
    int32_t* cr = counts + (size_t)r * n;
    const int32_t input = pen && count ? rows[r].token : -1;
    // the chunk [lo, hi), its whole 16-byte pieces [vlo, vhi)
    const uint32_t lo = blockIdx.x * LP_CHUNK;
    if (lo >= n) return;
    const uint32_t hi = min(n, lo + LP_CHUNK);
    const uint32_t head = min(hi - lo, (uint32_t)((16u - (uint32_t)((uintptr_t)(lr + lo) & 15u)) & 15u) / 2u);
    const uint32_t vlo = lo + head;
    const bool co_aligned = !pen || ((uintptr_t)(cr + vlo) & 15u) == 0;
    const uint32_t nvec = co_aligned ? (hi - vlo) / 8 : 0, vhi = vlo + 8 * nvec;

    if (tid < nvec) {
        const uint32_t t = vlo + 8 * tid;
        const uint4 v = *reinterpret_cast<const uint4*>(lr + t);
        uint32_t w[4] = {v.x, v.y, v.z, v.w};
        int32_t c[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        if (pen) {
            const int4 c0 = *reinterpret_cast<const int4*>(cr + t), c1 = *reinterpret_cast<const int4*>(cr + t + 4);
            c[0] = c0.x, c[1] = c0.y, c[2] = c0.z, c[3] = c0.w;
            c[4] = c1.x, c[5] = c1.y, c[6] = c1.z, c[7] = c1.w;
            const uint32_t d = (uint32_t)(input - (int32_t)t); // (input = -1: far above 8)
            if (input >= 0 && d < 8) {
                int32_t bumped = 0;
#pragma unroll
                for (uint32_t j = 0; j < 8; j++) {
                    c[j] += j == d ? 1 : 0;
                    bumped = j == d ? c[j] : bumped;
                }
                cr[input] = bumped;
            }
        }
        uint32_t bits = 0xFFu;
        if (masked) {
            const uint32_t sh = t & 31;
            bits = mr[t >> 5] >> sh;
            if (sh > 24) bits |= mr[(t >> 5) + 1] << (32 - sh); // (t + 7 < n lies in that word)
        }
#pragma unroll
        for (uint32_t j = 0; j < 4; j++) {
            const bf16_t a = logit_rule((bf16_t)(w[j] & 0xFFFFu), c[2 * j], (bits >> (2 * j)) & 1u, s);
            const bf16_t b = logit_rule((bf16_t)(w[j] >> 16), c[2 * j + 1], (bits >> (2 * j + 1)) & 1u, s);
            w[j] = (uint32_t)a | ((uint32_t)b << 16);
        }
        *reinterpret_cast<uint4*>(lr + t) = make_uint4(w[0], w[1], w[2], w[3]);
    }
    for (uint32_t t = lo + tid; t < vlo; t += LP_THREADS) logit_element(lr, mr, cr, t, input, masked, pen, s);
    for (uint32_t t = vhi + tid; t < hi; t += LP_THREADS) logit_element(lr, mr, cr, t, input, masked, pen, s);
}

// the lockstep form: every row is active and counts its input token
extern "C" __global__ void __launch_bounds__(LP_THREADS)
mc_b_logits_process_bfloat(bf16_t* logits, uint32_t n, const row_logits* table, const uint32_t* masks, int32_t* counts, const step_state* rows)
{
    logits_process_body(logits, n, table, masks, counts, rows, 1);
}

// ragged: rows[r].pos < 0 marks an idle row, whose logits and counts stay as they are; count = 0 (the packed passes): the counts
// are read as they stand
extern "C" __global__ void __launch_bounds__(LP_THREADS)
mc_b_logits_process_rows_bfloat(bf16_t* logits, uint32_t n, const row_logits* table, const uint32_t* masks, int32_t* counts,
                                const step_state* rows, int32_t count)
{
    if (rows[blockIdx.y].pos < 0) return; // (uniform)
    logits_process_body(logits, n, table, masks, counts, rows, count);
}

// ------------------------------------------------------------------------------------------
// A verify call whose rows carry a mask or penalties (include/metalchat_hip.h Part 2m): the rule above for the M PACKED rows of the
// call, grid (ceil(n / LP_CHUNK), M).  Packed row m belongs to batch row vrows[m].row (abi.h verify_row): its settings are
// table[row], the step's table, its mask the row's, and its count of token t
//   c = counts[row][t] + #{ i : bit i of vrows[m].anc set and tokens[vrows[m].off + i] == t }
// -- the slot's count plus the chunk tokens fed up to and including this chunk row (a tree: the path from the root to the node),
// what the ragged steps would have counted in front of this pick.  counts is only READ here: mc_vs_count_accepted adds the accepted
// path behind the acceptance.  The <= 16 chunk tokens of the segment are read once per workgroup into LDS (-1 where the bit is
// clear); a thread compares them against the first of its 8 elements and only a hit walks the 8.  Workgroups of packed rows whose
// batch row has nothing set exit at once.  Memory access as above; no atomics, nothing in private memory.
// ------------------------------------------------------------------------------------------
__device__ __forceinline__ int32_t
v_path_hits(const int32_t* tk, uint32_t t)
{
    int32_t hits = 0;
#pragma unroll
    for (int i = 0; i < MC_VERIFY_MAX_LEN; i++) hits += tk[i] == (int32_t)t ? 1 : 0;
    return hits;
}

extern "C" __global__ void __launch_bounds__(LP_THREADS)
mc_vs_logits_process_bfloat(bf16_t* logits, uint32_t n, const verify_row* vrows, const row_logits* table, const uint32_t* masks,
                            const int32_t* counts, const int32_t* tokens)
{
    __shared__ int32_t tk[MC_VERIFY_MAX_LEN];
    const uint32_t m = blockIdx.y, tid = threadIdx.x;
    const verify_row v = vrows[m];
    const row_logits s = table[v.row];
    if (!s.flags) return; // (uniform)
    const bool masked = (s.flags & ROW_LOGITS_MASK) != 0, pen = (s.flags & ROW_LOGITS_PENALTY) != 0;
    const uint32_t lo = blockIdx.x * LP_CHUNK;
    if (lo >= n) return; // (uniform)
    if (tid < (uint32_t)MC_VERIFY_MAX_LEN) tk[tid] = pen && ((v.anc >> tid) & 1u) ? tokens[v.off + (int32_t)tid] : -1;
    __syncthreads();
    bf16_t* lr = logits + (size_t)m * n;
    const uint32_t* mr = masks + (size_t)v.row * ((n + 31) / 32);
    const int32_t* cr = counts + (size_t)v.row * n;
    // the chunk [lo, hi), its whole 16-byte pieces [vlo, vhi)
    const uint32_t hi = min(n, lo + LP_CHUNK);
    const uint32_t head = min(hi - lo, (uint32_t)((16u - (uint32_t)((uintptr_t)(lr + lo) & 15u)) & 15u) / 2u);
    const uint32_t vlo = lo + head;
    const bool co_aligned = !pen || ((uintptr_t)(cr + vlo) & 15u) == 0;
    const uint32_t nvec = co_aligned ? (hi - vlo) / 8 : 0, vhi = vlo + 8 * nvec;

    if (tid < nvec) {
        const uint32_t t = vlo + 8 * tid;
        const uint4 q = *reinterpret_cast<const uint4*>(lr + t);
        uint32_t w[4] = {q.x, q.y, q.z, q.w};
        int32_t c[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        if (pen) {
            const int4 c0 = *reinterpret_cast<const int4*>(cr + t), c1 = *reinterpret_cast<const int4*>(cr + t + 4);
            c[0] = c0.x, c[1] = c0.y, c[2] = c0.z, c[3] = c0.w;
            c[4] = c1.x, c[5] = c1.y, c[6] = c1.z, c[7] = c1.w;
#pragma unroll
            for (int i = 0; i < MC_VERIFY_MAX_LEN; i++) {
                const uint32_t d = (uint32_t)(tk[i] - (int32_t)t); // (-1: far above 8)
                if (d < 8) {
#pragma unroll
                    for (uint32_t j = 0; j < 8; j++) c[j] += j == d ? 1 : 0;
                }
            }
        }
        uint32_t bits = 0xFFu;
        if (masked) {
            const uint32_t sh = t & 31;
            bits = mr[t >> 5] >> sh;
            if (sh > 24) bits |= mr[(t >> 5) + 1] << (32 - sh); // (t + 7 < n lies in that word)
        }
#pragma unroll
        for (uint32_t j = 0; j < 4; j++) {
            const bf16_t a = logit_rule((bf16_t)(w[j] & 0xFFFFu), c[2 * j], (bits >> (2 * j)) & 1u, s);
            const bf16_t b = logit_rule((bf16_t)(w[j] >> 16), c[2 * j + 1], (bits >> (2 * j + 1)) & 1u, s);
            w[j] = (uint32_t)a | ((uint32_t)b << 16);
        }
        *reinterpret_cast<uint4*>(lr + t) = make_uint4(w[0], w[1], w[2], w[3]);
    }
    for (uint32_t e = 0; e < 2; e++)
        for (uint32_t t = (e ? vhi : lo) + tid; t < (e ? hi : vlo); t += LP_THREADS) {
            const int32_t c = pen ? cr[t] + v_path_hits(tk, t) : 0;
            const bool allowed = !masked || ((mr[t >> 5] >> (t & 31)) & 1u);
            lr[t] = logit_rule(lr[t], c, allowed, s);
        }
}
