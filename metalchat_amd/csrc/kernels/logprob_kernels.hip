// Row log-probabilities (mc_logprobs_*, include/metalchat_hip.h Part 2n): behind the pick, two launches give the log-probability of
// the token a row picked and of its top_n most likely tokens.  With y[0..n) the row's bfloat16 logits as the pick read them (after
// the row's mask and penalties, before temperature and truncation) the rule is (tests/logprob_rule.py, float64):
//   M     = max y
//   S     = sum over t of exp(double(y[t]) - double(M))        exp(-inf) = 0
//   lse   = double(M) + log(S)
//   lp[t] = float(double(y[t]) - lse)                           one rounding; a banned token's lp is -inf
//   top n = the n largest y in make_key's order (value descending, -0 == +0, then LOWER index), each with its lp
// -- the model's distribution over the processed logits at temperature 1, not the sampler's truncated nucleus.  exp, log, the sums
// and the last subtraction are evaluated in double (as exp_precise is, common.h), so only the order of the double sum separates a
// device result from the rule, and that moves a result across a float rounding boundary at most.
//   parts   grid (ceil(n / LOGPROB_CHUNK), R), LOGPROB_THREADS threads, the shape of mc_b_logits_process_*: a workgroup streams one
//           chunk of one row, 8 logits per thread from the chunk's first 16-byte boundary on with one 16-byte load, the (at most 7)
//           elements in front of that boundary and behind the last whole piece one to a thread.  It writes the chunk's maximum m_c,
//           s_c = sum exp(double(y) - double(m_c)) (0 for a chunk whose maximum is -inf: (-inf) - (-inf) is never formed) and the
//           chunk's top_n best keys, sorted: top_n rounds of a workgroup maximum over the keys below the last winner (a key holds
//           its index, so no two are equal).  A chunk shorter than top_n pads with 0, which is no key.
//   finish  grid (1, R), one workgroup per row: M = max m_c, S = sum of s_c * exp(double(m_c) - double(M)) in chunk order, lse, the
//           token's lp, then top_n rounds of a workgroup maximum over the row's nchunk * top_n chunk keys (<= LOGPROB_KEY_CAP, held
//           in registers; the host refuses more) and their lp.  The token and the slot come from rows[r] (a step or a packed pass:
//           rows[r].token is the pick, rows[r].step_index its slot, as the pick kernels index tokens_out) or, rows null, from
//           picks[r] and r (a verify call).
// The _rows forms: workgroups of idle rows (rows[r].pos < 0) exit after the scalar load of the row's state, before anything else is
// read or written.  No atomics, no workgroup waits for another, nothing in private memory.
#include "common.h"

using namespace mc;
using namespace mc::abi;

__device__ __forceinline__ uint64_t
logprob_wave_max(uint64_t k)
{
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) k = max((unsigned long long)k, (unsigned long long)__shfl_xor((unsigned long long)k, off, 64));
    return k;
}

// the largest key of the workgroup; wk: one slot per wave, the caller alternates two of them between rounds (one barrier a round)
__device__ __forceinline__ uint64_t
logprob_block_max(uint64_t k, unsigned long long* wk)
{
    k = logprob_wave_max(k);
    if ((threadIdx.x & 63) == 0) wk[threadIdx.x >> 6] = k;
    __syncthreads();
    return max(max(wk[0], wk[1]), max(wk[2], wk[3]));
}

__device__ __forceinline__ float
logprob_block_maxf(float m, float* wm)
{
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) m = fmaxf(m, __shfl_xor(m, off, 64));
    if ((threadIdx.x & 63) == 0) wm[threadIdx.x >> 6] = m;
    __syncthreads();
    return fmaxf(fmaxf(wm[0], wm[1]), fmaxf(wm[2], wm[3]));
}

__device__ __forceinline__ void
logprob_parts_body(const bf16_t* logits, uint32_t n, uint32_t top_n, logprob_part* parts, uint64_t* keys)
{
    __shared__ float wm[4];
    __shared__ double ws[4];
    __shared__ unsigned long long wk[2][4];
    const uint32_t r = blockIdx.y, c = blockIdx.x, tid = threadIdx.x;
    const uint32_t lo = c * LOGPROB_CHUNK;
    if (lo >= n) return; // (uniform)
    const bf16_t* lr = logits + (size_t)r * n;
    // the chunk [lo, hi), its whole 16-byte pieces [vlo, vhi)
    const uint32_t hi = min(n, lo + LOGPROB_CHUNK);
    const uint32_t head = min(hi - lo, (uint32_t)((16u - (uint32_t)((uintptr_t)(lr + lo) & 15u)) & 15u) / 2u);
    const uint32_t vlo = lo + head, nvec = (hi - vlo) / 8, vhi = vlo + 8 * nvec;

    // a thread's logits: 8 of a whole piece, one in front of the first piece, one behind the last; an empty place has key 0 and value -inf
    float v[10];
    uint64_t k[10];
#pragma unroll
    for (uint32_t j = 0; j < 10; j++) v[j] = -INFINITY, k[j] = 0;
    if (tid < nvec) {
        const uint32_t t = vlo + 8 * tid;
        const uint4 q = *reinterpret_cast<const uint4*>(lr + t);
        const uint32_t w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
        for (uint32_t j = 0; j < 4; j++) {
            v[2 * j] = bf2f((bf16_t)(w[j] & 0xFFFFu));
            v[2 * j + 1] = bf2f((bf16_t)(w[j] >> 16));
        }
#pragma unroll
        for (uint32_t j = 0; j < 8; j++) k[j] = make_key(v[j], t + j);
    }
    if (tid < head) {
        v[8] = bf2f(lr[lo + tid]);
        k[8] = make_key(v[8], lo + tid);
    }
    if (tid < hi - vhi) {
        v[9] = bf2f(lr[vhi + tid]);
        k[9] = make_key(v[9], vhi + tid);
    }

    float m = v[0];
#pragma unroll
    for (uint32_t j = 1; j < 10; j++) m = fmaxf(m, v[j]);
    m = logprob_block_maxf(m, wm);
    double s = 0.0;
    if (m > -INFINITY) { // (uniform)
        const double dm = (double)m;
#pragma unroll
        for (uint32_t j = 0; j < 10; j++) s += v[j] > -INFINITY ? exp((double)v[j] - dm) : 0.0;
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) s += __shfl_xor(s, off, 64);
        if ((tid & 63) == 0) ws[tid >> 6] = s;
        __syncthreads();
        s = ((ws[0] + ws[1]) + ws[2]) + ws[3];
    }
    if (tid == 0) {
        logprob_part p;
        p.s = s;
        p.m = m;
        p.pad = 0;
        parts[(size_t)r * gridDim.x + c] = p;
    }

    uint64_t* kr = keys + ((size_t)r * gridDim.x + c) * top_n;
    uint64_t prev = ~0ull;
    for (uint32_t i = 0; i < top_n; i++) {
        uint64_t best = 0;
#pragma unroll
        for (uint32_t j = 0; j < 10; j++) best = max((unsigned long long)best, (unsigned long long)(k[j] < prev ? k[j] : 0ull));
        best = logprob_block_max(best, wk[i & 1]);
        if (tid == 0) kr[i] = best;
        prev = best; // (0 once the chunk has run out: nothing lies below it)
    }
}

extern "C" __global__ void __launch_bounds__(LOGPROB_THREADS)
mc_logprob_parts_bfloat(const bf16_t* logits, uint32_t n, uint32_t top_n, logprob_part* parts, uint64_t* keys, const step_state* rows)
{
    logprob_parts_body(logits, n, top_n, parts, keys);
}

// ragged: rows[r].pos < 0 marks an idle row
extern "C" __global__ void __launch_bounds__(LOGPROB_THREADS)
mc_logprob_parts_rows_bfloat(const bf16_t* logits, uint32_t n, uint32_t top_n, logprob_part* parts, uint64_t* keys, const step_state* rows)
{
    if (rows[blockIdx.y].pos < 0) return; // (uniform)
    logprob_parts_body(logits, n, top_n, parts, keys);
}

__device__ __forceinline__ void
logprob_finish_body(const bf16_t* logits, uint32_t n, uint32_t top_n, uint32_t nchunk, const logprob_part* parts, const uint64_t* keys,
                    const step_state* rows, const int32_t* picks, uint32_t nslots, float* out_lp, int32_t* out_ids, float* out_top)
{
    __shared__ float wm[4];
    __shared__ double terms[LOGPROB_THREADS];
    __shared__ double lse_s;
    __shared__ unsigned long long wk[2][4];
    const uint32_t r = blockIdx.y, tid = threadIdx.x;
    const int32_t token = rows ? rows[r].token : picks[r];
    const uint32_t slot = rows ? (uint32_t)rows[r].step_index : r;
    if (slot >= nslots) return; // (uniform)
    const bf16_t* lr = logits + (size_t)r * n;

    float mc = -INFINITY;
    double sc = 0.0;
    if (tid < nchunk) {
        const logprob_part p = parts[(size_t)r * nchunk + tid];
        mc = p.m;
        sc = p.s;
    }
    const float M = logprob_block_maxf(mc, wm);
    terms[tid] = mc > -INFINITY ? sc * exp((double)mc - (double)M) : 0.0; // (a chunk whose maximum is -inf adds nothing)
    __syncthreads();
    if (tid == 0) {
        double S = 0.0;
        for (uint32_t c = 0; c < min(nchunk, LOGPROB_THREADS); c++) S += terms[c];
        lse_s = (double)M + log(S);
    }
    __syncthreads();
    const double lse = lse_s;
    if (tid == 0 && (uint32_t)token < n) out_lp[slot] = (float)((double)bf2f(lr[token]) - lse);

    const uint32_t total = min(nchunk * top_n, LOGPROB_KEY_CAP);
    const uint64_t* kr = keys + (size_t)r * nchunk * top_n;
    uint64_t k[LOGPROB_FINISH_KEYS];
#pragma unroll
    for (uint32_t j = 0; j < LOGPROB_FINISH_KEYS; j++) {
        const uint32_t i = tid + LOGPROB_THREADS * j;
        k[j] = i < total ? kr[i] : 0ull;
    }
    uint64_t prev = ~0ull, mine = 0;
    for (uint32_t i = 0; i < top_n; i++) {
        uint64_t best = 0;
#pragma unroll
        for (uint32_t j = 0; j < LOGPROB_FINISH_KEYS; j++) best = max((unsigned long long)best, (unsigned long long)(k[j] < prev ? k[j] : 0ull));
        best = logprob_block_max(best, wk[i & 1]);
        mine = tid == i ? best : mine;
        prev = best;
    }
    if (tid < top_n && mine != 0) {
        const uint32_t t = key_index(mine);
        if (t < n) {
            out_ids[(size_t)slot * top_n + tid] = (int32_t)t;
            out_top[(size_t)slot * top_n + tid] = (float)((double)bf2f(lr[t]) - lse);
        }
    }
}

extern "C" __global__ void __launch_bounds__(LOGPROB_THREADS)
mc_logprob_finish_bfloat(const bf16_t* logits, uint32_t n, uint32_t top_n, uint32_t nchunk, const logprob_part* parts, const uint64_t* keys,
                         const step_state* rows, const int32_t* picks, uint32_t nslots, float* out_lp, int32_t* out_ids, float* out_top)
{
    logprob_finish_body(logits, n, top_n, nchunk, parts, keys, rows, picks, nslots, out_lp, out_ids, out_top);
}

extern "C" __global__ void __launch_bounds__(LOGPROB_THREADS)
mc_logprob_finish_rows_bfloat(const bf16_t* logits, uint32_t n, uint32_t top_n, uint32_t nchunk, const logprob_part* parts, const uint64_t* keys,
                              const step_state* rows, const int32_t* picks, uint32_t nslots, float* out_lp, int32_t* out_ids, float* out_top)
{
    if (rows[blockIdx.y].pos < 0) return; // (uniform)
    logprob_finish_body(logits, n, top_n, nchunk, parts, keys, rows, picks, nslots, out_lp, out_ids, out_top);
}
