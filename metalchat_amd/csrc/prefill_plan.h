// What the prompt pass launches, decided without a device: which kernel family multiplies a prompt GEMM and with what tiles and K ranges (plan_gemm),
// which attention kernel a prompt of M rows takes and its packed / extend forms (plan_attention, plan_packed_attention, plan_extend_attention), the form
// and grid of the rope + cache write (plan_rope) and the predicates that fold a launch into its neighbour (act_epi_ok, fold_parts_ok, fold_norm_ok).
// Pure integer arithmetic over a linear's five shape fields, M, a few config words, the CU count, the MC_PF_* switches and one bool (lib_on) -- no HIP,
// no mc_decoder -- so the choices are pinned on the CPU, grids included (tests/cpp/test_prefill_plan.cc against tests/golden/prompt_plans.json and
// prompt_launch_logs.json).  prefill.cc launches what these say; everything that touches the device (the derived weight copies, the library GEMM, the
// scratch) stays there.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <string>

#include "../../include/metalchat_hip.h" // MC_WFMT_*, MC_QMODE_*, MC_FAMILY_*
#include "decoder_options.h"
#include "gemv_plan.h" // gemv_shape: the five fields of a linear_w

struct prefill_env { // of a decoder, fixed when it is created -- except lib_on
    int tb; // sizeof(T)
    int qmode, family;
    unsigned cus; // compute units of the device
    int dim, ffn_dim, n_heads, n_kv_heads, head_dim, max_seq_len;
    bool lib_on; // opt.pf_lib until the library fails (mc_decoder::pf_lib_on)
    const decoder_options* opt;
};

inline const char*
pf_tname(const prefill_env& e)
{
    return e.tb == 2 ? "bfloat" : "float";
}

// ---------------------------------------------------------------- the prompt GEMM: Y[M, L.out] = T(X[M, L.in] Wd^T) (+ res), the fused matrices of the decode GEMV

// the row tile of the big prompt GEMM at M rows, and the K splits it takes for this matrix (plan_gemm() below)
inline unsigned
gemm_row_tile(const prefill_env& e, int M)
{
    return e.tb == 2 && M >= 256 && !e.opt->pf_depth1 && !e.opt->pf_bm128 ? 256u : 128u;
}

inline unsigned
gemm_splits(const gemv_shape& L, const prefill_env& e, int M)
{
    const decoder_options& opt = *e.opt;
    const unsigned bm = gemm_row_tile(e, M);
    const unsigned tiles = ((L.out + 127) / 128) * ((M + bm - 1) / bm);
    const unsigned want = (bm == 256 ? 1u : 2u) * e.cus; // (256 rows: one 8-wave workgroup per CU)
    unsigned splits = 1;
    while (splits < 16 && tiles * splits < want && (unsigned)L.in / (splits * 2) >= 512) splits *= 2;
    // (round 4) ... but not past the point where the extra workgroups only start another round: 96 tiles on 256 CUs take one
    // round of K/2 at 2 splits and two rounds of K/4 at 4 -- the same time, with twice the partials written and read back
    // (MC_PF_SPLITS_OLD=1: the plain doubling rule)
    if (!opt.pf_splits_old && splits > 1) {
        auto rounds = [&](unsigned sp) { return (tiles * sp + want - 1) / want; };
        const unsigned half = splits / 2;
        if (rounds(splits) * half >= rounds(half) * splits) splits = half; // rounds(s)/s >= rounds(s/2)/(s/2)
    }
    return opt.pf_no_splitk ? 1u : splits;
}

// Short prompts (<= 64 rows) on int4 weights: the weight-streaming GEMM over the quad-interleaved copy (prefill_kernels.hip
// mc_pf2_gemm_i4_bfloat: matrix-pipe dequantisation straight into MFMA operands, no LDS image of W)
inline bool
pf2_ok(const gemv_shape& L, const prefill_env& e, int M)
{
    return e.opt->pf2_on && e.tb == 2 && L.fmt == MC_WFMT_I4 && e.qmode == MC_QMODE_EXACT && M <= 64 && L.group == 128 && L.in % 128 == 0 && L.in >= 256;
}

// K ranges of the weight-streaming GEMM: enough workgroups for the chip, at least two steps of 128 each
inline void
pf2_split(const gemv_shape& L, const prefill_env& e, unsigned& splits, unsigned& ktper)
{
    const unsigned nwg = ((unsigned)L.out + 127u) / 128u, KT = (unsigned)L.in / 128u;
    const unsigned target = e.cus * (unsigned)e.opt->pf2_wgs_per_cu;
    splits = std::max(1u, std::min(16u, (target + nwg - 1) / nwg));
    ktper = std::max(2u, (KT + splits - 1) / splits);
    splits = (KT + ktper - 1) / ktper;
}

// ---- the 256 x 256 ping-pong GEMM (round 5, kernels/pf_gemm8.h): bfloat16 rows, no adaptor, K in whole tiles of 64, scale groups
// of whole 16-runs; from opt.pf_g8_rows rows on (below that the 128-row tiles keep more workgroups busy)
inline bool
g8_ok(const gemv_shape& L, const prefill_env& e, int M)
{
    const decoder_options& opt = *e.opt;
    if (!opt.pf_g8_on || e.tb != 2 || L.lora_cols || M < opt.pf_g8_rows || opt.pf_small_gemm) return false;
    if (L.in % 64 != 0 || L.out % 4 != 0) return false;
    if (L.fmt != MC_WFMT_T && L.group && (L.group < 32 || (L.group & (L.group - 1)) != 0)) return false;
    if ((size_t)L.out * L.in * 2 > 0xFFFFFFFFull || (size_t)M * L.in * 2 > 0xFFFFFFFFull) return false; // (32-bit buffer offsets)
    return true;
}

// K ranges of a launch: one round of workgroups on the chip at most, eight K tiles per range at least
inline unsigned
g8_splits(const gemv_shape& L, const prefill_env& e, int M)
{
    const decoder_options& opt = *e.opt;
    const unsigned tiles = ((L.out + 255) / 256) * ((M + 255) / 256);
    unsigned splits = 1;
    while (splits < (unsigned)opt.pf_g8_max_splits && tiles * splits * 2 <= e.cus && (unsigned)L.in / 64u / (splits * 2) >= (unsigned)opt.pf_g8_min_ktiles) splits *= 2;
    return opt.pf_no_splitk ? 1u : splits;
}

// ---- the library GEMM of long prompts (prefill_blaslt.cc gemm_lib)
// Measured on MI355X (tools/blaslt_probe.py, profiles/r04_blaslt_probe.log; WBITS=16 tools/prefill_bench.py): the hand-written
// tiled GEMM reaches 600-725 TFLOP/s with AND without its dequantisation (plain bfloat weights: 180 us for w1|w3 at 512 rows
// against 168 with int4) -- its ceiling is the tile loop, not the exact arithmetic -- while hipBLASLt multiplies the same shapes
// at 1.1-1.36 PFLOP/s once a launch has >= 128 tiles of 256 x 256 and at 600-750 with 32-48 of them, where the split-K kernels
// here are as fast or faster.  The threshold was then swept on whole prompts of 256-1536 rows (profiles/r04_prefill_blaslt.log):
// 48 tiles is the best or equal at every length (w1|w3 from 256 rows on, wq|wk|wv from 512, every matrix of Llama-3-8B from 768).  The operand is Wd = T(T(q) T(s)), the very
// values the prompt kernels hold in LDS, kept as a bfloat16 copy [out][in] (2 bytes per weight more HBM: 14 GB for Llama-3-8B
// of 288); sums are fp32, rounded to T once (linear.h:70-81) -- only the order of the fp32 additions differs from the kernels'.
// Any failure of the library (absent, no algorithm, an error status) switches the path off (lib_on): the prompt kernels take over.
inline bool
lib_ok(const gemv_shape& L, const prefill_env& e, int M)
{
    const decoder_options& opt = *e.opt;
    if (!e.lib_on || e.tb != 2 || L.lora_cols || opt.pf_small_gemm) return false;
    if (L.fmt != MC_WFMT_T && (L.in % 16 != 0 || (L.group && (L.group & (L.group - 1)) != 0))) return false;
    if (L.in % 8 != 0 || L.out % 8 != 0) return false;
    if (opt.pf_lib_force) return true; // (MC_PF_BLASLT=2: every prompt GEMM that can, whatever its size -- how the tests reach it on small models)
    return M >= opt.pf_lib_rows && (size_t)((L.out + 255) / 256) * (size_t)((M + 255) / 256) >= (size_t)opt.pf_lib_tiles;
}

// ---- the prompt GEMM plan: which kernel family multiplies X[M][L.in] by this matrix, with what tiles and K ranges.  The one place that
// chooses: gemm_run() launches what it says, run_prefill() asks it about w1|w3.  epi: 0 store, 1 + residual, 2 stop at the fp32
// partial sums (gemm_to_parts), 3 / 4 silu / gelu * mul.  No launch, no allocation.
enum class gemm_family { lib, stream, g8, tiled, tile64 };
struct gemm_plan {
    gemm_family fam = gemm_family::tile64;
    unsigned bm = 64;                     // rows of X per workgroup
    unsigned splits = 1, ktper = 0;       // K ranges (grid z; lib: the one partial); stream: K steps of 128 per range
    unsigned gx = 0, gy = 0, block = 256; // the family's launch
    // what the kernel's name is made of besides the family
    int fmt = MC_WFMT_T, epi = 0, tb = 2;
    bool deep = false; // tiled: two K chunks in flight per workgroup (prefill_kernels.hip: measured best at every length); MC_PF_DEPTH=1
                       // selects the one-chunk build for A/B runs.  THE place that decides the _d2 suffix

    // does the launch leave fp32 partial sums for a reduce (or a consumer that adds them up) instead of T rows?
    bool
    writes_partials() const { return epi == 2 || splits > 1 || fam == gemm_family::stream; }
    // The kernel the plan implies: `parts` -- it writes fp32 partials (e2: no residual, no adaptor -- the reduce carries them), else T rows with
    // the caller's epilogue; `plain_copy` -- g8 over the dequantised bfloat16 copy of a quantised matrix (prefill.cc plain_copy_ok), THE place
    // that gives that launch its w_ name.  The library GEMM is no kernel of ours: "".
    std::string
    kernel(bool parts, bool plain_copy = false) const
    {
        const char* f = fmt == MC_WFMT_I4 ? "i4_" : (fmt == MC_WFMT_I8 ? "i8_" : "w_");
        const std::string t = tb == 2 ? "bfloat" : "float", e = "_e" + std::to_string(parts ? 2 : epi);
        switch (fam) {
        case gemm_family::lib: return "";
        case gemm_family::stream: return "mc_pf2_gemm_i4_" + t;
        case gemm_family::g8: return std::string("mc_pf_gemm8_") + (plain_copy ? "w_" : f) + "bfloat" + e;
        case gemm_family::tiled: return (bm == 256 ? "mc_pf_gemm256_" : "mc_pf_gemm128_") + (f + t) + (deep ? "_d2" : "") + e;
        case gemm_family::tile64: break;
        }
        return "mc_pf_gemm_" + (f + t) + e;
    }
};

inline gemm_plan
plan_gemm(const gemv_shape& L, const prefill_env& e, int M, int epi)
{
    // The families in priority order: the first whose gate holds multiplies.
    //   1. lib: hipBLASLt on the dequantised copy (lib_ok) -- a plain store (epi 0) or its fp32 sums as ONE partial (epi 2), nothing else
    //   2. stream: mc_pf2_gemm_i4_* (pf2_ok: int4, <= 64 rows; K ranges by pf2_split) -- no epilogue of its own, always through the reduce
    //   3. g8: the 256 x 256 ping-pong mc_pf_gemm8_* (g8_ok; K ranges by g8_splits) -- an activation epilogue (epi >= 3) does not split
    //   4. tiled: mc_pf_gemm{128,256}_* (row tile by gemm_row_tile, K ranges by gemm_splits) -- every other bfloat16 prompt: a short one
    //      is bound by the weight stream, and the unpipelined 64 x 64 tile needed 32-42 ms for 8-64 rows where this one needs 5
    //   5. tile64: mc_pf_gemm_* -- T = float (the parity path) and MC_PF_SMALL_GEMM=1; never splits
    gemm_plan P;
    P.fmt = L.fmt;
    P.epi = epi;
    P.tb = e.tb;
    const unsigned out = (unsigned)L.out;
    if ((epi == 0 || epi == 2) && lib_ok(L, e, M)) {
        P.fam = gemm_family::lib;
    } else if (pf2_ok(L, e, M)) {
        P.fam = gemm_family::stream;
        pf2_split(L, e, P.splits, P.ktper);
        P.gx = (out + 127u) / 128u;
        P.gy = 1;
        P.block = 512;
    } else if (g8_ok(L, e, M)) {
        P.fam = gemm_family::g8;
        P.bm = 256;
        P.splits = epi >= 3 ? 1u : g8_splits(L, e, M);
        P.gx = (out + 255u) / 256u;
        P.gy = ((unsigned)M + 255u) / 256u;
        P.block = 512;
    } else if (e.tb == 2 && !e.opt->pf_small_gemm) {
        // 256 rows of X per workgroup from 256 rows on (prefill_kernels.hip pf_gemm_big_body, BM): the W tile is dequantised once
        // per workgroup, and at 128 rows that vector work is ~ 0.8 of the matrix pipe's time
        // A 128 x 128 tile walks K serially (~1.5 us per 64-wide chunk), so a grid that does not
        // oversubscribe the CUs several times is latency-bound: split K until it does.
        P.fam = gemm_family::tiled;
        P.bm = gemm_row_tile(e, M);
        P.splits = gemm_splits(L, e, M);
        P.gx = (out + 127u) / 128u;
        P.gy = ((unsigned)M + P.bm - 1u) / P.bm;
        P.block = 2 * P.bm;
        P.deep = !e.opt->pf_depth1;
    } else {
        P.gx = (out + 63u) / 64u;
        P.gy = ((unsigned)M + 63u) / 64u;
    }
    return P;
}

// A prompt GEMM may stop at its fp32 partial sums for the kernel that consumes its rows (prefill.cc gemm_to_parts): bfloat16 rows, no adaptor
// (the reduce carries it), not the round-1 GEMM
inline bool
fold_parts_ok(const gemv_shape& L, const prefill_env& e)
{
    return e.opt->pf_fold_on && e.tb == 2 && !L.lora_cols && !e.opt->pf_small_gemm;
}

// Wo / w2 (prefill.cc gemm_residual): may the reduce of the split GEMM, the residual and the norm(s) behind it be one launch?
// gemma3's post norms (post_norm): the post norm with the residual and the next norm (prefill_kernels.hip mc_pf_rmsnorm2_parts_bfloat, which takes
// no next norm too; MC_PF_NORM2=0: the three launches).  llama: h = T(x + T(sum of the partials)), rmsnorm(h) -- only where a next norm follows
inline bool
fold_norm_ok(const prefill_env& e, bool post_norm, bool next_norm)
{
    const bool fits = e.dim % 8 == 0 && e.dim / 8 <= 4 * 256;
    return post_norm ? fits && e.tb == 2 && e.opt->pf_norm2 : fits && next_norm;
}

// silu(w1 x) * (w3 x) in the epilogue of an unsplit 256-row GEMM (prefill_kernels.hip pf_gemm_big_body EPI 3; the
// table of exponentials rides in `res`).  MC_PF_ACT_EPI=0: the separate launch
// (gemma: gelu from the table of round 6 -- the 256 x 256 GEMM's e4 epilogue only; without the table the separate launch with its fp64 tanh)
// p13: plan_gemm(w13, M, 0); gelu_table: the decoder holds the table (mc_decoder::pf_gtab)
inline bool
act_epi_ok(const gemv_shape& w13, const prefill_env& e, const gemm_plan& p13, bool gelu_table)
{
    const bool gemma = e.family == MC_FAMILY_GEMMA3;
    return e.opt->pf_act_epi && !w13.lora_cols && p13.splits == 1 &&
           (p13.fam == gemm_family::g8 ? e.ffn_dim % 2 == 0 && (!gemma || gelu_table)
                                       : p13.fam == gemm_family::tiled && !gemma && p13.bm == 256 && !e.opt->pf_depth1);
}

// ---------------------------------------------------------------- rope + cache write of the M rows behind wq|wk|wv (prefill.cc qkv_rope_cache)
// packed / tree: the rows are the chunks of several batch rows (mc_pp_*), chunks that are trees (mc_tv_*) -- the four-pair arithmetic whatever
// MC_PF_ROPE_PACK says (bit for bit the one-pair launch's).  v4: four rotation pairs per thread (prefill_kernels.hip pf_rope_cache_v4_body: a
// quarter of the waves of the one-pair launch, which is bound by the rate waves start at, and the transposed V cache written 16 slots at a
// time); MC_PF_ROPE_PACK=0: pair, the launch of rounds 1-5.  Each reads the GEMM's rows or, where it split K, its partial sums (`parts`).
enum class rope_form { packed, tree, v4, pair };
struct rope_plan {
    rope_form form;
    std::string name;
    unsigned gx, gy, block;
};
inline bool
rope_v4_ok(const prefill_env& e, bool qk_norm)
{
    const int hd = e.head_dim;
    return e.opt->pf_rope_pack && e.tb == 2 && hd % 8 == 0 && hd <= 2048 && 2048 % hd == 0 &&
           (!qk_norm || hd == 128 || hd == 256); // (q / k norms: the head sizes whose sum order the kernel reproduces)
}
// batch: 0 one prompt, 1 packed rows, 2 packed trees; qk_norm: the layer has a q or a k norm
inline rope_plan
plan_rope(const prefill_env& e, int M, bool parts, int batch, bool qk_norm)
{
    const unsigned H = (unsigned)e.n_heads, KV = (unsigned)e.n_kv_heads, hd = (unsigned)e.head_dim;
    if (!batch && !rope_v4_ok(e, qk_norm))
        return {rope_form::pair, std::string(parts ? "mc_pf_rope_cache_parts_" : "mc_pf_rope_cache_") + pf_tname(e), H + 2 * KV, (unsigned)M, hd / 2};
    const unsigned per = 2048u / hd; // heads of a row per workgroup of 256 threads
    const unsigned gx = ((H + KV) * (unsigned)M + per - 1) / per + KV * (((unsigned)M + 15u) / 16u); // q / k units, then v tiles of 16 rows
    if (batch == 2) return {rope_form::tree, parts ? "mc_tv_rope_cache_parts_bfloat" : "mc_tv_rope_cache_bfloat", gx, 1, 256};
    if (batch) return {rope_form::packed, parts ? "mc_pp_rope_cache_parts_bfloat" : "mc_pp_rope_cache_bfloat", gx, 1, 256};
    return {rope_form::v4, parts ? "mc_pf_rope_cache_parts_v4_bfloat" : "mc_pf_rope_cache_v4_bfloat", gx, 1, 256};
}

// ---------------------------------------------------------------- attention
struct attn_plan {
    std::string name;
    unsigned gx, gy, block;
};

// THE two-heads rule: two query heads of a kv head per workgroup where the grouping allows it: each K / V
// fragment is loaded once for both (MC_PF_ATTN_HEADS=1: one head per workgroup)
// (measured: 2048 rows 15.8 -> 14.0 ms, 512 rows 2.05 -> 1.56 ms per prompt; with too few
// workgroups to fill the chip -- 128 rows -- it loses, 0.46 -> 0.61 ms)
// row_tiles: the 16-row tiles of the launch (one prompt: of its M rows; packed rows: of all segments)
inline bool
attn_two_heads_fit(const prefill_env& e)
{
    return (e.n_heads / e.n_kv_heads) % 2 == 0 && e.head_dim <= 128;
}
inline bool
attn_two_heads(const prefill_env& e, unsigned row_tiles)
{
    const bool enough = row_tiles * (unsigned)(e.n_heads / 2) >= 2u * e.cus;
    return attn_two_heads_fit(e) && (e.opt->pf_attn_heads >= 0 ? e.opt->pf_attn_heads == 2 : enough);
}

// the fused attention launch of ONE prompt of M rows (the probabilities stay on chip): which kernel, its grid and block
inline attn_plan
plan_attention(const prefill_env& e, int M)
{
    const decoder_options& opt = *e.opt;
    const int H = e.n_heads, KV = e.n_kv_heads, hd = e.head_dim;
    const bool heads_given = opt.pf_attn_heads >= 0;
    const bool two = attn_two_heads(e, (unsigned)((M + 15) / 16));
    // four query heads per workgroup (head_dim 128, 360 registers: one workgroup per CU): at 1024 rows and more
    // the launch is bound by the K / V fragments its waves pull out of L2 (1.6 GB per layer at 2048 rows, ~ 6 TB/s),
    // and four heads per fragment halve them again: 2048 rows 44.5 -> 42.6 ms, 1024: 22.75 -> 22.3, 512: 11.8 -> 11.7
    const bool four = (H / KV) % 4 == 0 && hd == 128 &&
                      (heads_given ? opt.pf_attn_heads == 4 : (unsigned)((M + 15) / 16) * (unsigned)(H / 4) >= e.cus);
    // long prompts (round 5): K / V tiles through LDS, 32 rows x 4 heads per workgroup (prefill_kernels.hip pf_attn_lds_body)
    const bool eight = (H / KV) % 4 == 0 && hd == 128 && e.max_seq_len % 8 == 0 &&
                       (heads_given ? opt.pf_attn_heads == 8 : (opt.pf_attn8_on && M >= opt.pf_attn8_rows));
    // (row tiles of 32 rows, dealt in pairs -- tile x with tile (last - x): equal work under the causal mask -- when the
    //  pairs still cover the CUs; MC_PF_ATTN8_PAIR=0 / 1 forces either)
    const unsigned ntl = (unsigned)(M + 31) / 32u;
    const bool pair_given = opt.pf_attn8_pair >= 0;
    const bool pair = pair_given ? opt.pf_attn8_pair != 0 : ((ntl + 1u) / 2u) * (unsigned)(H / 4) >= e.cus;
    // head_dim 256 (round 6; Gemma-7B: a kv head per query head): the same K / V tiles through LDS for 64 rows of ONE head, four waves
    // (MC_PF_ATTN8_ROWS256: from how many rows; MC_PF_ATTN_HEADS=1: never)
    const bool eight256 = hd == 256 && e.max_seq_len % 8 == 0 && (heads_given ? opt.pf_attn_heads == 8 : (opt.pf_attn8_on && M >= opt.pf_attn8_rows256));
    if (eight256) {
        const unsigned ntl64 = (unsigned)(M + 63) / 64u;
        const bool pair64 = pair_given ? opt.pf_attn8_pair != 0 : ((ntl64 + 1u) / 2u) * (unsigned)H >= e.cus;
        return {"mc_pf_attn8_bfloat_hd256", pair64 ? (ntl64 + 1u) / 2u : ntl64, (unsigned)H, 256};
    }
    // head_dim 64 (round 6; TinyLlama-1.1B: 8 query heads per kv head, Llama-3.2-1B: 4): 8 heads x 16 rows or 4 heads x 32 rows per workgroup
    const unsigned nh64 = (H / KV) % 8 == 0 ? 8u : ((H / KV) % 4 == 0 ? 4u : 0u);
    const bool eight64 = hd == 64 && nh64 && e.max_seq_len % 8 == 0 && (heads_given ? opt.pf_attn_heads == 8 : (opt.pf_attn8_on && M >= opt.pf_attn8_rows64));
    if (eight64) {
        const unsigned rt64 = 128u / nh64, ntl = ((unsigned)M + rt64 - 1u) / rt64;
        const bool pr = pair_given ? opt.pf_attn8_pair != 0 : ((ntl + 1u) / 2u) * ((unsigned)H / nh64) >= e.cus;
        return {nh64 == 8 ? "mc_pf_attn8_bfloat_hd64_h8" : "mc_pf_attn8_bfloat_hd64_h4", pr ? (ntl + 1u) / 2u : ntl, (unsigned)H / nh64, 512};
    }
    if (eight) return {"mc_pf_attn8_bfloat_hd128", pair ? (ntl + 1u) / 2u : ntl, (unsigned)H / 4, 512};
    if (four) return {"mc_pf_attn4_bfloat_hd128", ((unsigned)M + 15) / 16, (unsigned)H / 4, 256};
    return {std::string(two ? "mc_pf_attn2_bfloat_hd" : "mc_pf_attn_bfloat_hd") + std::to_string(hd), ((unsigned)M + 15) / 16, (unsigned)(two ? H / 2 : H), 256};
}

// packed rows (mc_rows_prefill, kernels/packed_kernels.hip): one or two query heads per workgroup by the rule of one prompt, over the ntiles tiles
// of all segments; the LDS-tile and four-head forms have no packed counterpart (DESIGN.md "The packed prompt pass")
inline attn_plan
plan_packed_attention(const prefill_env& e, int ntiles)
{
    const bool two = attn_two_heads(e, (unsigned)ntiles);
    return {std::string(two ? "mc_pp_attn2_bfloat_hd" : "mc_pp_attn_bfloat_hd") + std::to_string(e.head_dim), (unsigned)ntiles,
            (unsigned)(two ? e.n_heads / 2 : e.n_heads), 256};
}

// chunks that see their context (mc_extend_rows, kernels/extend_kernels.hip): the exp sums of every key range, then p V over the ranges, then the
// ranges of a split tile added in order; two query heads of a kv head per workgroup wherever the grouping allows it (the ranges, not the row
// tiles, fill the chip).  Chunks that are trees (mc_tree_verify): the mc_tv_* forms of the first two.  Grids: (heads, ranges of the group) for
// sums and pv, (n_heads, ranges) for the reduce; 256 threads each.
struct extend_plan {
    std::string sums, pv, reduce;
    unsigned heads; // grid x of sums and pv
};
inline extend_plan
plan_extend_attention(const prefill_env& e, bool tree)
{
    const bool two = attn_two_heads_fit(e);
    const std::string sfx = std::string(two ? "2" : "") + "_bfloat_hd" + std::to_string(e.head_dim);
    return {(tree ? "mc_tv_sums" : "mc_px_sums") + sfx, (tree ? "mc_tv_pv" : "mc_px_pv") + sfx, "mc_px_reduce_bfloat_hd" + std::to_string(e.head_dim),
            (unsigned)(two ? e.n_heads / 2 : e.n_heads)};
}
