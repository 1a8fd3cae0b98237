// What the decode launches for the first half of one block -- from the row handed to the block to the finished attention row, or past Wo where the
// form holds it: plan_block().  Nine forms and five attention tails, chosen by integer arithmetic and string building on the layer's three linears, six
// fields of the model, what a decoder fixes when it is created (block_env: the GEMV environment, the range count, the occupancy answers), and two pieces
// of run-time state (block_state) -- no HIP, no mc_decoder, so the choice is pinned on the CPU, name, grid and flags included
// (tests/cpp/test_block_plan.cc against tests/golden/decode_block_plans.json).  plan_token() (token_plan.h) asks it once per block, with the pending
// post-norm it carries from block to block; mc_decoder::attn_launch() packs the arguments of the form it names.
#pragma once

#include <algorithm>
#include <cstdint>
#include <initializer_list>
#include <string>
#include <utility>

#include "../../include/metalchat_hip.h" // MC_WFMT_*, MC_FAMILY_*
#include "decoder_options.h"
#include "gemv_plan.h"

struct block_shape { // of a layer_w
    gemv_shape qkv, wo, w13;
};
struct block_model { // of a mc_decoder_config
    int family, n_heads, n_kv_heads, head_dim, dim, max_seq_len;
};
// co-resident workgroups per CU of the hand-off launches (the occupancy API's answer; -1: not asked yet)
struct block_occupancy {
    int fused = -1, wo = -1, wo_w = -1, wo_i8 = -1, wo_qkn = -1, qkv_qkn = -1, qkv_only = -1, wo_i4_wide = -1, w13 = -1;
};
struct block_env { // of a decoder: fixed when it is created, the occupancy answers by its first step (mc_decoder::query_occupancy)
    gemv_env g;
    int nsplit = 1;        // 64-slot ranges of the cache
    int n_own = 0;         // blocks of this stage
    bool granules = false; // the granule buffers of the in-launch hand-offs exist (bfloat rows only, all or none: mc_decoder_create)
    int pv_ranges = 1;     // ranges of the P.V launch where its sums are reduced by their own launch
    std::string tname;     // "bfloat" / "float"
    block_occupancy occ;
};
struct block_state { // what changes between tokens
    bool attn_fused_on; // opt.attn_fused, until a hand-off gives up (mc_decoder::handoff_failed) and again after rearm_after clean tokens
    bool pending_pn;    // gemma3: a post-norm is left to the next pre-norm GEMV
};

// Computed per layer per eager step: the fall-back latch (handoff_failed), the re-arm (note_clean_tokens), taps and a late occupancy answer all change
// it between tokens.
enum class block_form { // (by the numbers of plan_block's list)
    qkv_wo_w13_w, qkv_wo_w, qkv_wo_i8, qkv_wo_i4 /* 4, 5 */, qkv_only, qkv_wo_qkn /* 8 */,
    wo_qkn, wo_i4, fused, fused_qkn, fused_t2, scores_pv // 7, 9 -- wq|wk|wv as a GEMV -- by their attention tail a - e
};
struct block_plan {
    block_form form = block_form::scores_pv;
    std::string name;     // the kernel of the form's attention launch
    int tiles = 1, vsh = 0, ns = 1; // 64-slot tiles per range; log2 of the virtual kv heads per cache head (kv_virtual_shift); ranges per kv head: nsplit / tiles
    unsigned grid = 0;    // workgroups of that launch
    uint32_t fast = 0;    // its `fastpath` argument (handoff.h)
    int chain_f = 0, chain_p = 0; // qkv_wo_w13_w: pairs per fetcher wave, most pairs of a poller wave
    bool qkv_gemv = false, rope_kv = false; // wq|wk|wv is a GEMV in front of the launch (7, 9); ... and gemma3's q/k-norm + rope + cache write a launch of their own (mc_rope_kv_T) behind it
    bool wo_gemv = false, pv_fold = false;  // Wo is a GEMV behind the launch; ... whose prologue adds the range sums of P.V (pv_fold)
    // scores_pv only: the P.V launch behind the scores -- its ranges of cache slots (grid z), its workgroup, and whether mc_attn_pv_reduce_T follows
    int pv_ranges = 0;
    unsigned pv_block = 0;
    bool pv_reduce = false;
};

// The gates every launch with an in-launch hand-off shares: the switch (MC_ATTN_FUSED, and the latch of handoff_failed), bfloat rows -- the granule
// buffers attn_psum_g / attn_slab_g / attn_row_g / attn_qkv_g / attn_hid_g exist for them only, all or none (mc_decoder_create) -- and layer tags of one byte
inline bool
handoffs_ok(const block_env& e, const block_state& st) { return st.attn_fused_on && e.granules && e.g.tb == 2 && e.n_own <= 254; }
// 256-thread attention workgroups per CU that may wait for one another.
// Co-residency from what a CU can HOLD of the real kernel (hipModuleOccupancyMaxActiveBlocksPerMultiprocessor, asked once:
// query_occupancy), capped by what was measured to pay (opt.attn_fused_max_wgs_per_cu).  The API is advisory (ROCm 7.2 reads
// one block per CU high for SGPR-heavy 256-thread kernels, MI355X_MICROARCH.md), and another stream can take CUs away
// at any time: a launch that is not resident after all gives up and the host falls back (handoff_failed).
inline unsigned
fused_wgs_per_cu(const block_env& e)
{
    const unsigned most = e.g.opt->attn_fused_max_wgs_per_cu;
    return std::min(most, e.occ.fused < 0 ? most : (unsigned)e.occ.fused);
}
// scores + softmax + P.V in one launch: bfloat rows, layer tags of one byte, and a grid that is certainly co-resident (its
// workgroups wait for one another) and gathers from few producers: at most opt.attn_fused_max_wgs_per_cu 256-thread workgroups
// of 64 cache slots per CU
inline bool
attn_fused(const block_model& m, const block_env& e, const block_state& st)
{
    return handoffs_ok(e, st) && (unsigned)(e.nsplit * m.n_kv_heads) <= fused_wgs_per_cu(e) * e.g.cus;
}
// ... with 128-slot ranges (mc_attn_fused_t2_bfloat: two score tiles per wave) where the 64-slot ranges are too many workgroups to
// be resident together -- Llama-3-8B at S = 8192: 1024 -> 512.  Round 3 measured that form at 14.8 us against 6.3 + 8.5 for
// the two launches; with the XCD-local hand-offs of round 4 it is re-measured (MC_ATTN_T2)
inline bool
attn_fused_t2(const block_model& m, const block_env& e, const block_state& st)
{
    return e.g.opt->attn_t2_on && handoffs_ok(e, st) && !attn_fused(m, e, st) && e.nsplit % 2 == 0 && (m.head_dim == 128 || m.head_dim == 64) &&
           m.n_kv_heads % 8 == 0 && (unsigned)(e.nsplit / 2 * m.n_kv_heads) <= fused_wgs_per_cu(e) * e.g.cus;
}
// Does this decoder take launches with in-launch hand-offs now?  What the retry paths ask (mc_decoder_step, mc_decoder_generate: the state in front of
// a step is kept where its hand-offs may give up) and what every form of plan_block but scores_pv implies (pinned by tests/test_block_plan_cpu.py).
inline bool
block_uses_handoffs(const block_model& m, const block_env& e, const block_state& st) { return attn_fused(m, e, st) || attn_fused_t2(m, e, st); }

// The XCD-local fast path of hand-offs A / B / Q (handoff.h) pays where the workgroups of one kv head CAN share an XCD: they
// are the blocks b with equal b % n_kv, blocks with equal b % 8 share an XCD, so n_kv must be a multiple of 8.  With
// TinyLlama's 4 kv heads half of every head's ranges sit on another XCD and are found only by the occasional look at the
// fabric copy: mc_attn_fused_bfloat 24.1 us against 7.0 without the fast path (profiles/r04_kernel_stats_tinyllama_fastpath_regression.csv)
inline bool
handoff_fast_here(const block_model& m, const block_env& e) { return e.g.opt->handoff_fast && m.n_kv_heads % 8 == 0; }
// ... and for the launches that are the attention ALONE (mc_attn_fused_T: no GEMV phase that needs every workgroup of the
// grid) any other head count is dealt with a stride of the next multiple of 8 -- bit 1 of the kernel's `fastpath` argument; the
// grid is nsplit x that stride and the workgroups without a head leave at once -- when the heads that then share an XCD
// still fit its CUs
inline uint32_t
handoff_mode_alone(const block_model& m, const block_env& e)
{
    if (!e.g.opt->handoff_fast) return 0u;
    const unsigned KV = (unsigned)m.n_kv_heads;
    if (KV % 8u == 0u) return 1u;
    const bool fits = (unsigned)e.nsplit * ((KV + 7u) / 8u) <= fused_wgs_per_cu(e) * e.g.cus / 8u;
    return fits ? 3u : 0u;
}

// VIRTUAL kv heads of the launches with wq|wk|wv inside (decode_kernels.hip attn_fused_bf, kv_shift): a model with 1, 2 or 4 kv heads is
// launched as 8 heads of n_rep / (8 / KV) query heads each, 8 / KV of them on one cache head -- a workgroup on every CU, a virtual
// head's ranges on one XCD.  Returns log2 of the heads per cache head (0: the real heads).
inline int
kv_virtual_shift(const block_model& m, const block_env& e)
{
    const int KV = m.n_kv_heads, n_rep = m.n_heads / KV;
    if (!e.g.opt->kv_virtual_on || KV >= 8 || 8 % KV != 0 || n_rep % (8 / KV) != 0) return 0;
    return KV == 4 ? 1 : (KV == 2 ? 2 : 3);
}

// The row-pair deal of the launches with wq|wk|wv inside: a kv head's (n_rep + 2) hd / 2 row pairs of wq|wk|wv (its query heads' rows, its K and
// its V row) go evenly over the head's `ns` workgroups, at most `cap` to each
inline bool
deal_ok(int pg, int ns, int cap) { return pg % ns == 0 && pg / ns <= cap; }

// The fewest 64-slot tiles per range among `cands` with WHOLE ranges (nsplit / t of them per head, `heads` heads) on at most one workgroup per
// CU that `ok(t, ns, grid)` takes; 0 = none.
// (wide ranges of a cache that is not whole ranges long -- S = 4040 -- would leave a ragged last range: refused here; the form such a
//  context takes instead is pinned by tests/test_context_gpu.py::test_contexts_of_partial_ranges_against_the_oracle_and_the_form_they_take.
//  64-slot ranges with a short last one are taken: tests/test_attn_kernels_gpu.py runs them at S = 2040)
template <typename F> inline int
whole_range_tiles(const block_model& m, const block_env& e, std::initializer_list<int> cands, int heads, F&& ok)
{
    for (int t : cands) {
        if (e.nsplit % t || (t > 1 && m.max_seq_len % (64 * t))) continue;
        const int ns = e.nsplit / t;
        const unsigned grid = (unsigned)(ns * heads);
        if (grid <= e.g.cus && ok(t, ns, grid)) return t;
    }
    return 0;
}

// P.V over four ranges of cache slots (256 workgroups instead of 64: a CU takes in ~ 25 GB/s, and 64 of them need
// ~ 4 us for the V cache of one layer at S = 2048) with the range sums added by the Wo GEMV's prologue (gemv.h
// PRO_PARTS) instead of a reduce launch
inline bool
pv_fold(const gemv_shape& wo, const block_model& m, const block_env& e)
{
    return e.g.opt->pv_fold_on && (lin_ok(wo, e.g) || ling_kib(wo, e.g)) && !wo.lora_cols && m.max_seq_len <= 16384;
}

// ... with the Wo GEMV and its residual in the same launch (attn_block_kernels.hip): int4 weights on bfloat rows with scale
// groups of whole lane blocks, K = H * hd of 1 or 2 KiB per row in one of the built (head_dim, K) pairs, no adaptor, at
// most two row pairs per wave of the launch
inline bool
attn_wo_fused(const gemv_shape& wo, const block_model& m, const block_env& e, const block_state& st)
{
    const decoder_options& opt = *e.g.opt;
    if (!opt.attn_wo_on || !attn_fused(m, e, st) || e.occ.wo == 0 || !lin_ok(wo, e.g) || wo.lora_cols || wo.out % 2 != 0) return false;
    const int hd = m.head_dim, k = wo.in / 2048;
    // (K = 8192, Llama-3-70B: measured slower than the two launches -- attn_block_kernels.hip)
    const bool built = (hd == 128 && k == 2) || (hd == 64 && k == 1) || (hd == 256 && k == 2) || (hd == 128 && k == 4 && opt.attn_wo_k4);
    // (one 512-thread workgroup per CU: the kernels hold up to 132 VGPRs, two such workgroups would not be resident together)
    return built && wo.in == m.n_heads * hd && (unsigned)wo.out / 2 <= 2u * 8u * (unsigned)(e.nsplit * m.n_kv_heads) &&
           (unsigned)(e.nsplit * m.n_kv_heads) <= e.g.cus;
}

// ffn_norm + w1|w3 + act*mul as the next phase of the plain-weight block's launch (round 6, mc_attn_qkv_wo_w13_w_bfloat_hd64_k4_q4_f{3p3,4p4}, attn_block_kernels.hip):
// behind the Wo phase half the waves of every workgroup fetch w1|w3 row pairs into registers while the other half waits for the hidden row.
// For that block with 64-slot ranges on `grid` workgroups: exactly one workgroup per CU, w1|w3 plain bfloat with K = 2048, no adaptor.
// Returns 10 F + P (pairs per fetcher wave, most pairs of a poller wave), 0 = no.
inline int
chain_w13_fetch(const gemv_shape& w13, const block_model& m, const block_env& e, unsigned grid)
{
    const decoder_options& opt = *e.g.opt;
    if (!opt.chain_w13_on || e.occ.w13 <= 0 || w13.fmt != MC_WFMT_T || w13.lora_cols) return 0;
    if (m.dim != 2048 || w13.in != 2048 || w13.out % 2 || grid != e.g.cus || opt.lin_waves != 8) return 0;
    const unsigned nb = ((unsigned)w13.out / 2 + grid - 1) / grid; // pairs of the fullest workgroup
    // (the fetchers F each, the pollers the rest, at most P each.  Returns 10 F + P.)
    unsigned f = nb <= 24u ? 3u : 4u;
    if (opt.chain_f >= 0) f = (unsigned)opt.chain_f; // (MC_CHAIN_F)
    if (f < 1u || 4u * f > nb) return 0;
    const unsigned p_ = (nb - 4u * f + 3u) / 4u; // the fullest poller
    // built: f3p3 (22 pairs per workgroup: TinyLlama) and f4p4 (32: Llama-3.2-1B) -- the even deals, the measured best (attn_block_kernels.hip)
    const unsigned pcap = f == 3u ? 3u : (f == 4u ? 4u : 0u);
    return pcap && p_ <= pcap ? (int)(10u * f + pcap) : 0;
}

inline block_plan
plan_block(const block_shape& L, const block_model& m, const block_env& e, const block_state& st)
{
    // The forms in priority order: the first whose conditions hold is the block's.
    //   1. plain weights, the whole chain: mc_attn_qkv_wo_w13_w_* (only where form 2 has 64-slot ranges)
    //   2. mc_attn_qkv_wo_w_* (_t2 / _t4)
    //   3. mc_attn_qkv_wo_i8_*_t{1,2,4}
    //   4. mc_attn_qkv_wo_i4_*
    //   5. ... with wide ranges, _t{2,4}
    //   6. llama only: mc_attn_qkv_i4_*_hd128_q4, then Wo as a GEMV
    //   7. llama: the wq|wk|wv GEMV with the rope epilogue (p1_e4), then an attention tail
    //   8. gemma3: mc_attn_qkv_wo_qkn_*_p{1,2}_t*
    //   9. gemma3: the wq|wk|wv GEMV (p2_e0 while a post-norm is pending, else p1_e0), then an attention tail
    // The attention tails of 7 and 9:
    //   a. mc_attn_wo_qkn_* (gemma3, head_dim 256)
    //   b. mc_attn_wo_i4_*
    //   c. mc_attn_fused (_qkn where gemma3's norms go inside, otherwise behind mc_rope_kv)
    //   d. mc_attn_fused_t2
    //   e. scores + P.V, the range sums folded into Wo's prologue or reduced by their own launch
    // 1 - 5 and 8 end behind Wo (llama: + residual, in `hidden`; gemma3: in `proj`), so do a and b; the others leave the attention row to a Wo GEMV.
    const decoder_options& opt = *e.g.opt;
    const std::string& tname = e.tname;
    const int nsplit = e.nsplit;
    const bool gemma = m.family == MC_FAMILY_GEMMA3;
    const int H = m.n_heads, KV = m.n_kv_heads, hd = m.head_dim, n_rep = H / KV;
    const int pg = (n_rep + 2) * hd / 2; // row pairs of wq|wk|wv per kv head (deal_ok)
    const gemv_shape &qkv = L.qkv, &wo = L.wo;
    // ---- the shared gates
    const bool fused = attn_fused(m, e, st); // (implies handoffs_ok)
    const bool qkv_rows_ok = qkv.out == (H + 2 * KV) * hd, wo_rows_ok = wo.in == H * hd && wo.out % 2 == 0;
    // wq|wk|wv AND Wo inside the attention launch (1 - 5): both switches, no adaptor on either matrix, llama
    const bool qkv_wo_in = handoffs_ok(e, st) && opt.attn_qkv_on && opt.attn_wo_on && !gemma && !qkv.lora_cols && !wo.lora_cols && qkv_rows_ok && wo_rows_ok;
    // ... int4, the built shape (Llama-3-8B: rows of 2 KiB, mc_attn_qkv_wo_i4_bfloat_hd128_k2_q2*)
    const bool i4_shape = lin_ok(wo, e.g) && lin_ok(qkv, e.g) && hd == 128 && wo.in == 4096 && qkv.in == 4096 && qkv.group == wo.group && n_rep <= 16;
    auto tiles_of = [&](std::initializer_list<int> cands, int heads, auto&& ok) { return whole_range_tiles(m, e, cands, heads, ok); };
    block_plan P;
    // (the name is built by the arm that returns, and moved: no string is made for a form that is not taken)
    auto one_launch = [&](block_form form, int tiles, int vsh, std::string name) -> block_plan&& {
        P.form = form;
        P.name = std::move(name);
        P.tiles = tiles;
        P.vsh = vsh;
        P.ns = nsplit / tiles;
        P.grid = (unsigned)(P.ns * (KV << vsh));
        P.fast = (vsh ? opt.handoff_fast : handoff_fast_here(m, e)) ? 1u : 0u;
        return std::move(P);
    };

    // 1, 2: PLAIN bfloat weights (mc_attn_qkv_wo_w_bfloat_hd64_k4_q4: Llama-3.2-1B, the reference's default model): rows of 4 KiB (K = 2048), at most
    // ONE row pair per wave in either GEMV phase; fewer than 8 kv heads are launched as 8 virtual ones.  64-slot ranges (S <= 2048) or, round 5, 128- / 256-slot
    // ranges at S = 4096 / 8192 (_t{2,4}; they share MC_ATTN_I4_WIDE with the int4 form)
    if (qkv_wo_in && qkv.fmt == MC_WFMT_T && wo.fmt == MC_WFMT_T && e.occ.wo_w != 0 && hd == 64 && wo.in == 2048 && qkv.in == 2048) {
        const int vsh = kv_virtual_shift(m, e), pgv = ((n_rep >> vsh) + 2) * hd / 2;
        const int t = (n_rep >> vsh) > 16 || pgv < 64 || pgv > 512 ? 0 : tiles_of({1, 2, 4}, KV << vsh, [&](int t_, int ns, unsigned grid) {
            return (t_ == 1 ? fused : opt.attn_i4_wide_on) && deal_ok(pgv, ns, 8) && (unsigned)wo.out / 2 <= 8u * grid;
        });
        const int chain = t == 1 ? chain_w13_fetch(L.w13, m, e, (unsigned)(nsplit * (KV << vsh))) : 0;
        if (chain) {
            P.chain_f = chain / 10;
            P.chain_p = chain % 10;
            return one_launch(block_form::qkv_wo_w13_w, 1, vsh, "mc_attn_qkv_wo_w13_w_bfloat_hd64_k4_q4_f" + std::to_string(P.chain_f) + "p" + std::to_string(P.chain_p));
        }
        if (t) return one_launch(block_form::qkv_wo_w, t, vsh, std::string("mc_attn_qkv_wo_w_bfloat_hd64_k4_q4") + (t > 1 ? "_t" + std::to_string(t) : std::string()));
    }
    // 3: INT8 weights (round 5, mc_attn_qkv_wo_i8_bfloat_hd128_k4_q4_t{1,4}: Llama-3-8B int8): rows of 4 KiB (K = 4096),
    // one 512-thread workgroup per CU -- 64-slot ranges up to S = 2048 (t1), 256-slot ranges at S = 8192 (t4: 32 ranges x 8 kv heads)
    if (qkv_wo_in && opt.attn_i8_on && qkv.fmt == MC_WFMT_I8 && wo.fmt == MC_WFMT_I8 && e.occ.wo_i8 != 0) {
        auto group_ok = [](const gemv_shape& W) { return W.group == 0 || (W.group >= 16 && (W.group & (W.group - 1)) == 0); };
        const bool built = group_ok(qkv) && group_ok(wo) && qkv.group == wo.group && hd == 128 && wo.in == 4096 && qkv.in == 4096 && KV % 8 == 0 && n_rep <= 16;
        const int t = !built ? 0 : tiles_of({1, 2, 4}, KV, [&](int, int ns, unsigned grid) {
            return deal_ok(pg, ns, 16) && (unsigned)wo.out / 2 <= 8u * grid;
        });
        if (t) return one_launch(block_form::qkv_wo_i8, t, 0, "mc_attn_qkv_wo_i8_bfloat_hd128_k4_q4_t" + std::to_string(t));
    }
    if (qkv_wo_in && i4_shape) {
        auto name = [&] { return "mc_attn_qkv_wo_i4_" + tname + "_hd128_k" + std::to_string(wo.in / 2048) + "_q" + std::to_string(qkv.in / 2048); };
        // 4: INT4 (attn_block_kernels.hip qkv_in_launch): where Wo goes into the launch of 64-slot ranges (attn_wo_fused), the kv head's row pairs
        // dealt over its nsplit workgroups, at most two per wave
        if (attn_wo_fused(wo, m, e, st) && deal_ok(pg, nsplit, 16) && pg >= 64 && pg <= 512) return one_launch(block_form::qkv_wo_i4, 1, 0, name());
        // 5: ... with WIDE ranges (round 5, mc_attn_qkv_wo_i4_bfloat_hd128_k2_q2_t{2,4}): contexts whose 64-slot ranges are more workgroups
        // than CUs -- Llama-3-8B at S = 4096 / 8192 -- as 128- / 256-slot ranges, one 512-thread workgroup per CU
        const int t = !opt.attn_i4_wide_on || e.occ.wo_i4_wide == 0 || KV % 8 != 0 ? 0 : tiles_of({2, 4}, KV, [&](int, int ns, unsigned grid) {
            return deal_ok(pg, ns, 16) && pg >= 64 && (unsigned)wo.out / 2 <= 16u * grid;
        });
        if (t) return one_launch(block_form::qkv_wo_i4, t, 0, name() + "_t" + std::to_string(t));
    }
    // 6: wq|wk|wv in the launch WITHOUT Wo (round 5, mc_attn_qkv_i4_bfloat_hd128_q4: Llama-3-70B -- its Wo rows of 4 KiB stay a GEMV, attn_wo_fused): rows of
    // 4 KiB for wq|wk|wv too (K = 8192), up to three pairs per wave, the kv head's pairs gathered in two passes of 512.  MC_ATTN_QKV_ONLY=1 only.
    if (!gemma && fused && opt.attn_qkv_on && opt.attn_qkv_only_on && e.occ.qkv_only != 0 && lin_ok(qkv, e.g) && !qkv.lora_cols && qkv_rows_ok && qkv.in == 8192 &&
        m.dim == 8192 && hd == 128 && KV % 8 == 0 && (unsigned)(nsplit * KV) <= e.g.cus && n_rep <= 16 && pg <= 1024 &&
        deal_ok(pg, nsplit, 24) && pg / nsplit >= 8) {
        P.wo_gemv = true;
        return one_launch(block_form::qkv_only, 1, 0, "mc_attn_qkv_i4_" + tname + "_hd128_q4");
    }
    // gemma3 (round 5): q_norm / k_norm + rotation + cache write + attention + Wo in ONE launch from the raw wq|wk|wv rows
    // (mc_attn_wo_qkn_i4_bfloat_hd256_k2_t{1,2,4}: one 512-thread workgroup per CU, whole ranges of 64, 128 or 256 slots -- S = 1024, 2048, 4096 at
    // Gemma-7B's 16 kv heads, 16 x 16 workgroups at S = 2048)
    int qkn_tiles = 0;
    if (gemma && handoffs_ok(e, st) && opt.attn_wo_qkn_on && opt.attn_wo_on && opt.attn_qkn_on && hd == 256 && e.occ.wo_qkn != 0 && lin_ok(wo, e.g) && !wo.lora_cols &&
        wo_rows_ok && wo.in == 4096 && n_rep <= 16)
        qkn_tiles = tiles_of({1, 2, 4}, KV, [&](int t_, int, unsigned grid) {
            return (t_ > 1 || m.max_seq_len % 64 == 0) && (unsigned)wo.out / 2 <= 2u * 8u * grid;
        });
    // 8: ... with wq|wk|wv and the block's norms in the launch too (mc_attn_qkv_wo_qkn_i4_bfloat_hd256_k2_p{1,2}_t*, attn_block_kernels.hip
    // qkv_qkn_in_launch): rows of 1.5 KiB (K = 3072), the kv head's rotation pairs dealt evenly over its ranges, at most three per wave, one thread
    // per pair in the hand-off.  _p2: the previous block's ffn post-norm + residual is its prologue.
    if (qkn_tiles && opt.attn_qkv_qkn_on && opt.attn_qkv_on && e.occ.qkv_qkn != 0 && lin_split_ok(qkv, e.g) && !qkv.lora_cols && qkv.in == 3072 && m.dim == 3072 &&
        qkv.group == wo.group && qkv_rows_ok && pg <= 512 && deal_ok(pg, nsplit / qkn_tiles, 24))
        return one_launch(block_form::qkv_wo_qkn, qkn_tiles, 0,
                          "mc_attn_qkv_wo_qkn_i4_" + tname + "_hd256_k2_p" + (st.pending_pn ? "2" : "1") + "_t" + std::to_string(qkn_tiles));

    // 7, 9: wq|wk|wv as a GEMV, then the tail
    P.qkv_gemv = true;
    if (qkn_tiles) return one_launch(block_form::wo_qkn, qkn_tiles, 0, "mc_attn_wo_qkn_i4_" + tname + "_hd256_k2_t" + std::to_string(qkn_tiles)); // a
    // (gemma3 normalises q and k per head before the rotation, attention.h:174-175: that needs whole heads, so rope + cache write are a launch of
    //  their own -- except inside the one-launch attention where that is what follows: mc_attn_fused_qkn_bfloat, decode_kernels.hip q_from_qkv_rows)
    P.rope_kv = gemma;
    if (attn_wo_fused(wo, m, e, st)) return one_launch(block_form::wo_i4, 1, 0, "mc_attn_wo_i4_" + tname + "_hd" + std::to_string(hd) + "_k" + std::to_string(wo.in / 2048)); // b
    P.wo_gemv = true;
    if (fused) { // c
        if (gemma && opt.attn_qkn_on && (hd == 128 || hd == 256)) {
            P.rope_kv = false;
            return one_launch(block_form::fused_qkn, 1, 0, "mc_attn_fused_qkn_" + tname);
        }
        one_launch(block_form::fused, 1, 0, "mc_attn_fused_" + tname);
        P.fast = handoff_mode_alone(m, e);
        P.grid = (unsigned)nsplit * ((P.fast & 2u) ? ((unsigned)KV + 7u) & ~7u : (unsigned)KV);
        return P;
    }
    if (attn_fused_t2(m, e, st)) { // d
        one_launch(block_form::fused_t2, 2, 0, "mc_attn_fused_t2_" + tname);
        P.fast = opt.handoff_fast ? 1u : 0u;
        return P;
    }
    P.form = block_form::scores_pv; // e
    P.name = "mc_attn_scores_" + tname;
    P.pv_fold = pv_fold(wo, m, e);
    // softmax normalisation + P.V: folded, four ranges of one round of loads per wave (four k-steps of 32 slots each) and no reduce launch
    const int fold_waves = std::max(4, std::min(16, ((m.max_seq_len + 31) / 32 / 4 + 3) / 4));
    P.pv_ranges = P.pv_fold ? 4 : e.pv_ranges;
    P.pv_block = P.pv_fold ? 64u * (unsigned)fold_waves : (unsigned)opt.pv_block;
    P.pv_reduce = P.pv_ranges > 1 && !P.pv_fold;
    return P;
}
