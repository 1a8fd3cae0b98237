// What the decode launches for ONE token of one sequence (mc_decoder_step, mc_decoder_generate, a pipeline stage's token), in order: plan_token().
// The embed, every block -- plan_block's attention launch between the GEMVs plan_gemv names -- gemma3's post-norms, folded into the next pre-norm
// launch or rows of their own, the taps, the head and the pick's one to three launches.  Operands are SYMBOLIC (token_row, token_res, token_norm): no
// HIP, no mc_decoder, no device pointer, so the whole sequence is pinned on the CPU (tests/cpp/test_token_plan.cc against
// tests/golden/decode_token_plans.json).  mc_decoder::run_token() binds pointers to the symbols, packs each kernel's arguments and decides nothing.
#pragma once

#include <string>
#include <utility>
#include <vector>

#include "block_plan.h"
#include "gemv_plan.h"
#include "sampler_plan.h"

enum class token_op {
    park_row, embed, qkv_gemv, rope_kv, attn, scores, pv, pv_reduce, wo_gemv, post_norm_attn, w13_gemv, w2_gemv, post_norm_ffn, tap,
    head_gemv, fold_pick, argmax, candidates, sample
};
// the rows of a decoder's arena a step reads (x) and writes (y); `in` is the caller's inbound row of a later pipeline stage
enum class token_row { none, in, hidden, hidden_b, proj, qkv, q_rot, gate, attn_out, pv_parts, logits };
// a GEMV's `res` argument: a row to add, the layer's rope + cache-write descriptor (EPI 4), a post-norm descriptor of `res_layer` (PRO 2; the attention
// launches whose prologue applies one carry it too), or one of the pick's two descriptors (EPI 5)
enum class token_res { none, row, qkv_epi, pn_attn, pn_ffn, pick_atomic, pick_per_wg };
enum class token_norm { none, attention, ffn, final };

// ---------------------------------------------------------------- the ONE table: which (prologue, epilogue), norm weight and `res` a decode GEMV takes
enum class gemv_role { qkv, wo, w13, w2, head };
struct gemv_use {
    int pro, epi;
    token_norm norm;
    token_res res;
};
// behind_pn: gemma3's folded post-norm in front of this GEMV is its prologue (PRO 2) -- qkv and head: the previous block's ffn post-norm, w13: the block's
// attention post-norm.  pv_fold: Wo's prologue adds P.V's range sums (block_plan.h).  pick: the head's greedy pick, 0 none, 1 atomic, 2 one key per workgroup.
inline gemv_use
gemv_use_of(gemv_role r, bool gemma, bool behind_pn, bool pv_fold = false, int pick = 0)
{
    using N = token_norm;
    using R = token_res;
    switch (r) {
    case gemv_role::qkv: // llama: attention_norm + wq|wk|wv + rope + cache write in ONE launch; gemma3: q_norm / k_norm, rope and the cache write follow
        return !gemma ? gemv_use{1, 4, N::attention, R::qkv_epi} : behind_pn ? gemv_use{2, 0, N::attention, R::pn_ffn} : gemv_use{1, 0, N::attention, R::none};
    case gemv_role::wo: // llama with the residual, gemma3 into `proj` for its post-norm
        return {pv_fold ? 3 : 0, gemma ? 0 : 1, N::none, gemma ? R::none : R::row};
    case gemv_role::w13: // ffn_norm + w1|w3 + act*mul
        return behind_pn ? gemv_use{2, 3, N::ffn, R::pn_attn} : gemv_use{1, gemma ? 3 : 2, N::ffn, R::none};
    case gemv_role::w2:
        return {0, gemma ? 0 : 1, N::none, gemma ? R::none : R::row};
    case gemv_role::head: // (the post-norm prologue passes its row through `res`, so that variant takes no pick)
        return behind_pn ? gemv_use{2, 0, N::final, R::pn_ffn}
                         : gemv_use{1, pick ? 5 : 0, N::final, pick == 2 ? R::pick_per_wg : pick == 1 ? R::pick_atomic : R::none};
    }
    return {0, 0, N::none, R::none};
}

// ---------------------------------------------------------------- inputs
struct token_layer {
    block_shape b;
    gemv_shape w2;
};
struct token_fixed { // what a decoder fixes when it is created (its weights loaded, its sampler set)
    block_model m;
    const block_env* e;
    std::vector<token_layer> layers; // the owned blocks
    gemv_shape head;
    int emb_fmt, vocab;
    bool first_stage, last_stage;
    int top_k;
    float inv_temp_T, top_p_T;
};
struct token_state { // what changes between tokens
    bool attn_fused_on, want_taps;
    int sampler_kind;
    bool lazy;      // inside mc_decoder_generate: the fold of the pick may wait for the next token's embed
    bool advance;   // the embed also advances the step state
    bool in_hidden; // the inbound row already is `hidden`
};

// gemma3: post-norms folded into the prologue of the launch that consumes them (gemv.h PRO 2) -- 7 launches per block instead of 9.  Not with parity
// taps (they want every block output in HBM) and only while the row fits the prologue's register path.
inline bool
fold_post_norms(const token_fixed& f, const token_state& st)
{
    const decoder_options& opt = *f.e->g.opt;
    return f.m.family == MC_FAMILY_GEMMA3 && !st.want_taps && opt.gemma_fuse && (size_t)f.m.dim * f.e->g.tb / 16 <= (size_t)4 * opt.gemv_block;
}
// is a post-norm pending in front of the head?  (the last block's, on the stage that owns it)
inline bool
head_behind_post_norm(const token_fixed& f, const token_state& st) { return f.last_stage && !f.layers.empty() && fold_post_norms(f, st); }
// does the greedy pick ride in the head's own launch (gemv.h EPI_STORE_PICK)?
inline bool
head_pick_ok(const token_fixed& f, const token_state& st, bool behind_pn)
{
    const decoder_options& opt = *f.e->g.opt;
    return st.sampler_kind == MC_SAMPLER_GREEDY && opt.head_pick_on && !behind_pn && opt.lin_waves == 8 && !f.head.lora_cols &&
           (lin_ok(f.head, f.e->g) || ling_kib(f.head, f.e->g)) && f.vocab % 2 == 0;
}
// chained greedy generation on one stage: can the fold wait for the next token's embedding launch?
inline bool
lazy_pick_ok(const token_fixed& f, const token_state& st, bool behind_pn)
{
    const decoder_options& opt = *f.e->g.opt;
    return opt.lazy_pick_on && f.first_stage && f.last_stage && head_pick_ok(f, st, behind_pn) && opt.head_pick_mode == 2 && f.emb_fmt == MC_WFMT_T && !st.want_taps;
}

// ---------------------------------------------------------------- the answer
struct token_launch {
    std::string name;
    unsigned gx = 0, gy = 1, gz = 1, block = 0, lds = 0;
};
struct token_step {
    token_op op;
    int layer = -1; // the owned block; -1: the embed, the head, the pick
    token_launch L; // (park_row and tap are copies: no launch)
    // GEMVs: the pair, the operands, and whether this is the adaptor's `A x` in front of its linear (y is then the linear's adaptor vector)
    int pro = 0, epi = 0;
    bool adaptor = false, pn_by_value = false; // (gemv_plan::postnorm_by_value)
    token_row x = token_row::none, y = token_row::none, res_row = token_row::none;
    token_res res = token_res::none;
    int res_layer = -1; // whose pn_attn / pn_ffn
    token_norm norm = token_norm::none;
    // embed: it also advances the step state (chained generation on a first stage); every workgroup folds the previous token's pick_keys first (a lazy token)
    bool advance = false, fold_keys = false;
};
// The steps are EMITTED one by one, as they are planned (plan_token's `emit(step)`): the decoder launches each at once, so the planning of the later blocks
// runs while the device works on the earlier ones, as the inline code's did; the test program collects them (`steps`).  What the steps share stays here.
struct token_plan {
    std::vector<token_step> steps;  // (the collecting plan_token(f, st) only)
    std::vector<block_plan> blocks; // per owned block, from its first step on: what the `attn` / `scores` / `pv` steps of that layer pack their arguments from
    bool lazy = false;              // the head left one key per workgroup and NO fold behind it: the next embed, or the caller's last fold_pick, folds
    mc::abi::sampler_params sampler{};
    uint32_t sampler_chunk = 0;
    std::string error; // non-empty: no kernel serves a step
};

namespace token_plan_detail {

// one GEMV of the table: behind its adaptor's `A x` where the linear has one (through the same prologue, so both see the identical normalised row)
template <typename Emit> inline void
push_gemv(token_plan& P, Emit& emit, token_op op, int layer, const gemv_shape& W, const gemv_env& g, const gemv_use& u, token_row x, token_row y, token_row res_row, int res_layer)
{
    auto one = [&](const gemv_shape& S, int epi, bool adaptor) {
        gemv_plan G = plan_gemv(S, g, u.pro, epi);
        if (G.error && P.error.empty()) P.error = G.error;
        token_step s;
        s.op = op;
        s.layer = layer;
        s.L = {std::move(G.name), G.wgs, 1, 1, G.block, G.lds};
        s.pro = u.pro;
        s.epi = epi;
        s.adaptor = adaptor;
        s.pn_by_value = G.postnorm_by_value;
        s.x = x;
        s.y = adaptor ? token_row::none : y;
        s.norm = u.norm;
        // (the adaptor stores plainly: of `res` it takes the post-norm its prologue applies, nothing else)
        const bool keeps_res = !adaptor || u.pro == 2;
        s.res = keeps_res ? u.res : token_res::none;
        s.res_row = keeps_res && u.res == token_res::row ? res_row : token_row::none;
        s.res_layer = keeps_res && (u.res == token_res::pn_attn || u.res == token_res::pn_ffn) ? res_layer : -1;
        emit(s);
    };
    if (W.lora_cols) one(gemv_shape{MC_WFMT_T, W.lora_cols, W.in, 0, 0}, 0, true); // the stacked A [lora_cols][in]: plain T, one level
    one(W, u.epi, false);
}

inline token_step
step_of(token_op op, int layer, token_launch L = {}, token_row x = token_row::none, token_row y = token_row::none)
{
    token_step s;
    s.op = op;
    s.layer = layer;
    s.L = std::move(L);
    s.x = x;
    s.y = y;
    return s;
}

} // namespace token_plan_detail

// The head and the pick behind it: final norm + output head (llama.h:128-133), then greedy inside the head's launch, by mc_argmax_keys over its
// per-workgroup keys (left to the next embed in a lazy token), by mc_argmax_T, or make_default_sampler's two launches (MC_SAMPLER_DRAW: its last phase
// draws).  pending: the block whose ffn post-norm is the head's prologue, -1 none.  The prompt pass ends with these steps too, nothing pending.
template <typename Emit> inline void
plan_head(token_plan& P, const token_fixed& f, const token_state& st, int pending, Emit&& emit)
{
    auto push = [&](token_op op, int layer, token_launch L = {}, token_row x = token_row::none, token_row y = token_row::none) { emit(token_plan_detail::step_of(op, layer, std::move(L), x, y)); };
    using namespace token_plan_detail;
    const decoder_options& opt = *f.e->g.opt;
    const std::string& T = f.e->tname;
    const bool pick = head_pick_ok(f, st, pending >= 0);
    const gemv_use u = gemv_use_of(gemv_role::head, f.m.family == MC_FAMILY_GEMMA3, pending >= 0, false, pick ? (opt.head_pick_mode == 2 ? 2 : 1) : 0);
    push_gemv(P, emit, token_op::head_gemv, -1, f.head, f.e->g, u, pending >= 0 ? token_row::proj : token_row::hidden, token_row::logits, token_row::none, pending);
    if (pick) {
        P.lazy = st.lazy && lazy_pick_ok(f, st, pending >= 0);
        if (opt.head_pick_mode == 2 && !P.lazy) push(token_op::fold_pick, -1, {"mc_argmax_keys", 1, 1, 1, 256, 0});
        return;
    }
    if (st.sampler_kind == MC_SAMPLER_GREEDY) {
        push(token_op::argmax, -1, {"mc_argmax_" + T, 1, 1, 1, 1024, 0}, token_row::logits);
        return;
    }
    if (const std::string why = mcimpl::sampler_plan(f.top_k, f.vocab, f.inv_temp_T, f.top_p_T, &P.sampler, &P.sampler_chunk); !why.empty()) {
        if (P.error.empty()) P.error = why;
        return;
    }
    push(token_op::candidates, -1, {"mc_topk_candidates_" + T, P.sampler.nlists, 1, 1, 64, 0}, token_row::logits);
    push(token_op::sample, -1, {(st.sampler_kind == MC_SAMPLER_DRAW ? "mc_draw_" : "mc_sample_") + T, 1, 1, 1, 128, P.sampler.cap * 8});
}

template <typename Emit> inline void
plan_token(token_plan& P, const token_fixed& f, const token_state& st, Emit&& emit)
{
    auto push = [&](token_op op, int layer, token_launch L = {}, token_row x = token_row::none, token_row y = token_row::none) { emit(token_plan_detail::step_of(op, layer, std::move(L), x, y)); };
    using namespace token_plan_detail;
    using R = token_row;
    const block_model& m = f.m;
    const block_env& e = *f.e;
    const std::string& T = e.tname;
    const bool gemma = m.family == MC_FAMILY_GEMMA3;
    const int H = m.n_heads, KV = m.n_kv_heads, hd = m.head_dim, n_own = (int)f.layers.size();
    const bool fuse_pn = fold_post_norms(f, st);
    P.blocks.reserve(n_own);
    R cur = st.in_hidden ? R::hidden : R::in; // the current hidden row
    if (f.first_stage) {
        // (a lazy token: the previous token's pick is folded HERE, by every workgroup of this launch, instead of by a mc_argmax_keys launch behind its head)
        const bool q8 = f.emb_fmt != MC_WFMT_T;
        token_step s = step_of(token_op::embed, -1, {(q8 ? "mc_embed_q8_" : "mc_embed_") + T, ((unsigned)m.dim + 255) / 256, 1, 1, 256, 0}, R::none, R::hidden);
        s.advance = st.advance;
        s.fold_keys = st.advance && st.lazy && lazy_pick_ok(f, st, head_behind_post_norm(f, st));
        emit(s);
        if (st.want_taps) push(token_op::tap, -1, {}, R::hidden);
        cur = R::hidden;
    }
    if (fuse_pn && cur != R::hidden && n_own > 0) {
        // the residual pointers of the folded prologues are fixed at `hidden`: a later pipeline stage first parks its inbound row there
        push(token_op::park_row, -1, {}, cur, R::hidden);
        cur = R::hidden;
    }
    int pending = -1; // gemma3: the block whose ffn post-norm (+ residual hidden_b -> hidden) is left to the next pre-norm launch, applied to `proj`
    for (int li = 0; li < n_own; li++) {
        const token_layer& L = f.layers[li];
        P.blocks.push_back(plan_block(L.b, m, e, block_state{st.attn_fused_on, pending >= 0}));
        const block_plan& B = P.blocks.back();
        // the step that takes the block's input applies the pending post-norm: `proj` in, the post-norm's descriptor with it, the block input left in `hidden`
        auto take_pending = [&](token_step& s) {
            s.x = R::proj;
            s.res = token_res::pn_ffn;
            s.res_layer = pending;
            pending = -1;
            cur = R::hidden;
        };
        if (B.qkv_gemv) {
            const bool pn = pending >= 0;
            push_gemv(P, emit, token_op::qkv_gemv, li, L.b.qkv, e.g, gemv_use_of(gemv_role::qkv, gemma, pn), pn ? R::proj : cur, R::qkv, R::none, pending);
            if (pn) {
                pending = -1;
                cur = R::hidden;
            }
            if (B.rope_kv) push(token_op::rope_kv, li, {"mc_rope_kv_" + T, (unsigned)(H + 2 * KV), 1, 1, (unsigned)hd / 2, 0}, R::qkv, R::q_rot);
        }
        // the attention launch of the form: x is what it starts from, y where it ends (block_plan.h: behind Wo, or at the attention row)
        const R wo_y = gemma ? R::proj : R::hidden;
        switch (B.form) {
        case block_form::qkv_wo_w13_w:
        case block_form::qkv_wo_w:
        case block_form::qkv_wo_i8:
        case block_form::qkv_wo_i4: push(token_op::attn, li, {B.name, B.grid, 1, 1, 512, 0}, cur, R::hidden); break;
        case block_form::qkv_only: push(token_op::attn, li, {B.name, B.grid, 1, 1, 512, 0}, cur, R::attn_out); break;
        case block_form::qkv_wo_qkn: {
            token_step s = step_of(token_op::attn, li, {B.name, B.grid, 1, 1, 512, 0}, cur, R::proj);
            if (pending >= 0) take_pending(s);
            emit(s);
            break;
        }
        case block_form::wo_qkn: push(token_op::attn, li, {B.name, B.grid, 1, 1, 512, 0}, R::qkv, R::proj); break;
        case block_form::wo_i4: {
            token_step s = step_of(token_op::attn, li, {B.name, B.grid, 1, 1, 512, 0}, R::q_rot, wo_y);
            if (!gemma) {
                s.res = token_res::row;
                s.res_row = cur;
            }
            emit(s);
            break;
        }
        case block_form::fused_qkn: push(token_op::attn, li, {B.name, B.grid, 1, 1, 256, 0}, R::qkv, R::attn_out); break;
        case block_form::fused:
        case block_form::fused_t2: push(token_op::attn, li, {B.name, B.grid, 1, 1, 256, 0}, R::q_rot, R::attn_out); break;
        case block_form::scores_pv:
            push(token_op::scores, li, {B.name, (unsigned)e.nsplit, (unsigned)KV, 1, 256, 0}, R::q_rot);
            push(token_op::pv, li, {"mc_attn_pv_" + T, (unsigned)hd / 16, (unsigned)KV, (unsigned)B.pv_ranges, B.pv_block, 0}, R::none,
                 B.pv_ranges > 1 ? R::pv_parts : R::attn_out);
            if (B.pv_reduce) push(token_op::pv_reduce, li, {"mc_attn_pv_reduce_" + T, ((unsigned)(H * hd) + 255) / 256, 1, 1, 256, 0}, R::pv_parts, R::attn_out);
            break;
        }
        // wo (+ residual) where the launches above stopped at the attention row
        if (B.wo_gemv)
            push_gemv(P, emit, token_op::wo_gemv, li, L.b.wo, e.g, gemv_use_of(gemv_role::wo, gemma, false, B.pv_fold), B.pv_fold ? R::pv_parts : R::attn_out, wo_y, cur, -1);
        // gemma3: the attention post-norm + residual, unless it is the w1|w3 GEMV's prologue
        if (gemma && !fuse_pn) push(token_op::post_norm_attn, li, {"mc_rmsnorm_row_" + T, 1, 1, 1, 1024, 0}, cur, R::hidden);
        // ffn_norm + w1|w3 + act*mul (qkv_wo_w13_w: a phase of the attention launch)
        if (B.form != block_form::qkv_wo_w13_w)
            push_gemv(P, emit, token_op::w13_gemv, li, L.b.w13, e.g, gemv_use_of(gemv_role::w13, gemma, fuse_pn), fuse_pn ? R::proj : R::hidden, R::gate, R::none, li);
        // w2 (+ residual); gemma3: into `proj`, its post-norm left to the next pre-norm launch -- the next block's, or the head's -- or a row of its own
        // where the folds are off or the row leaves this pipeline stage
        push_gemv(P, emit, token_op::w2_gemv, li, L.w2, e.g, gemv_use_of(gemv_role::w2, gemma, false), R::gate, gemma ? R::proj : R::hidden, R::hidden, -1);
        if (gemma && fuse_pn && (li + 1 < n_own || f.last_stage))
            pending = li;
        else if (gemma)
            push(token_op::post_norm_ffn, li, {"mc_rmsnorm_row_" + T, 1, 1, 1, 1024, 0}, fuse_pn ? R::hidden_b : R::hidden, R::hidden);
        cur = R::hidden;
        if (st.want_taps) push(token_op::tap, li, {}, R::hidden);
    }
    if (f.last_stage) {
        if (n_own == 0 && !f.first_stage) push(token_op::park_row, -1, {}, cur, R::hidden);
        plan_head(P, f, st, pending, emit);
    }
}

// ... collected: what the test program prints
inline token_plan
plan_token(const token_fixed& f, const token_state& st)
{
    token_plan P;
    plan_token(P, f, st, [&P](const token_step& s) { P.steps.push_back(s); });
    return P;
}
