// What ONE call on a batch launches, in order (the pieces: batch_plan.h): plan_batch_token() -- a token of mc_batch_step / _generate and
// mc_ragged_step / _generate, from the begin launch to the last launch behind the pick --, plan_rows_tail() -- the same list from the final norm on,
// behind the prompt pass of mc_rows_prefill / mc_extend_rows -- and plan_verify_call() -- the head of mc_verify_rows / mc_tree_verify over the packed
// rows.  A plan carries the call's refusal, the launches with an op tag each, the tables the call uploads and what it needs reserved; the n tokens
// of a generate call run one list (pos and advance are arguments), and the part of a token no setting changes -- everything in front of the final
// norm -- is listed once, when the batch is created (batch_fixed::body): a call plans its tail alone.  No HIP, no mc_batch, no device pointer: tests/cpp/test_batch_plan.cc and
// test_verify_settings_plan.cc print the lists on the CPU.  mc_batch::run() (batch.cc) binds each op's arguments and decides nothing.
#pragma once

#include <cassert>

#include "batch_plan.h"

namespace mcimpl {

// one value per distinct argument list
enum class batch_op {
    begin_lockstep, begin_rows, begin_rolling, embed, embed_rows, attn_norm, ffn_norm, final_norm,
    qkv_adaptor, qkv_gemv, wo_adaptor, wo_gemv, w13_adaptor, w13_gemv, w2_adaptor, w2_gemv, head_gemv, // adaptor: a = T(A x) in front of its linear
    rope, scores, pv,
    process, process_rows, process_rows_count, // the ragged form takes the count flag: off behind a prompt pass
    argmax, candidates, sample, candidates_mixed, pick_mixed,
    logprob_parts, logprob_finish,
    v_norm, v_head, v_process, v_argmax, v_candidates, v_sample, v_accept, v_tree_accept, v_count, v_compact
};
struct batch_launch {
    batch_op op;
    int layer = -1; // -1: the begin, the embed, the head and everything behind it
    launch_plan L;
};

// what a batch fixes at its creation: B, the split of the attention scores, the candidate keys it holds per row, the launches of a step in its
// three forms (lockstep, ragged, ragged on a rolling batch) and the head's GEMV -- and with them the BODY of a token in each form, from the begin
// launch to the last layer's w2: no setting of a call changes it, so a call's plan points at it and no call builds it again
struct batch_fixed {
    mc_decoder_config cfg{};
    int B = 0, nsplit = 0, n_layers = 0;
    bool wide = false; // B > 16: every GEMV of the batch is the wide kernel, whose argument list has the rows of the matrix in front of ldy
    size_t cand_per_row = 0;
    linear_shape head;
    batch_gemv_plan head_gemv;
    step_plan steps[3];
    std::vector<batch_launch> body[3];
};
// Parts: as refusal() reads them
template <typename Parts> batch_fixed
fix_batch(const Parts& p, const batch_env& e)
{
    batch_fixed f;
    f.cfg = p.cfg;
    f.B = e.B;
    f.nsplit = (p.cfg.max_seq_len + PB - 1) / PB;
    f.n_layers = (int)p.layers.size();
    f.cand_per_row = (size_t)std::max(((uint32_t)p.cfg.vocab + 511) / 512, 1u) * 128;
    f.head = p.output;
    f.head_gemv = plan_batch_gemv(p.output, 0, e);
    f.wide = f.head_gemv.wide;
    assert(!f.head_gemv.lora && "the admission refuses an adaptor on the head: a token's plan lists no adaptor launch in front of it");
    using op = batch_op;
    for (int form = 0; form < 3; form++) {
        const step_plan& st = f.steps[form] = plan_step(p.cfg, e.B, f.nsplit, form > 0, form == 2);
        std::vector<batch_launch>& body = f.body[form];
        auto gemv = [&](op adaptor, op main, const batch_gemv_plan& g, int layer) { // (a linear with an adaptor: a = T(A x) in front)
            assert(g.wide == f.wide);
            if (g.lora) body.push_back({adaptor, layer, g.adaptor});
            body.push_back({main, layer, g.main});
        };
        body.push_back({form == 0 ? op::begin_lockstep : (form == 2 ? op::begin_rolling : op::begin_rows), -1, st.begin});
        body.push_back({form == 0 ? op::embed : op::embed_rows, -1, st.embed});
        for (int l = 0; l < f.n_layers; l++) {
            const auto& L = p.layers[l];
            body.push_back({op::attn_norm, l, st.rmsnorm});
            gemv(op::qkv_adaptor, op::qkv_gemv, plan_batch_gemv(L.qkv, 0, e), l);
            body.push_back({op::rope, l, st.rope});
            body.push_back({op::scores, l, st.scores});
            body.push_back({op::pv, l, st.pv});
            gemv(op::wo_adaptor, op::wo_gemv, plan_batch_gemv(L.wo, 1, e), l);
            body.push_back({op::ffn_norm, l, st.rmsnorm});
            gemv(op::w13_adaptor, op::w13_gemv, plan_batch_gemv(L.w13, 2, e), l);
            gemv(op::w2_adaptor, op::w2_gemv, plan_batch_gemv(L.w2, 1, e), l);
        }
    }
    return f;
}

// what may change between calls (and cannot inside one): the switches, the decoder's sampler and what the row slots carry
struct call_settings {
    bool rolling = false, verify_settings_on = false, logprobs_on = false;
    int logprobs_top = 0, n_seed_pairs = 0;
    decoder_sampler dec;
    const std::vector<row_setting>& samplers;         // [B]
    const std::vector<row_logit_setting>& logit_rows; // [B]
};

struct batch_call_plan {
    std::string refusal; // "" = none, else the call fails with `code`
    mc_status code = MC_OK;
    bool ragged = false, rolling = false, tree = false;
    const std::vector<batch_launch>* body = nullptr; // a token: the batch's fixed list in front of `launches` (batch_fixed::body)
    std::vector<batch_launch> launches;              // what the call's settings decide: from the final norm on; a verify call: its whole head
    // the tables the call uploads (empty: none, the launches that read it are not in the list)
    std::vector<row_sampler> samplers; // [B]
    std::vector<row_logits> logits;    // [B]
    std::vector<verify_row> verify;    // [M]
    sampler_params sp{};
    uint32_t chunk = 0, lp_nchunk = 0;
    // what the call needs reserved: the packed rows of a verify call's head, those of them with candidate keys, the log-probability records of
    // one token (B, or M; their width is the batch's top_n, which a call does not decide)
    int M = 0, cand_rows = 0, lp_slots = 0;

    void add(batch_op op, const launch_plan& l) { launches.push_back({op, -1, l}); }
    // the whole list in order (the tests print it; the executor walks the two parts where they lie)
    std::vector<batch_launch> listed() const
    {
        std::vector<batch_launch> all = body ? *body : std::vector<batch_launch>{};
        all.insert(all.end(), launches.begin(), launches.end());
        return all;
    }
    batch_call_plan& refuse(const std::string& why)
    {
        refusal = why;
        code = MC_ERR_RUNTIME;
        return *this;
    }
};

// the checks in the order the calls made them: the log-probability launches, then the pick
inline batch_call_plan
plan_token_from(const batch_fixed& f, const call_settings& s, bool ragged, bool count, bool tail)
{
    using op = batch_op;
    const int vocab = f.cfg.vocab;
    batch_call_plan c;
    c.ragged = ragged;
    c.rolling = ragged && s.rolling;
    const logprobs_plan lprob = plan_logprobs(s.logprobs_on, s.logprobs_top, vocab, f.B, ragged);
    if (!lprob.refusal.empty()) return c.refuse(lprob.refusal);
    const logits_plan lg = plan_logits(s.logit_rows, vocab, ragged);
    const head_plan h = plan_head(s.samplers, s.dec, vocab, ragged, f.cand_per_row);
    if (!h.refusal.empty()) return c.refuse(h.refusal);
    if (!tail) c.body = &f.body[!ragged ? 0 : (s.rolling ? 2 : 1)];
    c.add(op::final_norm, f.steps[0].rmsnorm);
    c.add(op::head_gemv, f.head_gemv.main); // (no adaptor: the admission refuses one on the head)
    if (lg.any) c.add(!ragged ? op::process : (count ? op::process_rows_count : op::process_rows), lg.launch);
    if (h.form == PICK_GREEDY) {
        c.add(op::argmax, h.first);
    } else {
        const bool mixed = h.form == PICK_MIXED;
        c.add(mixed ? op::candidates_mixed : op::candidates, h.first);
        c.add(mixed ? op::pick_mixed : op::sample, h.second);
        if (mixed) c.samplers = h.table;
    }
    if (lprob.any) {
        c.add(op::logprob_parts, lprob.parts);
        c.add(op::logprob_finish, lprob.finish);
        c.lp_slots = f.B;
    }
    if (lg.any) c.logits = lg.table;
    c.sp = h.sp;
    c.chunk = h.chunk;
    c.lp_nchunk = lprob.nchunk;
    return c;
}

// ONE token of a step or ragged call; the rows with penalties count their input token
inline batch_call_plan
plan_batch_token(const batch_fixed& f, const call_settings& s, bool ragged)
{
    return plan_token_from(f, s, ragged, true, false);
}

// behind a prompt pass (mc_rows_prefill, mc_extend_rows): the ragged token from the final norm on, nothing counted
inline batch_call_plan
plan_rows_tail(const batch_fixed& f, const call_settings& s)
{
    return plan_token_from(f, s, true, false, true);
}

// the head of mc_verify_rows / mc_tree_verify (nodes: the call's tv_node table in packed order, null = chains) over the M packed rows of nseg
// segments: norm, head, [process], argmax or the two sampling launches, [logprob parts, finish], accept, [count], [compact].  With the batch's switch
// off (verify_settings_on) the calls have refused every row that would need the bracketed settings launches
inline batch_call_plan
plan_verify_call(const batch_fixed& f, const call_settings& s, const int32_t* lens, int M, int nseg, const tv_node* nodes)
{
    using op = batch_op;
    const int vocab = f.cfg.vocab;
    batch_call_plan c;
    c.tree = nodes != nullptr;
    c.M = M;
    const logprobs_plan lprob = plan_logprobs(s.logprobs_on, s.logprobs_top, vocab, M, false);
    if (!lprob.refusal.empty()) return c.refuse(lprob.refusal);
    verify_pick_plan vp;
    verify_logits_plan vl;
    if (s.verify_settings_on) {
        vp = plan_verify_pick(lens, s.samplers, s.dec, vocab, s.n_seed_pairs, nodes, f.cand_per_row);
        if (!vp.refusal.empty()) return c.refuse(vp.refusal);
        vl = plan_verify_logits(lens, s.logit_rows, vocab, M, nseg);
    }
    const verify_plan v = plan_verify_head(f.head, f.cfg, f.n_layers, M, nseg, c.tree);
    c.add(op::v_norm, v.norm);
    c.add(op::v_head, v.head);
    if (vl.any) c.add(op::v_process, vl.process);
    if (vp.greedy) {
        c.add(op::v_argmax, v.argmax);
    } else {
        c.add(op::v_candidates, vp.first);
        c.add(op::v_sample, vp.second);
        c.cand_rows = M;
    }
    if (lprob.any) {
        c.add(op::logprob_parts, lprob.parts);
        c.add(op::logprob_finish, lprob.finish);
        c.lp_slots = M;
    }
    c.add(c.tree ? op::v_tree_accept : op::v_accept, v.accept);
    if (vl.count) c.add(op::v_count, vl.counting);
    if (c.tree) c.add(op::v_compact, v.compact);
    if (!vp.greedy || vl.any) c.verify = vp.table;
    if (vl.any) c.logits = vl.table;
    c.sp = vp.sp;
    c.chunk = vp.chunk;
    c.lp_nchunk = lprob.nchunk;
    return c;
}

} // namespace mcimpl
