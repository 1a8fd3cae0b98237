// The batch's step path (the map of the whole: batch_impl.h): creation and release; prepare() and run(), which reserve for and execute the ordered
// plan of any call on a batch (batch_call_plan.h) -- every launch's arguments are bound here --; the log-probability records; and the lockstep
// (mc_batch_step / _generate) and ragged (mc_ragged_step / _generate) entry points.
#include "batch_impl.h"

using namespace mcimpl;

// y[r] = epi(W x[r]) for the B rows, the launch plan_batch_gemv planned: the wide form (fx.wide, one answer for every linear of a batch) takes L.out
// in front of ldy; adaptor: a = T(A x) for all rows into lora_vec, the launch the plan lists in front of a linear with an adaptor (L.lora, what
// plan_batch_gemv read), whose main launch takes the adaptor's five arguments behind its own
mc_status
mc_batch::gemv(const launch_plan& l, bool adaptor, const batch_linear& L, const void* xin, void* y, uint32_t ldy)
{
    auto args = [&](const void* w, const void* scales, void* out, uint32_t ngroups, uint32_t group, uint32_t rows_out, uint32_t ld) {
        return fx.wide ? pack(w, scales, xin, out, (uint32_t)L.in, ngroups, group, (uint32_t)B, rows_out, ld)
                                 : pack(w, scales, xin, out, (uint32_t)L.in, ngroups, group, (uint32_t)B, ld);
    };
    if (adaptor) return launch(l, args(L.lora_a, nullptr, lora_vec, 0, 0, (uint32_t)L.lora_cols, (uint32_t)lora_ld));
    arg_pack a = args(L.w, L.scales, y, (uint32_t)L.ngroups, (uint32_t)L.group, (uint32_t)L.out, ldy);
    if (L.lora) {
        a.push((const void*)lora_vec);
        a.push((uint32_t)lora_ld);
        a.push(L.lora_b);
        a.push((uint32_t)L.lora_cols);
        a.push(L.lora_scale);
    }
    return launch(l, std::move(a));
}

// Part 2n: `slots` records (of `cap` reserved), every slot filled with 0xFF: a slot no pick reaches (an idle or retired row, a row outside a
// packed call) reads as NaN bits and id -1
mc_status
mc_batch::begin_records(logprob_records& r, int slots, int cap)
{
    const int top = logprobs_top;
    mc_status s;
    if ((s = reserve(r.tok, r.tok_cap, slots, cap)) != MC_OK) return s;
    MC_HIP(hipMemsetAsync(r.tok, 0xFF, sizeof(float) * (size_t)slots, p.stream));
    if (top > 0) {
        if ((s = reserve(r.ids, r.ids_cap, slots, cap, sizeof(int32_t) * top)) != MC_OK || (s = reserve(r.top, r.top_cap, slots, cap, sizeof(float) * top)) != MC_OK)
            return s;
        MC_HIP(hipMemsetAsync(r.ids, 0xFF, sizeof(int32_t) * (size_t)slots * top, p.stream));
        MC_HIP(hipMemsetAsync(r.top, 0xFF, sizeof(float) * (size_t)slots * top, p.stream));
    }
    r.count = 0; // (until the call says whose they are: a step in front of its launches, a verify call behind them)
    return MC_OK;
}

// ... and copied out behind a getter's own checks (ids, top: may be null)
mc_status
mc_batch::copy_records(const logprob_records& r, size_t slots, float* tok, int32_t* ids, float* top)
{
    const size_t n = (size_t)logprobs_top;
    MC_HIP(hipSetDevice(p.ordinal));
    MC_HIP(hipStreamSynchronize(p.stream));
    MC_HIP(hipMemcpy(tok, r.tok, sizeof(float) * slots, hipMemcpyDeviceToHost));
    if (ids) MC_HIP(hipMemcpy(ids, r.ids, sizeof(int32_t) * slots * n, hipMemcpyDeviceToHost));
    if (top) MC_HIP(hipMemcpy(top, r.top, sizeof(float) * slots * n, hipMemcpyDeviceToHost));
    return MC_OK;
}

// A planned call of n tokens in front of its first launch: the refusal; tokens_dev; with log-probabilities the scratch of the two launches -- a
// part per (row, chunk) and the chunks' keys at the most top_n, sized by the bounds, so a change of top_n keeps them -- and the records; a verify
// call's packed rows (M <= 128; sized for any call) with -1 in the results of the rows not in the call; the tables, each sent when it differs from
// what the device holds (none while no launch of the plan reads it)
mc_status
mc_batch::prepare(const batch_call_plan& c, int n)
{
    if (!c.refusal.empty()) return fail(c.code, c.refusal);
    const mc_decoder_config& cfg = p.cfg;
    mc_status s = ensure_tokens(n);
    if (s != MC_OK) return s;
    if (c.lp_slots) {
        const int R = c.M ? MC_VERIFY_MAX_ROWS : B;
        const size_t nchunk = ((size_t)cfg.vocab + LOGPROB_CHUNK - 1) / LOGPROB_CHUNK;
        if ((s = reserve(lp_parts, lp_parts_cap, R, R, sizeof(logprob_part) * nchunk)) != MC_OK ||
            (s = reserve(lp_keys, lp_keys_cap, R, R, sizeof(uint64_t) * nchunk * MC_LOGPROBS_MAX_TOP)) != MC_OK ||
            (s = c.M ? begin_records(vs.records, c.M, MC_VERIFY_MAX_ROWS) : begin_records(records, n * B, n * B)) != MC_OK)
            return s;
        if (!c.M) records.count = n;
    }
    if (c.M) {
        const int out_max = 2 * MC_WIDE_BATCH_MAX + MC_VERIFY_MAX_ROWS + MC_VERIFY_MAX_LEN * MC_WIDE_BATCH_MAX;
        if ((s = reserve(vs.xn, vs.xn_cap, c.M, MC_VERIFY_MAX_ROWS, (size_t)cfg.dim * 2)) != MC_OK ||
            (s = reserve(vs.logits, vs.logits_cap, c.M, MC_VERIFY_MAX_ROWS, (size_t)cfg.vocab * 2)) != MC_OK ||
            (s = reserve(vs.out, vs.out_cap, 2 * B + c.M + MC_VERIFY_MAX_LEN * B, out_max)) != MC_OK)
            return s;
        MC_HIP(hipMemsetAsync(vs.out, 0xFF, sizeof(int32_t) * 2 * B, p.stream)); // -1: a row not in the call
        if (c.tree) MC_HIP(hipMemsetAsync(vs.out + 2 * B + c.M, 0xFF, sizeof(int32_t) * MC_VERIFY_MAX_LEN * B, p.stream)); // ... its path
        if (!c.verify.empty() && ((s = reserve(vs.tab, vs.tab_cap, c.M, MC_VERIFY_MAX_ROWS)) != MC_OK || (s = send_if_changed(vs.tab, vs.tab_sent, c.verify)) != MC_OK))
            return s;
        if (c.cand_rows && (s = reserve(vs.cand, vs.cand_cap, c.cand_rows, MC_VERIFY_MAX_ROWS, sizeof(uint64_t) * fx.cand_per_row)) != MC_OK) return s;
    }
    if (!c.logits.empty() && ((s = ensure(logits_tab_dev, sizeof(row_logits) * B)) != MC_OK || (s = send_if_changed(logits_tab_dev, logits_tab_sent, c.logits)) != MC_OK))
        return s;
    return c.samplers.empty() ? MC_OK : send_if_changed(samplers_dev, samplers_sent, c.samplers);
}

// ONE launch of a plan: its op's arguments, bound here and nowhere else.  A token -- lockstep: at a.pos for every row, the kernels read the
// shared state; advance: a chained step (row r's step_index moves by B).  Ragged: every row at its own rows[r].pos, the per-row kernels; a.pos is
// not used and the begin launch starts the step (advance: retires the rows that stopped, moves the others on); rows whose pos is -1 get no pick.
// The log-probability launches put the record in the slot the pick's token landed in (a verify call: of picks[m] in slot m).  A verify call --
// a.xrows: its M packed rows, a.ids: its ids on the device, a.nodes: a tree's table -- picks per packed row, then accepts per segment (the accepted
// row's logits into logits[row]), counts the accepted path on the penalised rows and (a tree) moves its K / V into place in every layer
mc_status
mc_batch::run(const batch_launch& l, const call_args& a)
{
    using op = batch_op;
    const batch_call_plan& c = a.plan;
    const mc_decoder_config& cfg = p.cfg;
    const int H = cfg.n_heads, KV = cfg.n_kv_heads, hd = cfg.head_dim, n_rep = H / KV, li = l.layer;
    const uint32_t vocab = (uint32_t)cfg.vocab;
    const uint64_t cstride = cache_elems;
    const int32_t advance = a.advance ? 1 : 0;
    const step_state* state = c.ragged ? rows : st; // the lockstep kernels read the shared state, their _rows forms row r's own
    const sampler_params& sp = c.sp;
    // a verify call's tables and results on the device: the segments, picks[M] and (a tree) paths[B][MC_VERIFY_MAX_LEN] behind accepted[B], next_tokens[B]
    const pp_seg* segs = c.M ? (const pp_seg*)pp_segs(pp_tab) : nullptr;
    int32_t* picks = c.M ? vs.out + 2 * B : nullptr;
    const int32_t* paths = c.tree ? picks + c.M : nullptr;
    switch (l.op) {
    case op::begin_lockstep: return set_pos(a.pos);
    case op::begin_rows:
        return launch(l.L, pack(rows, (const int32_t*)stop_dev, (int32_t)stop_host.size(), (int32_t)cfg.max_seq_len, (int32_t)B, advance));
    case op::begin_rolling:
        return launch(l.L, pack(rows, (const int32_t*)stop_dev, (int32_t)stop_host.size(), (int32_t)cfg.max_seq_len, (int32_t)p.pre_len, advance, rcos, rsin,
                                (uint32_t)hd, cfg.rope_theta));
    case op::embed:
    case op::embed_rows: {
        const bool q8 = p.emb_fmt != MC_WFMT_T;
        const void* emb = q8 ? nullptr : p.emb_table;
        const void* emb_q8 = q8 ? p.emb_table : nullptr;
        if (l.op == op::embed_rows) return launch(l.L, pack(emb, p.emb_scales, emb_q8, x, rows, (uint32_t)cfg.dim));
        return launch(l.L, pack(emb, p.emb_scales, emb_q8, x, rows, (uint32_t)cfg.dim, advance, (uint32_t)B));
    }
    case op::attn_norm: return launch(l.L, pack((const void*)x, p.layers[li].attention_norm, xn, (uint32_t)cfg.dim, cfg.norm_eps));
    case op::ffn_norm: return launch(l.L, pack((const void*)x, p.layers[li].ffn_norm, xn, (uint32_t)cfg.dim, cfg.norm_eps));
    case op::final_norm: return launch(l.L, pack((const void*)x, p.final_norm, xn, (uint32_t)cfg.dim, cfg.norm_eps));
    case op::qkv_adaptor:
    case op::qkv_gemv: return gemv(l.L, l.op == op::qkv_adaptor, p.layers[li].qkv, xn, qkv, (uint32_t)p.layers[li].qkv.out);
    case op::wo_adaptor:
    case op::wo_gemv: return gemv(l.L, l.op == op::wo_adaptor, p.layers[li].wo, att, x, (uint32_t)cfg.dim);
    case op::w13_adaptor:
    case op::w13_gemv: return gemv(l.L, l.op == op::w13_adaptor, p.layers[li].w13, xn, gate, (uint32_t)(p.layers[li].w13.out / 2));
    case op::w2_adaptor:
    case op::w2_gemv: return gemv(l.L, l.op == op::w2_adaptor, p.layers[li].w2, gate, x, (uint32_t)cfg.dim);
    case op::head_gemv: return gemv(l.L, false, p.output, xn, logits, vocab);
    case op::rope:
        return launch(l.L, pack(qkv, q, (void*)kc_of(li, 0), (void*)vt_of(li, 0), c.rolling ? rcos : fcos, c.rolling ? rsin : fsin, state, (uint32_t)H, (uint32_t)KV,
                                (uint32_t)hd, (uint32_t)cfg.max_seq_len, cstride));
    case op::scores: // T(attn_scale): the scalar_mul of attention.h:196 is evaluated in T
        return launch(l.L, pack(q, (void*)kc_of(li, 0), expv, psum, state, (uint32_t)n_rep, (uint32_t)hd, (uint32_t)cfg.max_seq_len, round_bf_host(cfg.attn_scale),
                                (uint32_t)fx.nsplit, cstride));
    case op::pv:
        return launch(l.L, pack(expv, psum, (void*)vt_of(li, 0), att, state, (uint32_t)n_rep, (uint32_t)hd, (uint32_t)cfg.max_seq_len, (uint32_t)fx.nsplit, cstride));
    case op::process:
    case op::process_rows:
    case op::process_rows_count: { // count: the rows with penalties count their input token first (a step; the packed passes count nothing)
        arg_pack args = pack(logits, vocab, (const row_logits*)logits_tab_dev, (const uint32_t*)masks_dev, counts_dev, (const step_state*)rows);
        if (l.op != op::process) args.push((int32_t)(l.op == op::process_rows_count ? 1 : 0));
        return launch(l.L, std::move(args));
    }
    case op::argmax: return launch(l.L, pack(logits, vocab, rows, tokens_dev));
    case op::candidates: return launch(l.L, pack(logits, vocab, sp.kpad, cand, c.chunk));
    case op::sample: return launch(l.L, pack(cand, sp, seeds, (uint32_t)n_seed_pairs, rows, tokens_dev));
    case op::candidates_mixed:
        return launch(l.L, pack(logits, vocab, sp.kpad, cand, c.chunk, (const row_sampler*)samplers_dev, (const step_state*)rows, (int32_t)(c.ragged ? 1 : 0)));
    case op::pick_mixed:
        return launch(l.L, pack(logits, vocab, (const uint64_t*)cand, (const row_sampler*)samplers_dev, sp.nlists, sp.kpad, sp.cap, (const uint64_t*)seeds,
                                (uint32_t)n_seed_pairs, rows, tokens_dev));
    case op::logprob_parts:
    case op::logprob_finish: { // token and slot from the rows' state, or (a verify call) from picks[m] and m
        const void* rows_logits = c.M ? vs.logits : logits;
        const step_state* from = c.M ? nullptr : rows;
        const int32_t* from_picks = c.M ? picks : nullptr;
        const logprob_records& r = c.M ? vs.records : records;
        const uint32_t top = (uint32_t)logprobs_top, nslots = c.M ? (uint32_t)c.M : (uint32_t)(records.count * B);
        if (l.op == op::logprob_parts) return launch(l.L, pack(rows_logits, vocab, top, lp_parts, lp_keys, from));
        return launch(l.L, pack(rows_logits, vocab, top, c.lp_nchunk, (const logprob_part*)lp_parts, (const uint64_t*)lp_keys, from, from_picks, nslots, r.tok, r.ids,
                                r.top));
    }
    case op::v_norm: return launch(l.L, pack(a.xrows, p.final_norm, vs.xn, (uint32_t)cfg.dim, cfg.norm_eps));
    case op::v_head: {
        const batch_linear& L = p.output;
        return launch(l.L, pack(L.w, L.scales, (const void*)vs.xn, vs.logits, (uint32_t)L.in, (uint32_t)L.ngroups, (uint32_t)L.group, (uint32_t)c.M, (uint32_t)L.out,
                                vocab));
    }
    case op::v_process:
        return launch(l.L, pack(vs.logits, vocab, (const verify_row*)vs.tab, (const row_logits*)logits_tab_dev, (const uint32_t*)masks_dev, (const int32_t*)counts_dev,
                                a.ids));
    case op::v_argmax: return launch(l.L, pack((const void*)vs.logits, vocab, picks));
    case op::v_candidates: return launch(l.L, pack((const void*)vs.logits, vocab, sp.kpad, vs.cand, c.chunk, (const verify_row*)vs.tab));
    case op::v_sample:
        return launch(l.L, pack((const void*)vs.logits, vocab, (const uint64_t*)vs.cand, (const verify_row*)vs.tab, sp.nlists, sp.kpad, sp.cap, (const uint64_t*)seeds,
                                (uint32_t)n_seed_pairs, picks));
    case op::v_accept: return launch(l.L, pack(segs, a.ids, (const int32_t*)picks, (const void*)vs.logits, vocab, vs.out, vs.out + B, logits));
    case op::v_tree_accept:
        return launch(l.L, pack(segs, a.ids, a.nodes, (const int32_t*)picks, (const void*)vs.logits, vocab, vs.out, vs.out + B, (int32_t*)paths, logits));
    case op::v_count:
        return launch(l.L, pack(segs, a.ids, (const int32_t*)vs.out, paths, (const row_logits*)logits_tab_dev, counts_dev, vocab));
    case op::v_compact:
        return launch(l.L, pack(segs, (const int32_t*)vs.out, paths, kc, vt, (uint64_t)cache_elems, (uint32_t)B, (uint32_t)cfg.n_kv_heads, (uint32_t)cfg.head_dim,
                                (uint32_t)cfg.max_seq_len));
    }
    return fail(MC_ERR_RUNTIME, "mc_batch: a launch without an executor");
}

// the list from front to back -- a token: the fixed body first --, up to the first launch that fails
mc_status
mc_batch::run_all(const call_args& a)
{
    if (a.plan.body)
        for (const batch_launch& l : *a.plan.body)
            if (mc_status s = run(l, a); s != MC_OK) return s;
    for (const batch_launch& l : a.plan.launches)
        if (mc_status s = run(l, a); s != MC_OK) return s;
    return MC_OK;
}

namespace {

// rows' tokens and step indices for token 0 of a call (step_index = r: seed pair r % n_pairs, tokens_out[0][r]); a ragged
// call: their positions too (mc_b_rows_begin derives the rest), an idle row has no token
mc_status
start_rows(mc_batch* b, const int32_t* tokens, const int32_t* positions = nullptr)
{
    b->rows_host.assign(b->B, step_state{});
    for (int r = 0; r < b->B; r++) {
        if (positions) b->rows_host[r].pos = positions[r];
        b->rows_host[r].token = positions && positions[r] < 0 ? -1 : tokens[r];
        b->rows_host[r].step_index = r;
    }
    MC_HIP(hipMemcpyAsync(b->rows, b->rows_host.data(), sizeof(step_state) * b->B, hipMemcpyHostToDevice, b->p.stream));
    return MC_OK;
}

// token 0 of a ragged call: the rows, the stop ids, and -1 in every slot of tokens_out
mc_status
start_ragged(mc_batch* b, const int32_t* tokens, const int32_t* positions, const int32_t* stop_ids, int n_stop, int n)
{
    mc_status s = start_rows(b, tokens, positions);
    if (s != MC_OK) return s;
    b->stop_host.assign(stop_ids, stop_ids + n_stop);
    if ((s = b->reserve(b->stop_dev, b->stop_cap, n_stop, n_stop)) != MC_OK) return s;
    if (n_stop > 0) MC_HIP(hipMemcpyAsync(b->stop_dev, b->stop_host.data(), sizeof(int32_t) * n_stop, hipMemcpyHostToDevice, b->p.stream));
    MC_HIP(hipMemsetAsync(b->tokens_dev, 0xFF, sizeof(int32_t) * (size_t)n * b->B, b->p.stream));
    return MC_OK;
}

// the tail of the four step / generate calls: drain, the call's n x B tokens to the host (tokens_out may be null in a step) and the rows' new
// lengths.  positions null: lockstep, every row now holds start_pos + n.  Ragged: an active row holds its position + what it made -- n, or
// (produced given: mc_ragged_generate) the tokens in front of the first -1 of its column: a row's tokens are a prefix of it, -1 from the step
// after it stopped (an idle row: none)
mc_status
finish(mc_batch* b, int32_t start_pos, const int32_t* positions, int32_t n, int32_t* tokens_out, int32_t* produced = nullptr)
{
    const int B = b->B;
    MC_HIP(hipStreamSynchronize(b->p.stream));
    if (tokens_out) MC_HIP(hipMemcpy(tokens_out, b->tokens_dev, sizeof(int32_t) * (size_t)n * B, hipMemcpyDeviceToHost));
    for (int r = 0; r < B; r++) {
        int32_t made = n;
        if (produced) {
            made = 0;
            while (made < n && tokens_out[(size_t)made * B + r] >= 0) made++;
            produced[r] = made;
        }
        if (!positions) b->lengths[r] = start_pos + n;
        else if (positions[r] >= 0) b->lengths[r] = positions[r] + made;
    }
    return MC_OK;
}

// the four step / generate calls behind their checks: ONE token planned, once; everything reserved and sent; the rows (positions given: a ragged
// call, with its stop ids); the same list for each of the n tokens -- the position and the advance word are arguments, not plan --; the tail
mc_status
run_tokens(mc_batch* b, const int32_t* tokens, int32_t start_pos, const int32_t* positions, int32_t n, const int32_t* stop_ids, int32_t n_stop, int32_t* tokens_out,
           int32_t* produced = nullptr)
{
    MC_HIP(hipSetDevice(b->p.ordinal));
    const batch_call_plan plan = plan_batch_token(b->fx, b->settings(), positions != nullptr);
    mc_status s = b->prepare(plan, n);
    if (s == MC_OK) s = positions ? start_ragged(b, tokens, positions, stop_ids, n_stop, n) : start_rows(b, tokens);
    for (int i = 0; i < n && s == MC_OK; i++) s = b->run_all({plan, start_pos + i, i > 0});
    return s != MC_OK ? s : finish(b, start_pos, positions, n, tokens_out, produced);
}

// mc_batch_create and mc_wide_batch_create: `who` names the caller in the texts, `cap` is its largest batch, `wide` its admission
mc_status
batch_create(const std::string& who, int cap, bool wide, mc_decoder* d, int32_t batch, mc_batch** out)
{
    if (!d || !out) return fail(MC_ERR_INVALID_ARGUMENT, who + ": null argument");
    if (batch < 1 || batch > cap) return fail(MC_ERR_INVALID_ARGUMENT, who + ": batch must lie in [1, " + std::to_string(cap) + "]");
    *out = nullptr;
    decoder_parts parts;
    mc_status s = decoder_parts_of(d, &parts);
    if (s != MC_OK) return s;
    const std::string why = refusal(parts, wide);
    if (!why.empty()) return fail(MC_ERR_INVALID_ARGUMENT, who + ": " + why);
    MC_HIP(hipSetDevice(parts.ordinal));
    std::unique_ptr<mc_batch> b(new mc_batch);
    batch_env env;
    env.B = batch;
    MC_HIP(hipDeviceGetAttribute(&env.cus, hipDeviceAttributeMultiprocessorCount, parts.ordinal));
    env.tiles_env = wb_tiles_env_of(getenv("MC_WB_TILES"));
    b->fx = fix_batch(parts, env);
    b->d = d;
    b->p = parts;
    b->B = batch;
    b->lengths.assign(batch, 0);
    b->row_samplers.assign(batch, row_setting{});
    b->row_logit_set.assign(batch, row_logit_setting{});
    const mc_decoder_config& c = parts.cfg;
    const int H = c.n_heads, KV = c.n_kv_heads, hd = c.head_dim, L = (int)parts.layers.size();
    b->cache_elems = (size_t)KV * c.max_seq_len * hd;
    const size_t cache_bytes = (size_t)L * batch * b->cache_elems * 2;
    const int ffn = parts.layers.empty() ? 0 : parts.layers[0].w13.out / 2;
    if ((s = b->alloc(&b->kc, cache_bytes)) != MC_OK || (s = b->alloc(&b->vt, cache_bytes)) != MC_OK ||
        (s = b->alloc(&b->x, (size_t)batch * c.dim * 2)) != MC_OK || (s = b->alloc(&b->xn, (size_t)batch * c.dim * 2)) != MC_OK ||
        (s = b->alloc(&b->qkv, (size_t)batch * (H + 2 * KV) * hd * 2)) != MC_OK ||
        (s = b->alloc(&b->q, (size_t)batch * H * hd * 2)) != MC_OK || (s = b->alloc(&b->att, (size_t)batch * H * hd * 2)) != MC_OK ||
        (s = b->alloc(&b->gate, (size_t)batch * ffn * 2)) != MC_OK ||
        (s = b->alloc(&b->logits, (size_t)batch * c.vocab * 2)) != MC_OK ||
        (s = b->alloc(&b->expv, sizeof(float) * batch * H * c.max_seq_len)) != MC_OK ||
        (s = b->alloc(&b->psum, sizeof(float) * batch * H * b->fx.nsplit)) != MC_OK ||
        (s = b->alloc(&b->fcos, sizeof(float) * c.max_seq_len * (hd / 2))) != MC_OK ||
        (s = b->alloc(&b->fsin, sizeof(float) * c.max_seq_len * (hd / 2))) != MC_OK ||
        (s = b->alloc(&b->rcos, sizeof(float) * batch * (hd / 2))) != MC_OK ||
        (s = b->alloc(&b->rsin, sizeof(float) * batch * (hd / 2))) != MC_OK ||
        (s = b->alloc(&b->st, sizeof(step_state))) != MC_OK || (s = b->alloc(&b->rows, sizeof(step_state) * batch)) != MC_OK ||
        (s = b->alloc(&b->cand, sizeof(uint64_t) * batch * b->fx.cand_per_row)) != MC_OK ||
        (s = b->alloc(&b->samplers_dev, sizeof(row_sampler) * batch)) != MC_OK)
        return s;
    for (const batch_layer& l : parts.layers)
        for (const batch_linear* lin : {&l.qkv, &l.wo, &l.w13, &l.w2}) b->lora_ld = std::max(b->lora_ld, lin->lora_cols);
    if (b->lora_ld && (s = b->alloc(&b->lora_vec, (size_t)batch * b->lora_ld * 2)) != MC_OK) return s;
    // nn::rope's table for positions [0, max_seq_len) (a row depends on the absolute position only, nn/embedding.h:159-165)
    s = b->launch("mc_rope_table", (hd / 2 + 63) / 64, c.max_seq_len, 1, 64, 0,
                  pack(b->fcos, b->fsin, (uint32_t)c.max_seq_len, (uint32_t)hd, (uint32_t)0, c.rope_theta));
    if (s != MC_OK) return s;
    MC_HIP(hipStreamSynchronize(parts.stream));
    *out = b.release();
    return MC_OK;
}

} // namespace

extern "C" {

mc_status
mc_batch_create(mc_decoder* d, int32_t batch, mc_batch** out)
{
    return batch_create("mc_batch_create", BATCH_MAX, false, d, batch, out);
}

// ---- Part 2h: wide batches ----

mc_status
mc_wide_batch_create(mc_decoder* d, int32_t batch, mc_batch** out)
{
    return batch_create("mc_wide_batch_create", MC_WIDE_BATCH_MAX, true, d, batch, out);
}

void
mc_batch_release(mc_batch* b)
{
    delete b;
}

int32_t
mc_batch_size(const mc_batch* b)
{
    return b ? b->B : 0;
}

mc_status
mc_batch_step(mc_batch* b, const int32_t* tokens, int32_t start_pos, int32_t* next_tokens)
{
    if (!b || !tokens) return fail(MC_ERR_INVALID_ARGUMENT, "mc_batch_step: null argument");
    mc_status s;
    if ((s = refuse(step_bounds(start_pos, b->p.cfg.max_seq_len))) != MC_OK || (s = refuse(check_tokens(tokens, b->B, b->p.cfg.vocab))) != MC_OK) return s;
    return run_tokens(b, tokens, start_pos, nullptr, 1, nullptr, 0, next_tokens);
}

mc_status
mc_batch_generate(mc_batch* b, const int32_t* first_tokens, int32_t start_pos, int32_t n, int32_t* tokens_out)
{
    if (!b || !first_tokens || !tokens_out) return fail(MC_ERR_INVALID_ARGUMENT, "mc_batch_generate: null argument");
    if (n < 1) return fail(MC_ERR_INVALID_ARGUMENT, "mc_batch_generate: n must be positive");
    mc_status s;
    if ((s = refuse(generate_bounds(start_pos, n, b->p.cfg.max_seq_len))) != MC_OK || (s = refuse(check_tokens(first_tokens, b->B, b->p.cfg.vocab))) != MC_OK)
        return s;
    return run_tokens(b, first_tokens, start_pos, nullptr, n, nullptr, 0, tokens_out);
}

mc_status
mc_batch_get_logits(mc_batch* b, void* logits_T)
{
    if (!b || !logits_T) return fail(MC_ERR_INVALID_ARGUMENT, "mc_batch_get_logits: null argument");
    MC_HIP(hipSetDevice(b->p.ordinal));
    MC_HIP(hipStreamSynchronize(b->p.stream));
    MC_HIP(hipMemcpy(logits_T, b->logits, (size_t)b->B * b->p.cfg.vocab * 2, hipMemcpyDeviceToHost));
    return MC_OK;
}

// ---- Part 2c: ragged rows ----

mc_status
mc_ragged_step(mc_batch* b, const int32_t* tokens, const int32_t* positions, int32_t* next_tokens)
{
    if (!b || !tokens || !positions) return fail(MC_ERR_INVALID_ARGUMENT, "mc_ragged_step: null argument");
    const mc_decoder_config& c = b->p.cfg;
    mc_status s = refuse(check_ragged("mc_ragged_step", tokens, positions, 1, b->lengths.data(), b->B, c.max_seq_len, c.vocab, b->rolling));
    if (s != MC_OK) return s;
    return run_tokens(b, tokens, 0, positions, 1, nullptr, 0, next_tokens);
}

mc_status
mc_ragged_generate(mc_batch* b, const int32_t* first_tokens, const int32_t* positions, int32_t n, const int32_t* stop_ids,
                   int32_t n_stop, int32_t* tokens_out, int32_t* lengths)
{
    if (!b || !first_tokens || !positions || !tokens_out || !lengths || (n_stop > 0 && !stop_ids))
        return fail(MC_ERR_INVALID_ARGUMENT, "mc_ragged_generate: null argument");
    if (n < 1) return fail(MC_ERR_INVALID_ARGUMENT, "mc_ragged_generate: n must be positive");
    if (n_stop < 0) return fail(MC_ERR_INVALID_ARGUMENT, "mc_ragged_generate: n_stop must not be negative");
    const mc_decoder_config& c = b->p.cfg;
    mc_status s = refuse(check_ragged("mc_ragged_generate", first_tokens, positions, n, b->lengths.data(), b->B, c.max_seq_len, c.vocab, b->rolling));
    if (s != MC_OK) return s;
    return run_tokens(b, first_tokens, 0, positions, n, stop_ids, n_stop, tokens_out, lengths);
}

mc_status
mc_ragged_lengths(const mc_batch* b, int32_t* lengths)
{
    if (!b || !lengths) return fail(MC_ERR_INVALID_ARGUMENT, "mc_ragged_lengths: null argument");
    std::copy(b->lengths.begin(), b->lengths.end(), lengths);
    return MC_OK;
}

} // extern "C"
