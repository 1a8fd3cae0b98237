// The batch's step path (the map of the whole: batch_impl.h): creation and release, one token -- the launches batch_plan.h plans, with their
// arguments bound here --, and the lockstep (mc_batch_step / _generate) and ragged (mc_ragged_step / _generate) entry points.
#include "batch_impl.h"

using namespace mcimpl;

// y[r] = epi(W x[r]) for the B rows as g says (plan_batch_gemv): a linear with an adaptor takes a = T(A x) for all rows into lora_vec first,
// and its main launch the adaptor's five arguments behind its own
mc_status
mc_batch::gemv(const batch_linear& L, const batch_gemv_plan& g, const void* xin, void* y, uint32_t ldy)
{
    auto args = [&](const void* w, const void* scales, void* out, uint32_t ngroups, uint32_t group, uint32_t rows_out, uint32_t ld) {
        return g.wide ? pack(w, scales, xin, out, (uint32_t)L.in, ngroups, group, (uint32_t)B, rows_out, ld)
                      : pack(w, scales, xin, out, (uint32_t)L.in, ngroups, group, (uint32_t)B, ld);
    };
    if (g.lora) {
        mc_status s = launch(g.adaptor, args(L.lora_a, nullptr, lora_vec, 0, 0, (uint32_t)L.lora_cols, (uint32_t)lora_ld));
        if (s != MC_OK) return s;
    }
    arg_pack a = args(L.w, L.scales, y, (uint32_t)L.ngroups, (uint32_t)L.group, (uint32_t)L.out, ldy);
    if (g.lora) {
        a.push((const void*)lora_vec);
        a.push((uint32_t)lora_ld);
        a.push(L.lora_b);
        a.push((uint32_t)L.lora_cols);
        a.push(L.lora_scale);
    }
    return launch(g.main, std::move(a));
}

mc_status
mc_batch::plan_call(bool ragged)
{
    step = &steps[!ragged ? 0 : (rolling ? 2 : 1)];
    return plan_pick(ragged);
}

// no table (and no launch) of the logit processors while no row has anything set; the samplers' table for the mixed form only
mc_status
mc_batch::plan_pick(bool ragged)
{
    mc_status s;
    lpp = plan_logprobs(logprobs_on, logprobs_top, p.cfg.vocab, B, ragged);
    if (!lpp.refusal.empty()) return fail(MC_ERR_RUNTIME, lpp.refusal);
    if (lpp.any && (s = reserve_logprob_scratch(B)) != MC_OK) return s;
    lp = plan_logits(row_logit_set, p.cfg.vocab, ragged);
    if (lp.any && ((s = ensure(logits_tab_dev, sizeof(row_logits) * B)) != MC_OK || (s = send_if_changed(logits_tab_dev, logits_tab_sent, lp.table)) != MC_OK))
        return s;
    pick = plan_head(row_samplers, decoder_sampler_of(d), p.cfg.vocab, ragged, cand_per_row);
    if (!pick.refusal.empty()) return fail(MC_ERR_RUNTIME, pick.refusal);
    return pick.form == PICK_MIXED ? send_if_changed(samplers_dev, samplers_sent, pick.table) : MC_OK;
}

// one token of the call plan_call planned.  Lockstep: at `pos` for every row; advance: a chained step (row r's step_index moves by B).
// Ragged: every row at its own rows[r].pos instead, the same launches with the per-row kernels; `pos` is not used, and
// mc_b_rows_begin starts the step (advance: retires the rows that stopped, moves the others on).
mc_status
mc_batch::enqueue_token(int pos, bool advance)
{
    const mc_decoder_config& c = p.cfg;
    const step_plan& sp = *step;
    const int H = c.n_heads, KV = c.n_kv_heads, hd = c.head_dim, n_rep = H / KV;
    const float scale_T = round_bf_host(c.attn_scale); // T(attn_scale): the scalar_mul of attention.h:196 is evaluated in T
    const uint64_t cstride = cache_elems;
    const bool q8 = p.emb_fmt != MC_WFMT_T;
    const void* emb = q8 ? nullptr : p.emb_table;
    const void* emb_q8 = q8 ? p.emb_table : nullptr;
    mc_status s;
    if (sp.rolling)
        s = launch(sp.begin, pack(rows, (const int32_t*)stop_dev, (int32_t)stop_host.size(), (int32_t)c.max_seq_len, (int32_t)p.pre_len,
                                  (int32_t)(advance ? 1 : 0), rcos, rsin, (uint32_t)hd, c.rope_theta));
    else if (sp.ragged)
        s = launch(sp.begin, pack(rows, (const int32_t*)stop_dev, (int32_t)stop_host.size(), (int32_t)c.max_seq_len, (int32_t)B, (int32_t)(advance ? 1 : 0)));
    else
        s = set_pos(pos);
    if (s != MC_OK) return s;
    if (sp.ragged)
        s = launch(sp.embed, pack(emb, p.emb_scales, emb_q8, x, rows, (uint32_t)c.dim));
    else
        s = launch(sp.embed, pack(emb, p.emb_scales, emb_q8, x, rows, (uint32_t)c.dim, (int32_t)(advance ? 1 : 0), (uint32_t)B));
    if (s != MC_OK) return s;
    // the per-row launches: the lockstep kernel reads the shared state, its _rows form row r's own
    const step_state* state = sp.ragged ? rows : st;
    for (size_t li = 0; li < p.layers.size(); li++) {
        const batch_layer& L = p.layers[li];
        const layer_gemvs& g = gemvs[li];
        const int l = (int)li;
        if ((s = launch(sp.rmsnorm, pack((const void*)x, L.attention_norm, xn, (uint32_t)c.dim, c.norm_eps))) != MC_OK) return s;
        if ((s = gemv(L.qkv, g.qkv, xn, qkv, (uint32_t)L.qkv.out)) != MC_OK) return s;
        s = launch(sp.rope, pack(qkv, q, (void*)kc_of(l, 0), (void*)vt_of(l, 0), sp.rolling ? rcos : fcos, sp.rolling ? rsin : fsin, state, (uint32_t)H,
                                 (uint32_t)KV, (uint32_t)hd, (uint32_t)c.max_seq_len, cstride));
        if (s != MC_OK) return s;
        s = launch(sp.scores, pack(q, (void*)kc_of(l, 0), expv, psum, state, (uint32_t)n_rep, (uint32_t)hd, (uint32_t)c.max_seq_len, scale_T,
                                   (uint32_t)nsplit, cstride));
        if (s != MC_OK) return s;
        s = launch(sp.pv, pack(expv, psum, (void*)vt_of(l, 0), att, state, (uint32_t)n_rep, (uint32_t)hd, (uint32_t)c.max_seq_len, (uint32_t)nsplit,
                               cstride));
        if (s != MC_OK) return s;
        if ((s = gemv(L.wo, g.wo, att, x, (uint32_t)c.dim)) != MC_OK) return s;
        if ((s = launch(sp.rmsnorm, pack((const void*)x, L.ffn_norm, xn, (uint32_t)c.dim, c.norm_eps))) != MC_OK) return s;
        if ((s = gemv(L.w13, g.w13, xn, gate, (uint32_t)(L.w13.out / 2))) != MC_OK) return s;
        if ((s = gemv(L.w2, g.w2, gate, x, (uint32_t)c.dim)) != MC_OK) return s;
    }
    return head(sp.ragged, true);
}

// the final norm of x, the head and the pick per row as plan_pick planned them (the three forms: batch_plan.h plan_head), each row with its
// effective sampler; ragged: rows whose rows[r].pos is -1 get no pick.  Part 2l: with a mask or penalties on any row,
// mc_b_logits_process_* rewrites those rows' logits between the head and the pick; count: the rows with penalties count their input token
// first (a step; the packed passes count nothing).  Part 2n: with the batch's switch on, the two log-probability launches run behind the pick
// in all three forms, and the record lands in the slot the pick's token landed in
mc_status
mc_batch::head(bool ragged, bool count)
{
    const uint32_t vocab = (uint32_t)p.cfg.vocab;
    mc_status s;
    if ((s = launch(steps[0].rmsnorm, pack((const void*)x, p.final_norm, xn, (uint32_t)p.cfg.dim, p.cfg.norm_eps))) != MC_OK) return s;
    if ((s = gemv(p.output, head_gemv, xn, logits, vocab)) != MC_OK) return s;
    if ((s = process_logits(ragged, count)) != MC_OK) return s;
    const sampler_params& sp = pick.sp;
    switch (pick.form) {
    case PICK_GREEDY: s = launch(pick.first, pack(logits, vocab, rows, tokens_dev)); break;
    case PICK_UNIFORM:
        if ((s = launch(pick.first, pack(logits, vocab, sp.kpad, cand, pick.chunk))) != MC_OK) return s;
        s = launch(pick.second, pack(cand, sp, seeds, (uint32_t)n_seed_pairs, rows, tokens_dev));
        break;
    default:
        s = launch(pick.first, pack(logits, vocab, sp.kpad, cand, pick.chunk, (const row_sampler*)samplers_dev, (const step_state*)rows,
                                    (int32_t)(ragged ? 1 : 0)));
        if (s != MC_OK) return s;
        s = launch(pick.second, pack(logits, vocab, (const uint64_t*)cand, (const row_sampler*)samplers_dev, sp.nlists, sp.kpad, sp.cap,
                                     (const uint64_t*)seeds, (uint32_t)n_seed_pairs, rows, tokens_dev));
    }
    if (s != MC_OK || !lpp.any) return s;
    return enqueue_logprobs(lpp, logits, rows, nullptr, (uint32_t)(lp_n * B), lp_tok, lp_ids, lp_top);
}

// Part 2n: the records of a call of n tokens beside tokens_dev -- reserved, and every slot filled with 0xFF: a slot no pick reaches (an idle or
// retired row, a row outside a packed call) reads as NaN bits and id -1
mc_status
mc_batch::begin_logprobs(int n)
{
    if (!logprobs_on) return MC_OK;
    const int slots = n * B, top = logprobs_top;
    mc_status s;
    if ((s = reserve(lp_tok, lp_tok_cap, slots, slots)) != MC_OK) return s;
    MC_HIP(hipMemsetAsync(lp_tok, 0xFF, sizeof(float) * (size_t)slots, p.stream));
    if (top > 0) {
        if ((s = reserve(lp_ids, lp_ids_cap, slots, slots, sizeof(int32_t) * top)) != MC_OK || (s = reserve(lp_top, lp_top_cap, slots, slots, sizeof(float) * top)) != MC_OK)
            return s;
        MC_HIP(hipMemsetAsync(lp_ids, 0xFF, sizeof(int32_t) * (size_t)slots * top, p.stream));
        MC_HIP(hipMemsetAsync(lp_top, 0xFF, sizeof(float) * (size_t)slots * top, p.stream));
    }
    lp_n = n;
    return MC_OK;
}

// a part per (row, chunk) and the chunks' keys at the most top_n, for R rows: sized by the bounds, so a change of top_n keeps them
mc_status
mc_batch::reserve_logprob_scratch(int R)
{
    const size_t nchunk = ((size_t)p.cfg.vocab + LOGPROB_CHUNK - 1) / LOGPROB_CHUNK;
    mc_status s = reserve(lp_parts, lp_parts_cap, R, R, sizeof(logprob_part) * nchunk);
    if (s != MC_OK) return s;
    return reserve(lp_keys, lp_keys_cap, R, R, sizeof(uint64_t) * nchunk * MC_LOGPROBS_MAX_TOP);
}

mc_status
mc_batch::enqueue_logprobs(const logprobs_plan& l, const void* rows_logits, const step_state* state, const int32_t* picks, uint32_t nslots, float* out_tok,
                           int32_t* out_ids, float* out_top)
{
    const uint32_t vocab = (uint32_t)p.cfg.vocab, top = (uint32_t)logprobs_top;
    mc_status s = launch(l.parts, pack(rows_logits, vocab, top, lp_parts, lp_keys, state));
    if (s != MC_OK) return s;
    return launch(l.finish, pack(rows_logits, vocab, top, l.nchunk, (const logprob_part*)lp_parts, (const uint64_t*)lp_keys, state, picks, nslots, out_tok,
                                 out_ids, out_top));
}

mc_status
mc_batch::process_logits(bool ragged, bool count)
{
    if (!lp.any) return MC_OK;
    arg_pack a = pack(logits, (uint32_t)p.cfg.vocab, (const row_logits*)logits_tab_dev, (const uint32_t*)masks_dev, counts_dev, (const step_state*)rows);
    if (ragged) a.push((int32_t)(count ? 1 : 0));
    return launch(lp.launch, std::move(a));
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
    b->genv.B = batch;
    MC_HIP(hipDeviceGetAttribute(&b->genv.cus, hipDeviceAttributeMultiprocessorCount, parts.ordinal));
    b->genv.tiles_env = wb_tiles_env_of(getenv("MC_WB_TILES"));
    b->d = d;
    b->p = parts;
    b->B = batch;
    b->lengths.assign(batch, 0);
    b->row_samplers.assign(batch, row_setting{});
    b->row_logit_set.assign(batch, row_logit_setting{});
    const mc_decoder_config& c = parts.cfg;
    const int H = c.n_heads, KV = c.n_kv_heads, hd = c.head_dim, L = (int)parts.layers.size();
    b->nsplit = (c.max_seq_len + PB - 1) / PB;
    for (const batch_layer& l : parts.layers)
        b->gemvs.push_back({plan_batch_gemv(l.qkv, 0, b->genv), plan_batch_gemv(l.wo, 1, b->genv), plan_batch_gemv(l.w13, 2, b->genv),
                            plan_batch_gemv(l.w2, 1, b->genv)});
    b->head_gemv = plan_batch_gemv(parts.output, 0, b->genv);
    for (int form = 0; form < 3; form++) b->steps[form] = plan_step(c, batch, b->nsplit, form > 0, form == 2);
    b->cache_elems = (size_t)KV * c.max_seq_len * hd;
    const size_t cache_bytes = (size_t)L * batch * b->cache_elems * 2;
    const int ffn = parts.layers.empty() ? 0 : parts.layers[0].w13.out / 2;
    const uint32_t lists512 = ((uint32_t)c.vocab + 511) / 512;
    b->cand_per_row = (size_t)std::max(lists512, 1u) * 128;
    if ((s = b->alloc(&b->kc, cache_bytes)) != MC_OK || (s = b->alloc(&b->vt, cache_bytes)) != MC_OK ||
        (s = b->alloc(&b->x, (size_t)batch * c.dim * 2)) != MC_OK || (s = b->alloc(&b->xn, (size_t)batch * c.dim * 2)) != MC_OK ||
        (s = b->alloc(&b->qkv, (size_t)batch * (H + 2 * KV) * hd * 2)) != MC_OK ||
        (s = b->alloc(&b->q, (size_t)batch * H * hd * 2)) != MC_OK || (s = b->alloc(&b->att, (size_t)batch * H * hd * 2)) != MC_OK ||
        (s = b->alloc(&b->gate, (size_t)batch * ffn * 2)) != MC_OK ||
        (s = b->alloc(&b->logits, (size_t)batch * c.vocab * 2)) != MC_OK ||
        (s = b->alloc(&b->expv, sizeof(float) * batch * H * c.max_seq_len)) != MC_OK ||
        (s = b->alloc(&b->psum, sizeof(float) * batch * H * b->nsplit)) != MC_OK ||
        (s = b->alloc(&b->fcos, sizeof(float) * c.max_seq_len * (hd / 2))) != MC_OK ||
        (s = b->alloc(&b->fsin, sizeof(float) * c.max_seq_len * (hd / 2))) != MC_OK ||
        (s = b->alloc(&b->rcos, sizeof(float) * batch * (hd / 2))) != MC_OK ||
        (s = b->alloc(&b->rsin, sizeof(float) * batch * (hd / 2))) != MC_OK ||
        (s = b->alloc(&b->st, sizeof(step_state))) != MC_OK || (s = b->alloc(&b->rows, sizeof(step_state) * batch)) != MC_OK ||
        (s = b->alloc(&b->cand, sizeof(uint64_t) * batch * b->cand_per_row)) != MC_OK ||
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
    MC_HIP(hipSetDevice(b->p.ordinal));
    if ((s = b->plan_call(false)) != MC_OK || (s = b->ensure_tokens(1)) != MC_OK || (s = b->begin_logprobs(1)) != MC_OK || (s = start_rows(b, tokens)) != MC_OK ||
        (s = b->enqueue_token(start_pos, false)) != MC_OK)
        return s;
    return finish(b, start_pos, nullptr, 1, next_tokens);
}

mc_status
mc_batch_generate(mc_batch* b, const int32_t* first_tokens, int32_t start_pos, int32_t n, int32_t* tokens_out)
{
    if (!b || !first_tokens || !tokens_out) return fail(MC_ERR_INVALID_ARGUMENT, "mc_batch_generate: null argument");
    if (n < 1) return fail(MC_ERR_INVALID_ARGUMENT, "mc_batch_generate: n must be positive");
    mc_status s;
    if ((s = refuse(generate_bounds(start_pos, n, b->p.cfg.max_seq_len))) != MC_OK || (s = refuse(check_tokens(first_tokens, b->B, b->p.cfg.vocab))) != MC_OK)
        return s;
    MC_HIP(hipSetDevice(b->p.ordinal));
    if ((s = b->plan_call(false)) != MC_OK || (s = b->ensure_tokens(n)) != MC_OK || (s = b->begin_logprobs(n)) != MC_OK || (s = start_rows(b, first_tokens)) != MC_OK) return s;
    for (int i = 0; i < n; i++)
        if ((s = b->enqueue_token(start_pos + i, i > 0)) != MC_OK) return s;
    return finish(b, start_pos, nullptr, n, tokens_out);
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
    MC_HIP(hipSetDevice(b->p.ordinal));
    if ((s = b->plan_call(true)) != MC_OK || (s = b->ensure_tokens(1)) != MC_OK || (s = b->begin_logprobs(1)) != MC_OK ||
        (s = start_ragged(b, tokens, positions, nullptr, 0, 1)) != MC_OK ||
        (s = b->enqueue_token(0, false)) != MC_OK)
        return s;
    return finish(b, 0, positions, 1, next_tokens);
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
    MC_HIP(hipSetDevice(b->p.ordinal));
    if ((s = b->plan_call(true)) != MC_OK || (s = b->ensure_tokens(n)) != MC_OK || (s = b->begin_logprobs(n)) != MC_OK ||
        (s = start_ragged(b, first_tokens, positions, stop_ids, n_stop, n)) != MC_OK)
        return s;
    for (int i = 0; i < n; i++)
        if ((s = b->enqueue_token(0, i > 0)) != MC_OK) return s;
    return finish(b, 0, positions, n, tokens_out, lengths);
}

mc_status
mc_ragged_lengths(const mc_batch* b, int32_t* lengths)
{
    if (!b || !lengths) return fail(MC_ERR_INVALID_ARGUMENT, "mc_ragged_lengths: null argument");
    std::copy(b->lengths.begin(), b->lengths.end(), lengths);
    return MC_OK;
}

} // extern "C"
