// Part 2 of include/metalchat_hip.h: the fused per-token decode pipeline.
//
// This is the host-side driver the reference spreads over header-only templates:
//   nn::llama3::operator()        include/metalchat/nn/llama.h:113-134
//   nn::gemma3::operator()        include/metalchat/nn/gemma.h:110-137
//   nn::transformer::operator()   include/metalchat/nn/transformer.h:126-141
//   nn::attention::operator()     include/metalchat/nn/attention.h:161-206
//   nn::sink_cache / nn::rope     include/metalchat/nn/cache.h:96-232, nn/embedding.h:107-200
//   transformer<Layer>::transform include/metalchat/transformer.h:357-364
// Instead of ~1000 one-op launches and as many allocations per token it issues 4 to 6 launches per
// layer (llama3: wq|wk|wv, attention + Wo, w1|w3, w2 for the headline shapes -- token_plan.h plan_token) on one in-order stream over a pre-allocated arena, keeps the token / position state in
// HBM so successive steps chain without a host round trip, and (optionally) replays one captured
// hipGraph per token.
// struct mc_decoder itself, and which unit defines the rest of it (weights, prompt pass, library GEMM): decoder_impl.h.

#include "decoder_impl.h"

using namespace mcimpl;

mc_decoder::~mc_decoder()
{
    (void)hipSetDevice(dev->ordinal);
    drop_graph();
    for (void* p : allocs) (void)hipFree(p);
    if (blas) blaslt_release(blas);
    if (err_evt) (void)hipEventDestroy(err_evt);
    if (err_host) (void)hipHostFree(err_host);
}

void
mc_decoder::query_occupancy()
{
    block_occupancy& occ = benv.occ;
    if (tb != 2 || occ.fused >= 0) return;
    auto ask = [&](const std::string& name, int block) {
        hipFunction_t f;
        if (fn(name, &f) != MC_OK) return 0;
        int n = 0;
        if (hipModuleOccupancyMaxActiveBlocksPerMultiprocessor(&n, f, block, 0) != hipSuccess) return 0;
        return n;
    };
    occ.fused = ask("mc_attn_fused_bfloat", 256);
    const int hd = cfg.head_dim, k = cfg.n_heads * hd / 2048;
    occ.wo = ask("mc_attn_wo_i4_bfloat_hd" + std::to_string(hd) + "_k" + std::to_string(k), 512);
    occ.wo_w = hd == 64 ? ask("mc_attn_qkv_wo_w_bfloat_hd64_k4_q4", 512) : 0;
    occ.wo_i8 = hd == 128 ? ask("mc_attn_qkv_wo_i8_bfloat_hd128_k4_q4_t4", 512) : 0;
    occ.wo_qkn = hd == 256 ? ask("mc_attn_wo_qkn_i4_bfloat_hd256_k2_t2", 512) : 0;
    occ.qkv_qkn = hd == 256 ? ask("mc_attn_qkv_wo_qkn_i4_bfloat_hd256_k2_p2_t2", 512) : 0;
    occ.qkv_only = hd == 128 ? ask("mc_attn_qkv_i4_bfloat_hd128_q4", 512) : 0;
    occ.wo_i4_wide = hd == 128 ? ask("mc_attn_qkv_wo_i4_bfloat_hd128_k2_q2_t4", 512) : 0;
    occ.w13 = hd == 64 ? ask("mc_attn_qkv_wo_w13_w_bfloat_hd64_k4_q4_f4p4", 512) : 0;
    // (one kernel per family is asked: the widest-range / most-register instantiation, which bounds the others -- every form is ONE 512-thread
    //  workgroup per CU, so the answer that matters is "at least one")
    (void)hipGetLastError();
}

// a hand-off gave up: report nothing yet, make the NEXT launches independent of co-residency
void
mc_decoder::handoff_failed()
{
    (void)hipMemsetAsync(&state->err, 0, 4, stream);
    (void)hipStreamSynchronize(stream);
    attn_fused_on = false; // (block_plan.h handoffs_ok: every form of plan_block with a hand-off needs it)
    drop_graph();
    handoff_fallbacks++;
    clean_tokens = 0;
    if (handoff_fallbacks > 1 && rearm_after > 0 && rearm_after < (1 << 24)) rearm_after *= 2;
}

// a hand-off inside a launch that gave up (bounded waits, decode_kernels.hip): reported once, then cleared
mc_status
mc_decoder::check_handoffs(const step_state& st)
{
    if (!st.err) return MC_OK;
    return report_handoff(st.err);
}

mc_status
mc_decoder::report_handoff(uint32_t code)
{
    handoff_failed();
    char buf[384];
    snprintf(buf, sizeof buf, "decoder: an in-launch hand-off of the decode attention timed out (code 0x%08x): the workgroups of the "
                              "launch were not resident together.  What was computed since is invalid; the decoder now uses the "
                              "launches that need no co-residency -- repeat the call", code);
    return fail(MC_ERR_RUNTIME, buf);
}

// state.err at a point where the stream has just been synchronised (logits / hidden rows / caches read back, a prompt pass):
// a step nobody waited for must not leave a set flag behind -- every later hand-off would return at once, on rows that
// have not arrived, without an error
mc_status
mc_decoder::check_err_synced()
{
    if (!attn_psum_g) return MC_OK;
    uint32_t e = 0;
    MC_HIP(hipMemcpy(&e, &state->err, 4, hipMemcpyDeviceToHost));
    err_pending = false;
    return e ? report_handoff(e) : MC_OK;
}

// ... and at the start of every call: the flag of an earlier step that was copied out behind it (note_err_async), if that
// copy has completed -- never a wait
mc_status
mc_decoder::poll_pending_err()
{
    if (!err_pending || hipEventQuery(err_evt) != hipSuccess) return MC_OK;
    err_pending = false;
    const uint32_t e = *err_host;
    return e ? report_handoff(e) : MC_OK;
}

void
mc_decoder::note_err_async()
{
    if (!attn_psum_g || !err_host) return;
    if (hipMemcpyAsync(err_host, &state->err, 4, hipMemcpyDeviceToHost, stream) != hipSuccess) return;
    if (hipEventRecord(err_evt, stream) == hipSuccess) err_pending = true;
}

// one decode GEMV: what plan_gemv (gemv_plan.h) says -- kernel, grid, workgroup, LDS -- behind the adaptor's own GEMV where the linear has one
mc_status
mc_decoder::gemv(const linear_w& L, int pro, int epi, const void* x, void* y, const void* res,
     const void* norm_w, float mu)
{
    const gemv_plan P = plan_gemv(shape_of(L), benv.g, pro, epi);
    if (P.error) return fail(MC_ERR_RUNTIME, P.error);
    if (L.lora_cols) {
        // a = T(A x): the stacked adaptor inputs through the same kernel family (same prologue,
        // so a pre-norm GEMV and its adaptor see the identical normalised row)
        mc_status s = gemv(*L.lora_a, pro, 0, x, L.lora_vec, pro == 2 ? res : nullptr, norm_w, mu);
        if (s != MC_OK) return s;
    }
    return gemv_launch(L, P.name, P.wgs, P.block, P.lds, P.postnorm_by_value, x, y, res, norm_w, mu);
}

// ... the launch itself, as planned: a step of a token's plan comes here directly (its adaptor is a step of its own)
mc_status
mc_decoder::gemv_launch(const linear_w& L, const std::string& name, unsigned wgs, unsigned block, unsigned lds, bool pn_by_value, const void* x, void* y,
                        const void* res, const void* norm_w, float mu)
{
    if (pn_by_value) {
        const auto it = pn_host.find(res);
        if (it == pn_host.end()) return fail(MC_ERR_RUNTIME, "gemv: unknown post-norm descriptor");
        const postnorm_args& h = it->second;
        return launch(name, wgs, 1, 1, block, lds,
                      pack(L.w, L.scales, x, y, (const void*)h.res, norm_w, (uint32_t)L.out, (uint32_t)L.in, (uint32_t)L.group,
                           cfg.norm_eps, mu, (const void*)h.post_w, (const void*)h.h_out, (uint32_t)0, 0.0f));
    }
    return launch(name, wgs, 1, 1, block, lds,
                  pack(L.w, L.scales, x, y, res, norm_w, (uint32_t)L.out, (uint32_t)L.in,
                       (uint32_t)L.group, cfg.norm_eps, mu, (const void*)L.lora_vec,
                       (const void*)L.lora_b, (uint32_t)L.lora_cols, L.lora_scale));
}

mc_status
mc_decoder::ensure_rope(int pos, int len)
{
    // nn::rope::operator() (include/metalchat/nn/embedding.h:190-198): the table holds 2 * max_seq_len rows and is
    // regenerated from the requested position when that leaves the window (a table row depends on the absolute
    // position only, so where the window starts never shows in a value)
    if (rope_valid && pos >= rope_start && pos + len <= rope_start + rope_rows) return MC_OK;
    rope_start = pos + len <= rope_rows && !rope_valid ? 0 : pos;
    const unsigned half = cfg.head_dim / 2;
    for (int t = 0; t < 2; t++) {
        const float theta = t == 0 ? cfg.rope_theta : cfg.rope_sliding_theta;
        if (!rope_cos[t]) continue;
        mc_status s = launch("mc_rope_table", (half + 63) / 64, rope_rows, 1, 64, 0,
                             pack(rope_cos[t], rope_sin[t], (uint32_t)rope_rows,
                                  (uint32_t)cfg.head_dim, (uint32_t)rope_start, theta));
        if (s != MC_OK) return s;
    }
    rope_valid = true;
    // the window start lives in the step state: a captured mc_step_advance reads it there, so a graph captured
    // under another window stays valid
    return launch("mc_step_rope", 1, 1, 1, 64, 0, pack(state, (int32_t)rope_start));
}

// ------------------------------------------------------------------------------------------------
// One token: plan_token() (token_plan.h) says which launches, in which order, on which symbolic operands; everything from here to run_token() binds
// device pointers to those symbols and packs each kernel's arguments.
// ------------------------------------------------------------------------------------------------
token_fixed
mc_decoder::token_fixed_now() const
{
    token_fixed f{model(), &benv, {}, shape_of(output), emb_fmt, cfg.vocab, first_stage, last_stage, top_k, inv_temp_T, top_p_T};
    f.layers.reserve(layers.size());
    for (const layer_w& L : layers) f.layers.push_back({{shape_of(L.qkv), shape_of(L.wo), shape_of(L.w13)}, shape_of(L.w2)});
    return f;
}

// the one-workgroup fold of the head's per-workgroup keys: the token into the step state and the token list
mc_status
mc_decoder::fold_pick()
{
    return launch("mc_argmax_keys", 1, 1, 1, 256, 0, pack((const void*)pick_keys, (uint32_t)pick_slots, state, tokens_dev));
}

// The attention launch of a block in the form `P` (block_plan.h): from `x` -- the row handed to the block, the raw wq|wk|wv row or the rotated queries --
// to `y` -- behind Wo (+ the residual `res` where the form adds it) or the attention row.  pn: the post-norm descriptor the launch's prologue applies.
mc_status
mc_decoder::attn_launch(const layer_w& L, const block_plan& P, const void* x, void* y, const void* res, const void* pn)
{
    const int H = cfg.n_heads, KV = cfg.n_kv_heads, hd = cfg.head_dim, n_rep = H / KV;
    const float mu = cfg.family == MC_FAMILY_GEMMA3 ? 1.0f : 0.0f;
    const float scale_T = tb == 2 ? bf2f_host(f2bf_host(cfg.attn_scale)) : cfg.attn_scale;
    const uint32_t S = (uint32_t)cfg.max_seq_len, tag = (uint32_t)(&L - layers.data()) + 1, ns = (uint32_t)P.ns;
    const float* rcos = rope_cos[L.rope_table];
    const float* rsin = rope_sin[L.rope_table];
    const void *kc = L.kc, *vt = L.vt, *wo_w = L.wo.w, *wo_s = L.wo.scales, *qkv_w = L.qkv.w, *qkv_s = L.qkv.scales, *an = L.attention_norm;
    const void *qn = L.q_norm, *kn = L.k_norm;
    void* const none = nullptr;
    arg_pack a;
    switch (P.form) {
    case block_form::qkv_wo_w13_w:
    case block_form::qkv_wo_w:
    case block_form::qkv_wo_i8:
    case block_form::qkv_wo_i4:
        // attention_norm, wq|wk|wv, rope, cache write, scores, softmax, P.V, wo + residual (transformer.h:130-133, attention.h:170-205) in ONE launch: every
        // hand-off but the last stays inside one kv head (plain weights: fewer than 8 kv heads are launched as 8 virtual ones, kv_virtual_shift; P.ns ranges
        // of 64 P.tiles slots per kv head)
        a = pack(kc, vt, attn_out, attn_psum_g, attn_slab_g, attn_row_g, attn_qkv_g, state, (uint32_t)(n_rep >> P.vsh), (uint32_t)(KV << P.vsh), S, scale_T, ns, tag,
                 wo_w, wo_s, x, y, (uint32_t)L.wo.out, (uint32_t)L.wo.group, an, qkv_w, qkv_s, rcos, rsin, cfg.norm_eps, mu, P.fast, none, (uint32_t)P.vsh);
        // ... and ffn_norm, w1|w3, act*mul (transformer.h:135-137, 53-59) too: the block up to the gate row in ONE launch
        if (P.form == block_form::qkv_wo_w13_w) push_all(a, attn_hid_g, (const void*)L.w13.w, (const void*)L.ffn_norm, gate, (uint32_t)L.w13.out, none);
        break;
    case block_form::qkv_only:
        // attention_norm, wq|wk|wv, rope, cache write, scores, softmax, P.V (transformer.h:130, attention.h:170-203) in ONE launch; Wo + residual from the finished row
        a = pack(kc, vt, y, attn_psum_g, attn_slab_g, attn_qkv_g, state, (uint32_t)n_rep, (uint32_t)KV, S, scale_T, ns, tag, x, (uint32_t)L.qkv.group,
                 an, qkv_w, qkv_s, rcos, rsin, cfg.norm_eps, mu, P.fast, none);
        break;
    case block_form::qkv_wo_qkn: {
        // gemma3, ONE launch from the row handed to the block to Wo's output: (the previous block's ffn post-norm + residual,) attention_norm, wq|wk|wv,
        // q_norm / k_norm, rope, cache write, scores, softmax, P.V, wo (transformer.h:126-133, attention.h:170-205); the attention post-norm and its
        // residual are the w1|w3 GEMV's prologue (or a post_norm_attn step)
        postnorm_args h{};
        if (pn) {
            const auto it = pn_host.find(pn);
            if (it == pn_host.end()) return fail(MC_ERR_RUNTIME, "attention block: unknown post-norm descriptor");
            h = it->second;
        }
        a = pack(kc, vt, attn_out, attn_psum_g, attn_slab_g, attn_row_g, attn_qkv_g, state, (uint32_t)n_rep, (uint32_t)KV, S, scale_T, ns, tag, wo_w, wo_s, x, y,
                 (uint32_t)L.wo.out, (uint32_t)L.wo.group, an, qkv_w, qkv_s, rcos, rsin, cfg.norm_eps, mu, P.fast, none, qn, kn, (const void*)h.post_w,
                 (const void*)h.res, (void*)h.h_out);
        break;
    }
    case block_form::wo_qkn:
        // q_norm / k_norm, rope, cache write, scores, softmax, P.V, wo (attention.h:170-205) in ONE launch; the post-norm and the residual are the next
        // GEMV's prologue (or a post_norm_attn step)
        a = pack(x, kc, vt, attn_out, attn_psum_g, attn_slab_g, attn_row_g, state, (uint32_t)n_rep, (uint32_t)KV, S, scale_T, ns, tag, wo_w, wo_s,
                 (const void*)nullptr, y, (uint32_t)L.wo.out, (uint32_t)L.wo.group, (uint32_t)0, P.fast, none, qn, kn, rcos, rsin, cfg.norm_eps, mu);
        break;
    case block_form::wo_i4:
        // scores, softmax, P.V, wo + residual  (attention.h:191-205, transformer.h:132-133) in ONE launch
        a = pack(x, kc, vt, attn_out, attn_psum_g, attn_slab_g, attn_row_g, state, (uint32_t)n_rep, (uint32_t)KV, S, scale_T, ns, tag, wo_w, wo_s, res, y,
                 (uint32_t)L.wo.out, (uint32_t)L.wo.group, (uint32_t)(res ? 1 : 0), P.fast, none);
        break;
    case block_form::fused_qkn:
        // q_norm / k_norm, rope, cache write, scores, softmax, P.V (attention.h:170-203) in ONE launch, then Wo from the finished row
        a = pack(x, kc, vt, y, attn_psum_g, attn_slab_g, state, (uint32_t)n_rep, (uint32_t)KV, (uint32_t)hd, S, scale_T, ns, tag, P.fast, qn, kn, rcos, rsin,
                 cfg.norm_eps, mu);
        break;
    case block_form::fused:
    case block_form::fused_t2:
        // scores, softmax, P.V                 (attention.h:191-203) in ONE launch of 64- or 128-slot ranges, then Wo from the finished row
        a = pack(x, kc, vt, y, attn_psum_g, attn_slab_g, state, (uint32_t)n_rep, (uint32_t)KV, (uint32_t)hd, S, scale_T, ns, tag, none, P.fast);
        break;
    case block_form::scores_pv:
        // scores, softmax denominators         (attention.h:195-200); P.V follows as the `pv` step
        return launch(P.name, nsplit, KV, 1, 256, 0, pack(x, kc, expv, psum, none, state, (uint32_t)n_rep, (uint32_t)hd, S, scale_T, (uint32_t)nsplit));
    }
    return launch(P.name, P.grid, 1, 1, P.form == block_form::fused_qkn || P.form == block_form::fused || P.form == block_form::fused_t2 ? 256 : 512, 0, std::move(a));
}

mc_status
mc_decoder::run_step(const token_plan& P, const token_step& s, const void* in)
{
    if (!P.error.empty()) return fail(MC_ERR_RUNTIME, P.error);
    const int dim = cfg.dim, H = cfg.n_heads, KV = cfg.n_kv_heads, hd = cfg.head_dim;
    const bool gemma = cfg.family == MC_FAMILY_GEMMA3;
    const float mu = gemma ? 1.0f : 0.0f;
    const size_t row_bytes = (size_t)dim * tb;
    auto row = [&](token_row r) -> void* {
        switch (r) {
        case token_row::none: return nullptr;
        case token_row::in: return const_cast<void*>(in);
        case token_row::hidden: return hidden;
        case token_row::hidden_b: return hidden_b;
        case token_row::proj: return proj;
        case token_row::qkv: return qkv;
        case token_row::q_rot: return q_rot;
        case token_row::gate: return gate;
        case token_row::attn_out: return attn_out;
        case token_row::pv_parts: return pv_parts;
        case token_row::logits: return logits;
        }
        return nullptr;
    };
    layer_w* L = s.layer >= 0 ? &layers[s.layer] : nullptr;
    const token_launch& K = s.L;
    const void* res = nullptr;
    switch (s.res) {
    case token_res::none: break;
    case token_res::row: res = row(s.res_row); break;
    case token_res::qkv_epi: res = L->qkv_epi; break;
    case token_res::pn_attn: res = layers[s.res_layer].pn_attn; break;
    case token_res::pn_ffn: res = layers[s.res_layer].pn_ffn; break;
    case token_res::pick_atomic: res = pick_desc + offsetof(pick_block, atomic); break;
    case token_res::pick_per_wg: res = pick_desc + offsetof(pick_block, per_wg); break;
    }
    mc_status r = MC_OK;
    switch (s.op) {
    case token_op::park_row: MC_HIP(hipMemcpyAsync(hidden, row(s.x), row_bytes, hipMemcpyDeviceToDevice, stream)); break;
    case token_op::tap: MC_HIP(hipMemcpyAsync((char*)taps + (size_t)(s.layer + 1) * row_bytes, hidden, row_bytes, hipMemcpyDeviceToDevice, stream)); break;
    case token_op::embed: {
        float sc = std::sqrt((float)dim);
        if (tb == 2) sc = bf2f_host(f2bf_host(sc));
        const int32_t adv_seq = s.advance ? (int32_t)cfg.max_seq_len : 0; // (chained generation on a first stage: the embed also advances the step state)
        r = launch(K.name, K.gx, 1, 1, K.block, 0,
                   emb_fmt == MC_WFMT_T
                       ? pack(emb_table, hidden, state, (uint32_t)dim, sc, (int32_t)(gemma ? 1 : 0), adv_seq, (int32_t)pre_len,
                              s.fold_keys ? (const void*)pick_keys : (const void*)nullptr, (uint32_t)pick_slots, s.fold_keys ? tokens_dev : (int32_t*)nullptr)
                       : pack(emb_table, emb_scales, hidden, state, (uint32_t)dim, sc, (int32_t)(gemma ? 1 : 0), adv_seq, (int32_t)pre_len));
        break;
    }
    case token_op::qkv_gemv:
    case token_op::wo_gemv:
    case token_op::w13_gemv:
    case token_op::w2_gemv:
    case token_op::head_gemv: {
        const linear_w& W = s.op == token_op::head_gemv ? output : s.op == token_op::qkv_gemv ? L->qkv : s.op == token_op::wo_gemv ? L->wo
                          : s.op == token_op::w13_gemv ? L->w13 : L->w2;
        const void* norm_w = s.norm == token_norm::attention ? L->attention_norm : s.norm == token_norm::ffn ? L->ffn_norm
                           : s.norm == token_norm::final ? final_norm : nullptr;
        r = gemv_launch(s.adaptor ? *W.lora_a : W, K.name, K.gx, K.block, K.lds, s.pn_by_value, row(s.x), s.adaptor ? W.lora_vec : row(s.y), res, norm_w, mu);
        break;
    }
    case token_op::rope_kv:
        // gemma3: q_norm / k_norm per head, rope and the cache write as a launch of their own
        r = launch(K.name, K.gx, 1, 1, K.block, 0,
                   pack(qkv, q_rot, L->kc, L->vt, rope_cos[L->rope_table], rope_sin[L->rope_table], L->q_norm, L->k_norm, state, (uint32_t)H, (uint32_t)KV,
                        (uint32_t)hd, (uint32_t)cfg.max_seq_len, cfg.norm_eps, mu));
        break;
    case token_op::attn:
    case token_op::scores: r = attn_launch(*L, P.blocks[s.layer], row(s.x), row(s.y), res, s.res == token_res::pn_ffn ? res : nullptr); break;
    case token_op::pv:
        // softmax normalisation + P.V          (attention.h:200-203): over gz ranges of cache slots, their sums folded into Wo's prologue or added by pv_reduce
        r = launch(K.name, K.gx, K.gy, K.gz, K.block, 0,
                   pack(expv, psum, L->vt, attn_out, state, (uint32_t)(H / KV), (uint32_t)hd, (uint32_t)cfg.max_seq_len, (uint32_t)nsplit, pv_parts, (uint32_t)H));
        break;
    case token_op::pv_reduce:
        r = launch(K.name, K.gx, 1, 1, K.block, 0, pack((const void*)pv_parts, attn_out, (uint32_t)(H * hd), (uint32_t)P.blocks[s.layer].pv_ranges));
        break;
    case token_op::post_norm_attn:
    case token_op::post_norm_ffn: {
        // gemma3's post-norm of `proj` as a launch of its own: hidden = res + norm(proj) w
        const void* w = s.op == token_op::post_norm_attn ? L->attention_post_norm : L->ffn_post_norm;
        r = launch(K.name, 1, 1, 1, K.block, 0, pack(proj, w, (const void*)row(s.x), hidden, (uint32_t)dim, cfg.norm_eps, mu));
        break;
    }
    case token_op::fold_pick: r = fold_pick(); break;
    case token_op::argmax: r = launch(K.name, 1, 1, 1, K.block, 0, pack(logits, (uint32_t)cfg.vocab, state, tokens_dev)); break;
    case token_op::candidates: r = launch(K.name, K.gx, 1, 1, K.block, 0, pack(logits, (uint32_t)cfg.vocab, P.sampler.kpad, cand, P.sampler_chunk)); break;
    case token_op::sample:
        r = launch(K.name, 1, 1, 1, K.block, K.lds,
                   pack(cand, P.sampler, seeds, (uint32_t)n_seed_pairs, state, tokens_dev, want_taps ? sampler_taps : (float*)nullptr));
        break;
    }
    return r;
}

// everything one token needs after the state has been set.  advance: the embedding launch also advances the step state.  Each step is launched as it is
// planned (the planning of the later blocks runs while the device works); after a step that failed nothing more is launched.
mc_status
mc_decoder::run_token(const void* hidden_src, bool advance)
{
    token_plan P;
    mc_status st = MC_OK;
    plan_token(P, token_fixed_now(), token_now(advance, hidden_src == hidden), [&](const token_step& s) {
        if (st == MC_OK) st = run_step(P, s, hidden_src);
    });
    return st == MC_OK && !P.error.empty() ? fail(MC_ERR_RUNTIME, P.error) : st;
}

// the head and the pick alone, nothing pending in front: where the prompt pass ends
mc_status
mc_decoder::run_head()
{
    token_plan P;
    mc_status st = MC_OK;
    plan_head(P, token_fixed_now(), token_now(false, true), -1, [&](const token_step& s) {
        if (st == MC_OK) st = run_step(P, s, nullptr);
    });
    return st == MC_OK && !P.error.empty() ? fail(MC_ERR_RUNTIME, P.error) : st; // (a refusal that left no step: the sampler's)
}

namespace mcimpl {

mc_status
find_layer(mc_decoder* d, int32_t layer, layer_w** out)
{
    const int li = layer - d->cfg.layer_begin;
    if (li < 0 || li >= d->n_own)
        return fail(MC_ERR_INVALID_ARGUMENT, "decoder: layer is not owned by this stage");
    *out = &d->layers[li];
    return MC_OK;
}

mc_status
check_ready(mc_decoder* d)
{
    for (auto& L : d->layers)
        if (!L.qkv.allocated || !L.wo.allocated || !L.w13.allocated || !L.w2.allocated ||
            !L.attention_norm || !L.ffn_norm)
            return fail(MC_ERR_RUNTIME, "decoder: layer weights are not loaded");
    if (d->first_stage && !d->emb_table) return fail(MC_ERR_RUNTIME, "decoder: tok_embeddings not loaded");
    if (d->last_stage && (!d->output.allocated || !d->final_norm))
        return fail(MC_ERR_RUNTIME, "decoder: output head not loaded");
    if (d->cfg.family == MC_FAMILY_GEMMA3 && !d->pn_ready) {
        for (auto& L : d->layers) {
            if (!L.attention_post_norm || !L.ffn_post_norm) return fail(MC_ERR_RUNTIME, "decoder: post-norm weights are not loaded");
            const postnorm_args a{L.attention_post_norm, d->hidden, d->hidden_b};
            const postnorm_args f{L.ffn_post_norm, d->hidden_b, d->hidden};
            MC_HIP(hipMemcpy(L.pn_attn, &a, sizeof a, hipMemcpyHostToDevice));
            MC_HIP(hipMemcpy(L.pn_ffn, &f, sizeof f, hipMemcpyHostToDevice));
            d->pn_host[L.pn_attn] = a;
            d->pn_host[L.pn_ffn] = f;
        }
        d->pn_ready = true;
    }
    return MC_OK;
}

} // namespace mcimpl

// ------------------------------------------------------------------------------------------
extern "C" {

mc_status
mc_decoder_create(mc_device* dev, mc_library* lib, mc_queue* q, const mc_decoder_config* cfg,
                  mc_decoder** out)
{
    if (!dev || !lib || !q || !cfg || !out)
        return fail(MC_ERR_INVALID_ARGUMENT, "mc_decoder_create: null argument");
    const mc_decoder_config& c = *cfg;
    if (c.n_heads % c.n_kv_heads != 0 || c.n_heads / c.n_kv_heads > 16)
        return fail(MC_ERR_INVALID_ARGUMENT,
                    "decoder: n_heads must be a multiple of n_kv_heads with at most 16 query heads "
                    "per kv head");
    if (c.head_dim != 32 && c.head_dim != 64 && c.head_dim != 128 && c.head_dim != 256)
        return fail(MC_ERR_INVALID_ARGUMENT, "decoder: head_dim must be 32, 64, 128 or 256");
    if (c.max_seq_len % 8 != 0 || c.max_seq_len < 8)
        return fail(MC_ERR_INVALID_ARGUMENT, "decoder: max_seq_len must be a multiple of 8");
    if (c.layer_begin < 0 || c.layer_end > c.n_layers || c.layer_begin > c.layer_end)
        return fail(MC_ERR_INVALID_ARGUMENT, "decoder: bad layer range");
    MC_HIP(hipSetDevice(dev->ordinal));

    auto d = std::unique_ptr<mc_decoder>(new mc_decoder());
    d->cfg = c;
    d->dev = dev;
    d->lib = lib;
    d->q = q;
    d->stream = q->stream;
    d->tb = c.dtype == MC_DTYPE_BF16 ? 2 : 4;
    d->tname = c.dtype == MC_DTYPE_BF16 ? "bfloat" : "float";
    d->pre_len = c.sink_pre_len >= 0 ? c.sink_pre_len : bit_width((uint32_t)c.max_seq_len) - 1;
    if (d->pre_len >= c.max_seq_len)
        return fail(MC_ERR_INVALID_ARGUMENT, "decoder: sink prefix must be shorter than the cache");
    d->nsplit = (c.max_seq_len + PB - 1) / PB;
    d->n_own = c.layer_end - c.layer_begin;
    d->first_stage = c.layer_begin == 0;
    d->last_stage = c.layer_end == c.n_layers;
    d->opt = read_options();
    d->attn_fused_on = d->opt.attn_fused;
    d->rearm_after = d->opt.rearm_after;
    d->pf_lib_on = d->opt.pf_lib;

    const size_t tb = d->tb;
    const int dim = c.dim, H = c.n_heads, KV = c.n_kv_heads, hd = c.head_dim;
    mc_status s;
#define A(ptr, bytes)                                   \
    s = d->alloc((void**)&(ptr), (bytes));              \
    if (s != MC_OK) return s;
    A(d->hidden, dim * tb);
    A(d->hidden_in, dim * tb);
    A(d->hidden_b, dim * tb);
    A(d->qkv, (size_t)(H + 2 * KV) * hd * tb);
    A(d->q_rot, (size_t)H * hd * tb);
    A(d->attn_out, (size_t)H * hd * tb);
    A(d->proj, dim * tb);
    A(d->gate, (size_t)c.ffn_dim * tb);
    A(d->logits, (size_t)c.vocab * tb);
    A(d->expv, (size_t)H * c.max_seq_len * 4);
    A(d->psum, (size_t)H * d->nsplit * 4);
    // P.V: one whole-context launch of 16-wave workgroups while a wave has at most ~16 k-steps of 32
    // slots (four rounds of loads); from 8192 slots on, ranges of 2048 slots + one reduce launch
    // (S = 8192, int8 weights: 1 range 369, 2: 391, 4: 402, 8: 383, 16: 347 tokens/s)
    d->pv_ranges = c.max_seq_len >= 8192 ? std::min(16, c.max_seq_len / 2048) : 1;
    if (d->opt.pv_ranges) d->pv_ranges = d->opt.pv_ranges;
    A(d->pv_parts, (size_t)std::max(d->pv_ranges, 4) * H * hd * 4);
    if (d->tb == 2) {
        // (twice: the XCD-local `fast` copy of every granule sits behind the `slow` one, handoff.h)
        A(d->attn_psum_g, (size_t)H * d->nsplit * 8 * 2);
        A(d->attn_slab_g, (size_t)H * hd * d->nsplit * 8 * 2);
        A(d->attn_row_g, (size_t)H * hd / 2 * 8);
        A(d->attn_hid_g, (size_t)dim / 2 * 8);
        A(d->attn_qkv_g, (size_t)(H + 2 * std::max(KV, 8)) * hd / 2 * 8 * 2); // (virtual kv heads: a K and a V row per virtual head)
    }
    // what the plans of the decode launches see of this decoder (gemv_plan.h, block_plan.h); the occupancy answers follow with the first step
    d->benv = block_env{gemv_env{d->tb, (int)c.qmode, (unsigned)dev->prop.multiProcessorCount, mc_decoder::pick_slots, &d->opt}, d->nsplit, d->n_own,
                        d->attn_psum_g != nullptr, d->pv_ranges, d->tname, block_occupancy{}};
    A(d->taps, (size_t)(d->n_own + 1) * dim * tb);
    A(d->state, sizeof(step_state));
    A(d->state_bak, sizeof(step_state));
    if (hipHostMalloc((void**)&d->err_host, 64, hipHostMallocDefault) == hipSuccess) {
        *d->err_host = 0;
        if (hipEventCreateWithFlags(&d->err_evt, hipEventDisableTiming) != hipSuccess) {
            (void)hipHostFree(d->err_host);
            d->err_host = nullptr;
        }
    }
    (void)hipGetLastError();
    d->tokens_cap = 1 << 16;
    A(d->tokens_dev, (size_t)d->tokens_cap * 4);
    A(d->pick_desc, sizeof(pick_block));
    A(d->pick_keys, (size_t)mc_decoder::pick_slots * 8);
    {
        pick_block blk{};
        blk.atomic = {(unsigned long long*)(d->pick_desc + offsetof(pick_block, key)), (uint32_t*)(d->pick_desc + offsetof(pick_block, ticket)),
                     d->state, d->tokens_dev};
        blk.per_wg = {(unsigned long long*)d->pick_keys, nullptr, d->state, d->tokens_dev};
        MC_HIP(hipMemcpy(d->pick_desc, &blk, sizeof blk, hipMemcpyHostToDevice));
    }
    d->rope_rows = 2 * c.max_seq_len; // nn/embedding.h:171: _M_seq_len(max_seq_len * 2)
    A(d->rope_cos[0], (size_t)d->rope_rows * (hd / 2) * 4);
    A(d->rope_sin[0], (size_t)d->rope_rows * (hd / 2) * 4);
    if (c.family == MC_FAMILY_GEMMA3 && c.rope_sliding_theta > 0.0f) {
        A(d->rope_cos[1], (size_t)d->rope_rows * (hd / 2) * 4);
        A(d->rope_sin[1], (size_t)d->rope_rows * (hd / 2) * 4);
    }
    d->layers.resize(d->n_own);
    for (int i = 0; i < d->n_own; i++) {
        layer_w& L = d->layers[i];
        const size_t cache_bytes = (size_t)KV * c.max_seq_len * hd * tb;
        A(L.kc, cache_bytes);
        A(L.vt, cache_bytes);
        const int gi = c.layer_begin + i;
        // nn/gemma.h:69-73: sliding iff (i + 1) % sliding_stride != 0
        L.rope_table = (c.family == MC_FAMILY_GEMMA3 && c.sliding_stride > 0 &&
                        ((gi + 1) % c.sliding_stride) != 0 && d->rope_cos[1])
                           ? 1
                           : 0;
        qkv_epilogue e{d->q_rot, L.kc, L.vt, d->rope_cos[L.rope_table], d->rope_sin[L.rope_table], d->state, (uint32_t)H, (uint32_t)KV,
                       (uint32_t)hd, (uint32_t)c.max_seq_len};
        A(L.qkv_epi, sizeof e);
        MC_HIP(hipMemcpyAsync(L.qkv_epi, &e, sizeof e, hipMemcpyHostToDevice, d->stream));
        MC_HIP(hipStreamSynchronize(d->stream)); // `e` is a stack temporary
        A(L.pn_attn, sizeof(postnorm_args));
        A(L.pn_ffn, sizeof(postnorm_args));
    }
#undef A
    MC_HIP(hipStreamSynchronize(d->stream));
    *out = d.release();
    return MC_OK;
}

void
mc_decoder_release(mc_decoder* d)
{
    delete d;
}

mc_status
mc_decoder_set_sampler(mc_decoder* d, int32_t kind, int32_t top_k, float temperature, float top_p)
{
    if (!d) return fail(MC_ERR_INVALID_ARGUMENT, "mc_decoder_set_sampler: null argument");
    if (kind != MC_SAMPLER_GREEDY && kind != MC_SAMPLER_DEFAULT && kind != MC_SAMPLER_DRAW)
        return fail(MC_ERR_INVALID_ARGUMENT, "mc_decoder_set_sampler: unknown sampler");
    if (kind != MC_SAMPLER_GREEDY) { // MC_SAMPLER_DRAW shares the chain: the same checks, texts, rounding and allocations
        // the argument checks of nucleus_sampler (nn/sampling.h:165-174)
        if (!(temperature > 0.0f)) return fail(MC_ERR_INVALID_ARGUMENT, "nucleus_sampler: temperature must be positive");
        if (top_p < 0.0f || top_p > 1.0f)
            return fail(MC_ERR_INVALID_ARGUMENT, "nucleus_sampler: probability must be in [0.0, 1.0]");
        if (top_k < 1 || top_k > 128)
            return fail(MC_ERR_INVALID_ARGUMENT, "topk_sampler: the fused sampler keeps 1..128 candidates");
        if (!d->last_stage) return fail(MC_ERR_INVALID_ARGUMENT, "decoder: only the last stage samples");
        MC_HIP(hipSetDevice(d->dev->ordinal));
        d->drop_graph();
        const uint32_t chunks = ((uint32_t)d->cfg.vocab + 511u) / 512u; // (the most lists any top_k makes: sampler_plan)
        if (!d->cand) {
            mc_status s = d->alloc((void**)&d->cand, (size_t)chunks * 128 * 8);
            if (s != MC_OK) return s;
            s = d->alloc((void**)&d->sampler_taps, 7 * 128 * 4);
            if (s != MC_OK) return s;
        }
        const bool bf = d->tb == 2;
        auto rt = [&](float v) { return bf ? bf2f_host(f2bf_host(v)) : v; };
        d->top_k = top_k;
        d->inv_temp_T = rt(1.0f / rt(temperature)); // T temp = T(1) / _M_temperature  (sampling.h:190)
        d->top_p_T = rt(top_p);
    } else {
        d->drop_graph();
    }
    d->sampler_kind = kind;
    return MC_OK;
}

mc_status
mc_decoder_set_seeds(mc_decoder* d, const uint64_t* seeds, int32_t n_pairs)
{
    if (!d || (n_pairs > 0 && !seeds)) return fail(MC_ERR_INVALID_ARGUMENT, "mc_decoder_set_seeds: null argument");
    if (n_pairs < 0) return fail(MC_ERR_INVALID_ARGUMENT, "mc_decoder_set_seeds: negative count");
    MC_HIP(hipSetDevice(d->dev->ordinal));
    if (n_pairs > d->seed_cap) {
        d->drop_graph(); // pointer changes
        mc_status s = d->alloc((void**)&d->seeds, (size_t)n_pairs * 16);
        if (s != MC_OK) return s;
        d->seed_cap = n_pairs;
    }
    if (n_pairs) MC_HIP(hipMemcpy(d->seeds, seeds, (size_t)n_pairs * 16, hipMemcpyHostToDevice));
    if (n_pairs != d->n_seed_pairs) d->drop_graph();
    d->n_seed_pairs = n_pairs;
    return MC_OK;
}

mc_status
mc_decoder_get_sampler_taps(mc_decoder* d, float* out_7xk)
{
    if (!d || !out_7xk) return fail(MC_ERR_INVALID_ARGUMENT, "mc_decoder_get_sampler_taps: null argument");
    if (d->sampler_kind == MC_SAMPLER_GREEDY || !d->sampler_taps)
        return fail(MC_ERR_INVALID_ARGUMENT, "decoder: the default sampler is not active");
    MC_HIP(hipSetDevice(d->dev->ordinal));
    MC_HIP(hipStreamSynchronize(d->stream));
    const int k = std::min(d->top_k, d->cfg.vocab);
    MC_HIP(hipMemcpy(out_7xk, d->sampler_taps, (size_t)7 * k * 4, hipMemcpyDeviceToHost));
    return MC_OK;
}

mc_status
mc_decoder_get_config(const mc_decoder* d, mc_decoder_config* out)
{
    if (!d || !out) return fail(MC_ERR_INVALID_ARGUMENT, "mc_decoder_get_config: null argument");
    *out = d->cfg;
    return MC_OK;
}

mc_status
mc_decoder_step(mc_decoder* d, int32_t token, int32_t start_pos, const void* hidden_in,
                int32_t* next_token)
{
    if (!d) return fail(MC_ERR_INVALID_ARGUMENT, "mc_decoder_step: null argument");
    mc_status s = check_ready(d);
    if (s != MC_OK) return s;
    if (start_pos < 0) return fail(MC_ERR_INVALID_ARGUMENT, "decoder: negative start position");
    // token < 0 keeps the token the previous step left in the state (and means nothing to a later stage)
    if (d->first_stage && token >= d->cfg.vocab)
        return fail(MC_ERR_INVALID_ARGUMENT, "decoder: token id outside the vocabulary");
    if (!d->first_stage && !hidden_in)
        return fail(MC_ERR_INVALID_ARGUMENT, "decoder: a non-first stage needs the inbound hidden row");
    MC_HIP(hipSetDevice(d->dev->ordinal));
    s = d->poll_pending_err();
    if (s != MC_OK) return s;
    d->query_occupancy();
    for (int attempt = 0;; attempt++) {
        const bool handoffs = d->uses_handoffs();
        // (a step whose hand-offs give up is repeated on the launches that need no co-residency: the state in front of it)
        if (handoffs) MC_HIP(hipMemcpyAsync(d->state_bak, d->state, sizeof(step_state), hipMemcpyDeviceToDevice, d->stream));
        s = d->ensure_rope(start_pos);
        if (s != MC_OK) return s;
        s = d->launch("mc_step_set", 1, 1, 1, 64, 0,
                      pack(d->state, token, start_pos, (int32_t)d->cfg.max_seq_len, (int32_t)d->pre_len,
                           (int32_t)d->rope_start, (int32_t)(start_pos == 0 ? 1 : 0)));
        if (s != MC_OK) return s;
        s = d->run_token(d->first_stage ? nullptr : hidden_in);
        if (s != MC_OK) return s;
        d->last_pos = start_pos;
        if (start_pos == 0) d->ring_turned = false;
        if (start_pos >= d->cfg.max_seq_len) d->ring_turned = true;
        if (!(next_token && d->last_stage)) {
            // nobody waits for this step: its flag is copied out behind it and looked at by the calls that follow (poll_pending_err)
            // and by every call that synchronises (check_err_synced); a set flag makes THAT call fail and latches the decoder
            if (handoffs) d->note_err_async();
            d->note_clean_tokens(1);
            return MC_OK;
        }
        step_state st;
        MC_HIP(hipMemcpyAsync(&st, d->state, sizeof st, hipMemcpyDeviceToHost, d->stream));
        MC_HIP(hipStreamSynchronize(d->stream));
        *next_token = st.token;
        if (!st.err) {
            d->note_clean_tokens(1);
            return MC_OK;
        }
        if (attempt > 0 || !handoffs) return d->check_handoffs(st);
        // the step again, from the state in front of it: its cache row goes to the same slot, every other row is untouched
        d->handoff_failed();
        MC_HIP(hipMemcpyAsync(d->state, d->state_bak, sizeof(step_state), hipMemcpyDeviceToDevice, d->stream));
    }
}

mc_status
mc_decoder_generate(mc_decoder* d, int32_t first_token, int32_t start_pos, int32_t n,
                    int32_t* tokens_out)
{
    if (!d || n <= 0) return fail(MC_ERR_INVALID_ARGUMENT, "mc_decoder_generate: bad argument");
    if (!d->first_stage || !d->last_stage)
        return fail(MC_ERR_INVALID_ARGUMENT, "mc_decoder_generate: single-stage decoders only");
    if (n > d->tokens_cap) return fail(MC_ERR_INVALID_ARGUMENT, "mc_decoder_generate: n too large");
    if (first_token >= d->cfg.vocab) return fail(MC_ERR_INVALID_ARGUMENT, "decoder: token id outside the vocabulary");
    if (start_pos < 0) return fail(MC_ERR_INVALID_ARGUMENT, "decoder: negative start position");
    mc_status s = check_ready(d);
    if (s != MC_OK) return s;
    MC_HIP(hipSetDevice(d->dev->ordinal));
    s = d->poll_pending_err();
    if (s != MC_OK) return s;
    d->query_occupancy();
    const bool handoffs = d->uses_handoffs();
    if (handoffs) MC_HIP(hipMemcpyAsync(d->state_bak, d->state, sizeof(step_state), hipMemcpyDeviceToDevice, d->stream));
    s = d->ensure_rope(start_pos);
    if (s != MC_OK) return s;
    s = d->launch("mc_step_set", 1, 1, 1, 64, 0,
                  pack(d->state, first_token, start_pos, (int32_t)d->cfg.max_seq_len,
                       (int32_t)d->pre_len, (int32_t)d->rope_start, (int32_t)(start_pos == 0 ? 1 : 0)));
    if (s != MC_OK) return s;
    // step_index restarts at 0 for every generate call
    MC_HIP(hipMemsetAsync(&d->state->step_index, 0, 4, d->stream));
    if (start_pos == 0) d->ring_turned = false;
    if (start_pos + n > d->cfg.max_seq_len) d->ring_turned = true;
    // the head leaves one key per workgroup; the fold into a token is done by the NEXT token's embedding launch (every
    // workgroup of it folds the 2 KB itself) and by one mc_argmax_keys launch behind the LAST token of the call: a launch
    // less per token (4.7 us of 1240)
    struct lazy_scope {
        mc_decoder* d;
        ~lazy_scope() { d->lazy_pick = false; }
    } lazy_guard{d};
    {
        const token_fixed f = d->token_fixed_now();
        const token_state now = d->token_now(false, true);
        d->lazy_pick = lazy_pick_ok(f, now, head_behind_post_norm(f, now)); // (one answer: the head's own plan asks the same question of the same inputs)
    }
    s = d->run_token(nullptr);
    if (s != MC_OK) return s;
    for (int i = 1; i < n; i++) {
        const int pos = start_pos + i;
        s = d->ensure_rope(pos); // moves the table window when pos leaves it (the step state carries the new start)
        if (s != MC_OK) return s;
        if (d->cfg.use_graph) {
            if (d->graph_exec && d->graph_lazy != d->lazy_pick) d->drop_graph();
            if (!d->graph_exec) {
                d->drop_graph();
                d->graph_lazy = d->lazy_pick;
                MC_HIP(hipStreamBeginCapture(d->stream, hipStreamCaptureModeGlobal));
                mc_status s2 = d->run_token(nullptr, true); // the embedding launch advances the step state

                hipError_t e = hipStreamEndCapture(d->stream, &d->graph);
                if (s2 != MC_OK) return s2;
                if (e != hipSuccess) return hip_fail(e, "hipStreamEndCapture");
                MC_HIP(hipGraphInstantiate(&d->graph_exec, d->graph, nullptr, nullptr, 0));
            }
            MC_HIP(hipGraphLaunch(d->graph_exec, d->stream));
        } else {
            s = d->run_token(nullptr, true);
            if (s != MC_OK) return s;
        }
    }
    if (d->lazy_pick) {
        s = d->fold_pick(); // the last token's pick
        if (s != MC_OK) return s;
        d->lazy_pick = false;
    }
    d->last_pos = start_pos + n - 1;
    if (tokens_out) {
        MC_HIP(hipMemcpyAsync(tokens_out, d->tokens_dev, (size_t)n * 4, hipMemcpyDeviceToHost, d->stream));
    }
    step_state st;
    MC_HIP(hipMemcpyAsync(&st, d->state, sizeof st, hipMemcpyDeviceToHost, d->stream));
    MC_HIP(hipStreamSynchronize(d->stream));
    if (!st.err) {
        d->note_clean_tokens(n);
        return MC_OK;
    }
    // A hand-off gave up somewhere in the chain.  While the ring has not turned inside this call every row the chain wrote sits
    // behind kv_len of the state in front of it: the call is repeated from there, exactly, on the launches that need no
    // co-residency.  Past max_seq_len the failed chain has overwritten rows its own first steps attend to: reported instead.
    if (handoffs && start_pos + n <= d->cfg.max_seq_len) {
        d->handoff_failed();
        MC_HIP(hipMemcpyAsync(d->state, d->state_bak, sizeof(step_state), hipMemcpyDeviceToDevice, d->stream));
        return mc_decoder_generate(d, first_token, start_pos, n, tokens_out);
    }
    return d->check_handoffs(st);
}

int32_t
mc_decoder_handoff_fallbacks(const mc_decoder* d)
{
    return d ? d->handoff_fallbacks : 0;
}

int32_t
mc_decoder_handoff_rearms(const mc_decoder* d)
{
    return d ? d->handoff_rearms : 0;
}

int32_t
mc_decoder_handoffs_active(const mc_decoder* d)
{
    return d && d->attn_fused_on ? 1 : 0;
}

void*
mc_decoder_hidden_out(mc_decoder* d)
{
    return d->hidden;
}

void*
mc_decoder_hidden_in(mc_decoder* d)
{
    return d->hidden_in;
}

mc_status
mc_decoder_set_taps(mc_decoder* d, int32_t enable)
{
    if (!d) return fail(MC_ERR_INVALID_ARGUMENT, "mc_decoder_set_taps: null argument");
    if (d->want_taps != (enable != 0)) {
        // taps change the launch sequence (tap copies, unfused gemma post-norms, sampler tap pointer): a captured
        // token no longer matches
        MC_HIP(hipSetDevice(d->dev->ordinal));
        d->drop_graph();
    }
    d->want_taps = enable != 0;
    return MC_OK;
}

mc_status
mc_decoder_get_logits(mc_decoder* d, void* out)
{
    MC_HIP(hipSetDevice(d->dev->ordinal));
    MC_HIP(hipStreamSynchronize(d->stream));
    MC_HIP(hipMemcpy(out, d->logits, (size_t)d->cfg.vocab * d->tb, hipMemcpyDeviceToHost));
    return d->check_err_synced(); // (a step nobody waited for: its hand-offs are looked at where its results are read)
}

mc_status
mc_decoder_get_hidden(mc_decoder* d, int32_t layer, void* out)
{
    // layer = global layer index, -1 = embedding output; only meaningful with taps enabled
    const int li = layer - d->cfg.layer_begin + 1;
    if (li < 0 || li > d->n_own) return fail(MC_ERR_INVALID_ARGUMENT, "decoder: tap out of range");
    if (!d->want_taps) return fail(MC_ERR_RUNTIME, "decoder: taps are disabled (mc_decoder_set_taps)");
    MC_HIP(hipSetDevice(d->dev->ordinal));
    MC_HIP(hipStreamSynchronize(d->stream));
    MC_HIP(hipMemcpy(out, (char*)d->taps + (size_t)li * d->cfg.dim * d->tb, (size_t)d->cfg.dim * d->tb,
                     hipMemcpyDeviceToHost));
    return d->check_err_synced();
}

mc_status
mc_decoder_export_kv(mc_decoder* d, int32_t layer, void* keys, void* values, int32_t* n_valid)
{
    layer_w* L;
    mc_status s = find_layer(d, layer, &L);
    if (s != MC_OK) return s;
    MC_HIP(hipSetDevice(d->dev->ordinal));
    const mc_decoder_config& c = d->cfg;
    const size_t bytes = (size_t)c.max_seq_len * c.n_kv_heads * c.head_dim * d->tb;
    device_tmp kt, vtmp;
    MC_HIP(kt.alloc(bytes));
    MC_HIP(vtmp.alloc(bytes));
    s = d->launch("mc_kv_export_" + d->tname, 512, 1, 1, 256, 0,
                  pack(L->kc, L->vt, kt.ptr, vtmp.ptr, d->state, (uint32_t)c.n_kv_heads, (uint32_t)c.head_dim,
                       (uint32_t)c.max_seq_len, (uint32_t)d->pre_len));
    step_state st{};
    hipError_t e = hipStreamSynchronize(d->stream);
    if (s == MC_OK && e == hipSuccess) {
        e = hipMemcpy(&st, d->state, sizeof st, hipMemcpyDeviceToHost);
        const size_t nb = (size_t)st.kv_len * c.n_kv_heads * c.head_dim * d->tb;
        if (e == hipSuccess) e = hipMemcpy(keys, kt.ptr, nb, hipMemcpyDeviceToHost);
        if (e == hipSuccess) e = hipMemcpy(values, vtmp.ptr, nb, hipMemcpyDeviceToHost);
        if (n_valid) *n_valid = st.kv_len;
    }
    if (s != MC_OK) return s;
    if (e != hipSuccess) return hip_fail(e, "mc_decoder_export_kv");
    return st.err ? d->report_handoff(st.err) : MC_OK;
}

mc_status
mc_decoder_import_kv(mc_decoder* d, int32_t layer, const void* keys, const void* values, int32_t n_valid)
{
    if (!d || !keys || !values) return fail(MC_ERR_INVALID_ARGUMENT, "mc_decoder_import_kv: null argument");
    layer_w* L;
    mc_status s = find_layer(d, layer, &L);
    if (s != MC_OK) return s;
    const mc_decoder_config& c = d->cfg;
    if (n_valid < 1 || n_valid > c.max_seq_len)
        return fail(MC_ERR_INVALID_ARGUMENT, "mc_decoder_import_kv: n_valid must lie in [1, max_seq_len]");
    MC_HIP(hipSetDevice(d->dev->ordinal));
    const size_t nb = (size_t)n_valid * c.n_kv_heads * c.head_dim * d->tb;
    device_tmp kt, vtmp;
    MC_HIP(kt.alloc(nb));
    hipError_t e = vtmp.alloc(nb);
    if (e == hipSuccess) e = hipMemcpy(kt.ptr, keys, nb, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(vtmp.ptr, values, nb, hipMemcpyHostToDevice);
    if (e == hipSuccess) {
        s = d->launch("mc_kv_import_" + d->tname, 512, 1, 1, 256, 0,
                      pack(L->kc, L->vt, (const void*)kt.ptr, (const void*)vtmp.ptr, (uint32_t)n_valid, (uint32_t)c.n_kv_heads,
                           (uint32_t)c.head_dim, (uint32_t)c.max_seq_len));
        // the state of a decoder that has just decoded position n_valid - 1 on an unturned ring
        if (s == MC_OK)
            s = d->launch("mc_step_set", 1, 1, 1, 64, 0,
                          pack(d->state, (int32_t)-1, (int32_t)(n_valid - 1), (int32_t)c.max_seq_len, (int32_t)d->pre_len,
                               (int32_t)d->rope_start, (int32_t)1));
        e = hipStreamSynchronize(d->stream);
    }
    if (e != hipSuccess) return hip_fail(e, "mc_decoder_import_kv");
    if (s != MC_OK) return s;
    d->ring_turned = false;
    d->last_pos = n_valid - 1;
    return MC_OK;
}

mc_status
mc_decoder_launch_log(mc_decoder* d, int32_t enable)
{
    if (!d) return fail(MC_ERR_INVALID_ARGUMENT, "mc_decoder_launch_log: null argument");
    d->launch_log.clear();
    d->log_on = enable != 0;
    if (d->log_on) {
        // a replayed graph would launch without passing through the log: the next chained token is captured anew
        MC_HIP(hipSetDevice(d->dev->ordinal));
        d->drop_graph();
    }
    return MC_OK;
}

size_t
mc_decoder_launch_log_read(mc_decoder* d, char* buf, size_t cap)
{
    if (!d) return 0;
    std::string all;
    for (const std::string& n : d->launch_log) {
        all += n;
        all += '\n';
    }
    if (buf && cap) {
        const size_t n = std::min(cap - 1, all.size());
        memcpy(buf, all.data(), n);
        buf[n] = 0;
    }
    return all.size() + 1;
}

// The decode GEMVs of one pass of mc_decoder_time_gemv(which), in launch order: "qkv", "wo", "w13", "w2" of every owned block (MC_TIME_GEMV_LAYERS=n: with the
// weights of block i % n), then "head" on the last stage; "all" = every one.  Each is the pair the token's table names (token_plan.h gemv_use_of) BEHIND THE
// PLAIN NORM: no post-norm in front, the partial-sum prologue when P.V is folded, the head with the greedy pick inside where head_pick_ok() says so.  The
// buffers are this table's own: Wo and w2 store into `proj`, so the hidden row stays what it was, and the pick leaves one key per workgroup in pick_keys
// whatever MC_HEAD_PICK says (the step state is not touched).
struct timed_gemv {
    const char* which;
    const linear_w* L;
    int pro, epi;
    const void* x;
    void* y;
    const void* res;
    const void* norm_w;
};
static std::vector<timed_gemv>
timed_gemvs(mc_decoder* d, const std::string& w)
{
    const bool gemma = d->cfg.family == MC_FAMILY_GEMMA3;
    const size_t lim = d->opt.time_gemv_layers ? (size_t)d->opt.time_gemv_layers : d->layers.size(); // (MC_TIME_GEMV_LAYERS)
    std::vector<timed_gemv> out;
    auto add = [&](const char* which, const linear_w& W, const layer_w* L, const gemv_use& u, const void* x, void* y) {
        if (w != "all" && w != which) return;
        const void* res = u.res == token_res::row ? d->hidden : u.res == token_res::qkv_epi ? L->qkv_epi
                        : u.res == token_res::none ? nullptr : (const void*)(d->pick_desc + offsetof(pick_block, per_wg));
        const void* norm_w = u.norm == token_norm::attention ? L->attention_norm : u.norm == token_norm::ffn ? L->ffn_norm
                           : u.norm == token_norm::final ? d->final_norm : nullptr;
        out.push_back({which, &W, u.pro, u.epi, x, y, res, norm_w});
    };
    for (size_t li = 0; li < d->layers.size(); li++) {
        const layer_w& L = d->layers[li % lim];
        const bool fold = !d->uses_handoffs() && pv_fold(mc_decoder::shape_of(L.wo), d->model(), d->benv);
        add("qkv", L.qkv, &L, gemv_use_of(gemv_role::qkv, gemma, false), d->hidden, d->qkv);
        add("wo", L.wo, &L, gemv_use_of(gemv_role::wo, gemma, false, fold), fold ? (const void*)d->pv_parts : (const void*)d->attn_out, d->proj);
        add("w13", L.w13, &L, gemv_use_of(gemv_role::w13, gemma, false), d->hidden, d->gate);
        add("w2", L.w2, &L, gemv_use_of(gemv_role::w2, gemma, false), d->gate, d->proj);
    }
    if (d->last_stage) {
        const bool pick = head_pick_ok(d->token_fixed_now(), d->token_now(false, true), false);
        add("head", d->output, nullptr, gemv_use_of(gemv_role::head, gemma, false, false, pick ? 2 : 0), d->hidden, d->logits);
    }
    return out;
}

mc_status
mc_decoder_gemv_kernel_name(mc_decoder* d, const char* which, char* buf, size_t cap)
{
    if (!d || !which || !buf || !cap) return fail(MC_ERR_INVALID_ARGUMENT, "mc_decoder_gemv_kernel_name: bad argument");
    std::string name;
    if (std::string(which) == "attn") {
        // the decode attention of the first owned block: one launch with Wo, one launch, or scores + P.V (plan_block)
        mc_status s0 = check_ready(d);
        if (s0 != MC_OK) return s0;
        if (d->layers.empty()) return fail(MC_ERR_INVALID_ARGUMENT, "mc_decoder_gemv_kernel_name: this stage owns no block");
        d->query_occupancy();
        const block_plan P = d->plan_block(d->layers[0]);
        name = P.form == block_form::scores_pv ? P.name + " + mc_attn_pv_" + d->tname : P.name;
        const size_t n0 = std::min(cap - 1, name.size());
        memcpy(buf, name.data(), n0);
        buf[n0] = 0;
        return MC_OK;
    }
    mc_status s = check_ready(d);
    if (s != MC_OK) return s;
    const std::vector<timed_gemv> table = timed_gemvs(d, which);
    if (table.empty()) return fail(MC_ERR_INVALID_ARGUMENT, std::string("mc_decoder_gemv_kernel_name: no such GEMV '") + which + "'");
    const timed_gemv& g = table.front();
    const gemv_plan P = plan_gemv(mc_decoder::shape_of(*g.L), d->benv.g, g.pro, g.epi);
    if (P.error) return fail(MC_ERR_RUNTIME, P.error);
    const size_t n = std::min(cap - 1, P.name.size());
    memcpy(buf, P.name.data(), n);
    buf[n] = 0;
    return MC_OK;
}

mc_status
mc_decoder_time_gemv(mc_decoder* d, const char* which, int32_t repeats, float* total_ms,
                     double* bytes_per_pass, int32_t* launches_per_pass)
{
    if (!d || !which || repeats <= 0)
        return fail(MC_ERR_INVALID_ARGUMENT, "mc_decoder_time_gemv: bad argument");
    mc_status s = check_ready(d);
    if (s != MC_OK) return s;
    MC_HIP(hipSetDevice(d->dev->ordinal));
    const float mu = d->cfg.family == MC_FAMILY_GEMMA3 ? 1.0f : 0.0f;
    const std::vector<timed_gemv> table = timed_gemvs(d, which);
    double bytes = 0;
    for (const timed_gemv& g : table) bytes += linear_bytes(*g.L);
    auto pass = [&]() -> mc_status {
        for (const timed_gemv& g : table) {
            mc_status r = d->gemv(*g.L, g.pro, g.epi, g.x, g.y, g.res, g.norm_w, mu);
            if (r != MC_OK) return r;
        }
        return MC_OK;
    };
    s = pass(); // warm-up
    if (s != MC_OK) return s;
    MC_HIP(hipEventRecord(d->q->t0, d->stream));
    for (int i = 0; i < repeats; i++) {
        s = pass();
        if (s != MC_OK) return s;
    }
    MC_HIP(hipEventRecord(d->q->t1, d->stream));
    MC_HIP(hipEventSynchronize(d->q->t1));
    MC_HIP(hipEventElapsedTime(total_ms, d->q->t0, d->q->t1));
    if (bytes_per_pass) *bytes_per_pass = bytes;
    if (launches_per_pass) *launches_per_pass = (int32_t)table.size();
    return MC_OK;
}

} // extern "C"

// ------------------------------------------------------------------------------------------------
// What the batched decode (batch_impl.h and its units) reads of a decoder: decoder_batch.h
// ------------------------------------------------------------------------------------------------
namespace mcimpl {

static batch_linear
batch_view(const linear_w& L)
{
    batch_linear b;
    b.fmt = L.fmt;
    b.out = L.out;
    b.in = L.in;
    b.group = L.group;
    b.ngroups = L.ngroups;
    b.w = L.w;
    b.scales = L.scales;
    b.lora = L.lora_cols != 0;
    if (b.lora) {
        b.lora_a = L.lora_a->w;
        b.lora_b = L.lora_b;
        b.lora_cols = L.lora_cols;
        b.lora_scale = L.lora_scale;
    }
    return b;
}

mc_status
decoder_parts_of(mc_decoder* d, decoder_parts* out)
{
    mc_status s = check_ready(d);
    if (s != MC_OK) return s;
    out->cfg = d->cfg;
    out->ordinal = d->dev->ordinal;
    out->stream = d->stream;
    out->pre_len = d->pre_len;
    out->emb_fmt = d->emb_fmt;
    out->emb_table = d->emb_table;
    out->emb_scales = d->emb_scales;
    out->output = batch_view(d->output);
    out->final_norm = d->final_norm;
    out->layers.clear();
    for (const layer_w& L : d->layers) {
        batch_layer b;
        b.qkv = batch_view(L.qkv);
        b.wo = batch_view(L.wo);
        b.w13 = batch_view(L.w13);
        b.w2 = batch_view(L.w2);
        b.attention_norm = L.attention_norm;
        b.ffn_norm = L.ffn_norm;
        b.kc = L.kc;
        b.vt = L.vt;
        out->layers.push_back(b);
    }
    return MC_OK;
}

decoder_sampler
decoder_sampler_of(const mc_decoder* d)
{
    decoder_sampler s;
    s.kind = d->sampler_kind;
    s.top_k = d->top_k;
    s.inv_temp_T = d->inv_temp_T;
    s.top_p_T = d->top_p_T;
    return s;
}

mc_status
decoder_cache_state(mc_decoder* d, int* kv_len, bool* rolled)
{
    MC_HIP(hipSetDevice(d->dev->ordinal));
    step_state st{};
    MC_HIP(hipMemcpyAsync(&st, d->state, sizeof st, hipMemcpyDeviceToHost, d->stream));
    MC_HIP(hipStreamSynchronize(d->stream));
    *kv_len = st.kv_len;
    *rolled = d->ring_turned || st.rolled != 0 || st.ring_base != 0;
    return MC_OK;
}

mc_status
decoder_launch(mc_decoder* d, const std::string& name, unsigned gx, unsigned gy, unsigned gz, unsigned bx, unsigned lds, arg_pack&& args)
{
    return d->launch(name, gx, gy, gz, bx, lds, std::move(args));
}

} // namespace mcimpl
