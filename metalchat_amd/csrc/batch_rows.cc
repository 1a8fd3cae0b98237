// The batch's rows passes (Parts 2d to 2g; the map of the whole: batch_impl.h): mc_rows_prefill, mc_extend_rows, mc_verify_rows and
// mc_tree_verify through one body, rows_pass -- the admission and the tables are rows_plan.h's, the prompt pass the decoder's, the head behind it
// the batch's own (head(), or verify_head() with what plan_verify_head plans) -- and mc_verify_get_logits; Part 2m's switch
// (mc_settings_verify_set), with which verify_head() also processes, samples and counts per packed row (plan_verify_pick, plan_verify_logits).
#include "batch_impl.h"

using namespace mcimpl;

// mc_verify_rows: the final norm, the head and a greedy pick for each of the M packed rows `xrows` of a call, then per segment
// the acceptance of its drafts (`tokens`: the call's ids on the device) and the accepted row's logits into logits[row].
// nodes (mc_tree_verify): the chunks are trees -- the walk in place of the prefix rule, then the accepted path's K / V
// moved into place in every layer, both reading the device's own results
mc_status
mc_batch::verify_head(const void* xrows, const int32_t* tokens, int M, int nseg, const tv_node* nodes)
{
    const mc_decoder_config& c = p.cfg;
    const batch_linear& L = p.output;
    const verify_plan v = plan_verify_head(L, c, (int)p.layers.size(), M, nseg, nodes != nullptr);
    mc_status s = launch(v.norm, pack(xrows, p.final_norm, v_xn, (uint32_t)c.dim, c.norm_eps));
    if (s != MC_OK) return s;
    s = launch(v.head, pack(L.w, L.scales, (const void*)v_xn, v_logits, (uint32_t)L.in, (uint32_t)L.ngroups, (uint32_t)L.group, (uint32_t)M,
                            (uint32_t)L.out, (uint32_t)c.vocab));
    if (s != MC_OK) return s;
    int32_t* picks = v_out + 2 * B;
    // Part 2m: the rows' processors rewrite the packed rows' logits in front of the pick; the pick of a call with a sampling row is the two
    // launches over the per-packed-row table.  A call whose rows are all greedy and unprocessed launches what it launched before
    if (v_lp.any)
        if ((s = launch(v_lp.process, pack(v_logits, (uint32_t)c.vocab, (const verify_row*)v_tab, (const row_logits*)logits_tab_dev, (const uint32_t*)masks_dev,
                                           (const int32_t*)counts_dev, tokens))) != MC_OK)
            return s;
    if (v_pick.greedy) {
        if ((s = launch(v.argmax, pack((const void*)v_logits, (uint32_t)c.vocab, picks))) != MC_OK) return s;
    } else {
        const sampler_params& sp = v_pick.sp;
        if ((s = launch(v_pick.first, pack((const void*)v_logits, (uint32_t)c.vocab, sp.kpad, v_cand, v_pick.chunk, (const verify_row*)v_tab))) != MC_OK) return s;
        s = launch(v_pick.second, pack((const void*)v_logits, (uint32_t)c.vocab, (const uint64_t*)v_cand, (const verify_row*)v_tab, sp.nlists, sp.kpad, sp.cap,
                                       (const uint64_t*)seeds, (uint32_t)n_seed_pairs, picks));
        if (s != MC_OK) return s;
    }
    // Part 2n: every pick gets its record, in front of the acceptance: each accepted token and the bonus token is one of them
    if (v_lpp.any && (s = enqueue_logprobs(v_lpp, v_logits, nullptr, picks, (uint32_t)M, v_lp_tok, v_lp_ids, v_lp_top)) != MC_OK) return s;
    int32_t* paths = v.tree ? picks + M : nullptr;
    if (!v.tree)
        s = launch(v.accept, pack((const pp_seg*)pp_segs(pp_tab), tokens, (const int32_t*)picks, (const void*)v_logits, (uint32_t)c.vocab, v_out,
                                  v_out + B, logits));
    else
        s = launch(v.accept, pack((const pp_seg*)pp_segs(pp_tab), tokens, nodes, (const int32_t*)picks, (const void*)v_logits, (uint32_t)c.vocab, v_out,
                                  v_out + B, paths, logits));
    if (s != MC_OK) return s;
    // ... and behind the acceptance the penalised rows count what was fed: the accepted path
    if (v_lp.count)
        if ((s = launch(v_lp.counting, pack((const pp_seg*)pp_segs(pp_tab), tokens, (const int32_t*)v_out, (const int32_t*)paths, (const row_logits*)logits_tab_dev,
                                            counts_dev, (uint32_t)c.vocab))) != MC_OK)
            return s;
    if (!v.tree) return MC_OK;
    return launch(v.compact, pack((const pp_seg*)pp_segs(pp_tab), (const int32_t*)v_out, (const int32_t*)paths, kc, vt, (uint64_t)cache_elems,
                                  (uint32_t)B, (uint32_t)c.n_kv_heads, (uint32_t)c.head_dim, (uint32_t)c.max_seq_len));
}

namespace {

// what mc_verify_rows adds to the pass: a pick after every chunk row and the acceptance (next_tokens is the pass's own argument)
struct verify_out {
    int32_t* accepted; // [B]
    int32_t* picks;    // [M], may be null
    // mc_tree_verify: the chunks are trees
    const int32_t* parents = nullptr; // [M], packed like the tokens
    int32_t* paths = nullptr;         // [B][MC_VERIFY_MAX_LEN], may be null
};

// mc_rows_prefill, mc_extend_rows, mc_verify_rows and mc_tree_verify: one body, `extend` selects the attention (and `who` the
// texts), `v` the head over every packed row in place of the head over each row's last, v->parents the tree form of that
mc_status
rows_pass(mc_batch* b, const char* who, bool extend, const int32_t* tokens, const int32_t* lens, const int32_t* positions, int32_t* next_tokens,
          const verify_out* v = nullptr)
{
    const mc_decoder_config& c = b->p.cfg;
    const int B = b->B;
    // check (rows_plan.h: the admission, the tables and the scratch sizes are plain arithmetic there), tables, upload, prompt pass, head
    const bool tree = v && v->parents;
    const rows_counts n = rows_check(who, tokens, lens, positions, b->lengths.data(), B, c.max_seq_len, c.vocab, v != nullptr);
    if (!n.refusal.empty()) return fail(MC_ERR_INVALID_ARGUMENT, n.refusal);
    if (tree)
        if (const std::string why = tree_check(who, v->parents, lens, B); !why.empty()) return fail(MC_ERR_INVALID_ARGUMENT, why);
    const int M = n.M, nseg = n.nseg, ntiles = n.ntiles;
    // MC_PX_KEYS, the experiment's handle on the key ranges, is read at the call (the tests set it between calls on a live batch)
    const char* keys_env = getenv("MC_PX_KEYS");
    const int keys_override = keys_env ? std::max(atoi(keys_env), 0) : PX_KEYS_RULE;
    const rows_scratch sc = rows_scratch_of(c.max_seq_len, c.n_heads, c.head_dim, keys_override);
    mc_status s;
    MC_HIP(hipSetDevice(b->p.ordinal));
    rows_tables(lens, positions, B, ntiles, b->rows_host, b->pp_host);
    if (tree) tree_nodes(v->parents, lens, B, ntiles, M, b->pp_host);
    if ((s = b->reserve(b->pp_tab, b->pp_tab_cap, (int)b->pp_host.size(), (int)sc.tab_bytes())) != MC_OK) return s;
    MC_HIP(hipMemcpyAsync(b->pp_tab, b->pp_host.data(), b->pp_host.size(), hipMemcpyHostToDevice, b->p.stream));
    packed_prefill pk;
    pk.segs = pp_segs(b->pp_tab);
    pk.nseg = nseg;
    pk.tiles = pp_tiles(b->pp_tab);
    pk.ntiles = ntiles;
    if (tree) pk.nodes = tv_nodes(b->pp_tab, ntiles);
    MC_HIP(hipMemcpyAsync(b->rows, b->rows_host.data(), sizeof(step_state) * B, hipMemcpyHostToDevice, b->p.stream));
    if ((s = b->ensure_tokens(1)) != MC_OK) return s;
    MC_HIP(hipMemsetAsync(b->tokens_dev, 0xFF, sizeof(int32_t) * B, b->p.stream));
    if (!v && (s = b->begin_logprobs(1)) != MC_OK) return s; // Part 2n: the one pick per row is a record in slot r
    pk.kc = b->kc;
    pk.vt = b->vt;
    pk.B = B;
    pk.cache_stride = b->cache_elems;
    pk.fcos = b->fcos;
    pk.fsin = b->fsin;
    pk.x_out = b->x;
    if (extend) {
        // scratch for one launch group, sized once (rows_scratch_of)
        int sums_slots = b->px_slots;
        if ((s = b->reserve(b->px_sums, sums_slots, sc.per_tile, sc.slots, sizeof(float) * c.n_heads * PP_TILE_ROWS)) != MC_OK ||
            (s = b->reserve(b->px_part, b->px_slots, sc.per_tile, sc.slots, sc.per_slot)) != MC_OK)
            return s;
        rows_ranges(b->pp_host, ntiles, b->px_slots, keys_override, b->px_host, b->px_groups);
        if ((s = b->reserve(b->px_tab, b->px_tab_cap, (int)b->px_host.size(), sc.tiles_max * sc.per_tile)) != MC_OK) return s;
        MC_HIP(hipMemcpyAsync(b->px_tab, b->px_host.data(), sizeof(px_range) * b->px_host.size(), hipMemcpyHostToDevice, b->p.stream));
        pk.extend = true;
        pk.ranges = b->px_tab;
        pk.groups = b->px_groups.data();
        pk.ngroups = (int)b->px_groups.size();
        pk.sums = b->px_sums;
        pk.part = b->px_part;
    }
    const void* rows_all = nullptr;
    const int32_t* ids = nullptr;
    if (v) {
        // (M <= 128 here; the scratch is sized for any call)
        if ((s = b->reserve(b->v_xn, b->v_xn_cap, M, MC_VERIFY_MAX_ROWS, (size_t)c.dim * 2)) != MC_OK ||
            (s = b->reserve(b->v_logits, b->v_logits_cap, M, MC_VERIFY_MAX_ROWS, (size_t)c.vocab * 2)) != MC_OK ||
            (s = b->reserve(b->v_out, b->v_out_cap, 2 * B + M + MC_VERIFY_MAX_LEN * B, 2 * MC_WIDE_BATCH_MAX + MC_VERIFY_MAX_ROWS + MC_VERIFY_MAX_LEN * MC_WIDE_BATCH_MAX)) !=
                MC_OK)
            return s;
        MC_HIP(hipMemsetAsync(b->v_out, 0xFF, sizeof(int32_t) * 2 * B, b->p.stream)); // -1: a row not in the call
        if (tree) MC_HIP(hipMemsetAsync(b->v_out + 2 * B + M, 0xFF, sizeof(int32_t) * MC_VERIFY_MAX_LEN * B, b->p.stream)); // ... its path
        pk.rows_all = &rows_all;
        pk.tokens_dev = &ids;
        // Part 2n: a record per packed row, in the [MC_VERIFY_MAX_ROWS] twins of the step's buffers
        b->v_lpp = plan_logprobs(b->logprobs_on, b->logprobs_top, c.vocab, M, false);
        if (!b->v_lpp.refusal.empty()) return fail(MC_ERR_RUNTIME, b->v_lpp.refusal);
        if (b->v_lpp.any) {
            const int top = b->logprobs_top;
            if ((s = b->reserve_logprob_scratch(MC_VERIFY_MAX_ROWS)) != MC_OK || (s = b->reserve(b->v_lp_tok, b->v_lp_tok_cap, M, MC_VERIFY_MAX_ROWS)) != MC_OK) return s;
            MC_HIP(hipMemsetAsync(b->v_lp_tok, 0xFF, sizeof(float) * MC_VERIFY_MAX_ROWS, b->p.stream));
            if (top > 0) {
                if ((s = b->reserve(b->v_lp_ids, b->v_lp_ids_cap, M, MC_VERIFY_MAX_ROWS, sizeof(int32_t) * top)) != MC_OK ||
                    (s = b->reserve(b->v_lp_top, b->v_lp_top_cap, M, MC_VERIFY_MAX_ROWS, sizeof(float) * top)) != MC_OK)
                    return s;
                MC_HIP(hipMemsetAsync(b->v_lp_ids, 0xFF, sizeof(int32_t) * MC_VERIFY_MAX_ROWS * top, b->p.stream));
                MC_HIP(hipMemsetAsync(b->v_lp_top, 0xFF, sizeof(float) * MC_VERIFY_MAX_ROWS * top, b->p.stream));
            }
        }
        // Part 2m: the pick and the processors of the rows in the call (with the switch off verify_settings has refused every row that would
        // need them); their tables go up with the call's other tables
        b->v_pick = verify_pick_plan{};
        b->v_lp = verify_logits_plan{};
        if (b->verify_settings_on) {
            const tv_node* host_nodes = tree ? tv_nodes(b->pp_host.data(), ntiles) : nullptr;
            b->v_pick = plan_verify_pick(lens, b->row_samplers, decoder_sampler_of(b->d), c.vocab, b->n_seed_pairs, host_nodes, b->cand_per_row);
            if (!b->v_pick.refusal.empty()) return fail(MC_ERR_RUNTIME, b->v_pick.refusal);
            b->v_lp = plan_verify_logits(lens, b->row_logit_set, c.vocab, M, nseg);
            if (!b->v_pick.greedy || b->v_lp.any) {
                if ((s = b->reserve(b->v_tab, b->v_tab_cap, M, MC_VERIFY_MAX_ROWS)) != MC_OK) return s;
                MC_HIP(hipMemcpyAsync(b->v_tab, b->v_pick.table.data(), sizeof(verify_row) * M, hipMemcpyHostToDevice, b->p.stream));
            }
            if (!b->v_pick.greedy && (s = b->reserve(b->v_cand, b->v_cand_cap, M, MC_VERIFY_MAX_ROWS, sizeof(uint64_t) * b->cand_per_row)) != MC_OK) return s;
            if (b->v_lp.any && ((s = b->ensure(b->logits_tab_dev, sizeof(row_logits) * B)) != MC_OK ||
                                (s = b->send_if_changed(b->logits_tab_dev, b->logits_tab_sent, b->v_lp.table)) != MC_OK))
                return s;
        }
    }
    if ((s = decoder_prefill_packed(b->d, tokens, M, pk)) != MC_OK) return s;
    if (v) s = b->verify_head(rows_all, ids, M, nseg, pk.nodes);
    else if ((s = b->plan_pick(true)) == MC_OK) s = b->head(true, false);
    if (s != MC_OK) return s;
    MC_HIP(hipStreamSynchronize(b->p.stream)); // (`tokens` is the caller's buffer; the tables are read by the launches)
    if (v) {
        b->v_rows = M;
        b->v_lp_rows = b->v_lpp.any ? M : 0;
        b->v_host.resize(2 * B + M + (tree ? MC_VERIFY_MAX_LEN * B : 0));
        MC_HIP(hipMemcpy(b->v_host.data(), b->v_out, sizeof(int32_t) * b->v_host.size(), hipMemcpyDeviceToHost));
        std::copy_n(b->v_host.begin(), B, v->accepted);
        if (next_tokens) std::copy_n(b->v_host.begin() + B, B, next_tokens);
        if (v->picks) std::copy_n(b->v_host.begin() + 2 * B, M, v->picks);
        if (v->paths) std::copy_n(b->v_host.begin() + 2 * B + M, MC_VERIFY_MAX_LEN * B, v->paths);
        // the rejected drafts' slots stay written past the length: the rewound state every rows call handles
        for (int r = 0; r < B; r++)
            if (lens[r] > 0) b->lengths[r] = positions[r] + v->accepted[r] + 1;
        return MC_OK;
    }
    for (int r = 0; r < B; r++)
        if (lens[r] > 0) b->lengths[r] = positions[r] + lens[r];
    if (next_tokens) MC_HIP(hipMemcpy(next_tokens, b->tokens_dev, sizeof(int32_t) * B, hipMemcpyDeviceToHost));
    return MC_OK;
}

// mc_verify_rows / mc_tree_verify (`who`): every row in the call picks greedily, and none carries a mask or penalties -- unless the batch's
// switch is on (Part 2m), when rows_pass plans the pick and the processors of such rows instead
mc_status
verify_settings(const mc_batch* b, const char* who, const int32_t* lens)
{
    if (b->verify_settings_on) return MC_OK;
    if (mc_status s = refuse(verify_samplers(who, lens, b->row_samplers, decoder_sampler_of(b->d))); s != MC_OK) return s;
    return refuse(verify_logit_rows(who, lens, b->row_logit_set));
}

} // namespace

extern "C" {

// ---- Part 2d: the packed prompt pass ----

mc_status
mc_rows_prefill(mc_batch* b, const int32_t* tokens, const int32_t* lens, const int32_t* positions, int32_t* next_tokens)
{
    if (!b || !tokens || !lens || !positions) return fail(MC_ERR_INVALID_ARGUMENT, "mc_rows_prefill: null argument");
    return rows_pass(b, "mc_rows_prefill", false, tokens, lens, positions, next_tokens);
}

// ---- Part 2e: chunks that see their row's context ----

mc_status
mc_extend_rows(mc_batch* b, const int32_t* tokens, const int32_t* lens, const int32_t* positions, int32_t* next_tokens)
{
    if (!b || !tokens || !lens || !positions) return fail(MC_ERR_INVALID_ARGUMENT, "mc_extend_rows: null argument");
    return rows_pass(b, "mc_extend_rows", true, tokens, lens, positions, next_tokens);
}

// ---- Part 2f: speculative verify ----

mc_status
mc_verify_rows(mc_batch* b, const int32_t* tokens, const int32_t* lens, const int32_t* positions, int32_t* accepted, int32_t* next_tokens,
               int32_t* picks)
{
    if (!b || !tokens || !lens || !positions || !accepted) return fail(MC_ERR_INVALID_ARGUMENT, "mc_verify_rows: null argument");
    if (mc_status s = verify_settings(b, "mc_verify_rows", lens); s != MC_OK) return s;
    const verify_out v{accepted, picks};
    return rows_pass(b, "mc_verify_rows", true, tokens, lens, positions, next_tokens, &v);
}

// ---- Part 2g: speculative verify over a draft tree per row ----

mc_status
mc_tree_verify(mc_batch* b, const int32_t* tokens, const int32_t* parents, const int32_t* lens, const int32_t* positions, int32_t* accepted,
               int32_t* next_tokens, int32_t* paths, int32_t* picks)
{
    if (!b || !tokens || !parents || !lens || !positions || !accepted) return fail(MC_ERR_INVALID_ARGUMENT, "mc_tree_verify: null argument");
    if (mc_status s = verify_settings(b, "mc_tree_verify", lens); s != MC_OK) return s;
    const verify_out v{accepted, picks, parents, paths};
    return rows_pass(b, "mc_tree_verify", true, tokens, lens, positions, next_tokens, &v);
}

// ---- Part 2m: verify calls for sampling, masked and penalised rows ----

mc_status
mc_settings_verify_set(mc_batch* b, int32_t enable)
{
    if (!b) return fail(MC_ERR_INVALID_ARGUMENT, "mc_settings_verify_set: null argument");
    if (mc_status s = refuse(check_verify_switch(enable)); s != MC_OK) return s;
    b->verify_settings_on = enable == 1;
    return MC_OK;
}

int32_t
mc_settings_verify_enabled(const mc_batch* b)
{
    return b && b->verify_settings_on ? 1 : 0;
}

mc_status
mc_verify_get_logits(mc_batch* b, void* logits_T)
{
    if (!b || !logits_T) return fail(MC_ERR_INVALID_ARGUMENT, "mc_verify_get_logits: null argument");
    if (!b->v_rows) return fail(MC_ERR_INVALID_ARGUMENT, "mc_verify_get_logits: no mc_verify_rows call on this batch yet");
    MC_HIP(hipSetDevice(b->p.ordinal));
    MC_HIP(hipStreamSynchronize(b->p.stream));
    MC_HIP(hipMemcpy(logits_T, b->v_logits, (size_t)b->v_rows * b->p.cfg.vocab * 2, hipMemcpyDeviceToHost));
    return MC_OK;
}

// ---- Part 2n: the records of the last verify call (the switch and mc_logprobs_get: batch_settings.cc) ----

mc_status
mc_logprobs_get_verify(mc_batch* b, float* pick_logprobs, int32_t* top_ids, float* top_logprobs)
{
    if (!b || !pick_logprobs) return fail(MC_ERR_INVALID_ARGUMENT, "mc_logprobs_get_verify: null argument");
    if (!b->logprobs_on) return fail(MC_ERR_INVALID_ARGUMENT, "mc_logprobs_get_verify: log-probabilities are switched off (mc_logprobs_set)");
    if (!b->v_lp_rows) return fail(MC_ERR_INVALID_ARGUMENT, "mc_logprobs_get_verify: no verify call with log-probabilities on this batch yet");
    const size_t M = (size_t)b->v_lp_rows, top = (size_t)b->logprobs_top;
    if (top == 0 && (top_ids || top_logprobs)) return fail(MC_ERR_INVALID_ARGUMENT, "mc_logprobs_get_verify: top_n is 0, the top arrays must be null");
    MC_HIP(hipSetDevice(b->p.ordinal));
    MC_HIP(hipStreamSynchronize(b->p.stream));
    MC_HIP(hipMemcpy(pick_logprobs, b->v_lp_tok, sizeof(float) * M, hipMemcpyDeviceToHost));
    if (top_ids) MC_HIP(hipMemcpy(top_ids, b->v_lp_ids, sizeof(int32_t) * M * top, hipMemcpyDeviceToHost));
    if (top_logprobs) MC_HIP(hipMemcpy(top_logprobs, b->v_lp_top, sizeof(float) * M * top, hipMemcpyDeviceToHost));
    return MC_OK;
}

} // extern "C"
