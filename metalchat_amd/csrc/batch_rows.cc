// The batch's rows passes (Parts 2d to 2g; the map of the whole: batch_impl.h): mc_rows_prefill, mc_extend_rows, mc_verify_rows and
// mc_tree_verify through one body, rows_pass -- the admission and the tables are rows_plan.h's, the prompt pass the decoder's, the head behind it
// the batch's own ordered plan (batch_call_plan.h plan_rows_tail or plan_verify_call, run by mc_batch::run) -- and mc_verify_get_logits; Part 2m's
// switch (mc_settings_verify_set), with which the verify plan also processes, samples and counts per packed row.
#include "batch_impl.h"

using namespace mcimpl;

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
    // check (rows_plan.h: the admission, the tables and the scratch sizes are plain arithmetic there)
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
    // tables
    rows_tables(lens, positions, B, ntiles, b->rows_host, b->pp_host);
    if (tree) tree_nodes(v->parents, lens, B, ntiles, M, b->pp_host);
    // plan: the head behind the prompt pass -- over every packed row (a verify call; with the switch off verify_settings has refused every row
    // whose settings it would need), or the ragged token's tail over each row's last
    const batch_call_plan plan = v ? plan_verify_call(b->fx, b->settings(), lens, M, nseg, tree ? tv_nodes(b->pp_host.data(), ntiles) : nullptr)
                                   : plan_rows_tail(b->fx, b->settings());
    // reserve from the plan (the one pick per row of a non-verify pass is token 0 of a call of one, its record in slot r), and for the prompt pass
    mc_status s;
    MC_HIP(hipSetDevice(b->p.ordinal));
    if ((s = b->prepare(plan, 1)) != MC_OK || (s = b->reserve(b->pp_tab, b->pp_tab_cap, (int)b->pp_host.size(), (int)sc.tab_bytes())) != MC_OK) return s;
    packed_prefill pk;
    if (extend) {
        // scratch for one launch group, sized once (rows_scratch_of)
        int sums_slots = b->px_slots;
        if ((s = b->reserve(b->px_sums, sums_slots, sc.per_tile, sc.slots, sizeof(float) * c.n_heads * PP_TILE_ROWS)) != MC_OK ||
            (s = b->reserve(b->px_part, b->px_slots, sc.per_tile, sc.slots, sc.per_slot)) != MC_OK)
            return s;
        rows_ranges(b->pp_host, ntiles, b->px_slots, keys_override, b->px_host, b->px_groups);
        if ((s = b->reserve(b->px_tab, b->px_tab_cap, (int)b->px_host.size(), sc.tiles_max * sc.per_tile)) != MC_OK) return s;
        pk.extend = true;
        pk.ranges = b->px_tab;
        pk.groups = b->px_groups.data();
        pk.ngroups = (int)b->px_groups.size();
        pk.sums = b->px_sums;
        pk.part = b->px_part;
    }
    // upload
    MC_HIP(hipMemcpyAsync(b->pp_tab, b->pp_host.data(), b->pp_host.size(), hipMemcpyHostToDevice, b->p.stream));
    if (extend) MC_HIP(hipMemcpyAsync(b->px_tab, b->px_host.data(), sizeof(px_range) * b->px_host.size(), hipMemcpyHostToDevice, b->p.stream));
    MC_HIP(hipMemcpyAsync(b->rows, b->rows_host.data(), sizeof(step_state) * B, hipMemcpyHostToDevice, b->p.stream));
    MC_HIP(hipMemsetAsync(b->tokens_dev, 0xFF, sizeof(int32_t) * B, b->p.stream));
    // prompt pass
    pk.segs = pp_segs(b->pp_tab);
    pk.nseg = nseg;
    pk.tiles = pp_tiles(b->pp_tab);
    pk.ntiles = ntiles;
    if (tree) pk.nodes = tv_nodes(b->pp_tab, ntiles);
    pk.kc = b->kc;
    pk.vt = b->vt;
    pk.B = B;
    pk.cache_stride = b->cache_elems;
    pk.fcos = b->fcos;
    pk.fsin = b->fsin;
    pk.x_out = b->x;
    call_args args{plan};
    if (v) {
        pk.rows_all = &args.xrows;
        pk.tokens_dev = &args.ids;
        args.nodes = pk.nodes;
    }
    if ((s = decoder_prefill_packed(b->d, tokens, M, pk)) != MC_OK) return s;
    // run the list, read back
    if ((s = b->run_all(args)) != MC_OK) return s;
    MC_HIP(hipStreamSynchronize(b->p.stream)); // (`tokens` is the caller's buffer; the tables are read by the launches)
    if (v) {
        verify_state& vs = b->vs;
        vs.rows = M;
        vs.records.count = plan.lp_slots; // (M, or 0: the getter refuses behind a call that failed on its way or recorded nothing)
        vs.host.resize(2 * B + M + (tree ? MC_VERIFY_MAX_LEN * B : 0));
        MC_HIP(hipMemcpy(vs.host.data(), vs.out, sizeof(int32_t) * vs.host.size(), hipMemcpyDeviceToHost));
        std::copy_n(vs.host.begin(), B, v->accepted);
        if (next_tokens) std::copy_n(vs.host.begin() + B, B, next_tokens);
        if (v->picks) std::copy_n(vs.host.begin() + 2 * B, M, v->picks);
        if (v->paths) std::copy_n(vs.host.begin() + 2 * B + M, MC_VERIFY_MAX_LEN * B, v->paths);
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
    if (!b->vs.rows) return fail(MC_ERR_INVALID_ARGUMENT, "mc_verify_get_logits: no mc_verify_rows call on this batch yet");
    MC_HIP(hipSetDevice(b->p.ordinal));
    MC_HIP(hipStreamSynchronize(b->p.stream));
    MC_HIP(hipMemcpy(logits_T, b->vs.logits, (size_t)b->vs.rows * b->p.cfg.vocab * 2, hipMemcpyDeviceToHost));
    return MC_OK;
}

// ---- Part 2n: the records of the last verify call (the switch and mc_logprobs_get: batch_settings.cc) ----

mc_status
mc_logprobs_get_verify(mc_batch* b, float* pick_logprobs, int32_t* top_ids, float* top_logprobs)
{
    if (!b || !pick_logprobs) return fail(MC_ERR_INVALID_ARGUMENT, "mc_logprobs_get_verify: null argument");
    if (!b->logprobs_on) return fail(MC_ERR_INVALID_ARGUMENT, "mc_logprobs_get_verify: log-probabilities are switched off (mc_logprobs_set)");
    if (!b->vs.records.count) return fail(MC_ERR_INVALID_ARGUMENT, "mc_logprobs_get_verify: no verify call with log-probabilities on this batch yet");
    if (b->logprobs_top == 0 && (top_ids || top_logprobs)) return fail(MC_ERR_INVALID_ARGUMENT, "mc_logprobs_get_verify: top_n is 0, the top arrays must be null");
    return b->copy_records(b->vs.records, (size_t)b->vs.records.count, pick_logprobs, top_ids, top_logprobs);
}

} // extern "C"
