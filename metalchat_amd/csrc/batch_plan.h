// What a batch (mc_batch_*, mc_ragged_*, the rows passes' heads; batch_impl.h) launches, decided without a device: the admission of a decoder
// (refusal), the GEMV of every matrix (plan_batch_gemv: family, tiles, grid, the adaptor's launch in front), the launches of a step whose name and
// grid follow from the config alone (plan_step), the head's pick in its three forms with the rows' effective samplers (plan_head, sampler_plan),
// the logit processors' table and launch (plan_logits), the two log-probability launches behind a pick (plan_logprobs), the head of a verify
// call (plan_verify_head; with row settings: plan_verify_pick, plan_verify_logits), and the checks of a call that need no device
// (check_ragged, check_tokens, step_bounds / generate_bounds, verify_samplers, verify_logit_rows, check_row).  Plain integer arithmetic over config
// words, a linear's shape and kernels/abi.h constants -- no HIP, no mc_decoder, no device pointers -- so tests/cpp/test_batch_plan.cc pins names,
// grids, blocks and LDS bytes on the CPU against a recording of the launches (tests/golden/batch_plans.json).  batch_call_plan.h composes these pieces
// into the ordered list of a whole call; the batch's units run that list and bind the arguments; fail(), the allocations, the uploads and the
// stream stay there.  A refusal is a text here, "" = none.
#pragma once

#include <algorithm>
#include <climits>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

#include "../../include/metalchat_hip.h" // mc_decoder_config, MC_WFMT_*, MC_SAMPLER_*
#include "kernels/abi.h"
#include "rows_plan.h" // rolled_rewind
#include "sampler_plan.h"

namespace mcimpl {

using namespace mc::abi;

static_assert(ROW_SAMPLER_GREEDY == MC_SAMPLER_GREEDY && ROW_SAMPLER_DEFAULT == MC_SAMPLER_DEFAULT && ROW_SAMPLER_DRAW == MC_SAMPLER_DRAW,
              "row_sampler::kind carries the public kinds");

struct launch_plan {
    std::string name;
    unsigned gx = 0, gy = 1, gz = 1, block = 0, lds = 0;
};

// ---------------------------------------------------------------- admission

// the shape of one fused matrix (batch_linear adds where it lies): rows [out][in] in MC_WFMT_* format, quantised in `ngroups` groups of `group`
// along in (group 0: one scale per row); lora: it has adaptors, lora_cols = adaptors x rank fused columns
struct linear_shape {
    int fmt = MC_WFMT_T, out = 0, in = 0, group = 0, ngroups = 0;
    bool lora = false;
    int lora_cols = 0;
};

// the admission predicate: "" = admitted, else the reason.  mc_batch_create (wide = false) takes one weight format for the whole
// decoder, int4 in groups that are multiples of 128 or plain T, and no adaptors.  mc_wide_batch_create (wide = true, Part 2i) judges
// every linear on its own: T, int4 or int8, quantised in groups that are multiples of 32 or one scale per row, and on the seven
// layer linears adaptors whose fused columns are a multiple of 16.  The conditions both share keep one text.
// Parts: cfg, emb_fmt, output and layers of {qkv, wo, w13, w2}, every linear a linear_shape (decoder_parts; the CPU test's own)
template <typename Parts> std::string
refusal(const Parts& p, bool wide)
{
    const mc_decoder_config& c = p.cfg;
    if (c.family != MC_FAMILY_LLAMA3) return "only llama3 decoders can be batched";
    if (c.dtype != MC_DTYPE_BF16) return "only bfloat16 decoders can be batched";
    if (c.layer_begin != 0 || c.layer_end != c.n_layers) return "the decoder must own every layer (a pipeline stage cannot be batched)";
    if (!wide && c.weight_format != MC_WFMT_I4 && c.weight_format != MC_WFMT_T)
        return "only int4 (group % 128 == 0) and plain bfloat16 weights can be batched";
    if (!wide && c.weight_format == MC_WFMT_I4 && c.group_size % 128 != 0) return "int4 weights need a group size that is a multiple of 128";
    if (c.qmode != MC_QMODE_EXACT) return "only the exact quantised arithmetic (MC_QMODE_EXACT) can be batched";
    if (c.head_dim != 128 && c.head_dim != 64) return "head_dim must be 128 or 64";
    if (c.n_kv_heads <= 0 || c.n_heads % c.n_kv_heads != 0 || c.n_heads / c.n_kv_heads > 16)
        return "n_heads must be a multiple of n_kv_heads, at most 16 per kv head";
    if (c.max_seq_len < 64) return "max_seq_len must be at least 64";
    if (p.emb_fmt != MC_WFMT_T && p.emb_fmt != MC_WFMT_I8) return "unsupported embedding format";
    auto bad = [&](const linear_shape& L, const char* name, bool head) -> std::string {
        if (!wide) {
            if (L.lora) return std::string("LoRA adaptors are not supported (") + name + ")";
            if (L.fmt != c.weight_format) return std::string("mixed weight formats (") + name + ")";
        } else {
            if (L.fmt != MC_WFMT_T && L.fmt != MC_WFMT_I4 && L.fmt != MC_WFMT_I8)
                return std::string(name) + ": only int4, int8 and plain bfloat16 weights can be batched";
            if (L.lora && head) return std::string("LoRA adaptors are not supported (") + name + ")";
            if (L.lora && L.lora_cols % 16 != 0) return std::string(name) + ": LoRA rank must be a multiple of 16";
        }
        if (L.out % 16 != 0 || L.in % (int)BG_K_UNIT != 0)
            return std::string(name) + ": the batched GEMV needs out_features % 16 == 0 and in_features % 1024 == 0";
        if (!wide && L.fmt == MC_WFMT_I4 && L.group % 128 != 0) return std::string(name) + ": int4 group size must be a multiple of 128";
        if (wide && L.fmt != MC_WFMT_T && L.group % 32 != 0)
            return std::string(name) + ": the group size of quantised weights must be a multiple of 32 (or 0: one scale per row)";
        return "";
    };
    const int H = c.n_heads, KV = c.n_kv_heads, hd = c.head_dim;
    for (const auto& L : p.layers) {
        for (auto [lin, name] : {std::pair<const linear_shape*, const char*>{&L.qkv, "wq|wk|wv"}, {&L.wo, "wo"}, {&L.w13, "w1|w3"}, {&L.w2, "w2"}}) {
            std::string r = bad(*lin, name, false);
            if (!r.empty()) return r;
        }
        if (L.qkv.out != (H + 2 * KV) * hd || L.qkv.in != c.dim || L.wo.in != H * hd || L.wo.out != c.dim || L.w13.out % 32 != 0 ||
            L.w13.in != c.dim || L.w2.in != L.w13.out / 2 || L.w2.out != c.dim)
            return "layer shapes do not chain";
    }
    std::string r = bad(p.output, "output", true);
    if (!r.empty()) return r;
    if (p.output.out != c.vocab || p.output.in != c.dim) return "output head shape";
    return "";
}

// ---------------------------------------------------------------- the GEMV: y[r] = epi(W x[r]) for the B rows

// of a batch, fixed at its creation: its rows, the device's compute units and MC_WB_TILES (0: by wb_tiles' rule)
struct batch_env {
    int B = 0, cus = 0, tiles_env = 0;
};

// MC_WB_TILES as mc_batch_create reads it: 1, 2, 4 or 8, anything else (or unset) = 0
inline int
wb_tiles_env_of(const char* value)
{
    const int t = value ? atoi(value) : 0;
    return t == 1 || t == 2 || t == 4 || t == 8 ? t : 0;
}

// 16-row weight tiles per workgroup of mc_wb_gemv_* for the matrix L: the most of 8, 4, 2 that still brings a workgroup to
// every compute unit, else 1 (measured: DESIGN.md "Wide batches").  MC_WB_TILES is the experiment's handle.  At most 4 for an
// int8 matrix or one with an adaptor: those kernels run 8 tiles as two passes of 4 (wide_kernels.hip), which only fetches x twice.
inline int
wb_tiles(const linear_shape& L, const batch_env& e)
{
    const int most = L.fmt == MC_WFMT_I8 || L.lora ? 4 : 8;
    if (e.tiles_env) return std::min(e.tiles_env, most);
    for (int t = most; t > 1; t /= 2)
        if ((L.out / 16 + t - 1) / t >= e.cus) return t;
    return 1;
}

inline const char*
fmt_name(int fmt)
{
    return fmt == MC_WFMT_I4 ? "i4" : (fmt == MC_WFMT_I8 ? "i8" : "w");
}

// The ONE place that chooses a GEMV launch: the format from L.fmt; up to 16 rows are the columns of mc_b_gemv_*'s single MFMA tile (it masks
// with m < B), more go through mc_wb_gemv_*, whose rows carry the same bits (wide_kernels.hip) and whose argument list has L.out in front of ldy
// (wide).  A linear with an adaptor takes two launches -- a = T(A x) for all rows, an ordinary T-format GEMV over the stacked A [lora_cols][in]
// (adaptor, in front), then the main launch in its _l form, which adds T(T(B a) scale) in front of its epilogue
struct batch_gemv_plan {
    bool wide = false, lora = false;
    launch_plan adaptor, main;
};
inline batch_gemv_plan
plan_batch_gemv(const linear_shape& L, int epi, const batch_env& e)
{
    batch_gemv_plan g;
    g.wide = e.B > 16;
    g.lora = L.lora;
    if (L.lora) {
        linear_shape A; // plain T, no scales and no adaptor of its own: one level
        A.out = L.lora_cols;
        A.in = L.in;
        g.adaptor = plan_batch_gemv(A, 0, e).main;
    }
    const int tiles = g.wide ? wb_tiles(L, e) : 1;
    g.main.name = std::string(g.wide ? "mc_wb_gemv_" : "mc_b_gemv_") + fmt_name(L.fmt) + "_bfloat_e" + std::to_string(epi) + (L.lora ? "_l" : "");
    g.main.gx = (unsigned)(L.out / 16 + tiles - 1) / tiles;
    g.main.block = BG_THREADS;
    return g;
}

// ---------------------------------------------------------------- one token of a call

// The launches of a step whose name and grid follow from the config, B and (ragged, rolling): the lockstep kernels read the shared state
// (mc_step_set starts the step), their _rows forms row r's own (mc_b_rows_begin; a rolling batch: mc_b_rows_begin_rolling, a workgroup per row)
struct step_plan {
    bool ragged = false, rolling = false; // rolling: ragged on a rolling batch
    launch_plan begin, embed, rmsnorm, rope, scores, pv;
};
inline step_plan
plan_step(const mc_decoder_config& c, int B, int nsplit, bool ragged, bool rolling)
{
    const unsigned H = c.n_heads, KV = c.n_kv_heads, hd = c.head_dim, b = B;
    const std::string sfx = ragged ? "_rows_bfloat" : "_bfloat";
    step_plan s;
    s.ragged = ragged;
    s.rolling = ragged && rolling;
    s.begin = !ragged ? launch_plan{"mc_step_set", 1, 1, 1, 64, 0}
                      : (s.rolling ? launch_plan{"mc_b_rows_begin_rolling", b, 1, 1, 64, 0} : launch_plan{"mc_b_rows_begin", 1, 1, 1, 64, 0});
    s.embed = {ragged ? "mc_b_embed_rows_bfloat" : "mc_b_embed_bfloat", ((unsigned)c.dim + 255) / 256, b, 1, 256, 0};
    s.rmsnorm = {"mc_b_rmsnorm_bfloat", 1, b, 1, 1024, 0};
    s.rope = {"mc_b_rope_kv" + sfx, H + 2 * KV, b, 1, hd / 2, 0};
    s.scores = {"mc_b_attn_scores" + sfx, (unsigned)nsplit, KV, b, 256, 0};
    s.pv = {"mc_b_attn_pv" + sfx, hd / 16, KV, b, 1024, 0};
    return s;
}

// ---------------------------------------------------------------- the pick

// the decoder's sampler as a batch reads it (decoder_sampler_of), and a row's effective one
struct decoder_sampler {
    int kind = MC_SAMPLER_GREEDY, top_k = 50;
    float inv_temp_T = 0.0f, top_p_T = 0.0f;
};
// Part 2k: the sampler of a row slot as mc_row_sampler_set took it (the caller's values, and rounded as the decoder rounds its own)
struct row_setting {
    int32_t kind = MC_SAMPLER_INHERIT, top_k = 0;
    float temperature = 0.0f, top_p = 0.0f;
    float inv_temp_T = 0.0f, top_p_T = 0.0f;
};
// row r's effective sampler: its own, or the decoder's while it inherits
inline decoder_sampler
sampler_of_row(const row_setting& rs, const decoder_sampler& dec)
{
    if (rs.kind == MC_SAMPLER_INHERIT) return dec;
    decoder_sampler e;
    e.kind = rs.kind;
    e.top_k = rs.top_k;
    e.inv_temp_T = rs.inv_temp_T;
    e.top_p_T = rs.top_p_T;
    return e;
}
// an effective sampler as the mixed launches read it (abi.h row_sampler): top_k capped at the vocabulary, a greedy row all zeros
inline row_sampler
row_sampler_of(const decoder_sampler& e, int vocab)
{
    if (e.kind == MC_SAMPLER_GREEDY) return row_sampler{ROW_SAMPLER_GREEDY, 0u, 0.0f, 0.0f};
    return row_sampler{e.kind == MC_SAMPLER_DRAW ? ROW_SAMPLER_DRAW : ROW_SAMPLER_DEFAULT, (uint32_t)std::min(e.top_k, vocab), e.inv_temp_T, e.top_p_T};
}

// (sampler_plan, the two launches of make_default_sampler for given settings: sampler_plan.h)

// The pick of a head takes the cheapest of three forms, chosen from the settings of ALL B rows (which rows go idle inside a chained call is
// not known on the host):
//   PICK_GREEDY   no row samples               mc_b_argmax
//   PICK_UNIFORM  all sample, settings equal   mc_b_topk_candidates_bfloat + mc_b_sample with the plan of those settings
//                 (all MC_SAMPLER_DRAW: + mc_draw_b, the same shape; the kind is one of the settings, so default and draw rows mix)
//   PICK_MIXED    anything else                the two mixed launches over the table of effective settings
// The first two are what a batch without row samplers launches for the decoder's sampler, argument for argument.  ragged: the _rows forms,
// where rows whose pos is -1 get no pick.  cand_per_row: the candidate keys the batch holds for each row.
enum pick_form { PICK_GREEDY, PICK_UNIFORM, PICK_MIXED };
struct head_plan {
    std::string refusal; // (MC_ERR_RUNTIME)
    pick_form form = PICK_GREEDY;
    launch_plan first, second; // PICK_GREEDY: first alone
    sampler_params sp{};
    uint32_t chunk = 0;
    std::vector<row_sampler> table; // [B]: the effective settings, what the mixed launches read
};
inline head_plan
plan_head(const std::vector<row_setting>& rows, const decoder_sampler& dec, int vocab, bool ragged, size_t cand_per_row)
{
    const unsigned B = (unsigned)rows.size();
    const std::string sfx = ragged ? "_rows_bfloat" : "_bfloat";
    head_plan h;
    const decoder_sampler sm = sampler_of_row(rows[0], dec);
    int sampling = 0, top_k_max = 0;
    bool alike = true;
    h.table.resize(B);
    for (unsigned r = 0; r < B; r++) {
        const decoder_sampler e = sampler_of_row(rows[r], dec);
        const bool samples = e.kind != MC_SAMPLER_GREEDY;
        h.table[r] = row_sampler_of(e, vocab);
        if (r > 0 && memcmp(&h.table[r], &h.table[0], sizeof(row_sampler)) != 0) alike = false;
        if (!samples) continue;
        sampling++;
        top_k_max = std::max(top_k_max, e.top_k);
    }
    if (!sampling) {
        h.first = {"mc_b_argmax" + sfx, 1, B, 1, 1024, 0};
        return h;
    }
    // make_default_sampler per row (sampler_kernels.hip): per-chunk candidates, then one workgroup per row
    h.form = alike ? PICK_UNIFORM : PICK_MIXED;
    h.refusal = sampler_plan(alike ? sm.top_k : top_k_max, vocab, sm.inv_temp_T, sm.top_p_T, &h.sp, &h.chunk);
    if (h.refusal.empty() && (size_t)h.sp.nlists * h.sp.kpad > cand_per_row) h.refusal = SAMPLER_ROW_TOO_LONG;
    if (!h.refusal.empty()) return h;
    if (alike) {
        h.first = {"mc_b_topk_candidates_bfloat", h.sp.nlists, B, 1, 64, 0};
        h.second = {(sm.kind == MC_SAMPLER_DRAW ? "mc_draw_b" : "mc_b_sample") + sfx, 1, B, 1, 128, h.sp.cap * 8};
    } else {
        h.first = {"mc_b_topk_candidates_mixed_bfloat", h.sp.nlists, B, 1, 64, 0};
        h.second = {"mc_b_pick_mixed" + sfx, 1, B, 1, 1024, h.sp.cap * 8};
    }
    return h;
}

// ---------------------------------------------------------------- the logit processors (Part 2l)

// the logit processor of a row slot as the caller set it
struct row_logit_setting {
    bool masked = false;
    float rep = 1.0f, freq = 0.0f, pres = 0.0f;
    bool penalised() const { return !(rep == 1.0f && freq == 0.0f && pres == 0.0f); }
};
// the table of the rows' processors and the ONE launch between the head GEMV and the pick that rewrites those rows' logits in place; any false:
// no row has anything set, no launch and no table.  The ragged form takes one more argument (count)
struct logits_plan {
    bool any = false;
    std::vector<row_logits> table; // [B]
    launch_plan launch;
};
inline logits_plan
plan_logits(const std::vector<row_logit_setting>& rows, int vocab, bool ragged)
{
    const unsigned B = (unsigned)rows.size();
    logits_plan p;
    p.table.assign(B, row_logits{});
    for (unsigned r = 0; r < B; r++) {
        const row_logit_setting& rs = rows[r];
        row_logits& t = p.table[r];
        t.flags = (rs.masked ? ROW_LOGITS_MASK : 0u) | (rs.penalised() ? ROW_LOGITS_PENALTY : 0u);
        if (!t.flags) continue;
        p.any = true;
        if (!rs.penalised()) continue;
        t.rep = rs.rep;
        t.inv_rep = 1.0f / rs.rep;
        t.freq = rs.freq;
        t.pres = rs.pres;
    }
    if (p.any) p.launch = {ragged ? "mc_b_logits_process_rows_bfloat" : "mc_b_logits_process_bfloat", ((unsigned)vocab + LP_CHUNK - 1) / LP_CHUNK, B, 1, LP_THREADS, 0};
    return p;
}

// ---------------------------------------------------------------- row log-probabilities (Part 2n)

static_assert(LOGPROBS_MAX_TOP == MC_LOGPROBS_MAX_TOP, "the kernels' bound is the public one");

// mc_logprobs_set's values ("" = fine)
inline std::string
check_logprobs(int32_t enable, int32_t top_n, int vocab)
{
    if (enable != 0 && enable != 1) return "mc_logprobs_set: enable must be 0 or 1";
    if (top_n < 0 || top_n > MC_LOGPROBS_MAX_TOP) return "mc_logprobs_set: top_n must lie in [0, " + std::to_string(MC_LOGPROBS_MAX_TOP) + "]";
    if (top_n > vocab) return "mc_logprobs_set: top_n (" + std::to_string(top_n) + ") is above the vocabulary (" + std::to_string(vocab) + ")";
    return "";
}

// The two launches behind the pick of R rows (logprob_kernels.hip): a part and top_n keys per (row, chunk), then one workgroup per row that folds
// them.  any false (the switch is off): nothing is launched.  ragged: the _rows forms, in which idle rows' workgroups exit; a verify call takes the
// plain forms over its M packed rows.  The finish launch holds a row's parts one to a thread and its nchunk * top_n keys in registers: a
// vocabulary beyond that is refused (MC_ERR_RUNTIME)
struct logprobs_plan {
    std::string refusal;
    bool any = false;
    uint32_t nchunk = 0;
    launch_plan parts, finish;
};
inline logprobs_plan
plan_logprobs(bool enabled, int top_n, int vocab, int R, bool ragged)
{
    logprobs_plan p;
    if (!enabled) return p;
    p.any = true;
    p.nchunk = ((uint32_t)vocab + LOGPROB_CHUNK - 1) / LOGPROB_CHUNK;
    if (p.nchunk > LOGPROB_THREADS || p.nchunk * (uint32_t)top_n > LOGPROB_KEY_CAP) {
        p.refusal = "mc_logprobs: the vocabulary has " + std::to_string(p.nchunk) + " chunks of " + std::to_string(LOGPROB_CHUNK) + ", with top_n " +
                    std::to_string(top_n) + " more than the finish launch folds (" + std::to_string(LOGPROB_THREADS) + " chunks, " +
                    std::to_string(LOGPROB_KEY_CAP) + " keys)";
        return p;
    }
    const std::string sfx = ragged ? "_rows_bfloat" : "_bfloat";
    p.parts = {"mc_logprob_parts" + sfx, p.nchunk, (unsigned)R, 1, LOGPROB_THREADS, 0};
    p.finish = {"mc_logprob_finish" + sfx, 1, (unsigned)R, 1, LOGPROB_THREADS, 0};
    return p;
}

// ---------------------------------------------------------------- the head of a verify call

// mc_verify_rows: the final norm, the head and a greedy pick for each of the M packed rows, then per segment the acceptance of its drafts.
// tree (mc_tree_verify): the walk in place of the prefix rule, then the accepted path's K / V moved into place in every layer (compact)
struct verify_plan {
    bool tree = false;
    launch_plan norm, head, argmax, accept, compact;
};
inline verify_plan
plan_verify_head(const linear_shape& L, const mc_decoder_config& c, int n_layers, int M, int nseg, bool tree)
{
    verify_plan v;
    v.tree = tree;
    v.norm = {"mc_b_rmsnorm_bfloat", 1, (unsigned)M, 1, 1024, 0};
    v.head = {std::string(L.fmt == MC_WFMT_I8 ? "mc_vhead_" : "mc_v_head_") + fmt_name(L.fmt) + "_bfloat", (unsigned)(L.out / 16 + VH_TILES - 1) / VH_TILES, 1, 1,
              BG_THREADS, 0};
    v.argmax = {"mc_v_argmax_bfloat", 1, (unsigned)M, 1, 1024, 0};
    const unsigned gx = std::min(64u, ((unsigned)c.vocab / 8 + 255) / 256);
    v.accept = {tree ? "mc_tv_accept" : "mc_v_accept", gx, (unsigned)nseg, 1, 256, 0};
    if (tree) v.compact = {"mc_tv_compact_bfloat", ((unsigned)(c.n_kv_heads * c.head_dim) + 255) / 256, (unsigned)nseg, (unsigned)n_layers, 256, 0};
    return v;
}

// ---------------------------------------------------------------- a verify call whose rows carry settings (Part 2m)

// The per-packed-row table of a verify call (abi.h verify_row) and its pick: chunk row j of batch row r draws with seed pair (j * B + r) %
// n_pairs -- token j of row r in mc_ragged_generate -- a tree's node at depth d with (d * B + r) % n_pairs (siblings are alternatives for one
// draw); a chain's anc word is (2 << j) - 1, a tree's the node's (nodes: the call's tv_node table in packed order, null = chains).  greedy: no
// row IN THE CALL samples -- plan_verify_head's mc_v_argmax_bfloat stays and nothing here is launched.  Otherwise first / second take its place
// over the M packed rows, with the kpad of the largest top_k among the call's sampling rows (rows outside the call do not count).
struct verify_pick_plan {
    std::string refusal; // (MC_ERR_RUNTIME)
    bool greedy = true;
    launch_plan first, second;
    sampler_params sp{};
    uint32_t chunk = 0;
    std::vector<verify_row> table; // [M]
};
inline verify_pick_plan
plan_verify_pick(const int32_t* lens, const std::vector<row_setting>& rows, const decoder_sampler& dec, int vocab, int n_pairs, const tv_node* nodes,
                 size_t cand_per_row)
{
    const int B = (int)rows.size();
    verify_pick_plan v;
    int top_k_max = 0;
    decoder_sampler first_sampling;
    for (int r = 0, off = 0; r < B; off += lens[r], r++) {
        if (lens[r] <= 0) continue;
        const decoder_sampler e = sampler_of_row(rows[r], dec);
        const bool samples = e.kind != MC_SAMPLER_GREEDY;
        const row_sampler rs = row_sampler_of(e, vocab);
        if (samples && v.greedy) first_sampling = e;
        if (samples) v.greedy = false, top_k_max = std::max(top_k_max, e.top_k);
        for (int32_t j = 0; j < lens[r]; j++) {
            const int32_t depth = nodes ? nodes[off + j].depth : j;
            const uint32_t anc = nodes ? nodes[off + j].anc : (2u << j) - 1u;
            const uint32_t seed = n_pairs > 0 ? (uint32_t)(((int64_t)depth * B + r) % n_pairs) : 0u;
            v.table.push_back(verify_row{rs, seed, anc, r, off});
        }
    }
    if (v.greedy) return v;
    v.refusal = sampler_plan(top_k_max, vocab, first_sampling.inv_temp_T, first_sampling.top_p_T, &v.sp, &v.chunk);
    if (v.refusal.empty() && (size_t)v.sp.nlists * v.sp.kpad > cand_per_row) v.refusal = SAMPLER_ROW_TOO_LONG;
    if (!v.refusal.empty()) return v;
    const unsigned M = (unsigned)v.table.size();
    v.first = {"mc_vs_topk_candidates_mixed_bfloat", v.sp.nlists, M, 1, 64, 0};
    v.second = {"mc_vs_pick_mixed_bfloat", 1, M, 1, 1024, v.sp.cap * 8};
    return v;
}

// ... and its logit processors: the [B] table is the step's (plan_logits), what decides is whether a row IN THE CALL has anything set (any: ONE
// process launch over the M packed rows between the head and the pick) and whether one has penalties (count: ONE launch behind the acceptance
// that adds the accepted path to those rows' counts)
struct verify_logits_plan {
    bool any = false, count = false;
    std::vector<row_logits> table; // [B]
    launch_plan process, counting;
};
inline verify_logits_plan
plan_verify_logits(const int32_t* lens, const std::vector<row_logit_setting>& rows, int vocab, int M, int nseg)
{
    verify_logits_plan p;
    for (size_t r = 0; r < rows.size(); r++) {
        if (lens[r] <= 0) continue;
        p.any = p.any || rows[r].masked || rows[r].penalised();
        p.count = p.count || rows[r].penalised();
    }
    if (!p.any) return p;
    p.table = plan_logits(rows, vocab, true).table;
    p.process = {"mc_vs_logits_process_bfloat", ((unsigned)vocab + LP_CHUNK - 1) / LP_CHUNK, (unsigned)M, 1, LP_THREADS, 0};
    if (p.count) p.counting = {"mc_vs_count_accepted", (unsigned)nseg, 1, 1, 64, 0};
    return p;
}

// mc_settings_verify_set's value
inline std::string
check_verify_switch(int32_t enable)
{
    return enable == 0 || enable == 1 ? "" : "mc_settings_verify_set: enable must be 0 or 1";
}

// ---------------------------------------------------------------- the checks of a call ("" = fine)

// the row (and, for a call that names one, the layer) of the call `who` on a batch of B rows; B < 0: the batch itself is null
inline std::string
check_row(const char* who, int B, int32_t row, int n_layers = -1, int32_t layer = 0)
{
    if (B < 0) return std::string(who) + ": null argument";
    if (row < 0 || row >= B) return std::string(who) + ": row out of range";
    if (n_layers >= 0 && (layer < 0 || layer >= n_layers)) return std::string(who) + ": layer out of range";
    return "";
}

inline std::string
check_tokens(const int32_t* tokens, int B, int vocab)
{
    for (int r = 0; r < B; r++)
        if (tokens[r] < 0 || tokens[r] >= vocab) return "mc_batch: token id outside the vocabulary";
    return "";
}

// the lockstep bounds of mc_batch_step and mc_batch_generate
inline std::string
step_bounds(int32_t start_pos, int max_seq_len)
{
    if (start_pos < 0 || start_pos + 1 > max_seq_len) return "mc_batch_step: start_pos + 1 must not exceed max_seq_len (a batch's cache does not roll)";
    return "";
}
inline std::string
generate_bounds(int32_t start_pos, int32_t n, int max_seq_len)
{
    if (start_pos < 0 || (int64_t)start_pos + n > max_seq_len)
        return "mc_batch_generate: start_pos + n must not exceed max_seq_len (a batch's cache does not roll)";
    return "";
}

// a ragged call's positions and tokens against the rows' lengths: -1 = idle, else 0 <= pos <= the row's length and pos < max_seq_len (a rolling
// batch: any pos, as long as the n steps of the call stay inside int32), with a token of the vocabulary; at least one row active
inline std::string
check_ragged(const char* what, const int32_t* tokens, const int32_t* positions, int32_t n, const int32_t* lengths, int B, int max_seq_len, int vocab,
             bool rolling)
{
    int active = 0;
    for (int r = 0; r < B; r++) {
        const int32_t pos = positions[r];
        if (pos == -1) continue;
        const std::string row = std::string(what) + ": row " + std::to_string(r) + ": ";
        if (pos < -1) return row + "position below -1 (-1 = idle)";
        if (!rolling && pos >= max_seq_len) return row + "position " + std::to_string(pos) + " must be below max_seq_len (a batch's cache does not roll)";
        if (rolling && (int64_t)pos + n > INT32_MAX) return row + "position " + std::to_string(pos) + " + n leaves the range of positions";
        if (pos > lengths[r])
            return row + "position " + std::to_string(pos) + " is past the row's length " + std::to_string(lengths[r]) +
                   " (its cache has no slots written beyond it)";
        if (const std::string why = rolled_rewind(lengths[r], max_seq_len, pos); !why.empty()) return row + why;
        if (tokens[r] < 0 || tokens[r] >= vocab) return row + "token id outside the vocabulary";
        active++;
    }
    if (!active) return std::string(what) + ": no active row (every position is -1)";
    return "";
}

// mc_verify_rows / mc_tree_verify (`who`): every row in the call (lens[r] > 0) must pick greedily.  A batch without row samplers keeps the
// decoder-wide refusal and its text
inline std::string
verify_samplers(const char* who, const int32_t* lens, const std::vector<row_setting>& rows, const decoder_sampler& dec)
{
    const bool any_set = std::any_of(rows.begin(), rows.end(), [](const row_setting& r) { return r.kind != MC_SAMPLER_INHERIT; });
    if (!any_set) {
        if (dec.kind == MC_SAMPLER_GREEDY) return "";
        return std::string(who) + ": the decoder's sampler is not greedy (accepting sampled drafts needs the draft's probabilities)";
    }
    for (size_t r = 0; r < rows.size(); r++)
        if (lens[r] > 0 && sampler_of_row(rows[r], dec).kind != MC_SAMPLER_GREEDY)
            return std::string(who) + ": row " + std::to_string(r) + ": the row's sampler is not greedy (accepting sampled drafts needs the draft's probabilities)";
    return "";
}

// ... and a row in the call with a mask or penalties is refused (its chunk rows would each need them)
inline std::string
verify_logit_rows(const char* who, const int32_t* lens, const std::vector<row_logit_setting>& rows)
{
    for (size_t r = 0; r < rows.size(); r++)
        if (lens[r] > 0 && (rows[r].masked || rows[r].penalised()))
            return std::string(who) + ": row " + std::to_string(r) + ": the row has a token mask or penalties (a verify call would need them per chunk row)";
    return "";
}

} // namespace mcimpl
