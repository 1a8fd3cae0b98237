// plan_token() (metalchat_amd/csrc/token_plan.h) from the command line, without HIP: one token per line of standard input,
//
//     6 model  16 env  5 fixed  6 state  5 head  n_layers  20 per layer  [FIELD=value ...]
//
// model: family n_heads n_kv_heads head_dim dim max_seq_len; env: tb qmode cus nsplit n_own granules pv_ranges and the nine occupancy answers (as
// test_block_plan.cc); fixed: first_stage last_stage emb_fmt vocab top_k; state: attn_fused_on want_taps sampler_kind lazy advance in_hidden; head and, per
// owned block, wq|wk|wv, Wo, w1|w3 and w2: fmt out in group lora_cols.  FIELD is a member of decoder_options.  Answered by one line per step
//
//     op layer name gx gy gz block lds pro epi adaptor pn_by_value x y res res_row res_layer norm advance fold_keys
//
// and a last line "end lazy=<0|1> head_behind_post_norm=<0|1> lazy_if_nothing_pending=<0|1> error=<text>" -- the third is lazy_pick_ok() asked as if no
// post-norm were pending in front of the head, whatever the truth: what a caller outside the token used to get.  Before it answers, the program holds every GEMV step against plan_gemv and every block against
// plan_block for the same inputs -- the pending flag worked out here, not taken from the plan -- and leaves with status 3 where they differ: the three
// headers cannot drift.  tests/test_token_plan_cpu.py feeds it the cases of tests/golden/decode_token_plans.json.
#include "../../metalchat_amd/csrc/token_plan.h"

#include <cstdio>
#include <iostream>
#include <sstream>

static bool
set_field(decoder_options& o, const std::string& field, int v)
{
#define MC_FIELD(f) \
    if (field == #f) { \
        o.f = static_cast<decltype(o.f)>(v); \
        return true; \
    }
    MC_FIELD(gemv_lin)
    MC_FIELD(gemv_ling)
    MC_FIELD(lin_split)
    MC_FIELD(lin_waves)
    MC_FIELD(gemv_m4)
    MC_FIELD(attn_fused)
    MC_FIELD(attn_wo_on)
    MC_FIELD(attn_qkv_on)
    MC_FIELD(pv_fold_on)
    MC_FIELD(gemma_fuse)
    MC_FIELD(head_pick_mode)
    MC_FIELD(head_pick_on)
    MC_FIELD(lazy_pick_on)
#undef MC_FIELD
    return false;
}

static const char* const OPS[] = {"park_row", "embed", "qkv_gemv", "rope_kv", "attn", "scores", "pv", "pv_reduce", "wo_gemv", "post_norm_attn",
                                  "w13_gemv", "w2_gemv", "post_norm_ffn", "tap", "head_gemv", "fold_pick", "argmax", "candidates", "sample"};
static const char* const ROWS[] = {"-", "in", "hidden", "hidden_b", "proj", "qkv", "q_rot", "gate", "attn_out", "pv_parts", "logits"};
static const char* const RES[] = {"-", "row", "qkv_epi", "pn_attn", "pn_ffn", "pick_atomic", "pick_per_wg"};
static const char* const NORMS[] = {"-", "attention", "ffn", "final"};

static bool
is_gemv(token_op op)
{
    return op == token_op::qkv_gemv || op == token_op::wo_gemv || op == token_op::w13_gemv || op == token_op::w2_gemv || op == token_op::head_gemv;
}

// every GEMV step is plan_gemv's answer, every block plan_block's, for the same inputs
static bool
consistent(const token_plan& P, const token_fixed& f, const token_state& st)
{
    const bool pn_folded = f.m.family == MC_FAMILY_GEMMA3 && !st.want_taps && f.e->g.opt->gemma_fuse && (size_t)f.m.dim * f.e->g.tb / 16 <= (size_t)4 * f.e->g.opt->gemv_block;
    if (P.blocks.size() != f.layers.size()) return false;
    for (size_t li = 0; li < f.layers.size(); li++) {
        // (a folded ffn post-norm waits in front of every block but the stage's first)
        const block_plan B = plan_block(f.layers[li].b, f.m, *f.e, block_state{st.attn_fused_on, pn_folded && li > 0});
        const block_plan& Q = P.blocks[li];
        if (B.form != Q.form || B.name != Q.name || B.grid != Q.grid || B.tiles != Q.tiles || B.vsh != Q.vsh || B.ns != Q.ns || B.fast != Q.fast ||
            B.qkv_gemv != Q.qkv_gemv || B.rope_kv != Q.rope_kv || B.wo_gemv != Q.wo_gemv || B.pv_fold != Q.pv_fold || B.pv_ranges != Q.pv_ranges ||
            B.pv_block != Q.pv_block || B.pv_reduce != Q.pv_reduce) {
            fprintf(stderr, "block %zu: plan_token holds %s, plan_block says %s\n", li, Q.name.c_str(), B.name.c_str());
            return false;
        }
    }
    for (const token_step& s : P.steps) {
        if (s.op == token_op::attn || s.op == token_op::scores) {
            const block_plan& B = P.blocks[s.layer];
            if (s.L.name != B.name || (s.op == token_op::attn && s.L.gx != B.grid)) {
                fprintf(stderr, "block %d: the step launches %s, its plan says %s\n", s.layer, s.L.name.c_str(), B.name.c_str());
                return false;
            }
        }
        if (!is_gemv(s.op)) continue;
        const token_layer* L = s.layer >= 0 ? &f.layers[s.layer] : nullptr;
        gemv_shape W = s.op == token_op::head_gemv ? f.head : s.op == token_op::qkv_gemv ? L->b.qkv : s.op == token_op::wo_gemv ? L->b.wo
                     : s.op == token_op::w13_gemv ? L->b.w13 : L->w2;
        if (s.adaptor) W = gemv_shape{MC_WFMT_T, W.lora_cols, W.in, 0, 0};
        const gemv_plan G = plan_gemv(W, f.e->g, s.pro, s.epi);
        if (G.error || G.name != s.L.name || G.wgs != s.L.gx || G.block != s.L.block || G.lds != s.L.lds || G.postnorm_by_value != s.pn_by_value || s.L.gy != 1 || s.L.gz != 1) {
            fprintf(stderr, "%s of block %d: the step launches %s, plan_gemv says %s\n", OPS[(int)s.op], s.layer, s.L.name.c_str(), G.name.c_str());
            return false;
        }
    }
    return true;
}

int
main()
{
    std::string line;
    while (std::getline(std::cin, line)) {
        if (line.empty()) continue;
        std::istringstream in(line);
        decoder_options opt;
        block_env e{};
        token_fixed f{};
        token_state st{};
        int granules = 0, first = 0, last = 0, fused_on = 0, taps = 0, lazy = 0, advance = 0, in_hidden = 0, n_layers = 0;
        auto shape = [&in](gemv_shape& s) { in >> s.fmt >> s.out >> s.in >> s.group >> s.lora_cols; };
        in >> f.m.family >> f.m.n_heads >> f.m.n_kv_heads >> f.m.head_dim >> f.m.dim >> f.m.max_seq_len;
        in >> e.g.tb >> e.g.qmode >> e.g.cus >> e.nsplit >> e.n_own >> granules >> e.pv_ranges;
        block_occupancy& o = e.occ;
        in >> o.fused >> o.wo >> o.wo_w >> o.wo_i8 >> o.wo_qkn >> o.qkv_qkn >> o.qkv_only >> o.wo_i4_wide >> o.w13;
        in >> first >> last >> f.emb_fmt >> f.vocab >> f.top_k;
        in >> fused_on >> taps >> st.sampler_kind >> lazy >> advance >> in_hidden;
        shape(f.head);
        if (!(in >> n_layers) || n_layers < 0 || n_layers > 1024) {
            fprintf(stderr, "bad case: %s\n", line.c_str());
            return 2;
        }
        f.layers.resize(n_layers);
        for (token_layer& L : f.layers) {
            shape(L.b.qkv);
            shape(L.b.wo);
            shape(L.b.w13);
            shape(L.w2);
        }
        if (!in) {
            fprintf(stderr, "bad case: %s\n", line.c_str());
            return 2;
        }
        e.g.pick_slots = 1024; // mc_decoder::pick_slots
        e.g.opt = &opt;
        e.granules = granules != 0;
        e.tname = e.g.tb == 2 ? "bfloat" : "float";
        f.e = &e;
        f.first_stage = first != 0;
        f.last_stage = last != 0;
        f.inv_temp_T = 1.0f;
        f.top_p_T = 0.5f;
        st.attn_fused_on = fused_on != 0;
        st.want_taps = taps != 0;
        st.lazy = lazy != 0;
        st.advance = advance != 0;
        st.in_hidden = in_hidden != 0;
        std::string kv;
        while (in >> kv) {
            const size_t eq = kv.find('=');
            if (eq == std::string::npos || !set_field(opt, kv.substr(0, eq), atoi(kv.c_str() + eq + 1))) {
                fprintf(stderr, "bad switch: %s\n", kv.c_str());
                return 2;
            }
        }
        const token_plan P = plan_token(f, st);
        if (P.error.empty() && !consistent(P, f, st)) return 3;
        for (const token_step& s : P.steps)
            printf("%s %d %s %u %u %u %u %u %d %d %d %d %s %s %s %s %d %s %d %d\n", OPS[(int)s.op], s.layer, s.L.name.empty() ? "-" : s.L.name.c_str(), s.L.gx, s.L.gy,
                   s.L.gz, s.L.block, s.L.lds, s.pro, s.epi, s.adaptor ? 1 : 0, s.pn_by_value ? 1 : 0, ROWS[(int)s.x], ROWS[(int)s.y], RES[(int)s.res],
                   ROWS[(int)s.res_row], s.res_layer, NORMS[(int)s.norm], s.advance ? 1 : 0, s.fold_keys ? 1 : 0);
        printf("end lazy=%d head_behind_post_norm=%d lazy_if_nothing_pending=%d error=%s\n", P.lazy ? 1 : 0, head_behind_post_norm(f, st) ? 1 : 0,
               lazy_pick_ok(f, st, false) ? 1 : 0, P.error.c_str());
    }
    return 0;
}
