// plan_block() (metalchat_amd/csrc/block_plan.h) from the command line, without HIP: one case per line of standard input,
//
//     15 shape  6 model  16 env  2 state  [FIELD=value ...]
//
// shape: fmt out in group lora_cols of wq|wk|wv, Wo and w1|w3; model: family n_heads n_kv_heads head_dim dim max_seq_len; env: tb qmode cus nsplit
// n_own granules pv_ranges and the nine occupancy answers (fused wo wo_w wo_i8 wo_qkn qkv_qkn qkv_only wo_i4_wide w13); state: attn_fused_on, a
// post-norm pending.  FIELD is a member of decoder_options (the switches a case sets; everything else at its default).  The type name is "bfloat"
// where tb is 2, else "float".  Answered by one line
//
//     form name tiles vsh ns grid fast chain_f chain_p qkv_gemv rope_kv wo_gemv pv_fold pv_ranges pv_block pv_reduce uses_handoffs
//
// the last being block_uses_handoffs().  tests/test_block_plan_cpu.py feeds it tests/golden/decode_block_plans.json.
#include "../../metalchat_amd/csrc/block_plan.h"

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
    MC_FIELD(dbg_variant)
    MC_FIELD(attn_fused)
    MC_FIELD(attn_fused_max_wgs_per_cu)
    MC_FIELD(attn_t2_on)
    MC_FIELD(handoff_fast)
    MC_FIELD(attn_wo_on)
    MC_FIELD(attn_wo_k4)
    MC_FIELD(attn_qkv_on)
    MC_FIELD(attn_qkv_only_on)
    MC_FIELD(attn_i8_on)
    MC_FIELD(attn_i4_wide_on)
    MC_FIELD(kv_virtual_on)
    MC_FIELD(chain_w13_on)
    MC_FIELD(chain_f)
    MC_FIELD(attn_qkv_qkn_on)
    MC_FIELD(attn_wo_qkn_on)
    MC_FIELD(attn_qkn_on)
    MC_FIELD(pv_fold_on)
    MC_FIELD(pv_block)
    MC_FIELD(pv_ranges)
#undef MC_FIELD
    return false;
}

int
main()
{
    static const char* const forms[] = {"qkv_wo_w13_w", "qkv_wo_w", "qkv_wo_i8", "qkv_wo_i4", "qkv_only", "qkv_wo_qkn",
                                        "wo_qkn",       "wo_i4",    "fused",     "fused_qkn", "fused_t2", "scores_pv"};
    std::string line;
    while (std::getline(std::cin, line)) {
        if (line.empty()) continue;
        std::istringstream in(line);
        block_shape L{};
        block_model m{};
        decoder_options opt;
        block_env e{};
        block_state st{};
        int granules = 0, fused_on = 0, pending = 0;
        gemv_shape* lin[3] = {&L.qkv, &L.wo, &L.w13};
        for (gemv_shape* s : lin) in >> s->fmt >> s->out >> s->in >> s->group >> s->lora_cols;
        in >> m.family >> m.n_heads >> m.n_kv_heads >> m.head_dim >> m.dim >> m.max_seq_len;
        in >> e.g.tb >> e.g.qmode >> e.g.cus >> e.nsplit >> e.n_own >> granules >> e.pv_ranges;
        block_occupancy& o = e.occ;
        in >> o.fused >> o.wo >> o.wo_w >> o.wo_i8 >> o.wo_qkn >> o.qkv_qkn >> o.qkv_only >> o.wo_i4_wide >> o.w13;
        if (!(in >> fused_on >> pending)) {
            fprintf(stderr, "bad case: %s\n", line.c_str());
            return 2;
        }
        e.g.pick_slots = 1024; // mc_decoder::pick_slots
        e.g.opt = &opt;
        e.granules = granules != 0;
        e.tname = e.g.tb == 2 ? "bfloat" : "float";
        st.attn_fused_on = fused_on != 0;
        st.pending_pn = pending != 0;
        std::string kv;
        while (in >> kv) {
            const size_t eq = kv.find('=');
            if (eq == std::string::npos || !set_field(opt, kv.substr(0, eq), atoi(kv.c_str() + eq + 1))) {
                fprintf(stderr, "bad switch: %s\n", kv.c_str());
                return 2;
            }
        }
        const block_plan P = plan_block(L, m, e, st);
        printf("%s %s %d %d %d %u %u %d %d %d %d %d %d %d %u %d %d\n", forms[(int)P.form], P.name.c_str(), P.tiles, P.vsh, P.ns, P.grid, P.fast, P.chain_f,
               P.chain_p, P.qkv_gemv ? 1 : 0, P.rope_kv ? 1 : 0, P.wo_gemv ? 1 : 0, P.pv_fold ? 1 : 0, P.pv_ranges, P.pv_block, P.pv_reduce ? 1 : 0,
               block_uses_handoffs(m, e, st) ? 1 : 0);
    }
    return 0;
}
