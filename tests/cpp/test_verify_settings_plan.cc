// What a verify call with row settings launches (metalchat_amd/csrc/batch_plan.h plan_verify_pick / plan_verify_logits, Part 2m of the ABI; the whole
// head of the call in order: batch_call_plan.h plan_verify_call) from the command line, without HIP: one request per line of standard input, one line of
// JSON per answer.  A launch is answered as [name, gx, gy, gz, block, lds], a refusal as {"refused": "<text>"}.
//
//     call     vocab n_kv_heads head_dim n_layers n_pairs tree logprobs top_n head_fmt  kind top_k temperature top_p (the decoder's)  B  lens[B]
//              {kind top_k temperature top_p}[B] (kind -1: inherits)  {masked rep freq pres}[B]  parents[sum of lens] (tree only)
//                  -> {"greedy", "kpad", "nlists", "chunk", "cap", "any", "count", "head": plan_verify_head's launches over a head of format head_fmt,
//                      "launches": the whole head of the call as plan_verify_call orders it, "table": [[kind, k, seed, anc, row, off] per packed row]}
//     switch   enable                                                                       -> {"ok": true} or the refusal
//
// The settings are rounded here as mc_decoder_set_sampler and mc_row_sampler_set round them.  tests/test_verify_settings_cpu.py asks.
#include "../../metalchat_amd/csrc/batch_call_plan.h"
#include "../../metalchat_amd/csrc/bf16_host.h"

#include <cstdio>
#include <iostream>
#include <sstream>

using namespace mcimpl;

static std::string
js(const launch_plan& l)
{
    return "[\"" + l.name + "\", " + std::to_string(l.gx) + ", " + std::to_string(l.gy) + ", " + std::to_string(l.gz) + ", " + std::to_string(l.block) + ", " +
           std::to_string(l.lds) + "]";
}

static std::string
js(const std::vector<launch_plan>& ls)
{
    std::string s = "[";
    for (size_t i = 0; i < ls.size(); i++) s += (i ? ", " : "") + js(ls[i]);
    return s + "]";
}

static bool
read_sampler(std::istream& in, int& kind, int& top_k, float& inv_temp_T, float& top_p_T)
{
    float temperature = 0.0f, top_p = 0.0f;
    if (!(in >> kind >> top_k >> temperature >> top_p)) return false;
    inv_temp_T = temperature > 0.0f ? round_bf_host(1.0f / round_bf_host(temperature)) : 0.0f;
    top_p_T = round_bf_host(top_p);
    return true;
}

static bool
call(std::istream& in)
{
    mc_decoder_config c{};
    int n_layers = 0, n_pairs = 0, tree = 0, B = 0, logprobs = 0, top_n = 0;
    linear_shape head;
    decoder_sampler dec;
    if (!(in >> c.vocab >> c.n_kv_heads >> c.head_dim >> n_layers >> n_pairs >> tree >> logprobs >> top_n >> head.fmt) || !read_sampler(in, dec.kind, dec.top_k, dec.inv_temp_T, dec.top_p_T) ||
        !(in >> B) || B < 1 || B > MC_WIDE_BATCH_MAX)
        return false;
    std::vector<int32_t> lens(B);
    int M = 0, nseg = 0, ntiles = 0;
    for (int32_t& l : lens) {
        if (!(in >> l) || l < 0 || l > MC_VERIFY_MAX_LEN) return false;
        M += l;
        nseg += l > 0;
        ntiles += (l + PP_TILE_ROWS - 1) / PP_TILE_ROWS;
    }
    std::vector<row_setting> rows(B);
    for (row_setting& r : rows)
        if (!read_sampler(in, r.kind, r.top_k, r.inv_temp_T, r.top_p_T)) return false;
    std::vector<row_logit_setting> lrows(B);
    for (row_logit_setting& r : lrows) {
        int masked = 0;
        if (!(in >> masked >> r.rep >> r.freq >> r.pres)) return false;
        r.masked = masked != 0;
    }
    // a tree's node table as rows_pass builds it (rows_plan.h)
    std::vector<char> tab;
    const tv_node* nodes = nullptr;
    if (tree) {
        std::vector<int32_t> parents(M), positions(B, 0);
        for (int32_t& p : parents)
            if (!(in >> p)) return false;
        if (const std::string why = tree_check("call", parents.data(), lens.data(), B); !why.empty()) {
            printf("{\"refused\": \"%s\"}\n", why.c_str());
            return true;
        }
        std::vector<step_state> states;
        rows_tables(lens.data(), positions.data(), B, ntiles, states, tab);
        tree_nodes(parents.data(), lens.data(), B, ntiles, M, tab);
        nodes = tv_nodes(tab.data(), ntiles);
    }
    const size_t cand_per_row = (size_t)std::max(((uint32_t)c.vocab + 511) / 512, 1u) * 128; // (batch.cc batch_create)
    const verify_pick_plan vp = plan_verify_pick(lens.data(), rows, dec, c.vocab, n_pairs, nodes, cand_per_row);
    if (!vp.refusal.empty()) {
        printf("{\"refused\": \"%s\"}\n", vp.refusal.c_str());
        return true;
    }
    const verify_logits_plan vl = plan_verify_logits(lens.data(), lrows, c.vocab, M, nseg);
    head.out = c.vocab;
    head.in = 1024;
    const verify_plan vh = plan_verify_head(head, c, n_layers, M, nseg, tree != 0);
    std::vector<launch_plan> before = {vh.norm, vh.head, vh.argmax, vh.accept}, launches;
    if (tree) before.push_back(vh.compact);
    batch_fixed f;
    f.cfg = c;
    f.B = B;
    f.n_layers = n_layers;
    f.cand_per_row = cand_per_row;
    f.head = head;
    const batch_call_plan plan = plan_verify_call(f, call_settings{false, true, logprobs != 0, top_n, n_pairs, dec, rows, lrows}, lens.data(), M, nseg, nodes);
    if (!plan.refusal.empty()) {
        printf("{\"refused\": \"%s\"}\n", plan.refusal.c_str());
        return true;
    }
    for (const batch_launch& l : plan.listed()) launches.push_back(l.L);
    std::string t = "[";
    for (size_t m = 0; m < vp.table.size(); m++) {
        const verify_row& v = vp.table[m];
        t += std::string(m ? ", " : "") + "[" + std::to_string(v.sampler.kind) + ", " + std::to_string(v.sampler.k) + ", " + std::to_string(v.seed) + ", " +
             std::to_string(v.anc) + ", " + std::to_string(v.row) + ", " + std::to_string(v.off) + "]";
    }
    t += "]";
    printf("{\"greedy\": %s, \"kpad\": %u, \"nlists\": %u, \"chunk\": %u, \"cap\": %u, \"any\": %s, \"count\": %s, \"head\": %s, \"launches\": %s, \"table\": %s}\n",
           vp.greedy ? "true" : "false", vp.sp.kpad, vp.sp.nlists, vp.chunk, vp.sp.cap, vl.any ? "true" : "false", vl.count ? "true" : "false", js(before).c_str(),
           js(launches).c_str(), t.c_str());
    return true;
}

int
main()
{
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string what;
        in >> what;
        bool ok = false;
        if (what == "call") ok = call(in);
        else if (what == "switch") {
            int32_t enable = 0;
            if ((ok = (bool)(in >> enable))) {
                const std::string why = check_verify_switch(enable);
                if (why.empty()) printf("{\"ok\": true}\n");
                else printf("{\"refused\": \"%s\"}\n", why.c_str());
            }
        }
        if (!ok) {
            fprintf(stderr, "bad request: %s\n", line.c_str());
            return 2;
        }
    }
    return 0;
}
