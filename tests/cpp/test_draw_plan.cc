// The pick of a batch with MC_SAMPLER_DRAW rows (metalchat_amd/csrc/batch_plan.h plan_head) from the command line, without HIP: one request per
// line of standard input, one line of JSON per answer, in the formats of test_batch_plan.cc's `head` request:
//
//     head     vocab ragged cand_per_row  kind top_k temperature top_p (the decoder's)  B  {kind top_k temperature top_p}[B] (kind -1: inherits)
//                                                                                                -> {"form", "launches", "sp", "chunk", "table"}
//
// The settings of EVERY sampling kind are rounded here as mc_decoder_set_sampler and mc_row_sampler_set round them (test_batch_plan.cc rounds
// MC_SAMPLER_DEFAULT's alone).  tests/test_draw_plan_cpu.py holds the answers.
#include "../../metalchat_amd/csrc/batch_plan.h"
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

static bool
read_sampler(std::istream& in, int& kind, int& top_k, float& inv_temp_T, float& top_p_T)
{
    float temperature = 0.0f, top_p = 0.0f;
    if (!(in >> kind >> top_k >> temperature >> top_p)) return false;
    const bool samples = kind == MC_SAMPLER_DEFAULT || kind == MC_SAMPLER_DRAW;
    inv_temp_T = samples ? round_bf_host(1.0f / round_bf_host(temperature)) : 0.0f;
    top_p_T = samples ? round_bf_host(top_p) : 0.0f;
    return true;
}

static bool
head(std::istream& in)
{
    int vocab = 0, ragged = 0, B = 0;
    size_t cand = 0;
    decoder_sampler dec;
    if (!(in >> vocab >> ragged >> cand) || !read_sampler(in, dec.kind, dec.top_k, dec.inv_temp_T, dec.top_p_T) || !(in >> B) || B < 1 ||
        B > MC_WIDE_BATCH_MAX)
        return false;
    std::vector<row_setting> rows(B);
    for (row_setting& r : rows) {
        int kind = 0, top_k = 0;
        if (!read_sampler(in, kind, top_k, r.inv_temp_T, r.top_p_T)) return false;
        r.kind = kind;
        r.top_k = top_k;
    }
    const head_plan h = plan_head(rows, dec, vocab, ragged != 0, cand);
    if (!h.refusal.empty()) {
        printf("{\"refused\": \"%s\"}\n", h.refusal.c_str());
        return true;
    }
    std::string ls = js(h.first);
    if (h.form != PICK_GREEDY) ls += ", " + js(h.second);
    printf("{\"form\": \"%s\", \"launches\": [%s], ", h.form == PICK_GREEDY ? "greedy" : (h.form == PICK_UNIFORM ? "uniform" : "mixed"), ls.c_str());
    printf("\"sp\": {\"k\": %u, \"ncand\": %u, \"cap\": %u, \"inv_temp\": %.9g, \"top_p\": %.9g, \"nlists\": %u, \"kpad\": %u}, \"chunk\": %u, \"table\": [", h.sp.k,
           h.sp.ncand, h.sp.cap, h.sp.inv_temp, h.sp.top_p, h.sp.nlists, h.sp.kpad, h.chunk);
    for (int r = 0; r < B; r++)
        printf("%s[%d, %u, %.9g, %.9g]", r ? ", " : "", h.table[r].kind, h.table[r].k, h.table[r].inv_temp, h.table[r].top_p);
    printf("]}\n");
    return true;
}

int
main()
{
    std::string line;
    while (std::getline(std::cin, line)) {
        if (line.empty()) continue;
        std::istringstream in(line);
        std::string kind;
        in >> kind;
        if (kind != "head" || !head(in)) {
            fprintf(stderr, "bad request: %s\n", line.c_str());
            return 2;
        }
    }
    return 0;
}
