// What a batch launches (metalchat_amd/csrc/batch_plan.h, and in which order: batch_call_plan.h) from the command line, without HIP: one request per line of standard input, one line of
// JSON per answer.  A linear is seven words, `fmt out in group ngroups lora lora_cols`; a launch is answered as [name, gx, gy, gz, block, lds];
// a refusal as {"refused": "<text>"}.
//
//     admit    wide family dtype layer_begin layer_end n_layers weight_format group_size qmode head_dim n_heads n_kv_heads max_seq_len dim vocab
//              emb_fmt nlayers {qkv wo w13 w2}[nlayers] output                                   -> {"admitted": true}
//     gemv     linear epi B cus tiles_env                                                        -> {"wide", "launches": [the adaptor's, the main]}
//     step     dim n_heads n_kv_heads head_dim B nsplit ragged rolling                           -> {"begin", "embed", "rmsnorm", "rope", "scores", "pv"}
//     head     vocab ragged cand_per_row  kind top_k temperature top_p (the decoder's)  B  {kind top_k temperature top_p}[B] (kind -1: inherits)
//                                                                                                -> {"form", "launches", "sp", "chunk", "table"}
//     logits   vocab ragged B {masked rep freq pres}[B]                                          -> {"any", "launches", "table"}
//     verify   linear (the head) vocab n_kv_heads head_dim n_layers M nseg tree                  -> {"launches"}
//     token    dim n_heads n_kv_heads head_dim n_layers vocab max_seq_len  B cus tiles_env ragged rolling  qkv wo w13 w2 output (linears, every layer
//              alike)  kind top_k temperature top_p (the decoder's)  {kind top_k temperature top_p}[B]  {masked rep freq pres}[B]  logprobs top_n
//                                                  -> {"launches": ONE token of the call in order (batch_call_plan.h plan_batch_token), "ops", "lp_slots"}
//     tail     (the same words; ragged is not read)                                              -> the list behind a prompt pass (plan_rows_tail)
//     ragged   what B max_seq_len vocab rolling n positions[B] tokens[B] lengths[B]              -> {"ok": true}
//     bounds   step start_pos max_seq_len | generate start_pos n max_seq_len | tokens B vocab tokens[B]
//     settings who B  kind (the decoder's)  lens[B] kind[B] {masked rep freq pres}[B]            (the two refusals of a verify call)
//
// The settings are rounded here as mc_decoder_set_sampler and mc_row_sampler_set round them.  tests/test_batch_plan_cpu.py holds the answers to
// a recording of the launches (tests/golden/batch_plans.json), to the tile rule, and to the texts of every refusal.
#include "../../metalchat_amd/csrc/batch_call_plan.h"
#include "../../metalchat_amd/csrc/bf16_host.h"

#include <cstdio>
#include <iostream>
#include <sstream>

using namespace mcimpl;

struct test_layer {
    linear_shape qkv, wo, w13, w2;
};
struct test_parts {
    mc_decoder_config cfg{};
    int emb_fmt = MC_WFMT_T;
    linear_shape output;
    std::vector<test_layer> layers;
};

static bool
read_linear(std::istream& in, linear_shape& L)
{
    int lora = 0;
    if (!(in >> L.fmt >> L.out >> L.in >> L.group >> L.ngroups >> lora >> L.lora_cols)) return false;
    L.lora = lora != 0;
    return true;
}

static bool
read_ints(std::istream& in, std::vector<int32_t>& v, int n)
{
    v.resize(n);
    for (int i = 0; i < n; i++)
        if (!(in >> v[i])) return false;
    return true;
}

static bool
read_logit_rows(std::istream& in, std::vector<row_logit_setting>& rows, int B)
{
    rows.assign(B, row_logit_setting{});
    for (row_logit_setting& r : rows) {
        int masked = 0;
        if (!(in >> masked >> r.rep >> r.freq >> r.pres)) return false;
        r.masked = masked != 0;
    }
    return true;
}

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

static void
answer_refusal(const std::string& why, const char* fine)
{
    if (why.empty()) printf("{\"%s\": true}\n", fine);
    else printf("{\"refused\": \"%s\"}\n", why.c_str());
}

static bool
admit(std::istream& in)
{
    test_parts p;
    mc_decoder_config& c = p.cfg;
    int wide = 0, nlayers = 0;
    if (!(in >> wide >> c.family >> c.dtype >> c.layer_begin >> c.layer_end >> c.n_layers >> c.weight_format >> c.group_size >> c.qmode >> c.head_dim >>
          c.n_heads >> c.n_kv_heads >> c.max_seq_len >> c.dim >> c.vocab >> p.emb_fmt >> nlayers) ||
        nlayers < 0 || nlayers > 64)
        return false;
    p.layers.resize(nlayers);
    for (test_layer& L : p.layers)
        if (!read_linear(in, L.qkv) || !read_linear(in, L.wo) || !read_linear(in, L.w13) || !read_linear(in, L.w2)) return false;
    if (!read_linear(in, p.output)) return false;
    answer_refusal(refusal(p, wide != 0), "admitted");
    return true;
}

static bool
gemv(std::istream& in)
{
    linear_shape L;
    int epi = 0;
    batch_env e;
    if (!read_linear(in, L) || !(in >> epi >> e.B >> e.cus >> e.tiles_env)) return false;
    const batch_gemv_plan g = plan_batch_gemv(L, epi, e);
    std::vector<launch_plan> ls;
    if (g.lora) ls.push_back(g.adaptor);
    ls.push_back(g.main);
    printf("{\"wide\": %s, \"launches\": %s}\n", g.wide ? "true" : "false", js(ls).c_str());
    return true;
}

static bool
step(std::istream& in)
{
    mc_decoder_config c{};
    int B = 0, nsplit = 0, ragged = 0, rolling = 0;
    if (!(in >> c.dim >> c.n_heads >> c.n_kv_heads >> c.head_dim >> B >> nsplit >> ragged >> rolling)) return false;
    const step_plan s = plan_step(c, B, nsplit, ragged != 0, rolling != 0);
    printf("{\"begin\": %s, \"embed\": %s, \"rmsnorm\": %s, \"rope\": %s, \"scores\": %s, \"pv\": %s}\n", js(s.begin).c_str(), js(s.embed).c_str(),
           js(s.rmsnorm).c_str(), js(s.rope).c_str(), js(s.scores).c_str(), js(s.pv).c_str());
    return true;
}

// (kind, top_k, temperature, top_p) as the caller gives them -> the rounded settings the host keeps
static bool
read_sampler(std::istream& in, int& kind, int& top_k, float& inv_temp_T, float& top_p_T)
{
    float temperature = 0.0f, top_p = 0.0f;
    if (!(in >> kind >> top_k >> temperature >> top_p)) return false;
    inv_temp_T = kind == MC_SAMPLER_DEFAULT ? round_bf_host(1.0f / round_bf_host(temperature)) : 0.0f;
    top_p_T = kind == MC_SAMPLER_DEFAULT ? round_bf_host(top_p) : 0.0f;
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
        answer_refusal(h.refusal, "");
        return true;
    }
    std::vector<launch_plan> ls{h.first};
    if (h.form != PICK_GREEDY) ls.push_back(h.second);
    printf("{\"form\": \"%s\", \"launches\": %s, ", h.form == PICK_GREEDY ? "greedy" : (h.form == PICK_UNIFORM ? "uniform" : "mixed"), js(ls).c_str());
    printf("\"sp\": {\"k\": %u, \"ncand\": %u, \"cap\": %u, \"inv_temp\": %.9g, \"top_p\": %.9g, \"nlists\": %u, \"kpad\": %u}, \"chunk\": %u, \"table\": [", h.sp.k,
           h.sp.ncand, h.sp.cap, h.sp.inv_temp, h.sp.top_p, h.sp.nlists, h.sp.kpad, h.chunk);
    for (int r = 0; r < B; r++)
        printf("%s[%d, %u, %.9g, %.9g]", r ? ", " : "", h.table[r].kind, h.table[r].k, h.table[r].inv_temp, h.table[r].top_p);
    printf("]}\n");
    return true;
}

static bool
logits(std::istream& in)
{
    int vocab = 0, ragged = 0, B = 0;
    std::vector<row_logit_setting> rows;
    if (!(in >> vocab >> ragged >> B) || B < 1 || B > MC_WIDE_BATCH_MAX || !read_logit_rows(in, rows, B)) return false;
    const logits_plan p = plan_logits(rows, vocab, ragged != 0);
    printf("{\"any\": %s, \"launches\": %s, \"table\": [", p.any ? "true" : "false", js(p.any ? std::vector<launch_plan>{p.launch} : std::vector<launch_plan>{}).c_str());
    for (int r = 0; r < B; r++)
        printf("%s[%u, %.9g, %.9g, %.9g, %.9g]", r ? ", " : "", p.table[r].flags, p.table[r].rep, p.table[r].inv_rep, p.table[r].freq, p.table[r].pres);
    printf("]}\n");
    return true;
}

static bool
verify(std::istream& in)
{
    linear_shape L;
    mc_decoder_config c{};
    int n_layers = 0, M = 0, nseg = 0, tree = 0;
    if (!read_linear(in, L) || !(in >> c.vocab >> c.n_kv_heads >> c.head_dim >> n_layers >> M >> nseg >> tree)) return false;
    const verify_plan v = plan_verify_head(L, c, n_layers, M, nseg, tree != 0);
    std::vector<launch_plan> ls{v.norm, v.head, v.argmax, v.accept};
    if (v.tree) ls.push_back(v.compact);
    printf("{\"launches\": %s}\n", js(ls).c_str());
    return true;
}

static bool
token(std::istream& in, bool tail)
{
    test_parts p;
    mc_decoder_config& c = p.cfg;
    batch_env e;
    int n_layers = 0, is_ragged = 0, rolling = 0, logprobs = 0, top_n = 0;
    test_layer L;
    if (!(in >> c.dim >> c.n_heads >> c.n_kv_heads >> c.head_dim >> n_layers >> c.vocab >> c.max_seq_len >> e.B >> e.cus >> e.tiles_env >> is_ragged >> rolling) ||
        n_layers < 0 || n_layers > 64 || e.B < 1 || e.B > MC_WIDE_BATCH_MAX || !read_linear(in, L.qkv) || !read_linear(in, L.wo) || !read_linear(in, L.w13) ||
        !read_linear(in, L.w2) || !read_linear(in, p.output))
        return false;
    p.layers.assign(n_layers, L);
    decoder_sampler dec;
    if (!read_sampler(in, dec.kind, dec.top_k, dec.inv_temp_T, dec.top_p_T)) return false;
    std::vector<row_setting> rows(e.B);
    for (row_setting& r : rows) {
        int kind = 0, top_k = 0;
        if (!read_sampler(in, kind, top_k, r.inv_temp_T, r.top_p_T)) return false;
        r.kind = kind;
        r.top_k = top_k;
    }
    std::vector<row_logit_setting> lrows;
    if (!read_logit_rows(in, lrows, e.B) || !(in >> logprobs >> top_n)) return false;
    const batch_fixed f = fix_batch(p, e);
    const call_settings s{rolling != 0, false, logprobs != 0, top_n, 0, dec, rows, lrows};
    const batch_call_plan plan = tail ? plan_rows_tail(f, s) : plan_batch_token(f, s, is_ragged != 0);
    if (!plan.refusal.empty()) {
        answer_refusal(plan.refusal, "");
        return true;
    }
    std::vector<launch_plan> ls;
    std::string ops = "[";
    for (const batch_launch& l : plan.listed()) {
        ops += (ls.empty() ? "[" : ", [") + std::to_string((int)l.op) + ", " + std::to_string(l.layer) + "]";
        ls.push_back(l.L);
    }
    printf("{\"launches\": %s, \"ops\": %s], \"lp_slots\": %d}\n", js(ls).c_str(), ops.c_str(), plan.lp_slots);
    return true;
}

static bool
ragged(std::istream& in)
{
    std::string what;
    int B = 0, S = 0, vocab = 0, rolling = 0, n = 0;
    std::vector<int32_t> pos, tokens, lengths;
    if (!(in >> what >> B >> S >> vocab >> rolling >> n) || B < 1 || B > MC_WIDE_BATCH_MAX || !read_ints(in, pos, B) || !read_ints(in, tokens, B) ||
        !read_ints(in, lengths, B))
        return false;
    answer_refusal(check_ragged(what.c_str(), tokens.data(), pos.data(), n, lengths.data(), B, S, vocab, rolling != 0), "ok");
    return true;
}

static bool
bounds(std::istream& in)
{
    std::string which;
    int a = 0, b = 0, c = 0;
    if (!(in >> which)) return false;
    if (which == "step" && (in >> a >> b)) answer_refusal(step_bounds(a, b), "ok");
    else if (which == "generate" && (in >> a >> b >> c)) answer_refusal(generate_bounds(a, b, c), "ok");
    else if (which == "tokens" && (in >> a >> b) && a >= 1 && a <= MC_WIDE_BATCH_MAX) {
        std::vector<int32_t> tokens;
        if (!read_ints(in, tokens, a)) return false;
        answer_refusal(check_tokens(tokens.data(), a, b), "ok");
    } else
        return false;
    return true;
}

static bool
settings(std::istream& in)
{
    std::string who;
    int B = 0;
    decoder_sampler dec;
    std::vector<int32_t> lens, kinds;
    std::vector<row_logit_setting> lrows;
    if (!(in >> who >> B >> dec.kind) || B < 1 || B > MC_WIDE_BATCH_MAX || !read_ints(in, lens, B) || !read_ints(in, kinds, B) || !read_logit_rows(in, lrows, B))
        return false;
    std::vector<row_setting> rows(B);
    for (int r = 0; r < B; r++) rows[r].kind = kinds[r];
    std::string why = verify_samplers(who.c_str(), lens.data(), rows, dec);
    if (why.empty()) why = verify_logit_rows(who.c_str(), lens.data(), lrows);
    answer_refusal(why, "ok");
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
        const bool ok = kind == "admit"      ? admit(in)
                        : kind == "gemv"     ? gemv(in)
                        : kind == "step"     ? step(in)
                        : kind == "head"     ? head(in)
                        : kind == "logits"   ? logits(in)
                        : kind == "verify"   ? verify(in)
                        : kind == "token"    ? token(in, false)
                        : kind == "tail"     ? token(in, true)
                        : kind == "ragged"   ? ragged(in)
                        : kind == "bounds"   ? bounds(in)
                        : kind == "settings" ? settings(in)
                                             : false;
        if (!ok) {
            fprintf(stderr, "bad request: %s\n", line.c_str());
            return 2;
        }
    }
    return 0;
}
