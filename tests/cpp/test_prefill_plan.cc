// The prompt plan (metalchat_amd/csrc/prefill_plan.h) from the command line, without HIP: one case per line of standard input,
//
//     KIND tb qmode family cus dim ffn_dim n_heads n_kv_heads head_dim max_seq_len lib_on ARGS... [FIELD=value ...]
//
// where FIELD is a member of decoder_options (the switches a case sets; everything else at its default), answered by one line:
//
//     gemm   fmt out in group lora_cols M epi plain ->  family name gx gy splits block ktper bm
//            (name: the kernel for what the plan writes -- partials or rows; plain: over the dequantised copy of the matrix;
//             the library GEMM: hipblasLtMatmul)
//     attn   M                                      ->  name gx gy block                                  (plan_attention)
//     packed ntiles                                 ->  name gx gy block                                  (plan_packed_attention)
//     extend tree                                   ->  sums pv reduce heads                              (plan_extend_attention)
//     rope   M parts batch qk_norm                  ->  name gx gy block                                  (plan_rope)
//     act    fmt out in group lora_cols M gtab      ->  0 / 1                                             (act_epi_ok of plan_gemm(.., 0))
//     fold   fmt out in group lora_cols post next   ->  parts norm                                        (fold_parts_ok, fold_norm_ok)
//
// tests/test_prefill_plan_cpu.py feeds it tests/golden/prompt_plans.json and the cases of tests/golden/prompt_launch_logs.json.
#include "../../metalchat_amd/csrc/prefill_plan.h"

#include <cstdio>
#include <cstdlib>
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
    MC_FIELD(pf2_on)
    MC_FIELD(pf2_wgs_per_cu)
    MC_FIELD(pf_attn8_on)
    MC_FIELD(pf_attn8_rows)
    MC_FIELD(pf_attn8_rows64)
    MC_FIELD(pf_attn8_rows256)
    MC_FIELD(pf_attn_heads)
    MC_FIELD(pf_attn8_pair)
    MC_FIELD(pf_rope_pack)
    MC_FIELD(pf_g8_on)
    MC_FIELD(pf_g8_max_splits)
    MC_FIELD(pf_g8_min_ktiles)
    MC_FIELD(pf_g8_rows)
    MC_FIELD(pf_small_gemm)
    MC_FIELD(pf_depth1)
    MC_FIELD(pf_bm128)
    MC_FIELD(pf_splits_old)
    MC_FIELD(pf_no_splitk)
    MC_FIELD(pf_fold_on)
    MC_FIELD(pf_norm2)
    MC_FIELD(pf_act_epi)
    MC_FIELD(pf_lib_force)
    MC_FIELD(pf_lib_rows)
    MC_FIELD(pf_lib_tiles)
#undef MC_FIELD
    return false;
}

int
main()
{
    static const char* const families[] = {"lib", "stream", "g8", "tiled", "tile64"};
    std::string line;
    while (std::getline(std::cin, line)) {
        if (line.empty()) continue;
        std::istringstream in(line);
        std::string kind;
        decoder_options opt;
        prefill_env e{};
        int lib_on = 0;
        if (!(in >> kind >> e.tb >> e.qmode >> e.family >> e.cus >> e.dim >> e.ffn_dim >> e.n_heads >> e.n_kv_heads >> e.head_dim >> e.max_seq_len >> lib_on)) {
            fprintf(stderr, "bad case: %s\n", line.c_str());
            return 2;
        }
        e.lib_on = lib_on != 0;
        e.opt = &opt;
        int a[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        const int nargs = kind == "gemm" ? 8 : kind == "act" || kind == "fold" ? 7 : kind == "rope" ? 4 : kind == "attn" || kind == "packed" || kind == "extend" ? 1 : -1;
        for (int i = 0; i < nargs; i++)
            if (!(in >> a[i])) {
                fprintf(stderr, "bad arguments: %s\n", line.c_str());
                return 2;
            }
        std::string kv;
        while (in >> kv) {
            const size_t eq = kv.find('=');
            if (eq == std::string::npos || !set_field(opt, kv.substr(0, eq), atoi(kv.c_str() + eq + 1))) {
                fprintf(stderr, "bad switch: %s\n", kv.c_str());
                return 2;
            }
        }
        const gemv_shape L{a[0], a[1], a[2], a[3], a[4]};
        if (kind == "gemm") {
            const gemm_plan P = plan_gemm(L, e, a[5], a[6]);
            const std::string name = P.fam == gemm_family::lib ? "hipblasLtMatmul" : P.kernel(P.writes_partials(), a[7] != 0);
            printf("%s %s %u %u %u %u %u %u\n", families[(int)P.fam], name.c_str(), P.gx, P.gy, P.splits, P.block, P.ktper, P.bm);
        } else if (kind == "attn" || kind == "packed") {
            const attn_plan A = kind == "attn" ? plan_attention(e, a[0]) : plan_packed_attention(e, a[0]);
            printf("%s %u %u %u\n", A.name.c_str(), A.gx, A.gy, A.block);
        } else if (kind == "extend") {
            const extend_plan E = plan_extend_attention(e, a[0] != 0);
            printf("%s %s %s %u\n", E.sums.c_str(), E.pv.c_str(), E.reduce.c_str(), E.heads);
        } else if (kind == "rope") {
            const rope_plan R = plan_rope(e, a[0], a[1] != 0, a[2], a[3] != 0);
            printf("%s %u %u %u\n", R.name.c_str(), R.gx, R.gy, R.block);
        } else if (kind == "act") {
            printf("%d\n", act_epi_ok(L, e, plan_gemm(L, e, a[5], 0), a[6] != 0) ? 1 : 0);
        } else if (kind == "fold") {
            printf("%d %d\n", fold_parts_ok(L, e) ? 1 : 0, fold_norm_ok(e, a[5] != 0, a[6] != 0) ? 1 : 0);
        } else {
            fprintf(stderr, "bad kind: %s\n", line.c_str());
            return 2;
        }
    }
    return 0;
}
