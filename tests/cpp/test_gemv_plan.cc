// plan_gemv() (metalchat_amd/csrc/gemv_plan.h) from the command line, without HIP: one case per line of standard input,
//
//     fmt out in group lora_cols pro epi tb qmode cus [FIELD=value ...]
//
// where FIELD is a member of decoder_options (the switches a case sets; everything else at its default), answered by one line
//
//     name wgs block lds family            or            error: <text>
//
// tests/test_gemv_plan_cpu.py feeds it tests/golden/decode_gemv_plans.json.
#include "../../metalchat_amd/csrc/gemv_plan.h"

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
    MC_FIELD(gemv_block)
    MC_FIELD(gemv_wgs_per_cu)
    MC_FIELD(gemv_block_env)
    MC_FIELD(gemv_lin)
    MC_FIELD(gemv_ling)
    MC_FIELD(i8_ling14)
    MC_FIELD(lin_split)
    MC_FIELD(ling_half)
    MC_FIELD(lin_k4_on)
    MC_FIELD(lin_waves)
    MC_FIELD(gemv_full_grid)
    MC_FIELD(dbg_variant)
    MC_FIELD(gemv_m4)
#undef MC_FIELD
    return false;
}

int
main()
{
    static const char* const families[] = {"classic", "fast", "m4", "m4d", "lin", "lin_k4", "lin_split", "ling"};
    std::string line;
    while (std::getline(std::cin, line)) {
        if (line.empty()) continue;
        std::istringstream in(line);
        gemv_shape L{};
        decoder_options opt;
        gemv_env e{};
        int pro = 0, epi = 0;
        if (!(in >> L.fmt >> L.out >> L.in >> L.group >> L.lora_cols >> pro >> epi >> e.tb >> e.qmode >> e.cus)) {
            fprintf(stderr, "bad case: %s\n", line.c_str());
            return 2;
        }
        e.pick_slots = 1024; // mc_decoder::pick_slots
        e.opt = &opt;
        std::string kv;
        while (in >> kv) {
            const size_t eq = kv.find('=');
            if (eq == std::string::npos || !set_field(opt, kv.substr(0, eq), atoi(kv.c_str() + eq + 1))) {
                fprintf(stderr, "bad switch: %s\n", kv.c_str());
                return 2;
            }
        }
        const gemv_plan P = plan_gemv(L, e, pro, epi);
        if (P.error) printf("error: %s\n", P.error);
        else printf("%s %u %u %u %s\n", P.name.c_str(), P.wgs, P.block, P.lds, families[(int)P.family]);
    }
    return 0;
}
