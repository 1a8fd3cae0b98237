// What the packed passes launch on an fp8 batch (csrc/prefill_plan.h with kv_format = MC_KV_FP8):
//   test_kv8_rows_plan HEAD_DIM N_HEADS N_KV_HEADS HEADS   (HEADS: MC_PF_ATTN_HEADS, 1 or 2)
// prints six kernel names: rope, rope over parts, packed attention, extend sums, extend pv, extend reduce.
#include "../../metalchat_amd/csrc/prefill_plan.h"

#include <cstdio>
#include <cstdlib>

int
main(int argc, char** argv)
{
    if (argc != 5) return 2;
    decoder_options opt;
    opt.pf_attn_heads = atoi(argv[4]);
    prefill_env e{2, 0, 0, 256, 0, 0, atoi(argv[2]), atoi(argv[3]), atoi(argv[1]), 256, false, &opt};
    const extend_plan x = plan_extend_attention(e, false, MC_KV_FP8);
    printf("%s\n%s\n%s\n%s\n%s\n%s\n", plan_rope(e, 40, false, 1, false, MC_KV_FP8).name.c_str(), plan_rope(e, 40, true, 1, false, MC_KV_FP8).name.c_str(),
           plan_packed_attention(e, 3, MC_KV_FP8).name.c_str(), x.sums.c_str(), x.pv.c_str(), x.reduce.c_str());
}
