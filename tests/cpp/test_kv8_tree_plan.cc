// What mc_tree_verify launches on an fp8 batch (csrc/prefill_plan.h and csrc/batch_plan.h with kv_format = MC_KV_FP8):
//   test_kv8_tree_plan HEAD_DIM N_HEADS N_KV_HEADS HEADS   (HEADS: MC_PF_ATTN_HEADS, 1 or 2)
// prints six kernel names -- rope, rope over parts, tree sums, tree pv, reduce, compact --, the compact launch's grid x for 3 segments and 2
// layers, and the refusal of a tree on an fp8 batch with the tree switch off and on (the packed switch on both times; "-" = admitted).
#include "../../metalchat_amd/csrc/batch_plan.h"
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
    const extend_plan x = plan_extend_attention(e, true, MC_KV_FP8);
    mc_decoder_config c{};
    c.n_kv_heads = e.n_kv_heads;
    c.head_dim = e.head_dim;
    c.vocab = 2048;
    mcimpl::linear_shape head{};
    head.out = c.vocab;
    const mcimpl::verify_plan v = mcimpl::plan_verify_head(head, c, 2, 21, 3, true, MC_KV_FP8);
    printf("%s\n%s\n%s\n%s\n%s\n%s\n%u\n", plan_rope(e, 21, false, 2, false, MC_KV_FP8).name.c_str(), plan_rope(e, 21, true, 2, false, MC_KV_FP8).name.c_str(),
           x.sums.c_str(), x.pv.c_str(), x.reduce.c_str(), v.compact.name.c_str(), v.compact.gx);
    for (int on = 0; on < 2; on++) {
        const std::string r = mcimpl::kv_packed_refusal("mc_tree_verify", MC_KV_FP8, true, true, on == 1);
        printf("%s\n", r.empty() ? "-" : r.c_str());
    }
}
