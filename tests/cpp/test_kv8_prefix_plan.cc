// The two attention launches of a ragged step by cache format (csrc/batch_plan.h plan_prefix_attention, Part 2s):
//   test_kv8_prefix_plan N_HEADS N_KV_HEADS HEAD_DIM MAX_SEQ B ATTACHED KV_FORMAT MC_SP8_GROUPS
// prints "name gx gy gz block" for the scores and the P.V launch, then the groups per P.V workgroup.  MC_SP8_GROUPS as the environment gives it
// ("-": unset); KV_FORMAT "-": the call as the callers from before Part 2s make it.
#include "../../metalchat_amd/csrc/batch_plan.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>

int
main(int argc, char** argv)
{
    if (argc != 9) return 2;
    mc_decoder_config c{};
    c.n_heads = atoi(argv[1]);
    c.n_kv_heads = atoi(argv[2]);
    c.head_dim = atoi(argv[3]);
    c.max_seq_len = atoi(argv[4]);
    const int B = atoi(argv[5]), nsplit = (c.max_seq_len + (int)mc::abi::PB - 1) / (int)mc::abi::PB;
    const bool attached = atoi(argv[6]) != 0;
    const int env = mcimpl::sp8_groups_env_of(strcmp(argv[8], "-") ? argv[8] : nullptr);
    const mcimpl::prefix_attention_plan a = strcmp(argv[7], "-") ? mcimpl::plan_prefix_attention(c, B, nsplit, attached, atoi(argv[7]), env)
                                                                 : mcimpl::plan_prefix_attention(c, B, nsplit, attached);
    for (const mcimpl::launch_plan* l : {&a.scores, &a.pv}) printf("%s %u %u %u %u\n", l->name.c_str(), l->gx, l->gy, l->gz, l->block);
    printf("%d\n", a.gw);
}
