// The two attention launches of a ragged step (csrc/batch_plan.h plan_prefix_attention):
//   test_prefix_plan N_HEADS N_KV_HEADS HEAD_DIM MAX_SEQ B ATTACHED
// prints "name gx gy gz block" for the scores and the P.V launch, then the group size and the shared slots of a prefix of MAX_SEQ - 1 positions.
#include "../../metalchat_amd/csrc/batch_plan.h"

#include <cstdio>
#include <cstdlib>

int
main(int argc, char** argv)
{
    if (argc != 7) return 2;
    mc_decoder_config c{};
    c.n_heads = atoi(argv[1]);
    c.n_kv_heads = atoi(argv[2]);
    c.head_dim = atoi(argv[3]);
    c.max_seq_len = atoi(argv[4]);
    const int nsplit = (c.max_seq_len + (int)mc::abi::PB - 1) / (int)mc::abi::PB;
    const mcimpl::prefix_attention_plan a = mcimpl::plan_prefix_attention(c, atoi(argv[5]), nsplit, atoi(argv[6]) != 0);
    for (const mcimpl::launch_plan* l : {&a.scores, &a.pv}) printf("%s %u %u %u %u\n", l->name.c_str(), l->gx, l->gy, l->gz, l->block);
    printf("%d %d\n", mcimpl::prefix_group(c), mcimpl::prefix_shared(c.max_seq_len - 1));
}
