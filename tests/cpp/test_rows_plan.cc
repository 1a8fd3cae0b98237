// The host side of the rows passes (metalchat_amd/csrc/rows_plan.h) from the command line, without HIP: one call per line of standard input,
//
//     who B max_seq_len vocab keys slots verify tree n_heads head_dim  lens[B]  positions[B]  lengths[B]  tokens[T]  parents[T if tree]
//
// T = the sum of the positive lens; keys: MC_PX_KEYS as rows_pass hands it down (-1 = not given); slots: the ranges one launch group may hold
// (0 = what rows_scratch_of sizes for n_heads and head_dim); lengths: the rows' valid cache positions.  Answered by one line of JSON: the refusal
//
//     {"refused": "<text>"}
//
// or what the call uploads: {"M", "nseg", "ntiles", "pos" (the rows' step states), "segs", "tiles", "ranges", "groups", "nodes", "scratch"}.
// tests/test_rows_tables_cpu.py and tests/test_tree_verify_cpu.py hold tests/rows_tables.py and tests/tree_rule.py to it.
#include "../../metalchat_amd/csrc/rows_plan.h"

#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <sstream>

using namespace mcimpl;

static bool
read_ints(std::istringstream& in, std::vector<int32_t>& v, size_t n)
{
    v.resize(n);
    for (size_t i = 0; i < n; i++)
        if (!(in >> v[i])) return false;
    return true;
}

int
main()
{
    std::string line;
    while (std::getline(std::cin, line)) {
        if (line.empty()) continue;
        std::istringstream in(line);
        std::string who;
        int B = 0, S = 0, vocab = 0, keys = PX_KEYS_RULE, slots = 0, verify = 0, tree = 0, H = 0, hd = 0;
        std::vector<int32_t> lens, pos, lengths, tokens, parents;
        bool ok = (bool)(in >> who >> B >> S >> vocab >> keys >> slots >> verify >> tree >> H >> hd) && B >= 1 && B <= MC_WIDE_BATCH_MAX &&
                  read_ints(in, lens, B) && read_ints(in, pos, B) && read_ints(in, lengths, B);
        size_t T = 0;
        for (int32_t n : lens) T += n > 0 ? (size_t)n : 0;
        ok = ok && read_ints(in, tokens, T) && (!tree || read_ints(in, parents, T));
        if (!ok) {
            fprintf(stderr, "bad call: %s\n", line.c_str());
            return 2;
        }
        const rows_counts n = rows_check(who, tokens.data(), lens.data(), pos.data(), lengths.data(), B, S, vocab, verify != 0);
        std::string why = n.refusal;
        if (why.empty() && tree) why = tree_check(who, parents.data(), lens.data(), B);
        if (!why.empty()) {
            printf("{\"refused\": \"%s\"}\n", why.c_str());
            continue;
        }
        const rows_scratch sc = rows_scratch_of(S, H, hd, keys);
        std::vector<step_state> rows;
        std::vector<char> tab;
        std::vector<px_range> ranges;
        std::vector<px_group> groups;
        rows_tables(lens.data(), pos.data(), B, n.ntiles, rows, tab);
        if (tree) tree_nodes(parents.data(), lens.data(), B, n.ntiles, n.M, tab);
        rows_ranges(tab, n.ntiles, slots ? slots : sc.slots, keys, ranges, groups);
        printf("{\"M\": %d, \"nseg\": %d, \"ntiles\": %d, \"pos\": [", n.M, n.nseg, n.ntiles);
        for (int r = 0; r < B; r++) printf("%s%d", r ? ", " : "", rows[r].pos);
        printf("], \"segs\": [");
        for (int i = 0; i < n.nseg; i++) {
            const pp_seg g = pp_segs(tab.data())[i];
            printf("%s[%d, %d, %d, %d]", i ? ", " : "", g.row, g.pos, g.off, g.len);
        }
        printf("], \"tiles\": [");
        for (int i = 0; i < n.ntiles; i++) printf("%s[%d, %d]", i ? ", " : "", pp_tiles(tab.data())[i].seg, pp_tiles(tab.data())[i].r0);
        printf("], \"ranges\": [");
        for (size_t i = 0; i < ranges.size(); i++) {
            const px_range& x = ranges[i];
            printf("%s[%d, %d, %d, %d, %d, %d, %d, %d]", i ? ", " : "", x.seg, x.r0, x.k_lo, x.k_hi, x.first, x.n, x.pad0, x.pad1);
        }
        printf("], \"groups\": [");
        for (size_t i = 0; i < groups.size(); i++) printf("%s[%d, %d, %s]", i ? ", " : "", groups[i].first, groups[i].count, groups[i].split ? "true" : "false");
        printf("], \"nodes\": [");
        for (int i = 0; tree && i < n.M; i++) {
            const tv_node v = tv_nodes(tab.data(), n.ntiles)[i];
            printf("%s[%d, %u]", i ? ", " : "", v.depth, v.anc);
        }
        printf("], \"scratch\": {\"tiles_max\": %d, \"per_tile\": %d, \"slots\": %d, \"per_slot\": %zu, \"tab_bytes\": %zu}}\n", sc.tiles_max, sc.per_tile,
               sc.slots, sc.per_slot, sc.tab_bytes());
    }
    return 0;
}
