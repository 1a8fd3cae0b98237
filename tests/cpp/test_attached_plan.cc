// A chunk or verify call that names rows attached to the shared prefix (csrc/rows_plan.h rows_ranges, plan_attached_attention; Part 2t):
//   test_attached_plan N_HEADS N_KV_HEADS HEAD_DIM KEYS ATTACHED_MASK LEN POS [LEN POS ..]
// KEYS: MC_PX_KEYS, -1 = the rule; bit r of ATTACHED_MASK: batch row r is attached; one (LEN, POS) per batch row.  Prints
//   T <tiles per unit>
//   range <seg> <r0> <k_lo> <k_hi> <first> <n>              per range of the table, in table order
//   unit <n> <range> ..                                     per entry of the unit table
//   launch <name> <gx> <gy>                                 per launch of one layer's attention, in order
#include "../../metalchat_amd/csrc/rows_plan.h"

#include <cstdio>
#include <cstdlib>

using namespace mcimpl;

int
main(int argc, char** argv)
{
    if (argc < 8 || (argc - 6) % 2) return 2;
    const int H = atoi(argv[1]), KV = atoi(argv[2]), hd = atoi(argv[3]), keys = atoi(argv[4]), mask = atoi(argv[5]), B = (argc - 6) / 2;
    std::vector<int32_t> lens(B), pos(B);
    std::vector<char> attached(B);
    int ntiles = 0;
    bool any = false;
    for (int r = 0; r < B; r++) {
        lens[r] = atoi(argv[6 + 2 * r]), pos[r] = atoi(argv[7 + 2 * r]);
        attached[r] = (mask >> r) & 1;
        any = any || (attached[r] && lens[r] > 0);
        ntiles += (lens[r] + PP_TILE_ROWS - 1) / PP_TILE_ROWS;
    }
    std::vector<step_state> rows;
    std::vector<char> tab;
    rows_tables(lens.data(), pos.data(), B, ntiles, rows, tab);
    const int T = ax_unit_tiles(hd, H / KV);
    std::vector<px_range> ranges;
    std::vector<px_group> groups;
    std::vector<ax_unit> units;
    if (any) rows_ranges(tab, ntiles, 4096, keys, ranges, groups, attached.data(), T, &units);
    else rows_ranges(tab, ntiles, 4096, keys, ranges, groups);
    printf("T %d\n", T);
    for (const px_range& e : ranges) printf("range %d %d %d %d %d %d\n", e.seg, e.r0, e.k_lo, e.k_hi, e.first, e.n);
    for (const ax_unit& u : units) {
        printf("unit %d", u.n);
        for (int i = 0; i < u.n; i++) printf(" %d", u.range[i]);
        printf("\n");
    }
    const ax_plan A = plan_attached_attention(H, KV, hd);
    const std::string sfx = std::string((H / KV) % 2 == 0 ? "2" : "") + "_bfloat_hd" + std::to_string(hd); // (prefill_plan.h plan_extend_attention, grouping allowed)
    for (const px_group& g : groups) {
        if (g.attached) {
            printf("launch %s %u %d\nlaunch %s %u %d\n", A.sums.c_str(), A.heads, g.ucount, A.pv.c_str(), A.heads, g.ucount);
        } else {
            const int gx = (H / KV) % 2 == 0 ? H / 2 : H;
            printf("launch mc_px_sums%s %d %d\nlaunch mc_px_pv%s %d %d\n", sfx.c_str(), gx, g.count, sfx.c_str(), gx, g.count);
        }
        if (g.split) printf("launch %s %d %d\n", A.reduce.c_str(), H, g.count);
    }
}
