// The host side of the rows passes (mc_rows_prefill, mc_extend_rows, mc_verify_rows, mc_tree_verify; batch_rows.cc rows_pass) without a device: the
// admission of a call (rows_check, tree_check), the tables its kernels index memory by -- pp_seg / pp_tile / tv_node (rows_tables, tree_nodes),
// px_range and the launch groups (rows_ranges) -- and the scratch sizes derived from them (rows_scratch_of).  Plain C++ over kernels/abi.h, no
// HIP, so tests/cpp/test_rows_plan.cc prints exactly what a call uploads and tests/rows_tables.py / tree_rule.py, which the kernel-level tests
// build their tables with, are held to it on the CPU.  batch_rows.cc keeps fail(), the reserves, the copies and the launches.
#pragma once

#include <algorithm>
#include <cstdint>
#include <string>
#include <vector>

#include "kernels/abi.h"

namespace mcimpl {

using namespace mc::abi;

// a launch group of mc_extend_rows: whole tiles, at most as many ranges as the scratch has slots
struct px_group {
    int first = 0, count = 0; // its ranges: [first, first + count) of the range table
    bool split = false;       // a tile of the group has several ranges (their partial outputs want mc_px_reduce)
};

// the tables inside one upload (mc_batch::pp_tab / pp_host.data()): MC_WIDE_BATCH_MAX segments, the call's tiles, a tree call's nodes
inline pp_seg* pp_segs(char* tab) { return reinterpret_cast<pp_seg*>(tab); }
inline pp_tile* pp_tiles(char* tab) { return reinterpret_cast<pp_tile*>(tab + sizeof(pp_seg) * MC_WIDE_BATCH_MAX); }
inline tv_node* tv_nodes(char* tab, int ntiles) { return reinterpret_cast<tv_node*>(pp_tiles(tab) + ntiles); }

// a row whose length exceeds max_seq_len has rolled: its evicted positions are gone, so it is continued at its length or
// restarted at 0 and nothing between ("" = fine, else the refusal behind the row's name)
inline std::string
rolled_rewind(int32_t length, int max_seq_len, int64_t pos)
{
    if (length <= max_seq_len || pos == 0 || pos >= length) return "";
    return "position " + std::to_string(pos) + " lies below the row's length " + std::to_string(length) + " and the row has rolled";
}

// How mc_extend_rows' attention deals the keys [0, S) of a 16-row tile over workgroups (kernels/extend_kernels.hip): the size of
// a key range, a multiple of 128; S or more = one range.  The rule looks at the tile's own segment only -- never at what else is
// in the call -- so that a row's bits depend on nothing but the row: a segment of at most two tiles (a short message) behind more
// than 512 keys brings too few workgroups for its keys and takes two ranges; every other tile has one (measured: DESIGN.md
// "Chunks that see their context").  keys_override is the experiment's handle (MC_PX_KEYS, read by rows_pass once per call): N = ranges of N
// keys for every tile, 0 = never split, PX_KEYS_RULE = not given.
constexpr int PX_KEYS_RULE = -1;
inline int
px_range_keys(int S, int len, int keys_override)
{
    if (keys_override != PX_KEYS_RULE) return keys_override <= 0 ? S : (keys_override + 127) / 128 * 128;
    return len <= 32 && S > 512 ? ((S + 1) / 2 + 127) / 128 * 128 : S;
}
// the most ranges a tile can have in a cache of max_seq slots
inline int
px_ranges_max(int max_seq, int keys_override)
{
    const int keys = px_range_keys(max_seq, 2, keys_override);
    return (max_seq + keys - 1) / keys;
}

// step 1 of rows_pass: the call's lengths, positions and tokens against the rows' caches (`lengths`: valid cache positions of each of the B
// rows); counts its packed rows, segments and tiles.  verify (mc_verify_rows, mc_tree_verify): a pick after every chunk row -- one attention tile
// per row, and no more rows than mc_v_head_* holds.  refusal "": admitted
struct rows_counts {
    std::string refusal;
    int M = 0, nseg = 0, ntiles = 0;
};
inline rows_counts
rows_check(const std::string& who, const int32_t* tokens, const int32_t* lens, const int32_t* positions, const int32_t* lengths, int B, int max_seq_len,
           int vocab, bool verify)
{
    rows_counts c;
    auto refuse = [&](const std::string& why) {
        c.refusal = why;
        return c;
    };
    int64_t total = 0;
    for (int r = 0; r < B; r++) {
        const std::string row = who + ": row " + std::to_string(r) + ": ";
        const int32_t len = lens[r], pos = positions[r];
        if (len < 0) return refuse(row + "length below 0 (0 = the row is not in the call)");
        if (len == 0) continue;
        if (len == 1) return refuse(row + "a one-token chunk is a step: mc_ragged_step");
        if (pos < 0) return refuse(row + "position below 0");
        if (pos > lengths[r])
            return refuse(row + "position " + std::to_string(pos) + " is past the row's length " + std::to_string(lengths[r]) +
                          " (its cache has no slots written beyond it)");
        if ((int64_t)pos + len > max_seq_len)
            return refuse(row + "position + length " + std::to_string((int64_t)pos + len) + " exceeds max_seq_len (a batch's cache does not roll)");
        if (const std::string why = rolled_rewind(lengths[r], max_seq_len, pos); !why.empty()) return refuse(row + why);
        for (int32_t i = 0; i < len; i++)
            if (tokens[total + i] < 0 || tokens[total + i] >= vocab) return refuse(row + "token id outside the vocabulary");
        total += len;
        c.nseg++;
        c.ntiles += (len + PP_TILE_ROWS - 1) / PP_TILE_ROWS;
    }
    if (c.nseg == 0) return refuse(who + ": no row in the call (every length is 0)");
    if (total > max_seq_len)
        return refuse(who + ": the rows' lengths add up to " + std::to_string(total) + ", more than max_seq_len (" + std::to_string(max_seq_len) +
                      "): split the call by rows");
    c.M = (int)total;
    if (verify)
        for (int r = 0; r < B; r++)
            if (lens[r] > MC_VERIFY_MAX_LEN)
                return refuse(who + ": row " + std::to_string(r) + ": a chunk of " + std::to_string(lens[r]) + " tokens is longer than MC_VERIFY_MAX_LEN (" +
                              std::to_string(MC_VERIFY_MAX_LEN) + ")");
    // (eight rows of at most 16 tokens never get here; a wide batch can: mc_v_head_* holds MC_VERIFY_MAX_ROWS rows)
    if (verify && c.M > MC_VERIFY_MAX_ROWS)
        return refuse(who + ": the chunks add up to " + std::to_string(c.M) + " rows, more than MC_VERIFY_MAX_ROWS (" + std::to_string(MC_VERIFY_MAX_ROWS) +
                      "): split the call by rows");
    return c;
}

// step 2: the rows' states, the segment table (packed in row order) and the ntiles attention tiles of the segments
inline void
rows_tables(const int32_t* lens, const int32_t* positions, int B, int ntiles, std::vector<step_state>& rows, std::vector<char>& tab)
{
    rows.assign(B, step_state{});
    tab.assign(sizeof(pp_seg) * MC_WIDE_BATCH_MAX + sizeof(pp_tile) * ntiles, 0);
    pp_seg* seg = pp_segs(tab.data());
    pp_tile* tile = pp_tiles(tab.data());
    for (int r = 0, off = 0, si = 0; r < B; r++) {
        rows[r].pos = lens[r] > 0 ? positions[r] : -1;
        rows[r].token = -1;
        rows[r].step_index = r; // seed pair r % n_pairs, next_tokens[r]
        if (lens[r] == 0) continue;
        for (int t = 0; t < lens[r]; t += PP_TILE_ROWS) *tile++ = {si, t};
        seg[si++] = {r, positions[r], off, lens[r]};
        off += lens[r];
    }
}

// step 3 (mc_extend_rows): the range table -- the keys [0, pos + last row of the tile] of every tile in ranges of px_range_keys --
// and the launch groups: whole tiles, at most `slots` ranges each
inline void
rows_ranges(const std::vector<char>& tab, int ntiles, int slots, int keys_override, std::vector<px_range>& ranges, std::vector<px_group>& groups)
{
    ranges.clear();
    groups.clear();
    char* base = const_cast<char*>(tab.data()); // (read only)
    for (int ti = 0; ti < ntiles; ti++) {
        const pp_tile t = pp_tiles(base)[ti];
        const pp_seg g = pp_segs(base)[t.seg];
        const int S = g.pos + std::min(t.r0 + PP_TILE_ROWS, g.len), keys = px_range_keys(S, g.len, keys_override), n = (S + keys - 1) / keys;
        const int first = (int)ranges.size();
        if (groups.empty() || groups.back().count + n > slots) groups.push_back({first, 0, false});
        groups.back().count += n;
        if (n > 1) groups.back().split = true;
        for (int k = 0; k < n; k++) ranges.push_back({t.seg, t.r0, k * keys, std::min((k + 1) * keys, S), first, n, 0, 0});
    }
}

// mc_tree_verify: every row's `parents` (root -1, then 0 <= parent < i; "" = fine), and the node table behind the tiles of `tab`
inline std::string
tree_check(const std::string& who, const int32_t* parents, const int32_t* lens, int B)
{
    for (int r = 0, off = 0; r < B; off += lens[r], r++) {
        const std::string row = who + ": row " + std::to_string(r) + ": ";
        if (lens[r] == 0) continue;
        if (parents[off] != -1) return row + "the parent of node 0 (the root) must be -1, not " + std::to_string(parents[off]);
        for (int32_t i = 1; i < lens[r]; i++)
            if (parents[off + i] < 0 || parents[off + i] >= i)
                return row + "the parent of node " + std::to_string(i) + " is " + std::to_string(parents[off + i]) + ", outside [0, " + std::to_string(i) +
                       ") (nodes come in topological order)";
    }
    return "";
}
inline void
tree_nodes(const int32_t* parents, const int32_t* lens, int B, int ntiles, int M, std::vector<char>& tab)
{
    tab.resize(tab.size() + sizeof(tv_node) * M);
    tv_node* node = tv_nodes(tab.data(), ntiles);
    for (int r = 0, off = 0; r < B; off += lens[r], r++)
        for (int32_t i = 0; i < lens[r]; i++) {
            const int32_t par = parents[off + i];
            node[off + i] = i == 0 ? tv_node{0, 1u} : tv_node{node[off + par].depth + 1, node[off + par].anc | (1u << i)};
        }
}

// What rows_pass reserves, sized once for any call of the batch: at most max_seq_len rows in at most MC_WIDE_BATCH_MAX segments, one per row of the
// batch (tiles_max); for mc_extend_rows the scratch of one launch group -- 64 MiB of partial outputs, and never less than one tile's ranges (slots)
// -- and a range table for every tile of the largest call with the most ranges a tile can have (tiles_max * per_tile)
struct rows_scratch {
    int tiles_max, per_tile, slots;
    size_t per_slot; // bytes of one range's partial outputs
    size_t tab_bytes() const { return sizeof(pp_seg) * MC_WIDE_BATCH_MAX + sizeof(pp_tile) * tiles_max + sizeof(tv_node) * MC_VERIFY_MAX_ROWS; }
};
inline rows_scratch
rows_scratch_of(int max_seq_len, int n_heads, int head_dim, int keys_override)
{
    rows_scratch s;
    s.tiles_max = max_seq_len / PP_TILE_ROWS + MC_WIDE_BATCH_MAX;
    s.per_tile = px_ranges_max(max_seq_len, keys_override);
    s.per_slot = (size_t)n_heads * PP_TILE_ROWS * head_dim * sizeof(float);
    s.slots = (int)std::min<size_t>(32768, std::max<size_t>((size_t)s.per_tile, ((size_t)64 << 20) / s.per_slot));
    return s;
}

} // namespace mcimpl
