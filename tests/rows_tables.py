"""The tables of the packed prompt pass and of mc_extend_rows, restated in Python for the kernel-level tests
(test_rows_kernels_gpu.py): the segment, tile and key-range tables of kernels/abi.h (pp_seg, pp_tile, px_range) and the launch groups,
built by the rules of metalchat_amd/csrc/rows_plan.h (rows_tables, rows_ranges, px_range_keys).

This is a RESTATEMENT, bound to the C++ rules on the CPU: they live in a header without HIP (csrc/rows_plan.h), and test_rows_tables_cpu.py
holds every function here to tests/cpp/test_rows_plan, a plain g++ program over that header, on the examples worked by hand and on 300
random calls.  test_rows_extend_gpu.test_a_call_in_several_launch_groups binds the host's own tables and groups on the device."""
import numpy as np

TILE_ROWS = 16   # abi.h PP_TILE_ROWS


def segments(lens, positions):
    """rows_tables: one (row, pos, off, len) per batch row with lens[row] > 0, packed in row order"""
    segs, off = [], 0
    for r, (n, p) in enumerate(zip(lens, positions)):
        if n == 0:
            continue
        segs.append((r, int(p), off, int(n)))
        off += int(n)
    return segs


def tiles(segs):
    """rows_tables: the 16-row tiles (segment index, first row inside it) of every segment, in segment order"""
    return [(si, t) for si, g in enumerate(segs) for t in range(0, g[3], TILE_ROWS)]


def default_keys(S, n):
    """px_range_keys without MC_PX_KEYS: a segment of at most 32 rows behind more than 512 keys takes two ranges"""
    return ((S + 1) // 2 + 127) // 128 * 128 if n <= 32 and S > 512 else S


def keys_of(k):
    """px_range_keys under MC_PX_KEYS=k: ranges of k keys (rounded up to 128) for every tile, k <= 0: never split"""
    return lambda S, n: S if k <= 0 else (k + 127) // 128 * 128


def ranges(segs, tls, keys_rule=default_keys):
    """rows_ranges: (seg, r0, k_lo, k_hi, first, n, 0, 0) per (tile, key range): the keys [0, pos + min(r0 + 16, len)) of a tile in
    ranges of keys_rule(S, len) keys"""
    tab = []
    for si, r0 in tls:
        _, pos, _, n = segs[si]
        S = pos + min(r0 + TILE_ROWS, n)
        keys = keys_rule(S, n)
        cnt = (S + keys - 1) // keys
        first = len(tab)
        for k in range(cnt):
            tab.append((si, r0, k * keys, min((k + 1) * keys, S), first, cnt, 0, 0))
    return tab


def groups(tab, slots):
    """rows_ranges: the launch groups (first range, ranges, holds a split tile) -- whole tiles, at most `slots` ranges each"""
    out, i = [], 0
    while i < len(tab):
        n = tab[i][5]
        assert tab[i][4] == i and n <= slots, (i, n, slots)
        if not out or out[-1][1] + n > slots:
            out.append([i, 0, False])
        out[-1][1] += n
        out[-1][2] = out[-1][2] or n > 1
        i += n
    return [tuple(g) for g in out]


def words(table, width):
    """a table as the int32 array the kernels read"""
    return np.asarray(table, np.int32).reshape(len(table), width)
