"""rows_tables.py (the Python restatement of batch.cc rows_tables / rows_ranges / px_range_keys that test_rows_kernels_gpu.py builds its
tables with) against examples worked by hand from the C++ rule, and the properties the kernels rely on.  Nothing here can bind the
restatement to the C++ code without a device: test_rows_extend_gpu.test_a_call_in_several_launch_groups does that."""
import os
import re
import subprocess

import numpy as np

import rows_tables as rt
from metalchat_amd import build as b

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
READELF = ["/opt/rocm/lib/llvm/bin/llvm-readelf", "/usr/bin/readelf"]
LONG_LENS = [5, 40, 16, 130, 2, 33]          # test_rows_extend_gpu.LONG_LENS / LONG_POS, max_seq_len 1024
LONG_POS = [1000, 700, 63, 513, 1022, 255]


def test_segments_and_tiles_by_hand():
    segs = rt.segments([0, 5, 0, 0, 33, 0, 16, 0], [9, 7, 0, 0, 64, 0, 3, 0])
    assert segs == [(1, 7, 0, 5), (4, 64, 5, 33), (6, 3, 38, 16)]          # rows with length 0 are not in the call
    assert rt.tiles(segs) == [(0, 0), (1, 0), (1, 16), (1, 32), (2, 0)]
    assert rt.words(segs, 4).dtype == np.int32 and rt.words(segs, 4).shape == (3, 4)


def test_the_long_contexts_of_the_extend_test_by_hand():
    """px_range_keys(S, len) = len <= 32 && S > 512 ? ((S + 1) / 2 + 127) / 128 * 128 : S.
    row 0: len 5 at 1000, S = 1005: (503 + 127) / 128 * 128 = 512 -> [0, 512), [512, 1005)
    row 4: len 2 at 1022, S = 1024: (512 + 127) / 128 * 128 = 512 -> [0, 512), [512, 1024)
    rows 1, 3, 5: longer than 32; row 2: S = 79 <= 512 -- one range per tile"""
    segs = rt.segments(LONG_LENS, LONG_POS)
    tls = rt.tiles(segs)
    assert len(tls) == 1 + 3 + 1 + 9 + 1 + 3
    tab = rt.ranges(segs, tls)
    per_seg = [[e for e in tab if e[0] == si] for si in range(6)]
    assert per_seg[0] == [(0, 0, 0, 512, 0, 2, 0, 0), (0, 0, 512, 1005, 0, 2, 0, 0)]
    assert per_seg[1] == [(1, 0, 0, 716, 2, 1, 0, 0), (1, 16, 0, 732, 3, 1, 0, 0), (1, 32, 0, 740, 4, 1, 0, 0)]
    assert per_seg[2] == [(2, 0, 0, 79, 5, 1, 0, 0)]
    assert [(e[1], e[3], e[5]) for e in per_seg[3]] == [(16 * t, 513 + min(16 * t + 16, 130), 1) for t in range(9)]
    assert per_seg[4] == [(4, 0, 0, 512, 15, 2, 0, 0), (4, 0, 512, 1024, 15, 2, 0, 0)]
    assert [(e[1], e[3], e[5]) for e in per_seg[5]] == [(0, 271, 1), (16, 287, 1), (32, 288, 1)]
    assert len(tab) == 20
    assert rt.groups(tab, 1024) == [(0, 20, True)]
    # MC_PX_KEYS=128: ceil(S / 128) ranges of every tile -- row 0: 8, row 2: 1, row 4: 8
    t128 = rt.ranges(segs, tls, rt.keys_of(128))
    assert [len([e for e in t128 if e[0] == si]) for si in range(6)] == [8, 6 + 6 + 6, 1, sum(-(-(513 + min(16 * t + 16, 130)) // 128) for t in range(9)), 8, 3 + 3 + 3]
    assert rt.keys_of(100)(700, 40) == 128 and rt.keys_of(129)(700, 40) == 256 and rt.keys_of(0)(700, 40) == 700


def test_the_default_rule_at_its_edges():
    assert rt.default_keys(512, 2) == 512 and rt.default_keys(513, 2) == 384        # (257 + 127) / 128 * 128
    assert rt.default_keys(513, 32) == 384 and rt.default_keys(513, 33) == 513
    assert rt.default_keys(2048, 2) == 1024 and rt.default_keys(1025, 17) == 640    # (513 + 127) / 128 * 128
    # the most ranges of a tile (px_ranges_max): two by the default rule
    for S in range(513, 2049):
        k = rt.default_keys(S, 2)
        assert k % 128 == 0 and -(-S // k) == 2, S


def properties(segs, tls, tab):
    i = 0
    for si, r0 in tls:
        _, pos, _, n = segs[si]
        S = pos + min(r0 + 16, n)
        first, cnt = tab[i][4], tab[i][5]
        assert first == i and cnt >= 1
        mine = tab[i:i + cnt]
        assert all(e[:2] == (si, r0) and e[4:] == (first, cnt, 0, 0) for e in mine)
        assert all(e[2] % 128 == 0 and e[2] < e[3] for e in mine)
        assert mine[0][2] == 0 and mine[-1][3] == S                         # [0, S) ...
        assert all(a[3] == b_[2] for a, b_ in zip(mine, mine[1:]))           # ... adjacent, ascending: covered exactly once
        i += cnt
    assert i == len(tab)


def test_ranges_cover_a_tile_exactly_once_and_groups_hold_whole_tiles():
    rng = np.random.default_rng(0)
    for trial in range(200):
        max_seq = int(rng.choice([256, 1000, 1024, 2048]))
        lens = [int(rng.choice([0, 2, 15, 16, 17, 31, 32, 33, 64, 65, 130])) for _ in range(8)]
        pos = [int(rng.integers(0, max_seq - n + 1)) if n else 0 for n in lens]
        if not any(lens):
            continue
        segs = rt.segments(lens, pos)
        tls = rt.tiles(segs)
        assert [g[2] for g in segs] == list(np.cumsum([0] + [g[3] for g in segs[:-1]]))
        for rule in (rt.default_keys, rt.keys_of(128), rt.keys_of(384), rt.keys_of(0)):
            tab = rt.ranges(segs, tls, rule)
            properties(segs, tls, tab)
            most = max(e[5] for e in tab)
            for slots in (most, most + 1, 2 * most + 3, 1 << 20):
                gs = rt.groups(tab, slots)
                assert gs[0][0] == 0 and sum(g[1] for g in gs) == len(tab)
                for (f0, c0, sp0), nxt in zip(gs, gs[1:] + [(len(tab), 0, False)]):
                    assert f0 + c0 == nxt[0] and 0 < c0 <= slots
                    assert tab[f0][4] == f0 and (nxt[0] == len(tab) or tab[nxt[0]][4] == nxt[0])   # whole tiles
                    assert sp0 == any(e[5] > 1 for e in tab[f0:f0 + c0])
                    if nxt[0] < len(tab):
                        assert c0 + tab[nxt[0]][5] > slots                                             # greedy: the next tile did not fit


def test_the_case_of_several_launch_groups_by_hand():
    """test_rows_extend_gpu.test_a_call_in_several_launch_groups: eight rows of 200 tokens at 1800, max_seq_len 2048, MC_PX_KEYS=128,
    1024 slots (64 MiB / (8 heads * 16 rows * 128 * 4 bytes)).  Tile t of a row: S = 1800 + min(16 t + 16, 200), ceil(S / 128) =
    15 for t <= 6 (S <= 1912), 16 for t >= 7 (S >= 1928): 7 * 15 + 6 * 16 = 201 ranges per row, 1608 in the call -> two groups"""
    segs = rt.segments([200] * 8, [1800] * 8)
    tab = rt.ranges(segs, rt.tiles(segs), rt.keys_of(128))
    assert len(tab) == 8 * 201
    gs = rt.groups(tab, 1024)
    assert len(gs) == 2 and gs[0][0] == 0 and gs[0][1] <= 1024 and gs[0][1] + gs[1][1] == 1608
    one = rt.segments([200], [1800])
    assert len(rt.groups(rt.ranges(one, rt.tiles(one), rt.keys_of(128)), 1024)) == 1


ROWS_KERNELS = [f"mc_px_{a}_bfloat_hd{hd}" for a in ("sums", "sums2", "pv", "pv2", "reduce") for hd in (64, 128)] + \
               [f"mc_pp_attn{a}_bfloat_hd{hd}" for a in ("", "2") for hd in (64, 128)] + \
               ["mc_pp_rope_cache_bfloat", "mc_pp_rope_cache_parts_bfloat", "mc_pp_gather_last_bfloat"]


def test_every_packed_and_extend_kernel_is_launched_by_name_in_the_kernel_tests():
    """the code object's mc_pp_* / mc_px_* names are exactly these seventeen, and test_rows_kernels_gpu.py names each of them"""
    hsaco, _ = b.build_all()
    tool = next((t for t in READELF if os.path.exists(t)), None)
    assert tool is not None, "no readelf available"
    out = subprocess.check_output([tool, "--symbols", "--wide", hsaco], text=True)
    symbols = {line.split()[-1] for line in out.splitlines() if " FUNC " in line}
    assert sorted(s for s in symbols if s.startswith(("mc_pp_", "mc_px_"))) == sorted(ROWS_KERNELS)
    text = open(os.path.join(ROOT, "tests", "test_rows_kernels_gpu.py")).read()
    named = set(re.findall(r'"(mc_p[px]_\w+)"', text))
    assert named == set(ROWS_KERNELS), sorted(set(ROWS_KERNELS) ^ named)
    assert "acc.load(" in text
