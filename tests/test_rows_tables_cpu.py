"""rows_tables.py (the Python restatement of the C++ rules rows_tables / rows_ranges / px_range_keys that test_rows_kernels_gpu.py builds its
tables with) against examples worked by hand from the C++ rule, the properties the kernels rely on -- and against the C++ rules themselves:
they live in csrc/rows_plan.h, a header without HIP that batch_rows.cc builds every call's tables with, and tests/cpp/test_rows_plan (a plain g++
program over it, rows_plan_program.py) must print the restatement's segments, tiles, ranges and groups for every by-hand example here, the calls
of test_rows_extend_gpu.py and 300 random calls.  A host rule that changes fails here, before a kernel test goes on testing the old one.
test_rows_extend_gpu.test_a_call_in_several_launch_groups still binds the uploaded tables on the device."""
import os
import re
import subprocess

import numpy as np

import rows_plan_program as rp
import rows_tables as rt
import tree_rule as tr
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


# ---- the binding: the restatement against csrc/rows_plan.h itself (tests/cpp/test_rows_plan)

def restated(lens, positions, keys=rp.RULE, slots=1024):
    segs = rt.segments(lens, positions)
    tls = rt.tiles(segs)
    tab = rt.ranges(segs, tls, rt.default_keys if keys == rp.RULE else rt.keys_of(keys))
    return segs, tls, tab, rt.groups(tab, slots)


def test_the_cpp_rules_give_the_restatement_on_every_example_worked_by_hand():
    by_hand = [([0, 5, 0, 0, 33, 0, 16, 0], [9, 7, 0, 0, 64, 0, 3, 0], 128, rp.RULE),    # test_segments_and_tiles_by_hand
               (LONG_LENS, LONG_POS, 1024, rp.RULE), (LONG_LENS, LONG_POS, 1024, 128),    # test_rows_extend_gpu's long contexts
               (LONG_LENS, LONG_POS, 1024, 100), (LONG_LENS, LONG_POS, 1024, 129), (LONG_LENS, LONG_POS, 1024, 0),
               ([200] * 8, [1800] * 8, 2048, 128), ([200], [1800], 2048, 128)]            # test_a_call_in_several_launch_groups
    by_hand += [([n], [S - n], 2048, rp.RULE) for S, n in ((512, 2), (513, 2), (513, 32), (513, 33), (2048, 2), (1025, 17))]   # the rule's edges
    answers = rp.ask([rp.call(lens, pos, S, keys=keys) for lens, pos, S, keys in by_hand])
    for (lens, pos, S, keys), a in zip(by_hand, answers):
        assert a["scratch"]["slots"] == 1024 and a["scratch"]["per_slot"] == 8 * 16 * 128 * 4     # 64 MiB / (8 heads * 16 rows * 128 * 4 bytes)
        assert rp.tables(a) == restated(lens, pos, keys), (lens, pos, S, keys)
        assert (a["M"], a["nseg"], a["ntiles"]) == (sum(lens), len(a["segs"]), len(a["tiles"]))
        assert a["pos"] == [p if n else -1 for n, p in zip(lens, pos)]
    # the literal tables of the by-hand tests, from the C++ side too
    assert answers[0]["segs"] == [[1, 7, 0, 5], [4, 64, 5, 33], [6, 3, 38, 16]] and answers[0]["tiles"] == [[0, 0], [1, 0], [1, 16], [1, 32], [2, 0]]
    assert [x for x in answers[1]["ranges"] if x[0] == 0] == [[0, 0, 0, 512, 0, 2, 0, 0], [0, 0, 512, 1005, 0, 2, 0, 0]]
    assert len(answers[1]["ranges"]) == 20 and answers[1]["groups"] == [[0, 20, True]]
    assert len(answers[6]["ranges"]) == 8 * 201 and len(answers[6]["groups"]) == 2 and len(answers[7]["groups"]) == 1
    # the most ranges of a tile and the tables' reserve: two by the rule, ceil(max_seq_len / 128) under MC_PX_KEYS=128
    assert answers[1]["scratch"]["per_tile"] == 2 and answers[2]["scratch"]["per_tile"] == 8 and answers[6]["scratch"]["per_tile"] == 16
    assert answers[6]["scratch"]["tiles_max"] == 2048 // 16 + 64


def random_call(rng):
    """a call that is valid by construction: position <= length, position + len <= S, lengths summing to at most S"""
    while True:
        B, S = int(rng.integers(1, 65)), int(rng.integers(64, 2049))
        tree = bool(rng.integers(0, 2))
        lens, left = [], min(S, 128) if tree else S
        for _ in range(B):
            n = int(rng.integers(2, 17 if tree else 131)) if rng.integers(0, 3) else 0
            n = n if n <= left else 0
            lens.append(n)
            left -= n
        if any(lens):
            break
    pos = [int(rng.integers(0, S - n + 1)) if n else int(rng.integers(0, S)) for n in lens]
    lengths = [p + int(rng.integers(0, 5)) for p in pos]
    parents = None
    if tree:
        parents = [par for n in lens if n for par in [-1] + [int(rng.integers(0, i)) for i in range(1, n)]]
    return dict(lens=lens, pos=pos, S=S, lengths=lengths, parents=parents, keys=int(rng.choice([rp.RULE, rp.RULE, 0, 128, 384])),
                H=int(rng.choice([8, 32])), hd=int(rng.choice([64, 128])))


def test_the_cpp_rules_give_the_restatement_on_300_random_calls():
    rng = np.random.default_rng(20260101)
    calls = [random_call(rng) for _ in range(300)]
    for c in calls:   # a launch group holds whole tiles: never fewer slots than the most ranges of a tile
        c["most"] = max(e[5] for e in restated(c["lens"], c["pos"], c["keys"], 1 << 20)[2])
        c["slots"] = int(rng.choice([c["most"], c["most"] + 1, 2 * c["most"] + 3, 0]))
    answers = rp.ask([rp.call(c["lens"], c["pos"], c["S"], lengths=c["lengths"], parents=c["parents"], keys=c["keys"], slots=c["slots"],
                              who="mc_tree_verify" if c["parents"] else "mc_extend_rows", n_heads=c["H"], head_dim=c["hd"]) for c in calls])
    assert sum(1 for c in calls if c["parents"]) > 100 and sum(1 for c in calls if not c["parents"]) > 100
    for c, a in zip(calls, answers):
        assert "refused" not in a, (c, a)   # none of them may be refused
        slots = c["slots"] or a["scratch"]["slots"]
        assert a["scratch"]["slots"] == min(32768, max(a["scratch"]["per_tile"], (64 << 20) // (c["H"] * 16 * c["hd"] * 4)))
        assert a["scratch"]["per_tile"] >= c["most"]
        assert rp.tables(a) == restated(c["lens"], c["pos"], c["keys"], slots), c
        if c["parents"]:
            nodes, off = [], 0
            for n in c["lens"]:
                par = c["parents"][off:off + n]
                nodes += [list(x) for x in zip(tr.depths(par), tr.anc_masks(par))] if n else []
                off += n
            assert a["nodes"] == nodes, c
        else:
            assert a["nodes"] == []


def test_every_refusal_of_a_rows_call_by_its_words():
    S = 64
    refusals = [
        (dict(lens=[-1, 2], positions=[0, 0]), "mc_extend_rows: row 0: length below 0 (0 = the row is not in the call)"),
        (dict(lens=[0, 1], positions=[0, 0]), "mc_extend_rows: row 1: a one-token chunk is a step: mc_ragged_step"),
        (dict(lens=[2], positions=[-3], lengths=[0]), "mc_extend_rows: row 0: position below 0"),
        (dict(lens=[2], positions=[9], lengths=[8]), "mc_extend_rows: row 0: position 9 is past the row's length 8 (its cache has no slots written beyond it)"),
        (dict(lens=[5], positions=[60]), "mc_extend_rows: row 0: position + length 65 exceeds max_seq_len (a batch's cache does not roll)"),
        (dict(lens=[2], positions=[10], lengths=[70]), "mc_extend_rows: row 0: position 10 lies below the row's length 70 and the row has rolled"),
        (dict(lens=[3], positions=[0], tokens=[1, 512, 2]), "mc_extend_rows: row 0: token id outside the vocabulary"),
        (dict(lens=[3], positions=[0], tokens=[1, -1, 2]), "mc_extend_rows: row 0: token id outside the vocabulary"),
        (dict(lens=[0, 0], positions=[0, 0]), "mc_extend_rows: no row in the call (every length is 0)"),
        (dict(lens=[40, 40], positions=[0, 0]), "mc_extend_rows: the rows' lengths add up to 80, more than max_seq_len (64): split the call by rows"),
        (dict(lens=[2, 17], positions=[0, 0], verify=True, who="mc_verify_rows"),
         "mc_verify_rows: row 1: a chunk of 17 tokens is longer than MC_VERIFY_MAX_LEN (16)"),
        (dict(lens=[16] * 9, positions=[0] * 9, verify=True, who="mc_verify_rows", max_seq_len=256),
         "mc_verify_rows: the chunks add up to 144 rows, more than MC_VERIFY_MAX_ROWS (128): split the call by rows"),
        (dict(lens=[3], positions=[0], parents=[0, 0, 1], who="mc_tree_verify"),
         "mc_tree_verify: row 0: the parent of node 0 (the root) must be -1, not 0"),
        (dict(lens=[0, 3], positions=[0, 0], parents=[-1, 0, 2], who="mc_tree_verify"),
         "mc_tree_verify: row 1: the parent of node 2 is 2, outside [0, 2) (nodes come in topological order)"),
        (dict(lens=[3], positions=[0], parents=[-1, -1, 0], who="mc_tree_verify"),
         "mc_tree_verify: row 0: the parent of node 1 is -1, outside [0, 1) (nodes come in topological order)"),
    ]
    lines = [rp.call(k.pop("lens"), k.pop("positions"), k.pop("max_seq_len", S), **k) for k, _ in refusals]
    assert [a.get("refused") for a in rp.ask(lines)] == [text for _, text in refusals]
    # a rolled row restarted at 0 is admitted (a chunk at its length would leave the cache); the chunks of the verify limit without `verify` are too
    ok = rp.ask([rp.call([2], [0], S, lengths=[70]), rp.call([2, 17], [0, 0], S)])
    assert ["refused" in a for a in ok] == [False, False]
