"""Speculative verify over a draft tree (mc_tree_verify, include/metalchat_hip.h Part 2g) without a GPU: the entry point is declared
once, exported and bound; the twelve mc_tv_* kernels are exactly the set in the code object and keep nothing in private memory; null
arguments are refused before a batch is looked at; and the rules (tree_rule.py, which the GPU tests hold the device to) on cases
worked by hand -- its depths and ancestor masks also against the host's own tree_nodes (csrc/rows_plan.h through tests/cpp/test_rows_plan;
random trees: test_rows_tables_cpu.py)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

import batch_plan_program as bp
import metalchat_amd as mc
import rows_plan_program as rp
import tree_rule as tr
from metalchat_amd import build as b

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
READELF = ["/opt/rocm/lib/llvm/bin/llvm-readelf", "/usr/bin/readelf"]
TREE_KERNELS = [f"mc_tv_{a}_bfloat_hd{hd}" for a in ("sums", "sums2", "pv", "pv2") for hd in (64, 128)] + \
               ["mc_tv_rope_cache_bfloat", "mc_tv_rope_cache_parts_bfloat", "mc_tv_accept", "mc_tv_compact_bfloat"]


def ints(*v):
    return (C.c_int32 * max(len(v), 1))(*v)


def readelf(*args):
    hsaco, _ = b.build_all()
    tool = next((t for t in READELF if os.path.exists(t)), None)
    assert tool is not None, "no readelf available"
    return subprocess.check_output([tool, *args, hsaco], text=True)


def test_the_entry_point_is_declared_once_exported_and_bound():
    text = open(os.path.join(ROOT, "include", "metalchat_hip.h")).read()
    assert re.findall(r"\b(mc_tree_\w+)\s*\(", text) == ["mc_tree_verify"]
    assert "Part 2g" in text
    lib = mc.capi()
    assert "mc_tree_verify" in lib._prototypes
    getattr(lib, "mc_tree_verify")
    assert callable(getattr(mc.Batch, "verify_tree")) and callable(getattr(mc.Batch, "verify_logits"))
    # b, tokens, parents, lens, positions, accepted, next_tokens, paths, picks
    res, args = lib._prototypes["mc_tree_verify"]
    assert len(args) == 9 and res == lib._prototypes["mc_verify_rows"][0]
    assert args[1:] == [lib._prototypes["mc_verify_rows"][1][1]] * 8


def test_the_tree_kernels_are_exactly_the_set_in_the_code_object():
    assert len(TREE_KERNELS) == 12
    formed = bp.formed_names()   # (the host forms these names: batch_plan.h through tests/cpp/test_batch_plan)
    for name in ("mc_tv_accept", "mc_tv_compact_bfloat"):
        assert name in formed, name
    dec = open(os.path.join(ROOT, "metalchat_amd", "csrc", "prefill_plan.h")).read()   # (the names prefill.cc launches are formed there)
    for stem in ('"mc_tv_sums"', '"mc_tv_pv"', '"mc_tv_rope_cache_bfloat"', '"mc_tv_rope_cache_parts_bfloat"'):
        assert stem in dec, stem
    out = readelf("--symbols", "--wide")
    symbols = {line.split()[-1] for line in out.splitlines() if " FUNC " in line}
    assert sorted(s for s in symbols if s.startswith("mc_tv_")) == sorted(TREE_KERNELS)


def test_no_tree_kernel_keeps_private_memory():
    """the code object's notes, read as test_verify_rows_cpu reads them: a private segment of 0 bytes and no spills for each"""
    name, fields = None, {}
    for line in readelf("--notes").splitlines():
        line = line.strip()
        if line.startswith("- .") or line.startswith(".") or line.startswith("-"):
            key, _, val = line.lstrip("- ").partition(":")
            key, val = key.strip(), val.strip()
            if key == ".name":
                name = val
                fields[name] = {}
            elif name and key in (".private_segment_fixed_size", ".vgpr_spill_count", ".sgpr_spill_count"):
                fields[name][key] = int(val)
    for n in TREE_KERNELS:
        assert n in fields, n
        assert fields[n] == {".private_segment_fixed_size": 0, ".vgpr_spill_count": 0, ".sgpr_spill_count": 0}, (n, fields[n])


def test_null_arguments_are_refused_without_a_device():
    lib = mc.capi()
    fake = C.c_void_p(1)  # never dereferenced: the pointers are checked first
    toks, par, lens, pos, acc, out, paths = ints(1, 2), ints(-1, 0), ints(2), ints(0), ints(0), ints(0, 0), ints(*([0] * 16))
    good = [fake, toks, par, lens, pos, acc, out, paths, out]
    for missing in range(6):   # b, tokens, parents, lens, positions, accepted; next_tokens, paths and picks may be null
        args = list(good)
        args[missing] = None
        assert lib.mc_tree_verify(*args) == 1, missing
        assert b"mc_tree_verify: null argument" in lib.mc_last_error(), missing


def test_depths_and_ancestor_masks_by_hand():
    #        0
    #      / | \
    #     1  2  3
    #        |  | \
    #        4  5  6
    #        |
    #        7
    par = [-1, 0, 0, 0, 2, 3, 3, 4]
    assert tr.depths(par) == [0, 1, 1, 1, 2, 2, 2, 3]
    assert tr.anc_masks(par) == [0b1, 0b11, 0b101, 0b1001, 0b10101, 0b101001, 0b1001001, 0b10010101]
    assert tr.ancestors(par, 7) == [0, 2, 4, 7] and tr.ancestors(par, 0) == [0]
    # a chain: node i sees nodes 0 .. i -- mc_verify_rows' causal rule
    assert list(tr.chain(5)) == [-1, 0, 1, 2, 3]
    assert tr.depths(tr.chain(16)) == list(range(16))
    assert tr.anc_masks(tr.chain(16)) == [(2 << i) - 1 for i in range(16)]
    # the host's node table (rows_plan.h tree_nodes) for the same trees, two rows of one call: the tree above and the chain
    a = rp.ask([rp.call([8, 0, 16], [5, 0, 40], 64, parents=par + list(tr.chain(16)), who="mc_tree_verify")])[0]
    assert a["nodes"] == [list(x) for x in zip(tr.depths(par), tr.anc_masks(par))] + [[i, (2 << i) - 1] for i in range(16)]
    assert a["M"] == 24 and a["ntiles"] == 2 and a["segs"] == [[0, 5, 0, 8], [2, 40, 8, 16]]


def test_the_walk_on_cases_worked_by_hand():
    # a star: the root's pick (8) is its third child, node 3; nothing below it -> one accepted, the next token is node 3's pick
    assert tr.walk([5, 6, 7, 8, 9], [-1, 0, 0, 0, 0], [8, 1, 2, 3, 4]) == (1, 3, [0, 3])
    # a star none of whose children is the pick
    assert tr.walk([5, 6, 7, 8, 9], [-1, 0, 0, 0, 0], [4, 1, 2, 3, 4]) == (0, 4, [0])
    # a decoy sibling (node 1, token 6) before the true child (node 2, token 7); the walk goes on below node 2
    assert tr.walk([5, 6, 7, 9, 9], [-1, 0, 0, 1, 2], [7, 9, 9, 1, 2]) == (2, 2, [0, 2, 4])
    # a match under a rejected node never counts: node 3 (token 9 under the decoy node 1) equals the pick after node 1, but node 1
    # itself was not the root's pick; node 2 is, and it has no child
    assert tr.walk([5, 6, 7, 9], [-1, 0, 0, 1], [7, 9, 3, 1]) == (1, 3, [0, 2])
    # duplicate siblings: nodes 1 and 2 both carry the pick 7 -- the lower index wins, so node 4 (under node 2) is out of reach
    # although its token is the pick after node 2; node 3 (under node 1) misses the pick after node 1
    assert tr.walk([5, 7, 7, 1, 2], [-1, 0, 0, 1, 2], [7, 9, 2, 0, 0]) == (1, 9, [0, 1])
    # a chain is verify_rule.accept
    assert tr.walk([5, 7, 8, 9], tr.chain(4), [7, 3, 9, 1])[:2] == (1, 3)
    assert tr.walk([5, 7, 8, 9], tr.chain(4), [7, 8, 9, 1]) == (3, 1, [0, 1, 2, 3])
    # rows: one not in the call
    acc, nxt, paths = tr.walk_rows([[5, 6, 7, 9, 9], None], [[-1, 0, 0, 1, 2], None], [[7, 9, 9, 1, 2], None])
    assert acc.dtype == nxt.dtype == paths.dtype == np.int32 and paths.shape == (2, 16)
    assert list(acc) == [2, -1] and list(nxt) == [2, -1]
    assert list(paths[0]) == [0, 2, 4] + [-1] * 13 and list(paths[1]) == [-1] * 16


def test_the_compaction_of_path_0_2_3_by_hand():
    # slots 10 .. 14 hold nodes 0 .. 4 of a chunk at pos 10; path [0, 2, 3]: slot 11 <- slot 12, slot 12 <- slot 13, the rest stays
    slots = np.arange(100, 120)
    out = tr.compact(slots, 10, [0, 2, 3])
    exp = slots.copy()
    exp[11], exp[12] = 112, 113
    assert list(out) == list(exp)
    assert list(slots) == list(range(100, 120))   # the input is not changed
    # a chain moves nothing
    assert list(tr.compact(slots, 3, [0, 1, 2, 3])) == list(slots)


def test_trie_merges_candidates_in_topological_order():
    # three continuations of token 5: two share the prefix [6, 7]
    tokens, parents = tr.trie(5, [[6, 7, 8], [6, 7, 9, 1], [2, 3]])
    assert list(tokens) == [5, 6, 7, 8, 9, 1, 2, 3]
    assert list(parents) == [-1, 0, 1, 2, 2, 4, 0, 6]
    tr.check_parents(parents)
    # full at max_nodes: the candidate is cut, a later one that needs no new node is not
    tokens, parents = tr.trie(5, [[1, 2, 3], [4, 4, 4], [1, 2]], max_nodes=5)
    assert list(tokens) == [5, 1, 2, 3, 4] and list(parents) == [-1, 0, 1, 2, 0]
    assert len(tr.trie(0, [range(1, 40)])[0]) == 16
