"""Speculative verify over a draft tree per row (mc_tree_verify, include/metalchat_hip.h Part 2g) on the device.

  1 a tree that is a chain is mc_verify_rows, bit for bit: accepted, next tokens, picks, all logits, lengths, exported K / V -- also
    with 128-key ranges (MC_PX_KEYS);
  2 isolation: twin batches whose trees differ in ONE node's token agree bit for bit in the logits and picks of every node that does
    not have that node among its ancestors-or-self (a star, two branches forking at the root, a caterpillar);
  3 every node against a chain of oracle.Model.step along its path (the oracle walks the tree in pre-order: its step at
    pos + depth overwrites that slot and sees [0, pos + depth], the node's ancestors), tol(BF16) with max_ulp 2 as
    test_rows_extend_gpu.check_rows; picks are the argmax of the device's own logits and the oracle's pick where clear_gap holds;
  4 acceptance known in advance: the true path is the oracle's greedy chain placed by test_verify_rows_gpu.place from the oracle
    alone, at non-consecutive node indices, a decoy sibling (the oracle's lowest logit) before every true child, under each decoy a
    child carrying the chain's true next token, one wrong token planted at draft index <= 3;
  5 after the call: K / V over the new length bit for bit what mc_verify_rows of the accepted path as a chain writes in layer 0
    (same side of the decoder's 64-row GEMM line), all layers within check_rows' bounds of the oracle, the next mc_ragged_step
    bit for bit that of a fresh row that imported the exported prefix;
  6 four rounds in a loop; the launch log; placement and company; the refusals, with nothing launched.

The greedy chains and their unambiguous positions are those of test_verify_rows_gpu (see its docstring: 161 of 192 positions)."""
import ctypes as C

import numpy as np
import pytest

import modelgen as mg
import parity
import tree_rule as tr
from oracle import mc_oracle as mo
from test_batch_gpu import LLAMA32_1B, SMALL, small_decoder
from test_context_gpu import random_cache
from test_prefill_gpu import tol
from test_rows_extend_gpu import release
from test_rows_prefill_gpu import clear_gap, gemm_launches, prompts_of, setup_rows
from test_verify_rows_gpu import POS, SEED, argmax, chains_of, import_prefix, place, run_from

pytestmark = pytest.mark.gpu
BF16 = 0


@pytest.fixture(scope="module")
def small():
    return mg.make_model(SMALL, seed=11, quant="i4", group=128)


@pytest.fixture(scope="module")
def llama1b():
    return mg.make_model(LLAMA32_1B, seed=5)


# ------------------------------------------------------------------------------------------ tree shapes
def star(n):
    return np.array([-1] + [0] * (n - 1), np.int32)


def two_branches(n):
    """two chains forking at the root: nodes 1, 3, 5, ... and 2, 4, 6, ..."""
    return np.array([-1, 0, 0] + [i - 2 for i in range(3, n)], np.int32)[:n]


def caterpillar(n):
    """a spine 0 - 2 - 4 - ... whose every node also has a leaf (1, 3, 5, ...) in front of its spine child"""
    return np.array([-1] + [(i - 1) // 2 * 2 for i in range(1, n)], np.int32)


def random_tree(n, rng):
    return np.array([-1] + [int(rng.integers(0, i)) for i in range(1, n)], np.int32)


def children_of(parents):
    ch = [[] for _ in parents]
    for i in range(1, len(parents)):
        ch[int(parents[i])].append(i)
    return ch


def decoy_tree(ch, s, n, j):
    """the chain's chunk g[s .. s + n) as a tree: true node T_d (token g[s + d], and for d == j + 1 the planted lowest-logit token)
    at depth d; in front of T_{d+1}, while nodes last, a decoy child of T_d (the oracle's lowest logit after T_d: never the pick)
    and under the decoy a child carrying the chain's true token of depth d + 2.  Returns tokens, parents and the true nodes'
    indices (non-consecutive)."""
    true_tok = [int(t) for t in ch.g[s:s + n]]
    if j is not None:
        true_tok[j + 1] = ch.low[s + j]
        assert true_tok[j + 1] != ch.g[s + j + 1]
    decoys = min(n - 1, (tr.MAX_NODES - n) // 2)
    tokens, parents, true_idx = [true_tok[0]], [-1], [0]
    for d in range(n - 1):
        if d < decoys:
            tokens += [ch.low[s + d], int(ch.g[s + d + 2])]
            parents += [true_idx[d], len(tokens) - 2]
        tokens.append(true_tok[d + 1])
        parents.append(true_idx[d])
        true_idx.append(len(tokens) - 1)
    assert len(tokens) <= tr.MAX_NODES
    return np.array(tokens, np.int32), np.array(parents, np.int32), true_idx


def expect_walk(ch, s, n, j, true_idx):
    """(accepted, next token, path) the oracle alone predicts -- valid where place() found the picks up to the plant unambiguous"""
    a = n - 1 if j is None else j
    return a, int(ch.g[s + a + 1]), true_idx[:a + 1]


def check_tree_row(batch, r, toks, par, acc, nxt, picks, paths, vl, logits, pos, what):
    """what every call must satisfy whatever the tree: picks are the argmax of the call's own logits, the walk is tree_rule's, the
    length and the batch's logits are those of the last accepted node"""
    for i in range(len(toks)):
        assert picks[r][i] == argmax(vl[r][i]), (what, i)
    a, nx, path = tr.walk(toks, par, picks[r])
    assert (int(acc[r]), int(nxt[r]), list(paths[r])) == (a, nx, path), (what, acc[r], nxt[r], paths[r], a, nx, path)
    assert batch.lengths()[r] == pos + a + 1, what
    parity.exact(logits[r], vl[r][path[-1]], f"{what}: the batch's logits are node {path[-1]}'s")


# ------------------------------------------------------------------------------------------ 1
@pytest.mark.parametrize("keys", [None, "128"])
def test_a_chain_tree_is_verify_rows(acc, small, monkeypatch, keys):
    if keys:
        monkeypatch.setenv("MC_PX_KEYS", keys)
    cfg, L = SMALL, SMALL["n_layers"]
    dec = small_decoder(acc, cfg, small)
    pos = [5, 7, 16, 40, 63, 240, 64, 20]           # 63: ends inside a 64-slot range; 240 + 16: the last cache slot
    lens = [2, 3, 5, 8, 11, 16, 13, 16]
    prompts = prompts_of(cfg, lens, 21)
    # (a random chunk is rejected at once; rows 1 and 6 carry the target's own picks so that drafts are accepted, too)
    ver, oa = setup_rows(dec, cfg, small, pos, SEED)
    tree, ob = setup_rows(dec, cfg, small, pos, SEED)
    _, _, first = ver.verify_rows(prompts, pos)
    for r in (1, 6):
        prompts[r][1:] = first[r][:-1]
    va, vn, vp = ver.verify_rows(prompts, pos)
    ta, tn, tp, paths = tree.verify_tree(prompts, [tr.chain(n) for n in lens], pos)
    assert va[1] >= 1 and va[6] >= 1, va
    parity.exact(ta, va, "accepted")
    parity.exact(tn, vn, "next tokens")
    parity.exact(tree.logits(), ver.logits(), "the batch's logits")
    assert list(tree.lengths()) == list(ver.lengths()) == [p + a + 1 for p, a in zip(pos, va)]
    for r, (x, y, u, w) in enumerate(zip(tp, vp, tree.verify_logits(), ver.verify_logits())):
        parity.exact(x, y, f"row {r} picks")
        parity.exact(u, w, f"row {r} logits of every node")
        assert list(paths[r]) == list(range(va[r] + 1)), (r, paths[r])
        for layer in range(L):
            for a, b, name in zip(tree.export_row_kv(r, layer), ver.export_row_kv(r, layer), "KV"):
                parity.exact(a, b, f"row {r} layer {layer} {name}")
    for om in ob:
        om.close()
    tree.release()
    release(ver, oa, dec)


# ------------------------------------------------------------------------------------------ 2
def test_isolation(acc, small):
    cfg = SMALL
    dec = small_decoder(acc, cfg, small)
    pos = POS
    shapes = [star(16), two_branches(13), caterpillar(16), star(16), two_branches(16), caterpillar(16), star(5), caterpillar(7)]
    changed = [1, 3, 2, 15, 4, 7, 0, 6]              # (row 6: the root -- every node depends on it)
    toks = prompts_of(cfg, [len(p) for p in shapes], 61)
    other = [t.copy() for t in toks]
    for r, x in enumerate(changed):
        other[r][x] = (other[r][x] + 1 + r) % cfg["vocab"]
    a, oa = setup_rows(dec, cfg, small, pos, SEED)
    b, ob = setup_rows(dec, cfg, small, pos, SEED)
    _, _, pa, _ = a.verify_tree(toks, shapes, pos)
    _, _, pb, _ = b.verify_tree(other, shapes, pos)
    la, lb = a.verify_logits(), b.verify_logits()
    same = differ = 0
    for r, (par, x) in enumerate(zip(shapes, changed)):
        masks = tr.anc_masks(par)
        for i in range(len(par)):
            if (masks[i] >> x) & 1:
                differ += int(not np.array_equal(la[r][i], lb[r][i]))
                continue
            same += 1
            parity.exact(la[r][i], lb[r][i], f"row {r} node {i} (node {x} changed, not among its ancestors): logits")
            assert pa[r][i] == pb[r][i], (r, i)
    # the star of row 0: 14 of 16 nodes are independent of node 1; and a changed token does reach the nodes below it
    assert same >= 60 and differ >= 8, (same, differ)
    for om in ob:
        om.close()
    b.release()
    release(a, oa, dec)


# ------------------------------------------------------------------------------------------ 3
def oracle_tree_walk(om, first, par, pos, rng, vocab):
    """the oracle steps the tree in pre-order, node i at pos + depth(i).  Tokens are given out on the way: a node's FIRST child in
    index order carries the oracle's pick after the node (the oracle's greedy chain runs root -> first child -> ...), its other
    children random ids.  Returns tokens, per node the oracle's logits, its pick, and the nodes of the greedy chain."""
    n, kids, depth = len(par), children_of(par), tr.depths(par)
    tokens, logits, pick = [0] * n, [None] * n, [0] * n
    tokens[0] = int(first)

    def visit(i):
        otok, ol = om.step(tokens[i], pos + depth[i])
        logits[i], pick[i] = ol, int(otok)
        for k, c in enumerate(kids[i]):
            tokens[c] = pick[i] if k == 0 else int((pick[i] + 1 + rng.integers(0, vocab - 1)) % vocab)
            visit(c)

    visit(0)
    greedy = [0]
    while kids[greedy[-1]]:
        greedy.append(kids[greedy[-1]][0])
    return np.array(tokens, np.int32), logits, pick, greedy


@pytest.mark.parametrize("shape", ["small-int4", "llama32-1b-bf16"])
def test_every_node_against_the_oracle_along_its_path(acc, small, llama1b, shape):
    import metalchat_amd as mc

    cfg, weights = (SMALL, small) if shape == "small-int4" else (LLAMA32_1B, llama1b)
    pos = POS if cfg is SMALL else [9, 7, 64, 20]
    rng = np.random.default_rng(71)
    trees = [caterpillar(16), two_branches(16), random_tree(16, rng), star(9), caterpillar(11), random_tree(12, rng), two_branches(2),
             random_tree(16, rng)][:len(pos)]
    rel, frac = tol(BF16)
    dec = small_decoder(acc, cfg, weights)
    batch = mc.Batch(dec, len(pos))
    oms, walks = [], []
    for r, p in enumerate(pos):
        om = mo.Model(cfg, weights)
        for layer in range(cfg["n_layers"]):
            k, v = random_cache(cfg, p, SEED + 100 * r + layer)
            om.set_kv(layer, k, v)
            batch.import_kv(r, layer, k, v)
        oms.append(om)
        walks.append(oracle_tree_walk(om, np.random.default_rng(r).integers(0, 2048), trees[r], p, rng, cfg["vocab"]))
    toks = [w[0] for w in walks]
    accepted, nxt, picks, paths = batch.verify_tree(toks, trees, pos)
    vl, logits = batch.verify_logits(), batch.logits()
    on_chain = unambiguous = 0
    for r, (tokens, ologits, opick, greedy) in enumerate(walks):
        what = f"{shape} row {r} (pos {pos[r]}, {len(tokens)} nodes)"
        for i in range(len(tokens)):
            st = parity.check(BF16, vl[r][i], ologits[i], rel=rel, max_ulp=2, max_frac=frac, what=f"{what} node {i} logits")
            clear = bool(clear_gap(ologits[i]))
            if clear:
                assert picks[r][i] == opick[i], (what, i, picks[r][i], opick[i])
            if i in greedy:
                on_chain, unambiguous = on_chain + 1, unambiguous + int(clear)
        check_tree_row(batch, r, tokens, trees[r], accepted, nxt, picks, paths, vl, logits, pos[r], what)
        print(f"{what}: last node {st}, accepted {accepted[r]} along {list(paths[r])}")
    print(f"{shape}: {unambiguous} of {on_chain} nodes on the oracle's greedy chains unambiguous")
    assert 2 * unambiguous >= on_chain, (unambiguous, on_chain)
    release(batch, oms, dec)


# ------------------------------------------------------------------------------------------ 4
KINDS = ["first", "middle", "last", "none", "middle", "first", "none", "last"]
WANT_N = [4, 8, 5, 6, 7, 5, 3, 4]     # middle: j = (n - 1) // 2 <= 3; last: j = n - 2 <= 3


def planned_call(batch, cfg, oms, chains, out=None, start=None):
    """per row a decoy_tree of the chain placed by place(); imports the oracle's prefix.  Returns plan[r] = (s, n, j, true_idx)
    and the call's arguments"""
    B = len(chains)
    plan, toks, pars, pos = {}, [None] * B, [None] * B, [0] * B
    for r, ch in enumerate(chains):
        s, n, j = place(ch, WANT_N[r], KINDS[r])
        assert j is None or j <= 3
        import_prefix(batch, r, oms[r], cfg, ch.p + s)
        if r != out:
            toks[r], pars[r], true_idx = decoy_tree(ch, s, n, j)
            plan[r], pos[r] = (s, n, j, true_idx), ch.p + s
    return plan, toks, pars, pos


def test_acceptance_known_in_advance(acc, small):
    import metalchat_amd as mc

    cfg, L = SMALL, SMALL["n_layers"]
    dec = small_decoder(acc, cfg, small)
    oms, chains = chains_of(cfg, small, POS, 24)
    out = 3                                       # the row that is not in the call
    batch = mc.Batch(dec, 8)
    plan, toks, pars, pos = planned_call(batch, cfg, oms, chains, out)
    print(f"(start, length, plant, true nodes) per row {plan}")
    assert any(t[3][1] != 1 for t in plan.values())          # the true path is not at consecutive indices
    before = [batch.export_row_kv(out, layer) for layer in range(L)]
    len_before, logits_before = batch.lengths()[out], batch.logits()[out].copy()
    accepted, nxt, picks, paths = batch.verify_tree(toks, pars, pos)
    vl, logits = batch.verify_logits(), batch.logits()
    for r, (s, n, j, true_idx) in plan.items():
        what = f"row {r} (chain at {s}, {n} true nodes, plant {j})"
        a, nx, path = expect_walk(chains[r], s, n, j, true_idx)
        assert (int(accepted[r]), int(nxt[r]), list(paths[r])) == (a, nx, path), (what, accepted[r], nxt[r], paths[r], a, nx, path)
        check_tree_row(batch, r, toks[r], pars[r], accepted, nxt, picks, paths, vl, logits, pos[r], what)
    exp = tr.walk_rows(toks, pars, picks)
    parity.exact(accepted, exp[0], "accepted against the rule")
    parity.exact(nxt, exp[1], "next tokens against the rule")
    assert accepted[out] == -1 and nxt[out] == -1 and picks[out] is None and paths[out] is None and vl[out] is None
    assert batch.lengths()[out] == len_before
    parity.exact(logits[out], logits_before, f"row {out} (not in the call): logits")
    for layer, (k, v) in enumerate(before):
        gk, gv = batch.export_row_kv(out, layer)
        parity.exact(gk, k, f"row {out} (not in the call) layer {layer} K")
        parity.exact(gv, v, f"row {out} (not in the call) layer {layer} V")
    release(batch, oms, dec)


# ------------------------------------------------------------------------------------------ 5
@pytest.mark.parametrize("shape", ["small-int4", "llama32-1b-bf16"])
def test_after_the_call(acc, small, llama1b, shape):
    import metalchat_amd as mc

    cfg, weights = (SMALL, small) if shape == "small-int4" else (LLAMA32_1B, llama1b)
    L = cfg["n_layers"]
    positions = POS if cfg is SMALL else [9, 7, 64, 20]
    B = len(positions)
    rel, frac = tol(BF16)
    dec = small_decoder(acc, cfg, weights)
    oms, chains = chains_of(cfg, weights, positions, 24)
    batch, chainb = mc.Batch(dec, B), mc.Batch(dec, B)
    plan, toks, pars, pos = planned_call(batch, cfg, oms, chains)
    for r, ch in enumerate(chains):
        import_prefix(chainb, r, oms[r], cfg, pos[r])
    dec.launch_log(True)
    accepted, nxt, picks, paths = batch.verify_tree(toks, pars, pos)
    tree_side = any(n.startswith("mc_pf2_gemm") for n in dec.launched())
    assert any(a >= 1 and list(p) != list(range(a + 1)) for a, p in zip(accepted, paths)), (accepted, paths)   # something was moved
    # the accepted path as a chain, filled up to the tree's length with other ids: the same packed rows, the same GEMM
    fill = prompts_of(cfg, [len(t) for t in toks], 81)
    chunks = []
    for r in range(B):
        c = fill[r].copy()
        c[:accepted[r] + 1] = toks[r][paths[r]]
        chunks.append(c)
    dec.launch_log(True)
    ca, _, _ = chainb.verify_rows(chunks, pos)
    assert any(n.startswith("mc_pf2_gemm") for n in dec.launched()) == tree_side
    at = np.array(pos) + accepted + 1
    assert list(batch.lengths()) == list(at)
    fresh = mc.Batch(dec, B)
    for r in range(B):
        what = f"{shape} row {r} (accepted {accepted[r]} along {list(paths[r])})"
        assert ca[r] >= accepted[r], (what, ca[r])          # (the path's tokens are the target's unambiguous picks)
        tk, tv = batch.export_row_kv(r, 0)
        ck, cv = chainb.export_row_kv(r, 0)
        assert tk.shape[0] == at[r]
        parity.exact(tk, ck[:at[r]], f"{what}: layer 0 K against mc_verify_rows of the path")
        parity.exact(tv, cv[:at[r]], f"{what}: layer 0 V against mc_verify_rows of the path")
        # the oracle along the accepted path
        om = mo.Model(cfg, weights)
        for layer in range(L):
            k, v = oms[r].kv(layer)
            om.set_kv(layer, k[:pos[r]], v[:pos[r]])
        for d, i in enumerate(paths[r]):
            om.step(int(toks[r][i]), pos[r] + d)
        for layer in range(L):
            gk, gv = batch.export_row_kv(r, layer)
            ok, ov = om.kv(layer)
            assert gk.shape[0] == at[r]
            parity.exact(gk[:pos[r]], ok[:pos[r]], f"{what} layer {layer} context K")
            parity.exact(gv[:pos[r]], ov[:pos[r]], f"{what} layer {layer} context V")
            parity.check(BF16, gk[pos[r]:], ok[pos[r]:at[r]], rel=rel, max_ulp=2, max_frac=frac, what=f"{what} layer {layer} K")
            parity.check(BF16, gv[pos[r]:], ov[pos[r]:at[r]], rel=rel, max_ulp=2, max_frac=frac, what=f"{what} layer {layer} V")
            fresh.import_kv(r, layer, gk, gv)
        om.close()
    a, b = batch.step_rows(nxt, at), fresh.step_rows(nxt, at)
    parity.exact(a, b, "the next step: picks")
    parity.exact(batch.logits(), fresh.logits(), "the next step: logits")
    assert list(batch.lengths()) == list(fresh.lengths()) == list(at + 1)
    for r in range(B):
        for layer in range(L):
            for x, y, name in zip(batch.export_row_kv(r, layer), fresh.export_row_kv(r, layer), "KV"):
                parity.exact(x, y, f"the next step: row {r} layer {layer} {name}")
    fresh.release()
    chainb.release()
    release(batch, oms, dec)


# ------------------------------------------------------------------------------------------ 6
def test_a_loop_of_four_rounds(acc, small):
    """every round continues at positions[r] + accepted[r] + 1 with the oracle's token there, behind a cache the device wrote (and
    compacted).  The walk, the lengths and the batch's logits are checked against the rule in every round; accepted / next / path
    against the oracle's prediction where the oracle's picks up to the plant are unambiguous"""
    import metalchat_amd as mc

    cfg = SMALL
    dec = small_decoder(acc, cfg, small)
    oms, chains = chains_of(cfg, small, POS, 80)
    batch = mc.Batch(dec, 8)
    for r, ch in enumerate(chains):
        import_prefix(batch, r, oms[r], cfg, ch.p)
    start, moved = [0] * 8, 0
    for rnd in range(4):
        toks, pars, pos, plan = [None] * 8, [None] * 8, [0] * 8, {}
        for r, ch in enumerate(chains):
            s, run = start[r], run_from(ch.clear, start[r])
            want = (r + 2 * rnd) % 5                  # a different plant per row and round; 4: none
            if want == 4 and run >= 2:
                n, j = min(run, 6), None
            else:
                j = min(want % 4, max(run - 1, 0))
                j = next((k for k in range(j, -1, -1) if ch.clear[s + k + 1]), j)
                n = min(8, j + 2 + r % 3)
            toks[r], pars[r], true_idx = decoy_tree(ch, s, n, j)
            plan[r], pos[r] = (s, n, j, true_idx), ch.p + s
        accepted, nxt, picks, paths = batch.verify_tree(toks, pars, pos)
        vl, logits = batch.verify_logits(), batch.logits()
        for r, (s, n, j, true_idx) in plan.items():
            ch, what = chains[r], f"round {rnd} row {r}"
            check_tree_row(batch, r, toks[r], pars[r], accepted, nxt, picks, paths, vl, logits, pos[r], what)
            a = n - 1 if j is None else j
            if all(ch.clear[s:s + a + 1]):
                assert (int(accepted[r]), int(nxt[r]), list(paths[r])) == expect_walk(ch, s, n, j, true_idx), (what, accepted[r], paths[r])
            else:
                assert accepted[r] <= a, (what, accepted[r], a)      # the plant is rejected for certain
            moved += int(list(paths[r]) != list(range(accepted[r] + 1)))
            start[r] = s + int(accepted[r]) + 1       # the oracle's token g[start] goes in at the row's new length
    assert moved >= 4, moved                          # (the loop did exercise the compaction)
    release(batch, oms, dec)


TV_NAMES = {"mc_pp_rope_cache_bfloat": "mc_tv_rope_cache_bfloat", "mc_pp_rope_cache_parts_bfloat": "mc_tv_rope_cache_parts_bfloat",
            "mc_v_accept": "mc_tv_accept"}


def tv_name(n):
    for a in ("sums", "pv"):
        if n.startswith(f"mc_px_{a}"):
            return n.replace("mc_px_", "mc_tv_")
    return TV_NAMES.get(n, n)


def test_the_launch_log(acc, small):
    import metalchat_amd as mc

    cfg = SMALL
    dec = small_decoder(acc, cfg, small)
    lens = [2, 16, 5, 16, 9, 3, 16, 12]
    prompts = prompts_of(cfg, lens, 41)
    rng = np.random.default_rng(42)
    trees = [random_tree(n, rng) for n in lens]
    ver, oa = setup_rows(dec, cfg, small, POS, 600)
    tree, ob = setup_rows(dec, cfg, small, POS, 600)
    warm = mc.Batch(dec, 8)
    warm.extend_rows(prompts, [0] * 8)   # (whatever the decoder's first prompt pass prepares once is done before the logs)
    warm.release()
    dec.launch_log(True)
    ver.verify_rows(prompts, POS)
    verify = dec.launched()
    dec.launch_log(True)
    tree.verify_tree(prompts, trees, POS)
    got = dec.launched()
    # mc_verify_rows' launches under their mc_tv_* names (mc_px_reduce_* is reused), plus one compaction
    assert got == [tv_name(n) for n in verify] + ["mc_tv_compact_bfloat"], (got, verify)
    assert [n for n in got if n.startswith("mc_tv_sums")] and not [n for n in got if n.startswith(("mc_px_sums", "mc_px_pv", "mc_pp_rope", "mc_v_accept"))]
    assert gemm_launches(got) == gemm_launches(verify)
    # a verify_rows call on the batch that verified a tree: no mc_tv_* launch
    dec.launch_log(True)
    tree.verify_rows([p[:2] for p in prompts], tree.lengths())
    after = dec.launched()
    assert not [n for n in after if n.startswith("mc_tv_")], after
    for om in ob:
        om.close()
    tree.release()
    release(ver, oa, dec)


# (batch size, {batch row: chunk index}) of one call; the trees' sizes are COMPANY_LENS, their contexts POS
COMPANY_LENS = [2, 16, 5, 16, 9, 3, 16, 12]
COMPANY_CALLS = [
    (8, {r: r for r in range(8)}),                                  # 79 packed rows
    (8, {5: 0, 2: 1, 7: 2, 0: 3, 3: 4, 6: 5, 1: 6, 4: 7}),          # 79: every chunk in another batch row
    (5, {0: 6, 1: 1, 2: 3, 3: 4, 4: 7}),                            # 69: a smaller batch, other company
    (3, {0: 6, 1: 1, 2: 4}),                                        # 41
    (3, {2: 4}),                                                    # 9: alone in the call
    (8, {5: 6, 0: 2, 3: 0}),                                        # 23
    (4, {3: 1, 0: 7, 1: 6, 2: 2}),                                  # 49
]


@pytest.mark.parametrize("shape", ["small-int4", "llama32-1b-bf16"])
def test_placement_and_company(acc, small, llama1b, shape):
    """a tree's picks, accepted, path, next token, logits of every node and K / V do not depend on its batch row, on B or on which
    other rows are in the call; with int4 weights among the calls on the same side of the decoder's 64-row GEMM line (see
    test_verify_rows_gpu.test_placement_and_company)"""
    import metalchat_amd as mc

    cfg, weights = (SMALL, small) if shape == "small-int4" else (LLAMA32_1B, llama1b)
    L, int4 = cfg["n_layers"], shape == "small-int4"
    dec = small_decoder(acc, cfg, weights)
    prompts = prompts_of(cfg, COMPANY_LENS, 51)
    rng = np.random.default_rng(52)
    trees = [random_tree(n, rng) for n in COMPANY_LENS]
    ref = {}
    for B, rows in COMPANY_CALLS:
        M = sum(COMPANY_LENS[i] for i in rows.values())
        side = "short" if int4 and M <= 64 else "long"
        batch = mc.Batch(dec, B)
        toks, pars, pos = [None] * B, [None] * B, [0] * B
        for r, i in rows.items():
            toks[r], pars[r], pos[r] = prompts[i], trees[i], POS[i]
            for layer in range(L):
                batch.import_kv(r, layer, *random_cache(cfg, POS[i], 700 + 100 * i + layer))
        dec.launch_log(True)
        accepted, nxt, picks, paths = batch.verify_tree(toks, pars, pos)
        streamed = any(n.startswith("mc_pf2_gemm") for n in dec.launched())
        assert streamed == (side == "short"), (shape, B, rows, M)
        vl, logits = batch.verify_logits(), batch.logits()
        for r in range(B):
            if r not in rows:
                assert accepted[r] == nxt[r] == -1 and picks[r] is None and paths[r] is None and vl[r] is None, (B, rows, r)
                continue
            i, what = rows[r], f"{shape} B {B} rows {rows} ({M} packed rows): tree {rows[r]}"
            got = dict(accepted=int(accepted[r]), next=int(nxt[r]), path=paths[r], picks=picks[r], verify_logits=vl[r].copy(), logits=logits[r].copy())
            for layer in range(L):
                got[f"K{layer}"], got[f"V{layer}"] = batch.export_row_kv(r, layer)
            if (side, i) not in ref:
                ref[side, i] = got, what
                continue
            exp, first = ref[side, i]
            for name in got:
                parity.exact(got[name], exp[name], f"{what} against {first}: {name}")
        batch.release()
    assert {i for _, i in ref} == set(range(8))
    dec.release()


def test_refusals(acc, small):
    import metalchat_amd as mc

    S = SMALL["max_seq_len"]
    dec = small_decoder(acc, SMALL, small)
    batch = mc.Batch(dec, 4)
    lib = mc.capi()
    ptr = C.POINTER(C.c_int32)
    dec.launch_log(True)
    assert lib.mc_verify_get_logits(batch._h, np.zeros(8, np.uint16).ctypes.data_as(C.c_void_p)) == 1
    assert lib.mc_last_error().decode().startswith("mc_verify_get_logits: no mc_verify_rows call"), lib.mc_last_error()
    assert dec.launched() == []
    batch.extend_rows([[1, 2, 3], None, None, None], [0, 0, 0, 0])  # row 0: length 3

    def call(tokens, lens, positions, words, parents=None, null_parents=False):
        t = np.ascontiguousarray(np.asarray(list(tokens) + [0], np.int32))
        if parents is None:   # chains
            parents = [i for n in lens for i in range(-1, max(n, 0) - 1)]
        par = np.ascontiguousarray(np.asarray(list(parents) + [0], np.int32))
        ln = np.ascontiguousarray(lens, np.int32)
        p = np.ascontiguousarray(positions, np.int32)
        a, out, picks, paths = np.zeros(4, np.int32), np.zeros(4, np.int32), np.zeros(len(t), np.int32), np.zeros(64, np.int32)
        dec.launch_log(True)
        st = lib.mc_tree_verify(batch._h, t.ctypes.data_as(ptr), None if null_parents else par.ctypes.data_as(ptr), ln.ctypes.data_as(ptr),
                                p.ctypes.data_as(ptr), a.ctypes.data_as(ptr), out.ctypes.data_as(ptr), paths.ctypes.data_as(ptr),
                                picks.ctypes.data_as(ptr))
        assert st == 1, words
        msg = lib.mc_last_error().decode()
        assert msg.startswith("mc_tree_verify: "), msg
        assert words in msg, (words, msg)
        assert dec.launched() == [], words
        assert list(batch.lengths()) == [3, 0, 0, 0], words

    # every case of test_rows_extend_gpu.test_refusals
    call([], [0, 0, 0, 0], [0, 0, 0, 0], "no row in the call")
    call([1, 2], [2, -1, 0, 0], [0, 0, 0, 0], "row 1: length below 0", parents=[-1, 0])
    call([1, 2, 3], [2, 1, 0, 0], [0, 0, 0, 0], "row 1: a one-token chunk is a step")
    call([1, 2], [0, 0, 2, 0], [0, 0, -1, 0], "row 2: position below 0")
    call([1, 2], [2, 0, 0, 0], [4, 0, 0, 0], "row 0: position 4 is past the row's length 3")
    call(list(range(S - 2)), [S - 2, 0, 0, 0], [3, 0, 0, 0], "row 0: position + length")
    call([1, SMALL["vocab"]], [0, 0, 0, 2], [0, 0, 0, 0], "row 3: token id outside the vocabulary")
    call([1, -5], [0, 0, 0, 2], [0, 0, 0, 0], "row 3: token id outside the vocabulary")
    call(list(range(S)) + [1, 2], [S - 100, 100, 2, 0], [0, 0, 0, 0], "add up to 258, more than max_seq_len")
    # a chunk of 17
    call(list(range(2 + 17)), [2, 0, 17, 0], [0, 0, 0, 0], "row 2: a chunk of 17 tokens is longer than MC_VERIFY_MAX_LEN (16)")
    # the parents
    call([1, 2], [2, 0, 0, 0], [0, 0, 0, 0], "null argument", null_parents=True)
    call([1, 2, 3, 4, 5], [2, 0, 3, 0], [0, 0, 0, 0], "row 2: the parent of node 0 (the root) must be -1, not 0", parents=[-1, 0, 0, 0, 1])
    call([1, 2, 3, 4, 5], [2, 0, 3, 0], [0, 0, 0, 0], "row 2: the parent of node 2 is 2, outside [0, 2)", parents=[-1, 0, -1, 0, 2])
    call([1, 2, 3, 4, 5], [2, 0, 3, 0], [0, 0, 0, 0], "row 2: the parent of node 1 is -1, outside [0, 1)", parents=[-1, 0, -1, -1, 0])
    call([1, 2, 3, 4, 5], [2, 0, 3, 0], [0, 0, 0, 0], "row 0: the parent of node 1 is 7, outside [0, 1)", parents=[-1, 7, -1, 0, 0])
    # the default sampler set on the decoder
    dec.set_sampler(mc.SAMPLER_DEFAULT, top_k=40, temperature=0.6, top_p=0.9)
    call([1, 2], [2, 0, 0, 0], [0, 0, 0, 0], "greedy")
    dec.set_sampler(mc.SAMPLER_GREEDY)
    accepted, nxt, picks, paths = batch.verify_tree([[1, 2, 3], None, None, None], [[-1, 0, 0], None, None, None], [3, 0, 0, 0])
    assert accepted[0] >= 0 and batch.lengths()[0] == 3 + accepted[0] + 1
    vl = batch.verify_logits()
    assert vl[0].shape == (3, SMALL["vocab"]) and vl[1] is None
    batch.release()
    dec.release()
