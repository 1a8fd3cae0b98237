"""Kernel-level tests of speculative verify over a draft tree (metalchat_amd/csrc/kernels/tree_kernels.hip), each kernel launched BY
NAME on buffers the test owns (the helpers and tables of test_rows_kernels_gpu.py / rows_tables.py; the node table of tree_rule.py):

  * chain masks: mc_tv_sums{,2} / mc_tv_pv{,2} are mc_px_sums{,2} / mc_px_pv{,2} bit for bit -- n_rep 1 and 3 (the one-head names)
    and 4 (the two-head names), head_dim 64 and 128, tiles in one and in several 128-key ranges;
  * tree masks: every node against the oracle's attention over its visible keys -- the context plus its ancestors and itself,
    gathered contiguously -- with the bound of the decode attention at H = 32 (test_rows_kernels_gpu.check_against); chunks at pos 0,
    63, 120 (the nodes straddle key 128 with 128-key ranges) and max_seq - 16; NaN in the K of a node's slot changes no bit of the
    nodes that do not see it, NaN in K and V past pos + len changes no bit at all;
  * mc_tv_rope_cache{,_parts}: q rows, K slots and V columns bit for bit the oracle's rope at pos + depth written to slot pos + i
    (whole caches compared), the q rows bit for bit mc_pp_rope_cache's of the same rows at pos + depth, and a chain tree the whole
    mc_pp_rope_cache launch;
  * mc_tv_accept on random trees against tree_rule.walk_rows; mc_tv_compact_bfloat on patterned caches against tree_rule.compact,
    whole buffers compared (every slot outside [pos + 1, pos + a] untouched), head_dim 64 and 128, 2 layers."""
import numpy as np
import pytest

import parity
import rows_tables as rt
import tree_rule as tr
from test_attn_kernels_gpu import oracle_attention
from test_batch_kernels_gpu import GUARD, NAN, bf, guarded
from test_rows_kernels_gpu import (B, KEYS128, PX_REDUCE, ROPE_S, Call, RopeCase, check_against, etab, one_group, pattern,  # noqa: F401
                                   px_launch)

pytestmark = pytest.mark.gpu
TV = {(64, 1): ("mc_tv_sums_bfloat_hd64", "mc_tv_pv_bfloat_hd64"), (64, 2): ("mc_tv_sums2_bfloat_hd64", "mc_tv_pv2_bfloat_hd64"),
      (128, 1): ("mc_tv_sums_bfloat_hd128", "mc_tv_pv_bfloat_hd128"), (128, 2): ("mc_tv_sums2_bfloat_hd128", "mc_tv_pv2_bfloat_hd128")}


def random_tree(n, rng):
    return [-1] + [int(rng.integers(0, i)) for i in range(1, n)]


def node_table(c, trees):
    """tv_node (depth, anc) per packed row of the call's buffers; rows of no segment hold depth -1 and no ancestor at all"""
    tab = np.zeros((c.rows_buf, 2), np.int64)
    tab[:, 0] = -1
    for i in range(len(c.items)):
        _, _, off, n = c.segs[c.seg_of[i]]
        assert len(trees[i]) == n <= 16
        tab[off:off + n, 0], tab[off:off + n, 1] = tr.depths(trees[i]), tr.anc_masks(trees[i])
    return tab.astype(np.uint32).view(np.int32).reshape(-1)


def tv_launch(acc, etab, c, tab, nh, nodes):
    """mc_tv_sums, mc_tv_pv and (a split tile) mc_px_reduce as prefill.cc run_prefill launches them for a tree call: one group"""
    import metalchat_amd as mc

    H, hd = c.H, c.hd
    count, split = len(tab), any(e[5] > 1 for e in tab)
    tabb, nodeb = acc.to_device(rt.words(tab, 8).reshape(-1)), acc.to_device(nodes)
    sumsb = acc.to_device(np.full(count * H * 16, np.nan, np.float32))
    partb = acc.to_device(np.full(count * H * 16 * hd, np.nan, np.float32))
    out0 = pattern(c.rows_buf * H * hd)
    outb = acc.to_device(out0)
    k_sums, k_pv = (acc.load(n) for n in TV[hd, nh])
    u32 = np.uint32
    grid = (H // nh * 256, count, 1)
    mc.KernelTask(k_sums, grid, (256, 1, 1), [c.qb, c.segb, tabb, u32(0), c.kb, np.uint64(c.cstride), sumsb, u32(H), u32(c.n_rep),
                                              u32(c.max_seq), c.scale, etab, nodeb])()
    mc.KernelTask(k_pv, grid, (256, 1, 1), [c.qb, c.segb, tabb, u32(0), c.kb, c.vb, np.uint64(c.cstride), sumsb, partb, outb, u32(H),
                                            u32(c.n_rep), u32(c.max_seq), c.scale, etab, nodeb])()
    if split:
        mc.KernelTask(acc.load(PX_REDUCE[hd]), (H * 256, count, 1), (256, 1, 1), [c.segb, tabb, u32(0), partb, outb, u32(H)])()
    acc.wait()
    return outb.download(np.uint16, out0.size).reshape(c.rows_buf, H, hd), sumsb.download(np.float32, count * H * 16).reshape(count, H, 16)


# chunks of 2 .. 16 nodes at pos 0, 63, 120 (16 nodes: slots 120 .. 135 straddle key 128), inside and at the end of the cache
MAX_SEQ = 1024
ITEMS = [(0, 0, 16), (1, 63, 16), (2, 120, 16), (4, MAX_SEQ - 16, 16), (5, 600, 2), (6, 127, 9), (7, 0, 5)]


# ------------------------------------------------------------------------------------------ chain masks
@pytest.mark.parametrize("hd,H,KV", [(64, 8, 8), (128, 6, 2), (64, 8, 2), (128, 8, 2), (128, 4, 4), (64, 6, 2)])
def test_tv_attention_with_chain_masks_is_px_attention(acc, etab, hd, H, KV):
    c = Call(MAX_SEQ, ITEMS, H, KV, hd, seed=hd + H + KV, gap=3).device(acc, "big")
    nodes = node_table(c, [tr.chain(n) for _, _, n in ITEMS])
    nh = 2 if c.n_rep % 2 == 0 else 1
    assert (c.n_rep, nh) in ((1, 1), (3, 1), (4, 2))
    for rule, name in ((rt.default_keys, "default rule"), (KEYS128, "128-key ranges")):
        tab = rt.ranges(c.segs, c.tiles, rule)
        assert {e[5] for e in tab} >= {1, 2}, name           # tiles in one range and in several
        what = f"{TV[hd, nh][0]} / {TV[hd, nh][1]} n_rep {c.n_rep} {name}"
        pout, psums = px_launch(acc, etab, c, tab, one_group(tab), nh)
        tout, tsums = tv_launch(acc, etab, c, tab, nh, nodes)
        parity.exact(tsums, psums, f"{what}: sums against mc_px_sums")
        parity.exact(tout, pout, f"{what}: outputs against mc_px_pv")
    c.check_caches_untouched(f"chain masks hd {hd}")


# ------------------------------------------------------------------------------------------ tree masks
def tree_reference(c, trees):
    """node j of segment i: the oracle's attention of q_j over the context [0, pos) and the slots of its ancestors and itself"""
    ref = []
    for i, (_, p, n) in enumerate(c.items):
        rows = []
        for j in range(n):
            vis = list(range(p)) + [p + a for a in tr.ancestors(trees[i], j)]
            rows.append(oracle_attention(c.q[i][j], c.k[i][vis], c.v[i][vis], c.n_rep, float(c.scale)))
        ref.append(np.stack(rows))
    return ref


@pytest.mark.parametrize("hd,H,KV", [(128, 32, 8), (64, 32, 32), (64, 32, 8), (128, 48, 16)])
def test_tv_attention_with_tree_masks_against_the_oracle(acc, etab, hd, H, KV):
    rng = np.random.default_rng(hd + KV)
    trees = [random_tree(n, rng) for _, _, n in ITEMS]
    trees[0] = [-1] + [0] * 15                               # a star
    trees[2] = [-1] + [(i - 1) // 2 * 2 for i in range(1, 16)]  # a caterpillar over key 128
    c = Call(MAX_SEQ, ITEMS, H, KV, hd, seed=3 * hd + H, gap=2).device(acc)
    nodes = node_table(c, trees)
    ref = tree_reference(c, trees)
    nh = 2 if c.n_rep % 2 == 0 else 1
    base = {}
    for rule, name in ((rt.default_keys, "default rule"), (KEYS128, "128-key ranges")):
        tab = rt.ranges(c.segs, c.tiles, rule)
        out, sums = tv_launch(acc, etab, c, tab, nh, nodes)
        check_against(c, out, ref, f"tree masks hd {hd} n_rep {c.n_rep} {name}")
        base[name] = out, sums
        if nh == 2:
            o1, s1 = tv_launch(acc, etab, c, tab, 1, nodes)
            parity.exact(o1, out, f"hd {hd} {name}: one-head kernels against the two-head kernels, outputs")
            parity.exact(s1, sums, f"hd {hd} {name}: one-head kernels against the two-head kernels, sums")
    c.check_caches_untouched(f"tree masks hd {hd}")
    # NaN in K and V past pos + len: no bit changes
    d = Call(MAX_SEQ, ITEMS, H, KV, hd, seed=3 * hd + H, gap=2).device(acc, "nan")
    # NaN in the K of one node's slot per segment (its V stays finite: the contract): the nodes that do not see it keep their bits
    hit = [int(rng.integers(1, n)) for _, _, n in ITEMS]
    kc, vt = d.caches("nan")
    for (r, p, n), x in zip(ITEMS, hit):
        kc[r, :, p + x] = NAN
    e = Call(MAX_SEQ, ITEMS, H, KV, hd, seed=3 * hd + H, gap=2)
    e.k_host, e.v_host = guarded(kc, B), guarded(vt, B)
    e.kb, e.vb, e.qb, e.segb = acc.to_device(e.k_host), acc.to_device(e.v_host), d.qb, d.segb
    for rule, name in ((rt.default_keys, "default rule"), (KEYS128, "128-key ranges")):
        tab = rt.ranges(c.segs, c.tiles, rule)
        out, sums = base[name]
        o, s = tv_launch(acc, etab, d, tab, nh, nodes)
        parity.exact(o, out, f"hd {hd} {name}: outputs with NaN behind the keys")
        parity.exact(s, sums, f"hd {hd} {name}: sums with NaN behind the keys")
        o, _ = tv_launch(acc, etab, e, tab, nh, nodes)
        kept = 0
        for i, ((_, _, n), x) in enumerate(zip(ITEMS, hit)):
            masks = tr.anc_masks(trees[i])
            keep = [j for j in range(n) if not (masks[j] >> x) & 1]
            kept += len(keep)
            parity.exact(e.rows_of(o, i)[keep], c.rows_of(out, i)[keep], f"hd {hd} {name}: segment {i}, NaN in node {x}'s K: nodes {keep}")
        assert kept >= 40, kept
    d.check_caches_untouched("NaN behind the keys")


# ------------------------------------------------------------------------------------------ rope + cache write
def rope_launch(acc, rc, name, rows, segs, nodes=None, splits=0):
    """mc_tv_rope_cache* / mc_pp_rope_cache* over `rows` with the segment table `segs`"""
    import metalchat_amd as mc

    H, KV, hd, M = rc.H, rc.KV, rc.hd, rc.M
    kb, vb = acc.to_device(guarded(rc.kc0, B)), acc.to_device(guarded(rc.vt0, B))
    q0 = pattern((M + 16) * H * hd)
    qo = acc.to_device(q0)
    u32 = np.uint32
    args = ([acc.to_device(np.ascontiguousarray(rows).reshape(-1))] + ([u32(splits)] if splits else []) +
            [u32(M), qo, acc.to_device(rt.words(segs, 4).reshape(-1)), u32(len(segs)), kb, vb, np.uint64(rc.cstride), rc.cb, rc.sb, u32(H),
             u32(KV), u32(hd), u32(ROPE_S)] + ([acc.to_device(nodes)] if nodes is not None else []))
    mc.KernelTask(acc.load(name), (rc.gx * 256, 1, 1), (256, 1, 1), args)()
    acc.wait()
    q = qo.download(np.uint16, q0.size).reshape(M + 16, H, hd)
    parity.exact(q[M:], q0.reshape(M + 16, H, hd)[M:], "q rows past M")
    return q[:M], kb.download(np.uint16, B * rc.cstride).reshape(B, rc.cstride), vb.download(np.uint16, B * rc.cstride).reshape(B, rc.cstride)


@pytest.mark.parametrize("H,KV,hd", [(16, 4, 64), (32, 2, 128)])
def test_tv_rope_cache_ropes_at_depth_and_writes_at_the_node_index(acc, H, KV, hd):
    rc = RopeCase(acc, H, KV, hd)                # segments of 2, 17, 5 and 33 rows: the rope launch knows no 16-node limit
    rng = np.random.default_rng(hd + KV)
    trees = [random_tree(n, rng) for _, _, _, n in rc.segs]
    depth = []
    for t in trees:                              # (not tree_rule.depths: it refuses more than 16 nodes, as the entry point does)
        d = [0] * len(t)
        for i in range(1, len(t)):
            d[i] = d[t[i]] + 1
        depth.append(d)
    depth = np.concatenate(depth)
    assert depth.max() > 3 and np.any(depth < np.concatenate([np.arange(len(t)) for t in trees]))   # some node off the chain
    nodes = np.stack([depth, np.zeros_like(depth)], axis=1).astype(np.int32).reshape(-1)   # (the rope reads depth alone)
    x = bf(rng.normal(0, 1, (rc.M, rc.NQ)))
    # expected: RopeCase.expect's arithmetic (the oracle's rope) at table row pos + depth, written to slot pos + i
    q = np.zeros((rc.M, H, hd), np.uint16)
    kc, vt = rc.kc0.copy(), rc.vt0.copy()
    for r in range(rc.M):
        row, slot = rc.slot(r)
        at = slot - (r - next(off for _, _, off, n in rc.segs if off <= r < off + n)) + int(depth[r])
        qn, kn, vn = rc.split_row(x[r])
        q[r] = rc.rope(qn, H, at)
        kc[row, :, slot] = rc.rope(kn, KV, at)
        vt[row, :, :, slot] = vn
    exp = q, guarded(kc, B).reshape(B, -1), guarded(vt, B).reshape(B, -1)
    got = rope_launch(acc, rc, "mc_tv_rope_cache_bfloat", x, rc.segs, nodes)
    for g, e, name in zip(got, exp, ("q rows", "K caches (every row, guards included)", "V caches (every row, guards included)")):
        parity.exact(g, e, f"mc_tv_rope_cache H {H} KV {KV} hd {hd}: {name}")
    # the q rows of mc_pp_rope_cache over the same rows, each a segment of its own at pos + depth (its cache writes collide: not compared)
    each = [(rc.slot(r)[0], rc.slot(r)[1] - (r - off) + int(depth[r]), r, 1) for _, _, off, n in rc.segs for r in range(off, off + n)]
    parity.exact(rope_launch(acc, rc, "mc_pp_rope_cache_bfloat", x, each)[0], got[0], f"mc_tv_rope_cache hd {hd}: q rows against mc_pp_rope_cache at pos + depth")
    # the parts form: parts that sum exactly -> the plain kernel on T(sum)
    for splits in (2, 5):
        parts = (rng.integers(-64, 65, (splits, rc.M, rc.NQ)) / 64.0).astype(np.float32)
        xs = bf(parts.sum(axis=0, dtype=np.float64).astype(np.float32))
        a, b_ = rope_launch(acc, rc, "mc_tv_rope_cache_parts_bfloat", parts, rc.segs, nodes, splits), rope_launch(acc, rc, "mc_tv_rope_cache_bfloat", xs, rc.segs, nodes)
        for g, e, name in zip(a, b_, ("q rows", "K caches", "V caches")):
            parity.exact(g, e, f"mc_tv_rope_cache_parts splits {splits} hd {hd}: {name} against the plain kernel on T(sum)")
    # a chain tree is the packed pass's launch
    chain = np.stack([np.concatenate([np.arange(n) for _, _, _, n in rc.segs]), np.zeros(rc.M, np.int64)], axis=1).astype(np.int32).reshape(-1)
    for g, e, name in zip(rope_launch(acc, rc, "mc_tv_rope_cache_bfloat", x, rc.segs, chain), rope_launch(acc, rc, "mc_pp_rope_cache_bfloat", x, rc.segs),
                          ("q rows", "K caches", "V caches")):
        parity.exact(g, e, f"mc_tv_rope_cache hd {hd} chain: {name} against mc_pp_rope_cache")


# ------------------------------------------------------------------------------------------ acceptance
ACCEPT_CASES = [([16] * 8, 2056), ([2, 0, 16, 5, 0, 9, 3, 0], 2056), ([0, 0, 0, 7], 128256), ([4, 8, 16, 2, 3, 16, 11, 6], 4096), ([2], 2048)]


@pytest.mark.parametrize("lens,vocab", ACCEPT_CASES)
def test_tv_accept_against_the_rule(acc, lens, vocab):
    import metalchat_amd as mc

    nb = len(lens)
    rng = np.random.default_rng(sum(lens) + vocab)
    segs = rt.segments(lens, [int(p) for p in rng.integers(0, 100, nb)])
    M = sum(lens)
    depths_seen = set()
    for trial in range(5):
        tokens = rng.integers(0, vocab, M).astype(np.int32)
        picks = rng.integers(0, vocab, M).astype(np.int32)
        toks, pars, prow = [None] * nb, [None] * nb, [None] * nb
        nodes = np.zeros((M, 2), np.int64)
        for row, _, off, n in segs:
            par = list(tr.chain(n)) if trial == 0 else random_tree(n, rng)
            kids = [[j for j in range(n) if par[j] == i] for i in range(n)]
            # a path to follow: from the root to a random child while there is one, stopped early at random (trial 0: to the end);
            # the pick after each of its nodes is the next node's token -- and a sibling in front of it may carry the same token
            # (the lower index wins), a sibling behind it always does (it must lose), a node under a rejected sibling matches, too
            cur = 0
            while kids[cur] and (trial == 0 or rng.integers(0, 4)):
                nxt = kids[cur][int(rng.integers(0, len(kids[cur])))]
                picks[off + cur] = tokens[off + nxt]
                for sib in kids[cur]:
                    if sib > nxt or (sib < nxt and rng.integers(0, 3) == 0):
                        tokens[off + sib] = tokens[off + nxt]
                    for g in kids[sib]:
                        if sib != nxt and rng.integers(0, 2):
                            tokens[off + g] = picks[off + sib]
                cur = min(s for s in kids[cur] if tokens[off + s] == tokens[off + nxt])
            toks[row], pars[row], prow[row] = tokens[off:off + n].copy(), par, picks[off:off + n].copy()
            nodes[off:off + n, 0], nodes[off:off + n, 1] = tr.depths(par), tr.anc_masks(par)
        exp_acc, exp_next, exp_paths = tr.walk_rows(toks, pars, prow)
        depths_seen |= set(int(a) for a in exp_acc if a >= 0)
        logits = rng.integers(0, 0x7F80, (M, vocab)).astype(np.uint16)
        ab, nxb = acc.to_device(np.full(nb + 2, -1, np.int32)), acc.to_device(np.full(nb + 2, -1, np.int32))
        pb = acc.to_device(np.full((nb + 1) * 16, -7, np.int32))
        lo = acc.to_device(np.full((nb + 1) * vocab, NAN, np.uint16))
        gx = min(64, (vocab // 8 + 255) // 256)
        mc.KernelTask(acc.load("mc_tv_accept"), (gx * 256, len(segs), 1), (256, 1, 1),
                      [acc.to_device(rt.words(segs, 4).reshape(-1)), acc.to_device(tokens), acc.to_device(nodes.astype(np.uint32).view(np.int32).reshape(-1)),
                       acc.to_device(picks), acc.to_device(logits.reshape(-1)), np.uint32(vocab), ab, nxb, pb, lo])()
        acc.wait()
        what = f"mc_tv_accept lens {lens} vocab {vocab} trial {trial}"
        parity.exact(ab.download(np.int32, nb + 2), np.concatenate([exp_acc, [-1, -1]]).astype(np.int32), f"{what}: accepted")
        parity.exact(nxb.download(np.int32, nb + 2), np.concatenate([exp_next, [-1, -1]]).astype(np.int32), f"{what}: next tokens")
        paths = pb.download(np.int32, (nb + 1) * 16).reshape(nb + 1, 16)
        got = lo.download(np.uint16, (nb + 1) * vocab).reshape(nb + 1, vocab)
        for row, _, off, n in segs:
            parity.exact(paths[row], exp_paths[row], f"{what}: row {row}'s path")
            last = int(exp_paths[row][exp_acc[row]])
            parity.exact(got[row], logits[off + last], f"{what}: row {row}'s logits are those of node {last}")
        for r in range(nb + 1):
            if r >= nb or lens[r] == 0:
                assert np.all(got[r] == NAN) and np.all(paths[r] == -7), f"{what}: row {r} written"
    assert len(depths_seen) >= (2 if max(lens) > 2 else 1), depths_seen


# ------------------------------------------------------------------------------------------ compaction
@pytest.mark.parametrize("hd,KV", [(64, 4), (128, 2), (128, 3)])
def test_tv_compact_moves_the_accepted_path_and_nothing_else(acc, hd, KV):
    import metalchat_amd as mc

    L, S = 2, 200
    # (batch row, pos, nodes, path): a chain (nothing moves), paths with gaps, the last cache slot, a one-node path, a row outside
    rows = [(0, 5, 16, [0, 1, 2, 3]), (1, 63, 16, [0, 2, 3, 9, 15]), (2, S - 16, 16, [0, 15]), (4, 0, 7, [0, 3, 4, 6]), (5, 120, 2, [0]),
            (6, 30, 16, list(range(16))), (7, 100, 12, [0, 5, 6, 7, 8, 9, 10, 11])]
    lens, pos = [0] * B, [0] * B
    accepted, paths = np.full(B, -1, np.int32), np.full((B, 16), -1, np.int32)
    for r, p, n, path in rows:
        lens[r], pos[r], accepted[r] = n, p, len(path) - 1
        paths[r, :len(path)] = path
    segs = rt.segments(lens, pos)
    cstride = KV * S * hd + GUARD
    rng = np.random.default_rng(hd + KV)
    kc = rng.integers(0, 0x7F80, (L, B, KV, S, hd)).astype(np.uint16)     # finite patterns, every element its own
    vt = rng.integers(0, 0x7F80, (L, B, KV, hd, S)).astype(np.uint16)
    k_host = np.concatenate([guarded(kc[l], B) for l in range(L)])
    v_host = np.concatenate([guarded(vt[l], B) for l in range(L)])
    kb, vb = acc.to_device(k_host), acc.to_device(v_host)
    mc.KernelTask(acc.load("mc_tv_compact_bfloat"), ((KV * hd + 255) // 256 * 256, len(segs), L), (256, 1, 1),
                  [acc.to_device(rt.words(segs, 4).reshape(-1)), acc.to_device(accepted), acc.to_device(paths.reshape(-1)), kb, vb,
                   np.uint64(cstride), np.uint32(B), np.uint32(KV), np.uint32(hd), np.uint32(S)])()
    acc.wait()
    ke, ve = kc.copy(), vt.copy()
    for r, p, n, path in rows:
        for l in range(L):
            ke[l, r] = tr.compact(kc[l, r].transpose(1, 0, 2), p, path).transpose(1, 0, 2)       # slots first
            ve[l, r] = tr.compact(vt[l, r].transpose(2, 0, 1), p, path).transpose(1, 2, 0)
    assert not np.array_equal(ke, kc) and np.array_equal(ke[:, 6], kc[:, 6]) and np.array_equal(ke[:, 3], kc[:, 3])
    parity.exact(kb.download(np.uint16, k_host.size), np.concatenate([guarded(ke[l], B) for l in range(L)]), f"mc_tv_compact hd {hd} KV {KV}: K, all layers, rows and guards")
    parity.exact(vb.download(np.uint16, v_host.size), np.concatenate([guarded(ve[l], B) for l in range(L)]), f"mc_tv_compact hd {hd} KV {KV}: V, all layers, rows and guards")
