"""The tree kernels on fp8 KV caches (kernels/kv8_tree_kernels.hip; Part 2q), launched BY NAME with the tables, buffers and launches of
test_kv_fp8_rows_kernels_gpu.py and test_tree_kernels_gpu.py.  Every check is bit for bit (tests/kv_fp8_rule.py): the attention against the bfloat16
tree kernels on planes holding deq of the same bytes, the write against quant of what mc_tv_rope_cache{,_parts}_bfloat stores, the compaction against
mc_tv_compact_bfloat on deq of the planes.  Two segments a launch, a branching tree of 16 nodes and one of 5; slots at and past pos + len hold NaN
bytes (0x7f) under exponent -128.  pos 27: the nodes' slots 27 .. 42 cross a 32-key block; pos 104 at max_seq 120: the tile ends at the cache's
end, on the V load that is clamped at max_seq - 8 (at max_seq 128 nothing is clamped)."""
import itertools

import numpy as np
import pytest

import kv_fp8_rule as kr
import parity
import rows_tables as rt
import test_kv_fp8_rows_kernels_gpu as r8
import test_rows_kernels_gpu as rk
import test_tree_kernels_gpu as tk
import tree_rule as tr
from test_batch_kernels_gpu import GUARD, bf, guarded
from test_kv_fp8_kernels_gpu import G, guarded8, task

pytestmark = pytest.mark.gpu
etab = rk.etab
B = rk.B
u32, u64 = np.uint32, np.uint64
TREE16 = [-1, 0, 0, 1, 1, 2, 2, 3, 5, 5, 8, 5, 11, 0, 13, 11]   # branching; 0 -> 2 -> 5 -> 11 is a path off the first chain
TREE5 = [-1, 0, 0, 1, 3]
PATH = [0, 2, 5, 11]
assert tr.ancestors(TREE16, 11) == PATH


def tv8_launch(acc, etab, c, tab, nh, nodes):
    """mc_tv8_sums, mc_tv8_pv and mc_px_reduce over one launch group, as prefill.cc launches them for a tree call on an fp8 batch"""
    H, hd, sfx = c.H, c.hd, f"{'2' if nh == 2 else ''}_bfloat_hd{c.hd}"
    tabb = acc.to_device(rt.words(tab, 8).reshape(-1))
    sumsb = acc.to_device(np.full(len(tab) * H * 16, np.nan, np.float32))
    partb = acc.to_device(np.full(len(tab) * H * 16 * hd, np.nan, np.float32))
    outb = acc.to_device(rk.pattern(c.rows_buf * H * hd))
    grid, head = (H // nh * 256, len(tab), 1), [c.qb, c.segb, tabb, u32(0)]
    tail = [u32(H), u32(c.n_rep), u32(c.max_seq), c.scale, etab, acc.to_device(nodes)]
    task(acc, "mc_tv8_sums" + sfx, grid, (256, 1, 1), head + r8.planes(c, False) + [sumsb] + tail)
    task(acc, "mc_tv8_pv" + sfx, grid, (256, 1, 1), head + r8.planes(c) + [sumsb, partb, outb] + tail)
    if any(e[5] > 1 for e in tab):
        task(acc, rk.PX_REDUCE[hd], (H * 256, len(tab), 1), (256, 1, 1), [c.segb, tabb, u32(0), partb, outb, u32(H)])
    return outb.download(np.uint16, c.rows_buf * H * hd).reshape(c.rows_buf, H, hd), sumsb.download(np.float32, len(tab) * H * 16).reshape(len(tab), H, 16)


def split_at_32(tab):
    """every tile with keys past 32 in the two ranges [0, 32), [32, S): partial outputs and mc_px_reduce, the nodes' slots in both"""
    out = []
    for seg, r0, lo, hi, _, _, a, b_ in tab:
        cuts = [(lo, 32), (32, hi)] if hi > 32 else [(lo, hi)]
        out += [(seg, r0, l, h, len(out), len(cuts), a, b_) for l, h in cuts]
    return out


@pytest.mark.parametrize("max_seq,pos", [(128, 27), (120, 27), (120, 104)])
@pytest.mark.parametrize("hd,nh", itertools.product((64, 128), (1, 2)))
def test_tree_attention_on_bytes_is_the_bfloat16_tree_attention_on_deq(acc, etab, monkeypatch, hd, nh, max_seq, pos):
    monkeypatch.setattr(r8, "ITEMS", [(1, pos, 16), (4, pos, 5)])
    c = r8.Call8(max_seq, 8, 2, hd).device(acc)
    nodes = tk.node_table(c, [TREE16, TREE5])
    one = rt.ranges(c.segs, c.tiles, rk.NO_SPLIT)
    assert [e[3] for e in one] == [pos + 16, pos + 5]
    for tab, name in ((one, "one range a tile"), (split_at_32(one), "tiles cut at key 32")):
        what = f"tv8 hd {hd} heads {nh} max_seq {max_seq} pos {pos} {name}"
        (want, wsums), (got, gsums) = tk.tv_launch(acc, etab, c, tab, nh, nodes), tv8_launch(acc, etab, c, tab, nh, nodes)
        parity.exact(gsums, wsums, f"{what}: sums against the bfloat16 kernel on deq")
        parity.exact(got, want, f"{what}: outputs against the bfloat16 kernel on deq")
    for b_, h, name in zip((c.kq, c.vq, c.kx, c.vx), c.host8, ("K bytes", "V bytes", "kexp", "vexp")):
        parity.exact(b_.download(np.uint8, h.size), h, f"hd {hd}: {name} and guards are untouched")


# ------------------------------------------------------------------------------------------ rope + cache write
@pytest.mark.parametrize("H,KV,hd", [(4, 2, 64), (8, 2, 128)])
@pytest.mark.parametrize("splits", [0, 3])
def test_tv8_rope_cache_writes_the_rule_of_the_bfloat16_tree_write(acc, monkeypatch, H, KV, hd, splits):
    monkeypatch.setattr(rk, "ROPE_ITEMS", [(1, 27, 16), (4, 104, 5)])   # packed rows 0 .. 15 and 16 .. 20: the second V tile holds 5 rows
    rc = rk.RopeCase(acc, H, KV, hd)
    M, S = rc.M, rk.ROPE_S
    nodes = np.stack([tr.depths(TREE16) + tr.depths(TREE5), tr.anc_masks(TREE16) + tr.anc_masks(TREE5)], axis=1).astype(np.int32).reshape(-1)
    rng = np.random.default_rng(hd + splits)
    if splits:   # parts whose sum is exact in fp32 in any order (test_pp_rope_cache_parts_sums_in_front_of_the_rope)
        rows = (rng.integers(-64, 65, (splits, M, rc.NQ)) / 64.0 * np.exp2(rng.integers(-4, 5, (1, M, 1)))).astype(np.float32)
        rows[:, M - 2, (H + KV) * hd:(H + KV + 1) * hd] = 0
    else:
        rows = bf(rng.normal(0, 1, (M, rc.NQ)) * np.exp2(rng.integers(-4, 5, (M, 1))))
        rows[M - 2, (H + KV) * hd:(H + KV + 1) * hd] = 0                  # kv head 0's V of one node: exponent -100
    name = "mc_tv_rope_cache_parts_bfloat" if splits else "mc_tv_rope_cache_bfloat"
    q_ref, kc, vt = tk.rope_launch(acc, rc, name, rows, rc.segs, nodes, splits)
    kc, vt = (x[:, :KV * S * hd] for x in (kc, vt))
    init = [rng.integers(0, 256, (B, n), dtype=np.uint8) for n in (KV * S * hd, KV * S * hd, KV * S, KV * S)]
    bufs = [acc.to_device(guarded8(p).reshape(-1)) for p in init]
    q0 = rk.pattern((M + 16) * H * hd)
    qo = acc.to_device(q0)
    rb = acc.to_device(np.ascontiguousarray(rows).reshape(-1))
    tail = ([qo, rc.segb, u32(len(rc.segs))] + bufs + [u64(KV * S * hd + G), u64(KV * S + G), rc.cb, rc.sb, u32(H), u32(KV), u32(hd), u32(S),
                                                      acc.to_device(nodes)])
    task(acc, name.replace("mc_tv_", "mc_tv8_"), (rc.gx * 256, 1, 1), (256, 1, 1), ([rb, u32(splits), u32(M)] if splits else [rb, u32(M)]) + tail)
    q = qo.download(np.uint16, q0.size).reshape(M + 16, H, hd)
    parity.exact(q, np.concatenate([q_ref, q0.reshape(M + 16, H, hd)[M:]]), "q rows are the bfloat16 tree kernel's (rope row pos + depth), the rows past M untouched")
    exp = [guarded8(p) for p in init]                                     # the initial bytes with exactly the nodes' slots pos + i replaced
    for r in range(M):
        row, slot = rc.slot(r)
        kb, ke = kr.quant(kc[row].reshape(KV, S, hd)[:, slot])
        vb, ve = kr.quant(vt[row].reshape(KV, hd, S)[:, :, slot])
        exp[0][row, :KV * S * hd].reshape(KV, S, hd)[:, slot] = kb
        exp[1][row, :KV * S * hd].reshape(KV, hd, S)[:, :, slot] = vb
        exp[2][row, :KV * S].reshape(KV, S)[:, slot] = ke.view(np.uint8)
        exp[3][row, :KV * S].reshape(KV, S)[:, slot] = ve.view(np.uint8)
    row, slot = rc.slot(M - 2)
    assert exp[3][row, :KV * S].reshape(KV, S)[0, slot] == np.uint8(256 + kr.E_MIN)
    for b_, e, what in zip(bufs, exp, ("K bytes", "V bytes", "kexp", "vexp")):
        parity.exact(b_.download(np.uint8, e.size).reshape(e.shape), e, f"H {H} hd {hd} splits {splits}: {what} (the nodes' slots, nothing else, the guards)")


# ------------------------------------------------------------------------------------------ compaction
@pytest.mark.parametrize("hd", [64, 128])
def test_tv8_compact_moves_bytes_and_exponents_along_the_path_and_nothing_else(acc, hd):
    L, S, KV = 2, 120, 2
    # (batch row, pos, nodes, path): the branching path, a chain up to the cache's last slots (nothing moves), nothing accepted
    rows = [(1, 27, 16, PATH), (4, 104, 16, [0, 1, 2, 3]), (6, 27, 5, [0])]
    lens, pos = [0] * B, [0] * B
    accepted, paths = np.full(B, -1, np.int32), np.full((B, 16), -1, np.int32)
    for r, p, n, path in rows:
        lens[r], pos[r], accepted[r] = n, p, len(path) - 1
        paths[r, :len(path)] = path
    segs = rt.segments(lens, pos)
    head = [acc.to_device(rt.words(segs, 4).reshape(-1)), acc.to_device(accepted), acc.to_device(paths.reshape(-1))]
    rng = np.random.default_rng(hd)
    (kb, ke), (vb, ve) = (kr.quant(bf(rng.normal(0, 1, (L, B, KV, S, hd)) * np.exp2(rng.integers(-6, 6, (L, B, KV, S, 1))))) for _ in range(2))
    before = [kb, vb.transpose(0, 1, 2, 4, 3), ke.view(np.uint8), ve.view(np.uint8)]     # K [KV][S][hd], V [KV][hd][S], exponents [KV][S]
    bufs = [acc.to_device(guarded8(np.ascontiguousarray(p).reshape(L * B, -1)).reshape(-1)) for p in before]
    owners = KV * hd // 16 + KV * hd + 2 * KV
    task(acc, "mc_tv8_compact", ((owners + 255) // 256 * 256, len(segs), L), (256, 1, 1),
         head + bufs + [u64(KV * S * hd + G), u64(KV * S + G), u32(B), u32(KV), u32(hd), u32(S)])
    after = [b_.download(np.uint8, L * B * (p[0, 0].size + G)).reshape(L * B, -1) for b_, p in zip(bufs, before)]
    # every byte and exponent, guards included: the rule on the planes as they lie (slots first)
    axes = [(1, 0, 2), (2, 0, 1), (1, 0), (1, 0)]
    exp = [np.array(p, copy=True) for p in before]
    for (r, p, n, path), l in itertools.product(rows, range(L)):
        for e, src, ax in zip(exp, before, axes):
            e[l, r] = tr.compact(src[l, r].transpose(ax), p, path).transpose(np.argsort(ax))
    assert not np.array_equal(exp[0], before[0]) and all(np.array_equal(e[:, [4, 6]], p[:, [4, 6]]) for e, p in zip(exp, before))
    for a, e, what in zip(after, exp, ("K bytes", "V bytes", "kexp", "vexp")):
        parity.exact(a, guarded8(e.reshape(L * B, -1)), f"mc_tv8_compact hd {hd}: {what}, all layers, rows and guards")
    # deq of the planes afterwards is mc_tv_compact_bfloat applied to deq of the planes before
    kd, vd = kr.deq(kb, ke), kr.deq(vb, ve).transpose(0, 1, 2, 4, 3)
    refs = [acc.to_device(np.concatenate([guarded(x[l], B) for l in range(L)])) for x in (kd, vd)]
    task(acc, "mc_tv_compact_bfloat", ((KV * hd + 255) // 256 * 256, len(segs), L), (256, 1, 1),
         head + refs + [u64(KV * S * hd + GUARD), u32(B), u32(KV), u32(hd), u32(S)])
    want = [x.download(np.uint16, L * B * (KV * S * hd + GUARD)).reshape(L * B, -1)[:, :KV * S * hd] for x in refs]
    ga, va, kxa, vxa = (a[:, :p[0, 0].size] for a, p in zip(after, before))
    parity.exact(kr.deq(ga.reshape(-1, S, hd), kxa.view(np.int8).reshape(-1, S)).reshape(L * B, -1), want[0], f"hd {hd}: deq of K against mc_tv_compact_bfloat on deq")
    got_v = kr.deq(va.reshape(-1, hd, S).transpose(0, 2, 1), vxa.view(np.int8).reshape(-1, S)).transpose(0, 2, 1)
    parity.exact(got_v.reshape(L * B, -1), want[1], f"hd {hd}: deq of V against mc_tv_compact_bfloat on deq")
