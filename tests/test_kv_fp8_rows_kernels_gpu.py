"""The packed passes' kernels on fp8 KV caches (kernels/kv8_rows_kernels.hip; Part 2p), launched BY NAME with test_rows_kernels_gpu.py's tables,
buffers and references.  Every check is bit for bit (tests/kv_fp8_rule.py): the write against quant of what mc_pp_rope_cache{,_parts}_bfloat stores,
the attention against the bfloat16 kernel of the same name on planes holding deq of the same bytes, and so against the float64 oracle under
check_against's tolerances.  Slots at and past pos + len hold NaN bytes (0x7f) under exponent -128, zeros in the bfloat16 planes."""
import numpy as np
import pytest

import kv_fp8_rule as kr
import parity
import rows_tables as rt
import test_rows_kernels_gpu as rk
from test_kv_fp8_kernels_gpu import G, guarded8, task

pytestmark = pytest.mark.gpu
etab = rk.etab
B = rk.B
u32, u64 = np.uint32, np.uint64

# chunk lengths 2, 16, 17 at pos 0, 37 and 95: S % 8 != 0, diagonal blocks, tiles of 1 and 16 rows, keys up to 112 of max_seq
ITEMS = [(0, 0, 2), (1, 37, 16), (2, 95, 17), (4, 0, 17), (5, 37, 2), (6, 95, 16), (7, 37, 17)]
# hd, H, KV: n_rep 1 and 4; max_seq 128 and 120 (no multiple of 32: the lanes of block 3's last lane group load V clamped at max_seq - 8)
# (H = 32: check_against counts the elements of one chunk row, as the bfloat16 tests' shapes say)
SHAPES = [(64, 32, 32, 128), (64, 32, 8, 128), (128, 32, 32, 128), (128, 32, 8, 128), (128, 32, 8, 120), (64, 32, 8, 120)]


class Call8(rk.Call):
    """rk.Call whose keys and values are deq(quant(.)), with the four fp8 planes of the same content beside the bfloat16 caches"""

    def __init__(self, max_seq, H, KV, hd):
        super().__init__(max_seq, ITEMS, H, KV, hd, seed=hd + H + max_seq)
        S = max_seq
        self.planes = [np.full((B, KV, S, hd), 0x7F, np.uint8), np.full((B, KV, hd, S), 0x7F, np.uint8),
                       np.full((B, KV, S), 0x80, np.uint8), np.full((B, KV, S), 0x80, np.uint8)]   # K, Vt, kexp, vexp (0x80 = -128)
        kq, vq, kx, vx = self.planes
        for i, (r, p, n) in enumerate(ITEMS):
            (kb, ke), (vb, ve) = kr.quant(self.k[i]), kr.quant(self.v[i])
            self.k[i], self.v[i] = kr.deq(kb, ke), kr.deq(vb, ve)
            kq[r, :, :p + n], kx[r, :, :p + n] = kb.transpose(1, 0, 2), ke.T.view(np.uint8)
            vq[r, :, :, :p + n], vx[r, :, :p + n] = vb.transpose(1, 2, 0), ve.T.view(np.uint8)
        self.bstride, self.xstride = KV * S * hd + G, KV * S + G

    def device(self, acc):
        super().device(acc)
        self.host8 = [guarded8(p.reshape(B, -1)).reshape(-1) for p in self.planes]
        self.kq, self.vq, self.kx, self.vx = (acc.to_device(h) for h in self.host8)
        return self


def planes(c, v=True):
    """the byte and exponent planes and their strides as every attention kernel here takes them (K only: mc_px8_sums)"""
    return ([c.kq, c.vq, c.kx, c.vx] if v else [c.kq, c.kx]) + [u64(c.bstride), u64(c.xstride)]


def px8_launch(acc, etab, c, tab, nh):
    """mc_px8_sums, mc_px8_pv and mc_px_reduce over one launch group, as prefill.cc launches them on an fp8 batch"""
    H, hd, sfx = c.H, c.hd, f"{'2' if nh == 2 else ''}_bfloat_hd{c.hd}"
    tabb = acc.to_device(rt.words(tab, 8).reshape(-1))
    sumsb = acc.to_device(np.full(len(tab) * H * 16, np.nan, np.float32))
    partb = acc.to_device(np.full(len(tab) * H * 16 * hd, np.nan, np.float32))
    outb = acc.to_device(rk.pattern(c.rows_buf * H * hd))
    grid, head, tail = (H // nh * 256, len(tab), 1), [c.qb, c.segb, tabb, u32(0)], [u32(H), u32(c.n_rep), u32(c.max_seq), c.scale, etab]
    task(acc, "mc_px8_sums" + sfx, grid, (256, 1, 1), head + planes(c, False) + [sumsb] + tail)
    task(acc, "mc_px8_pv" + sfx, grid, (256, 1, 1), head + planes(c) + [sumsb, partb, outb] + tail)
    if any(e[5] > 1 for e in tab):
        task(acc, rk.PX_REDUCE[hd], (H * 256, len(tab), 1), (256, 1, 1), [c.segb, tabb, u32(0), partb, outb, u32(H)])
    return outb.download(np.uint16, c.rows_buf * H * hd).reshape(c.rows_buf, H, hd), sumsb.download(np.float32, len(tab) * H * 16).reshape(len(tab), H, 16)


def pp8_launch(acc, etab, c, nh):
    H, hd = c.H, c.hd
    outb = acc.to_device(rk.pattern(c.rows_buf * H * hd))
    task(acc, f"mc_pp8_attn{'2' if nh == 2 else ''}_bfloat_hd{hd}", (len(c.tiles) * 256, H // nh, 1), (256, 1, 1),
         [c.qb, c.segb, acc.to_device(rt.words(c.tiles, 2).reshape(-1))] + planes(c) + [outb, u32(H), u32(c.n_rep), u32(c.max_seq), c.scale, etab])
    return outb.download(np.uint16, c.rows_buf * H * hd).reshape(c.rows_buf, H, hd)


def split3(c, tab):
    """the hand-made table: the first tile of the segment at pos 95, len 17 (111 keys) in the ranges [0, 32), [32, 96), [96, 111)"""
    si = next(i for i, g in enumerate(c.segs) if g[1] == 95 and g[3] == 17)
    at = next(j for j, e in enumerate(tab) if e[0] == si and e[1] == 0)
    assert tab[at][2:6] == (0, 111, at, 1)
    cut = [(si, 0, lo, hi, at, 3, 0, 0) for lo, hi in ((0, 32), (32, 96), (96, 111))]
    return tab[:at] + cut + [e[:4] + (e[4] + 2,) + e[5:] for e in tab[at + 1:]]


@pytest.mark.parametrize("hd,H,KV,max_seq", SHAPES)
def test_attention_on_bytes_is_the_bfloat16_attention_on_deq(acc, etab, hd, H, KV, max_seq):
    c = Call8(max_seq, H, KV, hd).device(acc)
    px_ref, pp_ref = rk.px_reference(c), rk.pp_reference(c)
    one = rt.ranges(c.segs, c.tiles, rk.NO_SPLIT)
    for nh in ((1, 2) if c.n_rep % 2 == 0 else (1,)):
        what = f"hd {hd} n_rep {c.n_rep} max_seq {max_seq} heads {nh}"
        for tab, name in ((one, "one range a tile"), (split3(c, one), "a tile in 3 ranges")):
            (want, wsums), (got, gsums) = rk.px_launch(acc, etab, c, tab, rk.one_group(tab), nh), px8_launch(acc, etab, c, tab, nh)
            parity.exact(gsums, wsums, f"px8 {what} {name}: sums against the bfloat16 kernel on deq")
            parity.exact(got, want, f"px8 {what} {name}: outputs against the bfloat16 kernel on deq")
            rk.check_against(c, got, px_ref, f"px8 {what} {name}")
        got = pp8_launch(acc, etab, c, nh)
        parity.exact(got, rk.pp_launch(acc, etab, c, nh), f"pp8 {what}: against the bfloat16 kernel on deq")
        rk.check_against(c, got, pp_ref, f"pp8 {what}")
    for b_, h, name in zip((c.kq, c.vq, c.kx, c.vx), c.host8, ("K bytes", "V bytes", "kexp", "vexp")):
        parity.exact(b_.download(np.uint8, h.size), h, f"hd {hd}: {name} and guards are untouched")


# ------------------------------------------------------------------------------------------ rope + cache write
# lengths 2 and 17; packed rows 0 .. 15 are one V tile over two segments; the segment at row 6 carries a zero V vector
ROPE_ITEMS = [(1, 0, 2), (3, 63, 17), (6, 100, 4)]


@pytest.mark.parametrize("H,KV,hd", [(4, 2, 64), (8, 2, 128)])
@pytest.mark.parametrize("splits", [0, 3])
def test_pp8_rope_cache_writes_the_rule_of_the_bfloat16_write(acc, monkeypatch, H, KV, hd, splits):
    monkeypatch.setattr(rk, "ROPE_ITEMS", ROPE_ITEMS)
    rc = rk.RopeCase(acc, H, KV, hd)
    M, S, NQ = rc.M, rk.ROPE_S, rc.NQ
    rng = np.random.default_rng(hd + splits)
    if splits:   # parts whose sum is exact in fp32 in any order (test_pp_rope_cache_parts_sums_in_front_of_the_rope)
        rows = (rng.integers(-64, 65, (splits, M, NQ)) / 64.0 * np.exp2(rng.integers(-4, 5, (1, M, 1)))).astype(np.float32)
        rows[:, M - 2, (H + KV) * hd:(H + KV + 1) * hd] = 0
    else:
        rows = rk.bf(rng.normal(0, 1, (M, NQ)) * np.exp2(rng.integers(-4, 5, (M, 1))))
        rows[M - 2, (H + KV) * hd:(H + KV + 1) * hd] = 0                   # kv head 0's V of one row: exponent -100
    q_ref, kc, vt = rc.launch(acc, rows, splits)
    kc, vt = (x[:, :KV * S * hd] for x in (kc, vt))
    init = [rng.integers(0, 256, (B, n), dtype=np.uint8) for n in (KV * S * hd, KV * S * hd, KV * S, KV * S)]
    bufs = [acc.to_device(guarded8(p).reshape(-1)) for p in init]
    q0 = rk.pattern((M + 16) * H * hd)
    qo = acc.to_device(q0)
    rb = acc.to_device(np.ascontiguousarray(rows).reshape(-1))
    tail = [qo, rc.segb, u32(len(rc.segs))] + bufs + [u64(KV * S * hd + G), u64(KV * S + G), rc.cb, rc.sb, u32(H), u32(KV), u32(hd), u32(S)]
    task(acc, "mc_pp8_rope_cache_parts_bfloat" if splits else "mc_pp8_rope_cache_bfloat", (rc.gx * 256, 1, 1), (256, 1, 1),
         ([rb, u32(splits), u32(M)] if splits else [rb, u32(M)]) + tail)
    q = qo.download(np.uint16, q0.size).reshape(M + 16, H, hd)
    parity.exact(q, np.concatenate([q_ref, q0.reshape(M + 16, H, hd)[M:]]), "q rows are the bfloat16 kernel's, the rows past M untouched")
    exp = [guarded8(p) for p in init]                                      # the initial bytes with exactly the call's slots replaced
    for r in range(M):
        row, slot = rc.slot(r)
        kb, ke = kr.quant(kc[row].reshape(KV, S, hd)[:, slot])
        vb, ve = kr.quant(vt[row].reshape(KV, hd, S)[:, :, slot])
        exp[0][row, :KV * S * hd].reshape(KV, S, hd)[:, slot] = kb
        exp[1][row, :KV * S * hd].reshape(KV, hd, S)[:, :, slot] = vb
        exp[2][row, :KV * S].reshape(KV, S)[:, slot] = ke.view(np.uint8)
        exp[3][row, :KV * S].reshape(KV, S)[:, slot] = ve.view(np.uint8)
    row, slot = rc.slot(M - 2)
    assert exp[3][row, :KV * S].reshape(KV, S)[0, slot] == np.uint8(256 + kr.E_MIN) and len({rc.slot(r)[0] for r in range(16)}) == 2
    for b_, e, name in zip(bufs, exp, ("K bytes", "V bytes", "kexp", "vexp")):
        parity.exact(b_.download(np.uint8, e.size).reshape(e.shape), e, f"H {H} hd {hd} splits {splits}: {name} (the chunks' slots, nothing else, the guards)")
