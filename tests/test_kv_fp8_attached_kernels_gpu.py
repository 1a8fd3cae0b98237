"""Kernel-level parity of mc_ax8_sums / mc_ax8_pv (kernels/kv8_attached_kernels.hip, Part 2u), launched BY NAME at test_attached_kernels_gpu.py's
shapes on fp8 planes built with kv_fp8_rule.py.  Every slot no row owns -- the prefix planes from `shared` on, the rows' planes in [0, shared) and
behind their keys, rows outside the call -- holds a NaN byte (0x7f, 0xff in turn) under exponent -128."""
import numpy as np
import pytest

import kv_fp8_rule as kr
import parity
import rows_tables as rt
from test_attached_kernels_gpu import H, ITEMS, MAX_SEQ, SHARED, forms
from test_batch_kernels_gpu import bf
from test_kv_fp8_kernels_gpu import G, guarded8, task
from test_kv_fp8_rows_kernels_gpu import px8_launch
from test_rows_kernels_gpu import B, PX_REDUCE, Call, check_against, etab, pattern, px_reference  # noqa: F401 (etab: a fixture)

pytestmark = pytest.mark.gpu
u32, u64 = np.uint32, np.uint64


def unowned(c, rows):
    """K, Vt, kexp, vexp of `rows` rows in which no slot is owned"""
    nan8 = lambda *shape: np.where(np.arange(int(np.prod(shape))) % 2, 0xFF, 0x7F).astype(np.uint8).reshape(shape)
    return [nan8(rows, c.KV, c.max_seq, c.hd), nan8(rows, c.KV, c.hd, c.max_seq)] + [np.full((rows, c.KV, c.max_seq), 0x80, np.uint8) for _ in "kv"]


def fill(p, r, lo, hi, k, v):
    """the slots [lo, hi) of row r of the planes p from the quantised vectors k, v = (bytes [slot][KV][hd], exponents [slot][KV])"""
    p[0][r, :, lo:hi], p[2][r, :, lo:hi] = k[0][lo:hi].transpose(1, 0, 2), k[1][lo:hi].T.view(np.uint8)
    p[1][r, :, :, lo:hi], p[3][r, :, lo:hi] = v[0][lo:hi].transpose(1, 2, 0), v[1][lo:hi].T.view(np.uint8)


def upload(acc, p):
    host = [guarded8(x.reshape(x.shape[0], -1)).reshape(-1) for x in p]
    return host, [acc.to_device(h) for h in host]


def ax8_launch(acc, etab, c, tab, rows, prefix):
    """mc_ax8_sums, mc_ax8_pv and (a split tile) mc_px_reduce over one group of attached tiles, as prefill.cc launches them on an fp8 batch; the
    unit table by rows_plan.h's rule (test_attached_kernels_gpu.ax_launch).  Returns the output rows and the sums of every range"""
    hd, (nh, T), firsts, units = c.hd, forms(c.hd, c.n_rep), [i for i, e in enumerate(tab) if e[4] == i], []
    for u in range(0, len(firsts), T):
        for k in range(max(tab[i][5] for i in firsts[u:u + T])):
            rs = [i + k for i in firsts[u:u + T] if k < tab[i][5]]
            units.append([len(rs)] + rs + [0] * (7 - len(rs)))
    tabb, unitb = acc.to_device(rt.words(tab, 8).reshape(-1)), acc.to_device(rt.words(units, 8).reshape(-1))
    sumsb, partb = (acc.to_device(np.full(len(tab) * H * 16 * n, np.nan, np.float32)) for n in (1, hd))
    out0 = pattern(c.rows_buf * H * hd)
    outb = acc.to_device(out0)
    (kq, vq, kx, vx), (pkq, pvq, pkx, pvx) = rows, prefix
    grid, head, strides = (H // nh * 256, len(units), 1), [c.qb, c.segb, tabb, unitb, u32(0), u32(0)], [u64(c.bstride), u64(c.xstride)]
    tail = [u32(H), u32(c.n_rep), u32(MAX_SEQ), u32(SHARED), c.scale, etab]
    task(acc, f"mc_ax8_sums_bfloat_hd{hd}", grid, (256, 1, 1), head + [kq, kx, pkq, pkx] + strides + [sumsb] + tail)
    task(acc, f"mc_ax8_pv_bfloat_hd{hd}", grid, (256, 1, 1), head + [kq, vq, kx, vx, pkq, pvq, pkx, pvx] + strides + [sumsb, partb, outb] + tail)
    if any(e[5] > 1 for e in tab):
        task(acc, PX_REDUCE[hd], (H * 256, len(tab), 1), (256, 1, 1), [c.segb, tabb, u32(0), partb, outb, u32(H)])
    return outb.download(np.uint16, out0.size).reshape(c.rows_buf, H, hd), sumsb.download(np.float32, len(tab) * H * 16).reshape(len(tab), H, 16)


@pytest.mark.parametrize("keys", [rt.keys_of(0), rt.keys_of(128)], ids=["one range", "128-key ranges"])
@pytest.mark.parametrize("hd,n_rep", [(64, 1), (64, 4), (128, 1), (128, 4)])
def test_attached_fp8_tiles_against_the_oracle_and_the_per_row_kernels(acc, etab, hd, n_rep, keys):
    KV = H // n_rep
    c = Call(MAX_SEQ, ITEMS, H, KV, hd, seed=hd + n_rep)
    rng = np.random.default_rng(hd * n_rep)
    pk, pv = kr.quant(bf(rng.normal(0, 0.4, (SHARED, KV, hd)))), kr.quant(bf(rng.normal(0, 0.5, (SHARED, KV, hd))))
    twin, own, prefix = unowned(c, B), unowned(c, B), unowned(c, 1)
    fill(prefix, 0, 0, SHARED, pk, pv)
    for i, (r, p, n) in enumerate(ITEMS):   # every row's first 192 keys are the prefix's, byte for byte; the reference reads deq of the bytes
        k, v = kr.quant(c.k[i]), kr.quant(c.v[i])
        for q, pq in ((k, pk), (v, pv)):
            q[0][:SHARED], q[1][:SHARED] = pq
        c.k[i], c.v[i] = kr.deq(*k), kr.deq(*v)
        fill(twin, r, 0, p + n, k, v)
        fill(own, r, SHARED, p + n, k, v)
    c.qb, c.segb = acc.to_device(c.q_rows().reshape(-1)), acc.to_device(rt.words(c.segs, 4).reshape(-1))
    c.bstride, c.xstride = KV * MAX_SEQ * hd + G, KV * MAX_SEQ + G
    tab = rt.ranges(c.segs, c.tiles, keys)
    assert [e[2:4] for e in tab[:2]] == ([(0, 128), (128, 216)] if len(tab) > 4 else [(0, 216), (0, 235)])
    _, (c.kq, c.vq, c.kx, c.vx) = upload(acc, twin)   # the twin: rows that hold byte copies of the prefix
    want, want_sums = px8_launch(acc, etab, c, tab, 2 if n_rep % 2 == 0 else 1)
    (own_host, own_dev), (prefix_host, prefix_dev) = upload(acc, own), upload(acc, prefix)
    got, got_sums = ax8_launch(acc, etab, c, tab, own_dev, prefix_dev)
    what = f"hd {hd} n_rep {n_rep} {len(tab)} ranges"
    check_against(c, got, px_reference(c), what)   # the float64 attention over deq(quant(.))
    parity.exact(got, want, f"{what}: outputs against mc_px8_* on rows that hold byte copies (rows of no segment included)")
    parity.exact(got_sums, want_sums, f"{what}: sums against mc_px8_sums")
    for d, h in zip(own_dev + prefix_dev, own_host + prefix_host):
        parity.exact(d.download(np.uint8, h.size), h, f"{what}: the rows' and the prefix's K, V, kexp, vexp planes and guards untouched")
