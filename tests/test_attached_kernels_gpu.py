"""Kernel-level parity of mc_ax_sums / mc_ax_pv (kernels/attached_kernels.hip, Part 2t): the attention of chunk tiles of rows attached to the
shared prefix, launched BY NAME on buffers the test owns -- the prefix planes hold the first 192 slots and NaN behind them, each row's own planes
NaN in [0, 192) and behind its keys -- against the oracle's attention over the logical cache (the bound of test_rows_kernels_gpu.check_against),
and bit for bit mc_px_* on rows that hold copies of the prefix, sums included, with nothing but the call's output rows written."""
import numpy as np
import pytest

import parity
import rows_tables as rt
from test_batch_kernels_gpu import NAN, bf, guarded
from test_rows_kernels_gpu import B, PX_REDUCE, Call, check_against, etab, one_group, pattern, px_launch, px_reference  # noqa: F401 (etab: a fixture)

pytestmark = pytest.mark.gpu
MAX_SEQ, SHARED, H = 256, 192, 32
ITEMS = [(0, 200, 16), (1, 230, 5), (2, 200, 20)]   # (batch row, pos, len): four tiles, the last of 4 rows


def forms(hd, n_rep):
    """abi.h ax_heads, ax_tiles"""
    nh = 4 if n_rep % 4 == 0 and 4 * hd <= 256 else 2 if n_rep % 2 == 0 and 2 * hd <= 256 else 1
    return nh, min(4, 192 // (nh * hd // 4))


def ax_launch(acc, etab, c, tab, kb, vb, pkb, pvb):
    """mc_ax_sums, mc_ax_pv and (a split tile) mc_px_reduce over one group of attached tiles, as prefill.cc launches them; the unit table by
    rows_plan.h's rule: the tiles T at a time, one entry per range ordinal.  Returns the output rows and the sums of every range"""
    import metalchat_amd as mc

    hd, u32 = c.hd, np.uint32
    nh, T = forms(hd, c.n_rep)
    firsts = [i for i, e in enumerate(tab) if e[4] == i]
    units = []
    for u in range(0, len(firsts), T):
        for k in range(max(tab[i][5] for i in firsts[u:u + T])):
            rs = [i + k for i in firsts[u:u + T] if k < tab[i][5]]
            units.append([len(rs)] + rs + [0] * (7 - len(rs)))
    tabb, unitb = acc.to_device(rt.words(tab, 8).reshape(-1)), acc.to_device(rt.words(units, 8).reshape(-1))
    sumsb = acc.to_device(np.full(len(tab) * H * 16, np.nan, np.float32))
    partb = acc.to_device(np.full(len(tab) * H * 16 * hd, np.nan, np.float32))
    out0 = pattern(c.rows_buf * H * hd)
    outb = acc.to_device(out0)
    grid, head = (H // nh * 256, len(units), 1), [c.qb, c.segb, tabb, unitb, u32(0), u32(0)]
    tail = [u32(H), u32(c.n_rep), u32(MAX_SEQ), u32(SHARED), c.scale, etab]
    mc.KernelTask(acc.load(f"mc_ax_sums_bfloat_hd{hd}"), grid, (256, 1, 1), head + [kb, pkb, np.uint64(c.cstride), sumsb] + tail)()
    mc.KernelTask(acc.load(f"mc_ax_pv_bfloat_hd{hd}"), grid, (256, 1, 1), head + [kb, vb, pkb, pvb, np.uint64(c.cstride), sumsb, partb, outb] + tail)()
    if any(e[5] > 1 for e in tab):
        mc.KernelTask(acc.load(PX_REDUCE[hd]), (H * 256, len(tab), 1), (256, 1, 1), [c.segb, tabb, u32(0), partb, outb, u32(H)])()
    acc.wait()
    return outb.download(np.uint16, out0.size).reshape(c.rows_buf, H, hd), sumsb.download(np.float32, len(tab) * H * 16).reshape(len(tab), H, 16)


@pytest.mark.parametrize("keys", [rt.keys_of(0), rt.keys_of(128)], ids=["one range", "128-key ranges"])
@pytest.mark.parametrize("hd,n_rep", [(64, 1), (64, 4), (128, 1), (128, 4)])
def test_attached_tiles_against_the_oracle_and_the_per_row_kernels(acc, etab, hd, n_rep, keys):
    KV = H // n_rep
    c = Call(MAX_SEQ, ITEMS, H, KV, hd, seed=hd + n_rep)
    rng = np.random.default_rng(hd * n_rep)
    pk, pv = bf(rng.normal(0, 0.4, (SHARED, KV, hd))), bf(rng.normal(0, 0.5, (SHARED, KV, hd)))
    for i in range(len(ITEMS)):   # every row's first 192 keys are the prefix's
        c.k[i][:SHARED], c.v[i][:SHARED] = pk, pv
    c.device(acc, "nan")          # the twin: rows that hold copies of the prefix
    tab = rt.ranges(c.segs, c.tiles, keys)
    assert [e[2:4] for e in tab[:2]] == ([(0, 128), (128, 216)] if len(tab) > 4 else [(0, 216), (0, 235)])
    want, want_sums = px_launch(acc, etab, c, tab, one_group(tab), 2 if n_rep % 2 == 0 else 1)
    # attached: the prefix planes, NaN at and behind `shared`; the rows' own planes, NaN in [0, shared) and behind their keys
    kc, vt = c.caches("nan")
    kc[:, :, :SHARED], vt[:, :, :, :SHARED] = NAN, NAN
    pkc, pvt = np.full((1, KV, MAX_SEQ, hd), NAN, np.uint16), np.full((1, KV, hd, MAX_SEQ), NAN, np.uint16)
    pkc[0, :, :SHARED], pvt[0, :, :, :SHARED] = pk.transpose(1, 0, 2), pv.transpose(1, 2, 0)
    host = [guarded(kc, B), guarded(vt, B), guarded(pkc, 1), guarded(pvt, 1)]
    dev = [acc.to_device(x) for x in host]
    got, got_sums = ax_launch(acc, etab, c, tab, *dev)
    what = f"hd {hd} n_rep {n_rep} {len(tab)} ranges"
    check_against(c, got, px_reference(c), what)
    parity.exact(got, want, f"{what}: outputs against mc_px_* on rows that hold copies (rows of no segment included)")
    parity.exact(got_sums, want_sums, f"{what}: sums against mc_px_sums")
    for d, h, name in zip(dev, host, ("K", "V", "prefix K", "prefix V")):
        parity.exact(d.download(np.uint16, h.size), h, f"{what}: {name} planes and guards untouched")
