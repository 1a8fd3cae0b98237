"""Kernel-level tests of the ONE-PROMPT attention (kernels/prefill_kernels.hip): all eleven names prefill.cc plan_attention may choose --
mc_pf_attn_bfloat_hd{32,64,128,256}, mc_pf_attn2_bfloat_hd{32,64,128}, mc_pf_attn4_bfloat_hd128 and the four LDS-tile kernels
mc_pf_attn8_bfloat_{hd128,hd64_h8,hd64_h4,hd256} -- launched BY NAME through the Part-1 seam on buffers the test owns, with the grid,
block and preconditions of pf_attn_rule.launch_shape, at 32 and 48 heads over 4 .. 32 kv heads (several kv heads per launch, n_rep larger
than a workgroup's heads), with and without a window, at chunks behind a context, and at caches that end inside a 64-key tile.

  A  per chunk row against the oracle's attention over the keys pf_attn_rule.visible gives (the reference's mask), with the bound of
     test_rows_kernels_gpu.check_against.  The oracle is the cost of this module, so a case compares a SELECTION of its rows (select_rows:
     the chunk's ends, the rows around every 32-row and 64-key edge and around the window, every 37th) and the references are shared
     between the kernels and cases of one (head_dim, H, KV): chunk row r always holds the same query and slot k the same key.  Every
     row of every case is still held to: finite; the LDS-tile kernels' paired grid bit for bit the single-tile grid; zeros behind S
     bit for bit N(0, 30) behind S; a cache laid out at max_seq 448 bit for bit the one at 440; rows at and past M untouched; the
     caches and their NaN guards untouched.
  B  the visible set TO THE BIT (pf_attn_rule.mask_probe / mask_expected): one key more or less in a row of n moves an output by
     about 1 / n, under a bf16 step from n = 100 or so, so no tolerance sees an off-by-one in pf_visible, `full`, `relevant`, t_lo / t_hi
     or clo / chi; on the probe it changes the expected bits.  Swept over M x start x window for every kernel and both attn8 grids.
  C  mc_pf_attn4_bfloat_hd128 bit for bit mc_pf_attn2_bfloat_hd128 (one template, pf_attn_kt_body) on every case of A."""
import functools
import time

import numpy as np
import pytest

import parity
import pf_attn_rule as pr
from test_attn_kernels_gpu import oracle_attention
from test_batch_kernels_gpu import GUARD, NAN, bf, f, guarded
from test_rows_kernels_gpu import etab, pattern, scale_of  # noqa: F401  (etab: a fixture)

pytestmark = pytest.mark.gpu
BF16 = 0
PAST = 64          # rows of Q and out behind the chunk: a pattern of NaNs, never read and never written
ROWS = 440         # the longest chunk / cache of section A

# kernel, head_dim, H, KV
SHAPES = [
    ("mc_pf_attn_bfloat_hd32", 32, 32, 32), ("mc_pf_attn_bfloat_hd64", 64, 48, 16), ("mc_pf_attn_bfloat_hd128", 128, 32, 32),
    ("mc_pf_attn_bfloat_hd256", 256, 32, 32), ("mc_pf_attn_bfloat_hd256", 256, 32, 16),
    ("mc_pf_attn2_bfloat_hd32", 32, 32, 8), ("mc_pf_attn2_bfloat_hd64", 64, 32, 16), ("mc_pf_attn2_bfloat_hd128", 128, 32, 4),
    ("mc_pf_attn4_bfloat_hd128", 128, 32, 8), ("mc_pf_attn4_bfloat_hd128", 128, 32, 4),
    ("mc_pf_attn8_bfloat_hd128", 128, 32, 8), ("mc_pf_attn8_bfloat_hd128", 128, 32, 4),
    ("mc_pf_attn8_bfloat_hd64_h8", 64, 32, 4), ("mc_pf_attn8_bfloat_hd64_h4", 64, 32, 8), ("mc_pf_attn8_bfloat_hd64_h4", 64, 48, 4),
    ("mc_pf_attn8_bfloat_hd256", 256, 32, 32), ("mc_pf_attn8_bfloat_hd256", 256, 32, 16),
]
SHAPE_IDS = [f"{k[6:]}-H{H}-KV{KV}" for k, _, H, KV in SHAPES]
# every case for the four-head kernel and the LDS-tile kernels -- and for an older kernel on one of THEIR shapes, whose references
# are computed anyway; a subset for the older 16-row kernels elsewhere
KEEP_ALL = {s[1:] for s in SHAPES if "attn4" in s[0] or "attn8" in s[0]}


# ------------------------------------------------------------------------------------------ data and launches
class Data:
    """the queries, keys and values of one (head_dim, H, KV): chunk row r holds q[r] and slot s holds k[s] / v[s] in every case, so
    the oracle's row for (r, keys [lo, hi]) serves every kernel and case that asks for it"""

    def __init__(self, hd, H, KV):
        self.hd, self.H, self.KV, self.n_rep, self.scale = hd, H, KV, H // KV, scale_of(hd)
        rng = np.random.default_rng([hd, H, KV])
        self.q = bf(rng.normal(0, 1, (ROWS, H, hd)))
        self.k = bf(rng.normal(0, 0.4, (ROWS, KV, hd)))      # magnitudes of test_rows_kernels_gpu.Call
        self.v = bf(rng.normal(0, 0.5, (ROWS, KV, hd)))
        self.refs = {}

    def caches(self, max_seq, S, tail):
        """K [KV][max_seq][hd], V [KV][hd][max_seq]; the slots [S, max_seq) hold N(0, 30) (as test_attn_kernels_gpu.device_caches) or zeros"""
        KV, hd = self.KV, self.hd
        kc, vt = np.zeros((KV, max_seq, hd), np.uint16), np.zeros((KV, hd, max_seq), np.uint16)
        if tail == "big":
            rng = np.random.default_rng(9)
            kc[:, S:] = bf(rng.normal(0, 30, (KV, max_seq - S, hd)))
            vt[:, :, S:] = bf(rng.normal(0, 30, (KV, hd, max_seq - S)))
        kc[:, :S] = self.k[:S].transpose(1, 0, 2)
        vt[:, :, :S] = self.v[:S].transpose(1, 2, 0)
        return kc, vt

    def reference(self, r, lo, hi):
        key = (r, lo, hi)
        if key not in self.refs:
            self.refs[key] = oracle_attention(self.q[r], self.k[lo:hi + 1], self.v[lo:hi + 1], self.n_rep, float(self.scale))
        return self.refs[key]


@functools.lru_cache(maxsize=None)
def data_of(hd, H, KV):
    return Data(hd, H, KV)


class Caches:
    """one K / V pair on the device, each followed by the NaN guard"""

    def __init__(self, acc, kc, vt):
        self.k_host, self.v_host = guarded([kc], 1), guarded([vt], 1)
        self.kb, self.vb = acc.to_device(self.k_host), acc.to_device(self.v_host)

    def check_untouched(self, what):
        assert np.all(self.k_host[-GUARD:] == NAN) and np.all(self.v_host[-GUARD:] == NAN)
        parity.exact(self.kb.download(np.uint16, self.k_host.size), self.k_host, f"{what}: K cache and guard")
        parity.exact(self.vb.download(np.uint16, self.v_host.size), self.v_host, f"{what}: V cache and guard")


def q_rows(q, M):
    """[M + PAST][H][hd]: the chunk's rows, then the pattern"""
    _, H, hd = q.shape
    rows = pattern((M + PAST) * H * hd).reshape(M + PAST, H, hd)
    rows[:M] = q[:M]
    return rows


def launch(acc, etab, kernel, c, qb, out, M, S, H, n_rep, max_seq, window, pair):
    """one launch as plan_attention would make it; `out` a Buffer or (Buffer, byte offset)"""
    import metalchat_amd as mc

    (gx, gy), threads = pr.launch_shape(kernel, M, H, pair, n_rep=n_rep, max_seq=max_seq, S=S)
    u32 = np.uint32
    mc.KernelTask(acc.load(kernel), (gx * threads, gy, 1), (threads, 1, 1),
                  [qb, c.kb, c.vb, out, u32(M), u32(S), u32(H), u32(n_rep), u32(max_seq), scale_of(pr.head_dim(kernel)), u32(window), etab])()


def grids(kernel):
    return (False, True) if pr.pairable(kernel) else (False,)


def outputs(acc, etab, kernel, d, case, tail, pairs=(False,), layout=None):
    """the chunk rows [M][H][hd] of one launch per entry of `pairs` on the caches of `case`, the cache laid out at `layout` slots
    (default: the case's max_seq); rows at and past M must keep the pattern, the rows of the chunk must be finite, the caches and
    guards must come back as uploaded"""
    max_seq, start, M, window = case
    max_seq, S = layout or max_seq, start + M
    what = f"{kernel} H {d.H} KV {d.KV} max_seq {max_seq} start {start} M {M} window {window} behind S: {tail}"
    c = Caches(acc, *d.caches(max_seq, S, tail))
    qb = acc.to_device(q_rows(d.q, M).reshape(-1))
    n = (M + PAST) * d.H * d.hd
    outb = acc.to_device(np.tile(pattern(n), len(pairs)))
    for i, pair in enumerate(pairs):
        launch(acc, etab, kernel, c, qb, (outb, i * n * 2), M, S, d.H, d.n_rep, max_seq, window, pair)
    acc.wait()
    got = outb.download(np.uint16, n * len(pairs)).reshape(len(pairs), M + PAST, d.H, d.hd)
    for i, pair in enumerate(pairs):
        parity.exact(got[i, M:], pattern(n).reshape(M + PAST, d.H, d.hd)[M:], f"{what} paired {pair}: output rows at and past M")
        assert np.all(np.isfinite(f(got[i, :M]))), f"{what} paired {pair}: not finite"
    parity.exact(qb.download(np.uint16, n), q_rows(d.q, M).reshape(-1), f"{what}: Q")
    c.check_untouched(what)
    return [got[i, :M] for i in range(len(pairs))]


# ------------------------------------------------------------------------------------------ the cases of section A
GROUPS = ["rows", "start", "window-0", "window-40", "end"]


def WINDOWS(M):
    return (1, 16, 17, 33, 64, 65, 100, M, M + 5)


def cases(kernel, hd, H, KV, group):
    """(max_seq, start, M, window) of one group"""
    RT, every = pr.row_tile(kernel), (hd, H, KV) in KEEP_ALL
    if group == "rows":     # 2 RT + 1: an odd tile count, the middle tile alone; 4 RT: an even one; ragged last tiles
        ms = [2, RT - 1, RT, RT + 1, 2 * RT + 1, 4 * RT, 5 * RT + 3] if every else [2, RT + 1, 5 * RT + 3]
        return [(320, 0, M, 0) for M in sorted({min(M, 200) for M in ms})]
    if group == "start":
        pl = [(21, 150), (31, 34), (63, 2), (64, 65), (100, 97)] if every else [(21, 150), (63, 2), (64, 65)]
        return [(320, s, M, 0) for s, M in pl]
    if group == "window-0":
        return [(320, 0, 193, w) for w in (WINDOWS(193) if every else (16, 33))]
    if group == "window-40":
        return [(320, 40, 130, w) for w in (WINDOWS(130) if every else (1, 17, 64, 65, 135))]
    # the end of a cache that is not whole 64-key tiles: what is read past it is zeroed or clamped by the kernel
    return ([(440, 0, 440, 0)] if hd <= 128 else []) + [(440, 300, 140, 0), (72, 0, 72, 0), (72, 40, 32, 0)]


def select_rows(M, start, window):
    """the chunk rows of a case that are compared with the oracle"""
    rows = {0, 1, M - 2, M - 1} | set(range(0, M, 37))
    rows |= {r for r in range(M) if r % 16 in (0, 15) or (start + r) % 32 in (0, 31)}
    if window:
        rows |= {window - 2, window - 1, window, window + 1}
    return sorted(r for r in rows if 0 <= r < M)


def check_rows(d, out, case, what):
    """test_rows_kernels_gpu.check_against for the selected rows of one case; prints the worst figures first"""
    _, start, M, window = case
    worst = dict(max_ulp=0, frac=0.0, normwise=0.0)
    fails, differ, total = [], 0, 0
    rows = select_rows(M, start, window)
    for r in rows:
        ref = d.reference(r, *pr.visible(r, M, start + M, window))
        differ, total = differ + int(np.sum(out[r] != ref)), total + ref.size
        try:
            st = parity.check(BF16, out[r], ref, rel=2e-3, max_ulp=1, max_frac=0.03, scale_aware=True, what=f"{what}: chunk row {r}")
            worst = {k: max(worst[k], st[k]) for k in worst}
        except AssertionError as e:
            fails.append(str(e))
    print(f"{what}: worst over {len(rows)} chunk rows {worst}; {differ / total:.4f} of all elements differ; {len(fails)} rows outside the bound")
    return fails


# ------------------------------------------------------------------------------------------ A
@pytest.mark.parametrize("group", GROUPS)
@pytest.mark.parametrize("kernel,hd,H,KV", SHAPES, ids=SHAPE_IDS)
def test_a_chunk_rows_against_the_oracle(acc, etab, kernel, hd, H, KV, group):
    d = data_of(hd, H, KV)
    fails = []
    for case in cases(kernel, hd, H, KV, group):
        max_seq, start, M, window = case
        what = f"{kernel} H {H} KV {KV} max_seq {max_seq} start {start} M {M} window {window}"
        outs = outputs(acc, etab, kernel, d, case, "big", grids(kernel))
        if len(outs) == 2:   # which workgroup takes a row tile does not enter a row's arithmetic
            parity.exact(outs[1], outs[0], f"{what}: row tiles in pairs against one per workgroup")
        if start + M < max_seq:   # the contract of DESIGN.md "The packed prompt pass": FINITE slots behind S do not matter
            parity.exact(outputs(acc, etab, kernel, d, case, "zero")[0], outs[0], f"{what}: zeros against N(0, 30) behind S")
        if max_seq == 440:
            parity.exact(outputs(acc, etab, kernel, d, case, "big", layout=448)[0], outs[0], f"{what}: the cache laid out at 448 slots")
        fails += check_rows(d, outs[0], case, what)
    assert not fails, fails[:5]


# ------------------------------------------------------------------------------------------ C
@pytest.mark.parametrize("KV", [8, 4])
def test_c_four_heads_per_workgroup_are_two_bit_for_bit(acc, etab, KV):
    """pf_attn_kt_body<128, 4> against <128, 2>: NH only adds heads to a workgroup -- every row sum, probability and output of a head
    goes through the same operations in the same order"""
    d = data_of(128, 32, KV)
    for group in GROUPS:
        for case in cases("mc_pf_attn4_bfloat_hd128", 128, 32, KV, group):
            four = outputs(acc, etab, "mc_pf_attn4_bfloat_hd128", d, case, "big")[0]
            two = outputs(acc, etab, "mc_pf_attn2_bfloat_hd128", d, case, "big")[0]
            parity.exact(four, two, f"KV {KV} (max_seq, start, M, window) {case}: attn4 against attn2")


# ------------------------------------------------------------------------------------------ B
B_M = [2, 15, 16, 17, 31, 32, 33, 63, 64, 65, 97, 130, 193]
# 14 and 30: start + r0 = 30 (mod 32) for a 16-row block at r0 is the one residue at which a 32-key block ends ONE key past the
# block's first row -- where `full` must still say no (measured: `blk + 31 - sq < rs0 + 2` in pf_attn_lds_body fails this test at these
# two starts and nowhere else).  The other starts put S - M on, one before and one behind the 32- / 64-key edges
B_START = [0, 1, 14, 30, 31, 33, 63, 64, 100]
B_WINDOW = [0, 1, 2, 15, 16, 17, 31, 32, 33, 63, 64, 65, 100]
B_PLACES = [(320, s, M) for s in B_START for M in B_M] + [(ms, ms - M, M) for ms in (72, 200) for M in B_M if M <= ms]   # ... and S = max_seq


@pytest.mark.parametrize("kernel,hd,H,KV", SHAPES, ids=SHAPE_IDS)
def test_b_the_visible_set_to_the_bit(acc, etab, kernel, hd, H, KV):
    """every (M, start, window): the launches of one placement (all windows, both grids) chained on the queue into one output buffer,
    one download; the expected bits from pf_attn_rule.mask_expected"""
    n_rep, pairs = H // KV, grids(kernel)
    t0, launches, bad = time.perf_counter(), 0, []
    for max_seq, start, M in B_PLACES:
        S = start + M
        q, kc, vt = pr.mask_probe(hd, H, KV, max_seq, start, M)
        c = Caches(acc, kc, vt)
        qb = acc.to_device(q_rows(q, M).reshape(-1))
        n = (M + PAST) * H * hd
        slots = [(w, p) for w in B_WINDOW for p in pairs]
        pat = pattern(n).reshape(M + PAST, H, hd)
        outb = acc.to_device(np.tile(pat.reshape(-1), len(slots)))
        for i, (w, p) in enumerate(slots):
            launch(acc, etab, kernel, c, qb, (outb, i * n * 2), M, S, H, n_rep, max_seq, w, p)
        acc.wait()
        launches += len(slots)
        got = outb.download(np.uint16, n * len(slots)).reshape(len(slots), M + PAST, H, hd)
        for i, (w, p) in enumerate(slots):
            exp = pr.mask_expected(hd, M, S, w) if p == pairs[0] else exp
            if not np.array_equal(got[i, :M], np.broadcast_to(exp[:, None, :], (M, H, hd))):
                wrong = np.flatnonzero(np.any(got[i, :M] != exp[:, None, :], axis=(1, 2)))
                bad.append(f"max_seq {max_seq} start {start} M {M} window {w} paired {p}: chunk rows {wrong[:8].tolist()} of {len(wrong)}")
            if not np.array_equal(got[i, M:], pat[M:]):
                bad.append(f"max_seq {max_seq} start {start} M {M} window {w} paired {p}: rows at and past M written")
        c.check_untouched(f"{kernel} max_seq {max_seq} start {start} M {M}")
    print(f"{kernel} H {H} KV {KV}: {launches} launches at {len(B_PLACES)} placements in {time.perf_counter() - t0:.2f} s; {len(bad)} differ")
    assert not bad, (len(bad), bad[:6])
