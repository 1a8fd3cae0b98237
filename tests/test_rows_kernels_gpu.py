"""Kernel-level parity of the packed prompt pass (kernels/packed_kernels.hip, mc_pp_*) and of the chunks that see their row's context
(kernels/extend_kernels.hip, mc_px_*): every kernel launched BY NAME through the Part-1 seam on buffers the test owns, with tables
built by rows_tables.py (the restatement of rows_plan.h's rules), against a plain reference of the same operation:

  * mc_px_sums{,2} + mc_px_pv{,2} + mc_px_reduce: chunk row i at position p = pos + i against the oracle's attention over the keys
    [0, p] of its row, with the bound of the decode attention (test_batch_kernels_gpu.test_b_attention_per_row); the one-head and
    two-head kernels bit for bit; launch groups (ebase != 0) bit for bit one launch; split against unsplit row sums within the
    fp32 additions counted from the code; rows past a chunk's end sum to exactly 0; whatever lies behind a row's keys -- large values,
    NaN, infinities -- and in the caches of rows outside the call changes no bit; nothing but the call's output rows is written;
  * mc_pp_attn / mc_pp_attn2: the reference's mask (the chunk's own columns only) against the oracle, and bit for bit the
    one-prompt kernels mc_pf_attn / mc_pf_attn2 on the same cache;
  * mc_pp_rope_cache{,_parts}: q rows, K slots and V columns bit for bit the oracle's rope at slot pos + i, whole caches compared;
  * mc_pp_gather_last: x[row] = the segment's last packed row, other rows of x untouched.

Every cache buffer holds B rows at cache_stride = KV * max_seq * hd + GUARD with a NaN guard behind each row, compared bit for bit
after the launches; Q / out / qkv buffers start as a pattern of NaNs, so that "not written" is parity.exact against the pattern."""
import numpy as np
import pytest

import parity
import rows_tables as rt
from oracle import mc_oracle as mo
from test_attn_kernels_gpu import oracle_attention
from test_batch_kernels_gpu import GUARD, NAN, bf, bf16_rne64, f, guarded, rope_table

pytestmark = pytest.mark.gpu
BF16 = 0
B = 8

PX = {(64, 1): ("mc_px_sums_bfloat_hd64", "mc_px_pv_bfloat_hd64"), (64, 2): ("mc_px_sums2_bfloat_hd64", "mc_px_pv2_bfloat_hd64"),
      (128, 1): ("mc_px_sums_bfloat_hd128", "mc_px_pv_bfloat_hd128"), (128, 2): ("mc_px_sums2_bfloat_hd128", "mc_px_pv2_bfloat_hd128")}
PX_REDUCE = {64: "mc_px_reduce_bfloat_hd64", 128: "mc_px_reduce_bfloat_hd128"}
PP_ATTN = {(64, 1): "mc_pp_attn_bfloat_hd64", (64, 2): "mc_pp_attn2_bfloat_hd64",
           (128, 1): "mc_pp_attn_bfloat_hd128", (128, 2): "mc_pp_attn2_bfloat_hd128"}
PF_ATTN = {1: "mc_pf_attn_bfloat_hd", 2: "mc_pf_attn2_bfloat_hd"}   # + head_dim: the one-prompt kernels
NO_SPLIT, KEYS128 = rt.keys_of(0), rt.keys_of(128)


# ------------------------------------------------------------------------------------------ helpers
def pattern(n):
    """n bf16 NaNs of distinct payloads (0x7FC1 .. 0x7FFB): a copy from the wrong place shows, too"""
    return (0x7FC1 + np.arange(n) % 59).astype(np.uint16)


def scale_of(hd):
    return np.float32(f(bf(np.array([hd ** -0.5])))[0])


@pytest.fixture(scope="module")
def etab(acc):
    import metalchat_amd as mc

    t = acc.alloc(65536 * 4)
    mc.KernelTask(acc.load("mc_exp_table_bfloat"), (256 * 256, 1, 1), (256, 1, 1), [t])()
    acc.wait()
    return t


# (batch row, position, length) of the segments of one call on B = 8 rows; one row stays outside every call.  Lengths 2 .. 130 (last
# tiles of 1, 2, 15 and 16 rows), positions around the 32-key blocks and 128-key range boundaries, and max_seq - len (the last slot)
CALLS = {
    "a": (1024, [(0, 0, 2), (1, 1, 15), (2, 31, 16), (4, 32, 17), (5, 63, 31), (6, 64, 32), (7, 127, 33)]),
    "b": (1024, [(0, 128, 64), (1, 511, 65), (3, 512, 130), (4, 513, 2), (5, 1008, 16), (6, 511, 17), (7, 991, 33)]),
    "c": (2048, [(1, 1918, 130), (2, 2046, 2), (3, 1, 32), (4, 127, 64), (5, 63, 65), (6, 1300, 17), (7, 512, 15)]),
    "d": (1000, [(0, 983, 17), (1, 998, 2), (2, 967, 33), (4, 513, 31), (5, 128, 16), (6, 0, 130), (7, 985, 15)]),   # not a multiple of 32
}
# call, head_dim, H, KV: n_rep 1 and 3 (the one-head names), 4 and 8 (the `2` names) at both head sizes.  Where a row is compared with the
# oracle H is 32 or 48: `max_frac` counts elements of one chunk row ([H][hd], as test_b_attention_per_row counts them over 2048 or
# 4096), and one probability that rounds to the other neighbour moves about half of its head's outputs by a step -- 8 % of a row of
# 6 heads, 1.6 % of a row of 32 (DESIGN.md "Chunks that see their context": what the kernel-level tests found)
SHAPES = [("a", 64, 32, 32), ("a", 128, 48, 16), ("b", 64, 48, 16), ("b", 128, 32, 32), ("c", 64, 32, 8), ("c", 128, 32, 4), ("d", 64, 32, 4),
          ("d", 128, 32, 8)]


class Call:
    """the buffers of one call: segment i of `items` keeps its data (a function of the seed and i) wherever it is placed"""

    def __init__(self, max_seq, items, H, KV, hd, seed, gap=0):
        self.max_seq, self.H, self.KV, self.hd, self.n_rep = max_seq, H, KV, hd, H // KV
        self.items = items
        order = sorted(range(len(items)), key=lambda i: items[i][0])      # the table is in batch-row order
        lens, pos = [0] * B, [0] * B
        for r, p, n in items:
            assert lens[r] == 0 and 0 <= r < B and n >= 2 and p + n <= max_seq
            lens[r], pos[r] = n, p
        segs = rt.segments(lens, pos)
        # `gap` packed rows in front of every segment that no segment owns (the kernels go by `off` alone)
        self.segs = [(r, p, off + gap * (i + 1), n) for i, (r, p, off, n) in enumerate(segs)]
        self.seg_of = {item: si for si, item in enumerate(order)}
        self.rows_buf = self.segs[-1][2] + self.segs[-1][3] + 16            # 16 rows behind the last segment
        self.tiles = rt.tiles(self.segs)
        self.q, self.k, self.v = [], [], []
        for i, (r, p, n) in enumerate(items):
            rng = np.random.default_rng([seed, i])
            self.q.append(bf(rng.normal(0, 1, (n, H, hd))))
            self.k.append(bf(rng.normal(0, 0.4, (p + n, KV, hd))))        # magnitudes of test_context_gpu.random_cache
            self.v.append(bf(rng.normal(0, 0.5, (p + n, KV, hd))))
        self.cstride = KV * max_seq * hd + GUARD
        self.scale = scale_of(hd)

    def owned(self):
        """packed rows that belong to a segment"""
        m = np.zeros(self.rows_buf, bool)
        for _, _, off, n in self.segs:
            m[off:off + n] = True
        return m

    def q_rows(self):
        q = pattern(self.rows_buf * self.H * self.hd).reshape(self.rows_buf, self.H, self.hd)
        for i in range(len(self.items)):
            _, _, off, n = self.segs[self.seg_of[i]]
            q[off:off + n] = self.q[i]
        return q

    def caches(self, tail="zero", seed=0):
        """K [B][KV][max_seq][hd] and V [B][KV][hd][max_seq]: a row of the call holds its keys in [0, pos + len) and `tail` behind
        them; a row outside the call holds NaN"""
        KV, S, hd = self.KV, self.max_seq, self.hd
        rng = np.random.default_rng([seed, 77])
        kc, vt = np.full((B, KV, S, hd), NAN, np.uint16), np.full((B, KV, hd, S), NAN, np.uint16)
        for i, (r, p, n) in enumerate(self.items):
            for c, shape in ((kc, (KV, S, hd)), (vt, (KV, hd, S))):
                if tail == "zero":
                    c[r] = 0
                elif tail == "big":
                    c[r] = bf(rng.normal(0, 30, shape))
                elif tail == "nan":
                    c[r] = NAN
                else:
                    c[r] = np.where(rng.integers(0, 2, shape) == 1, 0x7F80, 0xFF80).astype(np.uint16)   # +inf / -inf
            kc[r, :, :p + n] = self.k[i].transpose(1, 0, 2)
            vt[r, :, :, :p + n] = self.v[i].transpose(1, 2, 0)
        return kc, vt

    def device(self, acc, tail="zero"):
        kc, vt = self.caches(tail)
        self.k_host, self.v_host = guarded(kc, B), guarded(vt, B)
        self.kb, self.vb = acc.to_device(self.k_host), acc.to_device(self.v_host)
        self.qb = acc.to_device(self.q_rows().reshape(-1))
        self.segb = acc.to_device(rt.words(self.segs, 4).reshape(-1))
        return self

    def check_caches_untouched(self, what):
        """the attention only reads: caches and guards bit for bit what was uploaded"""
        parity.exact(self.kb.download(np.uint16, B * self.cstride), self.k_host, f"{what}: K caches and guards")
        parity.exact(self.vb.download(np.uint16, B * self.cstride), self.v_host, f"{what}: V caches and guards")

    def check_unowned(self, out, what):
        """output rows that belong to no segment (between segments, behind the last) keep the pattern"""
        keep = ~self.owned()
        parity.exact(out[keep], pattern(out.size).reshape(out.shape)[keep], f"{what}: output rows of no segment")

    def rows_of(self, out, i):
        _, _, off, n = self.segs[self.seg_of[i]]
        return out[off:off + n]


def px_launch(acc, etab, c, tab, grps, nh, slots=None):
    """mc_px_sums, mc_px_pv and (a group with a split tile) mc_px_reduce as prefill.cc run_prefill launches them, group by group
    with ebase = the group's first range.  The scratch of a group is `slots` slots (the largest group), refilled with NaN between
    groups; the sums buffer continues as a NaN guard up to the whole table's size, so that an index that forgets ebase reads NaN
    inside the buffer.  Returns the output rows and the sums of every range [ranges][H][16]"""
    import metalchat_amd as mc

    H, hd = c.H, c.hd
    slots = slots or max(g[1] for g in grps)
    assert all(g[1] <= slots for g in grps)
    cap = max(slots, len(tab))
    tabb = acc.to_device(rt.words(tab, 8).reshape(-1))
    nan_sums = np.full(cap * H * 16, np.nan, np.float32)
    nan_part = np.full((slots + 1) * H * 16 * hd, np.nan, np.float32)    # (a slot of guard behind it)
    sumsb, partb = acc.to_device(nan_sums), acc.to_device(nan_part)
    out0 = pattern(c.rows_buf * H * hd)
    outb = acc.to_device(out0)
    sums = np.zeros((len(tab), H, 16), np.float32)
    k_sums, k_pv = (acc.load(n) for n in PX[hd, nh])
    k_red = acc.load(PX_REDUCE[hd])
    u32 = np.uint32
    for gi, (first, count, split) in enumerate(grps):
        if gi:
            sumsb.upload(nan_sums)
            partb.upload(nan_part)
        grid = (H // nh * 256, count, 1)
        mc.KernelTask(k_sums, grid, (256, 1, 1), [c.qb, c.segb, tabb, u32(first), c.kb, np.uint64(c.cstride), sumsb, u32(H), u32(c.n_rep),
                                                  u32(c.max_seq), c.scale, etab])()
        acc.wait()
        got = sumsb.download(np.float32, cap * H * 16).reshape(cap, H, 16)
        sums[first:first + count] = got[:count]
        assert np.all(np.isnan(got[count:])), f"group {gi}: mc_px_sums wrote behind its {count} slots"
        mc.KernelTask(k_pv, grid, (256, 1, 1), [c.qb, c.segb, tabb, u32(first), c.kb, c.vb, np.uint64(c.cstride), sumsb, partb, outb, u32(H),
                                                u32(c.n_rep), u32(c.max_seq), c.scale, etab])()
        if split:   # (prefill.cc: only a group that holds a split tile)
            mc.KernelTask(k_red, (H * 256, count, 1), (256, 1, 1), [c.segb, tabb, u32(first), partb, outb, u32(H)])()
        acc.wait()
        part = partb.download(np.float32, nan_part.size).reshape(slots + 1, -1)
        assert np.all(np.isnan(part[count:])), f"group {gi}: mc_px_pv wrote behind its {count} slots"
    return outb.download(np.uint16, out0.size).reshape(c.rows_buf, H, hd), sums


def one_group(tab):
    return [(0, len(tab), any(e[5] > 1 for e in tab))]


def groups_at(tab, cuts):
    """launch groups with boundaries at the range indices `cuts` (each the first range of a tile)"""
    edges = [0] + list(cuts) + [len(tab)]
    assert edges == sorted(set(edges)) and all(e == len(tab) or tab[e][4] == e for e in edges), cuts
    return [(a, b_ - a, any(e[5] > 1 for e in tab[a:b_])) for a, b_ in zip(edges, edges[1:])]


def px_reference(c):
    """chunk row i of a segment at pos: the oracle's attention of q_i over the keys [0, pos + i] of its row"""
    return [np.stack([oracle_attention(c.q[i][r], c.k[i][:p + r + 1], c.v[i][:p + r + 1], c.n_rep, float(c.scale)) for r in range(n)])
            for i, (_, p, n) in enumerate(c.items)]


def pp_reference(c):
    """the reference's mask: the chunk's own columns [pos, pos + i] only"""
    return [np.stack([oracle_attention(c.q[i][r], c.k[i][p:p + r + 1], c.v[i][p:p + r + 1], c.n_rep, float(c.scale)) for r in range(n)])
            for i, (_, p, n) in enumerate(c.items)]


def check_against(c, out, ref, what):
    """every chunk row within the bound of the decode attention (test_b_attention_per_row); prints the worst figures first"""
    worst = dict(max_ulp=0, frac=0.0, normwise=0.0)
    fails, differ, total = [], 0, 0
    for i, (r, p, n) in enumerate(c.items):
        got = c.rows_of(out, i)
        differ, total = differ + int(np.sum(got != ref[i])), total + got.size
        for j in range(n):
            try:
                st = parity.check(BF16, got[j], ref[i][j], rel=2e-3, max_ulp=1, max_frac=0.03, scale_aware=True,
                                  what=f"{what}: row {r} pos {p} len {n} chunk row {j}")
                worst = {k: max(worst[k], st[k]) for k in worst}
            except AssertionError as e:
                fails.append(str(e))
    print(f"{what}: worst over the chunk rows {worst}; {differ / total:.4f} of all elements differ; {len(fails)} rows outside the bound")
    assert not fails, fails[:5]
    c.check_unowned(out, what)


def check_sums(c, tab, sums, what):
    """a row of a tile past the chunk's end has the sum 0.0 exactly in every range; a row of the chunk sees key 0, so the first range's
    sum and the tile's sum are positive"""
    i = 0
    while i < len(tab):
        si, r0, _, _, first, cnt = tab[i][:6]
        live = min(16, c.segs[si][3] - r0)
        s = sums[first:first + cnt]
        assert np.all(np.isfinite(s)), f"{what}: tile {si}/{r0}"
        assert np.all(s[:, :, live:] == 0.0), f"{what}: tile {si}/{r0}: a row past the chunk's end has a sum"
        assert np.all(s[0, :, :live] > 0.0), f"{what}: tile {si}/{r0}: a live row's first range sums to 0"
        assert np.all(s[:, :, :live] >= 0.0) and np.all(tile_sums(s)[:, :live] > 0.0), f"{what}: tile {si}/{r0}"
        i += cnt


def tile_sums(s):
    """the ranges of a tile added first to last in fp32, as mc_px_pv adds them"""
    t = np.zeros(s.shape[1:], np.float32)
    for k in range(s.shape[0]):
        t = (t + s[k]).astype(np.float32)
    return t


def sum_depth(keys):
    """fp32 additions on the longest path from one exp to the sum of a range of `keys` keys, from px_sums_body: a lane takes every
    fourth 32-key block of the range -- ceil(ceil(keys / 32) / 4) blocks -- and per block adds two values to rsum, each a tree of
    depth 2 over four exps (2 + 2 * blocks); then two shuffles across the lane groups and a tree of depth 2 over the four waves"""
    blocks = -(-(-(-keys // 32)) // 4)
    return 2 + 2 * blocks + 2 + 2


def check_split_sums(c, tab, sums, tab1, sums1, what):
    """the range sums of a split tile added first to last against the one-range sum of the same tile.  Every term is positive and
    both are sums of the SAME exps (one table value per score), so each lies within gamma_d = d 2^-24 / (1 - d 2^-24) of the exact
    sum, d = the additions on its longest path: sum_depth(keys of the longest range) + one per range added for the split form (a
    range starts at a multiple of 128 keys, so its blocks are whole), sum_depth(all keys) for the other; the 2 covers the
    denominators and the exact sum standing for the one-range sum.  |a - b| <= (d_a + d_b + 2) 2^-24 sum"""
    one = {(e[0], e[1]): sums1[j] for j, e in enumerate(tab1)}
    assert len(one) == len(tab1)
    i, worst = 0, 0.0
    while i < len(tab):
        si, r0, _, _, first, cnt = tab[i][:6]
        i += cnt
        if cnt == 1:
            parity.exact(sums[first], one[si, r0], f"{what}: tile {si}/{r0}: one range is the unsplit launch")
            continue
        total, ref = tile_sums(sums[first:first + cnt]).astype(np.float64), one[si, r0].astype(np.float64)
        d_split = max(sum_depth(e[3] - e[2]) for e in tab[first:first + cnt]) + cnt
        d_one = sum_depth(tab[first + cnt - 1][3])
        bound = (d_split + d_one + 2) * 2.0 ** -24 * ref
        worst = max(worst, float(np.max(np.abs(total - ref) / np.maximum(bound, 1e-300))))
        assert np.all(np.abs(total - ref) <= bound), f"{what}: tile {si}/{r0} ({cnt} ranges): split sums against the one-range sum"
    print(f"{what}: split sums against one-range sums: worst |difference| / bound = {worst:.3f}")


# ------------------------------------------------------------------------------------------ A1: chunks that see their context
@pytest.mark.parametrize("call,hd,H,KV", SHAPES)
def test_px_attention_against_the_oracle(acc, etab, call, hd, H, KV):
    max_seq, items = CALLS[call]
    c = Call(max_seq, items, H, KV, hd, seed=hd + H, gap=3).device(acc)
    ref = px_reference(c)
    nh = 2 if c.n_rep % 2 == 0 else 1
    tab1 = rt.ranges(c.segs, c.tiles, NO_SPLIT)
    out1, sums1 = px_launch(acc, etab, c, tab1, one_group(tab1), nh)
    check_against(c, out1, ref, f"call {call} hd {hd} n_rep {c.n_rep} unsplit")
    check_sums(c, tab1, sums1, f"call {call} hd {hd} unsplit")
    for rule, name in ((rt.default_keys, "default rule"), (KEYS128, "128-key ranges")):
        what = f"call {call} hd {hd} n_rep {c.n_rep} {name}"
        tab = rt.ranges(c.segs, c.tiles, rule)
        counts = {e[5] for e in tab}
        if rule is rt.default_keys:   # one range; two for a segment of at most 32 rows behind more than 512 keys (none in call a)
            assert counts == ({1} if call == "a" else {1, 2}), (what, counts)
        else:                         # up to max_seq / 128 ranges per tile
            assert max(counts) == -(-max(p + n for _, p, n in items) // 128) and len(counts) > 1, (what, counts)
        out, sums = px_launch(acc, etab, c, tab, one_group(tab), nh)
        check_against(c, out, ref, what)
        check_sums(c, tab, sums, what)
        check_split_sums(c, tab, sums, tab1, sums1, what)
        if nh == 2:   # one px_tile, heads independent: the one-head kernels give the same bits
            o1, s1 = px_launch(acc, etab, c, tab, one_group(tab), 1)
            parity.exact(o1, out, f"{what}: one-head kernels against the two-head kernels, outputs")
            parity.exact(s1, sums, f"{what}: one-head kernels against the two-head kernels, sums")
    c.check_caches_untouched(f"call {call} hd {hd}")


GROUP_SHAPES = [("b", 128, 8, 2, 2), ("b", 64, 6, 2, 1), ("d", 64, 8, 2, 2), ("c", 128, 4, 4, 1)]


@pytest.mark.parametrize("call,hd,H,KV,nh", GROUP_SHAPES)
def test_px_launch_groups_give_the_bits_of_one_launch(acc, etab, call, hd, H, KV, nh):
    """ebase != 0: one table as one group, as two and three groups of whole tiles, and cut by the host's rule at several scratch
    sizes -- the scratch sized to the largest group and refilled with NaN between groups"""
    max_seq, items = CALLS[call]
    c = Call(max_seq, items, H, KV, hd, seed=3 * hd + H).device(acc)
    for rule, name in ((rt.default_keys, "default rule"), (KEYS128, "128-key ranges")):
        tab = rt.ranges(c.segs, c.tiles, rule)
        out, sums = px_launch(acc, etab, c, tab, one_group(tab), nh)
        firsts = [i for i, e in enumerate(tab) if e[4] == i]
        split = [i for i in firsts if tab[i][5] > 1]
        behind = max(i + tab[i][5] for i in split if i + tab[i][5] < len(tab))   # a boundary right behind a split tile ...
        front = min(i for i in split if i > 0)                                    # ... and one right in front of one
        mid = firsts[len(firsts) // 2]
        cuts = [[behind], [front], sorted({front, behind}), sorted({firsts[1], mid})]
        most = max(e[5] for e in tab)
        host = [rt.groups(tab, s) for s in (most, most + 1, len(tab) // 2 + 1)]
        assert all(len(g) > 1 for g in host)
        for grps in [groups_at(tab, cu) for cu in cuts] + host:
            what = f"call {call} hd {hd} {name}: {len(grps)} groups at {[g[0] for g in grps]}"
            o, s = px_launch(acc, etab, c, tab, grps, nh)
            parity.exact(o, out, f"{what}: outputs")
            parity.exact(s, sums, f"{what}: sums")
    c.check_caches_untouched(f"call {call} hd {hd}")


@pytest.mark.parametrize("call,hd,H,KV,nh", [("d", 64, 8, 2, 2), ("d", 128, 6, 2, 1), ("a", 128, 8, 2, 2), ("b", 64, 4, 4, 1)])
def test_px_what_lies_behind_a_rows_keys_does_not_matter(acc, etab, call, hd, H, KV, nh):
    """the slots of a row's cache at and past pos + len hold, in turn, zeros, N(0, 30) values, NaN and infinities (K and V both; the
    caches of the row outside the call hold NaN throughout): the same bits.  mc_px_pv zeroes such V element by element and the K
    loads are clamped to the tile's last key"""
    max_seq, items = CALLS[call]
    base = None
    for tail in ("zero", "big", "nan", "inf"):
        c = Call(max_seq, items, H, KV, hd, seed=5 * hd + H).device(acc, tail)
        got = []
        for rule in (rt.default_keys, KEYS128):
            tab = rt.ranges(c.segs, c.tiles, rule)
            got.append(px_launch(acc, etab, c, tab, one_group(tab), nh))
        c.check_caches_untouched(f"call {call} hd {hd} tail {tail}")
        if base is None:
            base = got
            assert all(np.all(np.isfinite(f(c.rows_of(o, i)))) for o, _ in got for i in range(len(items)))
            continue
        for (o, s), (o0, s0), name in zip(got, base, ("default rule", "128-key ranges")):
            parity.exact(o, o0, f"call {call} hd {hd} {name}: outputs with {tail} behind the keys")
            parity.exact(s, s0, f"call {call} hd {hd} {name}: sums with {tail} behind the keys")


PLACED = [(1, 600, 20), (4, 37, 65), (6, 1000, 24)]          # rows 1, 4, 6 of 8
MOVED = [(7, 600, 20), (0, 37, 65), (2, 1000, 24)]           # the same segments on other rows: another table order, other offsets


@pytest.mark.parametrize("hd,H,KV,nh", [(128, 32, 8, 2), (64, 48, 16, 1)])
def test_px_placement_does_not_matter(acc, etab, hd, H, KV, nh):
    a = Call(1024, PLACED, H, KV, hd, seed=hd).device(acc)
    b_ = Call(1024, MOVED, H, KV, hd, seed=hd, gap=5).device(acc)
    assert [g[0] for g in a.segs] == [1, 4, 6] and [g[0] for g in b_.segs] == [0, 2, 7]
    assert [a.segs[a.seg_of[i]][2] for i in range(3)] != [b_.segs[b_.seg_of[i]][2] for i in range(3)]
    ref = px_reference(a)
    for rule, name in ((rt.default_keys, "default rule"), (KEYS128, "128-key ranges")):
        ta, tb = rt.ranges(a.segs, a.tiles, rule), rt.ranges(b_.segs, b_.tiles, rule)
        (oa, sa), (ob, sb) = px_launch(acc, etab, a, ta, one_group(ta), nh), px_launch(acc, etab, b_, tb, one_group(tb), nh)
        check_against(a, oa, ref, f"rows 1, 4, 6 hd {hd} {name}")
        b_.check_unowned(ob, f"moved hd {hd} {name}")
        for i in range(3):
            parity.exact(b_.rows_of(ob, i), a.rows_of(oa, i), f"hd {hd} {name}: segment {i} moved, outputs")
            ra = [j for j, e in enumerate(ta) if e[0] == a.seg_of[i]]
            rb = [j for j, e in enumerate(tb) if e[0] == b_.seg_of[i]]
            assert [ta[j][1:4] for j in ra] == [tb[j][1:4] for j in rb]
            parity.exact(sb[rb], sa[ra], f"hd {hd} {name}: segment {i} moved, sums")
    a.check_caches_untouched("rows 1, 4, 6")
    b_.check_caches_untouched("moved")


# ------------------------------------------------------------------------------------------ A2: the packed prompt pass's attention
def pp_launch(acc, etab, c, nh):
    """mc_pp_attn{,2}_bfloat_hd*: grid (tiles, H / NH), as prefill.cc run_prefill launches it"""
    import metalchat_amd as mc

    H, hd = c.H, c.hd
    out0 = pattern(c.rows_buf * H * hd)
    outb = acc.to_device(out0)
    tilb = acc.to_device(rt.words(c.tiles, 2).reshape(-1))
    u32 = np.uint32
    mc.KernelTask(acc.load(PP_ATTN[hd, nh]), (len(c.tiles) * 256, H // nh, 1), (256, 1, 1),
                  [c.qb, c.segb, tilb, c.kb, c.vb, np.uint64(c.cstride), outb, u32(H), u32(c.n_rep), u32(c.max_seq), c.scale, etab])()
    acc.wait()
    return outb.download(np.uint16, out0.size).reshape(c.rows_buf, H, hd)


def pf_launch(acc, etab, c, i, nh):
    """the one-prompt kernel on segment i's own cache: M = len rows at S = pos + len, no window"""
    import metalchat_amd as mc

    H, hd = c.H, c.hd
    r, p, n = c.items[i]
    off = c.segs[c.seg_of[i]][2]
    outb = acc.to_device(pattern(n * H * hd))
    u32 = np.uint32
    mc.KernelTask(acc.load(PF_ATTN[nh] + str(hd)), ((n + 15) // 16 * 256, H // nh, 1), (256, 1, 1),
                  [(c.qb, off * H * hd * 2), (c.kb, r * c.cstride * 2), (c.vb, r * c.cstride * 2), outb, u32(n), u32(p + n), u32(H), u32(c.n_rep),
                   u32(c.max_seq), c.scale, u32(0), etab])()
    acc.wait()
    return outb.download(np.uint16, n * H * hd).reshape(n, H, hd)


@pytest.mark.parametrize("call,hd,H,KV", SHAPES)
def test_pp_attention_against_the_oracle_and_the_one_prompt_kernels(acc, etab, call, hd, H, KV):
    max_seq, items = CALLS[call]
    c = Call(max_seq, items, H, KV, hd, seed=7 * hd + H, gap=2).device(acc)
    big = Call(max_seq, items, H, KV, hd, seed=7 * hd + H, gap=2).device(acc, "big")
    ref = pp_reference(c)
    for nh in ((1, 2) if c.n_rep % 2 == 0 else (1,)):
        what = f"call {call} {PP_ATTN[hd, nh]} n_rep {c.n_rep}"
        out = pp_launch(acc, etab, c, nh)
        check_against(c, out, ref, what)
        # finite values past pos + len do not matter (the contract: finite slots past S -- DESIGN.md "The packed prompt pass")
        parity.exact(pp_launch(acc, etab, big, nh), out, f"{what}: N(0, 30) behind the keys")
        # the one-prompt kernels' device bodies: a segment at pos = 0 (call a, d) and at pos = p, bit for bit
        for i, (r, p, n) in enumerate(items):
            parity.exact(c.rows_of(out, i), pf_launch(acc, etab, c, i, nh), f"{what}: row {r} pos {p} len {n} against the one-prompt kernel")
    c.check_caches_untouched(f"call {call} hd {hd}")
    big.check_caches_untouched(f"call {call} hd {hd} (N(0, 30) behind the keys)")


@pytest.mark.parametrize("hd,H,KV,nh", [(128, 32, 8, 2), (64, 48, 16, 1), (64, 32, 4, 2), (128, 32, 32, 1)])
def test_pp_placement_does_not_matter(acc, etab, hd, H, KV, nh):
    a = Call(1024, PLACED, H, KV, hd, seed=hd + 1).device(acc)
    b_ = Call(1024, MOVED, H, KV, hd, seed=hd + 1, gap=5).device(acc)
    oa, ob = pp_launch(acc, etab, a, nh), pp_launch(acc, etab, b_, nh)
    check_against(a, oa, pp_reference(a), f"{PP_ATTN[hd, nh]} rows 1, 4, 6")
    b_.check_unowned(ob, f"{PP_ATTN[hd, nh]} moved")
    for i in range(3):
        parity.exact(b_.rows_of(ob, i), a.rows_of(oa, i), f"{PP_ATTN[hd, nh]}: segment {i} moved")
    a.check_caches_untouched("rows 1, 4, 6")
    b_.check_caches_untouched("moved")


# ------------------------------------------------------------------------------------------ A3: rope + cache write
ROPE_ITEMS = [(1, 0, 2), (3, 63, 17), (4, 195, 5), (6, 100, 33)]   # rows not adjacent; 16-row V tiles over two and three segments; the last slot
ROPE_S, THETA = 200, 500000.0


def unpartner(x):
    """the inverse of packed_partners: fused [2j], [2j + 1] -> natural [j], [j + hd / 2]"""
    h, hd = x.shape
    return np.ascontiguousarray(x.reshape(h, hd // 2, 2).transpose(0, 2, 1)).reshape(h, hd)


class RopeCase:
    def __init__(self, acc, H, KV, hd):
        self.H, self.KV, self.hd, self.NQ = H, KV, hd, (H + 2 * KV) * hd
        lens, pos = [0] * B, [0] * B
        for r, p, n in ROPE_ITEMS:
            lens[r], pos[r] = n, p
        self.segs = rt.segments(lens, pos)
        self.M = sum(lens)
        per = 2048 // hd
        assert self.M % 16 and ((H + KV) * self.M) % per, "M a multiple neither of a V tile nor of the q / k units per workgroup"
        self.cb, self.sb, fcos, fsin = rope_table(acc, ROPE_S, hd, THETA)
        half = hd // 2
        self.rc, self.rs = np.zeros((ROPE_S, half), np.float32), np.zeros((ROPE_S, half), np.float32)
        L = mo.layout
        mo.rope_freqs(L(self.rc.shape), self.rc, L(self.rs.shape), self.rs, hd, 0, THETA)
        parity.exact(fcos, self.rc, "mc_rope_table cos against rope_freqs")
        parity.exact(fsin, self.rs, "mc_rope_table sin against rope_freqs")
        rng = np.random.default_rng(H + hd)
        self.kc0 = bf(rng.normal(0, 30, (B, KV, ROPE_S, hd)))
        self.vt0 = bf(rng.normal(0, 30, (B, KV, hd, ROPE_S)))
        self.cstride = KV * ROPE_S * hd + GUARD
        self.segb = acc.to_device(rt.words(self.segs, 4).reshape(-1))
        self.gx = ((H + KV) * self.M + per - 1) // per + KV * ((self.M + 15) // 16)    # prefill.cc pk_gx

    def slot(self, r):
        """packed row r -> (batch row, slot)"""
        for row, p, off, n in self.segs:
            if off <= r < off + n:
                return row, p + r - off
        raise AssertionError(r)

    def launch(self, acc, rows, splits=0):
        """rows: bf16 [M][NQ] (mc_pp_rope_cache_bfloat) or fp32 parts [splits][M][NQ] (mc_pp_rope_cache_parts_bfloat)"""
        import metalchat_amd as mc

        H, KV, hd, M = self.H, self.KV, self.hd, self.M
        kb, vb = acc.to_device(guarded(self.kc0, B)), acc.to_device(guarded(self.vt0, B))
        q0 = pattern((M + 16) * H * hd)
        qo = acc.to_device(q0)
        u32 = np.uint32
        tail = [qo, self.segb, u32(len(self.segs)), kb, vb, np.uint64(self.cstride), self.cb, self.sb, u32(H), u32(KV), u32(hd), u32(ROPE_S)]
        rb = acc.to_device(np.ascontiguousarray(rows).reshape(-1))
        if splits:
            mc.KernelTask(acc.load("mc_pp_rope_cache_parts_bfloat"), (self.gx * 256, 1, 1), (256, 1, 1), [rb, u32(splits), u32(M)] + tail)()
        else:
            mc.KernelTask(acc.load("mc_pp_rope_cache_bfloat"), (self.gx * 256, 1, 1), (256, 1, 1), [rb, u32(M)] + tail)()
        acc.wait()
        q = qo.download(np.uint16, q0.size).reshape(M + 16, H, hd)
        parity.exact(q[M:], q0.reshape(M + 16, H, hd)[M:], "q rows past M")
        return q[:M], kb.download(np.uint16, B * self.cstride).reshape(B, self.cstride), vb.download(np.uint16, B * self.cstride).reshape(B, self.cstride)

    def rope(self, x, heads, pos):
        """mo.rope of natural rows [heads][hd] at table row pos"""
        L = mo.layout
        o = np.zeros((heads, self.hd), np.uint16)
        mo.rope(BF16, L(o.shape), o, L(o.shape), np.ascontiguousarray(x), L(self.rc.shape), self.rc, L(self.rs.shape), self.rs, 1, heads, pos)
        return o

    def split_row(self, row):
        """a fused row [NQ] -> natural q [H][hd], natural k [KV][hd], v [KV][hd]"""
        H, KV, hd = self.H, self.KV, self.hd
        return unpartner(row[:H * hd].reshape(H, hd)), unpartner(row[H * hd:(H + KV) * hd].reshape(KV, hd)), row[(H + KV) * hd:].reshape(KV, hd)

    def expect(self, x):
        """fused bf16 rows [M][NQ] -> q rows, and the whole K / V buffers: the initial content with exactly the call's slots replaced"""
        q = np.zeros((self.M, self.H, self.hd), np.uint16)
        kc, vt = self.kc0.copy(), self.vt0.copy()
        for r in range(self.M):
            row, slot = self.slot(r)
            qn, kn, vn = self.split_row(x[r])
            q[r] = self.rope(qn, self.H, slot)
            kc[row, :, slot] = self.rope(kn, self.KV, slot)
            vt[row, :, :, slot] = vn
        return q, guarded(kc, B).reshape(B, -1), guarded(vt, B).reshape(B, -1)


ROPE_SHAPES = [(16, 4, 64), (32, 2, 64), (16, 4, 128), (32, 2, 128)]   # as test_b_rope_kv_lockstep_and_rows


@pytest.mark.parametrize("H,KV,hd", ROPE_SHAPES)
def test_pp_rope_cache_rows_slots_and_columns(acc, H, KV, hd):
    rc = RopeCase(acc, H, KV, hd)
    assert [rc.slot(r)[0] for r in (0, 15)] == [1, 3] and len({rc.slot(r)[0] for r in range(16, 32)}) == 3   # V tiles over 2 and 3 segments
    rng = np.random.default_rng(hd + KV)
    x = bf(rng.normal(0, 1, (rc.M, rc.NQ)))
    got = rc.launch(acc, x)
    for g, e, name in zip(got, rc.expect(x), ("q rows", "K caches (every row, guards included)", "V caches (every row, guards included)")):
        parity.exact(g, e, f"mc_pp_rope_cache H {H} KV {KV} hd {hd}: {name}")


@pytest.mark.parametrize("H,KV,hd", ROPE_SHAPES)
def test_pp_rope_cache_parts_sums_in_front_of_the_rope(acc, H, KV, hd):
    rc = RopeCase(acc, H, KV, hd)
    rng = np.random.default_rng(hd + H)
    for splits in (1, 2, 3, 4, 5):   # pf_part_sum8 goes in fours
        # parts that are small multiples of 2^-6: their sum is exact in fp32 in any order -> the plain kernel on T(sum), bit for bit
        parts = (rng.integers(-64, 65, (splits, rc.M, rc.NQ)) / 64.0).astype(np.float32)
        x = bf(parts.sum(axis=0, dtype=np.float64).astype(np.float32))
        got, plain = rc.launch(acc, parts, splits), rc.launch(acc, x)
        for g, p, e, name in zip(got, plain, rc.expect(x), ("q rows", "K caches", "V caches")):
            parity.exact(g, p, f"mc_pp_rope_cache_parts splits {splits} H {H} hd {hd}: {name} against the plain kernel on T(sum)")
            parity.exact(g, e, f"mc_pp_rope_cache_parts splits {splits} H {H} hd {hd}: {name} against the oracle's rope")
    # generic parts: the kernel ropes T(s32), s32 the fp32 sum in z order, which lies within eps = 5 * 2^-24 * sum |part| of the float64
    # sum s64.  Where every value that close to s64 rounds to the same bfloat the rope's input is T(s64), and every written value is
    # asserted within one bf16 step of the oracle's rope of T(s64).  Where it does not (s64 at a rounding boundary, or a sum that
    # cancelled to less than eps) every bfloat in [T(s64 - eps), T(s64 + eps)] is a correct rounding of the sum; the rope's fp32
    # operations and T are monotone in each input, so the written value must lie within one step of the span of the ropes of the
    # four corners (lo / hi of a pair's first and second element)
    splits = 5
    parts = rng.normal(0, 1, (splits, rc.M, rc.NQ)).astype(np.float32)
    s64 = parts.astype(np.float64).sum(axis=0)
    eps = splits * 2.0 ** -24 * np.abs(parts.astype(np.float64)).sum(axis=0)
    lo, hi = bf16_rne64(s64 - eps), bf16_rne64(s64 + eps)
    amb = lo != hi
    print(f"generic parts H {H} hd {hd}: {int(amb.sum())} of {amb.size} sums have more than one correct rounding")
    assert amb.mean() < 1e-2   # (about 2 eps / (a bf16 step): two in a thousand)
    q, kc, vt = rc.launch(acc, parts, splits)
    nb = (H + KV) * hd
    first = (np.arange(rc.NQ) % 2 == 0) | (np.arange(rc.NQ) >= nb)          # fused layout: element 2j of a pair (and all of v)
    cands = [rc.expect(np.where(first, a, b_)) for a in (lo, hi) for b_ in (lo, hi)]
    for gi, (g, name) in enumerate(zip((q, kc, vt), ("q rows", "K caches", "V caches"))):
        o = np.stack([parity.bf16_ordinal(cd[gi]) for cd in cands])
        go = parity.bf16_ordinal(g)
        if gi == 0:
            assert not np.any((g & 0x7FFF) > 0x7F80), f"generic parts H {H} hd {hd}: a NaN in the q rows"
        d = np.maximum(np.maximum(o.min(axis=0) - go, go - o.max(axis=0)), 0)
        print(f"generic parts H {H} hd {hd}: {name}: at most {int(d.max())} bf16 steps, {float(np.mean(d != 0)):.5f} of the values differ")
        assert d.max() <= 1, f"generic parts H {H} hd {hd}: {name}: {int(d.max())} bf16 steps from the rope of the float64 sum"
        if not amb.any():   # the rope's input is T(s64) exactly
            parity.exact(g, cands[0][gi], f"generic parts H {H} hd {hd}: {name}: every sum has one correct rounding")


# ------------------------------------------------------------------------------------------ A4: the last rows
@pytest.mark.parametrize("dim", [1024, 2048, 1000])
def test_pp_gather_last(acc, dim):
    import metalchat_amd as mc

    c = Call(1024, PLACED + [(3, 5, 2)], 4, 4, 64, seed=dim, gap=4)
    rng = np.random.default_rng(dim)
    rows = bf(rng.normal(0, 1, (c.rows_buf, dim)))
    x0 = pattern(B * dim).reshape(B, dim)
    xb = acc.to_device(x0.reshape(-1))
    mc.KernelTask(acc.load("mc_pp_gather_last_bfloat"), ((dim + 255) // 256 * 256, len(c.segs), 1), (256, 1, 1),
                  [acc.to_device(rows.reshape(-1)), acc.to_device(rt.words(c.segs, 4).reshape(-1)), xb, np.uint32(dim)])()
    acc.wait()
    got = xb.download(np.uint16, B * dim).reshape(B, dim)
    exp = x0.copy()
    for r, _, off, n in c.segs:
        exp[r] = rows[off + n - 1]
    assert [g[0] for g in c.segs] == [1, 3, 4, 6]
    parity.exact(got, exp, f"mc_pp_gather_last dim {dim}: the segments' last rows, the other rows of x untouched")
