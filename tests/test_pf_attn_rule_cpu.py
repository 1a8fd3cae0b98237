"""pf_attn_rule.py (what test_pf_attn_kernels_gpu.py holds the one-prompt attention kernels to) checked without a device:

  * `visible` against a literal [M][S] additive mask built the way the reference builds it (nn/attention.h:283-321);
  * `mask_expected` against the oracle's attention on the probe's visible slice, bit for bit: the probe's expected bits need no
    oracle on the GPU side because its sums are exact, and this is where that claim is checked;
  * the bound the GPU test applies per chunk row (test_rows_kernels_gpu.check_against: one bf16 step at the row's scale, at most
    3 % of a row's elements different at all) against a numpy restatement of the kernels' rounding points with float64 dot products
    standing for "some other order of the fp32 additions": a correct kernel of that family must pass it at the head counts and
    lengths the GPU test uses, which is what fixes 32 heads as the fewest a compared row may have."""
import numpy as np
import pytest

import parity
import pf_attn_rule as pr
from oracle import mc_oracle as mo
from test_attn_kernels_gpu import oracle_attention

BF16 = 0


def literal_mask(M, S, window):
    """make_causal_mask / make_sliding_causal_mask: full(-inf), triu(narrow(1, S - M, M), 1); the sliding one adds a second
    matrix, triu(narrow(1, S - M, M).t(), window)"""
    upper = np.full((M, S), -np.inf)
    upper[:, S - M:] = np.triu(upper[:, S - M:], 1)
    if not window:
        return upper
    lower = np.full((M, S), -np.inf)
    lower[:, S - M:] = np.triu(lower[:, S - M:].T, window).T
    return upper + lower


@pytest.mark.parametrize("start", [0, 1, 31, 64])
def test_visible_is_the_references_mask(start):
    for M in range(1, 71):
        S = start + M
        for window in (0, 1, 2, 16, 33, 64, 100):
            mask = literal_mask(M, S, window)
            assert np.all((mask == 0) | np.isneginf(mask))
            for r in range(M):
                lo, hi = pr.visible(r, M, S, window)
                assert np.array_equal(np.flatnonzero(mask[r] == 0), np.arange(lo, hi + 1)), (M, start, window, r)


def test_launch_shapes_and_preconditions():
    ls = pr.launch_shape
    assert ls("mc_pf_attn_bfloat_hd64", 33, 48, False, n_rep=3, max_seq=320, S=33) == ((3, 48), 256)
    assert ls("mc_pf_attn2_bfloat_hd32", 16, 32, False, n_rep=4, max_seq=320, S=20) == ((1, 16), 256)
    assert ls("mc_pf_attn4_bfloat_hd128", 17, 32, False, n_rep=8, max_seq=320, S=17) == ((2, 8), 256)
    assert ls("mc_pf_attn8_bfloat_hd128", 65, 32, False, n_rep=4, max_seq=320, S=65) == ((3, 8), 512)
    assert ls("mc_pf_attn8_bfloat_hd128", 65, 32, True, n_rep=4, max_seq=320, S=65) == ((2, 8), 512)
    assert ls("mc_pf_attn8_bfloat_hd64_h4", 193, 48, True, n_rep=12, max_seq=320, S=193) == ((4, 12), 512)
    assert ls("mc_pf_attn8_bfloat_hd64_h8", 33, 32, True, n_rep=8, max_seq=72, S=72) == ((2, 4), 512)
    assert ls("mc_pf_attn8_bfloat_hd256", 130, 32, False, n_rep=2, max_seq=440, S=440) == ((3, 32), 256)
    assert ls("mc_pf_attn8_bfloat_hd256", 130, 32, True, n_rep=2, max_seq=440, S=440) == ((2, 32), 256)
    for bad in (dict(n_rep=2, max_seq=320, S=40),      # four heads of a workgroup over two kv heads
                dict(n_rep=4, max_seq=324, S=40),      # a transposed cache row that is no multiple of 16 bytes
                dict(n_rep=4, max_seq=320, S=321),     # more keys than slots
                dict(n_rep=4, max_seq=320, S=39)):     # more chunk rows than keys
        with pytest.raises(AssertionError):
            ls("mc_pf_attn4_bfloat_hd128", 40, 32, False, **bad)
    with pytest.raises(AssertionError):
        ls("mc_pf_attn8_bfloat_hd64_h8", 40, 36, False, n_rep=9, max_seq=320, S=40)
    with pytest.raises(AssertionError):
        ls("mc_pf_attn4_bfloat_hd128", 40, 32, True, n_rep=4, max_seq=320, S=40)   # only the LDS-tile kernels deal pairs


@pytest.mark.parametrize("hd", [32, 64, 128, 256])
def test_mask_expected_is_the_oracles_attention_on_the_probe(hd):
    lengths = [1, 2, hd, hd + 1, 2 * hd + 7, 440]
    H, KV, start, M = 4, 2, 5, max(lengths)
    S = start + M
    scale = float(mo.from_bf16(mo.to_bf16(np.array([hd ** -0.5], np.float32)))[0])
    q, kc, vt = pr.mask_probe(hd, H, KV, (S + 3 + 7) // 8 * 8, start, M)
    # rows n - 1 of the unwindowed chunk (ranges that begin at the chunk's first slot) and its last row under a window of n
    for window, rows in [(0, [n - 1 for n in lengths])] + [(n, [M - 1, M - 2]) for n in lengths]:
        exp = pr.mask_expected(hd, M, S, window)
        for r in rows:
            lo, hi = pr.visible(r, M, S, window)
            k = np.ascontiguousarray(kc[:, lo:hi + 1].transpose(1, 0, 2))
            v = np.ascontiguousarray(vt[:, :, lo:hi + 1].transpose(2, 0, 1))
            ref = oracle_attention(q[r], k, v, H // KV, scale)
            parity.exact(ref, np.broadcast_to(exp[r], (H, hd)), f"hd {hd} window {window} row {r}: keys [{lo}, {hi}]")


def T(x):
    return mo.round_bf16(np.asarray(x, np.float32))


def kernel_roundings(q, k, v, n_rep, scale):
    """the rounding points of pf_attn_kt_body / pf_attn_lds_body in numpy: s = T(T(q.k) scale), e = exp(s), the fp32 row sum over the
    keys in sequence, p = T(e (1 / sum)), out = T(sum p v) added 32 keys at a time; dot products in float64"""
    H = q.shape[0]
    qf = mo.from_bf16(q).astype(np.float64)
    kf = np.repeat(mo.from_bf16(k).astype(np.float64).transpose(1, 0, 2), n_rep, axis=0)    # [H][n][hd]
    vf = np.repeat(mo.from_bf16(v).astype(np.float64).transpose(1, 0, 2), n_rep, axis=0)
    s = T(T(np.einsum("hd,hnd->hn", qf, kf)) * np.float32(scale))
    e = np.exp(s.astype(np.float64)).astype(np.float32)
    total = np.zeros(H, np.float32)
    for j in range(e.shape[1]):
        total = total + e[:, j]
    p = T(e * (np.float32(1.0) / total)[:, None]).astype(np.float64)
    acc = np.zeros(q.shape, np.float32)
    for b in range(0, e.shape[1], 32):
        acc = acc + np.einsum("hn,hnd->hd", p[:, b:b + 32], vf[:, b:b + 32]).astype(np.float32)
    return mo.to_bf16(acc)


CAP_LENGTHS = list(range(1, 41, 3)) + [63, 64, 65, 100, 129, 200, 257, 300, 440]


@pytest.mark.parametrize("hd,H,KV", [(128, 32, 8), (64, 32, 4), (256, 32, 32), (256, 32, 16)])
def test_the_row_bound_admits_another_order_of_the_same_roundings(hd, H, KV):
    rng = np.random.default_rng([hd, H, KV])
    scale = float(mo.from_bf16(mo.to_bf16(np.array([hd ** -0.5], np.float32)))[0])
    worst = dict(max_ulp=0, frac=0.0, normwise=0.0)
    for n in CAP_LENGTHS:
        q = mo.to_bf16(rng.normal(0, 1, (H, hd)).astype(np.float32))
        k = mo.to_bf16(rng.normal(0, 0.4, (n, KV, hd)).astype(np.float32))
        v = mo.to_bf16(rng.normal(0, 0.5, (n, KV, hd)).astype(np.float32))
        st = parity.check(BF16, kernel_roundings(q, k, v, H // KV, scale), oracle_attention(q, k, v, H // KV, scale), rel=2e-3, max_ulp=1,
                          max_frac=0.03, scale_aware=True, what=f"hd {hd} H {H} KV {KV} n {n}")
        worst = {key: max(worst[key], st[key]) for key in worst}
    print(f"hd {hd} H {H} KV {KV}: worst over {len(CAP_LENGTHS)} lengths {worst}")
