"""The rule of row log-probabilities (tests/logprob_rule.py; include/metalchat_hip.h Part 2n) without a GPU: six logits by hand, a
row with a single finite logit, the rule evaluated in the order the device evaluates it (chunks of 2048, per-thread partial sums,
a xor-tree per wave, the chunks merged in order) against the whole-row evaluation under the part's condition -- never more than
1 float32 ulp apart, bit-equal on at least 999 of every 1000 finite values -- and the order of the top n on ties."""
import math

import numpy as np
import pytest

import logprob_rule as lpr
from oracle import mc_oracle as mo

def bits(x):
    return mo.to_bf16(np.asarray(x, dtype=np.float32))


def test_six_logits_by_hand():
    y = [1.0, 0.0, -math.inf, 2.0, 1.0, -1.0]
    S = math.exp(-1.0) + math.exp(-2.0) + 0.0 + 1.0 + math.exp(-1.0) + math.exp(-3.0)
    lse = 2.0 + math.log(S)
    want = np.array([v - lse for v in y], dtype=np.float64).astype(np.float32)
    got = lpr.logprobs(bits(y))
    assert abs(lpr.lse(bits(y)) - lse) < 1e-14
    assert np.isneginf(got[2]) and np.isneginf(want[2])
    assert (lpr.ulps(got[[0, 1, 3, 4, 5]], want[[0, 1, 3, 4, 5]]) <= 1).all(), (got, want)   # (math.fsum-free hand sum: the last bit may differ)
    assert abs(float(np.exp(got[np.isfinite(got)].astype(np.float64)).sum()) - 1.0) < 1e-6
    ids, lp = lpr.top(bits(y), 6)
    assert ids.tolist() == [3, 0, 4, 1, 5, 2]                   # 2.0, the two 1.0 by index, 0.0, -1.0, the banned one last
    assert (lp == got[ids]).all() and np.isneginf(lp[5])


def test_a_single_finite_logit_has_probability_one():
    for V, at, v in ((6, 4, -3.5), (130, 129, 7.0), (4104, 2048, 0.0)):
        y = np.full(V, -np.inf, np.float32)
        y[at] = v
        got = lpr.logprobs(bits(y))
        assert got[at] == 0.0 and not np.signbit(got[at])
        assert np.isneginf(np.delete(got, at)).all()
        ids, lp = lpr.top(bits(y), 3)
        assert ids[0] == at and lp[0] == 0.0
        assert ids[1:].tolist() == [i for i in range(V) if i != at][:2] and np.isneginf(lp[1:]).all()   # the -inf tail in index order
        assert np.float32(v - lpr.lse_chunked(bits(y))) == 0.0


@pytest.mark.parametrize("V", [130, 2056, 4104, 128256])
def test_the_device_order_keeps_the_rules_bits(V):
    rng = np.random.default_rng(V)
    compared = differing = 0
    for rep in range(4):
        x = np.clip(rng.normal(0, 3, V), -9, 9).astype(np.float32)
        x[rng.random(V) < 0.3] = -np.inf
        if V == 4104:
            x[2048:4096] = -np.inf        # a whole middle chunk of -inf
        x[5] = 4.0
        b = bits(x)
        d = lpr.values(b)
        whole = lpr.logprobs(b)
        with np.errstate(invalid="ignore"):
            chunked = (d - lpr.lse_chunked(b)).astype(np.float32)
        n, k = lpr.check(chunked, whole, f"V {V} rep {rep}", share=False)
        compared += n
        differing += k
    assert compared > 0.6 * 4 * V * (0.5 if V == 4104 else 1)
    lpr.check_share(compared, differing, f"V {V}")


def test_the_top_n_order_on_ties():
    V = 4104
    y = np.full(V, -2.0, np.float32)
    y[[2049, 2047, 100, 4000]] = 3.0        # equal maxima on both sides of index 2048
    y[[7, 3]] = [0.0, -0.0]                  # -0.0 == +0.0: index decides
    y[10] = 0.0
    b = bits(y)
    assert b[3] == 0x8000
    ids, lp = lpr.top(b, 8)
    assert ids.tolist() == [100, 2047, 2049, 4000, 3, 7, 10, 0]
    assert (lp[:4] == lp[0]).all() and (lp[4:7] == lp[4]).all() and lp[0] > lp[4] > lp[7]
    assert lpr.order(b)[:8].tolist() == ids.tolist()
    # fewer finite logits than n: the tail is -inf, in index order
    z = np.full(130, -np.inf, np.float32)
    z[[129, 64]] = [1.0, 1.0]
    ids, lp = lpr.top(bits(z), 5)
    assert ids.tolist() == [64, 129, 0, 1, 2] and np.isneginf(lp[2:]).all() and lp[0] == lp[1] == np.float32(-math.log(2.0))
