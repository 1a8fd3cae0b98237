"""MC_SAMPLER_DRAW's rule (tests/draw_rule.py) held to what the header states about it, without a GPU:

  * k = 1 and top_p = 0 return make_default_sampler's pick (mo.sample_default) for every seed pair tried;
  * a masked position is never returned;
  * the fallback branch is reached (a constructed case), and total = 0 / NaN end at the stated position;
  * P(pos = j) = m[j] / total: the frequencies over 20 000 distinct seed pairs."""
import numpy as np

import draw_rule
from oracle import mc_oracle as mo

BF16 = 0
F = np.float32
SETTINGS = [(40, 0.9, 0.95), (5, 1.5, 0.5), (50, 0.6, 0.9)]   # the three the row-sampler tests use
PAIRS = [(0, 0), (1, 0), (0, 1), (12345, 678), (2**64 - 1, 2**63 + 5), (977, 2**40)] + [(1000 + 17 * i, 77 + i) for i in range(26)]
U_MAX = F(1.0) - F(2.0**-23)   # the generator's largest value: (x >> 9 | 0x3f800000) as a float, minus 1


def rows(n=2048, count=6, seed=3):
    rng = np.random.default_rng(seed)
    out = []
    for i in range(count):
        x = rng.standard_normal(n).astype(F) * F(2.5)
        if i % 2:   # exact ties at the maximum
            x[rng.integers(0, n, 3)] = x.max()
        out.append(mo.to_bf16(x))
    return out


def test_k_1_and_top_p_0_are_the_default_samplers_pick():
    for logits in rows():
        for k, t, p in [(1, 0.9, 0.95), (1, 1.5, 0.5), (40, 0.9, 0.0), (5, 1.5, 0.0), (128, 0.6, 0.0)]:
            for s0, s1 in PAIRS:
                want = mo.sample_default(BF16, logits, top_k=k, temperature=t, top_p=p, init_state=s0, init_seq=s1)
                tok, pos = draw_rule.draw(BF16, logits, k, t, p, s0, s1, with_pos=True)
                assert (tok, pos) == (want, 0), (k, t, p, s0, s1, tok, pos, want)


def test_a_masked_position_is_never_returned():
    drawn_above_0 = 0
    for logits in rows():
        for k, t, p in SETTINGS:
            toks, pos, taps = draw_rule.draw_many(BF16, logits, PAIRS, k, t, p)
            masked = taps[5]
            kept = int((masked > 0).sum())
            assert 1 <= kept <= masked.size and (masked[:kept] > 0).all() and (masked[kept:] == 0).all()   # the zeros are a suffix
            assert (pos < kept).all() and (masked[pos] > 0).all(), (k, t, p, pos, kept)
            assert np.array_equal(toks, taps[6][pos].astype(np.int64))
            drawn_above_0 += int((pos > 0).sum())
    assert drawn_above_0 > 100   # (the rows do draw: the statement is not held by position 0 alone)


def test_the_fallback_branch():
    # t = u * total < total for every normal total, even at u's maximum: total * 2^-23 is at least one ulp of total.  The product rounds up to
    # total only where total is denormal -- float32 cases exist, so the branch is reached by one: the sums never exceed t
    d = F(np.finfo(F).smallest_subnormal)
    assert F(U_MAX * d) == d and F(U_MAX * F(3 * d)) == F(3 * d)
    assert draw_rule.position(np.array([d, 0, 0], F), U_MAX) == 0
    assert draw_rule.position(np.array([2 * d, d, 0, 0], F), U_MAX) == 1        # the largest j with m[j] > 0, not the end of the row
    assert draw_rule.position(np.array([2 * d, d, 0, 0], F), F(0.25)) == 0      # (below the maximum the same row draws)
    one = F(1.0)
    assert F(U_MAX * one) < one and draw_rule.position(np.array([0.5, 0.5], F), U_MAX) == 1   # a normal total: the last kept entry by the sums
    # total = 0 and total = NaN: no sum exceeds t
    assert draw_rule.position(np.zeros(5, F), F(0.7)) == 0
    assert draw_rule.position(np.array([np.nan, 0.25, 0.0], F), F(0.7)) == 1
    assert draw_rule.position(np.array([np.nan, np.nan], F), F(0.7)) == 0
    # through the chain: a row that is -inf but for one entry keeps that entry alone, whatever the pair is
    logits = mo.to_bf16(np.full(2048, -np.inf, F))
    logits[1234] = mo.to_bf16(np.array([1.5], F))[0]
    for k, t, p in SETTINGS:
        toks, pos, taps = draw_rule.draw_many(BF16, logits, PAIRS, k, t, p)
        assert taps[5][0] == 1.0 and (taps[5][1:] == 0).all()
        assert (pos == 0).all() and (toks == 1234).all()


def test_the_frequencies_are_the_masked_probabilities():
    """one fixed row, k = 8, pairs (i, 7 i + 3) for i < 20 000 (fixed: the rule is deterministic in them); every position's frequency within
    4 binomial standard deviations of m[j] / total"""
    n, N = 2048, 20000
    x = np.full(n, -30.0, F)
    x[[5, 77, 300, 901, 1200, 1500, 1999, 2047]] = [2.0, 1.75, 1.5, 1.0, 0.5, 0.0, -0.5, -3.0]
    logits = mo.to_bf16(x)
    pairs = [(i, 7 * i + 3) for i in range(N)]
    assert len(set(pairs)) == N
    toks, pos, taps = draw_rule.draw_many(BF16, logits, pairs, top_k=8, temperature=1.0, top_p=0.95)
    m = taps[5].astype(np.float64)
    assert (m > 0).sum() >= 6 and m[-1] == 0   # the nucleus keeps most of the row and cuts its tail
    prob = m / m.sum()
    freq = np.bincount(pos, minlength=8) / N
    sd = np.sqrt(prob * (1 - prob) / N)
    print("p", prob, "freq", freq, "deviation / sd", (freq - prob) / np.where(sd > 0, sd, 1))
    assert (np.abs(freq - prob) <= 4 * sd).all(), (prob, freq, sd)
