"""Kernel-level check of the two mixed launches of the row samplers (batch_kernels.hip: mc_b_topk_candidates_mixed_bfloat,
mc_b_pick_mixed_bfloat / _rows_bfloat; include/metalchat_hip.h Part 2k), launched BY NAME through the Part-1 seam on hand-made
bfloat16 logits [8][1300] -- three candidate lists, the last one ragged (276 logits) -- with every row on settings of its own:

  * a greedy row picks the first index of the maximum (the maximum is planted twice);
  * a sampling row picks exactly what the oracle's make_default_sampler picks from its logits with its own seed pair: top_k 1 and
    128, top_p 0 and 1, temperature 0.25 and 4, rows with long runs of equal logits;
  * an idle row (`_rows` form) keeps every word of its state and its slot of tokens_out;
  * only the token word of a row's state changes, and only the rows' own slots of tokens_out;
  * the picks do not depend on the call's kpad: with the top_k = 128 row set to top_k = 3 the lists shrink from 128 to 64 keys and
    every other row picks the same token."""
import numpy as np
import pytest

import parity
from oracle import mc_oracle as mo
from test_batch_kernels_gpu import ST_POS, ST_STEP, ST_TOKEN, bf, f, first_max, states

pytestmark = pytest.mark.gpu
BF16 = 0
B, N, CAP = 8, 1300, 4096
GREEDY, DEFAULT = 0, 1
RS = np.dtype([("kind", np.int32), ("k", np.uint32), ("inv_temp", np.float32), ("top_p", np.float32)])   # kernels/abi.h row_sampler
SEEDS = np.array([[0, 0], [123456789, 987654321], [5, 6], [77, 1]], np.uint64)
IDLE = 7
# row: (kind, top_k, temperature, top_p)
SETTINGS = [(GREEDY, 0, 0.0, 0.0), (DEFAULT, 1, 0.6, 0.9), (DEFAULT, 128, 0.9, 0.95), (DEFAULT, 50, 0.6, 0.0),
            (DEFAULT, 50, 1.3, 1.0), (DEFAULT, 40, 0.25, 0.9), (DEFAULT, 40, 4.0, 0.95), (GREEDY, 0, 0.0, 0.0)]


def logits_rows():
    """8 rows, |x| <= 9.5 so that exp(x / 0.25) stays finite (the reference's softmax takes no maximum off).  Planted: the maximum
    twice (rows 0, 2, 5: the first occurrence wins, in another list than the second), runs of equal values (rows 3 and 6 are rounded
    to halves: a few dozen distinct values over 1300 logits; row 4 carries one run of 40 equal logits across the first list boundary),
    the maximum in the ragged last list (row 1)."""
    rng = np.random.default_rng(1300)
    x = np.clip(rng.normal(0, 2, (B, N)), -9.0, 8.0).astype(np.float32)
    x[0, [900, 17, 1299]] = 9.5
    x[1, 1290] = 9.0
    x[2, [600, 40]] = 9.5
    x[3] = np.round(x[3] * 2) / 2
    x[4, 492:532] = 6.0
    x[5, [1100, 300]] = 9.5
    x[6] = np.round(x[6] * 2) / 2
    x[7, [1024, 511]] = 9.25
    return bf(x)


def rt(v):
    return float(f(bf(np.array([v], np.float32)))[0])


def table(settings):
    t = np.zeros(B, RS)
    for r, (kind, top_k, temperature, top_p) in enumerate(settings):
        t[r]["kind"] = kind
        if kind == DEFAULT:   # as mc_row_sampler_set forms them
            t[r]["k"], t[r]["inv_temp"], t[r]["top_p"] = min(top_k, N), rt(1.0 / rt(temperature)), rt(top_p)
    return t


def run_mixed(acc, lb, settings, ragged):
    """the two launches as batch.cc head() makes them from batch_plan.h plan_head(); returns (the rows' states before, after, tokens_out)"""
    import metalchat_amd as mc

    kpad = 1
    while kpad < max(s[1] for s in settings if s[0] == DEFAULT):
        kpad *= 2
    chunk = max(512, kpad)
    lists = -(-N // chunk)
    assert lists == 3
    rows = states(B)
    rows[:, ST_POS] = np.arange(B)
    rows[:, ST_STEP] = 2 * B + np.arange(B)[::-1]
    if ragged:
        rows[IDLE, ST_POS] = -1
    rb = acc.to_device(rows.reshape(-1))
    tout = acc.to_device(np.full(4 * B, -1, np.int32))
    tb = acc.to_device(table(settings).view(np.uint8))
    cand = acc.alloc(B * lists * 128 * 8)
    seeds = acc.to_device(SEEDS.reshape(-1))
    mc.KernelTask(acc.load("mc_b_topk_candidates_mixed_bfloat"), (lists * 64, B, 1), (64, 1, 1),
                  [lb, np.uint32(N), np.uint32(kpad), cand, np.uint32(chunk), tb, rb, np.int32(1 if ragged else 0)])()
    mc.KernelTask(acc.load("mc_b_pick_mixed" + ("_rows_bfloat" if ragged else "_bfloat")), (1024, B, 1), (1024, 1, 1),
                  [lb, np.uint32(N), cand, tb, np.uint32(lists), np.uint32(kpad), np.uint32(CAP), seeds, np.uint32(len(SEEDS)), rb, tout],
                  lds_bytes=CAP * 8)()
    acc.wait()
    return rows, rb.download(np.int32, B * 12).reshape(B, 12), tout.download(np.int32, 4 * B), kpad


@pytest.fixture(scope="module")
def wanted():
    """the expected pick of every row under SETTINGS, and of row 2 at top_k = 3 -- computed once"""
    x = logits_rows()
    step = 2 * B + np.arange(B)[::-1]

    def want(r, kind, top_k, temperature, top_p):
        if kind == GREEDY:
            return first_max(x[r])
        s0, s1 = (int(v) for v in SEEDS[step[r] % len(SEEDS)])
        return mo.sample_default(BF16, x[r], top_k=top_k, temperature=temperature, top_p=top_p, init_state=s0, init_seq=s1)

    picks = [want(r, *SETTINGS[r]) for r in range(B)]
    assert picks[0] == 17 and picks[7] == 511 and picks[1] == 1290   # greedy: the first maximum; top_k = 1: the maximum
    return x, picks, want(2, DEFAULT, 3, 0.9, 0.95)


@pytest.mark.parametrize("ragged", [False, True])
def test_mixed_rows_pick_as_their_own_sampler(acc, wanted, ragged):
    x, picks, pick3 = wanted
    lb = acc.to_device(x.reshape(-1))
    settings3 = list(SETTINGS)
    settings3[2] = (DEFAULT, 3, 0.9, 0.95)
    for settings, want2, kpad_want in ((SETTINGS, picks[2], 128), (settings3, pick3, 64)):
        rows, got_rows, got_t, kpad = run_mixed(acc, lb, settings, ragged)
        assert kpad == kpad_want
        exp_t = np.full(4 * B, -1, np.int32)
        for r in range(B):
            what = f"kpad {kpad} ragged {ragged} row {r} {settings[r]}"
            if ragged and r == IDLE:
                parity.exact(got_rows[r], rows[r], f"{what}: the idle row's state")
                continue
            want = want2 if r == 2 else picks[r]
            assert got_rows[r, ST_TOKEN] == want, f"{what}: picked {got_rows[r, ST_TOKEN]}, expected {want}"
            exp_row = rows[r].copy()
            exp_row[ST_TOKEN] = want
            parity.exact(got_rows[r], exp_row, f"{what}: only the token word changes")
            exp_t[rows[r, ST_STEP]] = want
        parity.exact(got_t, exp_t, f"kpad {kpad} ragged {ragged}: tokens_out")
