"""Row samplers (mc_row_sampler_*, include/metalchat_hip.h Part 2k) on the device: each row of a batch picks with settings of its own.

  * a mixed batch -- greedy, two different default settings, one row inheriting the decoder's -- computes for every row, bit for
    bit, the tokens and K / V of a batch whose decoder-wide sampler is that row's effective setting, and each sampling row's pick is
    the oracle's make_default_sampler on the row's own logits with the row's own seed pair;
  * the same through every call a pick is made in: ragged steps with an idle row, a chained ragged call with a stop id, a rolling
    batch past the end of its cache, the packed prompt pass and chunks with context, a wide batch of 17 rows;
  * the launch forms: nothing set (or everything reset) launches what a fresh batch launches, rows set alike take the uniform
    launches, a mixed batch takes the two mixed ones and neither of the uniform picks;
  * verify looks at the rows in the call; the refusals, and what mc_row_sampler_get returns."""
import numpy as np
import pytest

import modelgen as mg
import parity
from oracle import mc_oracle as mo
from test_batch_gpu import SMALL, refused, small_decoder
from test_context_gpu import random_cache

pytestmark = pytest.mark.gpu
BF16 = 0
PAIRS = [(1000 + 17 * i, 77 + i) for i in range(5)]
GREEDY = "greedy"
DEC = (50, 0.6, 0.9)                                      # the decoder's sampler: what an inheriting row follows
SETTINGS = [GREEDY, (40, 0.9, 0.95), (5, 1.5, 0.5), None]  # row r of a batch takes SETTINGS[r % 4]; None = inherit
S64 = dict(SMALL, max_seq_len=64)                          # (the weights do not depend on max_seq_len)


@pytest.fixture(scope="module")
def small():
    return mg.make_model(SMALL, seed=11, quant="i4", group=128)


def effective(r):
    return SETTINGS[r % 4] or DEC


def set_decoder(dec, setting):
    import metalchat_amd as mc

    if setting == GREEDY:
        dec.set_sampler(mc.SAMPLER_GREEDY)
    else:
        dec.set_sampler(mc.SAMPLER_DEFAULT, top_k=setting[0], temperature=setting[1], top_p=setting[2])


def set_rows(batch, settings=SETTINGS):
    import metalchat_amd as mc

    for r in range(batch.B):
        s = settings[r % len(settings)]
        if s is None:
            batch.set_row_sampler(r, mc.SAMPLER_INHERIT)
        elif s == GREEDY:
            batch.set_row_sampler(r, mc.SAMPLER_GREEDY)
        else:
            batch.set_row_sampler(r, mc.SAMPLER_DEFAULT, top_k=s[0], temperature=s[1], top_p=s[2])


def fresh(dec, caches, wide=False, rolling=False):
    import metalchat_amd as mc

    b = mc.Batch(dec, len(caches), wide=wide)
    for r, kv in enumerate(caches):
        if kv is not None:
            b.import_kv(r, 0, *kv)
    if rolling:
        b.set_rolling(True)
    b.set_seeds(PAIRS)
    return b


def mixed_against_uniform(dec, caches, call, what, wide=False, rolling=False):
    """call(batch) -> int array [n][B].  Runs it on a batch with SETTINGS under a decoder set to DEC, then once per distinct effective
    setting on a batch without row samplers under a decoder set to it; the rows with that setting must agree in their tokens, their
    last logits and their K / V, bit for bit.  Returns the mixed batch's tokens and the names it launched."""
    B = len(caches)
    set_decoder(dec, DEC)
    mixed = fresh(dec, caches, wide, rolling)
    set_rows(mixed)
    dec.launch_log(True)
    got = np.asarray(call(mixed))
    names = dec.launched()
    dec.launch_log(False)
    assert got.ndim == 2 and got.shape[1] == B
    assert "mc_b_topk_candidates_mixed_bfloat" in names and [n for n in names if n.startswith("mc_b_pick_mixed")], (what, sorted(set(names)))
    assert not [n for n in names if n.startswith(("mc_b_argmax", "mc_b_sample"))], (what, sorted(set(names)))
    lengths = mixed.lengths()
    for setting in dict.fromkeys(effective(r) for r in range(B)):
        set_decoder(dec, setting)
        uniform = fresh(dec, caches, wide, rolling)
        want = np.asarray(call(uniform))
        assert list(uniform.lengths()) == list(lengths), (what, setting)
        for r in (r for r in range(B) if effective(r) == setting):
            assert np.array_equal(got[:, r], want[:, r]), (what, r, setting, got[:, r], want[:, r])
            parity.exact(mixed.logits()[r], uniform.logits()[r], f"{what} row {r}: logits")
            for a, b_, name in zip(mixed.export_row_kv(r, 0), uniform.export_row_kv(r, 0), "KV"):
                assert a.shape[0] == min(lengths[r], dec.cfg["max_seq_len"])
                parity.exact(a, b_, f"{what} row {r} under {setting}: {name}")
        uniform.release()
    mixed.release()
    return got, names


# ------------------------------------------------------------------------------------------ 1
def test_mixed_equals_uniform_bit_for_bit(acc, small):
    B, n, pos0 = 4, 8, 30
    dec = small_decoder(acc, SMALL, small)
    caches = [random_cache(SMALL, pos0, 700 + r) for r in range(B)]
    first = np.array([5, 900, 1500, 31], np.int32)
    got, names = mixed_against_uniform(dec, caches, lambda b: b.generate(first, pos0, n), "generate")
    assert "mc_b_pick_mixed_bfloat" in names
    # stepwise: every pick is the row's own sampler on the row's own logits with the row's own pair
    set_decoder(dec, DEC)
    stepwise = fresh(dec, caches)
    set_rows(stepwise)
    toks = first
    for i in range(3):
        stepwise.set_seeds([PAIRS[(i * B + r) % len(PAIRS)] for r in range(B)])   # a step uses pair r % n_pairs: rotate the list
        toks = stepwise.step(toks, pos0 + i)
        assert np.array_equal(toks, got[i]), (i, toks, got[i])
        logits = stepwise.logits()
        for r in range(B):
            if effective(r) == GREEDY:
                v = mo.from_bf16(logits[r]).astype(np.float64)
                want = int(np.flatnonzero(v == v.max())[0])
            else:
                k, t, p = effective(r)
                s0, s1 = PAIRS[(i * B + r) % len(PAIRS)]
                want = mo.sample_default(BF16, logits[r], top_k=k, temperature=t, top_p=p, init_state=s0, init_seq=s1)
            assert toks[r] == want, (i, r, effective(r), toks[r], want)
    stepwise.release()
    dec.release()


# ------------------------------------------------------------------------------------------ 2
def test_ragged_step_with_an_idle_row(acc, small):
    lens = [30, 41, 7, 60, 65, 20]
    dec = small_decoder(acc, SMALL, small)
    caches = [random_cache(SMALL, n, 800 + r) for r, n in enumerate(lens)]
    toks = np.array([5, 900, 1500, 31, 77, 3], np.int32)
    pos = np.array(lens, np.int32)
    pos[5] = -1   # a sampling row idle: its workgroups of both launches exit
    got, names = mixed_against_uniform(dec, caches, lambda b: b.step_rows(toks, pos)[None, :], "step_rows")
    assert "mc_b_pick_mixed_rows_bfloat" in names
    assert got[0, 5] == -1 and (got[0, :5] >= 0).all()
    dec.release()


def test_chained_ragged_call_with_a_stop_id(acc, small):
    lens, n = [30, 41, 7, 60], 6
    dec = small_decoder(acc, SMALL, small)
    caches = [random_cache(SMALL, m, 800 + r) for r, m in enumerate(lens)]
    first = np.array([5, 900, 1500, 31], np.int32)
    free, _ = mixed_against_uniform(dec, caches, lambda b: b.generate_rows(first, lens, n)[0], "generate_rows")
    stop = int(free[2, 1])   # row 1 (a sampling row) stops on its third token
    got, _ = mixed_against_uniform(dec, caches, lambda b: b.generate_rows(first, lens, n, stop=[stop])[0], "generate_rows with a stop id")
    assert np.array_equal(got[:3, 1], free[:3, 1]) and (got[3:, 1] == -1).all(), got[:, 1]
    for r in (0, 2, 3):   # the others go on (unless they draw the stop id themselves)
        produced = int((got[:, r] >= 0).sum())
        assert np.array_equal(got[:produced, r], free[:produced, r]) and (produced == n or got[produced - 1, r] == stop), (r, got[:, r])
    dec.release()


def test_rolling_rows_past_the_end(acc, small):
    S = S64["max_seq_len"]
    dec = small_decoder(acc, S64, small)
    caches = [random_cache(S64, S - 1, 900 + r) for r in range(4)]
    first = np.array([5, 900, 1500, 31], np.int32)
    got, _ = mixed_against_uniform(dec, caches, lambda b: b.generate_rows(first, [S - 1] * 4, 3)[0], "rolling", rolling=True)
    assert (got >= 0).all()   # positions S - 1, S and S + 1: no row stops at the end of its cache
    dec.release()


def test_prompt_passes(acc, small):
    rng = np.random.default_rng(21)
    dec = small_decoder(acc, SMALL, small)
    prompts = [rng.integers(0, SMALL["vocab"], n).astype(np.int32) for n in (5, 17, 33, 9)]
    chunks = [rng.integers(0, SMALL["vocab"], n).astype(np.int32) for n in (3, 2, 4, 6)]

    def call(b):
        a = b.prefill_rows(prompts)
        return np.stack([a, b.extend_rows(chunks, [len(p) for p in prompts])])

    got, names = mixed_against_uniform(dec, [None] * 4, call, "prefill_rows + extend_rows")
    assert (got >= 0).all()
    assert "mc_b_pick_mixed_rows_bfloat" in names
    dec.release()


def test_wide_batch(acc, small):
    B, pos0 = 17, 30
    dec = small_decoder(acc, SMALL, small)
    caches = [random_cache(SMALL, pos0, 700 + r) for r in range(B)]
    first = (np.arange(B, dtype=np.int32) * 113 + 5) % SMALL["vocab"]
    _, names = mixed_against_uniform(dec, caches, lambda b: b.generate(first, pos0, 3), "wide generate", wide=True)
    assert [n for n in names if n.startswith("mc_wb_gemv_")], sorted(set(names))
    dec.release()


# ------------------------------------------------------------------------------------------ 3
def test_launch_forms(acc, small):
    import metalchat_amd as mc

    B, pos0 = 4, 30
    dec = small_decoder(acc, SMALL, small)
    caches = [random_cache(SMALL, pos0, 700 + r) for r in range(B)]
    toks = np.array([5, 900, 1500, 31], np.int32)

    def log(batch, ragged):
        dec.launch_log(True)
        batch.step_rows(toks, [pos0] * B) if ragged else batch.step(toks, pos0)
        names = dec.launched()
        dec.launch_log(False)
        return names

    alike = (40, 0.9, 0.95)
    for ragged, sfx in ((False, "_bfloat"), (True, "_rows_bfloat")):
        for setting, picks in ((GREEDY, ["mc_b_argmax" + sfx]), (DEC, ["mc_b_topk_candidates_bfloat", "mc_b_sample" + sfx])):
            set_decoder(dec, setting)
            base = log(fresh(dec, caches), ragged)   # what a batch launches today
            assert base[-len(picks):] == picks and not [n for n in base if "_mixed" in n], base[-3:]
            b = fresh(dec, caches)
            assert log(b, ragged) == base, "no row sampler set"
            set_rows(b)
            mixed = log(b, ragged)
            assert mixed[:-2] == base[:-len(picks)], "only the pick changes"
            assert mixed[-2:] == ["mc_b_topk_candidates_mixed_bfloat", "mc_b_pick_mixed" + sfx], mixed[-3:]
            assert not [n for n in mixed if n.startswith(("mc_b_argmax", "mc_b_sample")) or n == "mc_b_topk_candidates_bfloat"], mixed
            b.reset_row_samplers()
            assert log(b, ragged) == base, "after reset_row_samplers"
            # all rows set alike: the uniform launches of those settings, whatever the decoder says
            for r in range(B):
                b.set_row_sampler(r, mc.SAMPLER_DEFAULT, *alike)
            same = log(b, ragged)
            assert same[-2:] == ["mc_b_topk_candidates_bfloat", "mc_b_sample" + sfx] and not [n for n in same if "_mixed" in n], same[-3:]
            for r in range(B):
                b.set_row_sampler(r, mc.SAMPLER_GREEDY)
            same = log(b, ragged)
            assert same[-1] == "mc_b_argmax" + sfx and not [n for n in same if "_mixed" in n or n.startswith(("mc_b_sample", "mc_b_topk"))], same[-3:]
            b.release()
    dec.release()


# ------------------------------------------------------------------------------------------ 4
def test_verify_looks_at_the_rows_in_the_call(acc, small):
    import metalchat_amd as mc

    B = 3
    rng = np.random.default_rng(5)
    dec = small_decoder(acc, SMALL, small)
    prompts = [rng.integers(0, SMALL["vocab"], n).astype(np.int32) for n in (12, 20, 7)]
    lens = [len(p) for p in prompts]
    drafts = [rng.integers(0, SMALL["vocab"], n).astype(np.int32) for n in (4, 6, 3)]
    chain = [np.arange(-1, len(d) - 1, dtype=np.int32) for d in drafts]

    def batch_with_prompts():
        b = mc.Batch(dec, B)
        b.prefill_rows(prompts)
        return b

    for tree in (False, True):
        verify = (lambda b, rows: b.verify_tree([drafts[r] if r in rows else None for r in range(B)],
                                                [chain[r] if r in rows else None for r in range(B)], lens)[:3]) if tree else \
                 (lambda b, rows: b.verify_rows([drafts[r] if r in rows else None for r in range(B)], lens))
        set_decoder(dec, GREEDY)
        greedy = batch_with_prompts()
        want = verify(greedy, (0, 1))
        set_decoder(dec, DEC)
        b = batch_with_prompts()   # (its prompt picks are sampled: the caches are the same)
        b.set_row_sampler(0, mc.SAMPLER_GREEDY)
        b.set_row_sampler(1, mc.SAMPLER_GREEDY)
        before = list(b.lengths())
        dec.launch_log(True)
        with pytest.raises(mc.McError) as e:
            verify(b, (0, 1, 2))
        assert e.value.status == 1 and "row 2" in str(e.value) and "greedy" in str(e.value), str(e.value)
        assert str(e.value).endswith(("mc_tree_verify" if tree else "mc_verify_rows") +
                                     ": row 2: the row's sampler is not greedy (accepting sampled drafts needs the draft's probabilities)")
        assert dec.launched() == [] and list(b.lengths()) == before
        dec.launch_log(False)
        got = verify(b, (0, 1))   # the sampling row 2 is not in the call: admitted
        for g, w, name in zip(got, want, ("accepted", "next_tokens", "picks")):
            for r in range(B):
                assert np.array_equal(g[r], w[r]) if g[r] is not None else w[r] is None, (tree, name, r, g[r], w[r])
        assert list(b.lengths()) == list(greedy.lengths())
        # nothing set and a sampling decoder: the decoder-wide refusal keeps its text
        b.reset_row_samplers()
        refused(lambda: verify(b, (0, 1)), "the decoder's sampler is not greedy")
        b.release()
        greedy.release()
    dec.release()


# ------------------------------------------------------------------------------------------ 5
def test_refusals_and_get(acc, small):
    import metalchat_amd as mc

    dec = small_decoder(acc, SMALL, small)
    b = mc.Batch(dec, 4)
    assert [b.row_sampler(r) for r in range(4)] == [(mc.SAMPLER_INHERIT, None, None, None)] * 4
    b.set_row_sampler(1, mc.SAMPLER_DEFAULT, top_k=20, temperature=1.0, top_p=0.3)
    b.set_row_sampler(2, mc.SAMPLER_GREEDY)
    set_value = (mc.SAMPLER_DEFAULT, 20, 1.0, np.float32(0.3))   # the caller's float, not the bfloat16 it is rounded to
    dec.launch_log(True)
    for args, words in (((4, mc.SAMPLER_GREEDY), "mc_row_sampler_set: row out of range"),
                        ((-1, mc.SAMPLER_GREEDY), "mc_row_sampler_set: row out of range"),
                        ((1, 7), "mc_row_sampler_set: unknown sampler"),
                        ((1, -2), "mc_row_sampler_set: unknown sampler"),
                        ((1, mc.SAMPLER_DEFAULT, 50, 0.0, 0.9), "nucleus_sampler: temperature must be positive"),
                        ((1, mc.SAMPLER_DEFAULT, 50, 0.6, 1.5), "nucleus_sampler: probability must be in [0.0, 1.0]"),
                        ((1, mc.SAMPLER_DEFAULT, 129, 0.6, 0.9), "topk_sampler: the fused sampler keeps 1..128 candidates"),
                        ((1, mc.SAMPLER_DEFAULT, 0, 0.6, 0.9), "topk_sampler: the fused sampler keeps 1..128 candidates")):
        refused(lambda: b.set_row_sampler(*args), words)
        assert dec.launched() == [], words
        assert b.row_sampler(1) == set_value, words
        assert b.row_sampler(2)[0] == mc.SAMPLER_GREEDY and b.row_sampler(0)[0] == b.row_sampler(3)[0] == mc.SAMPLER_INHERIT
    with pytest.raises(mc.McError) as e:
        b.row_sampler(4)
    assert e.value.status == 1 and "mc_row_sampler_get: row out of range" in str(e.value)
    b.set_row_sampler(1, mc.SAMPLER_INHERIT)
    assert b.row_sampler(1) == (mc.SAMPLER_INHERIT, None, None, None)
    b.set_row_sampler(1, mc.SAMPLER_DEFAULT, top_k=128, temperature=0.01, top_p=1.0)   # the ends of the ranges are admitted
    b.set_row_sampler(3, mc.SAMPLER_DEFAULT, top_k=1, temperature=100.0, top_p=0.0)
    b.reset_row_samplers()
    assert [b.row_sampler(r)[0] for r in range(4)] == [mc.SAMPLER_INHERIT] * 4
    assert dec.launched() == []
    b.release()
    dec.release()
