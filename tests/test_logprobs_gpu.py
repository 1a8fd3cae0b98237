"""Row log-probabilities (mc_logprobs_*, include/metalchat_hip.h Part 2n) on the device, on the SMALL model of test_batch_gpu.py
(V = 2048, one layer, int4 g128).  Every record is compared with the rule of tests/logprob_rule.py on the logits the batch
returns, under the part's condition: never more than 1 float32 ulp, bit-equal on at least 999 of 1000 finite values, ids exact.

  1. twin      after one step the records are the rule on logits(); the switch changes no token, logit or K / V bit
  2. chained   generate_rows with a stop id and an idle row equals stepwise step_rows record for record, the stop token's
               record is there, everything behind it and the idle row hold the fill; lockstep generate equals lockstep steps
  3. settings  greedy, default and draw rows, a row masked to 5 tokens and a penalised row: the records follow the processed logits
  4. contract  the same row alone, as row 3 of 4 and as row 16 of a wide 17: the same bits
  5. packed    prefill_rows and extend_rows record their one pick per row, rows outside the call hold the fill
  6. verify    verify_rows and verify_tree: a record per packed row, greedy and under set_verify_settings with a drawing row
  7. launches  off: the list of a fresh batch; on: exactly two more per token, directly behind the pick; off again: the old list
  8. refusals  each with its text"""
import numpy as np
import pytest

import logprob_rule as lpr
import modelgen as mg
import parity
from test_batch_gpu import SMALL, refused, small_decoder
from test_context_gpu import random_cache
from test_row_logits_gpu import configure, row, some_mask
from test_row_sampler_gpu import DEC, GREEDY, PAIRS, fresh, set_decoder
from test_rows_prefill_gpu import prompts_of

pytestmark = pytest.mark.gpu
V = SMALL["vocab"]
POS0 = 30
FILL = 0xFFFFFFFF
PARTS, FINISH = "mc_logprob_parts", "mc_logprob_finish"


@pytest.fixture(scope="module")
def small():
    return mg.make_model(SMALL, seed=11, quant="i4", group=128)


class Tally:
    """the 999-in-1000 condition over all the values one test compares"""

    def __init__(self):
        self.compared = self.differing = 0

    def record(self, bits, token, rec, top_n, what):
        """rec = (the token's lp, ids [top_n], lp [top_n]) against the rule on the row's logits `bits`"""
        tok, ids, lps = rec
        ids_want, lps_want = lpr.top(bits, top_n)
        assert np.asarray(ids).tolist() == ids_want.tolist(), f"{what}: the top ids"
        got = np.concatenate([[tok], lps]).astype(np.float32)
        want = np.concatenate([[lpr.logprobs(bits)[token]], lps_want]).astype(np.float32)
        n, k = lpr.check(got, want, what, share=False)
        self.compared, self.differing = self.compared + n, self.differing + k

    def done(self, what):
        assert self.compared > 0
        lpr.check_share(self.compared, self.differing, what)


def u32(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same_bits(a, b, what):
    for x, y, name in zip(a, b, ("token lp", "top ids", "top lp")):
        parity.exact(u32(x), u32(y), f"{what}: {name}")


def is_fill(rec):
    return bool((u32(rec[0]) == FILL).all() and (np.asarray(rec[1]) == -1).all() and (u32(rec[2]) == FILL).all())


def caches_of(B, seed=700):
    return [random_cache(SMALL, POS0, seed + r) for r in range(B)]


FIRST = np.array([5, 900, 1500, 31], np.int32)


# ------------------------------------------------------------------------------------------ 1
def test_twin(acc, small):
    B, top_n = 4, 5
    dec = small_decoder(acc, SMALL, small)
    caches = caches_of(B)
    b, twin = fresh(dec, caches), fresh(dec, caches)
    assert b.logprobs_setting() == (False, 0)
    b.set_logprobs(top_n)
    assert b.logprobs_setting() == (True, top_n) and twin.logprobs_setting() == (False, 0)
    tally = Tally()
    for name, call in (("lockstep", lambda x: x.step(FIRST, POS0)), ("ragged", lambda x: x.step_rows(FIRST, np.full(B, POS0, np.int32)))):
        nxt, want = call(b), call(twin)
        assert np.array_equal(nxt, want), name
        parity.exact(b.logits(), twin.logits(), f"{name}: the logits")
        for r in range(B):
            for x, y, kv in zip(b.export_row_kv(r, 0), twin.export_row_kv(r, 0), "KV"):
                parity.exact(x, y, f"{name} row {r}: {kv}")
        tok, ids, lps = b.logprobs(1)
        assert tok.shape == (1, B) and ids.shape == lps.shape == (1, B, top_n)
        logits = b.logits()
        for r in range(B):
            tally.record(logits[r], nxt[r], (tok[0, r], ids[0, r], lps[0, r]), top_n, f"{name} row {r}")
            assert ids[0, r, 0] == nxt[r] and tok[0, r] == lps[0, r, 0]     # a greedy pick is the most likely token
    tally.done("twin")
    for x in (b, twin, dec):
        x.release()


# ------------------------------------------------------------------------------------------ 2
def test_chained(acc, small):
    B, n, top_n = 4, 6, 3
    dec = small_decoder(acc, SMALL, small)
    caches = caches_of(B)
    pos = np.array([POS0, POS0, -1, POS0], np.int32)     # row 2 is idle
    # what the rows produce without a stop id: row 1's third token becomes the stop id
    scout = fresh(dec, caches)
    free, _ = scout.generate_rows(FIRST, pos, n)
    stop = int(free[2, 1])
    scout.release()
    # stepwise: one call per token, the host retires the rows that stopped
    b = fresh(dec, caches)
    b.set_logprobs(top_n)
    toks, p = FIRST.copy(), pos.copy()
    step_tokens = np.full((n, B), -1, np.int32)
    step_recs = []
    tally = Tally()
    for i in range(n):
        nxt = b.step_rows(toks, p)
        tok, ids, lps = b.logprobs(1)
        logits = b.logits()
        step_recs.append((tok[0].copy(), ids[0].copy(), lps[0].copy()))
        step_tokens[i] = nxt
        for r in range(B):
            if p[r] < 0:
                assert nxt[r] == -1 and is_fill((tok[0, r], ids[0, r], lps[0, r])), (i, r)
                continue
            tally.record(logits[r], nxt[r], (tok[0, r], ids[0, r], lps[0, r]), top_n, f"step {i} row {r}")
            if nxt[r] == stop:
                p[r] = -1
            else:
                p[r] += 1
                toks[r] = nxt[r]
        if (p < 0).all():
            break
    tally.done("stepwise")
    b.release()
    # chained: one call
    c = fresh(dec, caches)
    c.set_logprobs(top_n)
    got, lengths = c.generate_rows(FIRST, pos, n, stop=[stop])
    assert np.array_equal(got, step_tokens)
    assert lengths[1] <= 3 and got[lengths[1] - 1, 1] == stop and lengths[2] == 0 and lengths[0] > 0
    tok, ids, lps = c.logprobs(n)
    assert tok.shape == (n, B) and ids.shape == lps.shape == (n, B, top_n)
    for i in range(n):
        for r in range(B):
            rec = (tok[i, r], ids[i, r], lps[i, r])
            if i < lengths[r]:
                same_bits(rec, (step_recs[i][0][r], step_recs[i][1][r], step_recs[i][2][r]), f"token {i} row {r}")
                assert not is_fill(rec) and not np.isnan(tok[i, r])
            else:
                assert is_fill(rec), f"token {i} row {r}: a slot behind the stop (or of the idle row) must hold the fill"
    assert not np.isnan(tok[lengths[1] - 1, 1])     # the stop token's record
    c.release()
    # lockstep: generate against steps
    a, s = fresh(dec, caches), fresh(dec, caches)
    for x in (a, s):
        x.set_logprobs(top_n)
    chain = a.generate(FIRST, POS0, 3)
    whole = a.logprobs(3)
    toks = FIRST.copy()
    for i in range(3):
        nxt = s.step(toks, POS0 + i)
        assert np.array_equal(nxt, chain[i])
        same_bits(tuple(x[i] for x in whole), tuple(x[0] for x in s.logprobs(1)), f"lockstep token {i}")
        toks = nxt
    for x in (a, s, dec):
        x.release()


# ------------------------------------------------------------------------------------------ 3
def test_settings(acc, small):
    import metalchat_amd as mc

    B, top_n = 5, 20
    dec = small_decoder(acc, SMALL, small)
    set_decoder(dec, DEC)
    caches = caches_of(B)
    first = np.array([5, 900, 1500, 31, 77], np.int32)
    mask = some_mask(3, 5)
    assert mask.sum() == 5
    cfgs = [row(sampler=GREEDY), row(), row(sampler=GREEDY), row(mask=mask, sampler=GREEDY), row(pen=(1.3, 0.25, 0.5), prompt=[77, 77, 12], sampler=GREEDY)]
    b, raw = fresh(dec, caches), fresh(dec, caches)
    configure(b, cfgs)
    b.set_row_sampler(2, mc.SAMPLER_DRAW, top_k=40, temperature=0.9, top_p=0.95)
    b.set_seeds(mc.seed_pairs(np.random.default_rng(5), B))
    b.set_logprobs(top_n)
    pos = np.full(B, POS0, np.int32)
    nxt = b.step_rows(first, pos)
    raw.step_rows(first, pos)
    logits, unprocessed = b.logits(), raw.logits()
    assert not np.array_equal(logits[3], unprocessed[3]) and not np.array_equal(logits[4], unprocessed[4])
    parity.exact(logits[:3], unprocessed[:3], "the rows without processors")
    tok, ids, lps = b.logprobs(1)
    tally = Tally()
    for r in range(B):
        tally.record(logits[r], nxt[r], (tok[0, r], ids[0, r], lps[0, r]), top_n, f"row {r}")   # the PROCESSED logits
        assert np.isfinite(tok[0, r])
    tally.done("settings")
    # the masked row: its 5 allowed tokens in front, every banned id behind them with -inf
    allowed = mask[ids[0, 3]]
    assert allowed[:5].all() and not allowed[5:].any()
    assert np.isfinite(lps[0, 3, :5]).all() and np.isneginf(lps[0, 3, 5:]).all()
    assert ids[0, 3, 5:].tolist() == [t for t in range(V) if not mask[t]][:top_n - 5]     # the -inf tail in index order
    assert abs(float(np.exp(lps[0, 3, :5].astype(np.float64)).sum()) - 1.0) < 1e-6 and mask[nxt[3]]
    # the penalised row's records differ from what the raw logits would give
    assert lpr.logprobs(unprocessed[4])[nxt[4]] != tok[0, 4]
    for x in (b, raw, dec):
        x.release()


# ------------------------------------------------------------------------------------------ 4
def test_contract(acc, small):
    top_n = 20
    dec = small_decoder(acc, SMALL, small)
    kv = random_cache(SMALL, POS0, 4242)
    token = 1234
    recs = []
    for B, at, wide in ((1, 0, False), (4, 3, False), (17, 16, True)):
        caches = [random_cache(SMALL, POS0, 900 + r) for r in range(B)]
        caches[at] = kv
        b = fresh(dec, caches, wide=wide)
        b.set_logprobs(top_n)
        toks = np.array([(7 + 13 * r) % V for r in range(B)], np.int32)
        toks[at] = token
        pos = np.full(B, POS0, np.int32)
        if B > 1:
            pos[0] = POS0 - 3     # another row at another position
        nxt = b.step_rows(toks, pos)
        tok, ids, lps = b.logprobs(1)
        recs.append((nxt[at], tok[0, at].copy(), ids[0, at].copy(), lps[0, at].copy()))
        b.release()
    for other, name in zip(recs[1:], ("row 3 of 4", "row 16 of a wide 17")):
        assert other[0] == recs[0][0], name
        same_bits(other[1:], recs[0][1:], name)
    dec.release()


# ------------------------------------------------------------------------------------------ 5
def test_packed(acc, small):
    B, top_n = 4, 5
    dec = small_decoder(acc, SMALL, small)
    b = fresh(dec, [None] * B)
    b.set_logprobs(top_n)
    tally = Tally()
    prompts = prompts_of(SMALL, [9, 0, 21, 0], 3)
    nxt = b.prefill_rows([prompts[0], None, prompts[2], None])
    tok, ids, lps = b.logprobs(1)
    logits = b.logits()
    for r in range(B):
        rec = (tok[0, r], ids[0, r], lps[0, r])
        if r in (0, 2):
            tally.record(logits[r], nxt[r], rec, top_n, f"prefill row {r}")
        else:
            assert nxt[r] == -1 and is_fill(rec), f"prefill row {r}"
    refused(lambda: b.logprobs(2), "mc_logprobs_get: n must be the last call's n = 1")
    more = prompts_of(SMALL, [0, 0, 7, 0], 4)
    nxt = b.extend_rows([None, None, more[2], None], [0, 0, 21, 0])
    tok, ids, lps = b.logprobs(1)
    logits = b.logits()
    for r in range(B):
        rec = (tok[0, r], ids[0, r], lps[0, r])
        if r == 2:
            tally.record(logits[r], nxt[r], rec, top_n, f"extend row {r}")
        else:
            assert nxt[r] == -1 and is_fill(rec), f"extend row {r}"
    tally.done("packed")
    for x in (b, dec):
        x.release()


# ------------------------------------------------------------------------------------------ 6
@pytest.mark.parametrize("settings", [False, True])
def test_verify(acc, small, settings):
    import metalchat_amd as mc

    B, top_n = 4, 5
    dec = small_decoder(acc, SMALL, small)
    caches = caches_of(B)
    chunks = prompts_of(SMALL, [6, 0, 3, 0], 8)
    tree_parents = [np.array([-1, 0, 0, 1, 2, 3], np.int32), None, np.array([-1, 0, 1], np.int32), None]
    positions = np.array([POS0, -1, POS0, -1], np.int32)
    tally = Tally()
    for tree in (False, True):
        b = fresh(dec, caches)
        if settings:
            b.set_verify_settings(True)
            b.set_row_sampler(0, mc.SAMPLER_DRAW, top_k=40, temperature=0.9, top_p=0.95)
            b.set_row_mask(2, some_mask(9, V // 2))
            b.set_seeds(mc.seed_pairs(np.random.default_rng(6), 16 * B))
        b.set_logprobs(top_n)
        refused(b.verify_logprobs, "mc_logprobs_get_verify: no verify call with log-probabilities on this batch yet")
        call = [chunks[0], None, chunks[2], None]
        if tree:
            accepted, nxt, picks, paths = b.verify_tree(call, tree_parents, positions)
        else:
            accepted, nxt, picks = b.verify_rows(call, positions)
        logits, recs = b.verify_logits(), b.verify_logprobs()
        for r in range(B):
            if r not in (0, 2):
                assert recs[r] is None and picks[r] is None
                continue
            tok, ids, lps = recs[r]
            assert tok.shape == (len(chunks[r]),) and ids.shape == lps.shape == (len(chunks[r]), top_n)
            for j in range(len(chunks[r])):
                tally.record(logits[r][j], picks[r][j], (tok[j], ids[j], lps[j]), top_n, f"tree {tree} settings {settings} row {r} chunk row {j}")
                assert np.isfinite(tok[j])
            # the bonus token is one of the picks: its record is there
            last = paths[r][accepted[r]] if tree else accepted[r]
            assert picks[r][last] == nxt[r]
        b.release()
    tally.done("verify")
    dec.release()


# ------------------------------------------------------------------------------------------ 7
def test_launches(acc, small):
    B = 4
    dec = small_decoder(acc, SMALL, small)
    b = fresh(dec, caches_of(B))
    pos = np.array([POS0, -1, POS0, POS0], np.int32)

    def names_of(call):
        dec.launch_log(True)
        call()
        names = dec.launched()
        dec.launch_log(False)
        return names

    calls = {"step_rows": (lambda: b.step_rows(FIRST, pos), 1, "_rows_bfloat"), "generate_rows": (lambda: b.generate_rows(FIRST, pos, 3), 3, "_rows_bfloat"),
             "step": (lambda: b.step(FIRST, POS0), 1, "_bfloat"), "generate": (lambda: b.generate(FIRST, POS0, 3), 3, "_bfloat")}
    off = {k: names_of(c[0]) for k, c in calls.items()}
    for k, names in off.items():
        assert not [n for n in names if n.startswith("mc_logprob_")], k
    for top_n in (0, 20):
        b.set_logprobs(top_n)
        for k, (call, n, sfx) in calls.items():
            on = names_of(call)
            assert len(on) == len(off[k]) + 2 * n, (k, top_n)
            assert [x for x in on if not x.startswith("mc_logprob_")] == off[k], (k, top_n)
            at = [i for i, x in enumerate(on) if x == PARTS + sfx]
            assert len(at) == n and all(on[i + 1] == FINISH + sfx for i in at), (k, top_n)
            assert all(on[i - 1].startswith("mc_b_argmax") for i in at), (k, top_n, [on[i - 1] for i in at])   # directly behind the pick
            assert all(i + 2 == len(on) or on[i + 2] in ("mc_b_rows_begin", "mc_step_set") for i in at), (k, top_n)
    b.set_logprobs(enable=False)
    assert b.logprobs_setting()[0] is False
    for k, (call, n, sfx) in calls.items():
        assert names_of(call) == off[k], k
    for x in (b, dec):
        x.release()


# ------------------------------------------------------------------------------------------ 8
def test_refusals(acc, small):
    import metalchat_amd as mc

    B = 4
    dec = small_decoder(acc, SMALL, small)
    b = fresh(dec, caches_of(B))
    lib = mc.capi()
    for enable, top_n, text in ((2, 0, b"mc_logprobs_set: enable must be 0 or 1"), (-1, 0, b"mc_logprobs_set: enable must be 0 or 1"),
                                (1, 21, b"mc_logprobs_set: top_n must lie in [0, 20]"), (1, -1, b"mc_logprobs_set: top_n must lie in [0, 20]")):
        assert lib.mc_logprobs_set(b._h, enable, top_n) == 1 and lib.mc_last_error() == text
        assert b.logprobs_setting() == (False, 0)
    refused(lambda: b.logprobs(1), "mc_logprobs_get: log-probabilities are switched off (mc_logprobs_set)")
    refused(b.verify_logprobs, "mc_logprobs_get_verify: log-probabilities are switched off (mc_logprobs_set)")
    b.step(FIRST, POS0)                 # a call with the switch off leaves no record
    b.set_logprobs(0)
    refused(lambda: b.logprobs(1), "mc_logprobs_get: no step, generate or packed call with log-probabilities on this batch yet")
    refused(b.verify_logprobs, "mc_logprobs_get_verify: no verify call with log-probabilities on this batch yet")
    b.generate(FIRST, POS0, 2)
    refused(lambda: b.logprobs(1), "mc_logprobs_get: n must be the last call's n = 2")
    tok, ids, lps = b.logprobs(2)
    assert tok.shape == (2, B) and ids.shape == (2, B, 0) and np.isfinite(tok).all()
    out, top = np.zeros(2 * B, np.float32), np.zeros(2 * B, np.int32)
    import ctypes as C
    assert lib.mc_logprobs_get(b._h, 2, out.ctypes.data_as(C.POINTER(C.c_float)), top.ctypes.data_as(C.POINTER(C.c_int32)), None) == 1
    assert lib.mc_last_error() == b"mc_logprobs_get: top_n is 0, the top arrays must be null"
    assert lib.mc_logprobs_get(b._h, 2, None, None, None) == 1 and lib.mc_last_error() == b"mc_logprobs_get: null argument"
    b.set_logprobs(3)                   # a new setting drops the records of the old one
    refused(lambda: b.logprobs(2), "mc_logprobs_get: no step, generate or packed call with log-probabilities on this batch yet")
    b.step(FIRST, POS0)
    tok, ids, lps = b.logprobs(1)
    assert ids.shape == (1, B, 3) and (ids >= 0).all()
    for x in (b, dec):
        x.release()
