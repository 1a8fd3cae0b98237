"""Row logit processors (mc_row_mask_*, mc_row_penalty_*, include/metalchat_hip.h Part 2l) on the device: a row slot's token mask
and repetition / frequency / presence penalties, against the rule of tests/logits_rule.py on the raw logits of a twin batch that
carries nothing -- every comparison bit for bit.

  1  twin       after one step the processed rows' logits are the rule on the twin's, each pick is the row's own sampler on them,
                and the row with nothing set equals the twin's in tokens, logits and K / V;
  2  chained    a chained ragged call with a stop id and an idle row equals stepwise calls, which equal the rule step by step with
                the counts tracked on the host; the counts read back equal the host's;
  3  mask       with 5 allowed tokens every pick of 8 chained steps lies in the set: greedy, sampling and mixed batches;
  4  contract   the same row alone, as row 3 of 4 and as row 16 of a wide 17 gives the same bits;
  5  rolling    two steps past max_seq_len on a rolling batch;
  6  launches   nothing set (or everything reset or neutral): the launches of a fresh batch; one row set: one more, before the pick;
  7  packed     prefill_rows and extend_rows honour mask and penalties and leave the counts alone;
  8  refusals   every refusal with its text; verify calls look at the rows in the call."""
import numpy as np
import pytest

import logits_rule as lr
import modelgen as mg
import parity
from oracle import mc_oracle as mo
from test_batch_gpu import SMALL, refused, small_decoder
from test_context_gpu import random_cache
from test_row_sampler_gpu import DEC, GREEDY, PAIRS, S64, fresh, set_decoder

pytestmark = pytest.mark.gpu
BF16 = 0
V = SMALL["vocab"]
NEUTRAL = (1.0, 0.0, 0.0)


@pytest.fixture(scope="module")
def small():
    return mg.make_model(SMALL, seed=11, quant="i4", group=128)


def row(mask=None, pen=NEUTRAL, prompt=(), sampler=None):
    """a row slot's settings: mask (bool [V] or None), penalties, the tokens counted as its prompt, sampler (None: the decoder's)"""
    return dict(mask=mask, pen=pen, prompt=list(prompt), sampler=sampler)


def penalised(cfg):
    return tuple(cfg["pen"]) != NEUTRAL


def some_mask(seed, n_allowed, also=()):
    m = np.zeros(V, bool)
    m[np.random.default_rng(seed).choice(V, n_allowed, replace=False)] = True
    m[list(also)] = True
    return m


def configure(batch, cfgs, processors=True):
    """the rows' samplers, and (processors) their masks, penalties and prompts"""
    import metalchat_amd as mc

    for r, c in enumerate(cfgs):
        if c["sampler"] == GREEDY:
            batch.set_row_sampler(r, mc.SAMPLER_GREEDY)
        elif c["sampler"] is not None:
            batch.set_row_sampler(r, mc.SAMPLER_DEFAULT, *c["sampler"])
        if not processors:
            continue
        if c["mask"] is not None:
            batch.set_row_mask(r, c["mask"])
        if penalised(c):
            batch.set_row_penalties(r, *c["pen"])
        if c["prompt"]:
            batch.count_row_tokens(r, c["prompt"])


def host_counts(cfgs):
    counts = np.zeros((len(cfgs), V), np.int32)
    for r, c in enumerate(cfgs):
        np.add.at(counts[r], c["prompt"], 1)
    return counts


def rule(raw, cfg, counts):
    return lr.process(raw, counts if penalised(cfg) else None, cfg["mask"], *cfg["pen"])


def want_pick(bits, sampler, pair):
    sampler = sampler or DEC
    if sampler == GREEDY:
        return lr.first_max(bits)
    k, t, p = sampler
    return mo.sample_default(BF16, bits, top_k=k, temperature=t, top_p=p, init_state=pair[0], init_seq=pair[1])


def stepwise(dec, caches, cfgs, first, pos, n, stop=(), rolling=False, pairs=PAIRS):
    """n ragged steps, one call each, on a batch with cfgs next to a twin that carries the samplers only and is fed the same
    inputs; every step's processed logits and picks are checked against the rule with the counts tracked here.  Returns the
    tokens [n][B] (-1: idle), the host's counts and the batch."""
    B, S = len(caches), dec.cfg["max_seq_len"]
    b, twin = fresh(dec, caches, rolling=rolling), fresh(dec, caches, rolling=rolling)
    configure(b, cfgs)
    configure(twin, cfgs, processors=False)
    counts = host_counts(cfgs)
    toks, p = np.array(first, np.int32), np.array(pos, np.int32)
    out = np.full((n, B), -1, np.int32)
    for i in range(n):
        step_pairs = [pairs[(i * B + r) % len(pairs)] for r in range(B)]   # a step uses pair r % n_pairs: rotate the list
        b.set_seeds(step_pairs)
        active = [r for r in range(B) if p[r] >= 0]
        for r in active:
            if penalised(cfgs[r]):
                counts[r, toks[r]] += 1
        nxt = b.step_rows(toks, p)
        twin.step_rows(toks, p)
        raw, got = twin.logits(), b.logits()
        for r in range(B):
            if r not in active:
                assert nxt[r] == -1
                continue
            exp = rule(raw[r], cfgs[r], counts[r])
            parity.exact(got[r], exp, f"step {i} row {r}: the processed logits")
            assert nxt[r] == want_pick(exp, cfgs[r]["sampler"], step_pairs[r]), (i, r, nxt[r])
        out[i] = nxt
        for r in active:
            if nxt[r] in stop or (not rolling and p[r] + 1 >= S):
                p[r] = -1
            else:
                p[r] += 1
                toks[r] = nxt[r]
    twin.release()
    return out, counts, b


# ------------------------------------------------------------------------------------------ 1
def test_twin(acc, small):
    B, pos0 = 4, 30
    dec = small_decoder(acc, SMALL, small)
    set_decoder(dec, DEC)
    caches = [random_cache(SMALL, pos0, 700 + r) for r in range(B)]
    toks = np.array([5, 900, 1500, 31], np.int32)
    samplers = [None, GREEDY, (40, 0.9, 0.95), GREEDY]
    twin = fresh(dec, caches)
    configure(twin, [row(sampler=s) for s in samplers], processors=False)
    twin_next = twin.step(toks, pos0)
    raw = twin.logits()
    # the masks ban what the twin's rows would pick greedily; the prompts hold the input token and high logits
    top = [list(np.argsort(-mo.from_bf16(raw[r]).astype(np.float64), kind="stable")[:6]) for r in range(B)]
    m1, m3 = some_mask(1, V // 2, top[1][1:3]), some_mask(3, V // 3, top[3][2:4])
    m1[top[1][0]] = m3[top[3][0]] = False
    cfgs = [row(sampler=samplers[0]),
            row(mask=m1, prompt=[7, 7, 900], sampler=samplers[1]),
            row(pen=(1.3, 0.25, 0.5), prompt=[1500, 1500] + top[2][:3] + [9], sampler=samplers[2]),
            row(mask=m3, pen=(1.5, 0.125, 0.0), prompt=top[3][1:5] * 2, sampler=samplers[3])]
    b = fresh(dec, caches)
    configure(b, cfgs)
    nxt = b.step(toks, pos0)
    got = b.logits()
    counts = host_counts(cfgs)
    for r in (2, 3):
        counts[r, toks[r]] += 1
    for r in range(B):
        exp = rule(raw[r], cfgs[r], counts[r])
        parity.exact(got[r], exp, f"row {r}: the processed logits")
        assert nxt[r] == want_pick(exp, samplers[r], PAIRS[r % len(PAIRS)]), (r, nxt[r])
        parity.exact(b.row_token_counts(r), counts[r] if r != 1 else host_counts(cfgs)[1], f"row {r}: the counts")
    assert not np.array_equal(got[2], raw[2]) and not np.array_equal(got[3], raw[3])
    assert nxt[1] != top[1][0] and m1[nxt[1]] and nxt[3] != top[3][0] and m3[nxt[3]]
    # the row with nothing set: the twin's row
    assert nxt[0] == twin_next[0]
    parity.exact(got[0], raw[0], "row 0: logits")
    for a, t, name in zip(b.export_row_kv(0, 0), twin.export_row_kv(0, 0), "KV"):
        parity.exact(a, t, f"row 0: {name}")
    for x in (b, twin, dec):
        x.release()


# ------------------------------------------------------------------------------------------ 2
def chained_cfgs():
    return [row(pen=(1.3, 0.5, 0.25), prompt=[5, 5, 12], sampler=GREEDY),
            row(pen=(1.1, 0.25, 0.0), prompt=[900], sampler=(40, 0.9, 0.95)),
            row(mask=some_mask(2, V // 2), pen=(2.0, 0.0, 1.0), sampler=GREEDY),
            row(pen=(1.5, 0.5, 0.5), prompt=[31, 32, 32], sampler=GREEDY)]   # idle: its counts stay


def test_chained(acc, small):
    lens, n = [30, 41, 7, 60], 8
    dec = small_decoder(acc, SMALL, small)
    set_decoder(dec, DEC)
    caches = [random_cache(SMALL, m, 800 + r) for r, m in enumerate(lens)]
    first = np.array([5, 900, 1500, 31], np.int32)
    pos = np.array(lens, np.int32)
    pos[3] = -1
    cfgs = chained_cfgs()
    free, _, fb = stepwise(dec, caches, cfgs, first, pos, 3)
    fb.release()
    stop = int(free[2, 1])   # row 1 stops on its third token
    want, counts, sb = stepwise(dec, caches, cfgs, first, pos, n, stop=[stop])
    assert (want[3:, 1] == -1).all() and want[2, 1] == stop and (want[:, 3] == -1).all()
    assert (want[:, 0] >= 0).sum() >= 3 and (want[:, 2] >= 0).sum() >= 3
    b = fresh(dec, caches)
    configure(b, cfgs)
    got, produced = b.generate_rows(first, pos, n, stop=[stop])
    assert np.array_equal(got, want), (got, want)
    assert list(produced) == [int((want[:, r] >= 0).sum()) for r in range(4)]
    parity.exact(b.logits()[0], sb.logits()[0], "the last step's logits of row 0")
    for r in range(4):
        parity.exact(b.row_token_counts(r), counts[r], f"chained: row {r}'s counts")
        parity.exact(sb.row_token_counts(r), counts[r], f"stepwise: row {r}'s counts")
    parity.exact(counts[3], host_counts(cfgs)[3], "the idle row counted nothing")
    # every pick of the chained call was counted before the next pick: the row's inputs, once each
    inputs0 = [int(first[0])] + [int(t) for t in got[:-1, 0] if t >= 0][: int(produced[0]) - 1]
    exp0 = host_counts(cfgs)[0]
    np.add.at(exp0, inputs0, 1)
    parity.exact(counts[0], exp0, "row 0's counts: its prompt and its step inputs")
    b.clear_row_counts(0)
    assert not b.row_token_counts(0).any() and np.array_equal(b.row_token_counts(1), counts[1])
    for x in (b, sb, dec):
        x.release()


def test_lockstep_chained_equals_ragged(acc, small):
    """mc_batch_generate counts and penalises as mc_ragged_generate does at equal positions: tokens, logits and counts"""
    B, n, pos0 = 3, 5, 30
    dec = small_decoder(acc, SMALL, small)
    set_decoder(dec, DEC)
    caches = [random_cache(SMALL, pos0, 700 + r) for r in range(B)]
    first = np.array([5, 900, 1500], np.int32)
    cfgs = [row(pen=(1.3, 0.5, 0.25), prompt=[5, 12], sampler=GREEDY), row(mask=some_mask(4, V // 2), pen=(1.1, 0.25, 0.5)), row()]
    lock, ragged = fresh(dec, caches), fresh(dec, caches)
    configure(lock, cfgs)
    configure(ragged, cfgs)
    dec.launch_log(True)
    got = lock.generate(first, pos0, n)
    names = dec.launched()
    dec.launch_log(False)
    assert names.count("mc_b_logits_process_bfloat") == n and "mc_b_logits_process_rows_bfloat" not in names
    want, _ = ragged.generate_rows(first, [pos0] * B, n)
    assert np.array_equal(got, want), (got, want)
    parity.exact(lock.logits(), ragged.logits(), "the last step's logits")
    for r in range(B):
        exp = host_counts(cfgs)[r]
        if penalised(cfgs[r]):
            np.add.at(exp, [int(first[r])] + [int(t) for t in got[:-1, r]], 1)
        parity.exact(lock.row_token_counts(r), exp, f"lockstep: row {r}'s counts")
        parity.exact(ragged.row_token_counts(r), exp, f"ragged: row {r}'s counts")
    for x in (lock, ragged, dec):
        x.release()


# ------------------------------------------------------------------------------------------ 3
def test_mask_property(acc, small):
    B, n, pos0 = 3, 8, 30
    dec = small_decoder(acc, SMALL, small)
    caches = [random_cache(SMALL, pos0, 700 + r) for r in range(B)]
    first = np.array([5, 900, 1500], np.int32)
    allowed = [some_mask(40 + r, 5) for r in range(B)]
    for what, decoder, samplers, pick in (("greedy", GREEDY, [None] * 3, "mc_b_argmax"), ("sampling", DEC, [None] * 3, "mc_b_sample"),
                                          ("mixed", DEC, [GREEDY, None, (128, 4.0, 1.0)], "mc_b_pick_mixed")):
        set_decoder(dec, decoder)
        for ragged in (False, True):
            b = fresh(dec, caches)
            configure(b, [row(mask=allowed[r], sampler=samplers[r]) for r in range(B)])
            dec.launch_log(True)
            got = b.generate_rows(first, [pos0] * B, n)[0] if ragged else b.generate(first, pos0, n)
            names = dec.launched()
            dec.launch_log(False)
            assert [x for x in names if x.startswith(pick)], (what, sorted(set(names)))
            assert got.shape == (n, B)
            for r in range(B):
                assert allowed[r].sum() == 5 and allowed[r][got[:, r]].all(), (what, ragged, r, got[:, r], np.flatnonzero(allowed[r]))
            b.release()
    dec.release()


# ------------------------------------------------------------------------------------------ 4
def test_contract(acc, small):
    pos0, n = 30, 3
    dec = small_decoder(acc, SMALL, small)
    set_decoder(dec, GREEDY)
    mine = random_cache(SMALL, pos0, 1234)
    me = row(mask=some_mask(9, V // 2), pen=(1.3, 0.5, 0.25), prompt=[77, 77, 400, 3], sampler=(40, 1.5, 0.95))
    others = [row(), row(mask=some_mask(10, 5), sampler=GREEDY), row(pen=(2.0, 1.0, 1.0), prompt=[77, 400], sampler=(5, 0.9, 0.5))]
    seen = []
    for B, at, wide in ((1, 0, False), (4, 3, False), (17, 16, True)):
        caches = [random_cache(SMALL, pos0, 700 + r) for r in range(B)]
        caches[at] = mine
        cfgs = [others[r % 3] for r in range(B)]
        cfgs[at] = me
        b = fresh(dec, caches, wide=wide)
        b.set_seeds([PAIRS[2]])   # one pair: every row and step draws from it, whatever B is
        configure(b, cfgs)
        first = (np.arange(B, dtype=np.int32) * 113 + 5) % V
        first[at] = 77
        toks, _ = b.generate_rows(first, [pos0] * B, n)
        seen.append((toks[:, at].copy(), b.logits()[at].copy(), b.row_token_counts(at), *b.export_row_kv(at, 0)))
        b.release()
    for other, where in zip(seen[1:], ("row 3 of 4", "row 16 of 17")):
        for a, o, name in zip(seen[0], other, ("tokens", "logits", "counts", "K", "V")):
            parity.exact(o, a, f"{where} against the row alone: {name}")
    assert (seen[0][0] >= 0).all() and seen[0][2].sum() == 4 + n
    dec.release()


# ------------------------------------------------------------------------------------------ 5
def test_rolling(acc, small):
    S = S64["max_seq_len"]
    dec = small_decoder(acc, S64, small)
    set_decoder(dec, DEC)
    caches = [random_cache(S64, S - 1, 900 + r) for r in range(3)]
    first = np.array([5, 900, 1500], np.int32)
    cfgs = [row(), row(mask=some_mask(5, V // 2), pen=(1.3, 0.5, 0.25), prompt=[900, 1], sampler=GREEDY), row(pen=(1.2, 0.0, 0.5))]
    want, counts, sb = stepwise(dec, caches, cfgs, first, [S - 1] * 3, 3, rolling=True)
    assert (want >= 0).all()   # positions S - 1, S and S + 1
    b = fresh(dec, caches, rolling=True)
    configure(b, cfgs)
    got, _ = b.generate_rows(first, [S - 1] * 3, 3)
    assert np.array_equal(got, want), (got, want)
    assert list(b.lengths()) == [S + 2] * 3
    for r in range(3):
        parity.exact(b.row_token_counts(r), counts[r], f"row {r}'s counts")
        parity.exact(b.logits()[r], sb.logits()[r], f"row {r}'s logits")
    for x in (b, sb, dec):
        x.release()


# ------------------------------------------------------------------------------------------ 6
def test_launches(acc, small):
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

    for ragged, sfx in ((False, "_bfloat"), (True, "_rows_bfloat")):
        for setting, npick in ((GREEDY, 1), (DEC, 2)):
            set_decoder(dec, setting)
            base = log(fresh(dec, caches), ragged)
            assert not [x for x in base if x.startswith("mc_b_logits_process")], base
            b = fresh(dec, caches)
            assert log(b, ragged) == base, "nothing set"
            b.set_row_penalties(2, 1.0, 0.0, 0.0)
            b.count_row_tokens(2, [5, 6])
            assert log(b, ragged) == base, "neutral penalties and counts alone"
            b.set_row_mask(1, [3, 4, 5])
            one = log(b, ragged)
            assert one.count("mc_b_logits_process" + sfx) == 1 and len([x for x in one if x.startswith("mc_b_logits_process")]) == 1, one
            assert one.index("mc_b_logits_process" + sfx) == len(base) - npick, "in front of the pick, behind the head"
            assert [x for x in one if not x.startswith("mc_b_logits_process")] == base
            b.set_row_penalties(3, 1.2, 0.0, 0.0)
            assert log(b, ragged) == one, "two rows set: still one launch"
            b.reset_row_logits()
            assert log(b, ragged) == base, "after reset_row_logits"
            assert b.row_mask(1) is None and b.row_penalties(3) == NEUTRAL and not b.row_token_counts(2).any()
            b.set_row_mask(0, [1])
            b.set_row_penalties(0, 1.0, 0.5, 0.0)
            assert log(b, ragged) == one
            b.set_row_mask(0, None)
            b.set_row_penalties(0)
            assert log(b, ragged) == base, "every mask removed and every penalty neutral"
            b.release()
    dec.release()


# ------------------------------------------------------------------------------------------ 7
def test_packed_passes(acc, small):
    rng = np.random.default_rng(21)
    dec = small_decoder(acc, SMALL, small)
    set_decoder(dec, GREEDY)
    prompts = [rng.integers(0, V, n).astype(np.int32) for n in (5, 17, 33)]
    chunks = [rng.integers(0, V, n).astype(np.int32) for n in (3, 2, 4)]
    cfgs = [row(mask=some_mask(70, 5)), row(mask=some_mask(71, 5), pen=(1.5, 0.5, 0.5), prompt=list(range(0, V, 3))),
            row(pen=(1.25, 0.25, 1.0), prompt=list(range(0, V, 2)))]
    b, twin = fresh(dec, [None] * 3), fresh(dec, [None] * 3)
    configure(b, cfgs)
    counts = host_counts(cfgs)
    dec.launch_log(True)
    for call, args in (("prefill_rows", (prompts,)), ("extend_rows", (chunks, [len(p) for p in prompts]))):
        nxt = getattr(b, call)(*args)
        getattr(twin, call)(*args)
        raw, got = twin.logits(), b.logits()
        for r in range(3):
            exp = rule(raw[r], cfgs[r], counts[r])
            parity.exact(got[r], exp, f"{call} row {r}: the processed logits")
            assert nxt[r] == lr.first_max(exp), (call, r, nxt[r])
            assert cfgs[r]["mask"] is None or cfgs[r]["mask"][nxt[r]], (call, r, nxt[r])
            parity.exact(b.row_token_counts(r), counts[r], f"{call} row {r}: the counts stay")
        assert not np.array_equal(got[2], raw[2])
    names = dec.launched()
    dec.launch_log(False)
    assert names.count("mc_b_logits_process_rows_bfloat") == 2 and "mc_b_logits_process_bfloat" not in names
    for x in (b, twin, dec):
        x.release()


# ------------------------------------------------------------------------------------------ 8
def test_refusals(acc, small):
    import ctypes as C

    import metalchat_amd as mc
    from metalchat_amd import runtime

    dec = small_decoder(acc, SMALL, small)
    set_decoder(dec, GREEDY)
    b = mc.Batch(dec, 3)
    lib, h, nw = runtime.capi(), b._h, (V + 31) // 32
    u32p, i32p = C.POINTER(C.c_uint32), C.POINTER(C.c_int32)
    keep = some_mask(1, 9)
    b.set_row_mask(1, keep)
    b.set_row_penalties(1, 1.5, 0.25, -0.5)
    b.count_row_tokens(1, [4, 4, 2047])
    words = lr.mask_words(keep)
    none = np.zeros(nw, np.uint32)
    ids = np.array([1, 2, V, 3], np.int32)
    neg = np.array([1, -1], np.int32)
    inf, nan = float("inf"), float("nan")
    dec.launch_log(True)
    cases = [
        (lambda: lib.mc_row_mask_set(h, 3, words.ctypes.data_as(u32p), nw), "mc_row_mask_set: row out of range"),
        (lambda: lib.mc_row_mask_set(h, -1, words.ctypes.data_as(u32p), nw), "mc_row_mask_set: row out of range"),
        (lambda: lib.mc_row_mask_set(h, 1, words.ctypes.data_as(u32p), nw - 1), "mc_row_mask_set: n_words"),
        (lambda: lib.mc_row_mask_set(h, 1, words.ctypes.data_as(u32p), nw + 1), "mc_row_mask_set: n_words"),
        (lambda: lib.mc_row_mask_set(h, 1, none.ctypes.data_as(u32p), nw), "mc_row_mask_set: the mask allows no token"),
        (lambda: lib.mc_row_mask_get(h, 3, C.byref(C.c_int32()), None, 0), "mc_row_mask_get: row out of range"),
        (lambda: lib.mc_row_mask_get(h, 1, C.byref(C.c_int32()), none.ctypes.data_as(u32p), nw - 1), "mc_row_mask_get: n_words"),
        (lambda: lib.mc_row_penalty_set(h, 3, 1.0, 0.0, 0.0), "mc_row_penalty_set: row out of range"),
        (lambda: lib.mc_row_penalty_set(h, 1, 0.0, 0.0, 0.0), "mc_row_penalty_set: repetition must be finite and positive"),
        (lambda: lib.mc_row_penalty_set(h, 1, -1.0, 0.0, 0.0), "mc_row_penalty_set: repetition must be finite and positive"),
        (lambda: lib.mc_row_penalty_set(h, 1, inf, 0.0, 0.0), "mc_row_penalty_set: repetition must be finite and positive"),
        (lambda: lib.mc_row_penalty_set(h, 1, nan, 0.0, 0.0), "mc_row_penalty_set: repetition must be finite and positive"),
        (lambda: lib.mc_row_penalty_set(h, 1, 1.0, inf, 0.0), "mc_row_penalty_set: frequency must be finite"),
        (lambda: lib.mc_row_penalty_set(h, 1, 1.0, nan, 0.0), "mc_row_penalty_set: frequency must be finite"),
        (lambda: lib.mc_row_penalty_set(h, 1, 1.0, 0.0, -inf), "mc_row_penalty_set: presence must be finite"),
        (lambda: lib.mc_row_penalty_set(h, 1, 1.0, 0.0, nan), "mc_row_penalty_set: presence must be finite"),
        (lambda: lib.mc_row_penalty_get(h, 3, None, None, None), "mc_row_penalty_get: row out of range"),
        (lambda: lib.mc_row_penalty_count(h, 3, ids.ctypes.data_as(i32p), 1), "mc_row_penalty_count: row out of range"),
        (lambda: lib.mc_row_penalty_count(h, 1, None, 2), "mc_row_penalty_count: null argument"),
        (lambda: lib.mc_row_penalty_count(h, 1, ids.ctypes.data_as(i32p), -1), "mc_row_penalty_count: n must not be negative"),
        (lambda: lib.mc_row_penalty_count(h, 1, ids.ctypes.data_as(i32p), 4), f"mc_row_penalty_count: token 2 (id {V}) is outside the vocabulary"),
        (lambda: lib.mc_row_penalty_count(h, 1, neg.ctypes.data_as(i32p), 2), "mc_row_penalty_count: token 1 (id -1) is outside the vocabulary"),
        (lambda: lib.mc_row_penalty_counts(h, 3, ids.ctypes.data_as(i32p)), "mc_row_penalty_counts: row out of range"),
        (lambda: lib.mc_row_penalty_clear(h, -1), "mc_row_penalty_clear: row out of range"),
    ]
    want_counts = np.zeros(V, np.int32)
    want_counts[[4, 2047]] = [2, 1]
    for call, text in cases:
        assert call() == 1, text
        assert lib.mc_last_error().decode().startswith(text), (text, lib.mc_last_error())
        assert dec.launched() == [], text
        assert np.array_equal(b.row_mask(1), keep) and b.row_penalties(1) == (1.5, 0.25, -0.5), text
        assert np.array_equal(b.row_token_counts(1), want_counts), text
        assert b.row_mask(0) is None and b.row_penalties(2) == NEUTRAL and not b.row_token_counts(0).any(), text
    dec.launch_log(False)
    # what is admitted: a null tokens with n = 0, bits at and above vocab are ignored, ids as an iterable
    assert lib.mc_row_penalty_count(h, 1, None, 0) == 0
    b.set_row_mask(2, {3, 4, 2047})
    assert list(np.flatnonzero(b.row_mask(2))) == [3, 4, 2047]
    b.set_row_mask(2, None)
    assert b.row_mask(2) is None
    with pytest.raises(ValueError):
        b.set_row_mask(2, [V])
    b.release()

    # verify calls: a row in the call with a mask or penalties is refused, outside the call it does not matter
    rng = np.random.default_rng(5)
    prompts = [rng.integers(0, V, n).astype(np.int32) for n in (12, 20, 7)]
    lens = [len(p) for p in prompts]
    drafts = [rng.integers(0, V, n).astype(np.int32) for n in (4, 6, 3)]
    chain = [np.arange(-1, len(d) - 1, dtype=np.int32) for d in drafts]
    for tree in (False, True):
        who = "mc_tree_verify" if tree else "mc_verify_rows"
        verify = (lambda b, rows: b.verify_tree([drafts[r] if r in rows else None for r in range(3)],
                                                [chain[r] if r in rows else None for r in range(3)], lens)[:3]) if tree else \
                 (lambda b, rows: b.verify_rows([drafts[r] if r in rows else None for r in range(3)], lens))
        plain = mc.Batch(dec, 3)
        plain.prefill_rows(prompts)
        want = verify(plain, (0, 1))
        for setting in ("mask", "penalties"):
            b = mc.Batch(dec, 3)
            b.prefill_rows(prompts)
            if setting == "mask":
                b.set_row_mask(2, [1, 2, 3])
            else:
                b.set_row_penalties(2, 1.0, 0.0, 0.5)
            before = list(b.lengths())
            dec.launch_log(True)
            with pytest.raises(mc.McError) as e:
                verify(b, (0, 1, 2))
            assert e.value.status == 1 and str(e.value).endswith(
                who + ": row 2: the row has a token mask or penalties (a verify call would need them per chunk row)"), str(e.value)
            assert dec.launched() == [] and list(b.lengths()) == before
            dec.launch_log(False)
            got = verify(b, (0, 1))
            for g, w, name in zip(got, want, ("accepted", "next_tokens", "picks")):
                for r in range(3):
                    assert np.array_equal(g[r], w[r]) if g[r] is not None else w[r] is None, (tree, setting, name, r)
            b.release()
            plain.release()
            plain = mc.Batch(dec, 3)
            plain.prefill_rows(prompts)
        plain.release()
    dec.release()
