"""MC_SAMPLER_DRAW (include/metalchat_hip.h Part 2, DESIGN.md s.4 "A sampler that draws") on the device, bit for bit against tests/draw_rule.py:

  * the kernels launched by name -- mc_topk_candidates_T + mc_draw_T on crafted rows, 64 seed pairs a row: the pick and all seven taps;
  * the batch-1 decoder: chained == stepwise, every token the rule on that step's logits, the taps the chain's;
  * the batch row contract with draw rows beside greedy and default ones, through every call a pick is made in;
  * the launch forms; best-of-n after one prompt pass; a draw row with a token mask; the refusals."""
import functools

import numpy as np
import pytest

import draw_rule
import modelgen as mg
import parity
from oracle import mc_oracle as mo
from test_batch_gpu import SMALL, refused, small_decoder
from test_context_gpu import random_cache

pytestmark = pytest.mark.gpu
BF16, F32 = 0, 1
TN = {BF16: "bfloat", F32: "float"}
GREEDY_K, DEFAULT_K, DRAW_K = 0, 1, 2                       # (= mc.SAMPLER_*; asserted in test_refusals)
GREEDY = (GREEDY_K,)
DEC = (DRAW_K, 50, 0.6, 0.9)                                # the decoder's sampler while a mixed batch runs (no row inherits it)
SETTINGS = [GREEDY, (DRAW_K, 40, 0.9, 0.95), (DEFAULT_K, 5, 1.5, 0.5), (DRAW_K, 5, 1.5, 0.5)]   # row r takes SETTINGS[r % 4]
PAIRS = [(1000 + 17 * i, 77 + i) for i in range(5)]
S64 = dict(SMALL, max_seq_len=64)
TAPS = ["scaled", "probs", "sorted", "cumsum", "diff", "masked", "ids"]


@pytest.fixture(scope="module")
def small():
    return mg.make_model(SMALL, seed=11, quant="i4", group=128)


def rule(logits, setting, pair, dt=BF16, **kw):
    return draw_rule.draw(dt, logits, setting[1], setting[2], setting[3], pair[0], pair[1], **kw)


# ------------------------------------------------------------------------------------------ 4: the kernels by name
KERNEL_NS, KERNEL_KS = [1000, 2048, 5000], [1, 5, 50, 128]   # one partial chunk, whole chunks, several lists with a tail
KERNEL_SETTING = {1: (0.9, 0.95), 5: (1.5, 0.9), 50: (1.0, 0.95), 128: (1.2, 0.98)}
KERNEL_PAIRS = [(3 + 1009 * i, 2**40 + 7 * i) for i in range(64)]
SP = np.dtype([("k", np.uint32), ("ncand", np.uint32), ("cap", np.uint32), ("inv_temp", np.float32),
               ("top_p", np.float32), ("nlists", np.uint32), ("kpad", np.uint32)])


def crafted_rows(dt, n, k):
    """three rows: plain, exact ties (at the maximum and through the body), and one whose nucleus keeps a single entry"""
    rng = np.random.default_rng(7 * n + k + dt)
    plain = rng.normal(0, 1.5, n).astype(np.float32)
    ties = np.round(rng.normal(0, 1.5, n) * 2).astype(np.float32) / 2
    ties[rng.integers(0, n, 3)] = ties.max()
    single = rng.normal(0, 1.0, n).astype(np.float32)
    single[n - 3] = 40.0
    return [mo.encode(dt, x) for x in (plain, ties, single)]


@functools.lru_cache(maxsize=None)
def kernel_reference(dt, n, k):
    """per crafted row: (logits, tokens[64], positions[64], taps) by the rule -- computed once, shared by the tests below"""
    t, p = KERNEL_SETTING[k]
    return [(x,) + draw_rule.draw_many(dt, x, KERNEL_PAIRS, k, t, p) for x in crafted_rows(dt, n, k)]


def launch_draw(acc, dt, logits, top_k, temperature, top_p, pairs, kernel="mc_draw"):
    """decoder.cc run_head()'s two launches with its geometry (sampler_plan.h); launch 2 once per pair: state i carries step_index i, so launch
    i draws with pair i and fills tokens_out[i].  Returns the tokens and the taps of the first and the last launch."""
    import metalchat_amd as mc

    n = logits.size
    k = min(top_k, n)
    kpad = 1
    while kpad < top_k:
        kpad *= 2
    chunk = max(512, kpad)
    lists = -(-n // chunk)
    assert lists <= 1024
    cand = acc.alloc(lists * kpad * 8)
    mc.KernelTask(acc.load("mc_topk_candidates", TN[dt]), (lists * 64, 1, 1), (64, 1, 1),
                  [acc.to_device(logits), np.uint32(n), np.uint32(kpad), cand, np.uint32(chunk)])()
    rt = (lambda v: float(mo.decode(dt, mo.encode(dt, np.array([v], np.float32)))[0]))
    p = np.zeros(1, SP)
    p["k"], p["ncand"], p["cap"], p["nlists"], p["kpad"] = k, lists * kpad, 4096, lists, kpad
    p["inv_temp"], p["top_p"] = rt(1.0 / rt(temperature)), rt(top_p)
    states = np.zeros((len(pairs), 12), np.int32)   # abi.h step_state: 12 words, word 5 = step_index
    states[:, 5] = np.arange(len(pairs))
    sb = acc.to_device(states)
    toks = acc.to_device(np.full(len(pairs), -1, np.int32))
    taps = [acc.to_device(np.full(7 * k, np.nan, np.float32)) for _ in range(2)]
    seeds = acc.to_device(np.array(pairs, np.uint64).reshape(-1))
    kern = acc.load(kernel, TN[dt])
    for i in range(len(pairs)):
        tp = taps[0] if i == 0 else (taps[1] if i == len(pairs) - 1 else None)
        mc.KernelTask(kern, (128, 1, 1), (128, 1, 1), [cand, p, seeds, np.uint32(len(pairs)), (sb, 48 * i), toks, tp], lds_bytes=4096 * 8)()
    acc.wait()
    picked = sb.download(np.int32, states.size).reshape(states.shape)[:, 0]
    out = toks.download(np.int32, len(pairs))
    assert np.array_equal(picked, out)   # the pick goes to the state's token and to tokens_out[step_index]
    return out, [t.download(np.float32, 7 * k).reshape(7, k) for t in taps]


def test_the_crafted_rows_draw():
    """The condition on the inputs (CPU, by the rule): over the cases with k >= 5 a position above 0 is drawn in at least a quarter of the
    (row, pair) combinations and at least 4 distinct positions occur -- without it the kernel test would pass on MC_SAMPLER_DEFAULT too."""
    pos = np.concatenate([r[2] for dt in (BF16, F32) for n in KERNEL_NS for k in KERNEL_KS if k >= 5 for r in kernel_reference(dt, n, k)])
    print("positions above 0:", float((pos > 0).mean()), "distinct:", len(set(pos.tolist())))
    assert (pos > 0).mean() >= 0.25 and len(set(pos.tolist())) >= 4
    for dt in (BF16, F32):
        for n in KERNEL_NS:
            for k in KERNEL_KS:
                plain, ties, single = kernel_reference(dt, n, k)
                assert (single[3][5] > 0).sum() == 1 and (single[2] == 0).all()         # the nucleus keeps a single entry
                assert len(np.unique(ties[3][0])) < k or k == 1                          # exact ties among the k best


@pytest.mark.parametrize("k", KERNEL_KS)
@pytest.mark.parametrize("n", KERNEL_NS)
@pytest.mark.parametrize("dt", [BF16, F32])
def test_draw_kernels_are_the_rule(acc, dt, n, k):
    t, p = KERNEL_SETTING[k]
    for name, (logits, want, _, otaps) in zip(("plain", "ties", "single"), kernel_reference(dt, n, k)):
        got, taps = launch_draw(acc, dt, logits, k, t, p, KERNEL_PAIRS)
        for which in taps:
            for r in range(7):
                parity.exact(which[r], otaps[r], f"{TN[dt]} n{n} k{k} {name}: tap '{TAPS[r]}'")
        assert np.array_equal(got, want), (TN[dt], n, k, name, got, want)


# ------------------------------------------------------------------------------------------ 5: the batch-1 decoder
@pytest.mark.parametrize("dt", [F32, BF16])
def test_decoder_chained_equals_stepwise_equals_the_rule(acc, dt):
    import metalchat_amd as mc

    n, setting = 12, (DRAW_K, 50, 1.0, 0.95)
    pairs = [(500 + 31 * i, 9 + i) for i in range(n)]
    cfg = mg.tiny_cfg(dt, max_seq_len=32)
    w = mg.make_model(cfg, seed=61, quant="i4", group=32)
    dec = mc.Decoder(acc, **mg.decoder_kwargs(cfg, weight_format=2, group_size=32))
    dec.load_model(w)
    dec.set_taps(True)
    dec.set_sampler(*setting)
    dec.launch_log(True)
    tok, stepped, above = 3, [], 0
    for pos in range(n):
        dec.set_seeds([pairs[pos]])
        got = dec.step(tok, pos)
        want, otaps, at = rule(dec.logits(), setting, pairs[pos], dt, taps=True, with_pos=True)
        assert got == want, (pos, got, want)
        parity.exact(dec.sampler_taps(), otaps, f"pos {pos} sampler taps")
        above += at > 0
        stepped.append(got)
        tok = got
    names = dec.launched()
    dec.launch_log(False)
    assert names.count("mc_draw_" + TN[dt]) == n and not [x for x in names if x.startswith(("mc_sample", "mc_argmax"))], sorted(set(names))
    assert above >= 2, "the pairs chosen draw above position 0 (checked by the rule)"
    for graph in (0, 1):   # chained on the device: token i with pair i
        d2 = mc.Decoder(acc, **mg.decoder_kwargs(cfg, weight_format=2, group_size=32, use_graph=graph))
        d2.load_model(w)
        d2.set_sampler(*setting)
        d2.set_seeds(pairs)
        assert list(d2.generate(3, 0, n)) == stepped
        d2.set_sampler(mc.SAMPLER_GREEDY)
        d2.release()
    dec.set_sampler(mc.SAMPLER_GREEDY)
    refused(lambda: dec.sampler_taps(), "decoder: the default sampler is not active")
    dec.release()


# ------------------------------------------------------------------------------------------ 6: the batch row contract
def effective(r):
    return SETTINGS[r % 4]


def set_decoder(dec, setting):
    dec.set_sampler(*setting)


def set_rows(batch):
    for r in range(batch.B):
        batch.set_row_sampler(r, *effective(r))


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


def mixed_against_uniform(dec, caches, call, what, last_i, wide=False, rolling=False):
    """call(batch) -> int array [n][B].  Runs it on a batch with SETTINGS, then once per distinct setting on a batch without row samplers under a
    decoder set to it: the rows with that setting agree in their tokens, last logits and K / V, bit for bit.  And the last token of every draw row
    still active is the rule on the row's own last logits with pair (last_i * B + r) % n_pairs.  Returns the mixed batch's tokens and launches."""
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
    assert not [n for n in names if n.startswith(("mc_b_argmax", "mc_b_sample", "mc_draw"))], (what, sorted(set(names)))
    lengths = mixed.lengths()
    logits = mixed.logits()
    checked = 0
    for r in range(B):
        if effective(r)[0] == DRAW_K and got[-1, r] >= 0:
            want = rule(logits[r], effective(r), PAIRS[(last_i * B + r) % len(PAIRS)])
            assert got[-1, r] == want, (what, r, got[-1, r], want)
            checked += 1
    assert checked >= 1, what
    for setting in dict.fromkeys(effective(r) for r in range(B)):
        set_decoder(dec, setting)
        uniform = fresh(dec, caches, wide, rolling)
        want = np.asarray(call(uniform))
        for r in (r for r in range(B) if effective(r) == setting):   # (the other rows pick otherwise here, and may stop elsewhere)
            assert uniform.lengths()[r] == lengths[r], (what, setting, r)
            assert np.array_equal(got[:, r], want[:, r]), (what, r, setting, got[:, r], want[:, r])
            parity.exact(logits[r], uniform.logits()[r], f"{what} row {r}: logits")
            for a, b_, name in zip(mixed.export_row_kv(r, 0), uniform.export_row_kv(r, 0), "KV"):
                assert a.shape[0] == min(lengths[r], dec.cfg["max_seq_len"])
                parity.exact(a, b_, f"{what} row {r} under {setting}: {name}")
        uniform.release()
    mixed.release()
    return got, names


def test_mixed_equals_uniform_and_every_draw_is_the_rule(acc, small):
    B, n, pos0 = 4, 8, 30
    dec = small_decoder(acc, SMALL, small)
    caches = [random_cache(SMALL, pos0, 700 + r) for r in range(B)]
    first = np.array([5, 900, 1500, 31], np.int32)
    got, names = mixed_against_uniform(dec, caches, lambda b: b.generate(first, pos0, n), "generate", n - 1)
    assert "mc_b_pick_mixed_bfloat" in names
    # stepwise: every pick is the row's own sampler on the row's own logits with the row's own pair
    set_decoder(dec, DEC)
    stepwise = fresh(dec, caches)
    set_rows(stepwise)
    toks, above = first, 0
    for i in range(n):
        pairs = [PAIRS[(i * B + r) % len(PAIRS)] for r in range(B)]
        stepwise.set_seeds(pairs)   # a step uses pair r % n_pairs: rotate the list
        toks = stepwise.step(toks, pos0 + i)
        assert np.array_equal(toks, got[i]), (i, toks, got[i])
        logits = stepwise.logits()
        for r in range(B):
            s = effective(r)
            if s == GREEDY:
                v = mo.from_bf16(logits[r]).astype(np.float64)
                want = int(np.flatnonzero(v == v.max())[0])
            elif s[0] == DEFAULT_K:
                want = mo.sample_default(BF16, logits[r], top_k=s[1], temperature=s[2], top_p=s[3], init_state=pairs[r][0], init_seq=pairs[r][1])
            else:
                want, at = rule(logits[r], s, pairs[r], with_pos=True)
                above += at > 0
            assert toks[r] == want, (i, r, s, toks[r], want)
    assert above >= 2, "the draw rows draw above position 0 (checked by the rule)"
    stepwise.release()
    dec.release()


def test_ragged_step_with_an_idle_row(acc, small):
    lens = [30, 41, 7, 60, 65, 20]
    dec = small_decoder(acc, SMALL, small)
    caches = [random_cache(SMALL, n, 800 + r) for r, n in enumerate(lens)]
    toks = np.array([5, 900, 1500, 31, 77, 3], np.int32)
    pos = np.array(lens, np.int32)
    pos[5] = -1   # a draw row idle: its workgroups of both launches exit
    got, names = mixed_against_uniform(dec, caches, lambda b: b.step_rows(toks, pos)[None, :], "step_rows", 0)
    assert "mc_b_pick_mixed_rows_bfloat" in names
    assert got[0, 5] == -1 and (got[0, :5] >= 0).all()
    dec.release()


def test_chained_ragged_call_with_a_stop_id(acc, small):
    lens, n = [30, 41, 7, 60], 6
    dec = small_decoder(acc, SMALL, small)
    caches = [random_cache(SMALL, m, 800 + r) for r, m in enumerate(lens)]
    first = np.array([5, 900, 1500, 31], np.int32)
    free, _ = mixed_against_uniform(dec, caches, lambda b: b.generate_rows(first, lens, n)[0], "generate_rows", n - 1)
    stop = int(free[2, 1])   # row 1 (a draw row) stops on its third token
    got, _ = mixed_against_uniform(dec, caches, lambda b: b.generate_rows(first, lens, n, stop=[stop])[0], "generate_rows with a stop id", n - 1)
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
    got, _ = mixed_against_uniform(dec, caches, lambda b: b.generate_rows(first, [S - 1] * 4, 3)[0], "rolling", 2, rolling=True)
    assert (got >= 0).all()   # positions S - 1, S and S + 1: no row stops at the end of its cache
    dec.release()


def test_prompt_passes(acc, small):
    rng = np.random.default_rng(21)
    dec = small_decoder(acc, SMALL, small)
    prompts = [rng.integers(0, SMALL["vocab"], n).astype(np.int32) for n in (5, 17, 33, 9)]
    chunks = [rng.integers(0, SMALL["vocab"], n).astype(np.int32) for n in (3, 2, 4, 6)]
    for what, call in (("prefill_rows", lambda b: b.prefill_rows(prompts)[None, :]),
                       ("prefill_rows + extend_rows", lambda b: np.stack([b.prefill_rows(prompts), b.extend_rows(chunks, [len(p) for p in prompts])]))):
        got, names = mixed_against_uniform(dec, [None] * 4, call, what, 0)   # the first token of a pass: pair r % n_pairs
        assert (got >= 0).all()
        assert "mc_b_pick_mixed_rows_bfloat" in names
    dec.release()


def test_wide_batch(acc, small):
    B, pos0 = 17, 30
    dec = small_decoder(acc, SMALL, small)
    caches = [random_cache(SMALL, pos0, 700 + r) for r in range(B)]
    first = (np.arange(B, dtype=np.int32) * 113 + 5) % SMALL["vocab"]
    _, names = mixed_against_uniform(dec, caches, lambda b: b.generate(first, pos0, 3), "wide generate", 2, wide=True)
    assert [n for n in names if n.startswith("mc_wb_gemv_")], sorted(set(names))
    dec.release()


# ------------------------------------------------------------------------------------------ 7: the launch forms
def test_launch_forms(acc, small):
    import metalchat_amd as mc

    B, pos0 = 4, 30
    dec = small_decoder(acc, SMALL, small)
    caches = [random_cache(SMALL, pos0, 700 + r) for r in range(B)]
    toks = np.array([5, 900, 1500, 31], np.int32)
    alike = (DRAW_K, 40, 0.9, 0.95)

    def log(batch, ragged):
        dec.launch_log(True)
        batch.step_rows(toks, [pos0] * B) if ragged else batch.step(toks, pos0)
        names = dec.launched()
        dec.launch_log(False)
        return names

    for ragged, sfx in ((False, "_bfloat"), (True, "_rows_bfloat")):
        uniform = ["mc_b_topk_candidates_bfloat", "mc_draw_b" + sfx]
        set_decoder(dec, alike)
        inherited = log(fresh(dec, caches), ragged)                  # the decoder's, no row sampler set
        assert inherited[-2:] == uniform and not [n for n in inherited if "_mixed" in n or n.startswith(("mc_b_sample", "mc_b_argmax"))], inherited[-3:]
        set_decoder(dec, GREEDY)
        b = fresh(dec, caches)
        for r in range(B):
            b.set_row_sampler(r, *alike)                             # every row set alike, whatever the decoder says
        own = log(b, ragged)
        assert own == inherited
        for other in ((mc.SAMPLER_GREEDY,), (mc.SAMPLER_DEFAULT,) + alike[1:], (DRAW_K, 40, 0.9, 0.5)):
            b.set_row_sampler(2, *other)                             # any mixture with a draw row: the mixed pair, and only the pick changes
            mixed = log(b, ragged)
            assert mixed[:-2] == inherited[:-2] and mixed[-2:] == ["mc_b_topk_candidates_mixed_bfloat", "mc_b_pick_mixed" + sfx], (other, mixed[-3:])
            assert not [n for n in mixed if n.startswith(("mc_b_argmax", "mc_b_sample", "mc_draw")) or n == "mc_b_topk_candidates_bfloat"], mixed
        b.release()
    dec.release()


# ------------------------------------------------------------------------------------------ 8: best-of-n
def test_best_of_n_after_one_prompt_pass(acc, small):
    import metalchat_amd as mc

    B, n = 8, 8
    setting = (DRAW_K, 50, 1.5, 0.9)
    rng = np.random.default_rng(8)
    prompt = rng.integers(0, SMALL["vocab"], 19).astype(np.int32)
    pairs = [(10_000 + 131 * j, 5 + 3 * j) for j in range(n * B)]
    assert len(set(pairs)) == n * B
    dec = small_decoder(acc, SMALL, small)
    first = dec.prefill(prompt)   # (the decoder is greedy: one prompt pass, one first token for every row)

    def forked():
        b = mc.Batch(dec, B)
        for r in range(B):
            b.fork(r, len(prompt))
            b.set_row_sampler(r, *setting)
        return b

    b = forked()
    toks, rows = np.full(B, first, np.int32), []
    for i in range(n):
        b.set_seeds(pairs[i * B:(i + 1) * B])
        toks = b.step(toks, len(prompt) + i)
        logits = b.logits()
        want = [rule(logits[r], setting, pairs[i * B + r]) for r in range(B)]
        assert list(toks) == want, (i, toks, want)
        rows.append(toks)
    rows = np.stack(rows)
    assert len({tuple(rows[:, r]) for r in range(B)}) >= 2, "the pairs chosen give different continuations (the tokens are the rule's, above)"
    b.release()
    b = forked()   # the same in one chained call: token i of row r draws with pair i * B + r
    b.set_seeds(pairs)
    assert np.array_equal(b.generate(np.full(B, first, np.int32), len(prompt), n), rows)
    b.release()
    b = forked()   # every pair the same: every row draws the same u on the same logits
    b.set_seeds([pairs[0]] * (n * B))
    same = b.generate(np.full(B, first, np.int32), len(prompt), n)
    assert (same == same[:, :1]).all(), same
    b.release()
    dec.release()


# ------------------------------------------------------------------------------------------ 9: with logit processors
def test_a_draw_row_with_a_token_mask(acc, small):
    import metalchat_amd as mc

    B, pos0 = 2, 30
    setting = (DRAW_K, 40, 1.5, 0.95)
    dec = small_decoder(acc, SMALL, small)
    caches = [random_cache(SMALL, pos0, 700 + r) for r in range(B)]
    toks = np.array([5, 900], np.int32)
    b = fresh(dec, caches)
    for r in range(B):
        b.set_row_sampler(r, *setting)
    b.step(toks, pos0)
    raw = mo.from_bf16(b.logits()[0]).astype(np.float64)
    banned = set(np.argsort(-raw, kind="stable")[:30].tolist())   # row 0 loses its 30 best tokens
    allowed = [t for t in range(SMALL["vocab"]) if t not in banned]
    b.set_row_mask(0, allowed)
    seen = set()
    for i in range(12):
        pairs = [(77 + 5 * i, 3 + i), (991 + i, 12)]
        b.set_seeds(pairs)
        got = b.step(toks, pos0)   # (the same step again: the same slot of the cache rewritten with the same row)
        logits = b.logits()         # the processed logits
        assert (mo.from_bf16(logits[0])[sorted(banned)] == -np.inf).all()
        for r in range(B):
            assert got[r] == rule(logits[r], setting, pairs[r]), (i, r, got[r])
        assert int(got[0]) not in banned
        seen.add(int(got[0]))
    assert len(seen) >= 2, "the pairs chosen draw different tokens (the tokens are the rule's, above)"
    b.release()
    dec.release()


# ------------------------------------------------------------------------------------------ 10: the refusals
def test_refusals(acc, small):
    import metalchat_amd as mc

    assert (mc.SAMPLER_GREEDY, mc.SAMPLER_DEFAULT, mc.SAMPLER_DRAW) == (GREEDY_K, DEFAULT_K, DRAW_K)
    dec = small_decoder(acc, SMALL, small)
    b = mc.Batch(dec, 3)
    b.set_row_sampler(1, mc.SAMPLER_DRAW, top_k=20, temperature=1.0, top_p=0.3)
    dec.set_sampler(mc.SAMPLER_DRAW, 20, 1.0, 0.3)
    dec.launch_log(True)
    for args, words in (((50, 0.0, 0.9), "nucleus_sampler: temperature must be positive"),
                        ((50, 0.6, 1.5), "nucleus_sampler: probability must be in [0.0, 1.0]"),
                        ((129, 0.6, 0.9), "topk_sampler: the fused sampler keeps 1..128 candidates")):
        refused(lambda: dec.set_sampler(mc.SAMPLER_DRAW, *args), words)
        refused(lambda: b.set_row_sampler(1, mc.SAMPLER_DRAW, *args), words)
        assert b.row_sampler(1) == (mc.SAMPLER_DRAW, 20, 1.0, np.float32(0.3)), words
    assert dec.launched() == []
    dec.launch_log(False)
    b.set_row_sampler(1, mc.SAMPLER_DRAW, top_k=128, temperature=0.01, top_p=1.0)   # the ends of the ranges are admitted
    b.set_row_sampler(1, mc.SAMPLER_DRAW, top_k=1, temperature=100.0, top_p=0.0)
    b.release()
    dec.set_sampler(mc.SAMPLER_GREEDY)

    # the verify calls: a draw row in the call is a row that is not greedy
    rng = np.random.default_rng(5)
    prompts = [rng.integers(0, SMALL["vocab"], n).astype(np.int32) for n in (12, 20, 7)]
    lens = [len(p) for p in prompts]
    drafts = [rng.integers(0, SMALL["vocab"], n).astype(np.int32) for n in (4, 6, 3)]
    chain = [np.arange(-1, len(d) - 1, dtype=np.int32) for d in drafts]
    for tree in (False, True):
        verify = (lambda b, rows: b.verify_tree([drafts[r] if r in rows else None for r in range(3)],
                                                [chain[r] if r in rows else None for r in range(3)], lens)[:3]) if tree else \
                 (lambda b, rows: b.verify_rows([drafts[r] if r in rows else None for r in range(3)], lens))
        who = "mc_tree_verify" if tree else "mc_verify_rows"
        greedy = mc.Batch(dec, 3)
        greedy.prefill_rows(prompts)
        want = verify(greedy, (0, 1))
        b = mc.Batch(dec, 3)
        b.prefill_rows(prompts)
        b.set_row_sampler(2, mc.SAMPLER_DRAW, 40, 0.9, 0.95)
        before = list(b.lengths())
        dec.launch_log(True)
        with pytest.raises(mc.McError) as e:
            verify(b, (0, 1, 2))
        assert e.value.status == 1
        assert str(e.value).endswith(who + ": row 2: the row's sampler is not greedy (accepting sampled drafts needs the draft's probabilities)"), str(e.value)
        assert dec.launched() == [] and list(b.lengths()) == before
        dec.launch_log(False)
        got = verify(b, (0, 1))   # the draw row is not in the call: admitted
        for g, w_ in zip(got, want):
            for r in range(3):
                assert np.array_equal(g[r], w_[r]) if g[r] is not None else w_[r] is None, (tree, r, g[r], w_[r])
        b.reset_row_samplers()
        dec.set_sampler(mc.SAMPLER_DRAW, 40, 0.9, 0.95)   # nothing set and a drawing decoder: the decoder-wide text
        refused(lambda: verify(b, (0, 1)), who + ": the decoder's sampler is not greedy")
        dec.set_sampler(mc.SAMPLER_GREEDY)
        b.release()
        greedy.release()
    dec.release()

    # a stage that is not the last one does not sample
    cfg = mg.tiny_cfg(BF16, n_layers=4)
    stage = mc.Decoder(acc, **mg.decoder_kwargs(cfg, weight_format=mc.WFMT_I4, group_size=32, layer_begin=0, layer_end=3))
    refused(lambda: stage.set_sampler(mc.SAMPLER_DRAW, 50, 0.6, 0.9), "decoder: only the last stage samples")
    stage.release()
