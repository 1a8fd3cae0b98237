"""Rolling rows (mc_rolling_set, mc_rolling_fork_row; include/metalchat_hip.h Part 2j) on the device: the ragged rows of a batch
decode past max_seq_len on the sink ring.  max_seq_len = 64 (the least a batch admits: pre_len 6, post 58) unless a case says otherwise.

  * rows that start below the end -- one at S - 1, one at 0, one idle -- run one chained call past the end and through the wrap of the
    ring base, each step's logits against the row's own oracle.Model fed the device's tokens, with test_ragged_gpu's bounds; the
    same at max_seq_len 256 over positions 252 .. 259 and for a QLoRA decoder on a wide batch;
  * the ring itself: each rolling step keeps the sink rows, drops logical row pre_len and appends the new row, bit for bit;
  * a row's bits do not depend on B, its index or its company (B = 1, row 5 of 8, row 20 of a wide 24);
  * one chained call == single steps; rows that stay below the end compute the same bits with rolling on and off;
  * mc_rolling_fork_row; and the refusals, with nothing launched and no length changed."""
import numpy as np
import pytest

import modelgen as mg
import parity
import rolling_rule as rr
from oracle import mc_oracle as mo
from test_batch_gpu import LLAMA32_1B, SMALL, small_decoder
from test_context_gpu import random_cache
from test_qlora_batch_gpu import decoder_of, qlora_model
from test_ragged_gpu import PAIRS, refused, with_sampler
from test_rows_prefill_gpu import clear_gap

pytestmark = pytest.mark.gpu
BF16 = 0
S = 64
S64 = dict(SMALL, max_seq_len=S)
L64 = dict(LLAMA32_1B, max_seq_len=S)
PRE, POST = rr.pre_len(S), S - rr.pre_len(S)
WRAP = S + POST + 3   # a row that reaches this position has seen its ring base pass through 0 again


@pytest.fixture(scope="module")
def small():
    return mg.make_model(S64, seed=11, quant="i4", group=128)


@pytest.fixture(scope="module")
def llama1b():
    return mg.make_model(L64, seed=5)


def caches_of(cfg, lens, seed):
    """per row: one random (K, V) of lens[r] positions per layer, None for an empty (or idle) row"""
    return [[random_cache(cfg, n, seed + 1000 * r + layer) for layer in range(cfg["n_layers"])] if n > 0 else None
            for r, n in enumerate(lens)]


def batch_of(dec, caches, wide=False, rolling=True):
    import metalchat_amd as mc

    b = mc.Batch(dec, len(caches), wide=wide)
    for r, kv in enumerate(caches):
        for layer, (k, v) in enumerate(kv or []):
            b.import_kv(r, layer, k, v)
    if rolling:
        b.set_rolling(True)
        assert b.rolling()
    return b


def exports(batch, r, layers=1):
    return [a for layer in range(layers) for a in batch.export_row_kv(r, layer)]


def same_bits(a, b, what):
    assert len(a) == len(b)
    for i, (x, y) in enumerate(zip(a, b)):
        assert x.shape == y.shape, (what, i, x.shape, y.shape)
        parity.exact(x, y, f"{what} [{i}]")


# ------------------------------------------------------------------------------------------ against the oracle
def rows_against_the_oracle(dec, cfg, weights, start, n, what, wide=False):
    """Rows at start[r] (-1: idle) behind random caches; ONE chained call of n steps with rolling on gives the tokens, a second batch
    run in calls of one step gives the same tokens and every step's logits, compared with each row's oracle fed the device's
    tokens.  Tokens are compared where the oracle's pick is unambiguous (clear_gap); returns (ambiguous, compared positions)."""
    Smax, L, B = cfg["max_seq_len"], cfg["n_layers"], len(start)
    start = np.array(start, np.int32)
    caches = caches_of(cfg, start, 500)
    active = [r for r in range(B) if start[r] >= 0]
    first = np.where(start >= 0, 7 + 13 * np.arange(B), -1).astype(np.int32)
    chained = batch_of(dec, caches, wide)
    dec.launch_log(True)
    got, lengths = chained.generate_rows(first, start, n)
    names = set(dec.launched())
    dec.launch_log(False)
    assert "mc_b_rows_begin_rolling" in names and "mc_b_rows_begin" not in names, sorted(names)
    assert list(lengths) == [n if r in active else 0 for r in range(B)]
    assert list(chained.lengths()) == [start[r] + n if r in active else 0 for r in range(B)]
    oms = {r: mo.Model(cfg, weights) for r in active}
    for r in active:
        for layer, (k, v) in enumerate(caches[r] or []):
            oms[r].set_kv(layer, k, v)
    stepwise = batch_of(dec, caches, wide)
    toks, ambiguous = first, 0
    for i in range(n):
        pos = np.where(start >= 0, start + i, -1).astype(np.int32)
        picks, _ = stepwise.generate_rows(toks, pos, 1)
        assert np.array_equal(picks[0], got[i]), (what, i, picks[0], got[i])
        logits = stepwise.logits()
        for r in active:
            otok, ologits = oms[r].step(int(toks[r]), int(pos[r]))
            parity.check(BF16, logits[r], ologits, rel=5e-3, max_ulp=2 + L, max_frac=0.7, what=f"{what} row {r} pos {pos[r]} logits")
            assert got[i, r] == int(np.argmax(mo.from_bf16(logits[r]))), (what, r, pos[r])
            if clear_gap(ologits):
                assert got[i, r] == otok, (what, r, pos[r], got[i, r], otok)
            else:
                ambiguous += 1
        toks = got[i]
    parity.exact(chained.logits()[active], stepwise.logits()[active], f"{what}: last logits, chained against stepwise")
    for r in active:
        held = rr.positions_held(int(start[r]) + n, Smax)
        injected = [i for i, p in enumerate(held) if p < start[r]]
        computed = [i for i, p in enumerate(held) if p >= start[r]]
        for layer in range(L):
            gk, gv = chained.export_row_kv(r, layer)
            ok, ov = oms[r].kv(layer)
            assert gk.shape == ok.shape == (len(held), cfg["n_kv_heads"], cfg["head_dim"]), (what, r, gk.shape, ok.shape)
            same_bits([gk, gv], list(stepwise.export_row_kv(r, layer)), f"{what} row {r} layer {layer}: chained against stepwise K / V")
            parity.exact(gk[injected], ok[injected], f"{what} row {r} layer {layer} injected K")
            parity.exact(gv[injected], ov[injected], f"{what} row {r} layer {layer} injected V")
            parity.check(BF16, gk[computed], ok[computed], rel=3.9e-3, max_ulp=2, max_frac=0.7, what=f"{what} row {r} layer {layer} computed K")
            parity.check(BF16, gv[computed], ov[computed], rel=3.9e-3, max_ulp=2, max_frac=0.7, what=f"{what} row {r} layer {layer} computed V")
    for r in range(B):
        if r not in active:
            assert (got[:, r] == -1).all() and chained.export_row_kv(r, 0)[0].shape[0] == 0
    chained.release()
    stepwise.release()
    for om in oms.values():
        om.close()
    return ambiguous, n * len(active)


@pytest.mark.parametrize("shape", ["small-int4", "llama32-1b-bf16", "small-int4-s256"])
def test_rolled_rows_against_the_oracle(acc, small, llama1b, shape):
    """Ambiguous positions (the oracle's top two logits within two bfloat steps, decided by the oracle alone on the CPU with each row
    fed its own picks): small-int4 52 of 375, llama32-1b-bf16 13 of 250, small-int4-s256 4 of 24 -- each below a quarter, which the
    test also requires of the run itself.  The llama32-1b case takes about ten seconds, nearly all of it the CPU oracle's 250 steps
    (two rows through the wrap of the ring base at dim 2048, two layers); the device's share is a fraction of a second."""
    if shape == "small-int4":
        cfg, weights, start, n = S64, small, [S - 1, 0, -1, 40], WRAP
    elif shape == "llama32-1b-bf16":
        cfg, weights, start, n = L64, llama1b, [S - 1, 0, -1], WRAP
    else:   # a context of several 64-slot ranges: positions 252 .. 259 for row 0
        cfg, weights, start, n = SMALL, mg.make_model(SMALL, seed=11, quant="i4", group=128), [252, 0, -1, 250], 8
    assert cfg is SMALL or max(start) + n >= WRAP and n >= WRAP
    dec = small_decoder(acc, cfg, weights)
    ambiguous, total = rows_against_the_oracle(dec, cfg, weights, start, n, shape)
    assert 4 * ambiguous <= total, (shape, ambiguous, total)
    dec.release()


def test_a_qlora_decoder_on_a_wide_batch_rolls(acc):
    """the smallest QLoRA shape of test_qlora_batch_gpu.py (int4 g32 with rank-16 adaptors, int8 embedding and head) at B = 20: 10 steps
    across the end.  Ambiguous positions by the oracle alone (as above): 6 of 30 (weight seeds 34 and 38: 4 and 3)."""
    weights = qlora_model(S64, 28)
    dec = decoder_of(acc, S64, weights)
    start = [-1] * 20
    start[0], start[7], start[19] = S - 1, S - 5, 0
    ambiguous, total = rows_against_the_oracle(dec, S64, weights, start, 10, "qlora wide B=20", wide=True)
    assert 4 * ambiguous <= total, (ambiguous, total)
    dec.release()


# ------------------------------------------------------------------------------------------ the ring itself
def test_each_rolling_step_drops_the_oldest_row_and_appends_the_new_one(acc, small):
    dec = small_decoder(acc, S64, small)
    caches = caches_of(S64, [S - 1, 20], 40)
    batch = batch_of(dec, caches)
    om = mo.Model(S64, small)
    om.set_kv(0, *caches[0][0])
    tok = batch.step_rows([5, 6], [S - 1, 20])       # row 0 is full and still linear
    om.step(5, S - 1)
    other = exports(batch, 1)
    before = exports(batch, 0)
    assert before[0].shape[0] == S and list(batch.lengths()) == [S, 21]
    parity.exact(before[0][: S - 1], caches[0][0][0], "the imported K rows before any roll")
    fed = []
    for p in range(S, WRAP):                         # ring_base 1 .. post - 1, 0, 1, 2, 3
        fed.append(int(tok[0]))
        tok = batch.step_rows([tok[0], -1], [p, -1])
        after = exports(batch, 0)
        for b_, a, name in zip(before, after, "KV"):
            assert a.shape[0] == S
            parity.exact(a[:PRE], b_[:PRE], f"pos {p} {name}: the sink rows stay")
            parity.exact(a[PRE: S - 1], b_[PRE + 1: S], f"pos {p} {name}: the post rows move up by one")
            assert not np.array_equal(a[S - 1], b_[S - 1]), f"pos {p} {name}: the last row is new"
        before = after
    assert batch.lengths()[0] == WRAP and rr.state(WRAP - 1, S)[0] == 3
    same_bits(exports(batch, 1), other, "the idle row beside it")
    for p, t in zip(range(S, WRAP), fed):
        om.step(t, p)
    ok, ov = om.kv(0)
    parity.exact(before[0][:PRE], ok[:PRE], "sink K rows: the imported ones")
    parity.check(BF16, before[0][PRE:], ok[PRE:], rel=3.9e-3, max_ulp=2, max_frac=0.7, what="K after the wrap against the oracle")
    parity.check(BF16, before[1][PRE:], ov[PRE:], rel=3.9e-3, max_ulp=2, max_frac=0.7, what="V after the wrap against the oracle")
    om.close()
    batch.release()
    dec.release()


# ------------------------------------------------------------------------------------------ independence
def run_the_row(dec, B, row, wide):
    """the row under test -- a cache of S - 1 positions, then 10 + 61 chained steps: 70 of them rolling -- at index `row` of a batch of
    B whose other rows are rolled (from S - 1 and from 3), not rolled (idle in the second call at length 20) and idle throughout"""
    company = {0: (S - 1, True), 1: (3, True), 2: (10, False)} if B > 1 else {}
    start = np.full(B, -1, np.int32)
    start[row] = S - 1
    for r, (p, _) in company.items():
        start[r] = p
    if B > 8:
        start[B - 1], company[B - 1] = 33, (33, True)
    caches = caches_of(S64, [int(p) if p > 0 else 0 for p in start], 60)
    caches[row] = [random_cache(S64, S - 1, 4242)]
    batch = batch_of(dec, caches, wide)
    first = np.where(start >= 0, 50 + 7 * np.arange(B), -1).astype(np.int32)
    first[row] = 77
    out = []
    got1, _ = batch.generate_rows(first, start, 10)
    out += [got1[:, row].copy(), batch.logits()[row].copy()]
    pos2 = np.array([start[r] + 10 if r == row or company.get(r, (0, False))[1] else -1 for r in range(B)], np.int32)
    got2, _ = batch.generate_rows(np.where(pos2 >= 0, got1[-1], -1), pos2, 61)
    out += [got2[:, row].copy(), batch.logits()[row].copy()] + exports(batch, row)
    lengths = batch.lengths()
    assert lengths[row] == S - 1 + 71
    if B > 1:
        assert list(lengths[:4]) == [S - 1 + 71, 3 + 71, 20, 0]
    batch.release()
    return out


def test_a_rows_bits_do_not_depend_on_the_batch(acc, small):
    dec = small_decoder(acc, S64, small)
    alone = run_the_row(dec, 1, 0, False)
    assert (alone[0] >= 0).all() and (alone[2] >= 0).all() and alone[4].shape[0] == S
    same_bits(run_the_row(dec, 8, 5, False), alone, "row 5 of 8 against the row alone")
    same_bits(run_the_row(dec, 24, 20, True), alone, "row 20 of a wide 24 against the row alone")
    dec.release()


# ------------------------------------------------------------------------------------------ call splitting, rows below the end
@pytest.mark.parametrize("sampler", ["greedy", "default"])
def test_chained_equals_stepwise_across_the_end(acc, small, sampler):
    B, n = 4, 12
    lens = [S - 3, 10, -1, S - 1]
    dec = small_decoder(acc, S64, small)
    with_sampler(dec, sampler)
    caches = caches_of(S64, lens, 800)
    first = np.array([5, 900, -1, 31], np.int32)
    chained = batch_of(dec, caches)
    chained.set_seeds(PAIRS)
    got, lengths = chained.generate_rows(first, lens, n)
    assert list(lengths) == [n, n, 0, n] and list(chained.lengths()) == [S - 3 + n, 10 + n, 0, S - 1 + n]
    stepwise = batch_of(dec, caches)
    toks = first
    for i in range(n):
        # token i of a chained call uses pair (i * B + r) % n_pairs; a step uses pair r % n_pairs: rotate the list
        stepwise.set_seeds([PAIRS[(i * B + r) % len(PAIRS)] for r in range(B)])
        toks = stepwise.step_rows(toks, [p + i if p >= 0 else -1 for p in lens])
        assert np.array_equal(toks, got[i]), (sampler, i, toks, got[i])
    active = [0, 1, 3]
    parity.exact(chained.logits()[active], stepwise.logits()[active], "last logits")
    for r in active:
        same_bits(exports(chained, r), exports(stepwise, r), f"{sampler} row {r} K / V after {n} tokens")
    chained.release()
    stepwise.release()
    dec.release()


@pytest.mark.parametrize("sampler", ["greedy", "default"])
def test_rows_below_the_end_do_not_change(acc, small, sampler):
    B, n = 4, 12
    lens = [30, 41, 0, 50]   # the longest ends at position 61
    dec = small_decoder(acc, S64, small)
    with_sampler(dec, sampler)
    caches = caches_of(S64, lens, 300)
    first = np.array([5, 900, 1500, 31], np.int32)
    off, on = batch_of(dec, caches, rolling=False), batch_of(dec, caches)
    assert not off.rolling()
    runs = []
    for b in (off, on):
        b.set_seeds(PAIRS)
        dec.launch_log(True)
        got, lengths = b.generate_rows(first, lens, n)
        runs.append(set(dec.launched()))
        step = b.step_rows(got[-1], np.array(lens) + n)
        b.got = [got, lengths, step, b.logits()] + [a for r in range(B) for a in exports(b, r)]
    dec.launch_log(False)
    assert "mc_b_rows_begin" in runs[0] and "mc_b_rows_begin_rolling" not in runs[0]
    assert "mc_b_rows_begin_rolling" in runs[1] and "mc_b_rows_begin" not in runs[1]
    same_bits(on.got, off.got, f"{sampler}: rolling on against rolling off")
    off.release()
    on.release()
    dec.release()


# ------------------------------------------------------------------------------------------ mc_rolling_fork_row
def test_fork_row(acc, llama1b):
    L = L64["n_layers"]
    dec = small_decoder(acc, L64, llama1b)
    caches = caches_of(L64, [S - 1, 0, 10], 70)
    batch = batch_of(dec, caches)
    got, _ = batch.generate_rows([11, -1, 22], [S - 1, -1, 10], 20)
    assert list(batch.lengths()) == [S + 19, 0, 30]
    third = exports(batch, 2, L)
    batch.fork_row(1, 0)                             # a rolled row onto an empty one
    assert list(batch.lengths()) == [S + 19, S + 19, 30]
    same_bits(exports(batch, 1, L), exports(batch, 0, L), "the copy's export")
    nxt = int(got[-1, 0])
    more, lengths = batch.generate_rows([nxt, nxt, -1], [S + 19, S + 19, -1], 10)
    assert list(lengths) == [10, 10, 0] and np.array_equal(more[:, 0], more[:, 1]), more
    logits = batch.logits()
    parity.exact(logits[1], logits[0], "logits of source and copy after 10 more steps")
    same_bits(exports(batch, 1, L), exports(batch, 0, L), "source and copy after 10 more steps")
    same_bits(exports(batch, 2, L), third, "the third row")
    assert list(batch.lengths()) == [S + 29, S + 29, 30]
    batch.fork_row(0, 2)                             # a short row onto a rolled one: linear again
    assert list(batch.lengths()) == [30, S + 29, 30]
    same_bits(exports(batch, 0, L), third, "a short row forked onto a rolled one")
    t = int(got[-1, 2])
    picks = batch.step_rows([t, -1, t], [30, -1, 30])
    assert picks[0] == picks[2]
    parity.exact(batch.logits()[0], batch.logits()[2], "the reset row steps as its source does")
    same_bits(exports(batch, 0, L), exports(batch, 2, L), "... K / V")
    batch.release()
    dec.release()


# ------------------------------------------------------------------------------------------ refusals
def test_refusals(acc, small):
    dec = small_decoder(acc, S64, small)
    batch = batch_of(dec, caches_of(S64, [S - 1, 10, 0], 5))
    batch.generate_rows([1, 2, -1], [S - 1, 10, -1], 5)
    assert list(batch.lengths()) == [S + 4, 15, 0]
    dec.launch_log(True)
    chunk = [3, 4, 5]
    cases = [
        (lambda: batch.step_rows([1, -1, -1], [S, -1, -1]), f"mc_ragged_step: row 0: position {S} lies below the row's length {S + 4} and the row has rolled"),
        (lambda: batch.generate_rows([1, -1, -1], [5, -1, -1], 2), f"mc_ragged_generate: row 0: position 5 lies below the row's length {S + 4} and the row has rolled"),
        (lambda: batch.step_rows([1, -1, -1], [S + 5, -1, -1]), f"row 0: position {S + 5} is past the row's length {S + 4}"),
        (lambda: batch.step_rows([-1, 1, -1], [-1, 16, -1]), "row 1: position 16 is past the row's length 15"),
        (lambda: batch.extend_rows([chunk, None, None], [S + 4, 0, 0]), f"mc_extend_rows: row 0: position + length {S + 7} exceeds max_seq_len"),
        (lambda: batch.verify_rows([chunk, None, None], [S + 4, 0, 0]), f"mc_verify_rows: row 0: position + length {S + 7} exceeds max_seq_len"),
        (lambda: batch.extend_rows([chunk, None, None], [20, 0, 0]), f"mc_extend_rows: row 0: position 20 lies below the row's length {S + 4} and the row has rolled"),
        (lambda: batch.fork_row(1, 1), "mc_rolling_fork_row: dst and src are the same row"),
        (lambda: batch.fork_row(3, 0), "mc_rolling_fork_row: row out of range"),
        (lambda: batch.fork_row(0, -1), "mc_rolling_fork_row: row out of range"),
    ]
    for fn, words in cases:
        refused(fn, words)
        assert dec.launched() == [], words
        assert list(batch.lengths()) == [S + 4, 15, 0], words
    # a restart at 0 is the one rewind a rolled row takes
    batch.step_rows([9, -1, -1], [0, -1, -1])
    assert list(batch.lengths()) == [1, 15, 0] and batch.export_row_kv(0, 0)[0].shape[0] == 1
    batch.release()
    dec.release()


def test_with_rolling_off_a_row_ends_with_its_cache(acc, small):
    dec = small_decoder(acc, S64, small)
    batch = batch_of(dec, caches_of(S64, [S - 3, 40], 600), rolling=False)
    assert not batch.rolling()
    got, lengths = batch.generate_rows([1, 2], [S - 3, 40], 6)
    assert list(lengths) == [3, 6] and (got[3:, 0] == -1).all() and (got[:3, 0] >= 0).all() and (got[:, 1] >= 0).all()
    assert list(batch.lengths()) == [S, 46] and batch.export_row_kv(0, 0)[0].shape[0] == S
    dec.launch_log(True)
    refused(lambda: batch.step_rows([1, -1], [S, -1]), f"row 0: position {S} must be below max_seq_len (a batch's cache does not roll)")
    refused(lambda: batch.generate_rows([1, -1], [S, -1], 2), f"row 0: position {S} must be below max_seq_len (a batch's cache does not roll)")
    assert dec.launched() == [] and list(batch.lengths()) == [S, 46]
    # ... and switched on, the same row goes on from there; switched off again, a rolled row can only be restarted
    batch.set_rolling(True)
    batch.step_rows([1, -1], [S, -1])
    batch.set_rolling(False)
    assert list(batch.lengths()) == [S + 1, 46]
    dec.launch_log(True)
    refused(lambda: batch.step_rows([1, -1], [S + 1, -1]), f"row 0: position {S + 1} must be below max_seq_len")
    refused(lambda: batch.step_rows([1, -1], [S - 1, -1]), f"row 0: position {S - 1} lies below the row's length {S + 1} and the row has rolled")
    assert dec.launched() == []
    batch.release()
    dec.release()
