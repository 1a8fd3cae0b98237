"""Ragged rows (mc_ragged_*, include/metalchat_hip.h Part 2c) on the device: the rows of a batch, each at its own position.

  * a row at position p computes, bit for bit, what a one-row lockstep batch computes at p;
  * parity per row against its own oracle.Model, with rows crossing 64-slot boundaries at different steps;
  * all rows at one position reproduce the lockstep calls bit for bit; chained == stepwise;
  * stop ids, idle rows, refilling a row by a fork, the end of a row's cache, and the refusals.
"""
import numpy as np
import pytest

import parity
from oracle import mc_oracle as mo
from test_batch_gpu import LLAMA32_1B, SMALL, small_decoder
from test_context_gpu import random_cache

import modelgen as mg

pytestmark = pytest.mark.gpu
BF16 = 0
S = SMALL["max_seq_len"]


@pytest.fixture(scope="module")
def small():
    return mg.make_model(SMALL, seed=11, quant="i4", group=128)


def batch_of(dec, caches):
    """a batch whose row r holds caches[r] (one (k, v) per layer), or nothing for None"""
    import metalchat_amd as mc

    b = mc.Batch(dec, len(caches))
    for r, kv in enumerate(caches):
        for layer, (k, v) in enumerate(kv or []):
            b.import_kv(r, layer, k, v)
    return b


def test_a_row_equals_a_single_row(acc, small):
    lens = [5, 63, 64, 65, 127, 128, 200, 250]
    dec = small_decoder(acc, SMALL, small)
    caches = [[random_cache(SMALL, n, 300 + r)] for r, n in enumerate(lens)]
    toks = np.array([17 + 211 * r for r in range(8)], np.int32)
    batch = batch_of(dec, caches)
    assert list(batch.lengths()) == lens
    picks = batch.step_rows(toks, lens)
    logits = batch.logits()
    assert list(batch.lengths()) == [n + 1 for n in lens]
    for r, n in enumerate(lens):
        one = batch_of(dec, [caches[r]])
        pick = one.step([toks[r]], n)
        assert pick[0] == picks[r], (r, n)
        parity.exact(logits[r], one.logits()[0], f"row {r} at {n}: logits")
        for a, b_, name in zip(batch.export_row_kv(r, 0), one.export_kv(0, 0), "KV"):
            assert a.shape[0] == n + 1
            parity.exact(a, b_, f"row {r} at {n}: {name}")
        one.release()
    batch.release()
    dec.release()


@pytest.mark.parametrize("shape", ["small-int4", "llama32-1b-bf16", "small-int4-int8-embedding", "small-int4-group-256"])
def test_rows_against_the_oracle(acc, small, shape):
    group = 256 if shape == "small-int4-group-256" else 128
    if shape == "small-int4":
        cfg, weights = SMALL, small
    elif shape == "llama32-1b-bf16":
        cfg, weights = LLAMA32_1B, mg.make_model(LLAMA32_1B, seed=5)
    else:   # admitted formats no other ragged test loads: an int8 embedding table, int4 groups of 256
        cfg, weights = SMALL, mg.make_model(SMALL, seed=13, quant="i4", group=group, emb_quant=shape.endswith("int8-embedding"))
    L, B, n_steps = cfg["n_layers"], 4, 6
    lens = [60, 62, 125, 190]  # 64-slot boundaries crossed at steps 4, 2, 3 and 2
    dec = small_decoder(acc, cfg, weights, **({"group_size": group} if cfg is SMALL else {}))
    oms = [mo.Model(cfg, weights) for _ in range(B)]
    caches = []
    for r in range(B):
        caches.append([random_cache(cfg, lens[r], 1000 * r + layer) for layer in range(L)])
        for layer in range(L):
            oms[r].set_kv(layer, *caches[r][layer])
    batch = batch_of(dec, caches)
    dec.launch_log(True)
    toks = np.array([7 + 13 * r for r in range(B)], np.int32)
    for i in range(n_steps):
        pos = np.array(lens, np.int32) + i
        picks = batch.step_rows(toks, pos)
        logits = batch.logits()
        nxt = np.zeros(B, np.int32)
        for r in range(B):
            otok, ologits = oms[r].step(int(toks[r]), int(pos[r]))
            parity.check(BF16, logits[r], ologits, rel=5e-3, max_ulp=2 + L, max_frac=0.7, what=f"{shape} row {r} pos {pos[r]} logits")
            assert picks[r] == int(np.argmax(mo.from_bf16(logits[r]))), (shape, r, pos[r])
            nxt[r] = otok
        toks = nxt
    for r in range(B):
        for layer in range(L):
            gk, gv = batch.export_row_kv(r, layer)
            ok, ov = oms[r].kv(layer)
            n = lens[r]
            assert gk.shape == ok.shape == (n + n_steps, cfg["n_kv_heads"], cfg["head_dim"])
            parity.exact(gk[:n], ok[:n], f"{shape} row {r} layer {layer} injected K")
            parity.exact(gv[:n], ov[:n], f"{shape} row {r} layer {layer} injected V")
            parity.check(BF16, gk[n:], ok[n:], rel=3.9e-3, max_ulp=2, max_frac=0.7, what=f"{shape} row {r} computed K")
            parity.check(BF16, gv[n:], ov[n:], rel=3.9e-3, max_ulp=2, max_frac=0.7, what=f"{shape} row {r} computed V")
    names = set(dec.launched())
    assert {"mc_b_rows_begin", "mc_b_embed_rows_bfloat", "mc_b_rope_kv_rows_bfloat", "mc_b_attn_scores_rows_bfloat",
            "mc_b_attn_pv_rows_bfloat", "mc_b_argmax_rows_bfloat"} <= names, sorted(names)
    assert not {"mc_step_set", "mc_b_attn_scores_bfloat", "mc_b_attn_pv_bfloat"} & names, sorted(names)
    batch.release()
    for om in oms:
        om.close()
    dec.release()


def with_sampler(dec, sampler):
    import metalchat_amd as mc

    if sampler == "default":
        dec.set_sampler(mc.SAMPLER_DEFAULT, top_k=40, temperature=0.9, top_p=0.95)


PAIRS = [(1000 + 17 * i, 77 + i) for i in range(5)]


@pytest.mark.parametrize("sampler", ["greedy", "default"])
def test_equal_positions_equal_lockstep(acc, small, sampler):
    B, n, pos0 = 4, 8, 30
    dec = small_decoder(acc, SMALL, small)
    with_sampler(dec, sampler)
    caches = [[random_cache(SMALL, pos0, 700 + r)] for r in range(B)]
    first = np.array([5, 900, 1500, 31], np.int32)
    lock, rag = batch_of(dec, caches), batch_of(dec, caches)
    lock.set_seeds(PAIRS)
    rag.set_seeds(PAIRS)
    want = lock.generate(first, pos0, n)
    got, lengths = rag.generate_rows(first, [pos0] * B, n)
    assert np.array_equal(got, want), (got, want)
    assert list(lengths) == [n] * B and list(rag.lengths()) == [pos0 + n] * B
    parity.exact(rag.logits(), lock.logits(), "logits after generate")
    want1 = lock.step(want[-1], pos0 + n)
    got1 = rag.step_rows(want[-1], [pos0 + n] * B)
    assert np.array_equal(got1, want1)
    parity.exact(rag.logits(), lock.logits(), "logits after step")
    for r in range(B):
        for a, b_, name in zip(rag.export_row_kv(r, 0), lock.export_kv(r, 0), "KV"):
            assert a.shape[0] == pos0 + n + 1
            parity.exact(a, b_, f"{sampler} row {r} {name}")
    lock.release()
    rag.release()
    dec.release()


@pytest.mark.parametrize("sampler", ["greedy", "default"])
def test_chained_equals_stepwise(acc, small, sampler):
    B, n = 4, 12
    lens = [30, 41, 7, 60]
    dec = small_decoder(acc, SMALL, small)
    with_sampler(dec, sampler)
    caches = [[random_cache(SMALL, lens[r], 800 + r)] for r in range(B)]
    first = np.array([5, 900, 1500, 31], np.int32)
    chained = batch_of(dec, caches)
    chained.set_seeds(PAIRS)
    got, lengths = chained.generate_rows(first, lens, n)
    assert got.shape == (n, B) and list(lengths) == [n] * B
    stepwise = batch_of(dec, caches)
    toks = first
    for i in range(n):
        # token i of a chained call uses pair (i * B + r) % n_pairs; a step uses pair r % n_pairs: rotate the list
        stepwise.set_seeds([PAIRS[(i * B + r) % len(PAIRS)] for r in range(B)])
        toks = stepwise.step_rows(toks, np.array(lens) + i)
        assert np.array_equal(toks, got[i]), (sampler, i, toks, got[i])
    parity.exact(chained.logits(), stepwise.logits(), "last logits")
    for r in range(B):
        for a, b_, name in zip(chained.export_row_kv(r, 0), stepwise.export_row_kv(r, 0), "KV"):
            parity.exact(a, b_, f"{sampler} row {r} {name} after {n} tokens")
    chained.release()
    stepwise.release()
    dec.release()


def test_stop_ids(acc, small):
    B, n, held = 4, 10, 40
    pos = [20, 25, 30, 40]  # the first three rewind into caches of 40 positions
    dec = small_decoder(acc, SMALL, small)
    caches = [[random_cache(SMALL, held, 900 + r)] for r in range(B)]
    first = np.array([3, 333, 1333, 2000], np.int32)
    free = batch_of(dec, caches)
    want, wl = free.generate_rows(first, pos, n)
    assert list(wl) == [n] * B
    # a stop set of two tokens the free run produced (row a at step i, row b at step j), under which some row runs on
    for (ra, ia), (rb, ib) in [((0, 2), (2, 5)), ((1, 3), (3, 6)), ((3, 1), (0, 7)), ((2, 4), (1, 0))]:
        stop = sorted({int(want[ia, ra]), int(want[ib, rb])})
        at = [next((i for i in range(n) if want[i, r] in stop), None) for r in range(B)]
        if None in at:
            break
    assert None in at, (want, stop)
    stopped = batch_of(dec, caches)
    got, lengths = stopped.generate_rows(first, pos, n, stop=stop)
    for r in range(B):
        k, v = stopped.export_kv(r, 0)  # the whole imported range: the lockstep position is not moved by ragged calls
        assert k.shape[0] == held
        fk, fv = free.export_kv(r, 0)
        if at[r] is None:
            assert np.array_equal(got[:, r], want[:, r]) and lengths[r] == n, r
            parity.exact(k, fk, f"row {r} K")
            parity.exact(v, fv, f"row {r} V")
            continue
        m = at[r] + 1
        assert np.array_equal(got[:m, r], want[:m, r]) and got[m - 1, r] in stop, (r, got[:, r])
        assert (got[m:, r] == -1).all(), (r, got[:, r])
        assert lengths[r] == m and stopped.lengths()[r] == pos[r] + m
        end = pos[r] + m
        parity.exact(k[:end], fk[:end], f"row {r} K before the stop")
        parity.exact(v[:end], fv[:end], f"row {r} V before the stop")
        parity.exact(k[end:], caches[r][0][0][end:], f"row {r} K after the stop: untouched")
        parity.exact(v[end:], caches[r][0][1][end:], f"row {r} V after the stop: untouched")
        assert stopped.export_row_kv(r, 0)[0].shape[0] == end
    free.release()
    stopped.release()
    dec.release()


def test_idle_rows(acc, small):
    B, n = 4, 5
    lens = [33, 50, 70, 12]
    dec = small_decoder(acc, SMALL, small)
    caches = [[random_cache(SMALL, lens[r], 400 + r)] for r in range(B)]
    first = np.array([9, 99, 999, 1999], np.int32)
    busy, idle = batch_of(dec, caches), batch_of(dec, caches)
    want, _ = busy.generate_rows(first, lens, n)
    want_step = busy.step_rows(want[-1], np.array(lens) + n)
    pos = np.array(lens) + 0
    pos[1] = -1
    t = first.copy()
    t[1] = -1  # an idle row's token is never read
    got, lengths = idle.generate_rows(t, pos, n)
    assert (got[:, 1] == -1).all() and lengths[1] == 0
    last = want[-1].copy()
    last[1] = -1
    got_step = idle.step_rows(last, np.where(pos < 0, -1, pos + n))
    assert got_step[1] == -1
    assert idle.lengths()[1] == lens[1]
    k, v = idle.export_row_kv(1, 0)
    parity.exact(k, caches[1][0][0], "idle row K")
    parity.exact(v, caches[1][0][1], "idle row V")
    for r in (0, 2, 3):
        assert np.array_equal(got[:, r], want[:, r]) and got_step[r] == want_step[r], r
        parity.exact(idle.logits()[r], busy.logits()[r], f"row {r} logits")
        for a, b_, name in zip(idle.export_row_kv(r, 0), busy.export_row_kv(r, 0), "KV"):
            parity.exact(a, b_, f"row {r} {name} beside an idle row")
    busy.release()
    idle.release()
    dec.release()


def test_refill_a_row(acc, small):
    import metalchat_amd as mc

    B, n1 = 4, 5
    rng = np.random.default_rng(21)
    p1 = rng.integers(0, SMALL["vocab"], 50).astype(np.int32)
    p2 = rng.integers(0, SMALL["vocab"], 70).astype(np.int32)
    dec = small_decoder(acc, SMALL, small)
    first = np.array([12, 1200, 120, 2012], np.int32)

    def start():
        dec.prefill(p1, 0)
        b = mc.Batch(dec, B)
        for r in range(B):
            b.fork(r, len(p1))
        toks, _ = b.generate_rows(first, [len(p1)] * B, n1)
        return b, toks[-1].copy()

    plain, last_p = start()
    refill, last_r = start()
    assert np.array_equal(last_p, last_r)
    dec.prefill(p2, 0)
    refill.fork(2, len(p2))
    assert list(refill.lengths()) == [len(p1) + n1, len(p1) + n1, len(p2), len(p1) + n1]
    om = mo.Model(SMALL, small)
    om.forward(p2, 0)
    pos_p = np.array([len(p1) + n1] * B)
    pos_r = pos_p.copy()
    pos_r[2] = len(p2)
    tok2 = 77
    last_r[2] = tok2
    for i in range(3):
        last_p = plain.step_rows(last_p, pos_p + i)
        got = refill.step_rows(last_r, pos_r + i)
        logits = refill.logits()
        otok, ologits = om.step(int(last_r[2]), int(pos_r[2] + i))
        parity.check(BF16, logits[2], ologits, rel=5e-3, max_ulp=3, max_frac=0.7, what=f"refilled row step {i} logits")
        for r in (0, 1, 3):
            assert got[r] == last_p[r], (i, r)
            parity.exact(logits[r], plain.logits()[r], f"row {r} step {i} logits")
        last_r = got.copy()
        last_r[2] = otok
    for r in (0, 1, 3):
        for a, b_, name in zip(refill.export_row_kv(r, 0), plain.export_row_kv(r, 0), "KV"):
            parity.exact(a, b_, f"row {r} {name} beside a refilled row")
    assert refill.lengths()[2] == len(p2) + 3
    om.close()
    plain.release()
    refill.release()
    dec.release()


def test_a_row_stops_at_the_end_of_its_cache(acc, small):
    B, n = 4, 6
    lens = [S - 3, 40, 41, 42]
    dec = small_decoder(acc, SMALL, small)
    caches = [[random_cache(SMALL, lens[r], 600 + r)] for r in range(B)]
    batch = batch_of(dec, caches)
    got, lengths = batch.generate_rows(np.array([1, 2, 3, 4], np.int32), lens, n)
    assert list(lengths) == [3, n, n, n]
    assert (got[:3, 0] >= 0).all() and (got[3:, 0] == -1).all() and (got[:, 1:] >= 0).all()
    assert list(batch.lengths()) == [S] + [lens[r] + n for r in (1, 2, 3)]
    assert batch.export_row_kv(0, 0)[0].shape[0] == S
    batch.release()
    dec.release()


def refused(fn, words):
    import metalchat_amd as mc

    with pytest.raises(mc.McError) as e:
        fn()
    assert e.value.status == 1, str(e.value)
    assert words in str(e.value), str(e.value)


def test_refusals(acc, small):
    dec = small_decoder(acc, SMALL, small)
    batch = batch_of(dec, [[random_cache(SMALL, 10, 5)], None])
    dec.launch_log(True)
    cases = [
        (lambda: batch.step_rows([1, 2], [11, -1]), "row 0: position 11 is past the row's length 10"),
        (lambda: batch.step_rows([1, 2], [10, 1]), "row 1: position 1 is past the row's length 0"),
        (lambda: batch.generate_rows([1, 2], [S, -1], 2), "row 0: position 256 must be below max_seq_len"),
        (lambda: batch.step_rows([1, 2], [-2, 0]), "row 0: position below -1"),
        (lambda: batch.step_rows([SMALL["vocab"], 2], [10, -1]), "row 0: token id outside the vocabulary"),
        (lambda: batch.generate_rows([1, -5], [10, 0], 2), "row 1: token id outside the vocabulary"),
        (lambda: batch.generate_rows([1, 2], [10, 0], 0), "n must be positive"),
        (lambda: batch.generate_rows([1, 2], [-1, -1], 3), "no active row"),
        (lambda: batch.step_rows([-1, -1], [-1, -1]), "no active row"),
    ]
    for fn, words in cases:
        refused(fn, words)
        assert dec.launched() == [], words
    assert list(batch.lengths()) == [10, 0]
    batch.release()
    dec.release()


def test_the_decoder_is_untouched(acc, small):
    import metalchat_amd as mc

    ref = small_decoder(acc, SMALL, small)
    ref.step(9, 0)
    want = ref.logits()
    dec = small_decoder(acc, SMALL, small)
    before = dec.derived_weight_bytes()
    batch = mc.Batch(dec, 8)
    batch.generate_rows(np.arange(8, dtype=np.int32) * 5, [0, -1, 0, -1, 0, 0, 0, 0], 6, stop=[1, 2, 3])
    batch.step_rows(np.arange(8, dtype=np.int32), [1, -1, 0, -1, 1, 0, 1, 0])
    dec.step(9, 0)
    assert np.array_equal(dec.logits(), want)
    assert dec.derived_weight_bytes() == before == 0
    batch.release()
    ref.release()
    dec.release()
