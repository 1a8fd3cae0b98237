"""Shared-prefix rows (mc_prefix_*, Part 2r) on the device: rows attached to one copy of a 100-position prefix (shared 64, tail 36) against a twin
batch whose rows hold full copies, bit for bit; whatever B is; what the steps launch; the refusals, with nothing launched and no length changed."""
import numpy as np
import pytest

import modelgen as mg
import parity
from test_batch_gpu import SMALL, small_decoder
from test_context_gpu import random_cache
from test_ragged_gpu import PAIRS, refused

pytestmark = pytest.mark.gpu
N, SHARED, ORD = 100, 64, 70      # the prefix, its shared slots, the ordinary row's own cache
FIRST = np.array([5, 900, 31, 1500, 0], np.int32)
POS = np.array([N, N, ORD, N, -1], np.int32)


@pytest.fixture(scope="module", params=["i4", "plain"])
def dec(acc, request):
    d = small_decoder(acc, SMALL, mg.make_model(SMALL, seed=11, **(dict(quant="i4", group=128) if request.param == "i4" else {})))
    yield d
    d.release()


def pair(dec, B, attached, ordinary=(), wide=False, fork=0):
    """(batch with `attached` rows on the shared prefix, twin whose rows hold full copies); fork: the prefix is the decoder's first positions"""
    import metalchat_amd as mc

    sp, twin, prefix = mc.Batch(dec, B, wide=wide), mc.Batch(dec, B, wide=wide), random_cache(SMALL, N, 41)
    sp.prefix_fork(fork) if fork else sp.prefix_import_kv(0, *prefix)
    for r in attached:
        sp.attach_row(r)
        twin.fork(r, fork) if fork else twin.import_kv(r, 0, *prefix)
    for r in ordinary:
        for b in (sp, twin):
            b.import_kv(r, 0, *random_cache(SMALL, ORD, 42))
    return sp, twin


def same_rows(a, b, rows, what):
    for ra, rb in rows:
        for x, y in zip(a.export_row_kv(ra, 0), b.export_row_kv(rb, 0)):
            parity.exact(x, y, f"{what}: export of row {ra}")


def test_attached_rows_beside_an_ordinary_and_an_idle_row(dec):
    sp, twin = pair(dec, 5, [0, 1, 3], [2])
    assert sp.prefix_info() == (N, SHARED) and [sp.attached(r) for r in range(5)] == [True, True, False, True, False]
    assert list(sp.lengths()) == list(twin.lengths()) == [N, N, ORD, N, 0]
    probe, _ = pair(dec, 5, [0, 1, 3], [2])[1].generate_rows(FIRST, POS, 40)
    stop = [int(probe[17, 1])]                           # ends row 1 mid-call at the latest
    got, gl = sp.generate_rows(FIRST, POS, 40, stop=stop)   # 40 steps: the attached rows cross slots 128 and 160
    want, wl = twin.generate_rows(FIRST, POS, 40, stop=stop)
    assert np.array_equal(got, want) and list(gl) == list(wl) and gl[1] <= 18 and list(sp.lengths()) == list(twin.lengths())
    nxt = np.where(POS >= 0, sp.lengths(), -1).astype(np.int32)
    assert np.array_equal(sp.step_rows(FIRST, nxt), twin.step_rows(FIRST, nxt))
    parity.exact(sp.logits()[:4], twin.logits()[:4], "logits behind the following step")
    same_rows(sp, twin, [(r, r) for r in range(5)], "after the calls")
    sp.detach_row(3, True)
    chunk, at = [None, None, None, np.array([7, 8, 9], np.int32), None], [0, 0, 0, int(sp.lengths()[3]), 0]
    assert np.array_equal(sp.extend_rows(chunk, at), twin.extend_rows(chunk, at)) and list(sp.lengths()) == list(twin.lengths())
    same_rows(sp, twin, [(3, 3)], "materialised, then extended")
    sp.detach_row(0, False)
    assert sp.lengths()[0] == 0 and not sp.attached(0) and not sp.attached(3)


def test_a_prefix_forked_from_the_decoder(dec):
    dec.prefill(np.arange(3, 3 + 80, dtype=np.int32), 0)
    sp, twin = pair(dec, 3, [0, 2], fork=80)
    first, pos = [5, 0, 9], [80, -1, 80]
    assert sp.prefix_info() == (80, 64) and np.array_equal(sp.generate_rows(first, pos, 6)[0], twin.generate_rows(first, pos, 6)[0])
    same_rows(sp, twin, [(0, 0), (2, 2)], "forked prefix")


def test_a_wide_batch_of_attached_rows_with_records_and_a_drawing_row(dec):
    import metalchat_amd as mc

    sp5 = pair(dec, 5, [0, 1, 3], [2])[0]
    want5, _ = sp5.generate_rows(FIRST, POS, 12)
    B = 17
    sp, twin = pair(dec, B, range(B), wide=True)
    first = np.full(B, 77, np.int32)
    first[[0, 9, 16]] = FIRST[[0, 1, 3]]
    for b in (sp, twin):
        b.set_logprobs(3)
        b.set_row_sampler(4, mc.SAMPLER_DRAW, top_k=20, temperature=0.9, top_p=0.9)
        b.set_seeds(PAIRS)
    got, want = sp.generate_rows(first, [N] * B, 12)[0], twin.generate_rows(first, [N] * B, 12)[0]
    assert np.array_equal(got, want)
    for a, b in zip(sp.logprobs(12), twin.logprobs(12)):
        assert a.tobytes() == b.tobytes(), "log-probability records"
    assert np.array_equal(got[:, [0, 9, 16]], want5[:, [0, 1, 3]]), "a row's bits do not depend on B, its index or its group"
    same_rows(sp5, sp, [(0, 0), (1, 9), (3, 16)], "B = 5 against B = 17")


def test_what_the_steps_launch(dec):
    sp, twin = pair(dec, 5, [0, 1, 3], [2])

    def log(b):
        dec.launch_log(True)
        b.step_rows(FIRST, np.where(POS >= 0, b.lengths(), -1).astype(np.int32))
        names = dec.launched()
        dec.launch_log(False)
        return names

    plain, attached = log(twin), log(sp)
    assert {"mc_sp_attn_scores_bfloat", "mc_sp_attn_pv_bfloat"} <= set(attached) and not any(n.startswith("mc_sp_") for n in plain)
    assert len(attached) <= len(plain) + SMALL["n_layers"]
    assert [n for n in attached if not n.startswith("mc_sp_")] == [n for n in plain if "attn" not in n]
    for r in (0, 1, 3):
        sp.detach_row(r, True)
    assert log(sp) == plain, "no attached row: the list of a batch that never held a prefix"


def test_refusals(dec):
    import metalchat_amd as mc

    sp = pair(dec, 5, [0, 1, 3], [2])[0]
    fp8, rolling, empty = mc.Batch(dec, 2, wide=True, kv="fp8"), mc.Batch(dec, 2), mc.Batch(dec, 2)
    rolling.set_rolling(True)
    kv, lens = random_cache(SMALL, N, 41), list(sp.lengths())
    chunk, at = [np.array([1, 2], np.int32)] + [None] * 4, [N, 0, 0, 0, 0]
    text = ": row 0 is attached to the shared prefix (mc_prefix_detach it first)"
    dec.launch_log(True)
    cases = [
        (lambda: fp8.prefix_import_kv(0, *kv), "mc_prefix_import_kv: the batch holds an fp8 cache"),
        (lambda: fp8.prefix_fork(10), "mc_prefix_fork: the batch holds an fp8 cache"),
        (lambda: rolling.prefix_import_kv(0, *kv), "mc_prefix_import_kv: the batch is rolling"),
        (lambda: rolling.prefix_fork(10), "mc_prefix_fork: the batch is rolling"),
        (lambda: sp.prefix_import_kv(0, *kv), "mc_prefix_import_kv: row 0 is attached"),
        (lambda: sp.prefix_fork(10), "mc_prefix_fork: row 0 is attached"),
        (lambda: sp.set_rolling(True), "mc_rolling_set: the batch holds a shared prefix"),
        (lambda: empty.attach_row(0), "mc_prefix_attach: the batch holds no shared prefix"),
        (lambda: sp.attach_row(5), "mc_prefix_attach: row out of range"),
        (lambda: sp.attach_row(1), "mc_prefix_attach: row 1 is already attached"),
        (lambda: sp.detach_row(2), "mc_prefix_detach: row 2 is not attached"),
        (lambda: sp.step_rows(FIRST, [SHARED - 1, N, ORD, N, -1]), "mc_ragged_step: row 0: position 63 lies inside the shared prefix"),
        (lambda: sp.generate_rows(FIRST, [N, 10, ORD, N, -1], 2), "mc_ragged_generate: row 1: position 10 lies inside the shared prefix"),
        (lambda: sp.step(FIRST, 10), "mc_batch_step" + text),
        (lambda: sp.generate(FIRST, 10, 2), "mc_batch_generate" + text),
        (lambda: sp.fork(0, 5), "mc_batch_fork" + text),
        (lambda: sp.import_kv(0, 0, *kv), "mc_batch_import_kv" + text),
        (lambda: sp.export_kv(0, 0), "mc_batch_export_kv" + text),
        (lambda: sp.fork_row(0, 2), "mc_rolling_fork_row" + text),
        (lambda: sp.fork_row(2, 0), "mc_rolling_fork_row" + text),
        (lambda: sp.prefill_rows(chunk), "mc_rows_prefill" + text),
        (lambda: sp.extend_rows(chunk, at), "mc_extend_rows" + text),
        (lambda: sp.verify_rows(chunk, at), "mc_verify_rows" + text),
        (lambda: sp.verify_tree(chunk, [np.array([-1, 0], np.int32)] + [None] * 4, at), "mc_tree_verify" + text),
    ]
    for fn, words in cases:
        refused(fn, words)
        assert list(sp.lengths()) == lens, words
    assert dec.launched() == [], dec.launched()
    dec.launch_log(False)
