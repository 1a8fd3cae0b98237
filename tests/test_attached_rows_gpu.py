"""Packed chunks and verify on attached rows (mc_attached_packed_set, Part 2t) through the public calls: rows attached to one copy of a
200-position prefix (shared 192) against a twin batch whose rows hold full copies, bit for bit -- picks, accepted counts, lengths, the logits
of every chunk row, the records, the rows' exports and the ragged steps that follow; what the calls launch; the refusals."""
import numpy as np
import pytest

import modelgen as mg
import parity
from metalchat_amd import runtime
from test_batch_gpu import SMALL, small_decoder
from test_context_gpu import random_cache
from test_ragged_gpu import PAIRS, refused

pytestmark = pytest.mark.gpu
N, SHARED, ORD, B = 200, 192, 70, 4
ATTACHED = [0, 1, 3]          # row 2 is ordinary, with a cache of its own
FIRST = np.array([5, 900, 31, 1500], np.int32)


@pytest.fixture(scope="module")
def dec(acc):
    d = small_decoder(acc, SMALL, mg.make_model(SMALL, seed=11))
    d.prefill(np.arange(3, 7, dtype=np.int32), 0)   # (the decoder's first prompt pass builds its exp table: not a launch of the calls compared)
    yield d
    d.release()


def pair(dec):
    """(batch with rows 0, 1, 3 attached and the switch on, twin whose rows hold full copies); row 1 has moved by three ragged steps"""
    import metalchat_amd as mc

    sp, twin, prefix = mc.Batch(dec, B), mc.Batch(dec, B), random_cache(SMALL, N, 41)
    sp.prefix_import_kv(0, *prefix)
    sp.set_attached_packed(True)
    for b in (sp, twin):
        for r in ATTACHED:
            sp.attach_row(r) if b is sp else twin.import_kv(r, 0, *prefix)
        b.import_kv(2, 0, *random_cache(SMALL, ORD, 42))
        b.generate_rows(FIRST, [-1, N, -1, -1], 3)
    assert sp.attached_packed and not twin.attached_packed and list(sp.lengths()) == list(twin.lengths()) == [N, N + 3, ORD, N]
    return sp, twin


def chunks(dec):
    """what the verify call feeds: the model's own continuation of rows 0, 1, 3 with a wrong draft somewhere, so that some drafts are accepted"""
    cont, _ = pair(dec)[1].generate_rows(FIRST, [N, N + 3, -1, N], 15)
    rows = [np.concatenate([[FIRST[r]], cont[:n - 1, r]]).astype(np.int32) for r, n in ((0, 16), (1, 5), (3, 7))]
    rows[0][9], rows[2][3] = 7, 7
    return [rows[0], rows[1], None, rows[2]], [N, N + 3, 0, N]


def same_state(sp, twin, what):
    assert list(sp.lengths()) == list(twin.lengths()), what
    for r in range(B):
        for x, y in zip(sp.export_row_kv(r, 0), twin.export_row_kv(r, 0)):
            parity.exact(x, y, f"{what}: export of row {r}")


def attention(names):
    return [n for n in names if n.startswith(("mc_ax_", "mc_px_"))]


@pytest.mark.parametrize("mode", ["rule", "MC_PX_KEYS=128", "settings and a drawing row", "records"])
def test_verify_and_extend_on_attached_rows(dec, monkeypatch, mode):
    import metalchat_amd as mc

    if mode == "MC_PX_KEYS=128":
        monkeypatch.setenv("MC_PX_KEYS", "128")
    drafts, at = chunks(dec)
    sp, twin = pair(dec)
    for b in (sp, twin):
        if mode.startswith("settings"):
            b.set_verify_settings(True)
            b.set_row_sampler(1, mc.SAMPLER_DRAW, top_k=20, temperature=0.9, top_p=0.9)
            b.set_seeds(PAIRS)
        if mode == "records":
            b.set_logprobs(3)
    logs, res = [], []
    for b in (sp, twin):
        dec.launch_log(True)
        res.append(b.verify_rows(drafts, at))
        logs.append(dec.launched())
        dec.launch_log(False)
    (acc_a, nxt_a, picks_a), (acc_b, nxt_b, picks_b) = res
    assert list(acc_a) == list(acc_b) and list(nxt_a) == list(nxt_b), (acc_a, acc_b)
    for r in ATTACHED:
        assert np.array_equal(picks_a[r], picks_b[r]), f"picks of row {r}"
        parity.exact(sp.verify_logits()[r], twin.verify_logits()[r], f"{mode}: logits of row {r}'s chunk rows")
        if mode == "records":
            for x, y in zip(sp.verify_logprobs()[r], twin.verify_logprobs()[r]):
                assert x.tobytes() == y.tobytes(), f"records of row {r}"
    assert list(sp.lengths()) == [at[r] + acc_a[r] + 1 if r != 2 else ORD for r in range(B)]
    same_state(sp, twin, f"{mode}: after verify_rows")
    hd = SMALL["head_dim"]
    assert {f"mc_ax_sums_bfloat_hd{hd}", f"mc_ax_pv_bfloat_hd{hd}"} <= set(logs[0]) and not any(n.startswith("mc_ax_") for n in logs[1])
    assert [n for n in logs[0] if n not in attention(logs[0])] == [n for n in logs[1] if n not in attention(logs[1])]
    # a 20-token chunk (two tiles) on an attached row beside the ordinary row: mc_ax_* and mc_px_* groups in one call
    msg = [None, np.arange(40, 60, dtype=np.int32), np.array([3, 4, 5], np.int32), None]
    at2 = [0, int(sp.lengths()[1]), ORD, 0]
    dec.launch_log(True)
    got = sp.extend_rows(msg, at2)
    names = dec.launched()
    dec.launch_log(False)
    assert np.array_equal(got, twin.extend_rows(msg, at2))
    assert any(n.startswith("mc_ax_pv") for n in names) and any(n.startswith("mc_px_pv") for n in names)
    same_state(sp, twin, f"{mode}: after extend_rows")
    nxt = sp.lengths().astype(np.int32)
    ta, tb = sp.generate_rows(FIRST, nxt, 4)[0], twin.generate_rows(FIRST, nxt, 4)[0]
    assert np.array_equal(ta, tb), f"{mode}: four ragged steps behind the calls"
    same_state(sp, twin, f"{mode}: after the ragged steps")


def test_refusals(dec):
    import metalchat_amd as mc

    sp, fp8 = pair(dec)[0], mc.Batch(dec, 2, wide=True, kv="fp8")
    lens = list(sp.lengths())
    two = np.array([1, 2], np.int32)
    chunk, text = [two, None, None, None], ": row 0 is attached to the shared prefix (mc_prefix_detach it first)"
    dec.launch_log(True)
    for fn, words in [
        (lambda: sp.verify_rows(chunk, [SHARED - 1, 0, 0, 0]), "mc_verify_rows: row 0: position 191 lies inside the shared prefix"),
        (lambda: sp.extend_rows([None, None, None, two], [0, 0, 0, 10]), "mc_extend_rows: row 3: position 10 lies inside the shared prefix"),
        (lambda: sp.prefill_rows(chunk), "mc_rows_prefill" + text),
        (lambda: sp.verify_tree(chunk, [np.array([-1, 0], np.int32)] + [None] * 3, [N, 0, 0, 0]), "mc_tree_verify" + text),
        (lambda: fp8.set_attached_packed(True), "mc_attached_packed_set: the batch holds an fp8 cache"),
        (lambda: runtime._check(runtime.capi().mc_attached_packed_set(sp._h, 2)), "mc_attached_packed_set: on must be 0 or 1"),
    ]:
        refused(fn, words)
        assert list(sp.lengths()) == lens and sp.attached_packed, words
    assert dec.launched() == [], dec.launched()
    dec.launch_log(False)
