"""Packed chunks and verify on attached rows of an fp8 batch (Part 2u) through the public calls: test_attached_rows_gpu.py's layout on an fp8 batch with
its three switches on, against an fp8 twin whose rows hold full copies, bit for bit; what the calls launch; and the switch."""
import numpy as np
import pytest

import modelgen as mg
import parity
from test_attached_rows_gpu import ATTACHED, B, FIRST, N, ORD, attention, chunks, same_state
from test_batch_gpu import SMALL, small_decoder
from test_context_gpu import random_cache
from test_ragged_gpu import refused

pytestmark = pytest.mark.gpu
HD = SMALL["head_dim"]


@pytest.fixture(scope="module", params=["i4", "plain"])
def dec(acc, request):
    d = small_decoder(acc, SMALL, mg.make_model(SMALL, seed=11, **(dict(quant="i4", group=128) if request.param == "i4" else {})))
    d.prefill(np.arange(3, 7, dtype=np.int32), 0)   # (the decoder's first prompt pass builds its exp table: not a launch of the calls compared)
    yield d
    d.release()


def pair(dec):
    """(fp8 batch with rows 0, 1, 3 attached and the three switches on, fp8 twin whose rows hold full copies); row 1 has moved by three ragged steps"""
    import metalchat_amd as mc

    sp, twin, prefix = mc.Batch(dec, B, wide=True, kv="fp8"), mc.Batch(dec, B, wide=True, kv="fp8"), random_cache(SMALL, N, 41)
    sp.set_kv_prefix(True)
    sp.prefix_import_kv(0, *prefix)
    for b in (sp, twin):
        b.set_kv_packed(True)
        for r in ATTACHED:
            sp.attach_row(r) if b is sp else twin.import_kv(r, 0, *prefix)
        b.import_kv(2, 0, *random_cache(SMALL, ORD, 42))
        b.generate_rows(FIRST, [-1, N, -1, -1], 3)
    sp.set_attached_packed(True)
    assert sp.attached_packed and not twin.attached_packed and list(sp.lengths()) == list(twin.lengths()) == [N, N + 3, ORD, N]
    return sp, twin


def logged(dec, call):
    dec.launch_log(True)
    out, names = call(), dec.launched()
    dec.launch_log(False)
    return out, names, [n for n in names if n not in attention(names) and not n.startswith(("mc_ax8_", "mc_px8_"))]


@pytest.mark.parametrize("mode", ["rule", "MC_PX_KEYS=128", "records"])
def test_verify_and_extend_on_attached_fp8_rows(dec, monkeypatch, mode):
    if mode == "MC_PX_KEYS=128":
        monkeypatch.setenv("MC_PX_KEYS", "128")
    drafts, at = chunks(dec)   # (a bfloat16 batch's continuation with a wrong draft in two rows: drafts are drafts)
    sp, twin = pair(dec)
    if mode == "records":
        sp.set_logprobs(3), twin.set_logprobs(3)
    (acc_a, nxt_a, picks_a), names, rest = logged(dec, lambda: sp.verify_rows(drafts, at))
    (acc_b, nxt_b, picks_b), names_b, rest_b = logged(dec, lambda: twin.verify_rows(drafts, at))
    assert list(acc_a) == list(acc_b) and list(nxt_a) == list(nxt_b), (acc_a, acc_b)
    for r in ATTACHED:
        assert np.array_equal(picks_a[r], picks_b[r]), f"picks of row {r}"
        parity.exact(sp.verify_logits()[r], twin.verify_logits()[r], f"{mode}: logits of row {r}'s chunk rows")
        if mode == "records":
            assert [x.tobytes() for x in sp.verify_logprobs()[r]] == [y.tobytes() for y in twin.verify_logprobs()[r]], f"records of row {r}"
    same_state(sp, twin, f"{mode}: after verify_rows")
    assert {f"mc_ax8_sums_bfloat_hd{HD}", f"mc_ax8_pv_bfloat_hd{HD}"} <= set(names) and rest == rest_b
    assert not any(n.startswith(("mc_ax_", "mc_ax8_")) for n in names_b) and not any(n.startswith("mc_ax_") for n in names)
    # a 20-token chunk (two tiles) on an attached row beside the ordinary row: mc_ax8_* and mc_px8_* groups in one call
    msg, at2 = [None, np.arange(40, 60, dtype=np.int32), np.array([3, 4, 5], np.int32), None], [0, int(sp.lengths()[1]), ORD, 0]
    got, names, _ = logged(dec, lambda: sp.extend_rows(msg, at2))
    assert np.array_equal(got, twin.extend_rows(msg, at2))
    assert any(n.startswith("mc_ax8_pv") for n in names) and any(n.startswith("mc_px8_pv") for n in names) and not any(n.startswith("mc_ax_") for n in names)
    same_state(sp, twin, f"{mode}: after extend_rows")
    nxt = sp.lengths().astype(np.int32)
    assert np.array_equal(sp.generate_rows(FIRST, nxt, 4)[0], twin.generate_rows(FIRST, nxt, 4)[0]), f"{mode}: four ragged steps behind the calls"
    same_state(sp, twin, f"{mode}: after the ragged steps")


def test_the_switch(dec):
    import metalchat_amd as mc

    fp8 = mc.Batch(dec, B, wide=True, kv="fp8")
    dec.launch_log(True)
    for prefix_on, packed_on in ((False, False), (True, False), (False, True)):   # either fp8 switch off: refused, the hint names both
        fp8.set_kv_prefix(prefix_on), fp8.set_kv_packed(packed_on)
        refused(lambda: fp8.set_attached_packed(True), "mc_attached_packed_set: the batch holds an fp8 cache")
        refused(lambda: fp8.set_attached_packed(True), "mc_kv_prefix_set and mc_kv_packed_set")
    fp8.set_kv_prefix(True)
    assert not fp8.attached_packed and dec.launched() == []
    dec.launch_log(False)
    fp8.set_attached_packed(True)                                                 # both on: admitted
    sp = pair(dec)[0]
    sp.set_kv_tree(True)
    lens, chunk = list(sp.lengths()), [np.array([1, 2], np.int32), None, None, None]
    words = ": row 0 is attached to the shared prefix (mc_prefix_detach it first)"
    dec.launch_log(True)
    refused(lambda: sp.prefill_rows(chunk), "mc_rows_prefill" + words)
    refused(lambda: sp.verify_tree(chunk, [np.array([-1, 0], np.int32)] + [None] * 3, [N, 0, 0, 0]), "mc_tree_verify" + words)
    sp.set_kv_packed(False)                                                       # the packed passes' own refusal comes first
    refused(lambda: sp.extend_rows(chunk, [N, 0, 0, 0]), "mc_extend_rows: the batch holds an fp8 cache, which the packed passes do not read or write")
    assert dec.launched() == [] and list(sp.lengths()) == lens and fp8.attached_packed and sp.attached_packed
    dec.launch_log(False)
