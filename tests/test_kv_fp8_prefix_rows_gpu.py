"""Shared-prefix rows on an fp8 batch (mc_kv_prefix_set, Part 2s) through the public calls: rows attached to one fp8 copy of a 100-position prefix
(shared 64, tail 36) against a twin fp8 batch whose rows hold full copies through import_kv, bit for bit; a prefix forked from the decoder;
whatever B is; what the steps launch; and the switch."""
import numpy as np
import pytest

import modelgen as mg
import parity
from test_batch_gpu import SMALL, small_decoder
from test_context_gpu import random_cache
from test_prefix_rows_gpu import FIRST, N, ORD, POS, SHARED, same_rows
from test_ragged_gpu import refused

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", params=["i4", "plain"])
def dec(acc, request):
    d = small_decoder(acc, SMALL, mg.make_model(SMALL, seed=11, **(dict(quant="i4", group=128) if request.param == "i4" else {})))
    yield d
    d.release()


def pair(dec, B, attached, ordinary=(), fork=0):
    """(fp8 batch with `attached` rows on the shared prefix, fp8 twin whose rows hold full copies); fork: the prefix is the decoder's first positions"""
    import metalchat_amd as mc

    sp, twin, prefix = mc.Batch(dec, B, wide=True, kv="fp8"), mc.Batch(dec, B, wide=True, kv="fp8"), random_cache(SMALL, N, 41)
    sp.set_kv_prefix(True)
    sp.prefix_fork(fork) if fork else sp.prefix_import_kv(0, *prefix)
    for r in attached:
        sp.attach_row(r)
        twin.fork(r, fork) if fork else twin.import_kv(r, 0, *prefix)
    for r in ordinary:
        for b in (sp, twin):
            b.import_kv(r, 0, *random_cache(SMALL, ORD, 42))
    return sp, twin


def test_attached_rows_beside_an_ordinary_and_an_idle_row(dec):
    sp, twin = pair(dec, 5, [0, 1, 3], [2])
    assert sp.kv_prefix() and not twin.kv_prefix() and sp.prefix_info() == (N, SHARED)
    assert [sp.attached(r) for r in range(5)] == [True, True, False, True, False] and list(sp.lengths()) == list(twin.lengths()) == [N, N, ORD, N, 0]
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
    for b in (sp, twin):
        b.set_kv_packed(True)
    chunk, at = [None, None, None, np.array([7, 8, 9], np.int32), None], [0, 0, 0, int(sp.lengths()[3]), 0]
    assert np.array_equal(sp.extend_rows(chunk, at), twin.extend_rows(chunk, at)) and list(sp.lengths()) == list(twin.lengths())
    same_rows(sp, twin, [(3, 3)], "materialised, then extended")


def test_a_prefix_forked_from_the_decoder(dec):
    dec.prefill(np.arange(3, 3 + 80, dtype=np.int32), 0)
    sp, twin = pair(dec, 3, [0, 2], fork=80)
    first, pos = [5, 0, 9], [80, -1, 80]
    assert sp.prefix_info() == (80, 64) and np.array_equal(sp.generate_rows(first, pos, 6)[0], twin.generate_rows(first, pos, 6)[0])
    same_rows(sp, twin, [(0, 0), (2, 2)], "forked prefix")


def test_a_wide_batch_of_attached_rows(dec):
    sp5 = pair(dec, 5, [0, 1, 3], [2])[0]
    want5, _ = sp5.generate_rows(FIRST, POS, 12)
    B = 17
    sp, twin = pair(dec, B, range(B))
    first = np.full(B, 77, np.int32)
    first[[0, 9, 16]] = FIRST[[0, 1, 3]]
    got, want = sp.generate_rows(first, [N] * B, 12)[0], twin.generate_rows(first, [N] * B, 12)[0]
    assert np.array_equal(got, want)
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
    assert {"mc_sp8_attn_scores_bfloat", "mc_sp8_attn_pv_bfloat"} <= set(attached)
    assert not any(n.startswith(("mc_sp_", "mc_b_attn_")) for n in attached), attached   # neither the bfloat16 forms nor the per-row _f8_rows ones
    assert [n for n in attached if not n.startswith("mc_sp8_")] == [n for n in plain if "attn" not in n]
    for r in (0, 1, 3):
        sp.detach_row(r, True)
    assert log(sp) == plain, "no attached row: the list of a batch that never held a prefix"


def test_the_switch(dec):
    import metalchat_amd as mc

    fp8, bf16, kv = mc.Batch(dec, 2, wide=True, kv="fp8"), mc.Batch(dec, 2), random_cache(SMALL, N, 41)
    dec.launch_log(True)
    refused(lambda: fp8.prefix_import_kv(0, *kv), "mc_prefix_import_kv: the batch holds an fp8 cache (a shared prefix is bfloat16)")
    refused(lambda: fp8.prefix_fork(10), "mc_prefix_fork: the batch holds an fp8 cache (a shared prefix is bfloat16)")
    assert mc.runtime.capi().mc_kv_prefix_set(fp8._h, 2) == 1 and "mc_kv_prefix_set: on must be 0 or 1" in mc.runtime.capi().mc_last_error().decode()
    assert dec.launched() == [] and not fp8.kv_prefix()
    dec.launch_log(False)
    fp8.set_kv_prefix(True)
    fp8.set_kv_prefix(False)                              # no prefix yet: the switch turns freely
    fp8.set_kv_prefix(True)
    fp8.prefix_import_kv(0, *kv)
    refused(lambda: fp8.set_kv_prefix(False), "mc_kv_prefix_set: the batch holds a shared prefix")
    assert fp8.kv_prefix() and fp8.prefix_info() == (N, SHARED)
    bf16.set_kv_prefix(True)                              # accepted, changes nothing
    bf16.prefix_import_kv(0, *kv)
    bf16.set_kv_prefix(False)
    assert bf16.prefix_info() == (N, SHARED)
