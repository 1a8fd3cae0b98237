"""The packed passes on an fp8 batch (mc_kv_packed_set, include/metalchat_hip.h Part 2p) through the public calls, on the small synthetic
decoder of test_batch_gpu.py with int4 and with plain weights.  What can be pinned bit for bit is: layer 0's K / V depend on no cache, so
their export is deq(quant(.)) of a bfloat16 batch's after the same call (tests/kv_fp8_rule.py), a row's bits do not depend on its company,
and verify_rows picks what extend_rows' logits say.  The one statement about accuracy is measured against the bfloat16 batch."""
import numpy as np
import pytest

import kv_fp8_rule as kr
import parity
import verify_rule as vr
from oracle import mc_oracle as mo
from test_batch_gpu import SMALL, refused, small_decoder
from test_kv_fp8_batch_gpu import prompt as toks, weights  # noqa: F401 (the module's fixture: int4 and plain weights of SMALL)

pytestmark = pytest.mark.gpu
PROMPTS, CHUNKS = (5, 16, 33), (3, 17)


@pytest.fixture(params=["i4", "w"])
def dec(request, acc, weights):
    d = small_decoder(acc, SMALL, weights[request.param])
    yield d
    d.release()


def batch(dec, B, kv="fp8", on=True):
    import metalchat_amd as mc

    b = mc.Batch(dec, B, wide=True, kv=kv)
    b.set_kv_packed(on)
    return b


def rel_l2(got, ref):
    got, ref = (mo.from_bf16(x).astype(np.float64) for x in (got, ref))
    return float(np.linalg.norm(got - ref) / np.linalg.norm(ref))   # (a NaN fails the bound)


def test_the_switch_admits_three_calls_and_never_the_tree(dec):
    f8 = batch(dec, 3, on=False)
    chunk, tree, text = [toks(3, 1), None, None], [np.array([-1, 0, 0], np.int32), None, None], ": the batch holds an fp8 cache"
    for on in (False, True):
        f8.set_kv_packed(on)
        assert f8.kv_packed == on
        refused(lambda: f8.verify_tree(chunk, tree, [0, -1, -1]), "mc_tree_verify" + text)
        if not on:
            refused(lambda: f8.prefill_rows(chunk), "mc_rows_prefill" + text)
            refused(lambda: f8.extend_rows(chunk, [0, -1, -1]), "mc_extend_rows" + text)
            refused(lambda: f8.verify_rows(chunk, [0, -1, -1]), "mc_verify_rows" + text)
    parity.exact(f8.lengths(), np.zeros(3, np.int32), "the lengths after the refused calls")
    f8.prefill_rows(chunk)
    refused(lambda: f8.extend_rows([toks(2, 2), None, None], [5, -1, -1]), "is past the row's length 3")   # (its own admission holds)
    f8.release()


def same_row(call, alone, among):
    """row 1 of the batch of two against row 3 of the batch of four"""
    for x, y, name in zip((alone.logits()[1],) + alone.export_row_kv(1, 0), (among.logits()[3],) + among.export_row_kv(3, 0), ("logits", "K", "V")):
        parity.exact(x, y, f"{call}: the row's {name} alone and among other rows")


def test_layer0_export_and_placement(dec):
    prompts = [toks(n, 10 + n) for n in PROMPTS]
    f8, b16, alone = batch(dec, 4), batch(dec, 4, kv="bf16"), batch(dec, 2)
    for b in (f8, b16):
        b.prefill_rows([prompts[0], None, prompts[1], prompts[2]])
    alone.prefill_rows([None, prompts[2]])
    for r, n in ((0, 5), (2, 16), (3, 33)):
        (gk, gv), (rk_, rv) = f8.export_row_kv(r, 0), b16.export_row_kv(r, 0)
        assert gk.shape[0] == n
        parity.exact(gk, kr.roundtrip(rk_), f"row {r}: layer-0 K is deq(quant(K of the bfloat16 batch))")
        parity.exact(gv, kr.roundtrip(rv), f"row {r}: layer-0 V")
    same_row("prefill_rows", alone, f8)
    # extend_rows behind 40 tokens: row 3 holds 33, a chunk of 7 brings it (and the lone row) to 40
    more, chunk = toks(7, 50), toks(17, 51)
    f8.extend_rows([toks(3, 52), None, None, more], [5, -1, -1, 33])
    alone.extend_rows([None, more], [-1, 33])
    f8.extend_rows([None, None, toks(3, 53), chunk], [-1, -1, 16, 40])
    alone.extend_rows([None, chunk], [-1, 40])
    same_row("extend_rows", alone, f8)
    for b in (f8, b16, alone):
        b.release()


# relative L2 error of the fp8 batch's logits against the bfloat16 batch's making the same calls, as measured on an MI355X with these weights:
# after prefill_rows (all rows), after extend_rows (its rows), after the ragged step behind them.  The assertions allow twice that, Part 2o's margin.
MEASURED = {"i4": (1.00491e-2, 8.53348e-3, 7.88438e-3), "w": (7.70684e-3, 6.86368e-3, 6.88912e-3)}


def test_logits_stay_close_to_the_bfloat16_batch_and_a_step_continues(dec, request):
    fmt = request.node.callspec.params["dec"]
    prompts, chunks = [toks(n, 20 + n) for n in PROMPTS], [toks(CHUNKS[0], 30), None, toks(CHUNKS[1], 31)]
    f8, b16 = batch(dec, 3), batch(dec, 3, kv="bf16")
    for b in (f8, b16):
        b.prefill_rows(prompts)
    errs = [rel_l2(f8.logits(), b16.logits())]
    for b in (f8, b16):
        b.extend_rows(chunks, [PROMPTS[0], -1, PROMPTS[2]])
    errs.append(rel_l2(f8.logits()[[0, 2]], b16.logits()[[0, 2]]))
    for b in (f8, b16):
        assert np.all(b.step_rows(toks(3, 32), [PROMPTS[0] + CHUNKS[0], PROMPTS[1], PROMPTS[2] + CHUNKS[1]]) >= 0)
    errs.append(rel_l2(f8.logits(), b16.logits()))
    print(f"kv fp8 packed closeness {fmt}: relative L2 error of the logits after prefill, extend, a ragged step: {errs}")
    assert all(e <= 2 * m for e, m in zip(errs, MEASURED[fmt])), (fmt, errs, MEASURED[fmt])
    for b in (f8, b16):
        b.release()


def test_verify_rows_picks_what_extend_rows_logits_say(dec):
    ctx, drafts = [toks(n, 40 + n) for n in (33, 16)], [toks(4, 60), toks(4, 61)]   # [the last accepted token, a 3-token draft]
    f8 = batch(dec, 2)
    f8.prefill_rows(ctx)
    first = f8.verify_rows(drafts, [33, 16])[2]
    drafts[0][1] = first[0][0]                           # row 0's first draft is what the target picks: accepted
    acc_, nxt, picks = f8.verify_rows(drafts, [33, 16])  # (the rejected drafts' slots stay written past the length: rewound, written again)
    for r in range(2):                                   # a twin per prefix of the chunk (extend_rows takes 2 tokens and more)
        for i in range(1, 4):
            twin = batch(dec, 2)
            twin.prefill_rows(ctx)
            twin.extend_rows([drafts[q][:i + 1] if q == r else None for q in range(2)], [len(ctx[q]) if q == r else -1 for q in range(2)])
            assert picks[r][i] == int(np.argmax(mo.from_bf16(twin.logits()[r]))), f"row {r}: the pick after chunk row {i}"
            twin.release()
    ea, en = vr.accept_rows(drafts, picks)
    parity.exact(acc_, ea, "accepted lengths by tests/verify_rule.py")
    parity.exact(nxt, en, "next tokens by tests/verify_rule.py")
    assert picks[0][0] == first[0][0] and acc_[0] >= 1
    parity.exact(f8.lengths(), np.array([33, 16], np.int32) + acc_ + 1, "the rows' lengths")
    f8.release()
