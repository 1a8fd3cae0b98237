"""fp8 KV caches for batch rows (mc_kv_batch_create, include/metalchat_hip.h Part 2o) through the public calls, on the small synthetic
decoder of the wide-batch tests with int4 and with plain weights.  The format is a storage format: what can be pinned bit for bit is
pinned that way -- layer 0's K / V do not depend on attention, so its export is deq(quant(.)) of a bfloat16 batch's (tests/kv_fp8_rule.py),
and a row's bits do not depend on B or its company -- and the one statement about accuracy is measured against the bfloat16 batch."""
import numpy as np
import pytest

import kv_fp8_rule as kr
import modelgen as mg
import parity
from oracle import mc_oracle as mo
from test_batch_gpu import SMALL, refused, small_decoder
from test_context_gpu import random_cache

pytestmark = pytest.mark.gpu
S, HD, VOCAB = SMALL["max_seq_len"], SMALL["head_dim"], SMALL["vocab"]


@pytest.fixture(scope="module")
def weights():
    return {"i4": mg.make_model(SMALL, seed=11, quant="i4", group=128), "w": mg.make_model(SMALL, seed=12)}


def prompt(n, seed):
    return np.random.default_rng(seed).integers(0, VOCAB, n).astype(np.int32)


def test_creation_reports_the_format_and_the_bytes(acc, weights):
    import metalchat_amd as mc

    dec = small_decoder(acc, SMALL, weights["i4"])
    B = 3
    f8, b16, wide = mc.Batch(dec, B, wide=True, kv="fp8"), mc.Batch(dec, B, wide=True, kv="bf16"), mc.Batch(dec, B, wide=True)
    assert (f8.kv_format, b16.kv_format, wide.kv_format) == ("fp8", "bf16", "bf16")
    full = 2 * SMALL["n_layers"] * B * SMALL["n_kv_heads"] * S * HD * 2
    assert b16.kv_bytes == wide.kv_bytes == full
    assert f8.kv_bytes * 2 * HD == full * (HD + 1)
    # MC_KV_BF16 steps as mc_wide_batch_create's batch does, bit for bit
    toks = np.array([5, 900, 77], np.int32)
    for pos in range(3):
        nxt = [b.step(toks, pos) for b in (b16, wide)]
        parity.exact(nxt[0], nxt[1], f"MC_KV_BF16 picks at {pos}")
        parity.exact(b16.logits(), wide.logits(), f"MC_KV_BF16 logits at {pos}")
        toks = nxt[0]
    refused(lambda: mc.Batch(dec, B, wide=True, kv=2), "mc_kv_batch_create: kv_format must be MC_KV_BF16 (0) or MC_KV_FP8 (1)")
    refused(lambda: mc.Batch(dec, 65, wide=True, kv="fp8"), "mc_kv_batch_create: batch must lie in [1, 64]")
    # the four packed calls: refused with their text, nothing enqueued, the lengths as they were
    f8.import_kv(0, 0, *random_cache(SMALL, 10, 1))
    before = f8.lengths().copy()
    chunk = [np.array([3, 4, 5], np.int32), None, None]
    text = ": the batch holds an fp8 cache"
    refused(lambda: f8.prefill_rows(chunk), "mc_rows_prefill" + text)
    refused(lambda: f8.extend_rows(chunk, [10, -1, -1]), "mc_extend_rows" + text)
    refused(lambda: f8.verify_rows(chunk, [10, -1, -1]), "mc_verify_rows" + text)
    refused(lambda: f8.verify_tree(chunk, [np.array([-1, 0, 0], np.int32), None, None], [10, -1, -1]), "mc_tree_verify" + text)
    parity.exact(f8.lengths(), before, "the lengths after the refused calls")
    for b in (f8, b16, wide):
        b.release()
    dec.release()


@pytest.mark.parametrize("fmt", ["i4", "w"])
def test_layer0_export_is_deq_of_quant_and_rolls(acc, weights, fmt):
    """fork behind the decoder's prompt pass, ragged steps across the 64-slot boundary with an idle row; then one row imported near the
    end of its cache rolls past max_seq_len.  Both batches are fed the same tokens, so layer 0's K / V are the same values before storage."""
    import metalchat_amd as mc

    dec = small_decoder(acc, SMALL, weights[fmt])
    n0, B = 62, 3
    dec.prefill(prompt(n0, 3), 0)
    f8, b16 = mc.Batch(dec, B, wide=True, kv="fp8"), mc.Batch(dec, B, wide=True)
    for b in (f8, b16):
        b.fork(0, n0)
        b.fork(2, n0 - 7)
        for i in range(4):                          # row 0 writes slots 62 .. 65, row 2 slots 55 .. 58, row 1 is idle
            nxt = b.step_rows(prompt(B, 100 + i), [n0 + i, -1, n0 - 7 + i])
            assert nxt[1] == -1 and nxt[0] >= 0
    for r, n in ((0, n0 + 4), (2, n0 - 3)):
        (gk, gv), (rk, rv) = f8.export_row_kv(r, 0), b16.export_row_kv(r, 0)
        assert gk.shape == (n, SMALL["n_kv_heads"], HD)
        parity.exact(gk, kr.roundtrip(rk), f"{fmt} row {r}: layer-0 K is deq(quant(K of the bfloat16 batch))")
        parity.exact(gv, kr.roundtrip(rv), f"{fmt} row {r}: layer-0 V")
    assert np.any(gk != rk), "the fp8 export is not the bfloat16 export"
    # the lockstep view of the export, and a copy of the planes as they lie
    f8.fork_row(1, 0)
    parity.exact(f8.export_row_kv(1, 0)[1], f8.export_row_kv(0, 0)[1], "mc_rolling_fork_row copies bytes and exponents")
    # one rolled row: imported up to S - 3, then 8 steps on the ring
    k0, v0 = random_cache(SMALL, S - 3, 9)
    for b in (f8, b16):
        b.set_rolling(True)
        b.import_kv(1, 0, k0, v0)
        for i in range(8):
            b.step_rows(prompt(B, 200 + i), [-1, S - 3 + i, -1])
    assert f8.lengths()[1] == S + 5
    (gk, gv), (rk, rv) = f8.export_row_kv(1, 0), b16.export_row_kv(1, 0)
    assert gk.shape[0] == S
    parity.exact(gk, kr.roundtrip(rk), f"{fmt}: the rolled row's K, the ring unrolled")
    parity.exact(gv, kr.roundtrip(rv), f"{fmt}: the rolled row's V")
    for b in (f8, b16):
        b.release()
    dec.release()


@pytest.mark.parametrize("fmt", ["i4", "w"])
def test_a_rows_bits_do_not_depend_on_the_batch(acc, weights, fmt):
    import metalchat_amd as mc

    dec = small_decoder(acc, SMALL, weights[fmt])
    n = 61
    k, v = random_cache(SMALL, n, 21)
    k2, v2 = random_cache(SMALL, 30, 22)

    def run(B, row, other):
        b = mc.Batch(dec, B, wide=True, kv="fp8")
        b.import_kv(row, 0, k, v)
        pos, tok = [-1] * B, [0] * B
        pos[row], tok[row] = n, 77
        if other is not None:
            b.import_kv(other, 0, k2, v2)
            pos[other], tok[other] = 30, 5
        toks, made = b.generate_rows(tok, pos, 6)          # across the 64-slot boundary
        logits = b.logits()[row].copy()
        b.release()
        assert made[row] == 6
        return toks[:, row], logits

    alone, together = run(1, 0, None), run(3, 2, 0)        # row 1 of the batch of three stays idle
    parity.exact(together[0], alone[0], f"{fmt}: the row's tokens at B = 1 and B = 3")
    parity.exact(together[1], alone[1], f"{fmt}: the row's logits at B = 1 and B = 3")
    dec.release()


# the relative L2 error of the fp8 batch's logits against the bfloat16 batch's after 16 steps behind a forked prompt of 48 tokens, as measured on
# an MI355X with these weights: int4 5.29e-3, plain 5.02e-3.  The assertion allows twice that for other seeds of the synthetic weights;
# e4m3's relative step of 2^-4 makes anything tighter a statement about the seed.
MEASURED = {"i4": 5.2897e-3, "w": 5.01904e-3}


@pytest.mark.parametrize("fmt", ["i4", "w"])
def test_logits_stay_close_to_the_bfloat16_batch(acc, weights, fmt):
    import metalchat_amd as mc

    dec = small_decoder(acc, SMALL, weights[fmt])
    n0, B = 48, 2
    dec.prefill(prompt(n0, 5), 0)
    f8, b16 = mc.Batch(dec, B, wide=True, kv="fp8"), mc.Batch(dec, B, wide=True)
    for b in (f8, b16):
        for r in range(B):
            b.fork(r, n0)
    toks = np.array([11, 1200], np.int32)
    for i in range(16):                                     # both batches are fed the bfloat16 batch's picks
        f8.step(toks, n0 + i)
        toks = b16.step(toks, n0 + i)
    got, ref = (mo.from_bf16(b.logits()).astype(np.float64) for b in (f8, b16))
    err = float(np.linalg.norm(got - ref) / np.linalg.norm(ref))
    print(f"kv fp8 closeness {fmt}: relative L2 error of the logits {err:.6g}")
    assert np.all(np.isfinite(got))
    assert err <= 2 * MEASURED[fmt], f"{fmt}: relative L2 error {err:.4g} against the bfloat16 batch (measured {MEASURED[fmt]:.4g})"
    for b in (f8, b16):
        b.release()
    dec.release()
