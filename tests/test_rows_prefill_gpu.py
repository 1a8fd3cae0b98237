"""The packed prompt pass (mc_rows_prefill, include/metalchat_hip.h Part 2d) on the device: the prompts of several batch rows in
one prompt pass over the decoder's weights.

  * each row against its own oracle.Model.forward (K / V of its new positions, last-row logits, the pick), with prompt lengths
    across 16- and 64-row boundaries and rows at positions > 0, at SMALL (int4 g128, head_dim 128) and Llama-3.2-1B widths
    (bfloat weights, head_dim 64), with the bounds of test_prefill_gpu.check_against_oracle;
  * every weight matrix is multiplied once per call, as for one prompt of the same total length;
  * where a prompt is packed does not change its bits; one prompt packed alone equals mc_decoder_prefill + mc_batch_fork;
  * ragged steps and a second packed chunk continue from the call; rows outside the call and the decoder are untouched;
  * the refusals, with nothing launched.
"""
import ctypes as C

import numpy as np
import pytest

import modelgen as mg
import parity
from oracle import mc_oracle as mo
from test_batch_gpu import LLAMA32_1B, SMALL, small_decoder
from test_context_gpu import random_cache
from test_prefill_gpu import tol

pytestmark = pytest.mark.gpu
BF16 = 0
LENS = [2, 15, 16, 17, 31, 33, 64, 65]  # 243 rows <= max_seq_len 256: across 16- and 64-row tile boundaries
POS = [0, 7, 0, 40, 0, 3, 0, 20]        # rows 1, 3, 5 and 7 start behind an earlier context


@pytest.fixture(scope="module")
def small():
    return mg.make_model(SMALL, seed=11, quant="i4", group=128)


@pytest.fixture(scope="module")
def llama1b():
    return mg.make_model(LLAMA32_1B, seed=5)


def prompts_of(cfg, lens, seed):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, cfg["vocab"], n).astype(np.int32) for n in lens]


def clear_gap(logits_T):
    """the oracle's pick is unambiguous: its top two logits lie more than two bfloat steps apart"""
    v = np.sort(mo.from_bf16(logits_T).astype(np.float64))
    rms = np.sqrt(np.mean(v * v))
    return v[-1] - v[-2] > 2 * 2.0 ** -7 * max(abs(v[-1]), rms)


def setup_rows(dec, cfg, weights, positions, seed):
    """a batch whose row r holds a random context of positions[r] rows (none for 0), and row r's oracle with the same context"""
    import metalchat_amd as mc

    B = len(positions)
    batch = mc.Batch(dec, B)
    oms = []
    for r, p in enumerate(positions):
        om = mo.Model(cfg, weights)
        for layer in range(cfg["n_layers"]):
            if p:
                k, v = random_cache(cfg, p, seed + 100 * r + layer)
                batch.import_kv(r, layer, k, v)
                om.set_kv(layer, k, v)
        oms.append(om)
    return batch, oms


def check_rows(cfg, batch, oms, prompts, positions, picks, what, exact_context=True):
    """row r against oms[r].forward(prompts[r], positions[r]): K / V of the first and last layer at the new positions (an imported
    context bit for bit), the last-row logits and the pick"""
    rel, frac = tol(BF16)
    logits = batch.logits()
    for r, (tokens, p) in enumerate(zip(prompts, positions)):
        if tokens is None:
            continue
        otok, ologits = oms[r].forward(tokens, p, 0)
        n = len(tokens)
        parity.check(BF16, logits[r], ologits, rel=rel, max_ulp=2, max_frac=frac, what=f"{what} row {r} logits")
        assert picks[r] == int(np.argmax(mo.from_bf16(logits[r]))), (what, r)
        if clear_gap(ologits):
            assert picks[r] == otok, (what, r, picks[r], otok)
        for layer in sorted({0, cfg["n_layers"] - 1}):
            gk, gv = batch.export_row_kv(r, layer)
            ok, ov = oms[r].kv(layer)
            assert gk.shape == ok.shape == (p + n, cfg["n_kv_heads"], cfg["head_dim"]), (what, r)
            if exact_context:
                parity.exact(gk[:p], ok[:p], f"{what} row {r} layer {layer} context K")
                parity.exact(gv[:p], ov[:p], f"{what} row {r} layer {layer} context V")
            parity.check(BF16, gk[p:], ok[p:], rel=rel, max_ulp=2, max_frac=frac, what=f"{what} row {r} layer {layer} K")
            parity.check(BF16, gv[p:], ov[p:], rel=rel, max_ulp=2, max_frac=frac, what=f"{what} row {r} layer {layer} V")


@pytest.mark.parametrize("shape", ["small-int4", "llama32-1b-bf16"])
def test_rows_against_the_oracle(acc, small, llama1b, shape):
    cfg, weights = (SMALL, small) if shape == "small-int4" else (LLAMA32_1B, llama1b)
    # (Llama-3.2-1B widths: four of the rows -- the oracle's prompt pass is plain C)
    lens, pos = (LENS, POS) if cfg is SMALL else ([2, 17, 33, 65], [0, 7, 0, 20])
    dec = small_decoder(acc, cfg, weights)
    batch, oms = setup_rows(dec, cfg, weights, pos, 500)
    prompts = prompts_of(cfg, lens, 1)
    dec.launch_log(True)
    picks = batch.prefill_rows(prompts, pos)
    names = set(dec.launched())
    assert list(batch.lengths()) == [p + n for p, n in zip(pos, lens)]
    check_rows(cfg, batch, oms, prompts, pos, picks, shape)
    hd = cfg["head_dim"]
    assert {"mc_pp_gather_last_bfloat", "mc_b_rmsnorm_bfloat", "mc_b_argmax_rows_bfloat"} <= names, sorted(names)
    assert {f"mc_pp_attn2_bfloat_hd{hd}", f"mc_pp_attn_bfloat_hd{hd}"} & names, sorted(names)
    assert {"mc_pp_rope_cache_bfloat", "mc_pp_rope_cache_parts_bfloat"} & names, sorted(names)
    assert not [n for n in names if n.startswith(("mc_pf_rope", "mc_pf_attn", "mc_argmax", "mc_gemv_"))], sorted(names)
    batch.release()
    for om in oms:
        om.close()
    dec.release()


def gemm_launches(names):
    return [n for n in names if n.startswith(("mc_pf_gemm", "mc_pf2_gemm", "hipblasLt"))]


def test_each_weight_matrix_is_multiplied_once(acc, small):
    import metalchat_amd as mc

    dec = small_decoder(acc, SMALL, small)
    prompts = prompts_of(SMALL, LENS, 2)
    batch = mc.Batch(dec, 8)
    dec.launch_log(True)
    batch.prefill_rows(prompts)
    packed = dec.launched()
    # one prompt of the same total length through the decoder: the same GEMM launches, in the same order
    dec.launch_log(True)
    dec.prefill(np.concatenate(prompts), 0)
    single = dec.launched()
    L = SMALL["n_layers"]
    assert gemm_launches(packed) == gemm_launches(single), (packed, single)
    mats = [n for n in gemm_launches(packed) if not n.startswith("mc_pf_splitk")]
    assert len(mats) == 4 * L, packed  # wq|wk|wv, wo, w1|w3, w2
    for name, per_call in (("mc_pp_gather_last_bfloat", 1), ("mc_b_gemv_i4_bfloat_e0", 1), ("mc_pf_embed_bfloat", 1)):
        assert packed.count(name) == per_call, (name, packed)
    assert len([n for n in packed if n.startswith("mc_pp_rope_cache")]) == L
    assert len([n for n in packed if n.startswith("mc_pp_attn")]) == L
    assert len(packed) < 20 * L + 10, packed  # nothing per row
    batch.release()
    dec.release()


def test_placement_does_not_matter(acc, small):
    import metalchat_amd as mc

    dec = small_decoder(acc, SMALL, small)
    prompts = prompts_of(SMALL, LENS, 3)
    perm = [5, 2, 7, 0, 3, 6, 1, 4]  # prompt i goes to row perm[i]
    a, b = mc.Batch(dec, 8), mc.Batch(dec, 8)
    pa = a.prefill_rows(prompts)
    la = a.logits()
    moved = [None] * 8
    for i, r in enumerate(perm):
        moved[r] = prompts[i]
    pb = b.prefill_rows(moved)
    lb = b.logits()
    for i, r in enumerate(perm):
        assert pa[i] == pb[r], (i, r)
        parity.exact(lb[r], la[i], f"prompt {i}: logits")
        for (ka, va), (kb, vb) in [(a.export_row_kv(i, 0), b.export_row_kv(r, 0))]:
            parity.exact(kb, ka, f"prompt {i}: K")
            parity.exact(vb, va, f"prompt {i}: V")
    a.release()
    b.release()
    dec.release()


def test_one_prompt_alone_equals_the_decoder(acc, llama1b):
    import metalchat_amd as mc

    cfg = LLAMA32_1B
    dec = small_decoder(acc, cfg, llama1b)
    tokens = prompts_of(cfg, [45], 4)[0]
    forked = mc.Batch(dec, 2)
    dec.prefill(tokens, 0)
    forked.fork(1, len(tokens))
    packed = mc.Batch(dec, 2)
    picks = packed.prefill_rows([None, tokens])
    assert picks[0] == -1
    for name, (a, b) in zip("KV", zip(packed.export_row_kv(1, 0), forked.export_kv(1, 0))):
        parity.exact(a, b, f"layer 0 {name}")
    om = mo.Model(cfg, llama1b)
    om.forward(tokens, 0, 0)
    rel, frac = tol(BF16)
    for name, (a, b) in zip("KV", zip(packed.export_row_kv(1, cfg["n_layers"] - 1), om.kv(cfg["n_layers"] - 1))):
        parity.check(BF16, a, b, rel=rel, max_ulp=2, max_frac=frac, what=f"last layer {name}")
    om.close()
    packed.release()
    forked.release()
    dec.release()


def test_decode_and_a_second_chunk_continue(acc, small):
    L = SMALL["n_layers"]
    dec = small_decoder(acc, SMALL, small)
    lens, pos = [20, 33, 9, 64], [0, 5, 0, 0]
    batch, oms = setup_rows(dec, SMALL, small, pos, 900)
    prompts = prompts_of(SMALL, lens, 5)
    picks = batch.prefill_rows(prompts, pos)
    toks = np.zeros(4, np.int32)
    for r in range(4):
        toks[r], _ = oms[r].forward(prompts[r], pos[r], 0)
    # ragged decode steps from positions + lens, each row fed its oracle's pick (bounds of test_ragged_gpu.py)
    at = np.array(pos) + np.array(lens)
    for i in range(3):
        got = batch.step_rows(toks, at)
        logits = batch.logits()
        for r in range(4):
            otok, ologits = oms[r].step(int(toks[r]), int(at[r]))
            parity.check(BF16, logits[r], ologits, rel=5e-3, max_ulp=2 + L, max_frac=0.7, what=f"step {i} row {r} logits")
            assert got[r] == int(np.argmax(mo.from_bf16(logits[r])))
            toks[r] = otok
        at += 1
    assert list(batch.lengths()) == list(at)
    # a second chunk appended to rows 0 and 2 at their lengths; rows 1 and 3 stay out
    more = prompts_of(SMALL, [17, 40], 6)
    second = [more[0], None, more[1], None]
    before = [batch.export_row_kv(r, 0) for r in (1, 3)]
    picks = batch.prefill_rows(second, [int(at[0]), 0, int(at[2]), 0])
    assert picks[1] == picks[3] == -1
    check_rows(SMALL, batch, oms, second, [int(at[0]), 0, int(at[2]), 0], picks, "second chunk", exact_context=False)
    for r, (k, v) in zip((1, 3), before):
        parity.exact(batch.export_row_kv(r, 0)[0], k, f"row {r} K")
    batch.release()
    for om in oms:
        om.close()
    dec.release()


def test_rows_outside_the_call_are_untouched(acc, small):
    dec = small_decoder(acc, SMALL, small)
    pos = [30, 0, 12, 0, 50, 0]
    batch, oms = setup_rows(dec, SMALL, small, pos, 1300)
    prompts = prompts_of(SMALL, [10, 70, 10, 3, 10, 2], 7)
    call = [None, prompts[1], None, prompts[3], None, prompts[5]]
    before = {r: batch.export_row_kv(r, 0) for r in (0, 2, 4)}
    picks = batch.prefill_rows(call, [0] * 6)
    assert [picks[r] for r in (0, 2, 4)] == [-1, -1, -1]
    assert all(picks[r] >= 0 for r in (1, 3, 5))
    assert list(batch.lengths()) == [30, 70, 12, 3, 50, 2]
    for r, (k, v) in before.items():
        gk, gv = batch.export_row_kv(r, 0)
        parity.exact(gk, k, f"row {r} K")
        parity.exact(gv, v, f"row {r} V")
    batch.release()
    for om in oms:
        om.close()
    dec.release()


def test_the_decoder_is_untouched(acc, small):
    import metalchat_amd as mc

    prompt = prompts_of(SMALL, [24], 8)[0]
    dec, ref = small_decoder(acc, SMALL, small), small_decoder(acc, SMALL, small)
    for d in (dec, ref):
        d.prefill(prompt, 0)
    kv0 = dec.export_kv(0)
    batch = mc.Batch(dec, 4)
    batch.prefill_rows(prompts_of(SMALL, [100, 50, 60, 30], 9))
    for a, b, name in zip(dec.export_kv(0), kv0, "KV"):
        parity.exact(a, b, f"decoder {name}")
    t1, t2 = dec.step(77, len(prompt)), ref.step(77, len(prompt))
    assert t1 == t2
    parity.exact(dec.logits(), ref.logits(), "decoder step after the call")
    batch.release()
    dec.release()
    ref.release()


def test_refusals(acc, small):
    import metalchat_amd as mc

    S = SMALL["max_seq_len"]
    dec = small_decoder(acc, SMALL, small)
    batch = mc.Batch(dec, 4)
    batch.prefill_rows([[1, 2, 3], None, None, None])  # row 0: length 3
    lib = mc.capi()
    ptr = C.POINTER(C.c_int32)

    def call(tokens, lens, positions, words):
        t = np.ascontiguousarray(np.asarray(list(tokens) + [0], np.int32))
        ln = np.ascontiguousarray(lens, np.int32)
        p = np.ascontiguousarray(positions, np.int32)
        out = np.zeros(4, np.int32)
        dec.launch_log(True)
        st = lib.mc_rows_prefill(batch._h, t.ctypes.data_as(ptr), ln.ctypes.data_as(ptr), p.ctypes.data_as(ptr), out.ctypes.data_as(ptr))
        assert st == 1, words
        msg = lib.mc_last_error().decode()
        assert words in msg, (words, msg)
        assert dec.launched() == [], words

    call([], [0, 0, 0, 0], [0, 0, 0, 0], "no row in the call")
    call([1, 2], [2, -1, 0, 0], [0, 0, 0, 0], "row 1: length below 0")
    call([1, 2, 3], [2, 1, 0, 0], [0, 0, 0, 0], "row 1: a one-token chunk is a step")
    call([1, 2], [0, 0, 2, 0], [0, 0, -1, 0], "row 2: position below 0")
    call([1, 2], [2, 0, 0, 0], [4, 0, 0, 0], "row 0: position 4 is past the row's length 3")
    call(list(range(S - 2)), [S - 2, 0, 0, 0], [3, 0, 0, 0], "row 0: position + length")
    call([1, SMALL["vocab"]], [0, 0, 0, 2], [0, 0, 0, 0], "row 3: token id outside the vocabulary")
    call([1, -5], [0, 0, 0, 2], [0, 0, 0, 0], "row 3: token id outside the vocabulary")
    call(list(range(S)) + [1, 2], [S - 100, 100, 2, 0], [0, 0, 0, 0], "add up to 258, more than max_seq_len")
    assert list(batch.lengths()) == [3, 0, 0, 0]
    batch.release()
    dec.release()


def test_longer_rows_in_a_larger_cache(acc):
    """rows longer than the 64-row tiles' pairs of SMALL, in a copy of the config with max_seq_len 1024 (sum 700)"""
    cfg = dict(SMALL, max_seq_len=1024)
    weights = mg.make_model(cfg, seed=12, quant="i4", group=128)
    dec = small_decoder(acc, cfg, weights)
    lens, pos = [300, 129, 271], [0, 0, 200]
    batch, oms = setup_rows(dec, cfg, weights, pos, 1700)
    prompts = prompts_of(cfg, lens, 10)
    picks = batch.prefill_rows(prompts, pos)
    check_rows(cfg, batch, oms, prompts, pos, picks, "long rows")
    batch.release()
    for om in oms:
        om.close()
    dec.release()
