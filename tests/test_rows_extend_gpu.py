"""Chunks that see their row's context (mc_extend_rows, include/metalchat_hip.h Part 2e) on the device: the packed prompt pass whose
chunk row i attends to every cache column at or below its own position.

  * each row against a chain of oracle.Model.step over its chunk behind a random imported context (K / V of the first and last
    layer, last logits, the pick), with the bounds test_rows_prefill_gpu.check_rows applies to a prompt pass; lengths across
    16- and 64-row boundaries, contexts that end inside a 64-slot range, the last cache slot, several key ranges per tile;
  * the launch log holds the new attention and none of the reference-mask attention; one multiplication per weight matrix;
  * where a prompt is placed does not change its bits;
  * at position 0 the call means what mc_rows_prefill means; a prompt fed in chunks equals the prompt fed at once;
  * steps and a second chunk continue from the call, a rewind gives the bits of a fresh row; rows outside the call and the decoder
    are untouched; the refusals, with nothing launched.
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
from test_rows_prefill_gpu import clear_gap, gemm_launches, prompts_of, setup_rows

pytestmark = pytest.mark.gpu
BF16 = 0
LENS = [2, 15, 16, 17, 31, 33, 64, 65]
POS = [5, 7, 16, 40, 63, 3, 64, 20]


@pytest.fixture(scope="module")
def small():
    return mg.make_model(SMALL, seed=11, quant="i4", group=128)


@pytest.fixture(scope="module")
def llama1b():
    return mg.make_model(LLAMA32_1B, seed=5)


def chain(om, tokens, p):
    """what len(tokens) successive decode steps of the oracle compute: the last pick and logits (the cache holds the rest)"""
    for i, t in enumerate(tokens):
        otok, ologits = om.step(int(t), p + i)
    return otok, ologits


def check_rows(cfg, batch, oms, prompts, positions, picks, what, reference=chain, exact_context=True, max_ulp=2, rel=None):
    """row r against reference(oms[r], prompts[r], positions[r]) with the bounds of test_rows_prefill_gpu.check_rows; returns how
    many rows were in the call and how many of their picks were compared with the oracle's (its pick being unambiguous)"""
    trel, frac = tol(BF16)
    rel = trel if rel is None else rel
    logits = batch.logits()
    rows = picked = 0
    for r, (tokens, p) in enumerate(zip(prompts, positions)):
        if tokens is None:
            continue
        otok, ologits = reference(oms[r], tokens, p)
        n = len(tokens)
        rows += 1
        st = parity.check(BF16, logits[r], ologits, rel=rel, max_ulp=max_ulp, max_frac=frac, what=f"{what} row {r} logits")
        print(f"{what} row {r} (pos {p}, len {n}): logits {st}")
        assert picks[r] == int(np.argmax(mo.from_bf16(logits[r]))), (what, r)
        if clear_gap(ologits):
            picked += 1
            assert picks[r] == otok, (what, r, picks[r], otok)
        for layer in sorted({0, cfg["n_layers"] - 1}):
            gk, gv = batch.export_row_kv(r, layer)
            ok, ov = oms[r].kv(layer)
            assert gk.shape == ok.shape == (p + n, cfg["n_kv_heads"], cfg["head_dim"]), (what, r)
            if exact_context:
                parity.exact(gk[:p], ok[:p], f"{what} row {r} layer {layer} context K")
                parity.exact(gv[:p], ov[:p], f"{what} row {r} layer {layer} context V")
            parity.check(BF16, gk[p:], ok[p:], rel=rel, max_ulp=max_ulp, max_frac=frac, what=f"{what} row {r} layer {layer} K")
            parity.check(BF16, gv[p:], ov[p:], rel=rel, max_ulp=max_ulp, max_frac=frac, what=f"{what} row {r} layer {layer} V")
    return rows, picked


def attention_names(hd):
    return {f"mc_px_{a}_bfloat_hd{hd}" for a in ("sums", "sums2", "pv", "pv2")}


def check_log(names, hd):
    assert attention_names(hd) & set(names), sorted(set(names))
    assert len([n for n in names if n.startswith("mc_px_sums")]) == len([n for n in names if n.startswith("mc_px_pv")])
    bad = [n for n in names if n.startswith(("mc_pp_attn", "mc_pf_attn", "mc_pf_rope", "mc_gemv_", "mc_argmax"))]
    assert not bad, sorted(set(names))
    assert {"mc_pp_gather_last_bfloat", "mc_b_rmsnorm_bfloat", "mc_b_argmax_rows_bfloat"} <= set(names), sorted(set(names))
    assert {"mc_pp_rope_cache_bfloat", "mc_pp_rope_cache_parts_bfloat"} & set(names), sorted(set(names))


def release(batch, oms, dec):
    batch.release()
    for om in oms:
        om.close()
    dec.release()


@pytest.mark.parametrize("shape", ["small-int4", "llama32-1b-bf16"])
def test_rows_against_the_oracle(acc, small, llama1b, shape):
    cfg, weights = (SMALL, small) if shape == "small-int4" else (LLAMA32_1B, llama1b)
    lens, pos = (LENS, POS) if cfg is SMALL else ([2, 17, 33, 65], [9, 7, 64, 20])
    dec = small_decoder(acc, cfg, weights)
    batch, oms = setup_rows(dec, cfg, weights, pos, 500)
    prompts = prompts_of(cfg, lens, 1)
    dec.launch_log(True)
    picks = batch.extend_rows(prompts, pos)
    names = dec.launched()
    assert list(batch.lengths()) == [p + n for p, n in zip(pos, lens)]
    rows, picked = check_rows(cfg, batch, oms, prompts, pos, picks, shape)
    assert 2 * picked >= rows, (picked, rows)
    check_log(names, cfg["head_dim"])
    release(batch, oms, dec)


LONG_LENS = [5, 40, 16, 130, 2, 33]
LONG_POS = [1000, 700, 63, 513, 1022, 255]


def long_case(acc, keys=None):
    cfg = dict(SMALL, max_seq_len=1024)
    weights = mg.make_model(cfg, seed=12, quant="i4", group=128)
    dec = small_decoder(acc, cfg, weights)
    batch, oms = setup_rows(dec, cfg, weights, LONG_POS, 1700)
    prompts = prompts_of(cfg, LONG_LENS, 10)
    dec.launch_log(True)
    picks = batch.extend_rows(prompts, LONG_POS)
    names = dec.launched()
    rows, picked = check_rows(cfg, batch, oms, prompts, LONG_POS, picks, f"long contexts (keys {keys})")
    assert 2 * picked >= rows, (picked, rows)
    check_log(names, cfg["head_dim"])
    # a tile with several key ranges was launched: only then is there anything to reduce
    assert names.count("mc_px_reduce_bfloat_hd128") == cfg["n_layers"], names
    logits = batch.logits()
    kv = [batch.export_row_kv(r, 0) for r in range(len(LONG_POS))]
    release(batch, oms, dec)
    return picks, logits, kv


def test_long_contexts_and_split_keys(acc):
    """max_seq_len 1024: by the host's rule (a segment of at most 32 rows behind more than 512 keys: two key ranges) rows 0 and 4
    are split and the others are not -- both counts the rule can produce"""
    long_case(acc)


def test_every_range_count(acc, monkeypatch):
    """the same call with ranges of 128 keys for every tile (MC_PX_KEYS, read at the call): one to eight ranges per tile, several
    tiles of a segment split, the same bounds"""
    monkeypatch.setenv("MC_PX_KEYS", "128")
    long_case(acc, 128)


def test_the_launch_log(acc, small):
    import metalchat_amd as mc

    dec = small_decoder(acc, SMALL, small)
    prompts = prompts_of(SMALL, LENS, 2)
    batch, oms = setup_rows(dec, SMALL, small, POS, 600)
    dec.launch_log(True)
    batch.extend_rows(prompts, POS)
    extend = dec.launched()
    other = mc.Batch(dec, 8)
    dec.launch_log(True)
    other.prefill_rows(prompts)
    packed = dec.launched()
    L = SMALL["n_layers"]
    check_log(extend, SMALL["head_dim"])
    assert gemm_launches(extend) == gemm_launches(packed), (extend, packed)
    assert len([n for n in gemm_launches(extend) if not n.startswith("mc_pf_splitk")]) == 4 * L, extend
    for name, per_call in (("mc_pp_gather_last_bfloat", 1), ("mc_b_gemv_i4_bfloat_e0", 1), ("mc_pf_embed_bfloat", 1)):
        assert extend.count(name) == per_call, (name, extend)
    assert len([n for n in extend if n.startswith("mc_pp_rope_cache")]) == L
    assert len([n for n in extend if n.startswith("mc_px_sums")]) == L  # one launch group: the call fits the scratch
    assert not [n for n in extend if n.startswith("mc_px_reduce")], extend  # no tile behind more than 512 keys: none is split
    assert len(extend) < 20 * L + 10, extend  # nothing per row
    other.release()
    release(batch, oms, dec)


def test_a_call_in_several_launch_groups(acc, monkeypatch):
    """a call whose ranges exceed the scratch of one launch group (rows_plan.h rows_ranges: groups of whole tiles, the kernels' `ebase`):
    eight rows of 200 tokens behind 1800 keys with ranges of 128 keys -- 13 tiles of 15 or 16 ranges per row, 1608 ranges, and a
    scratch of 64 MiB / (8 heads * 16 rows * 128 * 4 bytes) = 1024 slots: two groups.  A row's bits depend on its own segment only,
    so every row must come out bit for bit as it does extended alone, in a call of its own that fits one group (201 ranges)"""
    monkeypatch.setenv("MC_PX_KEYS", "128")
    cfg = dict(SMALL, max_seq_len=2048)
    L, pos, n = cfg["n_layers"], 1800, 200
    weights = mg.make_model(cfg, seed=13, quant="i4", group=128)
    dec = small_decoder(acc, cfg, weights)
    import metalchat_amd as mc

    prompts = prompts_of(cfg, [n] * 8, 12)

    def rows_behind_their_contexts():
        b = mc.Batch(dec, 8)
        for r in range(8):
            for layer in range(L):
                k, v = random_cache(cfg, pos, 1900 + 100 * r + layer)
                b.import_kv(r, layer, k, v)
        return b

    together, alone = rows_behind_their_contexts(), rows_behind_their_contexts()
    dec.launch_log(True)
    picks = together.extend_rows(prompts, [pos] * 8)
    names = dec.launched()
    assert names.count("mc_px_sums2_bfloat_hd128") == 2 * L, names  # two launch groups per layer
    assert names.count("mc_px_pv2_bfloat_hd128") == 2 * L and names.count("mc_px_reduce_bfloat_hd128") == 2 * L, names
    logits = together.logits()
    for r in range(8):
        call = [None] * 8
        call[r] = prompts[r]
        dec.launch_log(True)
        own = alone.extend_rows(call, [pos] * 8)
        assert dec.launched().count("mc_px_sums2_bfloat_hd128") == L  # one group
        assert own[r] == picks[r] and picks[r] >= 0, (r, own[r], picks[r])
        parity.exact(logits[r], alone.logits()[r], f"row {r}: logits in two groups against the row alone")
        for a, b, name in zip(together.export_row_kv(r, 0), alone.export_row_kv(r, 0), "KV"):
            assert a.shape[0] == pos + n
            parity.exact(a, b, f"row {r}: layer 0 {name} in two groups against the row alone")
    together.release()
    alone.release()
    dec.release()


def test_placement_does_not_matter(acc, small):
    dec = small_decoder(acc, SMALL, small)
    prompts = prompts_of(SMALL, LENS, 3)
    perm = [5, 2, 7, 0, 3, 6, 1, 4]  # prompt i (and its context) goes to row perm[i]
    a, oa = setup_rows(dec, SMALL, small, POS, 700)
    pa = a.extend_rows(prompts, POS)
    la = a.logits()
    import metalchat_amd as mc

    b = mc.Batch(dec, 8)
    moved, mpos = [None] * 8, [0] * 8
    for i, r in enumerate(perm):
        moved[r], mpos[r] = prompts[i], POS[i]
        for layer in range(SMALL["n_layers"]):
            k, v = random_cache(SMALL, POS[i], 700 + 100 * i + layer)  # (setup_rows' context of row i)
            b.import_kv(r, layer, k, v)
    pb = b.extend_rows(moved, mpos)
    lb = b.logits()
    for i, r in enumerate(perm):
        assert pa[i] == pb[r], (i, r)
        parity.exact(lb[r], la[i], f"prompt {i}: logits")
        (ka, va), (kb, vb) = a.export_row_kv(i, 0), b.export_row_kv(r, 0)
        parity.exact(kb, ka, f"prompt {i}: K")
        parity.exact(vb, va, f"prompt {i}: V")
    b.release()
    release(a, oa, dec)


def test_position_zero_means_a_prompt_pass(acc, small):
    dec = small_decoder(acc, SMALL, small)
    zeros = [0] * 8
    prompts = prompts_of(SMALL, LENS, 4)
    batch, oms = setup_rows(dec, SMALL, small, zeros, 800)
    picks = batch.extend_rows(prompts, zeros)
    rows, picked = check_rows(SMALL, batch, oms, prompts, zeros, picks, "position 0", reference=lambda om, t, p: om.forward(t, p, 0))
    assert 2 * picked >= rows, (picked, rows)
    other, _ = setup_rows(dec, SMALL, small, zeros, 800)
    other.prefill_rows(prompts, zeros)
    rel, frac = tol(BF16)
    la, lb = batch.logits(), other.logits()
    for r in range(8):
        parity.check(BF16, la[r], lb[r], rel=rel, max_ulp=2, max_frac=frac, what=f"row {r} logits against prefill_rows")
        for (ka, va), (kb, vb) in [(batch.export_row_kv(r, 0), other.export_row_kv(r, 0))]:
            parity.check(BF16, ka, kb, rel=rel, max_ulp=2, max_frac=frac, what=f"row {r} K against prefill_rows")
            parity.check(BF16, va, vb, rel=rel, max_ulp=2, max_frac=frac, what=f"row {r} V against prefill_rows")
    other.release()
    release(batch, oms, dec)


def test_a_prompt_in_chunks(acc, small):
    """200 tokens at once, as 64 + 136 and as 17 + 100 + 83, each against ONE oracle forward of the whole prompt.  The chunked forms
    continue from a cache the device wrote: max_ulp 2 + n_layers and rel 5e-3, the project's figures for that
    (test_rows_prefill_gpu.test_decode_and_a_second_chunk_continue)"""
    L = SMALL["n_layers"]
    dec = small_decoder(acc, SMALL, small)
    prompt = prompts_of(SMALL, [200], 11)[0]
    batch, oms = setup_rows(dec, SMALL, small, [0, 0, 0], 0)
    whole = lambda om, t, p: om.forward(prompt, 0, 0)
    picks = batch.prefill_rows([prompt, None, None], [0, 0, 0])  # (two calls: a call takes at most max_seq_len rows)
    check_rows(SMALL, batch, oms[:1], [prompt], [0], picks, "at once", reference=whole)
    batch.prefill_rows([None, prompt[:64], prompt[:17]], [0, 0, 0])
    picks = batch.extend_rows([None, None, prompt[17:117]], [0, 0, 17])
    assert picks[0] == picks[1] == -1 and list(batch.lengths()) == [200, 64, 117]
    picks = batch.extend_rows([None, prompt[64:], prompt[117:]], [0, 64, 117])
    assert list(batch.lengths()) == [200, 200, 200]
    for r in (1, 2):
        # (the row's whole cache against the oracle's: `prompts` = the whole prompt at position 0)
        sel = [None] * 3
        sel[r] = prompt
        check_rows(SMALL, batch, oms, sel, [0, 0, 0], picks, f"in chunks, row {r}", reference=whole, max_ulp=2 + L, rel=5e-3)
    release(batch, oms, dec)


def test_steps_and_chunks_continue_and_a_rewind(acc, small):
    L = SMALL["n_layers"]
    dec = small_decoder(acc, SMALL, small)
    lens, pos = [20, 33, 9, 64], [30, 5, 64, 17]
    batch, oms = setup_rows(dec, SMALL, small, pos, 900)
    prompts = prompts_of(SMALL, lens, 5)
    picks = batch.extend_rows(prompts, pos)
    toks = np.zeros(4, np.int32)
    for r in range(4):
        toks[r], _ = chain(oms[r], prompts[r], pos[r])
    at = np.array(pos) + np.array(lens)
    assert list(batch.lengths()) == list(at)
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
    # generate_rows from the picks of a chunk: the first token it produces is the step's pick
    out, produced = batch.generate_rows(toks, at, 2)
    assert list(produced) == [2, 2, 2, 2] and list(batch.lengths()) == list(at + 2)
    # a second chunk behind the first on rows 0 and 2 (their caches: context, chunk, three steps); rows 1 and 3 stay out
    more = prompts_of(SMALL, [17, 40], 6)
    second, spos = [more[0], None, more[1], None], [int(at[0]), 0, int(at[2]), 0]
    before = [batch.export_row_kv(r, 0) for r in (1, 3)]
    picks = batch.extend_rows(second, spos)
    assert picks[1] == picks[3] == -1
    check_rows(SMALL, batch, oms, second, spos, picks, "second chunk", exact_context=False, max_ulp=2 + L, rel=5e-3)
    for r, (k, v) in zip((1, 3), before):
        parity.exact(batch.export_row_kv(r, 0)[0], k, f"row {r} K")
        parity.exact(batch.export_row_kv(r, 0)[1], v, f"row {r} V")
    # a rewind: row 0 back to position 12 of its context, against a fresh row holding the same first 12 cache rows
    import metalchat_amd as mc

    again = prompts_of(SMALL, [37], 7)[0]
    k12 = [tuple(a[:12] for a in batch.export_row_kv(0, layer)) for layer in range(L)]
    p_rew = batch.extend_rows([again, None, None, None], [12, 0, 0, 0])
    assert batch.lengths()[0] == 12 + 37
    fresh = mc.Batch(dec, 4)
    for layer in range(L):
        fresh.import_kv(0, layer, *k12[layer])
    p_new = fresh.extend_rows([again, None, None, None], [12, 0, 0, 0])
    assert p_rew[0] == p_new[0]
    parity.exact(batch.logits()[0], fresh.logits()[0], "rewound row: logits")
    for layer in range(L):
        for a, b, name in zip(batch.export_row_kv(0, layer), fresh.export_row_kv(0, layer), "KV"):
            parity.exact(a, b, f"rewound row: layer {layer} {name}")
    fresh.release()
    release(batch, oms, dec)


def test_rows_outside_the_call_are_untouched(acc, small):
    dec = small_decoder(acc, SMALL, small)
    L = SMALL["n_layers"]
    pos = [30, 8, 12, 0, 50, 21]
    batch, oms = setup_rows(dec, SMALL, small, pos, 1300)
    prompts = prompts_of(SMALL, [10, 70, 10, 3, 10, 2], 7)
    call = [None, prompts[1], None, prompts[3], None, prompts[5]]
    before = {r: [batch.export_row_kv(r, layer) for layer in range(L)] for r in (0, 2, 4)}
    picks = batch.extend_rows(call, pos)
    assert [picks[r] for r in (0, 2, 4)] == [-1, -1, -1]
    assert all(picks[r] >= 0 for r in (1, 3, 5))
    assert list(batch.lengths()) == [30, 78, 12, 3, 50, 23]
    for r, layers in before.items():
        for layer, (k, v) in enumerate(layers):
            gk, gv = batch.export_row_kv(r, layer)
            parity.exact(gk, k, f"row {r} layer {layer} K")
            parity.exact(gv, v, f"row {r} layer {layer} V")
    release(batch, oms, dec)


def test_the_decoder_is_untouched(acc, small):
    prompt = prompts_of(SMALL, [24], 8)[0]
    dec, ref = small_decoder(acc, SMALL, small), small_decoder(acc, SMALL, small)
    for d in (dec, ref):
        d.prefill(prompt, 0)
    kv0 = dec.export_kv(0)
    pos = [20, 9, 0, 64]
    batch, oms = setup_rows(dec, SMALL, small, pos, 1400)
    batch.extend_rows(prompts_of(SMALL, [100, 50, 60, 30], 9), pos)
    for a, b, name in zip(dec.export_kv(0), kv0, "KV"):
        parity.exact(a, b, f"decoder {name}")
    t1, t2 = dec.step(77, len(prompt)), ref.step(77, len(prompt))
    assert t1 == t2
    parity.exact(dec.logits(), ref.logits(), "decoder step after the call")
    ref.release()
    release(batch, oms, dec)


def test_refusals(acc, small):
    import metalchat_amd as mc

    S = SMALL["max_seq_len"]
    dec = small_decoder(acc, SMALL, small)
    batch = mc.Batch(dec, 4)
    batch.extend_rows([[1, 2, 3], None, None, None], [0, 0, 0, 0])  # row 0: length 3
    lib = mc.capi()
    ptr = C.POINTER(C.c_int32)

    def call(tokens, lens, positions, words):
        t = np.ascontiguousarray(np.asarray(list(tokens) + [0], np.int32))
        ln = np.ascontiguousarray(lens, np.int32)
        p = np.ascontiguousarray(positions, np.int32)
        out = np.zeros(4, np.int32)
        dec.launch_log(True)
        st = lib.mc_extend_rows(batch._h, t.ctypes.data_as(ptr), ln.ctypes.data_as(ptr), p.ctypes.data_as(ptr), out.ctypes.data_as(ptr))
        assert st == 1, words
        msg = lib.mc_last_error().decode()
        assert msg.startswith("mc_extend_rows: "), msg
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
