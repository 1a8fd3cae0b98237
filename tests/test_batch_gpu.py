"""Batched decode (mc_batch_*, include/metalchat_hip.h Part 2b) on the device: B sequences in lockstep over one decoder's weights.

  * parity per row against its own oracle.Model (nn::attention with input[bs, 1, dim] is B independent rows,
    include/metalchat/nn/attention.h:163-206) at Llama-3-8B widths (int4 g128, S = 2048) and Llama-3.2-1B widths (bfloat
    weights, head_dim 64, two layers, positions across a 64-slot boundary), with the bounds of test_context_gpu.py;
  * a row's bits do not depend on B, on the order of the rows or on what sits beside them;
  * fork of a prompt pass, chained == stepwise, the default sampler per row, the decoder untouched, and the refusals.
"""
import numpy as np
import pytest

import modelgen as mg
import parity
from oracle import mc_oracle as mo
from test_context_gpu import random_cache
from test_full_size_gpu import FULL_WIDTH, SEED, synth_model

pytestmark = pytest.mark.gpu
BF16 = 0

# an admitted shape small enough for quick oracle runs: every in_features % 1024 == 0, every out_features % 16 == 0
SMALL = dict(dtype=BF16, family=0, dim=1024, n_heads=8, n_kv_heads=2, head_dim=128, ffn_dim=2048, n_layers=1, vocab=2048,
             max_seq_len=256, rope_theta=500000.0, norm_eps=1e-5, attn_scale=128 ** -0.5)
LLAMA32_1B = dict(dtype=BF16, family=0, dim=2048, n_heads=32, n_kv_heads=8, head_dim=64, ffn_dim=8192, n_layers=2, vocab=2048,
                  max_seq_len=256, rope_theta=500000.0, norm_eps=1e-5, attn_scale=64 ** -0.5)


def small_decoder(acc, cfg, weights, **over):
    import metalchat_amd as mc

    kw = dict(weight_format=mc.WFMT_I4, group_size=128) if weights["layers"][0]["wq"]["kind"] == 1 else {}
    kw.update(over)
    dec = mc.Decoder(acc, **mg.decoder_kwargs(cfg, **kw))
    dec.load_model(weights)
    return dec


@pytest.fixture(scope="module")
def small():
    return mg.make_model(SMALL, seed=11, quant="i4", group=128)


def run_lockstep(acc, cfg, weights, dec, B, n_inject, n_steps, what):
    """Row r: its own random cache of n_inject rows and its own oracle; n_steps lockstep steps, each row fed its oracle's pick."""
    import metalchat_amd as mc

    L = cfg["n_layers"]
    batch = mc.Batch(dec, B)
    dec.launch_log(True)
    oms = [mo.Model(cfg, weights) for _ in range(B)]
    for r in range(B):
        for layer in range(L):
            k, v = random_cache(cfg, n_inject, 1000 * r + layer)
            oms[r].set_kv(layer, k, v)
            batch.import_kv(r, layer, k, v)
    for r in range(B):  # import -> export is the identity
        gk, gv = batch.export_kv(r, 0)
        ok, ov = oms[r].kv(0)
        parity.exact(gk, ok, f"{what} row {r} imported K")
        parity.exact(gv, ov, f"{what} row {r} imported V")
    toks = np.array([7 + 13 * r for r in range(B)], np.int32)
    for i in range(n_steps):
        pos = n_inject + i
        picks = batch.step(toks, pos)
        logits = batch.logits()
        nxt = np.zeros(B, np.int32)
        for r in range(B):
            otok, ologits = oms[r].step(int(toks[r]), pos)
            parity.check(BF16, logits[r], ologits, rel=5e-3, max_ulp=2 + L, max_frac=0.7, what=f"{what} row {r} pos {pos} logits")
            assert picks[r] == int(np.argmax(mo.from_bf16(logits[r]))), (what, r, pos)
            nxt[r] = otok
        toks = nxt
    for r in range(B):
        for layer in range(L):
            gk, gv = batch.export_kv(r, layer)
            ok, ov = oms[r].kv(layer)
            assert gk.shape == ok.shape == (n_inject + n_steps, cfg["n_kv_heads"], cfg["head_dim"])
            parity.exact(gk[:n_inject], ok[:n_inject], f"{what} row {r} layer {layer} injected K rows")
            parity.exact(gv[:n_inject], ov[:n_inject], f"{what} row {r} layer {layer} injected V rows")
            parity.check(BF16, gk[n_inject:], ok[n_inject:], rel=3.9e-3, max_ulp=2, max_frac=0.7, what=f"{what} row {r} computed K")
            parity.check(BF16, gv[n_inject:], ov[n_inject:], rel=3.9e-3, max_ulp=2, max_frac=0.7, what=f"{what} row {r} computed V")
    names = set(dec.launched())
    batch.release()
    for om in oms:
        om.close()
    return names


def test_llama3_8b_int4_rows_against_the_oracle(acc):
    import metalchat_amd as mc

    cfg = dict(dtype=BF16, n_layers=1, vocab=2048, max_seq_len=2048, norm_eps=1e-5, **FULL_WIDTH["llama3-8b"])
    weights = synth_model(cfg, SEED)
    dec = mc.Decoder(acc, **mg.decoder_kwargs(cfg, weight_format=mc.WFMT_I4, group_size=128))
    dec.init_synthetic(SEED)
    names = run_lockstep(acc, cfg, weights, dec, 4, 2040, 8, "8B int4 B=4")
    assert {"mc_b_gemv_i4_bfloat_e0", "mc_b_gemv_i4_bfloat_e1", "mc_b_gemv_i4_bfloat_e2", "mc_b_attn_scores_bfloat",
            "mc_b_attn_pv_bfloat", "mc_b_rope_kv_bfloat", "mc_b_argmax_bfloat"} <= names, sorted(names)
    assert not [n for n in names if n.startswith("mc_gemv_")], sorted(names)
    assert dec.derived_weight_bytes() == 0
    dec.release()


def test_llama32_1b_bfloat_rows_across_a_64_slot_boundary(acc):
    weights = mg.make_model(LLAMA32_1B, seed=5)
    dec = small_decoder(acc, LLAMA32_1B, weights)
    names = run_lockstep(acc, LLAMA32_1B, weights, dec, 3, 60, 8, "1B bf16 B=3")
    assert {"mc_b_gemv_w_bfloat_e0", "mc_b_gemv_w_bfloat_e1", "mc_b_gemv_w_bfloat_e2"} <= names, sorted(names)
    assert not [n for n in names if n.startswith("mc_gemv_")], sorted(names)
    dec.release()


@pytest.mark.parametrize("variant", ["int8-embedding", "int4-group-256"])
def test_small_rows_against_the_oracle_at_other_admitted_formats(acc, variant):
    """Admitted configurations no other batch test loads: an int8 embedding table (one f32 scale per row) and int4 weights in
    groups of 256, each row against its own oracle."""
    group = 256 if variant == "int4-group-256" else 128
    weights = mg.make_model(SMALL, seed=13, quant="i4", group=group, emb_quant=variant == "int8-embedding")
    dec = small_decoder(acc, SMALL, weights, group_size=group)
    names = run_lockstep(acc, SMALL, weights, dec, 3, 60, 6, f"SMALL {variant} B=3")
    assert {"mc_b_embed_bfloat", "mc_b_gemv_i4_bfloat_e0", "mc_b_gemv_i4_bfloat_e1", "mc_b_gemv_i4_bfloat_e2", "mc_b_rope_kv_bfloat",
            "mc_b_attn_scores_bfloat", "mc_b_attn_pv_bfloat", "mc_b_argmax_bfloat"} <= names, sorted(names)
    assert not [n for n in names if n.startswith("mc_gemv_")], sorted(names)
    dec.release()


def run_contents(acc, dec, contents, n_steps=3, pos0=40):
    """contents: list of (token, [(k, v) per layer]) -- one batch of len(contents) rows; returns per row (logits[n_steps], picks, k, v)"""
    import metalchat_amd as mc

    B = len(contents)
    batch = mc.Batch(dec, B)
    for r, (_, kv) in enumerate(contents):
        for layer, (k, v) in enumerate(kv):
            batch.import_kv(r, layer, k, v)
    toks = np.array([c[0] for c in contents], np.int32)
    logits, picks = [], []
    for i in range(n_steps):
        toks = batch.step(toks, pos0 + i)
        logits.append(batch.logits())
        picks.append(toks.copy())
    out = []
    for r in range(B):
        k, v = batch.export_kv(r, 0)
        out.append((np.stack([lg[r] for lg in logits]), np.array([p[r] for p in picks]), k, v))
    batch.release()
    return out


def same(a, b, what):
    for x, y, name in zip(a, b, ("logits", "picks", "K", "V")):
        assert np.array_equal(x, y), f"{what}: {name} differ"


def test_rows_are_independent_bit_for_bit(acc, small):
    dec = small_decoder(acc, SMALL, small)
    contents = [(3 + 101 * r, [random_cache(SMALL, 40, 500 + r)]) for r in range(8)]
    full = run_contents(acc, dec, contents)
    for B in (1, 2, 4):
        part = run_contents(acc, dec, contents[:B])
        for r in range(B):
            same(part[r], full[r], f"row {r} at B={B} vs B=8")
    perm = [5, 2, 7, 0, 3, 6, 1, 4]
    permuted = run_contents(acc, dec, [contents[p] for p in perm])
    for r, p in enumerate(perm):
        same(permuted[r], full[p], f"permuted row {r} (content {p})")
    clones = run_contents(acc, dec, [contents[6]] * 8)
    for r in range(8):
        same(clones[r], full[6], f"identical row {r}")
    dec.release()


def test_fork_of_a_prompt_pass(acc, small):
    import metalchat_amd as mc

    prompt = np.random.default_rng(3).integers(0, SMALL["vocab"], 100).astype(np.int32)
    dec = small_decoder(acc, SMALL, small)
    dec.prefill(prompt, 0)
    dk, dv = dec.export_kv(0)
    assert dk.shape[0] == 100
    batch = mc.Batch(dec, 4)
    for r in range(4):
        batch.fork(r, 100)
    for r in range(4):
        k, v = batch.export_kv(r, 0)
        parity.exact(k, dk, f"forked row {r} K")
        parity.exact(v, dv, f"forked row {r} V")
    toks = np.array([11, 222, 1033, 2047], np.int32)
    batch.step(toks, 100)
    logits = batch.logits()
    for r in range(4):
        om = mo.Model(SMALL, small)
        om.forward(prompt, 0)
        _, ologits = om.step(int(toks[r]), 100)
        parity.check(BF16, logits[r], ologits, rel=5e-3, max_ulp=3, max_frac=0.7, what=f"forked row {r} logits")
        om.close()
    batch.release()
    dec.release()


@pytest.mark.parametrize("sampler", ["greedy", "default"])
def test_chained_equals_stepwise(acc, small, sampler):
    import metalchat_amd as mc

    B, n, pos0 = 4, 16, 30
    dec = small_decoder(acc, SMALL, small)
    pairs = [(1000 + 17 * i, 77 + i) for i in range(5)]
    if sampler == "default":
        dec.set_sampler(mc.SAMPLER_DEFAULT, top_k=40, temperature=0.9, top_p=0.95)
    first = np.array([5, 900, 1500, 31], np.int32)
    caches = [random_cache(SMALL, pos0, 700 + r) for r in range(B)]

    def fresh():
        b = mc.Batch(dec, B)
        for r in range(B):
            b.import_kv(r, 0, *caches[r])
        return b

    chained = fresh()
    chained.set_seeds(pairs)
    got = chained.generate(first, pos0, n)
    assert got.shape == (n, B)
    stepwise = fresh()
    toks = first
    for i in range(n):
        # token i of a chained call uses pair (i * B + r) % n_pairs; a step uses pair r % n_pairs: rotate the list
        stepwise.set_seeds([pairs[(i * B + r) % len(pairs)] for r in range(B)])
        toks = stepwise.step(toks, pos0 + i)
        assert np.array_equal(toks, got[i]), (sampler, i, toks, got[i])
        if sampler == "default" and i < 4:
            # the sampler per row is the reference's make_default_sampler on that row's logits with its seed pair
            logits = stepwise.logits()
            for r in range(B):
                s0, s1 = pairs[(i * B + r) % len(pairs)]
                want = mo.sample_default(BF16, logits[r], top_k=40, temperature=0.9, top_p=0.95, init_state=s0, init_seq=s1)
                assert toks[r] == want, (i, r, toks[r], want)
    for r in range(B):
        for a, b_, name in zip(chained.export_kv(r, 0), stepwise.export_kv(r, 0), "KV"):
            parity.exact(a, b_, f"{sampler} row {r} {name} after {n} tokens")
    chained.release()
    stepwise.release()
    dec.release()


def test_the_decoder_is_untouched(acc, small):
    import metalchat_amd as mc

    ref = small_decoder(acc, SMALL, small)
    ref.step(9, 0)
    want = ref.logits()
    dec = small_decoder(acc, SMALL, small)
    before = dec.derived_weight_bytes()
    batch = mc.Batch(dec, 8)
    batch.generate(np.arange(8, dtype=np.int32) * 5, 0, 6)
    batch.step(np.arange(8, dtype=np.int32), 6)
    dec.step(9, 0)
    assert np.array_equal(dec.logits(), want)
    assert dec.derived_weight_bytes() == before == 0
    batch.release()
    ref.release()
    dec.release()


def refused(fn, words):
    import metalchat_amd as mc

    with pytest.raises(mc.McError) as e:
        fn()
    assert e.value.status == 1, str(e.value)
    assert words in str(e.value), str(e.value)


def test_refusals(acc, small):
    import metalchat_amd as mc

    tiny = mg.tiny_cfg(BF16, dim=1024, n_heads=8, n_kv_heads=2, head_dim=128, ffn_dim=2048, vocab=512, max_seq_len=64, n_layers=2)
    cases = [
        ("int8", tiny, mg.make_model(tiny, seed=1, quant="i8", group=128), dict(weight_format=mc.WFMT_I8, group_size=128),
         "int4"),
        ("gemma3", dict(tiny, family=1, rope_sliding_theta=10000.0, sliding_stride=2),
         mg.make_model(dict(tiny, family=1, rope_sliding_theta=10000.0, sliding_stride=2), seed=2), {}, "llama3"),
        ("pipeline stage", tiny, mg.make_model(tiny, seed=3), dict(layer_begin=1, layer_end=2), "pipeline stage"),
        ("lora", SMALL, mg.make_model(SMALL, seed=4, quant="i4", group=128, lora_rank=8), dict(weight_format=mc.WFMT_I4,
                                                                                               group_size=128), "LoRA"),
    ]
    for name, cfg, weights, over, words in cases:
        dec = mc.Decoder(acc, **mg.decoder_kwargs(cfg, **over))
        dec.load_model(weights)
        dec.launch_log(True)
        refused(lambda: mc.Batch(dec, 2), words)
        assert dec.launched() == [], name
        dec.release()
    # positions past the cache, and a fork of a decoder whose cache has rolled
    dec = small_decoder(acc, SMALL, small)
    batch = mc.Batch(dec, 2)
    dec.launch_log(True)
    S = SMALL["max_seq_len"]
    refused(lambda: batch.generate([1, 2], S - 4, 5), "max_seq_len")
    refused(lambda: batch.step([1, 2], S), "max_seq_len")
    assert dec.launched() == []
    dec.launch_log(False)
    dec.prefill(np.arange(S, dtype=np.int32) % 100, 0)
    dec.step(3, S)  # the sink ring turns
    dec.launch_log(True)
    refused(lambda: batch.fork(0, 10), "rolled")
    assert dec.launched() == []
    batch.release()
    dec.release()
