"""Parity at the context lengths and widths bench.py actually runs (BASELINE.json configs[1], [2], [0], [4]).

The CPU oracle cannot decode thousands of tokens in a test, so the cache is INJECTED on both sides
(mc_decoder_import_kv / mco_model_set_kv: n logical rows as if positions 0 .. n-1 had been decoded) and
the decode steps around and past max_seq_len are compared against the oracle on one full-width block
with the benchmark's own synthetic weights (tests/synthgen.py regenerates what mc_decoder_init_synthetic
put in HBM):
  * Llama-3-8B int4 g128, S = 2048, bf16 and f32: kv_len 2041 .. 2048 and eight steps past the end
    (multi-round score loops, whole-context P.V workgroups, the sink ring with pre_len 11);
  * Llama-3-8B int8, S = 8192 with the automatic P.V context ranges: kv_len 8186 .. 8192 and on past the end;
  * TinyLlama-1.1B shapes (head_dim 64, 8 query heads per kv head, ffn 5632, bf16 weights, vocab 32000);
  * Llama-3-70B widths (dim 8192, 64 heads, ffn 28672): K = 8192 / 28672 GEMVs;
  * rows already in the cache do not change by a single bit across a roll (nn/cache.h:187-204).
"""
import numpy as np
import pytest

import modelgen as mg
import parity
from oracle import mc_oracle as mo
from test_full_size_gpu import FULL_WIDTH, SEED, synth_model

pytestmark = pytest.mark.gpu
BF16, F32 = 0, 1


def random_cache(cfg, n, seed):
    """[n, n_kv, hd] keys / values of T with the magnitudes decoded rows have (scores stay far from overflow:
    the reference's softmax has no max shift, kernel/softmax.metal:24-88)."""
    rng = np.random.default_rng(seed)
    shape = (n, cfg["n_kv_heads"], cfg["head_dim"])
    k = mo.encode(cfg["dtype"], rng.normal(0, 0.4, shape).astype(np.float32))
    v = mo.encode(cfg["dtype"], rng.normal(0, 0.5, shape).astype(np.float32))
    return k, v


def run_injected(acc, cfg, weights, n_inject, n_steps, dec_over, rel_logits, max_ulp, max_frac, rel_f32=2e-4, what="", taps=True,
                 launched=None):
    """`launched` (a set) collects the host names of the kernels the decoder launched for these steps, so that a test can
    require the kernels it is about (a silent fallback to another kernel family must not pass);
    taps = False: the production launch sequence (gemma3: post-norms folded into the next GEMV's prologue) -- logits,
    tokens and caches only."""
    import metalchat_amd as mc

    dt = cfg["dtype"]
    om = mo.Model(cfg, weights)
    dec = mc.Decoder(acc, **mg.decoder_kwargs(cfg, **dec_over))
    dec.init_synthetic(SEED)
    dec.set_taps(taps)
    dec.launch_log(True)
    for layer in range(cfg["n_layers"]):
        k, v = random_cache(cfg, n_inject, 100 + layer)
        om.set_kv(layer, k, v)
        dec.import_kv(layer, k, v)
    gk, gv = dec.export_kv(0)
    ok, ov = om.kv(0)
    parity.exact(gk, ok, f"{what} imported K")  # import -> export is the identity (index work)
    parity.exact(gv, ov, f"{what} imported V")
    prev = (gk.copy(), gv.copy())
    tok, agree = 7, 0
    for i in range(n_steps):
        pos = n_inject + i
        otok, ologits = om.step(tok, pos)
        gtok = dec.step(tok, pos)
        if dt == BF16:
            for layer in range(cfg["n_layers"] if taps else 0):
                parity.check(dt, dec.hidden(layer), om.hidden(layer), rel=3.9e-3 * (1 + layer), max_ulp=max_ulp + layer, max_frac=max_frac,
                             what=f"{what} pos {pos} hidden[{layer}]")
            # (a logit is a 4096-term dot product of a hidden row that already carries last-bit differences from a
            # 2048-term softmax / P.V sum in another order: up to 3 scaled bf16 steps on single logits, as in the
            # long-context test of test_full_size_gpu.py; the f32 twin below holds 2e-4)
            parity.check(dt, dec.logits(), ologits, rel=rel_logits, max_ulp=max_ulp + cfg["n_layers"], max_frac=max_frac,
                         what=f"{what} pos {pos} logits")
        else:
            for layer in range(cfg["n_layers"]):
                parity.check(dt, dec.hidden(layer), om.hidden(layer), rel=rel_f32, what=f"{what} pos {pos} hidden[{layer}]")
            parity.check(dt, dec.logits(), ologits, rel=rel_f32, what=f"{what} pos {pos} logits")
        agree += int(gtok == otok)
        gk, gv = dec.export_kv(0)
        ok, ov = om.kv(0)
        assert gk.shape == ok.shape, (what, pos, gk.shape, ok.shape)
        S, pre = cfg["max_seq_len"], int(cfg["max_seq_len"]).bit_length() - 1
        # (1) index work is bit-exact: rows already in the cache do not move (before the cache is full) or move exactly
        # as sink_cache::copy moves them (prefix kept, post region rotated left by one, nn/cache.h:187-204)
        for new, old, name in ((gk, prev[0], "K"), (gv, prev[1], "V")):
            if pos < S:
                parity.exact(new[:-1], old, f"{what} pos {pos} {name}: rows already in the cache")
            else:
                parity.exact(new[:pre], old[:pre], f"{what} pos {pos} {name}: sink prefix")
                parity.exact(new[pre:S - 1], old[pre + 1:S], f"{what} pos {pos} {name}: rotated rows")
        prev = (gk.copy(), gv.copy())
        # (2) the injected rows still in the window are the oracle's rows bit for bit; rows either side computed
        # (rope of a GEMV output) carry the T tolerance
        rolled = max(0, pos + 1 - S)
        if rolled == 0:
            parity.exact(gk[:n_inject], ok[:n_inject], f"{what} pos {pos} injected K rows")
            parity.exact(gv[:n_inject], ov[:n_inject], f"{what} pos {pos} injected V rows")
            ck, cok, cv, cov = gk[n_inject:], ok[n_inject:], gv[n_inject:], ov[n_inject:]
        else:
            parity.exact(gk[:pre], ok[:pre], f"{what} pos {pos} injected K prefix")
            parity.exact(gv[:pre], ov[:pre], f"{what} pos {pos} injected V prefix")
            ncomp = pos + 1 - n_inject  # rows computed by the steps of this test: the tail of the window
            ck, cok, cv, cov = gk[S - ncomp:], ok[S - ncomp:], gv[S - ncomp:], ov[S - ncomp:]
            parity.exact(gk[pre:S - ncomp], ok[pre:S - ncomp], f"{what} pos {pos} injected K rows after {rolled} rolls")
            parity.exact(gv[pre:S - ncomp], ov[pre:S - ncomp], f"{what} pos {pos} injected V rows after {rolled} rolls")
        if dt == BF16:
            parity.check(dt, ck, cok, rel=3.9e-3, max_ulp=max_ulp, max_frac=max_frac, what=f"{what} pos {pos} computed K rows")
            parity.check(dt, cv, cov, rel=3.9e-3, max_ulp=max_ulp, max_frac=max_frac, what=f"{what} pos {pos} computed V rows")
        else:
            parity.check(dt, ck, cok, rel=rel_f32, what=f"{what} pos {pos} computed K rows")
            parity.check(dt, cv, cov, rel=rel_f32, what=f"{what} pos {pos} computed V rows")
        tok = otok
    if launched is not None:
        launched.update(dec.launched())
    dec.release()
    om.close()
    return agree


@pytest.mark.parametrize("dtype", [BF16, F32])
def test_llama3_8b_int4_at_the_benchmark_context(acc, dtype):
    # BASELINE configs[1]: S = 2048.  Steps at positions 2040 .. 2055: kv_len 2041 .. 2048, then eight rolls.
    import metalchat_amd as mc

    cfg = dict(dtype=dtype, n_layers=1, vocab=2048, max_seq_len=2048, norm_eps=1e-5, **FULL_WIDTH["llama3-8b"])
    weights = synth_model(cfg, SEED)
    names = set()
    agree = run_injected(acc, cfg, weights, 2040, 16, dict(weight_format=mc.WFMT_I4, group_size=128),
                         rel_logits=5e-3, max_ulp=2, max_frac=0.7, what=f"8B int4 S=2048 dt{dtype}", launched=names)
    assert agree >= 14
    if dtype == BF16:  # the kernels bench.py's headline runs (and its roofline names): not a fallback family
        # (round 4: wq|wk|wv, attention and Wo are ONE launch, mc_attn_qkv_wo_*; the layer is three launches)
        assert {"mc_attn_qkv_wo_i4_bfloat_hd128_k2_q2", "mc_gemv_i4_bfloat_lin2_p1_e2",
                "mc_gemv_i4_bfloat_lin7_p0_e1", "mc_gemv_i4_bfloat_lin2_p1_e5", "mc_argmax_keys"} <= names, sorted(names)
        assert not [n for n in names if n.startswith("mc_gemv") and "_lin" not in n], sorted(names)
        assert "mc_attn_fused_bfloat" not in names and "mc_attn_pv_bfloat" not in names
    else:
        assert "mc_gemv_i4_float_p1_e2" in names, sorted(names)


def test_llama3_8b_int8_at_8192_with_automatic_context_ranges(acc, monkeypatch):
    # BASELINE configs[2]: S = 8192, P.V split over max_seq_len / 2048 context ranges + the reduce launch, no override.
    import metalchat_amd as mc

    monkeypatch.delenv("MC_PV_RANGES", raising=False)
    cfg = dict(dtype=BF16, n_layers=1, vocab=2048, max_seq_len=8192, norm_eps=1e-5, **FULL_WIDTH["llama3-8b"])
    weights = synth_model(cfg, SEED, bits=8)
    # (round 4: the attention in ONE launch of 128-slot ranges -- mc_attn_fused_t2_bfloat, 512 workgroups -- where the 64-slot
    #  ranges would be 1024; MC_ATTN_T2=0: scores + P.V over context ranges folded into Wo's prologue, as before)
    # (round 5: attention_norm + wq|wk|wv + rope + cache write + attention over 256-slot ranges + wo + residual in ONE launch, one
    #  512-thread workgroup per CU -- mc_attn_qkv_wo_i8_bfloat_hd128_k4_q4_t4; MC_ATTN_I8=0: the five launches of round 4)
    names = set()
    agree = run_injected(acc, cfg, weights, 8185, 15, dict(weight_format=mc.WFMT_I8, group_size=128),
                         rel_logits=5e-3, max_ulp=2, max_frac=0.7, what="8B int8 S=8192 (three launches)", launched=names)
    assert agree >= 13
    assert {"mc_attn_qkv_wo_i8_bfloat_hd128_k4_q4_t4", "mc_gemv_i8_bfloat_ling4_p1_e2", "mc_gemv_i8_bfloat_ling14_p0_e1", "mc_gemv_i8_bfloat_ling4_p1_e5"} <= names, sorted(names)
    assert not {"mc_gemv_i8_bfloat_ling4_p1_e4", "mc_attn_fused_t2_bfloat", "mc_gemv_i8_bfloat_ling4_p0_e1"} & names, sorted(names)
    monkeypatch.setenv("MC_ATTN_I8", "0")
    for t2, attn in (("1", {"mc_attn_fused_t2_bfloat", "mc_gemv_i8_bfloat_ling4_p0_e1"}),
                     ("0", {"mc_attn_scores_bfloat", "mc_attn_pv_bfloat", "mc_gemv_i8_bfloat_ling4_p3_e1"})):
        monkeypatch.setenv("MC_ATTN_T2", t2)
        names = set()
        agree = run_injected(acc, cfg, weights, 8185, 15, dict(weight_format=mc.WFMT_I8, group_size=128),
                             rel_logits=5e-3, max_ulp=2, max_frac=0.7, what=f"8B int8 S=8192 (MC_ATTN_T2={t2})", launched=names)
        assert agree >= 13
        assert ({"mc_gemv_i8_bfloat_ling4_p1_e4", "mc_gemv_i8_bfloat_ling4_p1_e2", "mc_gemv_i8_bfloat_ling14_p0_e1", "mc_gemv_i8_bfloat_ling4_p1_e5"} | attn) <= names, sorted(names)


@pytest.mark.parametrize("S", [4096, pytest.param(8192, marks=pytest.mark.slow)])   # (no BASELINE config names these contexts: one representative under -m gpu)
def test_llama3_8b_int4_at_long_contexts_takes_the_three_launch_layer(acc, monkeypatch, S):
    # round 5: the int4 block with 128- / 256-slot ranges (mc_attn_qkv_wo_i4_bfloat_hd128_k2_q2_t{2,4}: one 512-thread workgroup per CU at S = 4096 /
    # 8192, where the 64-slot ranges are more workgroups than can wait for one another) against the oracle, near the end of the cache and past it
    # (the ring turns); MC_ATTN_I4_WIDE=0: the launches of round 4 (the wq|wk|wv GEMV, mc_attn_fused_t2_bfloat or scores + P.V, the Wo GEMV)
    import metalchat_amd as mc

    cfg = dict(dtype=BF16, n_layers=1, vocab=2048, max_seq_len=S, norm_eps=1e-5, **FULL_WIDTH["llama3-8b"])
    weights = synth_model(cfg, SEED)
    kern = f"mc_attn_qkv_wo_i4_bfloat_hd128_k2_q2_t{S // 2048}"
    for wide in ("1", "0"):
        monkeypatch.setenv("MC_ATTN_I4_WIDE", wide)
        names = set()
        agree = run_injected(acc, cfg, weights, S - 7, 12, dict(weight_format=mc.WFMT_I4, group_size=128), rel_logits=5e-3, max_ulp=2, max_frac=0.7,
                             what=f"8B int4 S={S} (MC_ATTN_I4_WIDE={wide})", launched=names)
        assert agree >= 10
        assert (kern in names) == (wide == "1"), sorted(names)
        assert ("mc_gemv_i4_bfloat_lin2_p1_e4" in names) == (wide == "0"), sorted(names)
        assert {"mc_gemv_i4_bfloat_lin2_p1_e2", "mc_gemv_i4_bfloat_lin7_p0_e1"} <= names, sorted(names)


@pytest.mark.slow   # (BASELINE's int8 config is S = 8192: test_llama3_8b_int8_at_8192_with_automatic_context_ranges)
def test_llama3_8b_int8_three_launch_layer_at_short_and_mid_contexts(acc, monkeypatch):
    # ... the same block at S = 2048 (64-slot ranges: `_t1`) and S = 8192 (`_t4`), full and at position 300 (most ranges empty), and across
    # the end of the cache (the ring turns).  Full contexts: run_injected's bounds against the oracle.  Position 300: int8 on bfloat rows sits
    # 4.3e-3 from the oracle vector-wise there with EITHER form of the layer (measured: 0.00427 / 0.00427 at S = 2048, 0.00427 / 0.00444 at
    # 8192; run_injected allows 3.9e-3) -- so the three launches are held to the five launches' own distance, and to the same tokens.
    import metalchat_amd as mc

    def distance(cfg, weights, n, names=None):
        om = mo.Model(cfg, weights)
        dec = mc.Decoder(acc, **mg.decoder_kwargs(cfg, weight_format=mc.WFMT_I8, group_size=128))
        dec.init_synthetic(SEED)
        dec.set_taps(True)
        dec.launch_log(True)
        k, v = random_cache(cfg, n, 100)
        om.set_kv(0, k, v)
        dec.import_kv(0, k, v)
        tok, worst, nrm, agree = 7, 0.0, 0.0, 0
        for i in range(6):
            otok, _ = om.step(tok, n + i)
            agree += int(dec.step(tok, n + i) == otok)
            a, b = mo.from_bf16(dec.hidden(0)).astype(np.float64), mo.from_bf16(om.hidden(0)).astype(np.float64)
            rms = np.sqrt(np.mean(b * b))
            worst = max(worst, float(np.max(np.abs(a - b) / (2.0 ** -7 * np.maximum(np.abs(b), rms)))))
            nrm = max(nrm, float(np.linalg.norm(a - b) / np.linalg.norm(b)))
            tok = otok
        if names is not None:
            names |= set(dec.launched())
        dec.release()
        om.close()
        return worst, nrm, agree

    for S, kern in ((2048, "mc_attn_qkv_wo_i8_bfloat_hd128_k4_q4_t1"), (8192, "mc_attn_qkv_wo_i8_bfloat_hd128_k4_q4_t4")):
        cfg = dict(dtype=BF16, n_layers=1, vocab=2048, max_seq_len=S, norm_eps=1e-5, **FULL_WIDTH["llama3-8b"])
        weights = synth_model(cfg, SEED, bits=8)
        if S == 2048:
            names = set()
            agree = run_injected(acc, cfg, weights, 2041, 10, dict(weight_format=mc.WFMT_I8, group_size=128), rel_logits=5e-3, max_ulp=2, max_frac=0.7,
                                 what="8B int8 S=2048 from 2041", launched=names)
            assert agree >= 8 and kern in names, sorted(names)
        names = set()
        w3, n3, a3 = distance(cfg, weights, 300, names)
        assert kern in names, sorted(names)
        monkeypatch.setenv("MC_ATTN_I8", "0")
        w5, n5, a5 = distance(cfg, weights, 300)
        monkeypatch.delenv("MC_ATTN_I8")
        print(f"S={S} position 300: three launches {w3:.2f} steps / {n3:.5f}, five launches {w5:.2f} / {n5:.5f}")
        assert w3 <= max(w5 * 1.1, 2.0) and n3 <= n5 * 1.1 and n3 <= 6e-3 and a3 >= 5 and a5 >= 5, (S, w3, n3, a3, w5, n5, a5)
        toks = {}
        for form in ("1", "0"):
            monkeypatch.setenv("MC_ATTN_I8", form)
            dec = mc.Decoder(acc, **mg.decoder_kwargs(cfg, weight_format=mc.WFMT_I8, group_size=128))
            dec.init_synthetic(SEED)
            k, v = random_cache(cfg, S - 6, 700)
            dec.import_kv(0, k, v)
            toks[form] = list(dec.generate(9, S - 6, 14))   # (past max_seq_len: the sink ring turns)
            dec.release()
        monkeypatch.delenv("MC_ATTN_I8")
        assert toks["1"] == toks["0"], (S, toks)


def t_weights_model(cfg, seed):
    """Plain T weights (nn::linear) exactly as mc_decoder_init_synthetic fills them with weight_format = T."""
    import synthgen as sg

    dt = cfg["dtype"]
    dim, H, KV, hd, ffn = cfg["dim"], cfg["n_heads"], cfg["n_kv_heads"], cfg["head_dim"], cfg["ffn_dim"]

    def lin(mid, out_f, in_f):
        return dict(kind=0, weight=mo.encode(dt, sg.values(seed, mid, out_f * in_f, 2, in_f).reshape(out_f, in_f)))

    def vec(mid, n):
        return mo.encode(dt, sg.values(seed, mid, n, 0))

    layers = []
    for i in range(cfg["n_layers"]):
        b = i * 16
        layers.append(dict(wq=lin(b + 0, H * hd, dim), wk=lin(b + 1, KV * hd, dim), wv=lin(b + 2, KV * hd, dim),
                           wo=lin(b + 3, dim, H * hd), w1=lin(b + 4, ffn, dim), w2=lin(b + 5, dim, ffn), w3=lin(b + 6, ffn, dim),
                           attention_norm=vec(b + 8, dim), ffn_norm=vec(b + 9, dim)))
    emb = mo.encode(dt, sg.values(seed, 0xFFFF0000, cfg["vocab"] * dim, 1).reshape(cfg["vocab"], dim))
    return dict(layers=layers, embedding=dict(kind=0, weight=emb), output=lin(0xFFFF0001, cfg["vocab"], dim),
                final_norm=vec(0xFFFF0002, dim))


@pytest.mark.parametrize("dtype", [BF16, F32])
def test_tinyllama_1b_shapes_end_to_end(acc, dtype):
    # BASELINE configs[0]: TinyLlama-1.1B -- head_dim 64, 8 query heads per kv head, ffn 5632 (a ragged K for the
    # 2048-weight chunks of the GEMV), plain T weights, the full 32000-row head.  Two blocks, from position 0 and at
    # S = 2048.  T = float pins the arithmetic (2e-4); T = bfloat is the benchmark's type.
    import metalchat_amd as mc

    cfg = dict(dtype=dtype, family=0, n_layers=2, vocab=32000, max_seq_len=2048, norm_eps=1e-5, dim=2048, n_heads=32,
               n_kv_heads=4, head_dim=64, ffn_dim=5632, rope_theta=10000.0, attn_scale=64 ** -0.5)
    weights = t_weights_model(cfg, SEED)
    om = mo.Model(cfg, weights)
    dec = mc.Decoder(acc, **mg.decoder_kwargs(cfg, weight_format=mc.WFMT_T, group_size=0))
    dec.init_synthetic(SEED)
    dec.set_taps(True)
    tok, agree = 5, 0
    for pos in range(5):
        otok, ologits = om.step(tok, pos)
        gtok = dec.step(tok, pos)
        for layer in range(-1, cfg["n_layers"]):
            if dtype == F32:
                parity.check(F32, dec.hidden(layer), om.hidden(layer), rel=2e-4, what=f"tinyllama f32 pos {pos} hidden[{layer}]")
                continue
            # (two blocks: the second block's output has passed two attention + ffn compositions, each of which can
            # move an element by a bf16 step)
            parity.check(BF16, dec.hidden(layer), om.hidden(layer), rel=3.9e-3 * (1 + max(layer, 0)), max_ulp=(2 + layer) if layer >= 0 else 0,
                         max_frac=(0.5 + 0.2 * layer) if layer >= 0 else 0.0, what=f"tinyllama pos {pos} hidden[{layer}]")
        if dtype == F32:
            parity.check(F32, dec.logits(), ologits, rel=2e-4, what=f"tinyllama f32 pos {pos} logits")
        else:
            # (measured: up to 3.2 scaled bf16 steps on single logits behind two blocks; the f32 twin holds 2e-4)
            parity.check(BF16, dec.logits(), ologits, rel=7.8e-3, max_ulp=4, max_frac=0.8, what=f"tinyllama pos {pos} logits")
        agree += int(gtok == otok)
        tok = otok
    assert agree >= 4
    dec.release()
    om.close()
    names = set()
    agree = run_injected(acc, cfg, weights, 2044, 8, dict(weight_format=mc.WFMT_T, group_size=0), rel_logits=7.8e-3,
                         max_ulp=3, max_frac=0.8, what=f"tinyllama S=2048 dt{dtype}", launched=names)
    assert agree >= 7
    if dtype == BF16:
        # (round 5: three launches per block -- the 4 kv heads as 8 virtual ones inside mc_attn_qkv_wo_w_*,
        #  test_tinyllama_takes_the_one_launch_block_as_eight_virtual_kv_heads below holds that form next to the five launches)
        # (round 6: TWO launches per block -- ffn_norm + w1|w3 + act*mul is a phase of the attention launch, mc_attn_qkv_wo_w13_w_*: tests/test_chain_gpu.py)
        assert {"mc_attn_qkv_wo_w13_w_bfloat_hd64_k4_q4_f3p3", "mc_gemv_w_bfloat_ling11_p0_e1", "mc_gemv_w_bfloat_ling4_p1_e5"} <= names, sorted(names)
        assert "mc_gemv_w_bfloat_ling4_p1_e2" not in names and "mc_attn_qkv_wo_w_bfloat_hd64_k4_q4" not in names, sorted(names)
        assert not {"mc_gemv_w_bfloat_ling4_p1_e4", "mc_attn_fused_bfloat", "mc_gemv_w_bfloat_ling4_p0_e1"} & names, sorted(names)


def test_llama32_1b_shapes_take_the_one_launch_block_with_plain_weights(acc, monkeypatch):
    # The reference's default model (src/llama.cc:19-31: Llama-3.2-1B -- dim 2048, 32 query / 8 kv heads of 64, ffn 8192, plain
    # bfloat weights): attention_norm + wq|wk|wv + rope + cache write + attention + wo + residual in ONE launch
    # (mc_attn_qkv_wo_w_bfloat_hd64_k4_q4, round 4), against the oracle at S = 2048 and at position 40 with injected caches --
    # and next to the five-launch form (MC_ATTN_QKV=0): the same tokens, logits within the suite's bound.
    import metalchat_amd as mc

    cfg = dict(dtype=BF16, family=0, n_layers=2, vocab=32000, max_seq_len=2048, norm_eps=1e-5, dim=2048, n_heads=32,
               n_kv_heads=8, head_dim=64, ffn_dim=8192, rope_theta=500000.0, attn_scale=64 ** -0.5)
    weights = t_weights_model(cfg, SEED)
    names = set()
    agree = run_injected(acc, cfg, weights, 2044, 8, dict(weight_format=mc.WFMT_T, group_size=0), rel_logits=7.8e-3,
                         max_ulp=3, max_frac=0.8, what="llama3.2-1b S=2048", launched=names)
    assert agree >= 7
    assert "mc_attn_qkv_wo_w13_w_bfloat_hd64_k4_q4_f4p4" in names and "mc_gemv_w_bfloat_ling4_p1_e4" not in names, sorted(names)   # (round 6: + w1|w3)
    agree = run_injected(acc, cfg, weights, 40, 8, dict(weight_format=mc.WFMT_T, group_size=0), rel_logits=7.8e-3,
                         max_ulp=3, max_frac=0.8, what="llama3.2-1b at position 40 (all but one range of the launch empty)")
    assert agree >= 7
    out = {}
    for form in ("1", "0"):
        monkeypatch.setenv("MC_ATTN_QKV", form)
        dec = mc.Decoder(acc, **mg.decoder_kwargs(cfg, weight_format=mc.WFMT_T, group_size=0))
        dec.init_synthetic(SEED)
        for layer in range(cfg["n_layers"]):
            k, v = random_cache(cfg, 1500, 300 + layer)
            dec.import_kv(layer, k, v)
        dec.launch_log(True)
        toks = list(dec.generate(9, 1500, 12))
        assert ("mc_attn_qkv_wo_w13_w_bfloat_hd64_k4_q4_f4p4" in set(dec.launched())) == (form == "1")
        out[form] = (toks, dec.logits().copy())
        dec.release()
    assert out["1"][0] == out["0"][0]
    parity.check(BF16, out["1"][1], out["0"][1], rel=7.8e-3, max_ulp=2, max_frac=0.6, what="one-launch block vs five launches, logits")


@pytest.mark.parametrize("shape,S", [("llama3.2-1b", 4096), pytest.param("tinyllama", 8192, marks=pytest.mark.slow),
                                     pytest.param("llama3-8b-int8", 4096, marks=pytest.mark.slow), pytest.param("gemma-7b", 4096, marks=pytest.mark.slow)])
def test_wide_ranges_keep_the_three_launch_layer_at_long_contexts(acc, monkeypatch, shape, S):
    # round 5: the one-launch blocks with 128- / 256-slot ranges (`_t2` / `_t4`) for plain bfloat weights (Llama-3.2-1B; TinyLlama as 8 virtual kv
    # heads) and int8 at S = 4096 -- against the oracle near the end of the cache and past it, and next to round 4's launches (MC_ATTN_I4_WIDE=0 /
    # MC_ATTN_I8=0): the same greedy tokens
    import metalchat_amd as mc

    if shape == "llama3-8b-int8":
        cfg = dict(dtype=BF16, n_layers=1, vocab=2048, max_seq_len=S, norm_eps=1e-5, **FULL_WIDTH["llama3-8b"])
        weights, fmt = synth_model(cfg, SEED, bits=8), dict(weight_format=mc.WFMT_I8, group_size=128)
        kern, off = f"mc_attn_qkv_wo_i8_bfloat_hd128_k4_q4_t{S // 2048}", {"MC_ATTN_I8": "0"}
    elif shape == "gemma-7b":   # (the gemma3 block with 256-slot ranges: 16 ranges x 16 kv heads at S = 4096; `_p2_t4` by name in test_attn_kernels_gpu.py)
        cfg = dict(dtype=BF16, n_layers=1, vocab=2048, max_seq_len=S, norm_eps=1e-5, dim=3072, n_heads=16, n_kv_heads=16, head_dim=256,
                   ffn_dim=4096, family=1, rope_theta=10000.0, rope_sliding_theta=10000.0, sliding_stride=2, attn_scale=256 ** -0.5)
        weights, fmt = synth_model(cfg, SEED), dict(weight_format=mc.WFMT_I4, group_size=128)
        kern, off = "mc_attn_qkv_wo_qkn_i4_bfloat_hd256_k2_p1_t4", {"MC_ATTN_WO_QKN": "0"}
    else:
        cfg = dict(dtype=BF16, family=0, n_layers=2, vocab=32000, max_seq_len=S, norm_eps=1e-5, dim=2048, n_heads=32,
                   n_kv_heads=8 if shape == "llama3.2-1b" else 4, head_dim=64, ffn_dim=8192 if shape == "llama3.2-1b" else 5632,
                   rope_theta=500000.0 if shape == "llama3.2-1b" else 10000.0, attn_scale=64 ** -0.5)
        weights, fmt = t_weights_model(cfg, SEED), dict(weight_format=mc.WFMT_T, group_size=0)
        kern, off = f"mc_attn_qkv_wo_w_bfloat_hd64_k4_q4_t{S // 2048}", {"MC_ATTN_I4_WIDE": "0"}
    toks = {}
    for form in ("wide", "off"):
        for k_ in ("MC_ATTN_I4_WIDE", "MC_ATTN_I8", "MC_ATTN_WO_QKN"):
            monkeypatch.delenv(k_, raising=False)
        if form == "off":
            for k_, v_ in off.items():
                monkeypatch.setenv(k_, v_)
        names = set()
        agree = run_injected(acc, cfg, weights, S - 5, 9, fmt, rel_logits=7.8e-3, max_ulp=3, max_frac=0.8, what=f"{shape} S={S} ({form})", launched=names)
        assert agree >= 7
        assert (kern in names) == (form == "wide"), sorted(names)


def test_tinyllama_takes_the_one_launch_block_as_eight_virtual_kv_heads(acc, monkeypatch):
    # BASELINE configs[0] (TinyLlama-1.1B: 4 kv heads x 8 query heads of 64, plain bfloat weights): the three-launch layer of
    # Llama-3.2-1B with the 4 kv heads launched as 8 VIRTUAL ones of 4 query heads each (round 5, decoder.cc kv_virtual_shift;
    # decode_kernels.hip attn_fused_bf kv_shift) -- against the oracle at S = 2048 and at position 40 with injected caches, and next
    # to the five-launch form (MC_KV_VIRTUAL=0): the same tokens, logits within the suite's bound, the same cache rows bit for bit.
    import metalchat_amd as mc

    cfg = dict(dtype=BF16, family=0, n_layers=2, vocab=32000, max_seq_len=2048, norm_eps=1e-5, dim=2048, n_heads=32,
               n_kv_heads=4, head_dim=64, ffn_dim=5632, rope_theta=10000.0, attn_scale=64 ** -0.5)
    weights = t_weights_model(cfg, SEED)
    names = set()
    agree = run_injected(acc, cfg, weights, 2044, 8, dict(weight_format=mc.WFMT_T, group_size=0), rel_logits=7.8e-3,
                         max_ulp=3, max_frac=0.8, what="tinyllama S=2048, virtual kv heads", launched=names)
    assert agree >= 7
    assert "mc_attn_qkv_wo_w13_w_bfloat_hd64_k4_q4_f3p3" in names and "mc_gemv_w_bfloat_ling4_p1_e4" not in names, sorted(names)   # (round 6: + w1|w3)
    out = {}
    for form in ("1", "0"):
        monkeypatch.setenv("MC_KV_VIRTUAL", form)
        dec = mc.Decoder(acc, **mg.decoder_kwargs(cfg, weight_format=mc.WFMT_T, group_size=0))
        dec.init_synthetic(SEED)
        for layer in range(cfg["n_layers"]):
            k, v = random_cache(cfg, 1500, 300 + layer)
            dec.import_kv(layer, k, v)
        dec.launch_log(True)
        toks = list(dec.generate(9, 1500, 12))
        assert ("mc_attn_qkv_wo_w13_w_bfloat_hd64_k4_q4_f3p3" in set(dec.launched())) == (form == "1"), sorted(set(dec.launched()))
        out[form] = (toks, dec.logits().copy(), dec.export_kv(0))
        dec.release()
    assert out["1"][0] == out["0"][0]
    # (the launches it replaces add the same products in the same order -- 64-slot ranges reduced in range order, the linear-order
    #  GEMV arithmetic -- so the two forms agree BIT FOR BIT, at a short context too: position 40, all but one range empty, where
    #  either form sits 3.1 scaled bf16 steps from the oracle on single elements of hidden[0], measured)
    parity.exact(out["1"][1], out["0"][1], "virtual kv heads vs five launches, logits")
    for start in (40,):
        got = {}
        for form in ("1", "0"):
            monkeypatch.setenv("MC_KV_VIRTUAL", form)
            dec = mc.Decoder(acc, **mg.decoder_kwargs(cfg, weight_format=mc.WFMT_T, group_size=0))
            dec.init_synthetic(SEED)
            for layer in range(cfg["n_layers"]):
                k, v = random_cache(cfg, start, 500 + layer)
                dec.import_kv(layer, k, v)
            got[form] = (list(dec.generate(11, start, 6)), dec.logits().copy())
            dec.release()
        assert got["1"][0] == got["0"][0]
        parity.exact(got["1"][1], got["0"][1], f"virtual kv heads vs five launches at position {start}, logits")
    # layer 0's cache rows do not depend on any attention: the rows the one-launch block wrote (twice each) are the GEMV's
    parity.exact(out["1"][2][0], out["0"][2][0], "K rows of layer 0")
    parity.exact(out["1"][2][1], out["0"][2][1], "V rows of layer 0")


def test_llama3_70b_widths_one_block(acc):
    # BASELINE configs[4] widths: dim 8192, 64 query / 8 kv heads, ffn 28672 -- rows of 4 and 14 KiB of int4 weights
    import metalchat_amd as mc

    # ... at the context bench.py runs them at (S = 2048: kv_len 2043 .. 2048 and four rolls)
    cfg = dict(dtype=BF16, family=0, n_layers=1, vocab=2048, max_seq_len=2048, norm_eps=1e-5, dim=8192, n_heads=64,
               n_kv_heads=8, head_dim=128, ffn_dim=28672, rope_theta=500000.0, attn_scale=128 ** -0.5)
    weights = synth_model(cfg, SEED)
    names = set()
    agree = run_injected(acc, cfg, weights, 2042, 10, dict(weight_format=mc.WFMT_I4, group_size=128), rel_logits=5e-3,
                         max_ulp=2, max_frac=0.7, what="70B widths S=2048", launched=names)
    assert agree >= 9
    # (K = 8192: the Wo GEMV stays a launch of its own behind the one-launch attention -- attn_block_kernels.hip; wq|wk|wv inside the attention
    #  launch was built in round 5, is tested below and measured no faster: off by default, decoder.cc attn_qkv_only_on)
    assert {"mc_gemv_i4_bfloat_lin4_p1_e4", "mc_attn_fused_bfloat", "mc_gemv_i4_bfloat_lin4_p0_e1", "mc_gemv_i4_bfloat_lin4_p1_e2",
            "mc_gemv_i4_bfloat_lin14_p0_e1", "mc_gemv_i4_bfloat_lin4_p1_e5"} <= names, sorted(names)


def test_llama3_70b_qkv_inside_the_attention_launch_equals_the_two_launches_bit_for_bit(acc, monkeypatch):
    # mc_attn_qkv_i4_bfloat_hd128_q4 = mc_gemv_i4_bfloat_lin4_p1_e4 + mc_attn_fused_bfloat: the GEMV's sums addition for addition, the same attention
    # phases -- hidden rows, logits, tokens and caches IDENTICAL, near an empty cache and across the end of a full one
    import metalchat_amd as mc

    cfg = dict(dtype=BF16, family=0, n_layers=2, vocab=2048, max_seq_len=2048, norm_eps=1e-5, dim=8192, n_heads=64,
               n_kv_heads=8, head_dim=128, ffn_dim=4096, rope_theta=500000.0, attn_scale=128 ** -0.5)
    S = cfg["max_seq_len"]
    out = {}
    for form, env in (("in", {"MC_ATTN_QKV_ONLY": "1"}), ("sep", {})):
        monkeypatch.delenv("MC_ATTN_QKV_ONLY", raising=False)
        for k_, v_ in env.items():
            monkeypatch.setenv(k_, v_)
        dec = mc.Decoder(acc, **mg.decoder_kwargs(cfg, weight_format=mc.WFMT_I4, group_size=128))
        dec.init_synthetic(SEED)
        dec.set_taps(True)
        dec.launch_log(True)
        rows = []
        for n_inject in (2, S - 4):
            for layer in range(cfg["n_layers"]):
                k, v = random_cache(cfg, n_inject, 900 + layer)
                dec.import_kv(layer, k, v)
            tok = 5
            for i in range(8):
                tok = dec.step(tok, n_inject + i)
                rows.append((tok, dec.logits().copy(), np.stack([dec.hidden(l) for l in range(-1, cfg["n_layers"])])))
        caches = [dec.export_kv(layer) for layer in range(cfg["n_layers"])]
        names = set(dec.launched())
        assert ("mc_attn_qkv_i4_bfloat_hd128_q4" in names) == (form == "in"), sorted(names)
        assert ({"mc_gemv_i4_bfloat_lin4_p1_e4", "mc_attn_fused_bfloat"} <= names) == (form == "sep"), sorted(names)
        out[form] = (rows, caches)
        dec.release()
    for i, ((ta, la, ha), (tb_, lb, hb)) in enumerate(zip(out["in"][0], out["sep"][0])):
        assert ta == tb_, i
        parity.exact(ha, hb, f"step {i}: hidden rows, wq|wk|wv inside the attention launch vs the GEMV + mc_attn_fused_bfloat")
        parity.exact(la, lb, f"step {i}: logits")
    for layer, ((ka, va), (kb_, vb_)) in enumerate(zip(out["in"][1], out["sep"][1])):
        parity.exact(ka, kb_, f"K cache of block {layer}")
        parity.exact(va, vb_, f"V cache of block {layer}")


@pytest.mark.parametrize("taps", [True, False])
def test_gemma_7b_widths_at_the_benchmark_context(acc, taps):
    # BASELINE configs[3] shapes on the gemma3 block: MHA (one query head per kv head: ONE live row of the 16-row MFMA
    # tile in QK^T and P.V), head_dim 256, K = 3072 (`_lin3s_`) and 24576 (`_lin12k4_`: round 6, the K range of a pair over four waves), S = 2048 with rolls.  taps = False is
    # the production launch sequence: both post-norms folded into the prologue of the GEMV that follows (`_p2_`).
    import metalchat_amd as mc

    cfg = dict(dtype=BF16, n_layers=1, vocab=2048, max_seq_len=2048, norm_eps=1e-5, dim=3072, n_heads=16, n_kv_heads=16, head_dim=256,
               ffn_dim=24576, family=1, rope_theta=10000.0, rope_sliding_theta=10000.0, sliding_stride=2, attn_scale=256 ** -0.5)
    weights = synth_model(cfg, SEED)
    names = set()
    # (four norms per block, a 24576-long w2 reduction and a 2048-term softmax / P.V per head: measured up to 1.03 x two scaled
    # bf16 steps on single elements of the block output -- three allowed; the vector-wise bounds are the llama ones)
    agree = run_injected(acc, cfg, weights, 2042, 10, dict(weight_format=mc.WFMT_I4, group_size=128), rel_logits=5e-3, max_ulp=3,
                         max_frac=0.7, what=f"gemma-7b widths S=2048 taps={taps}", taps=taps, launched=names)
    assert agree >= 9
    # (round 4: q_norm / k_norm, rope and the cache write ride in the attention launch; round 5: Wo, wq|wk|wv and the block's norms too --
    #  mc_attn_qkv_wo_qkn_i4_bfloat_hd256_k2_p1_t2 (one block: no post-norm in front of it), 16 ranges of 128 slots x 16 kv heads: THREE launches per block)
    want = {"mc_attn_qkv_wo_qkn_i4_bfloat_hd256_k2_p1_t2", "mc_gemv_i4_bfloat_lin12k4_p0_e0", "mc_gemv_i4_bfloat_lin3s_p1_e3" if taps else "mc_gemv_i4_bfloat_lin3s_p2_e3"}
    assert want <= names, sorted(names)
    # (`_lin3s_p{1,2}_e0` is the output head here: K = 3072 too)
    assert not ({"mc_rope_kv_bfloat", "mc_attn_fused_bfloat", "mc_attn_fused_qkn_bfloat", "mc_gemv_i4_bfloat_lin2_p0_e0"} & names), sorted(names)


@pytest.mark.parametrize("taps", [True, False])
def test_gemma_with_128_slot_ranges_takes_the_gemma_epilogue_behind_the_attention(acc, taps, monkeypatch):
    # gemma3 blocks whose attention is mc_attn_fused_t2_bfloat (block_plan.h plan_block, tail d): head_dim 128 and 16 kv heads at S = 4096 are
    # 64 x 16 workgroups of 64 slots -- more than two per CU -- and 32 x 16 = 512 of 128 slots, which fit (Gemma3-27B's widths have this shape).
    # Behind that launch Wo goes to `proj` and attention_post_norm (weights in [0.5, 1.5), not ones) + the residual follow: as a launch of their own
    # with taps, as the w1|w3 GEMV's prologue without.
    #   ONE block: against the oracle at the bounds of the one-block gemma cases (test_gemma_7b_widths_at_the_benchmark_context).
    #   TWO blocks (the second enters through the `_p2_e0` wq|wk|wv GEMV that carries the first one's ffn post-norm): those bounds were measured on
    #   one block's output and this model's second block lies outside them with ANY form of the attention (profiles/decode_plan_dispatch_diff.md:
    #   the same single-element figure with scores + P.V as launches of their own), so the second block is held to the distance of that form,
    #   MC_ATTN_T2=0 -- as test_llama3_8b_int8_three_launch_layer_at_short_and_mid_contexts holds one form to another: 1.1 x, the two differ in
    #   the order of the softmax and P.V partial sums only -- and to the oracle's tokens.
    import metalchat_amd as mc

    cfg = dict(dtype=BF16, n_layers=1, vocab=2048, max_seq_len=4096, norm_eps=1e-5, dim=2048, n_heads=16, n_kv_heads=16, head_dim=128,
               ffn_dim=4096, family=1, rope_theta=10000.0, rope_sliding_theta=10000.0, sliding_stride=2, attn_scale=128 ** -0.5)
    fmt = dict(weight_format=mc.WFMT_I4, group_size=128)
    never = QKV_WO + ("mc_attn_wo_i4_", "mc_attn_fused_bfloat", "mc_attn_fused_qkn_", "mc_attn_scores_")
    weights = synth_model(cfg, SEED)
    post = np.concatenate([mo.decode(BF16, w["attention_post_norm"]) for w in weights["layers"]])
    assert np.abs(post - 1.0).max() > 0.25
    names = set()
    agree = run_injected(acc, cfg, weights, 4090, 10, fmt, rel_logits=5e-3, max_ulp=3, max_frac=0.7,
                         what=f"gemma hd128 x 16 kv heads S=4096 taps={taps}", taps=taps, launched=names)
    assert agree >= 9
    assert {"mc_attn_fused_t2_bfloat", "mc_rope_kv_bfloat"} <= names, sorted(names)
    assert ("mc_rmsnorm_row_bfloat" in names) == taps, sorted(names)
    assert not [n for n in names if n.startswith(never)], sorted(names)

    cfg2 = dict(cfg, n_layers=2)
    weights2 = synth_model(cfg2, SEED)

    def distance():
        """worst single element (in scaled bf16 steps) and vector-wise distance from the oracle: of hidden[1] with taps, of the logits without"""
        om = mo.Model(cfg2, weights2)
        dec = mc.Decoder(acc, **mg.decoder_kwargs(cfg2, **fmt))
        dec.init_synthetic(SEED)
        dec.set_taps(taps)
        dec.launch_log(True)
        for layer in range(2):
            k, v = random_cache(cfg2, 4090, 100 + layer)
            om.set_kv(layer, k, v)
            dec.import_kv(layer, k, v)
        tok, worst, nrm, agree = 7, 0.0, 0.0, 0
        for i in range(10):
            otok, ologits = om.step(tok, 4090 + i)
            agree += int(dec.step(tok, 4090 + i) == otok)
            a, b = (dec.hidden(1), om.hidden(1)) if taps else (dec.logits(), ologits)
            a, b = mo.from_bf16(a).astype(np.float64), mo.from_bf16(b).astype(np.float64)
            rms = np.sqrt(np.mean(b * b))
            worst = max(worst, float(np.max(np.abs(a - b) / (2.0 ** -7 * np.maximum(np.abs(b), rms)))))
            nrm = max(nrm, float(np.linalg.norm(a - b) / np.linalg.norm(b)))
            tok = otok
        launched = set(dec.launched())
        dec.release()
        om.close()
        return worst, nrm, agree, launched

    wt, nt, at, names = distance()
    assert {"mc_attn_fused_t2_bfloat", "mc_gemv_i4_bfloat_lin1_p1_e0" if taps else "mc_gemv_i4_bfloat_lin1_p2_e0"} <= names, sorted(names)
    assert not [n for n in names if n.startswith(never)], sorted(names)
    monkeypatch.setenv("MC_ATTN_T2", "0")
    wc, nc, ac, control = distance()
    monkeypatch.delenv("MC_ATTN_T2")
    assert "mc_attn_scores_bfloat" in control and "mc_attn_fused_t2_bfloat" not in control, sorted(control)
    print(f"two blocks, taps={taps}: 128-slot ranges {wt:.2f} steps / {nt:.5f}, scores + P.V {wc:.2f} / {nc:.5f}")
    # (... and, so that the two forms cannot drift together unnoticed, vector-wise to 2e-2: the scores + P.V form -- round 1's launches, not the
    #  arm under test -- lies 1.59e-2 (hidden[1]) / 1.64e-2 (logits) from the oracle on this model over these ten steps across the end of the cache)
    assert wt <= wc * 1.1 and nt <= nc * 1.1 and nt <= 2e-2 and at >= 9 and ac >= 9, (wt, nt, at, wc, nc, ac)


@pytest.mark.parametrize("shape,S,env,name", [("gemma-7b", 2048, {}, "mc_attn_qkv_wo_qkn_i4_bfloat_hd256_k2_p1_t2"),
                                              ("gemma-7b", 2048, {"MC_ATTN_QKV_QKN": "0"}, "mc_attn_wo_qkn_i4_bfloat_hd256_k2_t2"),
                                              ("gemma-7b", 2040, {}, "mc_attn_fused_qkn_bfloat"),
                                              ("llama3-8b-int4", 2048, {}, "mc_attn_qkv_wo_i4_bfloat_hd128_k2_q2"),
                                              ("llama3-8b-int4", 2048, {"MC_ATTN_FUSED": "0"}, "mc_attn_scores_bfloat + mc_attn_pv_bfloat")])
def test_the_attention_kernel_the_decoder_names_is_the_one_it_launches(acc, monkeypatch, shape, S, env, name):
    """gemv_kernel_name("attn") (what bench.py prints as the attention kernel) is plan_block's answer for the first owned block between
    tokens -- no post-norm pending, so `_p1_` -- and therefore the kernel a step launches, gemma3's forms included."""
    import metalchat_amd as mc

    for k, v in env.items():
        monkeypatch.setenv(k, v)
    cfg, _, fmt, _ = _shape_cfg(shape, S, weights=False)
    dec = mc.Decoder(acc, **mg.decoder_kwargs(cfg, **fmt))
    dec.init_synthetic(SEED)
    assert dec.gemv_kernel_name("attn") == name
    dec.launch_log(True)
    dec.step(7, 0)
    assert set(name.split(" + ")) <= set(dec.launched()), sorted(set(dec.launched()))
    assert dec.gemv_kernel_name("attn") == name
    dec.release()


def test_rows_in_the_cache_do_not_move_across_a_roll(acc):
    # nn/cache.h:187-204: prefix kept, post region rotated left by one, new row last.  Small model, many rolls,
    # both dtypes; export(t + 1) must be the literal roll of export(t) bit for bit (only the last row is computed).
    import metalchat_amd as mc

    for dt in (BF16, F32):
        cfg = mg.tiny_cfg(dt, max_seq_len=24, n_layers=2)
        weights = mg.make_model(cfg, seed=3, quant="i4", group=32)
        dec = mc.Decoder(acc, **mg.decoder_kwargs(cfg, weight_format=mc.WFMT_I4, group_size=32))
        dec.load_model(weights)
        pre = int(cfg["max_seq_len"]).bit_length() - 1
        tok, prev = 3, None
        for pos in range(cfg["max_seq_len"] + 40):
            tok = dec.step(tok, pos)
            k, v = dec.export_kv(1)
            if pos >= cfg["max_seq_len"]:
                S = cfg["max_seq_len"]
                assert k.shape[0] == S
                for new, old in ((k, prev[0]), (v, prev[1])):
                    parity.exact(new[:pre], old[:pre], f"dt{dt} pos {pos}: sink prefix")
                    parity.exact(new[pre:S - 1], old[pre + 1:S], f"dt{dt} pos {pos}: rotated rows")
            prev = (k.copy(), v.copy())
        dec.release()


@pytest.mark.parametrize("max_seq", [2048, 8192])
def test_pv_ranges_folded_into_wo_equal_the_reduce_launch_bit_for_bit(acc, monkeypatch, max_seq):
    # P.V over four ranges of cache slots whose fp32 sums the Wo GEMV's prologue adds (gemv.h PRO_PARTS) must be the very
    # numbers of the same four ranges reduced by mc_attn_pv_reduce_T and followed by the plain Wo GEMV: hidden rows,
    # logits, tokens.  (A whole-context P.V adds the same products in another order: that is parity, not identity.)
    import metalchat_amd as mc

    monkeypatch.setenv("MC_PV_RANGES", "4")
    monkeypatch.setenv("MC_ATTN_FUSED", "0")  # (the two-launch attention: the one-launch form has no ranges to fold)
    # ... and the same waves per workgroup (they add their k-steps' sums in wave order): one round of loads per wave
    monkeypatch.setenv("MC_PV_BLOCK", "256" if max_seq == 2048 else "1024")

    cfg = dict(dtype=BF16, n_layers=2, vocab=2048, max_seq_len=max_seq, norm_eps=1e-5, **FULL_WIDTH["llama3-8b"])
    out = {}
    for fold in ("1", "0"):
        monkeypatch.setenv("MC_PV_FOLD", fold)
        dec = mc.Decoder(acc, **mg.decoder_kwargs(cfg, weight_format=mc.WFMT_I4, group_size=128))
        dec.init_synthetic(SEED)
        dec.set_taps(True)
        for layer in range(cfg["n_layers"]):
            k, v = random_cache(cfg, max_seq - 5, 300 + layer)
            dec.import_kv(layer, k, v)
        tok, rows = 11, []
        for i in range(9):  # up to the end of the cache and four rolls past it
            tok = dec.step(tok, max_seq - 5 + i)
            rows.append((tok, dec.logits().copy(), np.stack([dec.hidden(l) for l in range(-1, cfg["n_layers"])])))
        out[fold] = rows
        dec.release()
    for (ta, la, ha), (tb_, lb, hb) in zip(out["1"], out["0"]):
        assert ta == tb_
        parity.exact(la, lb, "logits, folded vs reduce launch")
        parity.exact(ha, hb, "hidden rows, folded vs reduce launch")


@pytest.mark.parametrize("shape", ["llama3-8b", "tinyllama", "gemma-7b", "llama3-8b-8192"])
def test_one_launch_attention_against_the_two_launch_form(acc, monkeypatch, shape):
    # mc_attn_fused_bfloat (scores, softmax, P.V of nn/attention.h:191-203 in one launch with two in-launch hand-offs) against
    # mc_attn_scores / mc_attn_pv + the partial-sum prologue of Wo: the same scores, numerators and denominators bit for bit,
    # the P.V sums added in another order (64-slot ranges in range order, against four ranges of interleaved k-steps) -- hidden
    # rows at most one bf16 step apart on a few elements, logits close, and the launch log shows which form ran.  Up to the
    # end of the cache and past it; a cache that is nearly EMPTY too (most ranges of the launch have nothing to publish).
    import metalchat_amd as mc

    if shape == "llama3-8b":
        cfg = dict(dtype=BF16, n_layers=2, vocab=2048, max_seq_len=2048, norm_eps=1e-5, **FULL_WIDTH["llama3-8b"])
        fmt = dict(weight_format=mc.WFMT_I4, group_size=128)
    elif shape == "llama3-8b-8192":
        cfg = dict(dtype=BF16, n_layers=1, vocab=2048, max_seq_len=8192, norm_eps=1e-5, **FULL_WIDTH["llama3-8b"])
        fmt = dict(weight_format=mc.WFMT_I8, group_size=128)
    elif shape == "tinyllama":
        cfg = dict(dtype=BF16, family=0, n_layers=2, vocab=2048, max_seq_len=2048, norm_eps=1e-5, dim=2048, n_heads=32, n_kv_heads=4, head_dim=64,
                   ffn_dim=5632, rope_theta=10000.0, attn_scale=64 ** -0.5)
        fmt = dict(weight_format=mc.WFMT_T, group_size=0)
    else:
        cfg = dict(dtype=BF16, n_layers=2, vocab=2048, max_seq_len=2048, norm_eps=1e-5, dim=3072, n_heads=16, n_kv_heads=16, head_dim=256,
                   ffn_dim=24576, family=1, rope_theta=10000.0, rope_sliding_theta=10000.0, sliding_stride=2, attn_scale=256 ** -0.5)
        fmt = dict(weight_format=mc.WFMT_I4, group_size=128)
    S = cfg["max_seq_len"]
    out = {}
    monkeypatch.setenv("MC_ATTN_FUSED_WGS", "4")  # (S = 8192 is four workgroups per CU: by default the two-launch form)
    monkeypatch.setenv("MC_ATTN_WO", "0")          # (the attention forms by themselves: the Wo GEMV as a launch of its own)
    for fused in ("1", "0"):
        monkeypatch.setenv("MC_ATTN_FUSED", fused)
        dec = mc.Decoder(acc, **mg.decoder_kwargs(cfg, **fmt))
        dec.init_synthetic(SEED)
        dec.set_taps(True)
        dec.launch_log(True)
        rows = []
        for n_inject in (3, S - 5):
            for layer in range(cfg["n_layers"]):
                k, v = random_cache(cfg, n_inject, 500 + layer)
                dec.import_kv(layer, k, v)
            tok = 11
            for i in range(9):
                tok = dec.step(tok, n_inject + i)
                rows.append((tok, dec.logits().copy(), np.stack([dec.hidden(l) for l in range(-1, cfg["n_layers"])])))
        names = set(dec.launched())
        # (gemma3: the one-launch form carries q_norm / k_norm + rope too, mc_attn_fused_qkn_bfloat)
        assert ("mc_attn_fused_bfloat" in names or "mc_attn_fused_qkn_bfloat" in names) == (fused == "1"), sorted(names)
        assert ("mc_attn_pv_bfloat" in names) == (fused == "0"), sorted(names)
        out[fused] = rows
        dec.release()
    # Each form is held to the oracle element by element in the tests above; between the two forms (a last-bit difference in a
    # few elements of the attention row reaches every output of the Wo GEMV, so about half of a block's output lands on the
    # neighbouring bf16 value) the bound is vector-wise: 1.5 bf16 steps per block, and the same greedy tokens.
    def nrm(a, b):
        a, b = mo.from_bf16(a).astype(np.float64), mo.from_bf16(b).astype(np.float64)
        return float(np.linalg.norm(a - b) / (np.linalg.norm(b) + 1e-30))

    same = 0
    for i, ((ta, la, ha), (tb_, lb, hb)) in enumerate(zip(out["1"], out["0"])):
        same += int(ta == tb_)
        parity.exact(ha[0], hb[0], f"{shape} step {i}: the embedding row")
        for layer in range(1, ha.shape[0]):
            # (measured up to 0.0095 behind two gemma3 blocks: four norms each renormalise the difference of the block before)
            assert nrm(ha[layer], hb[layer]) <= 6e-3 * layer, f"{shape} step {i} hidden[{layer - 1}], one launch vs two: {nrm(ha[layer], hb[layer]):.3g}"
        assert nrm(la, lb) <= 6e-3 * (ha.shape[0] + 1), f"{shape} step {i} logits, one launch vs two: {nrm(la, lb):.3g}"
    assert same >= len(out["1"]) - 2, (shape, same)


@pytest.mark.parametrize("shape", ["gemma-7b", "gemma-hd128-gqa"])
def test_gemma_norm_and_rope_inside_the_attention_launch_equal_the_two_launches_bit_for_bit(acc, monkeypatch, shape):
    # mc_attn_fused_qkn_bfloat = mc_rope_kv_bfloat (q_norm / k_norm over whole heads, rotation, cache write: nn/attention.h:170-177) +
    # mc_attn_fused_bfloat: hidden rows, logits, caches and tokens must be IDENTICAL to the two launches, near an empty cache and
    # across the end of a full one (the ring turns); sliding and global layers (two rope tables)
    import metalchat_amd as mc

    monkeypatch.setenv("MC_ATTN_WO_QKN", "0")  # (the attention launch by itself: with Wo inside too it is mc_attn_wo_qkn_*, tested below)
    base = dict(dtype=BF16, n_layers=2, vocab=2048, norm_eps=1e-5, family=1, rope_theta=10000.0, rope_sliding_theta=10000.0, sliding_stride=2)
    if shape == "gemma-7b":
        cfg = dict(base, max_seq_len=2048, dim=3072, n_heads=16, n_kv_heads=16, head_dim=256, ffn_dim=4096, attn_scale=256 ** -0.5)
    else:  # four query heads per kv head, head_dim 128
        cfg = dict(base, max_seq_len=2048, dim=2048, n_heads=16, n_kv_heads=4, head_dim=128, ffn_dim=4096, attn_scale=128 ** -0.5)
    S = cfg["max_seq_len"]
    out = {}
    for form, env in (("qkn", {}), ("sep", {"MC_ATTN_QKN": "0"})):
        monkeypatch.delenv("MC_ATTN_QKN", raising=False)
        for k_, v_ in env.items():
            monkeypatch.setenv(k_, v_)
        dec = mc.Decoder(acc, **mg.decoder_kwargs(cfg, weight_format=mc.WFMT_I4, group_size=128))
        dec.init_synthetic(SEED)
        dec.set_taps(True)
        dec.launch_log(True)
        rows = []
        for n_inject in (2, S - 4):
            for layer in range(cfg["n_layers"]):
                k, v = random_cache(cfg, n_inject, 700 + layer)
                dec.import_kv(layer, k, v)
            tok = 5
            for i in range(8):
                tok = dec.step(tok, n_inject + i)
                rows.append((tok, dec.logits().copy(), np.stack([dec.hidden(l) for l in range(-1, cfg["n_layers"])])))
        kk, vv = dec.export_kv(cfg["n_layers"] - 1)
        names = set(dec.launched())
        assert ("mc_attn_fused_qkn_bfloat" in names) == (form == "qkn"), sorted(names)
        assert ("mc_rope_kv_bfloat" in names) == (form == "sep"), sorted(names)
        out[form] = (rows, kk, vv)
        dec.release()
    for i, ((ta, la, ha), (tb_, lb, hb)) in enumerate(zip(out["qkn"][0], out["sep"][0])):
        assert ta == tb_, (shape, i)
        parity.exact(ha, hb, f"{shape} step {i}: hidden rows, one launch vs rope_kv + attention")
        parity.exact(la, lb, f"{shape} step {i}: logits")
    parity.exact(out["qkn"][1], out["sep"][1], f"{shape}: K cache")
    parity.exact(out["qkn"][2], out["sep"][2], f"{shape}: V cache")


@pytest.mark.parametrize("shape", ["llama3-8b", "llama3-8b-1024", "llama3-8b-768", "hd64", "gemma-hd256", "llama3-8b-2040"])
def test_attention_and_wo_in_one_launch_equal_the_two_launches_bit_for_bit(acc, monkeypatch, shape):
    # mc_attn_wo_i4_bfloat_* = mc_attn_fused_bfloat + the Wo GEMV (attn_block_kernels.hip): the same attention phases, the same row, the same per-row arithmetic -- hidden rows, logits, caches and tokens must be IDENTICAL to the two launches, near an empty
    # cache and across the end of a full one; the launch log shows which form ran.
    import metalchat_amd as mc

    base = dict(dtype=BF16, n_layers=2, vocab=2048, norm_eps=1e-5)
    if shape in ("llama3-8b", "llama3-8b-2040"):   # (2040: the 32 ranges of 2048, the last one 56 slots long)
        cfg = dict(base, max_seq_len=2040 if shape.endswith("2040") else 2048, **FULL_WIDTH["llama3-8b"])
        kernel = "mc_attn_wo_i4_bfloat_hd128_k2"
    elif shape == "llama3-8b-1024":  # 128 workgroups: every wave owns TWO row pairs of Wo (the most the kernel holds)
        cfg = dict(base, max_seq_len=1024, **FULL_WIDTH["llama3-8b"])
        kernel = "mc_attn_wo_i4_bfloat_hd128_k2"
    elif shape == "llama3-8b-768":   # 96 workgroups: 768 waves for 2048 pairs -- two or three pairs per wave: the host must not take it
        cfg = dict(base, max_seq_len=768, **FULL_WIDTH["llama3-8b"])
        kernel = None
    elif shape == "hd64":
        cfg = dict(base, max_seq_len=2048, family=0, dim=2048, n_heads=32, n_kv_heads=8, head_dim=64, ffn_dim=4096, rope_theta=10000.0,
                   attn_scale=64 ** -0.5)
        kernel = "mc_attn_wo_i4_bfloat_hd64_k1"
    else:  # gemma3 block, head_dim 256, Wo stored without a residual (its post-norm adds it); 1024 slots: one workgroup per CU
        cfg = dict(base, max_seq_len=1024, dim=3072, n_heads=16, n_kv_heads=16, head_dim=256, ffn_dim=4096, family=1, rope_theta=10000.0,
                   rope_sliding_theta=10000.0, sliding_stride=2, attn_scale=256 ** -0.5)
        kernel = "mc_attn_wo_qkn_i4_bfloat_hd256_k2_t1"   # (round 5: q_norm / k_norm + rope + cache write in the launch too)
    S = cfg["max_seq_len"]
    # "qkv": the default where it is built (round 4: wq|wk|wv, attention and Wo in ONE launch, mc_attn_qkv_wo_*);  "wo": the wq|wk|wv GEMV,
    # then attention + Wo in one launch;  "sep": the GEMV, mc_attn_fused_bfloat, then the Wo GEMV
    qkv_kernel = {"llama3-8b": "mc_attn_qkv_wo_i4_bfloat_hd128_k2_q2", "llama3-8b-2040": "mc_attn_qkv_wo_i4_bfloat_hd128_k2_q2",
                  "gemma-hd256": "mc_attn_qkv_wo_qkn_i4_bfloat_hd256_k2_p1_t1"}.get(shape)   # (gemma3 with parity taps: every block starts at its pre-norm)
    out = {}
    forms = [("qkv", {}), ("wo", {"MC_ATTN_QKV": "0"}), ("sep", {"MC_ATTN_WO": "0"})]
    if shape == "gemma-hd256":   # ... and round 4's form: mc_rope_kv, then attention + Wo in one launch
        forms.append(("rope_wo", {"MC_ATTN_WO_QKN": "0"}))
    for form, env in forms:
        for k_ in ("MC_ATTN_WO", "MC_ATTN_QKV", "MC_ATTN_WO_QKN"):
            monkeypatch.delenv(k_, raising=False)
        for k_, v_ in env.items():
            monkeypatch.setenv(k_, v_)
        dec = mc.Decoder(acc, **mg.decoder_kwargs(cfg, weight_format=mc.WFMT_I4, group_size=128))
        dec.init_synthetic(SEED)
        dec.set_taps(True)
        dec.launch_log(True)
        rows = []
        for n_inject in (2, S - 4):
            for layer in range(cfg["n_layers"]):
                k, v = random_cache(cfg, n_inject, 700 + layer)
                dec.import_kv(layer, k, v)
            tok = 5
            for i in range(8):
                tok = dec.step(tok, n_inject + i)
                rows.append((tok, dec.logits().copy(), np.stack([dec.hidden(l) for l in range(-1, cfg["n_layers"])])))
        kk, vv = dec.export_kv(cfg["n_layers"] - 1)
        names = set(dec.launched())
        if kernel is None:   # a shape the one-launch form with Wo does not cover: both forms are attention + a Wo launch
            assert not any(n.startswith("mc_attn_wo_") for n in names) and "mc_attn_fused_bfloat" in names, sorted(names)
        else:
            took_qkv = form == "qkv" and qkv_kernel is not None
            assert (qkv_kernel in names) == took_qkv, sorted(names)
            if form == "rope_wo":
                assert {"mc_attn_wo_i4_bfloat_hd256_k2", "mc_rope_kv_bfloat"} <= names and kernel not in names, sorted(names)
            else:
                assert (kernel in names) == (form != "sep" and not took_qkv), sorted(names)
            assert ("mc_attn_fused_bfloat" in names or "mc_attn_fused_qkn_bfloat" in names) == (form == "sep"), sorted(names)
            if shape != "gemma-hd256":   # (there the output head is a `_lin3s_p1_e0` launch too)
                assert any(n.endswith("_p1_e4") or n.endswith("_p2_e0") or n.endswith("_p1_e0") for n in names) == (not took_qkv), sorted(names)
        out[form] = (rows, kk, vv)
        dec.release()
    for form in [f for f, _ in forms if f != "sep"]:
        for i, ((ta, la, ha), (tb_, lb, hb)) in enumerate(zip(out[form][0], out["sep"][0])):
            assert ta == tb_, (shape, form, i)
            parity.exact(ha, hb, f"{shape} step {i}: hidden rows, {form} vs separate launches")
            parity.exact(la, lb, f"{shape} step {i}: logits, {form}")
        parity.exact(out[form][1], out["sep"][1], f"{shape}: K cache, {form}")
        parity.exact(out[form][2], out["sep"][2], f"{shape}: V cache, {form}")


def test_gemma_7b_attention_block_with_wo_inside_against_the_two_launches(acc, monkeypatch):
    # "block": mc_attn_qkv_wo_qkn_i4_bfloat_hd256_k2_p{1,2}_t2 (round 5: the post-norm of the block before, attention_norm, wq|wk|wv, q_norm /
    # k_norm, rope, cache write, attention over 128-slot ranges, Wo in ONE launch); "wo": the wq|wk|wv GEMV, then
    # mc_attn_wo_qkn_i4_bfloat_hd256_k2_t2; "sep": the GEMV, mc_attn_fused_qkn_bfloat (64-slot ranges), the Wo GEMV -- at Gemma-7B's widths,
    # S = 2048.  "block" against "wo": the same arithmetic (the GEMV's sums addition for addition) -- BIT FOR BIT, with parity taps (every
    # block starts at its pre-norm: `_p1_`) and in the production sequence (the post-norms folded: `_p2_` from the second block on).
    # Against "sep": the same scores and numerators, the denominators and the P.V sums added in another grouping -- the vector-wise bound
    # of test_one_launch_attention_against_the_two_launch_form and the same greedy tokens; the caches of the first block bit for bit (its
    # K / V rows do not depend on the range width).  Near an empty cache and across the end of a full one.
    import metalchat_amd as mc

    cfg = dict(dtype=BF16, n_layers=2, vocab=2048, max_seq_len=2048, norm_eps=1e-5, dim=3072, n_heads=16, n_kv_heads=16, head_dim=256,
               ffn_dim=4096, family=1, rope_theta=10000.0, rope_sliding_theta=10000.0, sliding_stride=2, attn_scale=256 ** -0.5)
    S = cfg["max_seq_len"]
    out = {}
    for taps in (True, False):
        for form, env in (("block", {}), ("wo", {"MC_ATTN_QKV_QKN": "0"}), ("sep", {"MC_ATTN_WO_QKN": "0"})):
            monkeypatch.delenv("MC_ATTN_WO_QKN", raising=False)
            monkeypatch.delenv("MC_ATTN_QKV_QKN", raising=False)
            for k_, v_ in env.items():
                monkeypatch.setenv(k_, v_)
            dec = mc.Decoder(acc, **mg.decoder_kwargs(cfg, weight_format=mc.WFMT_I4, group_size=128))
            dec.init_synthetic(SEED)
            dec.set_taps(taps)
            dec.launch_log(True)
            rows = []
            for n_inject in (2, S - 4):
                for layer in range(cfg["n_layers"]):
                    k, v = random_cache(cfg, n_inject, 700 + layer)
                    dec.import_kv(layer, k, v)
                tok = 5
                for i in range(8):
                    tok = dec.step(tok, n_inject + i)
                    hid = np.stack([dec.hidden(l) for l in range(-1, cfg["n_layers"])]) if taps else np.zeros(1, np.uint16)
                    rows.append((tok, dec.logits().copy(), hid))
            caches = [dec.export_kv(layer) for layer in range(cfg["n_layers"])]
            names = set(dec.launched())
            assert ("mc_attn_wo_qkn_i4_bfloat_hd256_k2_t2" in names) == (form == "wo"), sorted(names)
            assert ("mc_attn_fused_qkn_bfloat" in names) == (form == "sep"), sorted(names)
            assert ("mc_attn_qkv_wo_qkn_i4_bfloat_hd256_k2_p1_t2" in names) == (form == "block"), sorted(names)
            assert ("mc_attn_qkv_wo_qkn_i4_bfloat_hd256_k2_p2_t2" in names) == (form == "block" and not taps), sorted(names)
            out[form, taps] = (rows, caches)
            dec.release()

    def nrm(a, b):
        a, b = mo.from_bf16(a).astype(np.float64), mo.from_bf16(b).astype(np.float64)
        return float(np.linalg.norm(a - b) / (np.linalg.norm(b) + 1e-30))

    for taps in (True, False):
        for i, ((ta, la, ha), (tb_, lb, hb)) in enumerate(zip(out["block", taps][0], out["wo", taps][0])):
            assert ta == tb_, (taps, i)
            parity.exact(ha, hb, f"taps {taps} step {i}: hidden rows, the block in one launch vs the wq|wk|wv GEMV + attention with Wo")
            parity.exact(la, lb, f"taps {taps} step {i}: logits, the block in one launch")
        for layer, ((ka, va), (kb_, vb_)) in enumerate(zip(out["block", taps][1], out["wo", taps][1])):
            parity.exact(ka, kb_, f"taps {taps}: K cache of block {layer}, the block in one launch")
            parity.exact(va, vb_, f"taps {taps}: V cache of block {layer}")
    same = 0
    for i, ((ta, la, ha), (tb_, lb, hb)) in enumerate(zip(out["wo", True][0], out["sep", True][0])):
        same += int(ta == tb_)
        parity.exact(ha[0], hb[0], f"step {i}: the embedding row")
        for layer in range(1, ha.shape[0]):
            # (measured up to 0.0143 behind the second block: a last-bit difference in the attention row moves about half of Wo's outputs to
            #  the neighbouring bf16 value and four norms per block renormalise it; each form is held to the ORACLE element by element in
            #  test_gemma_7b_widths_at_the_benchmark_context and test_attn_kernels_gpu.py)
            assert nrm(ha[layer], hb[layer]) <= 1e-2 * layer, f"step {i} hidden[{layer - 1}], Wo inside vs two launches: {nrm(ha[layer], hb[layer]):.3g}"
        assert nrm(la, lb) <= 1e-2 * (ha.shape[0] + 1), f"step {i} logits: {nrm(la, lb):.3g}"
    assert same >= len(out["wo", True][0]) - 2, same
    parity.exact(out["wo", True][1][0][0], out["sep", True][1][0][0], "K cache of the first block")
    parity.exact(out["wo", True][1][0][1], out["sep", True][1][0][1], "V cache of the first block")


@pytest.mark.parametrize("shape", ["gemma-7b", "llama3-8b-int4-8192", "tinyllama-4096", "llama3-8b-int4-2040"])
def test_graph_replay_of_the_round5_blocks_equals_eager_across_the_end_of_the_cache(acc, shape):
    # The launches this round added to the default path -- the gemma3 block (mc_attn_qkv_wo_qkn_*: `_p1_` then `_p2_`), the int4 block with 256-slot
    # ranges, the plain-bfloat block with 128-slot ranges on 8 virtual kv heads -- in mc_decoder_generate's hipGraph replay against the eager
    # launches: the same 40 greedy tokens from 12 slots before the end of the cache on (the ring turns 28 times), the same last logits, bit for bit.
    import metalchat_amd as mc

    if shape == "gemma-7b":
        cfg = dict(dtype=BF16, n_layers=2, vocab=2048, max_seq_len=2048, norm_eps=1e-5, dim=3072, n_heads=16, n_kv_heads=16, head_dim=256,
                   ffn_dim=4096, family=1, rope_theta=10000.0, rope_sliding_theta=10000.0, sliding_stride=2, attn_scale=256 ** -0.5)
        fmt, kern = dict(weight_format=mc.WFMT_I4, group_size=128), "mc_attn_qkv_wo_qkn_i4_bfloat_hd256_k2_p2_t2"
    elif shape == "llama3-8b-int4-8192":
        cfg = dict(dtype=BF16, n_layers=2, vocab=2048, max_seq_len=8192, norm_eps=1e-5, **FULL_WIDTH["llama3-8b"])
        fmt, kern = dict(weight_format=mc.WFMT_I4, group_size=128), "mc_attn_qkv_wo_i4_bfloat_hd128_k2_q2_t4"
    elif shape == "llama3-8b-int4-2040":   # (the bench's block with the last of its 32 ranges 56 slots long)
        cfg = dict(dtype=BF16, n_layers=2, vocab=2048, max_seq_len=2040, norm_eps=1e-5, **FULL_WIDTH["llama3-8b"])
        fmt, kern = dict(weight_format=mc.WFMT_I4, group_size=128), "mc_attn_qkv_wo_i4_bfloat_hd128_k2_q2"
    else:
        cfg = dict(dtype=BF16, family=0, n_layers=2, vocab=32000, max_seq_len=4096, norm_eps=1e-5, dim=2048, n_heads=32, n_kv_heads=4, head_dim=64,
                   ffn_dim=5632, rope_theta=10000.0, attn_scale=64 ** -0.5)
        fmt, kern = dict(weight_format=mc.WFMT_T, group_size=0), "mc_attn_qkv_wo_w_bfloat_hd64_k4_q4_t2"
    S = cfg["max_seq_len"]
    out = {}
    for graph in (0, 1):
        dec = mc.Decoder(acc, **mg.decoder_kwargs(cfg, use_graph=graph, **fmt))
        dec.init_synthetic(SEED)
        for layer in range(cfg["n_layers"]):
            k, v = random_cache(cfg, S - 12, 1100 + layer)
            dec.import_kv(layer, k, v)
        dec.launch_log(True)
        toks = list(dec.generate(7, S - 12, 40))
        assert kern in set(dec.launched()), sorted(set(dec.launched()))
        out[graph] = (toks, dec.logits().copy())
        dec.release()
    assert out[0][0] == out[1][0], shape
    parity.exact(out[0][1], out[1][1], f"{shape}: the last logits, graph replay vs eager")


# ---- contexts that are not whole 64-slot ranges.  The decoder takes any max_seq_len that is a multiple of 8 and counts nsplit = ceil(S / 64) ranges,
# the last one short; the kernels clamp their reads at max_seq and mask the slots past kv_len.  Each case: one full-width block against the oracle from
# five slots before the end of the cache to seven steps past it (kv_len inside the short last range, then the sink ring: pre_len 10 at 2040, 9 at 1000,
# 11 at 4032 .. 8120), and the launch form the admission gates in decoder.cc pick, by kernel name -- a change of gate has to change this table.
# (form: kernels that must run, kernels that must not)
def _shape_cfg(shape, S, weights=True):
    """weights=False: no host copy of the synthetic weights (the third value is None)"""
    import metalchat_amd as mc

    synth = synth_model if weights else (lambda *a, **k: None)
    t_weights = t_weights_model if weights else (lambda *a: None)

    if shape.startswith("llama3-8b"):
        cfg = dict(dtype=BF16, n_layers=1, vocab=2048, max_seq_len=S, norm_eps=1e-5, **FULL_WIDTH["llama3-8b"])
        if shape == "llama3-8b-int8":
            return cfg, synth(cfg, SEED, bits=8), dict(weight_format=mc.WFMT_I8, group_size=128), dict(rel_logits=5e-3, max_ulp=2, max_frac=0.7)
        return cfg, synth(cfg, SEED), dict(weight_format=mc.WFMT_I4, group_size=128), dict(rel_logits=5e-3, max_ulp=2, max_frac=0.7)
    if shape == "gemma-7b":
        cfg = dict(dtype=BF16, n_layers=1, vocab=2048, max_seq_len=S, norm_eps=1e-5, dim=3072, n_heads=16, n_kv_heads=16, head_dim=256,
                   ffn_dim=4096, family=1, rope_theta=10000.0, rope_sliding_theta=10000.0, sliding_stride=2, attn_scale=256 ** -0.5)
        # (the bounds of test_gemma_7b_widths_at_the_benchmark_context)
        return cfg, synth(cfg, SEED), dict(weight_format=mc.WFMT_I4, group_size=128), dict(rel_logits=5e-3, max_ulp=3, max_frac=0.7)
    cfg = dict(dtype=BF16, family=0, n_layers=1, vocab=2048, max_seq_len=S, norm_eps=1e-5, dim=2048, n_heads=32,
               n_kv_heads=8 if shape == "llama3.2-1b" else 4, head_dim=64, ffn_dim=8192 if shape == "llama3.2-1b" else 5632,
               rope_theta=500000.0 if shape == "llama3.2-1b" else 10000.0, attn_scale=64 ** -0.5)
    return cfg, t_weights(cfg, SEED), dict(weight_format=mc.WFMT_T, group_size=0), dict(rel_logits=7.8e-3, max_ulp=3, max_frac=0.8)


QKV_WO = ("mc_attn_qkv_wo_i4_", "mc_attn_qkv_wo_i8_", "mc_attn_qkv_wo_w_", "mc_attn_qkv_wo_w13_", "mc_attn_qkv_wo_qkn_", "mc_attn_wo_qkn_")
PARTIAL_RANGE_FORMS = {
    # S = 2040: 32 ranges per kv head as at 2048 -- the one-launch blocks of the benchmark context, the last range 56 slots
    ("llama3-8b-int4", 2040): ({"mc_attn_qkv_wo_i4_bfloat_hd128_k2_q2"}, {"mc_attn_fused_bfloat", "mc_gemv_i4_bfloat_lin2_p1_e4"}),
    ("llama3-8b-int8", 2040): ({"mc_attn_qkv_wo_i8_bfloat_hd128_k4_q4_t1"}, {"mc_attn_fused_bfloat", "mc_gemv_i8_bfloat_ling4_p1_e4"}),
    # (gemma3: block_plan.h plan_block, tail a, takes whole ranges only -- the attention with q_norm / k_norm inside, between the two GEMVs)
    ("gemma-7b", 2040): ({"mc_attn_fused_qkn_bfloat"}, set(QKV_WO)),
    # S = 1000: 16 ranges per kv head, as at 1024, and the same form as there -- so the steps up to the end of the cache are held BIT FOR BIT to a
    # decoder with S = 1024 on the same rows (kv_len 996 .. 1000: the last range 40 slots long) instead of the oracle: measured at 4.7e-3 (int4),
    # 1.04 x two scaled steps (int8) and 3.95e-3 (Llama-3.2-1B) from the oracle vector-wise, where run_injected allows 3.9e-3 -- the distance of
    # these forms at a context of 1000 slots, whole ranges or not (see test_llama3_8b_int8_three_launch_layer_at_short_and_mid_contexts: 4.3e-3
    # at position 300 with either form).
    #   int4: 24 of the kv head's 384 wq|wk|wv row pairs per range, the block holds 16 -- the GEMV, then attention + Wo
    ("llama3-8b-int4", 1000): ({"mc_attn_wo_i4_bfloat_hd128_k2", "mc_gemv_i4_bfloat_lin2_p1_e4"}, {"mc_attn_qkv_wo_i4_bfloat_hd128_k2_q2"}, 1024),
    # (int8: 24 pairs per range against 16 -- the five launches)
    ("llama3-8b-int8", 1000): ({"mc_attn_fused_bfloat", "mc_gemv_i8_bfloat_ling4_p1_e4"}, set(QKV_WO), 1024),
    # (plain bfloat: 12 pairs per range against 8 -- the block leaves the one launch)
    ("llama3.2-1b", 1000): ({"mc_gemv_w_bfloat_ling4_p1_e4", "mc_attn_fused_bfloat"}, set(QKV_WO), 1024),
    ("tinyllama", 1000): ({"mc_gemv_w_bfloat_ling4_p1_e4", "mc_attn_fused_bfloat"}, set(QKV_WO)),
    # (gemma3: 16 x 16 workgroups, one per CU -- the rope launch, then attention + Wo in one launch: round 4's form)
    ("gemma-7b", 1000): ({"mc_attn_wo_i4_bfloat_hd256_k2", "mc_rope_kv_bfloat"}, set(QKV_WO)),
    # Where the wide ranges are refused (block_plan.h plan_block: forms 2, 3 and 5 take S % (64 t) == 0 only, whole_range_tiles;
    # attn_fused_t2 an even nsplit).  What the decoder takes today:
    #   S = 4040 (63 ranges and 8 slots: nsplit 64) and 4032 (63 whole ranges, odd): 64 / 63 x 8 workgroups of the one-launch attention between
    #   the wq|wk|wv and Wo GEMVs -- five launches per layer, where 4096 takes the three of `_t2`
    ("llama3-8b-int4", 4040): ({"mc_attn_fused_bfloat", "mc_gemv_i4_bfloat_lin2_p1_e4"}, set(QKV_WO)),
    ("llama3-8b-int4", 4032): ({"mc_attn_fused_bfloat", "mc_gemv_i4_bfloat_lin2_p1_e4"}, set(QKV_WO)),
    ("llama3.2-1b", 4040): ({"mc_gemv_w_bfloat_ling4_p1_e4", "mc_attn_fused_bfloat"}, set(QKV_WO)),
    ("llama3.2-1b", 4032): ({"mc_gemv_w_bfloat_ling4_p1_e4", "mc_attn_fused_bfloat"}, set(QKV_WO)),
    #   S = 8120 int8 (nsplit 127, odd; 1016 workgroups of 64 slots are more than can wait for one another): scores + P.V in two launches, the P.V
    #   context ranges folded into the Wo GEMV -- where 8192 takes the three launches of `_t4`
    ("llama3-8b-int8", 8120): ({"mc_attn_scores_bfloat", "mc_attn_pv_bfloat", "mc_gemv_i8_bfloat_ling4_p3_e1"}, set(QKV_WO) | {"mc_attn_fused_bfloat", "mc_attn_fused_t2_bfloat"}),
}


@pytest.mark.parametrize("shape,S", list(PARTIAL_RANGE_FORMS))
def test_contexts_of_partial_ranges_against_the_oracle_and_the_form_they_take(acc, shape, S):
    import metalchat_amd as mc

    cfg, weights, fmt, bounds = _shape_cfg(shape, S)
    want, never, *whole = PARTIAL_RANGE_FORMS[shape, S]
    if not whole:
        names = set()
        agree = run_injected(acc, cfg, weights, S - 5, 12, fmt, what=f"{shape} S={S}", launched=names, **bounds)
        assert agree >= 10
    else:
        out = {}
        for cap in (S, whole[0]):
            dec = mc.Decoder(acc, **mg.decoder_kwargs(dict(cfg, max_seq_len=cap), **fmt))
            dec.init_synthetic(SEED)
            dec.set_taps(True)
            dec.launch_log(True)
            k, v = random_cache(cfg, S - 5, 100)
            dec.import_kv(0, k, v)
            tok, rows = 7, []
            for pos in range(S - 5, S):
                tok = dec.step(tok, pos)
                rows.append((tok, dec.logits().copy(), dec.hidden(0).copy(), dec.export_kv(0)))
            out[cap] = (rows, set(dec.launched()))
            dec.release()
        names = out[S][1]
        assert out[whole[0]][1] == names, (sorted(names), sorted(out[whole[0]][1]))
        for i, ((ta, la, ha, (ka, va)), (tb, lb, hb, (kb, vb))) in enumerate(zip(out[S][0], out[whole[0]][0])):
            assert ta == tb, i
            parity.exact(ha, hb, f"{shape} kv_len {S - 4 + i}: hidden[0], S = {S} vs {whole[0]}")
            parity.exact(la, lb, f"{shape} kv_len {S - 4 + i}: logits")
            parity.exact(ka, kb, f"{shape} kv_len {S - 4 + i}: K cache")
            parity.exact(va, vb, f"{shape} kv_len {S - 4 + i}: V cache")
    assert want <= names, sorted(names)
    assert not [n for n in names if n.startswith(tuple(never))], sorted(names)
