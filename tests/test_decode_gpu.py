"""Parity of the fused HIP decode pipeline (C ABI part 2) against the CPU oracle, token by token:
hidden row after every layer, logits, greedy token, and the logical KV-cache view (bit-exact:
SURVEY.md A7).  Sizes are small so the oracle finishes in seconds; both dtypes, all weight
formats, llama3 and gemma3, and runs that go past max_seq_len to exercise the sink-cache ring
against the oracle's literal "copy prefix + roll + write" (include/metalchat/nn/cache.h:187-204)."""
import numpy as np
import pytest

import modelgen as mg
import parity
from oracle import mc_oracle as mo

pytestmark = pytest.mark.gpu

BF16, F32 = 0, 1


def run_pair(acc, cfg, weights, n_steps, dec_over, rel_hidden, rel_logits, first_token=3,
             max_frac=None, max_ulp=2):
    import metalchat_amd as mc

    om = mo.Model(cfg, weights)
    dec = mc.Decoder(acc, **mg.decoder_kwargs(cfg, **dec_over))
    dec.load_model(weights)
    dec.set_taps(True)
    dt = cfg["dtype"]
    if max_frac is None:
        # compositions in bf16: an upstream one-step difference perturbs every downstream value a
        # little, so many elements may land on the neighbouring bf16 value; what is bounded is HOW
        # FAR (scaled ulps) and the vector-wise error, see tests/parity.py
        max_frac = 0.5 if dt == BF16 else 1.0
    tok = first_token
    agree = 0
    stats = []
    for pos in range(n_steps):
        otok, ologits = om.step(tok, pos)
        gtok = dec.step(tok, pos)
        for layer in range(-1, cfg["n_layers"]):
            r = parity.check(dt, dec.hidden(layer), om.hidden(layer), rel=rel_hidden,
                             max_ulp=max_ulp if layer >= 0 else 0, max_frac=max_frac if layer >= 0 else 0.0,
                             what=f"pos {pos} hidden[{layer}]")
            stats.append(r)
        parity.check(dt, dec.logits(), ologits, rel=rel_logits, max_ulp=max_ulp, max_frac=max_frac,
                     what=f"pos {pos} logits")
        # KV cache: the new row is computed (rope of a GEMV output) so it carries the T tolerance;
        # rows written by earlier steps must not move at all once written -> compare whole view
        for layer in (0, cfg["n_layers"] - 1):
            gk, gv = dec.export_kv(layer)
            ok, ov = om.kv(layer)
            assert gk.shape == ok.shape and gv.shape == ov.shape, f"pos {pos} kv shape"
            parity.check(dt, gk, ok, rel=rel_hidden, max_ulp=max_ulp, max_frac=max_frac, what=f"pos {pos} K[{layer}]")
            parity.check(dt, gv, ov, rel=rel_hidden, max_ulp=max_ulp, max_frac=max_frac, what=f"pos {pos} V[{layer}]")
        agree += int(gtok == otok)
        tok = otok  # teacher-force the oracle's token so both sides see the same inputs
    dec.release()
    om.close()
    return agree, stats


@pytest.mark.parametrize("quant,fmt,group", [(None, 0, 0), ("i8", 1, 32), ("i4", 2, 32), ("i4", 2, 128)])
def test_llama_f32_matches_oracle(acc, quant, fmt, group):
    cfg = mg.tiny_cfg(F32, max_seq_len=32)
    weights = mg.make_model(cfg, seed=11, quant=quant, group=group or 32)
    agree, _ = run_pair(acc, cfg, weights, 12, dict(weight_format=fmt, group_size=group),
                        rel_hidden=1e-4, rel_logits=1e-4)
    assert agree == 12


@pytest.mark.parametrize("quant,fmt,group", [(None, 0, 0), ("i8", 1, 32), ("i4", 2, 32), ("i4", 2, 128)])
def test_llama_bf16_matches_oracle(acc, quant, fmt, group):
    cfg = mg.tiny_cfg(BF16, max_seq_len=32)
    weights = mg.make_model(cfg, seed=12, quant=quant, group=group or 32)
    agree, _ = run_pair(acc, cfg, weights, 12, dict(weight_format=fmt, group_size=group),
                        rel_hidden=2e-3, rel_logits=2e-3)
    assert agree >= 11  # a bf16 near-tie in the logits may flip one greedy pick


@pytest.mark.parametrize("dt", [F32, BF16])
def test_sink_cache_ring_past_max_seq_len(acc, dt):
    # max_seq_len 16 -> pre_len = bit_width(16) - 1 = 4; 40 steps = 24 rolls
    cfg = mg.tiny_cfg(dt, max_seq_len=16, n_layers=1)
    weights = mg.make_model(cfg, seed=13, quant="i4", group=32)
    # 40 chained tokens: in bf16 the one-step differences of every earlier token sit in the cache,
    # so the vector-wise bound is wider than for a fresh context
    rel = 1e-4 if dt == F32 else 5e-3
    agree, _ = run_pair(acc, cfg, weights, 40, dict(weight_format=2, group_size=32),
                        rel_hidden=rel, rel_logits=rel)
    assert agree >= 38


def test_decoder_config_validation_of_the_cache_length(acc):
    # decoder.cc mc_decoder_create: max_seq_len a positive multiple of 8, a sink prefix shorter than the cache
    import metalchat_amd as mc

    for S in (2044, 0):
        with pytest.raises(mc.McError, match="max_seq_len must be a multiple of 8"):
            mc.Decoder(acc, **mg.decoder_kwargs(mg.tiny_cfg(BF16, max_seq_len=S, n_layers=1)))
    for pre in (16, 17):
        with pytest.raises(mc.McError, match="sink prefix must be shorter than the cache"):
            mc.Decoder(acc, **mg.decoder_kwargs(mg.tiny_cfg(BF16, max_seq_len=16, n_layers=1, sink_pre_len=pre)))
    # the smallest legal cache (8 slots, pre_len = bit_width(8) - 1 = 3: one range of 64 slots holding 8) decodes past its end against the oracle
    cfg = mg.tiny_cfg(BF16, max_seq_len=8, n_layers=1)
    weights = mg.make_model(cfg, seed=19, quant="i4", group=32)
    agree, _ = run_pair(acc, cfg, weights, 20, dict(weight_format=2, group_size=32), rel_hidden=5e-3, rel_logits=5e-3)
    assert agree >= 18


@pytest.mark.parametrize("dt,ranges", [(F32, 3), (BF16, 3), (BF16, 8)])
def test_pv_context_ranges(acc, dt, ranges, monkeypatch):
    # long contexts split P.V over ranges of cache slots (fp32 partials + one reduce launch);
    # forced here on a short cache: 96 slots = 3 (6 for float) MFMA k-steps over 3 / 8 ranges --
    # ranges past kv_len contribute zeros -- and run past max_seq_len so the ring turns as well
    monkeypatch.setenv("MC_PV_RANGES", str(ranges))
    cfg = mg.tiny_cfg(dt, max_seq_len=96, n_layers=1)
    weights = mg.make_model(cfg, seed=17, quant="i4", group=32)
    rel = 1e-4 if dt == F32 else 5e-3
    agree, _ = run_pair(acc, cfg, weights, 100, dict(weight_format=2, group_size=32),
                        rel_hidden=rel, rel_logits=rel)
    assert agree >= 97


def test_quantised_embedding_and_per_row_head(acc):
    # quantization::lora_embedding + quantization::linear (per-row scale) for the output head
    cfg = mg.tiny_cfg(F32)
    weights = mg.make_model(cfg, seed=14, quant="i4", group=32, emb_quant=True, head_quant="i8row")
    agree, _ = run_pair(acc, cfg, weights, 6, dict(weight_format=2, group_size=32),
                        rel_hidden=1e-4, rel_logits=1e-4)
    assert agree == 6


@pytest.mark.parametrize("dt,only", [(F32, None), (BF16, None), (F32, ("wk", "w3"))])
def test_qlora_adaptors_match_oracle(acc, dt, only):
    # quantization::lora_linear with its adaptor: T(T(x Wd^T) + T(T(B(A x)) * scale)), scale 2.0,
    # on every projection (or only on one member of each fused group: the others must see + 0)
    cfg = mg.tiny_cfg(dt, max_seq_len=32)
    weights = mg.make_model(cfg, seed=31, quant="i4", group=32, lora_rank=16, lora_only=only)
    rel = 1e-4 if dt == F32 else 2e-3
    agree, _ = run_pair(acc, cfg, weights, 10, dict(weight_format=2, group_size=32),
                        rel_hidden=rel, rel_logits=rel)
    assert agree >= (10 if dt == F32 else 9)


def test_lora_argument_validation(acc):
    import metalchat_amd as mc

    cfg = mg.tiny_cfg(F32, n_layers=1)
    dec = mc.Decoder(acc, **mg.decoder_kwargs(cfg, weight_format=2, group_size=32))
    a = np.zeros((16, cfg["dim"]), np.float32)
    b = np.zeros((cfg["dim"], 16), np.float32)
    dec.load_lora(0, "wo", a, b, 2.0)
    with pytest.raises(mc.McError, match="shape mismatch"):
        dec.load_lora(0, "w2", a, b, 2.0)                       # w2 is [dim, ffn]
    with pytest.raises(mc.McError, match="multiple of 8"):
        dec.load_lora(0, "wo", a[:12], b[:, :12], 2.0)
    kq = np.zeros((cfg["n_kv_heads"] * cfg["head_dim"], 16), np.float32)
    dec.load_lora(0, "wk", a, kq, 2.0)
    with pytest.raises(mc.McError, match="share rank and scale"):
        dec.load_lora(0, "wv", a, kq, 1.0)
    dec.release()


@pytest.mark.parametrize("dt", [F32, BF16])
def test_gemma3_matches_oracle(acc, dt):
    cfg = mg.tiny_cfg(dt, family=1, n_layers=3, rope_sliding_theta=10000.0, sliding_stride=2,
                      attn_scale=float(1.0 / np.sqrt(48.0)))
    weights = mg.make_model(cfg, seed=15, quant="i4", group=32)
    rel = 1e-4 if dt == F32 else 3e-3
    agree, _ = run_pair(acc, cfg, weights, 8, dict(weight_format=2, group_size=32),
                        rel_hidden=rel, rel_logits=rel)
    assert agree >= 7


@pytest.mark.parametrize("dt", [F32, BF16])
def test_gemma3_fused_post_norms_without_taps(acc, dt, monkeypatch):
    # without parity taps the gemma3 block runs 7 launches: both post-norms are applied inside the
    # prologue of the GEMV that consumes them (gemv.h PRO 2).  Logits and tokens against the
    # oracle, one decoder and a two-stage split, eager and chained through the captured graph.
    import metalchat_amd as mc

    cfg = mg.tiny_cfg(dt, family=1, n_layers=4, rope_sliding_theta=10000.0, sliding_stride=2,
                      attn_scale=float(1.0 / np.sqrt(48.0)))
    weights = mg.make_model(cfg, seed=18, quant="i4", group=32)
    # T = float shows the fused arithmetic is the reference's (1e-4).  bf16, four gemma blocks
    # with four norms each: the vector-wise bound is the one of the chained llama runs (5e-3) and the
    # share of elements that land on the neighbouring bf16 value is larger than for llama (the bound
    # on HOW FAR stays 2 scaled steps)
    rel = 1e-4 if dt == F32 else 5e-3
    frac = 1.0 if dt == F32 else 0.7
    om = mo.Model(cfg, weights)
    kw = dict(weight_format=2, group_size=32)
    one = mc.Decoder(acc, **mg.decoder_kwargs(cfg, **kw))
    s0 = mc.Decoder(acc, **mg.decoder_kwargs(cfg, layer_begin=0, layer_end=2, **kw))
    s1 = mc.Decoder(acc, **mg.decoder_kwargs(cfg, layer_begin=2, layer_end=4, **kw))
    for d in (one, s0, s1):
        d.load_model(weights)
    tok, seq = 3, []
    for pos in range(8):
        otok, ologits = om.step(tok, pos)
        got = one.step(tok, pos)
        parity.check(dt, one.logits(), ologits, rel=rel, max_ulp=2, max_frac=frac, what=f"fused gemma pos {pos}")
        s0.step(tok, pos, sync=False)
        acc.wait()
        got2 = s1.step(-1, pos, hidden_in=s0.hidden_out_ptr())
        parity.check(dt, s1.logits(), ologits, rel=rel, max_ulp=2, max_frac=frac, what=f"fused gemma 2-stage pos {pos}")
        assert got2 == got
        seq.append(got)
        tok = otok
    om.close()
    # the same tokens when the steps are chained on the device (teacher forcing used the oracle's
    # tokens above, so replay the decoder's own chain)
    ref = mc.Decoder(acc, **mg.decoder_kwargs(cfg, **kw))
    ref.load_model(weights)
    monkeypatch.setenv("MC_GEMMA_UNFUSED", "1")
    unf = mc.Decoder(acc, **mg.decoder_kwargs(cfg, use_graph=1, **kw))
    monkeypatch.delenv("MC_GEMMA_UNFUSED")
    unf.load_model(weights)
    g = mc.Decoder(acc, **mg.decoder_kwargs(cfg, use_graph=1, **kw))
    g.load_model(weights)
    chain = list(g.generate(3, 0, 8))
    t, stepped = 3, []
    for pos in range(8):
        t = ref.step(t, pos)
        stepped.append(t)
    assert chain == stepped
    if dt == F32:
        assert list(unf.generate(3, 0, 8)) == chain   # fused and unfused agree on the tokens
    for d in (one, s0, s1, ref, unf, g):
        d.release()


def test_head_dim_128_gqa4(acc):
    # Llama-3-8B head geometry (hd 128, 4 query heads per kv head) at reduced width
    cfg = mg.tiny_cfg(BF16, dim=512, n_heads=4, n_kv_heads=1, head_dim=128, ffn_dim=1024,
                      max_seq_len=64, n_layers=1)
    weights = mg.make_model(cfg, seed=16, quant="i4", group=128)
    agree, _ = run_pair(acc, cfg, weights, 10, dict(weight_format=2, group_size=128),
                        rel_hidden=2e-3, rel_logits=2e-3)
    assert agree >= 9


def test_generate_chained_equals_stepwise(acc):
    """Device-side token feedback (mc_decoder_generate, with and without hipGraph replay) produces
    exactly the tokens of host-driven stepping: bit-exact integer path."""
    import metalchat_amd as mc

    cfg = mg.tiny_cfg(BF16, max_seq_len=32)
    weights = mg.make_model(cfg, seed=17, quant="i4", group=32)
    outs = []
    for graph in (0, 1):
        dec = mc.Decoder(acc, **mg.decoder_kwargs(cfg, weight_format=2, group_size=32, use_graph=graph))
        dec.load_model(weights)
        toks = dec.generate(5, 0, 40)  # runs past max_seq_len
        outs.append(toks)
        dec.release()
    dec = mc.Decoder(acc, **mg.decoder_kwargs(cfg, weight_format=2, group_size=32))
    dec.load_model(weights)
    tok, step = 5, []
    for pos in range(40):
        tok = dec.step(tok, pos)
        step.append(tok)
    dec.release()
    parity.exact(outs[0], np.array(step, np.int32), "generate vs step")
    parity.exact(outs[1], np.array(step, np.int32), "graph generate vs step")


def test_fast_qmode_error_is_reported(acc):
    """MC_QMODE_FAST skips the per-weight rounding of Wd to bf16; it is NOT bit-faithful to the
    reference and is only required to stay within a looser, stated bound."""
    cfg = mg.tiny_cfg(BF16, max_seq_len=32)
    weights = mg.make_model(cfg, seed=18, quant="i4", group=32)
    agree, _ = run_pair(acc, cfg, weights, 6, dict(weight_format=2, group_size=32, qmode=1),
                        rel_hidden=1e-2, rel_logits=1e-2, max_frac=0.9, max_ulp=4)
    assert agree >= 5


def test_a_captured_token_survives_a_moved_rope_window_and_a_new_conversation(acc):
    # the rope table holds 2 * max_seq_len rows and is regenerated when the position leaves it
    # (nn/embedding.h:190-198).  A hipGraph captured under one window start must not replay a stale
    # start: generate far past the window, then start a new conversation at position 0 on the SAME
    # decoder -- tokens must equal a fresh decoder's.  Toggling the parity taps in between must not
    # replay a graph captured with another launch sequence either.
    import metalchat_amd as mc

    cfg = mg.tiny_cfg(BF16, max_seq_len=16, n_layers=2)
    weights = mg.make_model(cfg, seed=5, quant="i4", group=32)

    def fresh():
        d = mc.Decoder(acc, **mg.decoder_kwargs(cfg, weight_format=mc.WFMT_I4, group_size=32, use_graph=1))
        d.load_model(weights)
        return d

    ref = fresh()
    want_long = list(ref.generate(3, 0, 80))      # window starts: 0, 32, 64
    want_short = list(fresh().generate(9, 0, 12))
    d = fresh()
    assert list(d.generate(3, 0, 80)) == want_long
    assert list(d.generate(9, 0, 12)) == want_short          # graph captured at window 64 replayed at window 0
    d.set_taps(True)
    assert list(d.generate(9, 0, 12)) == want_short          # taps on: the captured sequence is dropped
    d.set_taps(False)
    assert list(d.generate(3, 0, 80)) == want_long
    eager = mc.Decoder(acc, **mg.decoder_kwargs(cfg, weight_format=mc.WFMT_I4, group_size=32, use_graph=0))
    eager.load_model(weights)
    assert list(eager.generate(3, 0, 80)) == want_long
    with pytest.raises(mc.McError):
        d.step(cfg["vocab"], 0)                               # token id outside the vocabulary
    for x in (ref, d, eager):
        x.release()
