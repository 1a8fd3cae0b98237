"""Records tests/golden/decode_token_plans.json -- the launch logs of one token and of a short chained call, per case -- from a built checkout
of the commit in front of csrc/token_plan.h, through the launch_log / launched() API alone (no source patch; tools/experiments/README.md):

    python tools/experiments/token_plan_record.py <built checkout> <commit> <golden>                    (on the MI355X)

Per case: the kernel names of step(1, 0), step(-1, 1) and generate(3, 0, 4) on a fresh decoder, the tokens of the generate and a SHA-256 of logits()
behind it.  Every case is recorded twice, on two decoders; a hash that differs between the two is left out and the case says so.  A stage that is not
both first and last cannot generate: its case holds the two steps only (a later stage's inbound row is its own zeroed hidden_in).

Cases whose `recorded_under` is not empty were recorded with those switches ADDED to the case's own: the decoders of the gemma3 dim-2048 shape whose
greedy head sits behind a folded post-norm.  There the recorded commit deferred a pick that its head never made ("The token plan"), so its
default sequence is not a reference for anything; its MC_LAZY_PICK=0 sequence is what the plan yields for the case's own switches."""
import json
import os
import sys

TREE, COMMIT, OUT = os.path.abspath(sys.argv[1]), sys.argv[2], os.path.abspath(sys.argv[3])
sys.path[:0] = [TREE, os.path.join(TREE, "tests")]
sys.path.append(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..", "tests"))  # (token_plan_observe: the recorded commit has none)

import metalchat_amd as mc  # noqa: E402
import modelgen as mg  # noqa: E402
from token_plan_observe import observe  # noqa: E402

assert mc.__file__.startswith(TREE), mc.__file__

BF16, F32 = 0, 1
SMALL = dict(n_layers=1, vocab=512, max_seq_len=64)
I4 = dict(weight_format=2, group_size=128)
LLAMA_2048 = dict(SMALL, dim=2048, n_heads=16, n_kv_heads=4, head_dim=128, ffn_dim=4096)
GEMMA = dict(SMALL, family=1, dim=2048, n_heads=8, n_kv_heads=2, head_dim=256, ffn_dim=4096, n_layers=2, rope_sliding_theta=10000.0, sliding_stride=2)
MODELS = {  # tests/test_gemv_plan_gpu.py MODELS: (dtype, cfg overrides, make_model arguments or None for init_synthetic(7), decoder arguments)
    "i4-lin": (BF16, LLAMA_2048, None, I4),
    "i4-k4": (BF16, dict(LLAMA_2048, ffn_dim=24576), None, I4),
    "i4-3072": (BF16, dict(SMALL, dim=3072, n_heads=24, n_kv_heads=8, head_dim=128, ffn_dim=4096), None, I4),
    "i4-1024": (BF16, dict(SMALL, dim=1024, n_heads=8, n_kv_heads=2, head_dim=128, ffn_dim=4096), None, I4),
    "i4-g32-lora": (BF16, dict(LLAMA_2048, ffn_dim=2048), dict(seed=91, quant="i4", group=32, lora_rank=8), dict(weight_format=2, group_size=32)),
    "i4-fast": (BF16, LLAMA_2048, None, dict(I4, qmode=1)),
    "i8": (BF16, dict(SMALL, dim=4096, n_heads=32, n_kv_heads=8, head_dim=128, ffn_dim=14336), None, dict(weight_format=1, group_size=32)),
    "bf16": (BF16, dict(SMALL, dim=2048, n_heads=32, n_kv_heads=4, head_dim=64, ffn_dim=5632), None, dict()),
    "f32": (F32, dict(), None, dict()),
    "gemma": (BF16, GEMMA, None, I4),
    "gemma-lora": (BF16, GEMMA, dict(seed=92, quant="i4", group=128, lora_rank=8, lora_only=("w1", "w3")), I4),
}
W_I4, W_I8, W_BF = dict(weight_format=2, group_size=128), dict(weight_format=1, group_size=32), dict(weight_format=0, group_size=0)
G3 = dict(family=1, rope_sliding_theta=10000.0, sliding_stride=2)
SHAPES = {  # tools/experiments/block_plan_record.py SHAPES: the BASELINE shapes, one block (gemma3: two), vocabulary 512
    "tinyllama-bf16": (dict(dim=2048, n_heads=32, n_kv_heads=4, head_dim=64, ffn_dim=5632), W_BF, 1),
    "llama32-1b-bf16": (dict(dim=2048, n_heads=32, n_kv_heads=8, head_dim=64, ffn_dim=8192), W_BF, 1),
    "llama3-8b-i4": (dict(dim=4096, n_heads=32, n_kv_heads=8, head_dim=128, ffn_dim=14336), W_I4, 1),
    "llama3-8b-i8": (dict(dim=4096, n_heads=32, n_kv_heads=8, head_dim=128, ffn_dim=14336), W_I8, 1),
    "gemma-7b-i4": (dict(dim=3072, n_heads=16, n_kv_heads=16, head_dim=256, ffn_dim=24576, **G3), W_I4, 2),
    "llama3-70b-i4": (dict(dim=8192, n_heads=64, n_kv_heads=8, head_dim=128, ffn_dim=28672), W_I4, 1),
}
CONTEXTS = (1024, 2048, 4096, 8192)
LAZY_OFF = {"MC_LAZY_PICK": "0"}


def case(cfg, weights=None, env=None, taps=False, sampler="greedy", recorded_under=None):
    cfg = dict(cfg)
    cfg.setdefault("layer_begin", 0)
    cfg.setdefault("layer_end", cfg["n_layers"])
    return dict(cfg=cfg, weights=weights, env=env or {}, taps=taps, sampler=sampler, recorded_under=recorded_under or {})


def model_cfg(name, **over):
    dt, cfg_over, make, kw = MODELS[name]
    cfg = mg.tiny_cfg(dt, **dict(cfg_over, **over))
    return mg.decoder_kwargs(cfg, **kw), (dict(make, lora_only=list(make["lora_only"])) if make and make.get("lora_only") else make)


CASES = {}
for name in MODELS:
    cfg, make = model_cfg(name)
    CASES["model:" + name] = case(cfg, make, recorded_under=LAZY_OFF if name.startswith("gemma") else None)
for name, (widths, fmt, blocks) in SHAPES.items():
    for S in CONTEXTS:
        CASES[f"device:{name}-s{S}"] = case(dict(dtype=0, n_layers=blocks, vocab=512, max_seq_len=S, rope_theta=10000.0, norm_eps=1e-5,
                                                 attn_scale=float(widths["head_dim"]) ** -0.5, use_graph=0, **widths, **fmt))
for name in ("i4-lin", "gemma"):
    g = name == "gemma"  # (its greedy head sits behind a folded post-norm wherever nothing below takes the fold or the deferred pick away)
    cfg, make = model_cfg(name)
    v = "variant:" + name + ":"
    CASES[v + "taps"] = case(cfg, make, taps=True)
    CASES[v + "gemma-unfused"] = case(cfg, make, env={"MC_GEMMA_UNFUSED": "1"})
    CASES[v + "attn-unfused"] = case(cfg, make, env={"MC_ATTN_FUSED": "0"}, recorded_under=LAZY_OFF if g else None)
    for m in "012":
        CASES[v + "head-pick" + m] = case(cfg, make, env={"MC_HEAD_PICK": m}, recorded_under=LAZY_OFF if g and m == "2" else None)
    CASES[v + "lazy-off"] = case(cfg, make, env=dict(LAZY_OFF))
    CASES[v + "sampler-greedy"] = case(cfg, make, sampler="greedy", recorded_under=LAZY_OFF if g else None)
    CASES[v + "sampler-default"] = case(cfg, make, sampler="default")
    CASES[v + "sampler-draw"] = case(cfg, make, sampler="draw")
    quant = dict(seed=7, quant="i4", group=128, emb_quant=True)
    CASES[v + "emb-i8"] = case(cfg, quant)
    cfg2, _ = model_cfg(name, n_layers=2)
    CASES[v + "stage-first"] = case(dict(cfg2, layer_begin=0, layer_end=1), make)
    CASES[v + "stage-last"] = case(dict(cfg2, layer_begin=1, layer_end=2), make)
    CASES[v + "stage-no-block"] = case(dict(cfg2, layer_begin=2, layer_end=2), make)

if __name__ == "__main__":
    acc = mc.HardwareAccelerator()
    cases = {}
    for name, c in CASES.items():
        a, b = observe(acc, c, c["recorded_under"]), observe(acc, c, c["recorded_under"])
        assert a["handoff_fallbacks"] == 0 and b["handoff_fallbacks"] == 0, name
        for k in ("step0", "step1", "generate", "tokens"):
            assert a.get(k) == b.get(k), (name, k)
        a.pop("handoff_fallbacks")
        if a.get("logits_sha256") != b.get("logits_sha256"):
            a.pop("logits_sha256")
            a["note"] = "the logits hash was not repeatable on the recorded commit itself: left out"
        cases[name] = dict(c, **a)
        print(name, len(a["step0"]), len(a.get("generate", ())), a.get("tokens"), flush=True)
    with open(OUT, "w") as f:
        f.write('{"recorded_from": %s, "device": %s, "cus": %d,\n "calls": {"step0": "step(1, 0)", "step1": "step(-1, 1)", "generate": "generate(3, 0, 4)"},\n "cases": {\n'
                % (json.dumps(COMMIT), json.dumps(acc.name()), acc.compute_units()))
        f.write(",\n".join("  %s: %s" % (json.dumps(k), json.dumps(v)) for k, v in cases.items()))
        f.write("\n}}\n")
    with open(OUT) as f:
        json.load(f)
    print("recorded", len(cases), "cases")
