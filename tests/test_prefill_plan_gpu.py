"""The ordered launch log of the prompt pass, pinned for the smallest shapes at which each arm of the prompt GEMM plan
(prefill.cc plan_gemm) and each form of a run_prefill step is taken: an edit of the ladder shows up as a diff of kernel names,
not as a timing.  The expected sequences are data (tests/golden/prompt_launch_logs.json), recorded on the MI355X from the build
of the commit the file names -- the one in front of plan_gemm -- with this module's `record` entry point:

    PYTHONPATH=. python tests/test_prefill_plan_gpu.py record <commit> [file]      (this module copied into a built checkout of that commit)

Every case also names the kernels it is there for, so that a changed default fails here and does not just pin something else.
The library GEMM is left out (it needs a process without torch: test_prefill_gpu.py test_library_gemm_*)."""
import json
import os
import sys

import numpy as np
import pytest

import modelgen as mg
from oracle import mc_oracle as mo

pytestmark = pytest.mark.gpu
BF16, F32 = 0, 1
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "prompt_launch_logs.json")

# two blocks: the hand-over of the next block's norm (pf_xn) and the last block's arm both run
WIDE = dict(dim=1024, n_heads=8, n_kv_heads=2, head_dim=128, ffn_dim=2048, n_layers=2, vocab=512, max_seq_len=320)
GEMMA = dict(family=1, dim=2048, n_heads=8, n_kv_heads=2, head_dim=128, ffn_dim=1024, n_layers=2, vocab=512, max_seq_len=448,
             rope_sliding_theta=10000.0, sliding_stride=2)
MODELS = {
    # name: (dtype, cfg overrides, make_model arguments, decoder arguments)
    "i4": (BF16, WIDE, dict(seed=83, quant="i4", group=128), dict(weight_format=2, group_size=128)),
    "i4_lora": (BF16, WIDE, dict(seed=81, quant="i4", group=128, lora_rank=8), dict(weight_format=2, group_size=128)),
    "i8": (BF16, WIDE, dict(seed=84, quant="i8", group=32), dict(weight_format=1, group_size=32)),
    "bf16": (BF16, WIDE, dict(seed=85), dict()),
    "f32": (F32, dict(max_seq_len=32), dict(seed=86), dict()),
    "gemma": (BF16, GEMMA, dict(seed=171, quant="i4", group=128), dict(weight_format=2, group_size=128)),
}
PARTS = ("mc_pf_rope_cache_parts_", "mc_pf_act_mul_parts_", "mc_pf_rmsnorm_parts_", "mc_pf_rmsnorm2_parts_")
REDUCE = "mc_pf_splitk_reduce_bfloat"


def _has(prefix):
    return lambda names: any(n.startswith(prefix) for n in names)


def _none(*prefixes):
    return lambda names: not [n for n in names if n.startswith(prefixes)]


def _folded(names):
    # (one reduce stays: the last block's w2 has no next norm to fold into)
    return _has(PARTS)(names) and names.count(REDUCE) == 1


def _unfolded(names):
    return REDUCE in names and not [n for n in names if "_parts_" in n]


# id: (model, what runs, rows, switches, [what the log must show])
CASES = {}
for fold, shape in (("1", _folded), ("0", _unfolded)):
    CASES[f"i4-33-stream-fold{fold}"] = ("i4", "prompt", 33, {"MC_PF_FOLD": fold}, [_has("mc_pf2_gemm_i4_bfloat"), _none("mc_pf_gemm"), shape])
    CASES[f"i4-70-tiled128-fold{fold}"] = ("i4", "prompt", 70, {"MC_PF_FOLD": fold},
                                          [_has("mc_pf_gemm128_i4_bfloat_d2_e2"), _none("mc_pf2_gemm", "mc_pf_gemm8_", "mc_pf_gemm256_"), shape])
    CASES[f"i4-300-g8-fold{fold}"] = ("i4", "prompt", 300, {"MC_PF_FOLD": fold}, [_has("mc_pf_gemm8_"), _none("mc_pf2_gemm", "mc_pf_gemm128_", "mc_pf_gemm256_")])
    CASES[f"i4-300-tiled256-fold{fold}"] = ("i4", "prompt", 300, {"MC_PF_FOLD": fold, "MC_PF_GEMM8": "0"},
                                           [_has("mc_pf_gemm256_i4_bfloat_d2_"), _none("mc_pf2_gemm", "mc_pf_gemm8_")])
# an adaptor on every matrix: the reduce carries it, the fold is refused
CASES["lora-33-stream"] = ("i4_lora", "prompt", 33, {}, [_has("mc_pf2_gemm_i4_bfloat"), _unfolded])
CASES["lora-70-tiled128"] = ("i4_lora", "prompt", 70, {}, [_has("mc_pf_gemm128_i4_bfloat_d2_e2"), _unfolded])
CASES["i8-70-tiled128"] = ("i8", "prompt", 70, {}, [_has("mc_pf_gemm128_i8_bfloat_d2_"), _none("mc_pf2_gemm", "mc_pf_gemm8_")])
CASES["bf16-70-tiled128"] = ("bf16", "prompt", 70, {}, [_has("mc_pf_gemm128_w_bfloat_d2_"), _none("mc_pf2_gemm", "mc_pf_gemm8_")])
CASES["f32-21-tile64"] = ("f32", "prompt", 21, {}, [_has("mc_pf_gemm_w_float_e"), _none("mc_pf_gemm128_", "mc_pf_gemm256_", "mc_pf_gemm8_", "mc_pf2_"),
                                                     lambda names: not [n for n in names if "_parts_" in n]])
CASES["gemma-400-norm2-1"] = ("gemma", "prompt", 400, {"MC_PF_NORM2": "1"}, [lambda names: names.count("mc_pf_rmsnorm2_parts_bfloat") == 4])
CASES["gemma-400-norm2-0"] = ("gemma", "prompt", 400, {"MC_PF_NORM2": "0"}, [_none("mc_pf_rmsnorm2_parts_"), lambda names: REDUCE in names])
# two batch rows, 5 and 33 tokens: the packed forms of the rope + cache write and of the attention
CASES["i4-rows-prefill"] = ("i4", "prefill_rows", (5, 33), {}, [_has("mc_pp_rope_cache_"), _has("mc_pp_attn"), _has("mc_pf2_gemm_i4_bfloat")])
CASES["i4-rows-extend"] = ("i4", "extend_rows", (5, 33), {}, [_has("mc_pp_rope_cache_"), _has("mc_px_sums"), _has("mc_px_pv"), _has("mc_pf2_gemm_i4_bfloat")])
EXTEND_BEHIND = 40  # keys in front of each extend_rows chunk

_models = {}


def model(name):
    """(cfg, weights) of a model, made once per session and left unchanged"""
    if name not in _models:
        dt, over, make, _ = MODELS[name]
        cfg = mg.tiny_cfg(dt, **over)
        _models[name] = (cfg, mg.make_model(cfg, **make))
    return _models[name]


def launch_log(acc, case):
    """the launches of the case's one call, in order, from a decoder created under the case's switches"""
    import metalchat_amd as mc

    name, what, n, env, _ = CASES[case]
    cfg, weights = model(name)
    saved = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        dec = mc.Decoder(acc, **mg.decoder_kwargs(cfg, **MODELS[name][3]))
    finally:
        for k, v in saved.items():
            os.environ.pop(k) if v is None else os.environ.__setitem__(k, v)
    dec.load_model(weights)
    rng = np.random.default_rng(len(case))
    if what == "prompt":
        tokens = rng.integers(0, cfg["vocab"], n).tolist()
        dec.launch_log(True)
        dec.prefill(tokens, 0)
        names = dec.launched()
    else:
        batch = mc.Batch(dec, len(n))
        prompts = [rng.integers(0, cfg["vocab"], k).astype(np.int32) for k in n]
        if what == "extend_rows":
            shape = (EXTEND_BEHIND, cfg["n_kv_heads"], cfg["head_dim"])
            for r in range(len(n)):
                for layer in range(cfg["n_layers"]):
                    k, v = (mo.encode(cfg["dtype"], rng.normal(0, 0.4, shape).astype(np.float32)) for _ in range(2))
                    batch.import_kv(r, layer, k, v)
            dec.launch_log(True)
            batch.extend_rows(prompts, [EXTEND_BEHIND] * len(n))
        else:
            dec.launch_log(True)
            batch.prefill_rows(prompts)
        names = dec.launched()
        batch.release()
    dec.launch_log(False)
    dec.release()
    return names


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.mark.parametrize("case", sorted(CASES))
def test_prompt_launch_log_is_the_recorded_one(acc, golden, case):
    names = launch_log(acc, case)
    print(case, names)
    for i, shows in enumerate(CASES[case][4]):
        assert shows(names), (case, i, names)
    assert names == golden["cases"][case], (case, "recorded from", golden["recorded_from"])


def record(commit, path=GOLDEN):
    import metalchat_amd as mc

    acc = mc.HardwareAccelerator()
    cases = {case: launch_log(acc, case) for case in sorted(CASES)}
    for case, names in cases.items():
        for i, shows in enumerate(CASES[case][4]):
            assert shows(names), (case, i, names)
    with open(path, "w") as f:
        json.dump({"recorded_from": commit, "device": acc.name(), "cases": cases}, f, indent=0)
        f.write("\n")


if __name__ == "__main__":
    assert len(sys.argv) in (3, 4) and sys.argv[1] == "record", __doc__
    record(*sys.argv[2:])
