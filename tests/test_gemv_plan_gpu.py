"""The decode GEMVs as launched, pinned: for the smallest models at which each family of the plan (csrc/gemv_plan.h plan_gemv:
classic, _fast, _m4, _m4d, _lin<n>, _lin12k4, _lin3s, _ling<n>) is taken, the mc_gemv_* launches of one eager token and what
gemv_kernel_name() answers are the ones recorded from the build of the commit tests/golden/decode_gemv_plans.json names -- the one in
front of plan_gemv.  An edit of the priority list shows up as a diff of kernel names, not as a timing; grid, workgroup and LDS bytes
of the same recording are pinned without a GPU by test_gemv_plan_cpu.py.  No numeric comparison: the parity suite holds every one of
these kernels to the oracle.

Every decoder here runs under MC_ATTN_FUSED=0: the whole block as launches of its own, none of which waits for another workgroup.

The golden was written by this module's `record` entry point, copied into a built checkout of that commit with
tools/experiments/gemv_plan_record.patch applied (every gemv() call appends its decision to the file MC_GEMV_PLAN_RECORD names):

    PYTHONPATH=. python tests/test_gemv_plan_gpu.py record <commit> [file]
"""
import json
import os
import re
import sys
import tempfile

import pytest

import modelgen as mg

pytestmark = pytest.mark.gpu
BF16, F32 = 0, 1
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "decode_gemv_plans.json")
WHICH = ("qkv", "wo", "w13", "w2", "head")

SMALL = dict(n_layers=1, vocab=512, max_seq_len=64)
I4 = dict(weight_format=2, group_size=128)
LLAMA_2048 = dict(SMALL, dim=2048, n_heads=16, n_kv_heads=4, head_dim=128, ffn_dim=4096)
GEMMA = dict(SMALL, family=1, dim=2048, n_heads=8, n_kv_heads=2, head_dim=256, ffn_dim=4096, n_layers=2, rope_sliding_theta=10000.0, sliding_stride=2)
MODELS = {
    # name: (dtype, cfg overrides, make_model arguments or None for init_synthetic, decoder arguments)
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

# the switches of the cases and the decoder_options fields they set (csrc/decoder_options.h read_options): what the CPU program is given
FIELDS = {
    "MC_GEMV_LIN": lambda v: {"gemv_lin": int(v)},
    "MC_GEMV_LING": lambda v: {"gemv_ling": int(v)},
    "MC_I8_LING14": lambda v: {"i8_ling14": int(v)},
    "MC_LIN_SPLIT": lambda v: {"lin_split": int(v)},
    "MC_LING_HALF": lambda v: {"ling_half": int(v)},
    "MC_LIN_K4": lambda v: {"lin_k4_on": int(v)},
    "MC_GEMV_M4": lambda v: {"gemv_m4": int(v)},
    "MC_GEMV_BLOCK": lambda v: {"gemv_block": int(v), "gemv_block_env": 1},
    "MC_GEMV_WGS_PER_CU": lambda v: {"gemv_wgs_per_cu": int(v), "gemv_block_env": 1},
    "MC_GEMV_FULLGRID": lambda v: {"gemv_full_grid": int(v)},
    "MC_GEMV_DBG": lambda v: {"dbg_variant": int(v)},
    "MC_GEMMA_UNFUSED": lambda v: {},  # (the caller's choice of prologue, not the plan's)
}


def _has(pattern):
    return lambda names: any(re.search(pattern, n) for n in names)


def _none(pattern):
    return lambda names: not [n for n in names if re.search(pattern, n)]


CLASSIC_I4 = r"^mc_gemv_i4_bfloat_m4d?_p"
# id: (model, switches, [what the step's mc_gemv_* launches must show], {matrix: what gemv_kernel_name must show})
CASES = {
    "i4-lin": ("i4-lin", {}, [_has(r"_lin1_p3_e1$")],
               dict(qkv=r"_lin1_p1_e4$", wo=r"_lin1_p3_e1$", w13=r"_lin1_p1_e2$", w2=r"_lin2_p0_e1$", head=r"_lin1_p1_e5$")),
    "i4-k4": ("i4-k4", {}, [], dict(w2=r"_lin12k4_p0_e1$")),
    "i4-k4-off": ("i4-k4", {"MC_LIN_K4": "0"}, [_none("k4")], dict(w2=r"_lin12_p0_e1$")),
    "i4-3072": ("i4-3072", {}, [], dict(qkv=r"_lin3s_p1_e4$", w13=r"_lin3s_p1_e2$", head=r"_lin3s_p1_e0$")),
    "i4-3072-nosplit": ("i4-3072", {"MC_LIN_SPLIT": "0"}, [_none("_lin3s")], dict(qkv=CLASSIC_I4, w13=CLASSIC_I4, head=CLASSIC_I4)),
    "i4-1024": ("i4-1024", {}, [], dict(w13=r"_m4d_p1_e2$", wo=r"_m4_p0_e1$")),
    "i4-g32-lora": ("i4-g32-lora", {}, [_has(r"^mc_gemv_w_bfloat_ling4_p\d_e0$"), _none(r"^mc_gemv_i4_bfloat_(?!m4_)")], dict(qkv=r"_m4_p1_e4$")),
    "i4-fast": ("i4-fast", {}, [_has("_fast_"), _none("_lin")], dict(qkv=r"_fast_p1_e4$")),
    "i8": ("i8", {}, [_has(r"^mc_gemv_i8_bfloat_ling4_"), _has(r"^mc_gemv_i8_bfloat_ling14_")], dict(w2=r"_ling14_p0_e1$")),
    "i8-noling14": ("i8", {"MC_I8_LING14": "0"}, [_has("_ling4_"), _none("_ling14_")], dict(w2=r"^mc_gemv_i8_bfloat_p0_e1$")),
    "i8-noling": ("i8", {"MC_GEMV_LING": "0"}, [_none("_ling")], dict(w2=r"^mc_gemv_i8_bfloat_p0_e1$")),
    "bf16": ("bf16", {}, [_has(r"^mc_gemv_w_bfloat_ling4_"), _has(r"^mc_gemv_w_bfloat_ling11_")], dict(w2=r"_ling11_p0_e1$")),
    "bf16-nohalf": ("bf16", {"MC_LING_HALF": "0"}, [_has(r"^mc_gemv_w_bfloat_ling4_"), _has(r"^mc_gemv_w_bfloat_ling11_")], dict(w2=r"_ling11_p0_e1$")),
    "f32": ("f32", {}, [lambda names: names and all(n.startswith("mc_gemv_w_float_p") for n in names)], dict(qkv=r"^mc_gemv_w_float_p1_e4$")),
    "gemma": ("gemma", {}, [_has(r"_lin\d+_p2_e0$"), _has(r"_lin\d+_p2_e3$")], dict()),
    "gemma-unfused": ("gemma", {"MC_GEMMA_UNFUSED": "1"}, [_has("_p1_e0$"), _has("_p1_e3$"), _has("_p0_e0$"), _none("_p2_")], dict()),
    # (w1|w3 carries an adaptor and sits behind the attention post-norm: the linear-order `_p2_` kernels have no argument slots left for both)
    "gemma-lora": ("gemma-lora", {}, [_has(CLASSIC_I4 + "2_e3$"), _none(r"_lin\d+_p2_e3$")], dict()),
}
# tuning switches on i4-lin: asked through gemv_kernel_name only -- these builds' kernels need not exist, nothing is launched under them
NAME_ONLY = {f"i4-lin-{k[3:].lower()}{v}": ("i4-lin", {k: v}) for k, v in (
    ("MC_GEMV_LIN", "0"), ("MC_GEMV_M4", "0"), ("MC_GEMV_M4", "1"), ("MC_GEMV_M4", "3"), ("MC_GEMV_BLOCK", "512"), ("MC_GEMV_WGS_PER_CU", "4"),
    ("MC_GEMV_FULLGRID", "1"), ("MC_GEMV_DBG", "1"))}

# gemma3 with the post-norms folded in: the token launches w1|w3 and the head behind a post-norm (`_p2_`, no pick), mc_decoder_time_gemv -- and so
# gemv_kernel_name -- behind the plain norm (`_p1_`), as it always has: those two names are pinned by the golden only
BEHIND_POST_NORM = {"gemma": ("w13", "head"), "gemma-lora": ("w13", "head")}
_weights = {}


def observe(acc, model, switches, step=True):
    """({matrix: gemv_kernel_name}, the mc_gemv_* launches of one eager token at position 0) of a decoder created under the switches"""
    import metalchat_amd as mc

    dt, over, make, kw = MODELS[model]
    cfg = mg.tiny_cfg(dt, **over)
    saved = {k: os.environ.get(k) for k in switches}
    os.environ.update(switches)
    try:
        dec = mc.Decoder(acc, **mg.decoder_kwargs(cfg, **kw))
    finally:
        for k, v in saved.items():
            os.environ.pop(k) if v is None else os.environ.__setitem__(k, v)
    if make is None:
        dec.init_synthetic(7)
    else:
        if model not in _weights:
            _weights[model] = mg.make_model(cfg, **make)  # made once per session and left unchanged
        dec.load_model(_weights[model])
    which = {w: dec.gemv_kernel_name(w) for w in WHICH}
    names = []
    if step:
        dec.launch_log(True)
        dec.step(1, 0)
        names = [n for n in dec.launched() if n.startswith("mc_gemv_")]
        dec.launch_log(False)
    dec.release()
    return which, names


def check_shows(case, which, names):
    _, _, shows, named = CASES[case]
    for i, show in enumerate(shows):
        assert show(names), (case, i, names)
    for w, pattern in named.items():
        assert re.search(pattern, which[w]), (case, w, which[w])


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.mark.parametrize("case", sorted(CASES))
def test_decode_gemv_launches_are_the_recorded_ones(acc, golden, case):
    if golden["cus"] != acc.compute_units():
        pytest.skip(f"the golden was recorded on {golden['cus']} compute units, this device has {acc.compute_units()}: the grids, and with them _m4 / _m4d / k4, differ")
    model, switches = CASES[case][:2]
    which, names = observe(acc, model, dict(switches, MC_ATTN_FUSED="0"))
    print(case, which, names)
    check_shows(case, which, names)
    g = golden["cases"][case]
    assert names == g["step"], (case, "recorded from", golden["recorded_from"])
    assert which == g["which"], (case, "recorded from", golden["recorded_from"])
    # what the decoder names is what the token launched, matrix by matrix
    for w in WHICH:
        if w not in BEHIND_POST_NORM.get(case, ()):
            assert which[w] in names, (case, w, which[w])


def record(commit, path=GOLDEN):
    import metalchat_amd as mc

    acc = mc.HardwareAccelerator()
    fd, log = tempfile.mkstemp(suffix=".gemv_plans")
    os.close(fd)
    os.environ["MC_GEMV_PLAN_RECORD"] = log

    def recorded():
        with open(log) as f:
            lines = f.read().split("\n")
        open(log, "w").close()
        plans = []
        for line in lines:
            t = line.split()
            if t and t not in plans:
                plans.append(t)
        return [[int(x) for x in t[:10]] + [t[10]] + [int(x) for x in t[11:]] for t in plans]

    def options(switches):
        o = {}
        for k, v in switches.items():
            o.update(FIELDS[k](v))
        return o

    cases = {}
    for case in sorted(CASES):
        model, switches = CASES[case][:2]
        observe(acc, model, switches)  # the one-launch attention blocks: their GEMVs, and every name, on the record too
        which, names = observe(acc, model, dict(switches, MC_ATTN_FUSED="0"))
        check_shows(case, which, names)
        cases[case] = dict(model=model, switches=switches, options=options(switches), plans=recorded(), step=names, which=which)
    for case, (model, switches) in sorted(NAME_ONLY.items()):
        observe(acc, model, switches, step=False)
        which, _ = observe(acc, model, dict(switches, MC_ATTN_FUSED="0"), step=False)
        cases[case] = dict(model=model, switches=switches, options=options(switches), plans=recorded(), which=which)
    os.remove(log)
    with open(path, "w") as f:
        f.write('{"recorded_from": %s, "device": %s, "cus": %d,\n' % (json.dumps(commit), json.dumps(acc.name()), acc.compute_units()))
        f.write(' "plan_fields": ["fmt", "out", "in", "group", "lora_cols", "pro", "epi", "tb", "qmode", "cus", "name", "wgs", "block", "lds"],\n "cases": {\n')
        for i, (case, c) in enumerate(sorted(cases.items())):
            plans = c.pop("plans")
            f.write(' %s: {%s,\n  "plans": [\n%s]}%s\n' % (json.dumps(case), json.dumps(c)[1:-1], ",\n".join("   " + json.dumps(p) for p in plans),
                                                      "," if i + 1 < len(cases) else ""))
        f.write("}}\n")
    with open(path) as f:
        json.load(f)


if __name__ == "__main__":
    assert len(sys.argv) in (3, 4) and sys.argv[1] == "record", __doc__
    record(*sys.argv[2:])
