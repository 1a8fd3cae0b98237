"""What the prompt pass launches, pinned without a GPU: csrc/prefill_plan.h (plan_gemm, plan_attention and its packed / extend forms, plan_rope, the
fold predicates) is pure integer arithmetic, so tests/cpp/test_prefill_plan -- a plain g++ program over that header -- is asked

  * every decision recorded in tests/golden/prompt_plans.json and has to give the recorded answer in every field: family, kernel name, grid, K
    splits, workgroup, `ktper` and row tile of a GEMM; name, grid and workgroup of an attention or rope launch.  The recording is of the commit
    the file names, the one in front of prefill_plan.h, on the device it names (tools/experiments/prefill_plan_record.patch): the launches of every
    case of test_prefill_plan_gpu.py as they were made, and that commit's plan_gemm / plan_attention members asked directly at the shapes of
    Llama-3-8B, Gemma-7B, Llama-3.2-1B and TinyLlama on both sides of every threshold;
  * the cases of tests/golden/prompt_launch_logs.json (recorded from b696922, in front of plan_gemm itself): the family it plans for each of a
    block's linears is the family of the GEMM names in that log, and the attention and rope names it plans are the logged ones.

What this cannot cover: the arguments of a launch, the order of the launches (test_prefill_plan_gpu.py pins the names in order on the device) and
whatever touches the device -- the dequantised copies (plain_copy_ok), the library GEMM's own success."""
import json
import os
import re
import subprocess

import pytest

import pf_attn_rule
import test_prefill_plan_gpu as cases
from metalchat_amd import build as b

HERE = os.path.dirname(os.path.abspath(__file__))
with open(os.path.join(HERE, "golden", "prompt_plans.json")) as f:
    G = json.load(f)
with open(os.path.join(HERE, "golden", "prompt_launch_logs.json")) as f:
    LOGS = json.load(f)["cases"]
assert G["env_fields"] == ["tb", "qmode", "family", "cus", "dim", "ffn_dim", "n_heads", "n_kv_heads", "head_dim", "max_seq_len", "lib_on"]
assert G["record_fields"][:5] == ["kind", "env (index)", "options (index)", "args", "answer"]
SOURCES = sorted({r[5] for r in G["records"]})


def ask(lines):
    exe = b.build_prefill_plan_test()
    out = subprocess.run([exe], input="".join(line + "\n" for line in lines), capture_output=True, text=True, check=True).stdout
    answers = out.split("\n")[:-1]
    assert len(answers) == len(lines)
    return answers


def line_of(kind, env, args, options):
    return " ".join([kind, *(str(x) for x in env), *(str(x) for x in args), *(f"{k}={v}" for k, v in sorted(options.items()))])


@pytest.fixture(scope="module")
def answers():
    """the program's line for each record of the golden: one run over all of it"""
    return ask([line_of(kind, G["envs"][e], args.split(), G["options"][o]) for kind, e, o, args, _, _ in G["records"]])


@pytest.mark.parametrize("source", SOURCES)
def test_plan_is_the_recorded_one(answers, source):
    mine = [(r, a) for r, a in zip(G["records"], answers) if r[5] == source]
    assert mine
    for r, got in mine:
        assert got == r[4], (r, G["envs"][r[1]], G["options"][r[2]], "recorded from", G["recorded_from"])


def gemm_family(name):
    """the family a launched GEMM name belongs to (prefill_plan.h gemm_family)"""
    for prefix, fam in (("mc_pf2_gemm_", "stream"), ("mc_pf_gemm8_", "g8"), ("mc_pf_gemm128_", "tiled"), ("mc_pf_gemm256_", "tiled"), ("mc_pf_gemm_", "tile64"),
                        ("hipblasLtMatmul", "lib")):
        if name.startswith(prefix):
            return fam
    return None


def test_recording_covers_every_family_tile_split_and_attention_name():
    """what the recording is there for, asked of the golden itself: a re-recording that lost a family or an attention form fails here"""
    gemms = [r[4].split() for r in G["records"] if r[0] == "gemm"]
    assert {g[0] for g in gemms} == {"lib", "stream", "g8", "tiled", "tile64"}
    assert all(gemm_family(g[1]) == g[0] for g in gemms)
    tiled = [g for g in gemms if g[0] == "tiled"]
    assert {g[7] for g in tiled} == {"128", "256"}                                         # both row tiles ...
    assert {(g[7], int(g[4]) > 1) for g in tiled} == {(bm, s) for bm in ("128", "256") for s in (False, True)}   # ... split and unsplit
    assert {int(g[4]) > 1 for g in gemms if g[0] == "g8"} == {False, True} and {int(g[4]) > 1 for g in gemms if g[0] == "stream"} == {False, True}
    attn = {r[4].split()[0] for r in G["records"] if r[0] == "attn"}
    assert attn == set(pf_attn_rule.KERNELS), attn ^ set(pf_attn_rule.KERNELS)
    assert {r[4].split()[0] for r in G["records"] if r[0] == "packed"} >= {"mc_pp_attn_bfloat_hd128"}
    assert [r[4] for r in G["records"] if r[0] == "extend"] == ["mc_px_sums2_bfloat_hd128 mc_px_pv2_bfloat_hd128 mc_px_reduce_bfloat_hd128 4"]
    rope = {r[4].split()[0] for r in G["records"] if r[0] == "rope"}
    assert rope >= {"mc_pf_rope_cache_v4_bfloat", "mc_pf_rope_cache_parts_v4_bfloat", "mc_pf_rope_cache_float", "mc_pp_rope_cache_parts_bfloat"}
    # every case of test_prefill_plan_gpu.py left its launches, and lib_on was recorded both ways
    assert {s for s in SOURCES if s.startswith("launch:")} == {"launch:" + c for c in cases.CASES}
    assert {G["envs"][r[1]][10] for r in G["records"] if r[0] == "gemm"} == {0, 1}


# ---- the launch logs recorded in front of plan_gemm (b696922, 256 CUs)
SWITCH = {"MC_PF_FOLD": "pf_fold_on", "MC_PF_GEMM8": "pf_g8_on", "MC_PF_NORM2": "pf_norm2"}
WFMT = {None: 0, "i8": 1, "i4": 2}


def case_setup(case):
    """(env words, options, M, the block's linears as (fmt, out, in, group, lora_cols), packed tiles or None, extend?) of a case"""
    name, what, n, switches, _ = cases.CASES[case]
    dt, over, make, _ = cases.MODELS[name]
    cfg = cases.mg.tiny_cfg(dt, **over)
    H, KV, hd, dim, ffn = (cfg[k] for k in ("n_heads", "n_kv_heads", "head_dim", "dim", "ffn_dim"))
    env = [2 if dt == cases.BF16 else 4, 0, cfg["family"], 256, dim, ffn, H, KV, hd, cfg["max_seq_len"], 0]
    fmt, group, rank = WFMT[make.get("quant")], make.get("group", 0) if make.get("quant") else 0, make.get("lora_rank", 0)
    lin = {}
    for which, out, inn, nseg in (("qkv", (H + 2 * KV) * hd, dim, 3), ("wo", dim, H * hd, 1), ("w13", 2 * ffn, dim, 2), ("w2", dim, ffn, 1)):
        lin[which] = (fmt, out, inn, group, nseg * rank)
        if rank:
            lin[which + ".lora_a"] = (0, nseg * rank, inn, 0, 0)   # the stacked adaptor inputs: a plain GEMM of its own
    rows = what != "prompt"
    M = sum(n) if rows else n
    return env, {SWITCH[k]: int(v) for k, v in switches.items()}, M, lin, (sum(-(-k // 16) for k in n) if rows else None), what == "extend_rows"


@pytest.mark.parametrize("case", sorted(LOGS))
def test_plan_agrees_with_the_launch_logs_recorded_before_plan_gemm(case):
    env, options, M, lin, ntiles, extend = case_setup(case)
    log = LOGS[case]
    qk_norm = 1 if env[2] == 1 else 0   # (modelgen gives the gemma3 model its q / k norms)
    lines = [line_of("gemm", env, [*L, M, 0, 0], options) for L in lin.values()]
    lines += [line_of("gemm", env, [*lin["qkv"], M, 2, 0], options), line_of("fold", env, [*lin["qkv"], 0, 0], options)]
    lines += [line_of("attn", env, [M], options), line_of("packed", env, [ntiles or 1], options), line_of("extend", env, [0], options)]
    lines += [line_of("act", env, [*lin["w13"], M, 1], options)]
    got = ask(lines)
    # the family of each of the block's linears (and of an adaptor's A GEMM) is the family of the GEMM names in the log
    planned = {a.split()[0] for a in got[:len(lin)]}
    logged = {gemm_family(n) for n in log} - {None}
    assert planned == logged, (case, dict(zip(lin, got)), sorted(set(log)))
    # rope + cache: from the partial sums where wq|wk|wv may stop at them (fold_parts_ok) and splits K, in the packed form for rows
    qkv_parts, fold, attn, packed, ext, act = got[len(lin):]
    # the activation rides in the epilogue of w1|w3 (an _e3 / _e4 GEMM) exactly where act_epi_ok says so
    assert (act == "1") == any(re.search(r"_gemm\w*_e[34]$", n) for n in log), (case, act)
    parts = 1 if fold.split()[0] == "1" and int(qkv_parts.split()[4]) > 1 else 0
    rope = ask([line_of("rope", env, [M, parts, 1 if ntiles else 0, qk_norm], options)])[0].split()[0]
    assert [n for n in log if "_rope_cache_" in n] == [rope] * 2, (case, rope)
    # attention: float rows take the two-pass kernels (no plan); rows take the packed or the extend form
    logged_attn = sorted({n for n in log if re.match(r"mc_(pf_attn|pp_attn|px_sums|px_pv|px_reduce)", n)})
    if env[0] == 4:
        assert not logged_attn and "mc_pf_scores_float" in log
    elif extend:
        assert logged_attn == sorted(ext.split()[:2])   # (no tile of the case is split: no reduce)
    elif ntiles:
        assert logged_attn == [packed.split()[0]] and int(packed.split()[1]) == ntiles
    else:
        assert logged_attn == [attn.split()[0]]
