"""Shared-prefix rows on an fp8 batch (include/metalchat_hip.h Part 2s) without a GPU: the header declares the two calls once each, a null batch
gets the specified answers, the code object holds exactly the two mc_sp8_* kernels without a private segment or spills, and
plan_prefix_attention (csrc/batch_plan.h, asked through tests/cpp/test_kv8_prefix_plan) names the launches and grids by cache format and
MC_SP8_GROUPS."""
import os
import re
import subprocess

import pytest

from metalchat_amd import build as b
from metalchat_amd import runtime

KERNELS = {"mc_sp8_attn_scores_bfloat", "mc_sp8_attn_pv_bfloat"}
FP8 = 1


def test_the_header_declares_the_two_calls_once_each_and_a_null_batch_is_answered():
    with open(os.path.join(os.path.dirname(b.HERE), "include", "metalchat_hip.h")) as fh:
        declared = re.findall(r"^(?:mc_status|int32_t)\s+(mc_kv_prefix_\w+)\(", fh.read(), re.M)
    assert sorted(declared) == ["mc_kv_prefix_enabled", "mc_kv_prefix_set"]
    api = runtime.capi()
    assert api.mc_kv_prefix_enabled(None) == 0
    assert api.mc_kv_prefix_set(None, 1) == 1
    assert "mc_kv_prefix_set: null argument" in api.mc_last_error().decode()
    assert hasattr(runtime.Batch, "set_kv_prefix") and hasattr(runtime.Batch, "kv_prefix")


def test_the_code_object_holds_the_two_kernels_and_none_keeps_private_memory():
    out = subprocess.check_output(["/opt/rocm/lib/llvm/bin/llvm-readelf", "--notes", b.build_all()[0]], text=True)
    kernels = {m.group(1): k for k in out.split(".agpr_count")[1:] if (m := re.search(r"\.name:\s+(mc_sp8\w*)", k))}
    assert set(kernels) == KERNELS
    for k in kernels.values():
        assert [int(v) for v in re.findall(r"\.(?:private_segment_fixed_size|[sv]gpr_spill_count):\s+(\d+)", k)] == [0, 0, 0], k


@pytest.mark.parametrize("H,KV,hd,S,B,G", [(32, 8, 128, 2048, 8, 4), (32, 4, 64, 1000, 5, 2), (16, 1, 128, 104, 3, 1)])
def test_the_plan_names_the_launches_and_their_grids(H, KV, hd, S, B, G):
    def ask(attached, fmt, gw):
        out = subprocess.check_output([b.build_kv8_prefix_plan_test(), *map(str, (H, KV, hd, S, B, attached, fmt, gw))], text=True).splitlines()
        return [(n, *map(int, rest)) for n, *rest in (line.split() for line in out[:2])], int(out[2])

    nsplit, groups = (S + 63) // 64, (B + G - 1) // G
    rows = lambda f8: [(f"mc_b_attn_scores{f8}_rows_bfloat", nsplit, KV, B, 256), (f"mc_b_attn_pv{f8}_rows_bfloat", hd // 16, KV, B, 1024)]
    sp = [("mc_sp_attn_scores_bfloat", nsplit, KV, B + 1, 256), ("mc_sp_attn_pv_bfloat", hd // 16, KV, groups, 1024)]
    for gw in (1, 2, 4):
        assert ask(0, FP8, gw) == (rows("_f8"), 1)
        assert ask(1, FP8, gw) == ([("mc_sp8_attn_scores_bfloat", nsplit, KV, B + 1, 256), ("mc_sp8_attn_pv_bfloat", hd // 16, KV, (groups + gw - 1) // gw, 1024)], gw)
        assert ask(0, 0, gw) == (rows(""), 1) and ask(1, 0, gw) == (sp, 1)           # MC_KV_BF16: as today, whatever MC_SP8_GROUPS says
    assert ask(0, "-", "-") == (rows(""), 1) and ask(1, "-", "-") == (sp, 1)         # the call of the callers from before this part
    by_rule = ask(1, FP8, "-")
    assert by_rule == ask(1, FP8, 3) == ask(1, FP8, 8) and by_rule[1] in (1, 2, 4)   # anything else: by the rule
