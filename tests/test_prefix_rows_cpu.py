"""Shared-prefix rows (include/metalchat_hip.h Part 2r) without a GPU: the header declares exactly the six mc_prefix_* calls, the code object
holds the mc_sp_* kernels without a private segment or spills, a null batch gets the specified answers, and plan_prefix_attention
(csrc/batch_plan.h, asked through tests/cpp/test_prefix_plan) names the launches and their grids with and without attached rows."""
import os
import re
import subprocess

import pytest

from metalchat_amd import build as b
from metalchat_amd import runtime

CALLS = ["mc_prefix_attach", "mc_prefix_attached", "mc_prefix_detach", "mc_prefix_fork", "mc_prefix_import_kv", "mc_prefix_info"]
KERNELS = {"mc_sp_attn_scores_bfloat", "mc_sp_attn_pv_bfloat"}


def test_the_header_declares_the_six_calls_once_each():
    with open(os.path.join(os.path.dirname(b.HERE), "include", "metalchat_hip.h")) as fh:
        declared = re.findall(r"^(?:mc_status|int32_t)\s+(mc_prefix_\w+)\(", fh.read(), re.M)
    assert sorted(declared) == CALLS


def test_the_code_object_holds_the_kernels_and_none_keeps_private_memory():
    out = subprocess.check_output(["/opt/rocm/lib/llvm/bin/llvm-readelf", "--notes", b.build_all()[0]], text=True)
    kernels = {m.group(1): k for k in out.split(".agpr_count")[1:] if (m := re.search(r"\.name:\s+(mc_sp_\w*)", k))}
    assert set(kernels) == KERNELS
    for k in kernels.values():
        assert [int(v) for v in re.findall(r"\.(?:private_segment_fixed_size|[sv]gpr_spill_count):\s+(\d+)", k)] == [0, 0, 0], k


def test_a_null_batch():
    api = runtime.capi()
    assert api.mc_prefix_attached(None, 0) == 0
    for call, args in (("mc_prefix_fork", (1,)), ("mc_prefix_import_kv", (0, None, None, 1)), ("mc_prefix_attach", (0,)), ("mc_prefix_detach", (0, 1)),
                       ("mc_prefix_info", (None, None))):
        assert getattr(api, call)(None, *args) == 1
        assert f"{call}: null argument" in api.mc_last_error().decode()


@pytest.mark.parametrize("H,KV,hd,S,B,G", [(32, 8, 128, 2048, 8, 4), (32, 4, 64, 1000, 5, 2), (16, 1, 128, 104, 3, 1)])
def test_the_plan_names_the_launches_and_their_grids(H, KV, hd, S, B, G):
    def ask(attached):
        out = subprocess.check_output([b.build_prefix_plan_test(), *map(str, (H, KV, hd, S, B, attached))], text=True).splitlines()
        return [(n, *map(int, rest)) for n, *rest in (line.split() for line in out[:2])], out[2]

    nsplit = (S + 63) // 64
    launches, tail = ask(0)
    assert launches == [("mc_b_attn_scores_rows_bfloat", nsplit, KV, B, 256), ("mc_b_attn_pv_rows_bfloat", hd // 16, KV, B, 1024)]
    launches, tail = ask(1)
    assert launches == [("mc_sp_attn_scores_bfloat", nsplit, KV, B + 1, 256), ("mc_sp_attn_pv_bfloat", hd // 16, KV, (B + G - 1) // G, 1024)]
    assert tail == f"{G} {(S - 1) // 64 * 64}"
