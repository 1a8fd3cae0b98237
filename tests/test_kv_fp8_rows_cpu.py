"""The packed passes on an fp8 batch (include/metalchat_hip.h Part 2p) without a GPU: the two calls are exported and bound, the plan
(csrc/prefill_plan.h with kv_format = MC_KV_FP8, asked through tests/cpp/test_kv8_rows_plan) names a byte-form kernel for head_dim 64 / 128
and one or two query heads per workgroup, and every kernel it names is in the code object with no private segment and no spills."""
import itertools
import re
import subprocess

import pytest

from metalchat_amd import build as b
from metalchat_amd import runtime
from test_kernel_names_cpu import symbols  # noqa: F401 (the fixture)


def test_the_switch_is_exported_and_bound():
    api = runtime.capi()
    assert api.mc_kv_packed_enabled(None) == 0
    assert api.mc_kv_packed_set(None, 1) != 0
    assert hasattr(runtime.Batch, "set_kv_packed") and isinstance(runtime.Batch.kv_packed, property)


@pytest.mark.parametrize("hd,heads", itertools.product((64, 128), (1, 2)))
def test_the_plan_names_the_byte_forms_and_the_code_object_has_them(symbols, hd, heads):
    two = "2" if heads == 2 else ""
    names = subprocess.check_output([b.build_kv8_rows_plan_test(), str(hd), "8", "2", str(heads)], text=True).split()
    assert names == ["mc_pp8_rope_cache_bfloat", "mc_pp8_rope_cache_parts_bfloat", f"mc_pp8_attn{two}_bfloat_hd{hd}", f"mc_px8_sums2_bfloat_hd{hd}",
                     f"mc_px8_pv2_bfloat_hd{hd}", f"mc_px_reduce_bfloat_hd{hd}"]
    assert not [n for n in names if n not in symbols]
    assert {f"mc_px8_{a}_bfloat_hd{hd}" for a in ("sums", "pv")} <= symbols   # (n_rep odd: the one-head extend forms)


def test_the_byte_forms_keep_no_private_memory():
    """test_kernel_names_cpu.test_no_hot_kernel_keeps_private_memory's check on the fourteen new kernels"""
    out = subprocess.check_output(["/opt/rocm/lib/llvm/bin/llvm-readelf", "--notes", b.build_all()[0]], text=True)
    kernels = [k for k in out.split(".agpr_count")[1:] if re.search(r"\.name:\s+mc_p[px]8_", k)]
    assert len(kernels) == 14
    for k in kernels:
        assert [int(v) for v in re.findall(r"\.(?:private_segment_fixed_size|[sv]gpr_spill_count):\s+(\d+)", k)] == [0, 0, 0], k
