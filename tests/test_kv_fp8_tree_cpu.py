"""mc_tree_verify on an fp8 batch (include/metalchat_hip.h Part 2q) without a GPU: the two calls are exported and bound and refuse a null batch,
the code object holds exactly the eleven mc_tv8_* kernels, none with a private segment or spills, and the plans (csrc/prefill_plan.h and
csrc/batch_plan.h with kv_format = MC_KV_FP8, asked through tests/cpp/test_kv8_tree_plan) name them -- the one- and two-head forms at head_dim 64 and
128, the compact launch over its owners -- and refuse the tree by its own switch alone."""
import itertools
import re
import subprocess

import pytest

from metalchat_amd import build as b
from metalchat_amd import runtime

NAMES = ({"mc_tv8_rope_cache_bfloat", "mc_tv8_rope_cache_parts_bfloat", "mc_tv8_compact"} |
         {f"mc_tv8_{a}{two}_bfloat_hd{hd}" for a in ("sums", "pv") for two in ("", "2") for hd in (64, 128)})


def test_the_switch_is_exported_bound_and_refuses_a_null_batch():
    api = runtime.capi()
    assert api.mc_kv_tree_enabled(None) == 0
    assert api.mc_kv_tree_set(None, 1) != 0
    assert "mc_kv_tree_set: null argument" in api.mc_last_error().decode()
    assert hasattr(runtime.Batch, "set_kv_tree") and isinstance(runtime.Batch.kv_tree, property)


def test_the_code_object_holds_the_eleven_kernels_and_none_keeps_private_memory():
    out = subprocess.check_output(["/opt/rocm/lib/llvm/bin/llvm-readelf", "--notes", b.build_all()[0]], text=True)
    kernels = {m.group(1): k for k in out.split(".agpr_count")[1:] if (m := re.search(r"\.name:\s+(mc_tv8\w*)", k))}
    assert set(kernels) == NAMES and len(NAMES) == 11
    for k in kernels.values():
        assert [int(v) for v in re.findall(r"\.(?:private_segment_fixed_size|[sv]gpr_spill_count):\s+(\d+)", k)] == [0, 0, 0], k


@pytest.mark.parametrize("hd,heads", itertools.product((64, 128), (1, 2)))
def test_the_plans_name_the_byte_forms_and_the_refusal_follows_the_tree_switch(hd, heads):
    two, kv = ("2", 2) if heads == 2 else ("", 8)          # 8 query heads: n_rep 4 takes the two-head forms, n_rep 1 the one-head forms
    out = subprocess.check_output([b.build_kv8_tree_plan_test(), str(hd), "8", str(kv), str(heads)], text=True).splitlines()
    assert out[:6] == ["mc_tv8_rope_cache_bfloat", "mc_tv8_rope_cache_parts_bfloat", f"mc_tv8_sums{two}_bfloat_hd{hd}", f"mc_tv8_pv{two}_bfloat_hd{hd}",
                       f"mc_px_reduce_bfloat_hd{hd}", "mc_tv8_compact"]
    assert set(out[:6]) - {f"mc_px_reduce_bfloat_hd{hd}"} <= NAMES
    assert int(out[6]) == (kv * hd // 16 + kv * hd + 2 * kv + 255) // 256      # K words, V bytes, the two exponent planes
    assert out[7].startswith("mc_tree_verify: the batch holds an fp8 cache") and out[8] == "-"   # (the packed switch on both times)
