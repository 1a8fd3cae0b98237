"""The packed prompt pass (mc_rows_prefill, include/metalchat_hip.h Part 2d) without a GPU: the entry point is exported and bound,
every packed kernel the prompt pass can launch is in the code object, and null arguments are refused before a batch is looked at."""
import ctypes as C
import os
import re
import subprocess

import pytest

import metalchat_amd as mc
from metalchat_amd import build as b

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
READELF = ["/opt/rocm/lib/llvm/bin/llvm-readelf", "/usr/bin/readelf"]

# prefill.cc run_prefill (packed branches) launches these names (formed in prefill_plan.h plan_rope / plan_packed_attention; the gather: prefill.cc): rope + cache write from the GEMM's rows or its split-K partials, one
# or two query heads per attention workgroup at head_dim 64 / 128 (the batch's admitted sizes), and the gather of the last rows
PACKED_KERNELS = ["mc_pp_rope_cache_bfloat", "mc_pp_rope_cache_parts_bfloat", "mc_pp_gather_last_bfloat"] + [
    f"mc_pp_{a}_bfloat_hd{hd}" for a in ("attn", "attn2") for hd in (64, 128)]


def ints(*v):
    return (C.c_int32 * max(len(v), 1))(*v)


def test_the_entry_point_is_exported_and_bound():
    text = open(os.path.join(ROOT, "include", "metalchat_hip.h")).read()
    assert re.findall(r"\b(mc_rows_\w+)\s*\(", text) == ["mc_rows_prefill"]
    lib = mc.capi()
    assert "mc_rows_prefill" in lib._prototypes
    getattr(lib, "mc_rows_prefill")
    assert callable(getattr(mc.Batch, "prefill_rows"))


def test_every_packed_kernel_is_in_the_code_object():
    src = open(os.path.join(ROOT, "metalchat_amd", "csrc", "prefill.cc")).read() + open(os.path.join(ROOT, "metalchat_amd", "csrc", "prefill_plan.h")).read()
    for stem in ('"mc_pp_rope_cache_bfloat"', '"mc_pp_rope_cache_parts_bfloat"', '"mc_pp_attn2_bfloat_hd"', '"mc_pp_attn_bfloat_hd"',
                 '"mc_pp_gather_last_bfloat"'):
        assert stem in src, stem
    hsaco, _ = b.build_all()
    tool = next((t for t in READELF if os.path.exists(t)), None)
    if tool is None:
        pytest.skip("no readelf available")
    out = subprocess.check_output([tool, "--symbols", "--wide", hsaco], text=True)
    symbols = {line.split()[-1] for line in out.splitlines() if " FUNC " in line}
    missing = [n for n in PACKED_KERNELS if n not in symbols]
    assert not missing, missing


def test_null_arguments_are_refused_without_a_device():
    lib = mc.capi()
    fake = C.c_void_p(1)  # never dereferenced: the pointers are checked first
    toks, lens, pos, out = ints(1, 2), ints(2), ints(0), ints(0)
    for args in ((None, toks, lens, pos, out), (fake, None, lens, pos, out), (fake, toks, None, pos, out), (fake, toks, lens, None, out)):
        assert lib.mc_rows_prefill(*args) == 1
        assert b"mc_rows_prefill: null argument" in lib.mc_last_error()
