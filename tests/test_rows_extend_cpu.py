"""Chunks that see their row's context (mc_extend_rows, include/metalchat_hip.h Part 2e) without a GPU: the entry point is declared
once, exported and bound, every attention kernel the call can launch is in the code object, and null arguments are refused before
a batch is looked at."""
import ctypes as C
import os
import re
import subprocess

import pytest

import metalchat_amd as mc
from metalchat_amd import build as b

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
READELF = ["/opt/rocm/lib/llvm/bin/llvm-readelf", "/usr/bin/readelf"]

# prefill.cc run_prefill (the branch of a packed pass that extends) launches these names, formed in prefill_plan.h plan_extend_attention: the exp sums and p V of a key range with one
# or two query heads per workgroup, and the reduce over a split tile's ranges, at head_dim 64 / 128 (the batch's admitted sizes)
EXTEND_KERNELS = [f"mc_px_{a}_bfloat_hd{hd}" for a in ("sums", "sums2", "pv", "pv2", "reduce") for hd in (64, 128)]


def ints(*v):
    return (C.c_int32 * max(len(v), 1))(*v)


def test_the_entry_point_is_declared_once_exported_and_bound():
    text = open(os.path.join(ROOT, "include", "metalchat_hip.h")).read()
    assert re.findall(r"\b(mc_extend_\w+)\s*\(", text) == ["mc_extend_rows"]
    assert "Part 2e" in text
    lib = mc.capi()
    assert "mc_extend_rows" in lib._prototypes
    getattr(lib, "mc_extend_rows")
    assert callable(getattr(mc.Batch, "extend_rows"))
    assert lib._prototypes["mc_extend_rows"] == lib._prototypes["mc_rows_prefill"]


def test_every_extend_kernel_is_in_the_code_object():
    src = open(os.path.join(ROOT, "metalchat_amd", "csrc", "prefill_plan.h")).read()
    for stem in ('"mc_px_sums"', '"mc_px_pv"', '"mc_px_reduce_bfloat_hd"'):
        assert stem in src, stem
    hsaco, _ = b.build_all()
    tool = next((t for t in READELF if os.path.exists(t)), None)
    assert tool is not None, "no readelf available"
    out = subprocess.check_output([tool, "--symbols", "--wide", hsaco], text=True)
    symbols = {line.split()[-1] for line in out.splitlines() if " FUNC " in line}
    missing = [n for n in EXTEND_KERNELS if n not in symbols]
    assert not missing, missing


def test_null_arguments_are_refused_without_a_device():
    lib = mc.capi()
    fake = C.c_void_p(1)  # never dereferenced: the pointers are checked first
    toks, lens, pos, out = ints(1, 2), ints(2), ints(0), ints(0)
    for args in ((None, toks, lens, pos, out), (fake, None, lens, pos, out), (fake, toks, None, pos, out), (fake, toks, lens, None, out)):
        assert lib.mc_extend_rows(*args) == 1
        assert b"mc_extend_rows: null argument" in lib.mc_last_error()
