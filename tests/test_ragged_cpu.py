"""Ragged rows (mc_ragged_*, include/metalchat_hip.h Part 2c) without a GPU: every entry point is exported and bound, every
per-row kernel name the batch plan (batch_plan.h) can form is in the code object, and the arguments that need no device are refused."""
import ctypes as C
import os
import re
import subprocess

import pytest

import batch_plan_program as bp
import metalchat_amd as mc
from metalchat_amd import build as b

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
READELF = ["/opt/rocm/lib/llvm/bin/llvm-readelf", "/usr/bin/readelf"]

# what a ragged step launches besides the lockstep kernels it shares (the GEMVs, rmsnorm, top-k candidates): batch_plan.h forms
# the per-row names as "mc_b_<kernel>" + "_rows_bfloat"
RAGGED_KERNELS = ["mc_b_rows_begin", "mc_b_embed_rows_bfloat"] + [
    f"mc_b_{k}_rows_bfloat" for k in ("rope_kv", "attn_scores", "attn_pv", "argmax", "sample")] + [
    "mc_b_topk_candidates_bfloat", "mc_kv_export_bfloat"]

P = C.POINTER(C.c_int32)


def ints(*v):
    return (C.c_int32 * max(len(v), 1))(*v)


def test_every_ragged_entry_point_is_exported_and_bound():
    text = open(os.path.join(ROOT, "include", "metalchat_hip.h")).read()
    names = sorted(set(re.findall(r"\b(mc_ragged_\w+)\s*\(", text)))
    assert names == ["mc_ragged_export_kv", "mc_ragged_generate", "mc_ragged_lengths", "mc_ragged_step"], names
    lib = mc.capi()
    for n in names:
        assert n in lib._prototypes, n
        getattr(lib, n)  # exported by libmetalchat_hip.so
    for n in ("step_rows", "generate_rows", "lengths", "export_row_kv"):
        assert callable(getattr(mc.Batch, n)), n


def test_every_ragged_kernel_is_in_the_code_object():
    formed = bp.formed_names()   # (the host forms these names: batch_plan.h through tests/cpp/test_batch_plan)
    assert "mc_b_rows_begin" in formed and not [n for n in RAGGED_KERNELS if n.endswith("_rows_bfloat") and n not in formed]
    hsaco, _ = b.build_all()
    tool = next((t for t in READELF if os.path.exists(t)), None)
    if tool is None:
        pytest.skip("no readelf available")
    out = subprocess.check_output([tool, "--symbols", "--wide", hsaco], text=True)
    symbols = {line.split()[-1] for line in out.splitlines() if " FUNC " in line}
    missing = [n for n in RAGGED_KERNELS if n not in symbols]
    assert not missing, missing
    assert len([s for s in symbols if s.startswith("mc_b_")]) <= 64


def refused(status, words):
    assert status == 1
    msg = mc.capi().mc_last_error()
    assert words in msg, msg


def test_null_arguments_are_refused_without_a_device():
    lib = mc.capi()
    toks, pos, out = ints(1), ints(0), ints(0)
    refused(lib.mc_ragged_step(None, toks, pos, out), b"mc_ragged_step: null")
    refused(lib.mc_ragged_generate(None, toks, pos, 1, None, 0, out, out), b"mc_ragged_generate: null")
    refused(lib.mc_ragged_lengths(None, out), b"mc_ragged_lengths: null")
    refused(lib.mc_ragged_export_kv(None, 0, 0, None, None, out), b"mc_ragged_export_kv: null")


def test_counts_are_refused_before_the_batch_is_looked_at():
    lib = mc.capi()
    fake = C.c_void_p(1)  # never dereferenced: the counts are checked first
    toks, pos, out = ints(1), ints(0), ints(0)
    for n in (0, -1):
        refused(lib.mc_ragged_generate(fake, toks, pos, n, None, 0, out, out), b"n must be positive")
    refused(lib.mc_ragged_generate(fake, toks, pos, 4, ints(2), -1, out, out), b"n_stop must not be negative")
    refused(lib.mc_ragged_generate(fake, toks, pos, 4, None, 2, out, out), b"null")
