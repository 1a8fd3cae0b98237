"""Batched decode (mc_batch_*, include/metalchat_hip.h Part 2b) without a GPU: every entry point of the header is exported and
bound, every kernel name the host forms is in the code object, and the arguments that need no device are refused."""
import ctypes as C
import os
import re
import subprocess

import pytest

import metalchat_amd as mc
from metalchat_amd import build as b

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
READELF = ["/opt/rocm/lib/llvm/bin/llvm-readelf", "/usr/bin/readelf"]

# every name the batch plan (batch_plan.h) can form: mc_b_gemv_{i4|w}_bfloat_e{0,1,2} and the per-row launches, plus the existing kernels it reuses
BATCH_KERNELS = [f"mc_b_gemv_{f}_bfloat_e{e}" for f in ("i4", "w") for e in (0, 1, 2)] + [
    "mc_b_embed_bfloat", "mc_b_rmsnorm_bfloat", "mc_b_rope_kv_bfloat", "mc_b_attn_scores_bfloat", "mc_b_attn_pv_bfloat",
    "mc_b_argmax_bfloat", "mc_b_topk_candidates_bfloat", "mc_b_sample_bfloat",
    "mc_step_set", "mc_rope_table", "mc_kv_import_bfloat", "mc_kv_export_bfloat"]


def header_batch_functions():
    text = open(os.path.join(ROOT, "include", "metalchat_hip.h")).read()
    return sorted(set(re.findall(r"\b(mc_batch_\w+)\s*\(", text)))


def test_every_batch_entry_point_is_exported_and_bound():
    names = header_batch_functions()
    assert len(names) == 10, names
    lib = mc.capi()
    for n in names:
        assert n in lib._prototypes, n
        getattr(lib, n)  # exported by libmetalchat_hip.so


def test_every_batch_kernel_is_in_the_code_object():
    hsaco, _ = b.build_all()
    tool = next((t for t in READELF if os.path.exists(t)), None)
    if tool is None:
        pytest.skip("no readelf available")
    out = subprocess.check_output([tool, "--symbols", "--wide", hsaco], text=True)
    symbols = {line.split()[-1] for line in out.splitlines() if " FUNC " in line}
    missing = [n for n in BATCH_KERNELS if n not in symbols]
    assert not missing, missing
    # the batch adds few symbols to the code object
    assert len([s for s in symbols if s.startswith("mc_b_")]) <= 64


def test_create_refuses_without_a_device():
    lib = mc.capi()
    h = C.c_void_p()
    assert lib.mc_batch_create(None, 4, C.byref(h)) == 1
    assert b"null" in lib.mc_last_error()
    # the batch size is checked before anything else of the decoder is looked at
    fake = C.c_void_p(1)
    for bad in (0, -1, 9, 64):
        assert lib.mc_batch_create(fake, bad, C.byref(h)) == 1, bad
        assert b"batch must lie in [1, 8]" in lib.mc_last_error()
    assert not h.value
    assert lib.mc_batch_size(None) == 0
    lib.mc_batch_release(None)
    for call in (lambda: lib.mc_batch_step(None, None, 0, None), lambda: lib.mc_batch_generate(None, None, 0, 1, None),
                 lambda: lib.mc_batch_get_logits(None, None), lambda: lib.mc_batch_fork(None, 0, 1),
                 lambda: lib.mc_batch_set_seeds(None, None, 0)):
        assert call() == 1
