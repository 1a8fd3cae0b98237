"""Speculative verify (mc_verify_rows, include/metalchat_hip.h Part 2f) without a GPU: the two entry points are declared once,
exported and bound; the four kernels the call adds are in the code object and keep nothing in private memory; null arguments are
refused before a batch is looked at; and the acceptance rule (verify_rule.py, which the GPU tests hold the device to) on cases
worked by hand."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

import batch_plan_program as bp
import metalchat_amd as mc
import verify_rule as vr
from metalchat_amd import build as b

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
READELF = ["/opt/rocm/lib/llvm/bin/llvm-readelf", "/usr/bin/readelf"]
VERIFY_KERNELS = ["mc_v_head_i4_bfloat", "mc_v_head_w_bfloat", "mc_v_argmax_bfloat", "mc_v_accept"]


def ints(*v):
    return (C.c_int32 * max(len(v), 1))(*v)


def readelf(*args):
    hsaco, _ = b.build_all()
    tool = next((t for t in READELF if os.path.exists(t)), None)
    assert tool is not None, "no readelf available"
    return subprocess.check_output([tool, *args, hsaco], text=True)


def test_the_entry_points_are_declared_once_exported_and_bound():
    text = open(os.path.join(ROOT, "include", "metalchat_hip.h")).read()
    assert re.findall(r"\b(mc_verify_\w+)\s*\(", text) == ["mc_verify_rows", "mc_verify_get_logits"]
    assert "Part 2f" in text
    lib = mc.capi()
    for name in ("mc_verify_rows", "mc_verify_get_logits"):
        assert name in lib._prototypes
        getattr(lib, name)
    assert callable(getattr(mc.Batch, "verify_rows")) and callable(getattr(mc.Batch, "verify_logits"))
    # extend's arguments, then accepted, next_tokens, picks
    assert lib._prototypes["mc_verify_rows"][1][:4] == lib._prototypes["mc_extend_rows"][1][:4]
    assert len(lib._prototypes["mc_verify_rows"][1]) == 7
    assert lib._prototypes["mc_verify_get_logits"] == lib._prototypes["mc_batch_get_logits"]


def test_every_verify_kernel_is_in_the_code_object():
    formed = bp.formed_names()   # (the host forms these names: batch_plan.h through tests/cpp/test_batch_plan)
    for name in VERIFY_KERNELS:
        assert name in formed, name
    out = readelf("--symbols", "--wide")
    symbols = {line.split()[-1] for line in out.splitlines() if " FUNC " in line}
    assert sorted(s for s in symbols if s.startswith("mc_v_")) == sorted(VERIFY_KERNELS)


def test_no_verify_kernel_keeps_private_memory():
    """the code object's notes, read as test_kernel_names_cpu.test_no_hot_kernel_keeps_private_memory reads them: a private
    segment of 0 bytes and no spills for each of the four"""
    name, fields = None, {}
    for line in readelf("--notes").splitlines():
        line = line.strip()
        if line.startswith("- .") or line.startswith(".") or line.startswith("-"):
            key, _, val = line.lstrip("- ").partition(":")
            key, val = key.strip(), val.strip()
            if key == ".name":
                name = val
                fields[name] = {}
            elif name and key in (".private_segment_fixed_size", ".vgpr_spill_count", ".sgpr_spill_count"):
                fields[name][key] = int(val)
    for n in VERIFY_KERNELS:
        assert n in fields, n
        assert fields[n] == {".private_segment_fixed_size": 0, ".vgpr_spill_count": 0, ".sgpr_spill_count": 0}, (n, fields[n])


def test_null_arguments_are_refused_without_a_device():
    lib = mc.capi()
    fake = C.c_void_p(1)  # never dereferenced: the pointers are checked first
    toks, lens, pos, acc, out = ints(1, 2), ints(2), ints(0), ints(0), ints(0, 0)
    for args in ((None, toks, lens, pos, acc, out, out), (fake, None, lens, pos, acc, out, out), (fake, toks, None, pos, acc, out, out),
                 (fake, toks, lens, None, acc, out, out), (fake, toks, lens, pos, None, out, out)):
        assert lib.mc_verify_rows(*args) == 1
        assert b"mc_verify_rows: null argument" in lib.mc_last_error()
    for args in ((None, toks), (fake, None)):
        assert lib.mc_verify_get_logits(*args) == 1
        assert b"mc_verify_get_logits: null argument" in lib.mc_last_error()


def test_the_acceptance_rule_on_cases_worked_by_hand():
    # chunk = [last accepted token, drafts ...]; picks[i] = the target's pick after chunk row i
    # nothing accepted: the first draft (7) is not the pick after row 0 (9); the next token is that pick
    assert vr.accept([5, 7, 8, 9], [9, 8, 9, 1]) == (0, 9)
    # everything accepted: all three drafts are the picks before them; the next token is the pick after the last draft
    assert vr.accept([5, 7, 8, 9], [7, 8, 9, 1]) == (3, 1)
    # a match after a mismatch does not count: draft 2 (8) misses pick 1 (3); draft 3 (9) == pick 2 (9) is not looked at
    assert vr.accept([5, 7, 8, 9], [7, 3, 9, 1]) == (1, 3)
    # one draft, accepted and rejected
    assert vr.accept([5, 7], [7, 2]) == (1, 2)
    assert vr.accept([5, 7], [6, 2]) == (0, 6)
    # a draft equal to the chunk's own first token is nothing special
    assert vr.accept([5, 5, 5], [5, 4, 5]) == (1, 4)
    # rows: one not in the call
    acc, nxt = vr.accept_rows([[5, 7, 8], None, [1, 2]], [[7, 8, 4], None, [3, 9]])
    assert acc.dtype == nxt.dtype == np.int32
    assert list(acc) == [2, -1, 0] and list(nxt) == [4, -1, 3]
