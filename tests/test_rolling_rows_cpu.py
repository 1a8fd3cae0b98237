"""Rolling rows (mc_rolling_set / mc_rolling_enabled / mc_rolling_fork_row, include/metalchat_hip.h Part 2j) without a GPU: the
entry points are declared, exported and bound; the one new kernel is in the code object and keeps nothing in private memory; the
arguments that need no device are refused; and the state rule (rolling_rule.state, which the GPU tests hold the device to) is the
batch-1 decoder's derive_state replayed step by step."""
import ctypes as C
import os
import re
import subprocess

import batch_plan_program as bp
import metalchat_amd as mc
import rolling_rule as rr
from metalchat_amd import build as b

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
READELF = ["/opt/rocm/lib/llvm/bin/llvm-readelf", "/usr/bin/readelf"]
ROLLING_KERNELS = ["mc_b_rows_begin_rolling"]
ENTRY_POINTS = ["mc_rolling_set", "mc_rolling_enabled", "mc_rolling_fork_row"]


def readelf(*args):
    hsaco, _ = b.build_all()
    tool = next((t for t in READELF if os.path.exists(t)), None)
    assert tool is not None, "no readelf available"
    return subprocess.check_output([tool, *args, hsaco], text=True)


def test_the_entry_points_are_declared_exported_and_bound():
    text = open(os.path.join(ROOT, "include", "metalchat_hip.h")).read()
    assert "Part 2j" in text
    assert sorted(set(re.findall(r"\b(mc_rolling_\w+)\s*\(", text))) == sorted(ENTRY_POINTS)   # the part's own prefix, nothing else under it
    lib = mc.capi()
    for n in ENTRY_POINTS:
        assert len(re.findall(r"\b%s\s*\(" % n, text)) == 1, n     # declared once
        assert n in lib._prototypes, n
        getattr(lib, n)                                             # exported by libmetalchat_hip.so
    for n in ("set_rolling", "rolling", "fork_row"):
        assert callable(getattr(mc.Batch, n)), n
    i32 = lib._prototypes["mc_batch_size"][0]
    assert lib._prototypes["mc_rolling_set"] == (i32, [C.c_void_p, i32])
    assert lib._prototypes["mc_rolling_enabled"] == (i32, [C.c_void_p])
    assert lib._prototypes["mc_rolling_fork_row"] == (i32, [C.c_void_p, i32, i32])


def test_the_rolling_kernel_is_in_the_code_object_and_the_host_names_it():
    formed = bp.formed_names()   # (batch_plan.h through tests/cpp/test_batch_plan)
    assert "mc_b_rows_begin_rolling" in formed and "mc_b_rows_begin" in formed   # the default launch stays
    out = readelf("--symbols", "--wide")
    symbols = {line.split()[-1] for line in out.splitlines() if " FUNC " in line}
    assert not [n for n in ROLLING_KERNELS if n not in symbols]
    assert sorted(s for s in symbols if "rolling" in s) == ROLLING_KERNELS


def test_the_rolling_kernel_keeps_no_private_memory():
    """the code object's notes, read as test_tree_verify_cpu reads them: a private segment of 0 bytes and no spills"""
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
    for n in ROLLING_KERNELS:
        assert n in fields, n
        assert fields[n] == {".private_segment_fixed_size": 0, ".vgpr_spill_count": 0, ".sgpr_spill_count": 0}, (n, fields[n])


def refused(status, words):
    assert status == 1
    msg = mc.capi().mc_last_error()
    assert words in msg, msg


def test_null_and_out_of_range_arguments_are_refused_without_a_device():
    lib = mc.capi()
    refused(lib.mc_rolling_set(None, 1), b"mc_rolling_set: null argument")
    refused(lib.mc_rolling_fork_row(None, 0, 1), b"mc_rolling_fork_row: null argument")
    assert lib.mc_rolling_enabled(None) == 0
    fake = C.c_void_p(1)  # never dereferenced: the value is checked first
    for bad in (2, -1, 64):
        refused(lib.mc_rolling_set(fake, bad), b"mc_rolling_set: enable must be 0 or 1")


def test_the_state_rule_is_derive_state_replayed():
    for S in (64, 256):
        pre, post = rr.pre_len(S), S - rr.pre_len(S)
        assert (S, pre, post) in ((64, 6, 58), (256, 8, 248))
        steps = rr.replay(3 * S, S)
        assert len(steps) == 3 * S
        for p, want in enumerate(steps):
            assert rr.state(p, S) == want, (S, p, rr.state(p, S), want)
        # the ring base passes through 0 again and the new row always takes the slot of the oldest post-sink position
        assert rr.state(S - 1 + post, S)[0] == 0 and rr.state(S, S) == (1, pre, S)
        for p in range(S, 3 * S):
            assert pre <= rr.state(p, S)[1] < S
            assert rr.state(p, S)[1] == rr.state(p - post, S)[1]


def test_the_positions_a_row_holds():
    assert rr.positions_held(5, 64) == list(range(5))
    assert rr.positions_held(64, 64) == list(range(64))
    assert rr.positions_held(65, 64) == list(range(6)) + list(range(7, 65))
    held = rr.positions_held(200, 64)
    assert len(held) == 64 and held[:6] == list(range(6)) and held[6] == 142 and held[-1] == 199
