"""Row log-probabilities (include/metalchat_hip.h Part 2n) without a GPU: the four calls are declared, exported and bound with their
signatures; the refusals that need no device; the four kernels are in the code object with their block size, nothing in private
memory and no spills; and the plan (csrc/batch_plan.h plan_logprobs / check_logprobs through tests/cpp/test_logprob_plan, a plain
g++ program): nothing while the switch is off, two launches with grid (ceil(V / 2048), R) and (1, R) when it is on, the ragged
names, the refusal of a vocabulary the finish launch cannot fold, and the constants of kernels/abi.h."""
import ctypes as C
import json
import os
import re
import subprocess

import pytest

from metalchat_amd import build as b

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
READELF = "/opt/rocm/lib/llvm/bin/llvm-readelf"
CALLS = ["mc_logprobs_set", "mc_logprobs_enabled", "mc_logprobs_get", "mc_logprobs_get_verify"]
KERNELS = ["mc_logprob_parts_bfloat", "mc_logprob_parts_rows_bfloat", "mc_logprob_finish_bfloat", "mc_logprob_finish_rows_bfloat"]


def ask(lines):
    exe = b.build_logprob_plan_test()
    out = subprocess.run([exe], input="".join(line + "\n" for line in lines), capture_output=True, text=True, check=True).stdout
    answers = [json.loads(a) for a in out.split("\n")[:-1]]
    assert len(answers) == len(lines)
    return answers


def test_the_calls_are_declared_exported_and_bound():
    from metalchat_amd import runtime
    import metalchat_amd as mc

    b.build_all()
    text = open(os.path.join(ROOT, "include", "metalchat_hip.h")).read()
    part = text[text.index("Part 2n --"):]
    code = re.sub(r"/\*.*?\*/", "", "/*" + part, flags=re.S)
    so = C.CDLL(os.path.join(ROOT, "metalchat_amd", "lib", "libmetalchat_hip.so"))
    lib = runtime.capi()
    assert re.search(r"#define\s+MC_LOGPROBS_MAX_TOP\s+20\b", code)
    assert re.search(r"\bmc_status\s+mc_logprobs_set\s*\(\s*mc_batch\s*\*\s*b\s*,\s*int32_t\s+enable\s*,\s*int32_t\s+top_n\s*\)", code)
    assert re.search(r"\bint32_t\s+mc_logprobs_enabled\s*\(\s*const\s+mc_batch\s*\*\s*b\s*,\s*int32_t\s*\*\s*top_n\s*\)", code)
    assert re.search(r"\bmc_status\s+mc_logprobs_get\s*\(\s*mc_batch\s*\*\s*b\s*,\s*int32_t\s+n\s*,\s*float\s*\*\s*token_logprobs\s*,\s*int32_t\s*\*\s*top_ids\s*,"
                     r"\s*float\s*\*\s*top_logprobs\s*\)", code)
    assert re.search(r"\bmc_status\s+mc_logprobs_get_verify\s*\(\s*mc_batch\s*\*\s*b\s*,\s*float\s*\*\s*pick_logprobs\s*,\s*int32_t\s*\*\s*top_ids\s*,"
                     r"\s*float\s*\*\s*top_logprobs\s*\)", code)
    i32, pi, pf = C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_float)
    for name in CALLS:
        assert hasattr(so, name), name
        assert name in lib._prototypes, name
    assert lib._prototypes["mc_logprobs_set"] == (i32, [C.c_void_p, i32, i32])
    assert lib._prototypes["mc_logprobs_enabled"] == (i32, [C.c_void_p, pi])
    assert lib._prototypes["mc_logprobs_get"] == (i32, [C.c_void_p, i32, pf, pi, pf])
    assert lib._prototypes["mc_logprobs_get_verify"] == (i32, [C.c_void_p, pf, pi, pf])
    assert "not the sampler's truncated nucleus" in " ".join(part.split()).replace("* ", "")
    assert "Not covered:" in part
    for method in ("set_logprobs", "logprobs_setting", "logprobs", "verify_logprobs"):
        assert callable(getattr(mc.Batch, method)), method


def test_the_refusals_that_need_no_device():
    from metalchat_amd import runtime

    b.build_all()
    lib = runtime.capi()
    assert lib.mc_logprobs_set(None, 1, 0) == 1
    assert lib.mc_last_error() == b"mc_logprobs_set: null argument"
    top = C.c_int32(-7)
    assert lib.mc_logprobs_enabled(None, C.byref(top)) == 0 and top.value == -7
    assert lib.mc_logprobs_enabled(None, None) == 0
    out = (C.c_float * 4)()
    for call, args, name in ((lib.mc_logprobs_get, (None, 1, out, None, None), b"mc_logprobs_get"),
                             (lib.mc_logprobs_get_verify, (None, out, None, None), b"mc_logprobs_get_verify")):
        assert call(*args) == 1
        assert lib.mc_last_error() == name + b": null argument"
    # the values of mc_logprobs_set (a batch's vocabulary given)
    a = ask(["set 0 0 2048", "set 1 0 2048", "set 1 20 2048", "set 0 20 128256", "set 2 0 2048", "set -1 5 2048", "set 1 21 2048", "set 1 -1 2048",
             "set 1 20 16", "set 1 16 16"])
    assert a[0] == a[1] == a[2] == a[3] == a[9] == {"ok": True}
    assert a[4] == a[5] == {"refused": "mc_logprobs_set: enable must be 0 or 1"}
    assert a[6] == a[7] == {"refused": "mc_logprobs_set: top_n must lie in [0, 20]"}
    assert a[8] == {"refused": "mc_logprobs_set: top_n (20) is above the vocabulary (16)"}


def test_the_kernels_are_in_the_code_object_and_keep_nothing_in_private_memory():
    hsaco, _ = b.build_all()
    assert os.path.exists(READELF), "no llvm-readelf"
    syms = subprocess.check_output([READELF, "--symbols", "--wide", hsaco], text=True)
    funcs = {line.split()[-1] for line in syms.splitlines() if " FUNC " in line}
    assert sorted(s for s in funcs if s.startswith("mc_logprob_")) == sorted(KERNELS)
    out = subprocess.check_output([READELF, "--notes", hsaco], text=True)
    name, block, fields = None, None, {}
    for line in out.splitlines():
        line = line.strip()
        if line.startswith("- .") or line.startswith(".") or line.startswith("-"):
            key, _, val = line.lstrip("- ").partition(":")
            key, val = key.strip(), val.strip()
            if key == ".max_flat_workgroup_size":   # (a kernel's keys are sorted: this one comes before its .name)
                block = int(val)
            elif key == ".name":
                name = val
                fields[name] = {".max_flat_workgroup_size": block}
            elif name and key in (".private_segment_fixed_size", ".vgpr_spill_count", ".sgpr_spill_count"):
                fields[name][key] = int(val)
    for k in KERNELS:
        assert k in fields, k
        assert fields[k] == {".max_flat_workgroup_size": 256, ".private_segment_fixed_size": 0, ".vgpr_spill_count": 0, ".sgpr_spill_count": 0}, (k, fields[k])


def test_the_plan():
    assert ask(["abi"]) == [{"max_top": 20, "threads": 256, "chunk": 2048, "key_cap": 2048, "part_bytes": 16}]
    for V in (2048, 2056, 128256):
        for R in (8, 64):
            for top_n in (0, 5, 20):
                off, lock, ragged = ask([f"plan 0 {top_n} {V} {R} 0", f"plan 1 {top_n} {V} {R} 0", f"plan 1 {top_n} {V} {R} 1"])
                assert off == {"any": False}
                nchunk = -(-V // 2048)
                assert lock == {"any": True, "nchunk": nchunk, "parts": ["mc_logprob_parts_bfloat", nchunk, R, 1, 256, 0],
                                "finish": ["mc_logprob_finish_bfloat", 1, R, 1, 256, 0]}
                assert ragged == {"any": True, "nchunk": nchunk, "parts": ["mc_logprob_parts_rows_bfloat", nchunk, R, 1, 256, 0],
                                  "finish": ["mc_logprob_finish_rows_bfloat", 1, R, 1, 256, 0]}
    assert {-(-V // 2048) for V in (2048, 2056, 128256)} == {1, 2, 63}
    # a verify call: the plain names over its M packed rows
    assert ask(["plan 1 20 2048 23 0"])[0]["parts"] == ["mc_logprob_parts_bfloat", 1, 23, 1, 256, 0]
    # the finish launch folds at most 256 chunks and 2048 keys: 102 chunks at top_n 20 (V <= 208896), 256 at top_n <= 8
    ok, refused, ok0, refused0 = ask(["plan 1 20 208896 8 1", "plan 1 20 208897 8 1", "plan 1 0 524288 8 0", "plan 1 0 524289 8 0"])
    assert ok["nchunk"] == 102 and ok0["nchunk"] == 256
    assert refused == {"refused": "mc_logprobs: the vocabulary has 103 chunks of 2048, with top_n 20 more than the finish launch folds (256 chunks, 2048 keys)"}
    assert refused0 == {"refused": "mc_logprobs: the vocabulary has 257 chunks of 2048, with top_n 0 more than the finish launch folds (256 chunks, 2048 keys)"}
    # switched off, such a vocabulary is no refusal: nothing is planned
    assert ask(["plan 0 20 524289 8 0"]) == [{"any": False}]
