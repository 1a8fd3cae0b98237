"""Row samplers (include/metalchat_hip.h Part 2k) without a GPU: the three kernels of the mixed pick are in the built code object
and keep nothing in private memory, the three calls are declared, exported and prototyped, and the refusals that need no device."""
import ctypes as C
import os
import re
import subprocess

import pytest

from metalchat_amd import build as b

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
READELF = "/opt/rocm/lib/llvm/bin/llvm-readelf"
KERNELS = ["mc_b_topk_candidates_mixed_bfloat", "mc_b_pick_mixed_bfloat", "mc_b_pick_mixed_rows_bfloat"]
CALLS = ["mc_row_sampler_set", "mc_row_sampler_get", "mc_row_sampler_reset"]


@pytest.fixture(scope="module")
def notes():
    """kernel name -> its resource fields in the code object's notes (the parse of test_kernel_names_cpu.py)"""
    hsaco, _ = b.build_all()
    if not os.path.exists(READELF):
        pytest.skip("no llvm-readelf")
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
    return fields


def test_the_mixed_kernels_are_in_the_code_object(notes):
    missing = [k for k in KERNELS if k not in notes]
    assert not missing, missing
    # one workgroup of the argmax's size per row; one wave per candidate list
    assert notes["mc_b_pick_mixed_bfloat"][".max_flat_workgroup_size"] == 1024
    assert notes["mc_b_pick_mixed_rows_bfloat"][".max_flat_workgroup_size"] == 1024
    assert notes["mc_b_topk_candidates_mixed_bfloat"][".max_flat_workgroup_size"] == 64


def test_no_private_memory_in_the_pick_kernels(notes):
    """The mixed kernels and the uniform ones they must agree with (the sampler's body is shared): a private segment of zero bytes
    and no spills.  The body's last sort once selected between two structs by address, which put 48 bytes of every kernel with that
    body into private memory without a spill being reported."""
    bad = []
    for k in KERNELS + ["mc_b_sample_bfloat", "mc_b_sample_rows_bfloat", "mc_b_argmax_bfloat", "mc_b_argmax_rows_bfloat",
                        "mc_b_topk_candidates_bfloat", "mc_sample_bfloat", "mc_sample_float"]:
        fld = notes[k]
        assert set(fld) >= {".private_segment_fixed_size", ".vgpr_spill_count", ".sgpr_spill_count"}, (k, fld)
        if fld[".private_segment_fixed_size"] or fld[".vgpr_spill_count"] or fld[".sgpr_spill_count"]:
            bad.append((k, fld))
    assert not bad, bad


def test_the_calls_are_declared_exported_and_prototyped():
    from metalchat_amd import runtime

    b.build_all()
    text = open(os.path.join(ROOT, "include", "metalchat_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    so = C.CDLL(os.path.join(ROOT, "metalchat_amd", "lib", "libmetalchat_hip.so"))
    lib = runtime.capi()
    for name in CALLS:
        assert re.search(r"\bmc_status\s+" + name + r"\s*\(", code), name
        assert hasattr(so, name), name
        assert name in lib._prototypes, name
    assert re.search(r"MC_SAMPLER_INHERIT\s*=\s*-1", code)
    assert runtime.SAMPLER_INHERIT == -1 and runtime.SAMPLER_INHERIT not in (runtime.SAMPLER_GREEDY, runtime.SAMPLER_DEFAULT)
    import metalchat_amd as mc

    assert mc.SAMPLER_INHERIT == -1
    for method in ("set_row_sampler", "row_sampler", "reset_row_samplers"):
        assert callable(getattr(mc.Batch, method)), method


def test_a_null_batch_is_refused():
    from metalchat_amd import runtime

    b.build_all()
    lib = runtime.capi()
    kind = C.c_int32(5)
    assert lib.mc_row_sampler_set(None, 0, runtime.SAMPLER_GREEDY, 50, 0.6, 0.9) == 1
    assert lib.mc_last_error().decode().startswith("mc_row_sampler_set: "), lib.mc_last_error()
    assert lib.mc_row_sampler_reset(None) == 1
    assert lib.mc_last_error().decode().startswith("mc_row_sampler_reset: "), lib.mc_last_error()
    assert lib.mc_row_sampler_get(None, 0, C.byref(kind), None, None, None) == 1
    assert lib.mc_last_error().decode().startswith("mc_row_sampler_get: "), lib.mc_last_error()
    assert kind.value == 5
