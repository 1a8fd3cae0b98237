"""Wide batches (mc_wide_batch_create, include/metalchat_hip.h Part 2h) without a GPU: the entry point is in the header, exported
and bound; the six mc_wb_gemv_* kernels are in the code object and keep nothing in private memory; and the arguments that need
no device are refused."""
import ctypes as C
import os
import re
import subprocess

import pytest

import metalchat_amd as mc
from metalchat_amd import build as b

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
READELF = "/opt/rocm/lib/llvm/bin/llvm-readelf"
WIDE_KERNELS = [f"mc_wb_gemv_{f}_bfloat_e{e}" for f in ("i4", "w") for e in (0, 1, 2)]


def test_the_entry_point_is_in_the_header_exported_and_bound():
    text = open(os.path.join(ROOT, "include", "metalchat_hip.h")).read()
    assert re.search(r"\bmc_status\s+mc_wide_batch_create\s*\(\s*mc_decoder\s*\*\s*d,\s*int32_t\s+batch,\s*mc_batch\s*\*\*\s*out\s*\)\s*;", text)
    assert "Part 2h" in text
    lib = mc.capi()
    assert "mc_wide_batch_create" in lib._prototypes
    getattr(lib, "mc_wide_batch_create")  # exported by libmetalchat_hip.so


def kernel_metadata():
    hsaco, _ = b.build_all()
    if not os.path.exists(READELF):
        pytest.skip("no llvm-readelf")
    out = subprocess.check_output([READELF, "--notes", hsaco], text=True)
    name, lds, fields = None, 0, {}
    for line in out.splitlines():
        line = line.strip()
        if line.startswith((".", "-")):
            key, _, val = line.lstrip("- ").partition(":")
            key, val = key.strip(), val.strip()
            if key == ".group_segment_fixed_size":   # (a kernel's keys come in alphabetical order: this one before its .name)
                lds = int(val)
            elif key == ".name":
                name = val
                fields[name] = {".group_segment_fixed_size": lds}
            elif name and key in (".private_segment_fixed_size", ".vgpr_spill_count", ".sgpr_spill_count"):
                fields[name][key] = int(val)
    return fields


def test_the_wide_kernels_are_in_the_code_object_without_private_memory():
    fields = kernel_metadata()
    missing = [n for n in WIDE_KERNELS if n not in fields]
    assert not missing, missing
    for n in WIDE_KERNELS:
        f = fields[n]
        assert f[".private_segment_fixed_size"] == 0 and f[".vgpr_spill_count"] == 0 and f[".sgpr_spill_count"] == 0, (n, f)
        # the slice sums of ONE weight tile: [8 slices][4 column groups][64 lanes] of 16 bytes
        assert f[".group_segment_fixed_size"] == 8 * 4 * 64 * 16, (n, f)


def test_create_refuses_without_a_device():
    lib = mc.capi()
    h = C.c_void_p()
    assert lib.mc_wide_batch_create(None, 4, C.byref(h)) == 1
    assert b"mc_wide_batch_create: null argument" in lib.mc_last_error()
    fake = C.c_void_p(1)
    assert lib.mc_wide_batch_create(fake, 4, None) == 1
    assert b"mc_wide_batch_create: null argument" in lib.mc_last_error()
    # the batch size is checked before anything else of the decoder is looked at
    for bad in (0, -1, 65, 1000):
        assert lib.mc_wide_batch_create(fake, bad, C.byref(h)) == 1, bad
        assert b"mc_wide_batch_create: batch must lie in [1, 64]" in lib.mc_last_error()
    assert not h.value
