"""QLoRA rows (include/metalchat_hip.h Part 2i) without a GPU: the header carries the part; every kernel it adds -- the int8 GEMVs,
the int8 head and the _l forms with a LoRA adaptor's term -- is in the code object with no private segment, no spills and the LDS of
its family; the twelve GEMVs and two heads that were there keep theirs; and the arguments that need no device are refused."""
import ctypes as C
import os

import metalchat_amd as mc
from test_wide_batch_cpu import kernel_metadata

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FMTS, EPIS = ("i4", "i8", "w"), (0, 1, 2)
# the slice sums: [8 slices][64 lanes] of 16 bytes, times the 4 / 8 column groups of the wide kernels / the head
LDS = {"mc_b_gemv": 8 * 64 * 16, "mc_wb_gemv": 8 * 4 * 64 * 16,
       "mc_v_head": 8 * 8 * 64 * 16, "mc_vhead": 8 * 8 * 64 * 16}
NEW = ([f"{k}_i8_bfloat_e{e}" for k in ("mc_b_gemv", "mc_wb_gemv") for e in EPIS]
       + [f"{k}_{f}_bfloat_e{e}_l" for k in ("mc_b_gemv", "mc_wb_gemv") for f in FMTS for e in EPIS] + ["mc_vhead_i8_bfloat"])
OLD = [f"{k}_{f}_bfloat_e{e}" for k in ("mc_b_gemv", "mc_wb_gemv") for f in ("i4", "w") for e in EPIS] + ["mc_v_head_i4_bfloat", "mc_v_head_w_bfloat"]


def test_the_header_carries_part_2i():
    text = open(os.path.join(ROOT, "include", "metalchat_hip.h")).read()
    assert "Part 2i" in text and "LoRA rank must be a multiple of 16" in text
    assert text.index("Part 2h -- wide batches") < text.index("Part 2i -- QLoRA rows")


def test_the_kernels_are_in_the_code_object_without_private_memory():
    assert len(NEW) == 6 + 18 + 1 and len(OLD) == 14
    fields = kernel_metadata()
    missing = [n for n in NEW + OLD if n not in fields]
    assert not missing, missing
    for n in NEW + OLD:
        f = fields[n]
        assert f[".private_segment_fixed_size"] == 0 and f[".vgpr_spill_count"] == 0 and f[".sgpr_spill_count"] == 0, (n, f)
        assert f[".group_segment_fixed_size"] == next(v for k, v in LDS.items() if n.startswith(k + "_")), (n, f)


def test_create_refuses_without_a_device():
    lib = mc.capi()
    h = C.c_void_p()
    assert lib.mc_wide_batch_create(None, 17, C.byref(h)) == 1
    assert b"mc_wide_batch_create: null argument" in lib.mc_last_error()
    fake = C.c_void_p(1)
    assert lib.mc_wide_batch_create(fake, 17, None) == 1
    assert b"mc_wide_batch_create: null argument" in lib.mc_last_error()
    for bad in (0, 65):
        assert lib.mc_wide_batch_create(fake, bad, C.byref(h)) == 1, bad
        assert b"mc_wide_batch_create: batch must lie in [1, 64]" in lib.mc_last_error()
    assert lib.mc_batch_create(fake, 9, C.byref(h)) == 1
    assert b"mc_batch_create: batch must lie in [1, 8]" in lib.mc_last_error()
    assert not h.value
