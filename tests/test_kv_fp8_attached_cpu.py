"""Packed chunks and verify on attached rows of an fp8 batch (include/metalchat_hip.h Part 2u) without a GPU: the code object holds exactly the four
mc_ax8_* kernels (kernels/kv8_attached_kernels.hip), none with a private segment or spills."""
import re
import subprocess

from metalchat_amd import build as b

KERNELS = {f"mc_ax8_{k}_bfloat_hd{hd}" for k in ("sums", "pv") for hd in (64, 128)}


def test_the_code_object_holds_the_kernels_and_none_keeps_private_memory():
    out = subprocess.check_output(["/opt/rocm/lib/llvm/bin/llvm-readelf", "--notes", b.build_all()[0]], text=True)
    kernels = {m.group(1): k for k in out.split(".agpr_count")[1:] if (m := re.search(r"\.name:\s+(mc_ax8_\w*)", k))}
    assert set(kernels) == KERNELS
    for k in kernels.values():
        assert [int(v) for v in re.findall(r"\.(?:private_segment_fixed_size|[sv]gpr_spill_count):\s+(\d+)", k)] == [0, 0, 0], k
