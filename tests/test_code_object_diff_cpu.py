"""tools/code_object_diff.py on the built code object (no GPU needed): a file against itself is "identical" with exit status 0, and a
copy with ONE byte flipped inside the code of one named kernel is reported as exactly that kernel, with a non-zero exit status.
The tool is what a refactor of the kernel sources is held to: the code object it builds is its parent's, byte for byte.
Its other reports -- the resource figures of the metadata note, kernels that only one file has -- are checked on the built code
object (every figure of every kernel is read) and on two three-line code objects compiled here."""
import importlib.util
import os
import shutil
import subprocess
import sys

import pytest

from metalchat_amd import build as b

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "tools", "code_object_diff.py")
READELF = "/opt/rocm/lib/llvm/bin/llvm-readelf"
KERNEL = "mc_gemv_i4_bfloat_lin2_p1_e4"


@pytest.fixture(scope="module")
def hsaco():
    return b.build_kernels()


@pytest.fixture(scope="module")
def tool():
    spec = importlib.util.spec_from_file_location("code_object_diff", TOOL)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def run(a, c):
    return subprocess.run([sys.executable, TOOL, a, c], capture_output=True, text=True)


def test_a_code_object_is_identical_to_itself(hsaco):
    r = run(hsaco, hsaco)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "identical" in r.stdout.splitlines()[2], r.stdout


def test_one_flipped_byte_names_its_kernel(hsaco, tmp_path):
    # the symbol's file offset from the section header of .text: offset of .text + (symbol value - address of .text)
    text = None
    for line in subprocess.check_output([READELF, "--section-headers", "--wide", hsaco], text=True).splitlines():
        f = line.replace("[", " ").replace("]", " ").split()
        if len(f) >= 6 and f[1] == ".text":
            text = (int(f[3], 16), int(f[4], 16), int(f[5], 16))
    assert text is not None
    sym = None
    for line in subprocess.check_output([READELF, "--symbols", "--wide", hsaco], text=True).splitlines():
        f = line.split()
        if len(f) == 8 and f[3] == "FUNC" and f[7] == KERNEL:
            sym = (int(f[1], 16), int(f[2]))
    assert sym is not None, KERNEL
    addr, off, size = text
    value, length = sym
    assert addr <= value and value + length <= addr + size
    at = off + (value - addr) + length // 2
    copy = str(tmp_path / "flipped.hsaco")
    shutil.copyfile(hsaco, copy)
    with open(copy, "r+b") as fh:
        fh.seek(at)
        byte = fh.read(1)[0]
        fh.seek(at)
        fh.write(bytes([byte ^ 0xFF]))
    r = run(hsaco, copy)
    assert r.returncode != 0, r.stdout
    assert "identical" not in r.stdout
    named = [line.split(":")[0] for line in r.stdout.splitlines() if line.startswith("mc_") or ": code differs" in line]
    assert named == [KERNEL], r.stdout
    assert "1 of " in r.stdout.splitlines()[-1], r.stdout


def test_every_resource_figure_of_every_kernel_is_read(hsaco, tool):
    """The metadata note nests lists inside a kernel's entry (.args, .language_version): a parser that takes their `- ` for a new kernel
    loses the figures printed in front of them -- .agpr_count, .group_segment_fixed_size, .kernarg_segment_size."""
    meta, syms = tool.kernel_metadata(hsaco), tool.kernel_symbols(hsaco)
    assert set(meta) == set(syms) and len(meta) > 500, (len(meta), len(syms))
    lacking = {k: [f for f in tool.META_FIELDS if f not in v] for k, v in meta.items() if set(v) != set(tool.META_FIELDS)}
    assert not lacking, lacking
    m = meta[KERNEL]
    # fifteen explicit arguments end at byte 96 (six pointers, three words, two floats, two pointers, a word, a float); the hidden ones follow
    assert m[".kernarg_segment_size"] >= 96 and m[".vgpr_count"] > 0 and m[".sgpr_count"] > 0, m
    assert m[".private_segment_fixed_size"] == 0 and m[".vgpr_spill_count"] == 0 and m[".sgpr_spill_count"] == 0, m
    # a kernel with static LDS and known arguments: bmm_8_bfloat (ref_kernels.hip) takes three 36-byte tensor layouts and three pointers
    assert meta["bmm_8_bfloat"][".kernarg_segment_size"] == 144 and meta["bmm_8_bfloat"][".group_segment_fixed_size"] > 0, meta["bmm_8_bfloat"]


SRC = """#include <hip/hip_runtime.h>
extern "C" __global__ void k_same(float* p) { p[threadIdx.x] += 1.0f; }
extern "C" __global__ void k_lds(float* p) { __shared__ float s[%d]; s[threadIdx.x] = p[threadIdx.x]; __syncthreads(); p[threadIdx.x] = s[63 - threadIdx.x]; }
extern "C" __global__ void %s(float* p) { p[threadIdx.x] *= 2.0f; }
"""


def test_resource_figures_and_kernels_of_one_file_are_reported(tmp_path):
    """Two small code objects: k_same equal in both, k_lds with 256 against 512 bytes of LDS, k_only_a / k_only_b in one file each."""
    objs = []
    for tag, floats in (("a", 64), ("b", 128)):
        src, obj = tmp_path / f"{tag}.hip", tmp_path / f"{tag}.hsaco"
        src.write_text(SRC % (floats, "k_only_" + tag))
        subprocess.check_call([b.hipcc(), "--offload-arch=gfx950", "--genco", "--no-gpu-bundle-output", "-O3", "-o", str(obj), str(src)])
        objs.append(str(obj))
    r = run(*objs)
    assert r.returncode != 0, r.stdout
    lines = r.stdout.splitlines()
    assert "only in A: k_only_a" in lines and "only in B: k_only_b" in lines, r.stdout
    lds = [line for line in lines if line.startswith("k_lds:")]
    assert len(lds) == 1 and ".group_segment_fixed_size 256 / 512" in lds[0], r.stdout
    assert not [line for line in lines if line.startswith("k_same:")], r.stdout
    assert lines[-1].startswith("3 of 4 kernels differ"), r.stdout
