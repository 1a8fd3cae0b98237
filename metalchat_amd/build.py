"""Builds the two native artefacts, in-tree:

  lib/metalchat.hsaco        the gfx950 code object (all device kernels) -- the counterpart of the
                             reference's metalchat.metallib (kernel/CMakeLists.txt:27-49)
  lib/libmetalchat_hip.so    the C-ABI host library (include/metalchat_hip.h)

hipcc cross-compiles gfx950 without a GPU.  `python -m metalchat_amd.build` or build_all().
"""
from __future__ import annotations

import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
LIB = os.path.join(HERE, "lib")
HSACO = os.path.join(LIB, "metalchat.hsaco")
SO = os.path.join(LIB, "libmetalchat_hip.so")

KERNEL_SOURCES = [os.path.join(CSRC, "kernels", f) for f in (
    "metalchat_kernels.hip", "ref_kernels.hip", "gemv_kernels.hip", "decode_kernels.hip", "attn_block_kernels.hip",
    "synth_kernels.hip", "sampler_kernels.hip", "prefill_kernels.hip", "batch_kernels.hip", "packed_kernels.hip", "extend_kernels.hip", "verify_kernels.hip", "wide_kernels.hip", "tree_kernels.hip", "logit_kernels.hip", "logprob_kernels.hip", "common.h", "abi.h", "handoff.h", "gemv.h", "gemv_norm.h", "gemv_ksplit.h", "synth.h", "pf_gemm8.h")]
# the host library: every unit goes into the one hipcc command, units and headers together are what makes it stale
HOST_UNITS = [os.path.join(CSRC, f) for f in ("backend.cc", "decoder.cc", "weights.cc", "prefill.cc", "prefill_blaslt.cc", "pipeline.cc", "batch.cc",
                                               "batch_rows.cc", "batch_cache.cc", "batch_settings.cc", "model_io.cc", "text.cc")]
HOST_HEADERS = [os.path.join(CSRC, f) for f in ("json_min.h", "backend_impl.h", "decoder_impl.h", "decoder_batch.h", "decoder_options.h", "gemv_plan.h", "block_plan.h", "token_plan.h", "prefill_plan.h", "rows_plan.h",
                                                 "batch_plan.h", "batch_call_plan.h", "batch_impl.h", "bf16_host.h", "sampler_plan.h")] + [
    os.path.join(CSRC, "kernels", "synth.h"), os.path.join(CSRC, "kernels", "abi.h"),
    os.path.join(os.path.dirname(HERE), "include", "metalchat_hip.h")]


def _stale(target: str, sources) -> bool:
    if not os.path.exists(target):
        return True
    t = os.path.getmtime(target)
    return any(os.path.getmtime(s) > t for s in sources)


def hipcc() -> str:
    for c in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", "hipcc"):
        if c and (os.path.isabs(c) and os.path.exists(c) or not os.path.isabs(c)):
            return c
    raise RuntimeError("hipcc not found")


def build_kernels(force: bool = False) -> str:
    os.makedirs(LIB, exist_ok=True)
    if force or _stale(HSACO, KERNEL_SOURCES):
        cmd = [hipcc(), "--offload-arch=gfx950", "--genco", "--no-gpu-bundle-output", "-O3",
               "-std=c++17", "-fno-slp-vectorize",
               # a*b+c stays two roundings unless the source says fma: elementwise results then
               # match the CPU oracle (built with -ffp-contract=off) bit for bit
               "-ffp-contract=off", "-o", HSACO, KERNEL_SOURCES[0]]
        subprocess.check_call(cmd, cwd=os.path.join(CSRC, "kernels"))
    return HSACO


def build_host(force: bool = False) -> str:
    os.makedirs(LIB, exist_ok=True)
    if force or _stale(SO, HOST_UNITS + HOST_HEADERS):
        cmd = [hipcc(), "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wno-unused-function",
               *HOST_UNITS, "-ldl", "-o", SO]
        subprocess.check_call(cmd, cwd=CSRC)
    return SO


def _build_cpp_test(name: str, headers, force: bool, link_host: bool) -> str:
    """tests/cpp/<name>: a plain g++ program (no HIP headers), rebuilt when its source or one of `headers` is newer.  link_host: a program above
    the C ABI, linked against the host library; otherwise it stands on device-free headers alone and is compiled with -Wall."""
    root = os.path.dirname(HERE)
    src = os.path.join(root, "tests", "cpp", name + ".cc")
    out = os.path.join(root, "tests", "cpp", name)
    if force or _stale(out, [src, *headers] + ([SO] if link_host else [])):
        cmd = ["g++", "-std=c++17", "-O1"]
        if link_host:
            cmd += ["-I" + os.path.join(root, "include"), src, "-o", out, "-L" + LIB, "-lmetalchat_hip", "-Wl,-rpath," + LIB, "-Wl,-rpath,/opt/rocm/lib", "-pthread"]
        else:
            cmd += ["-Wall", src, "-o", out]
        subprocess.check_call(cmd)
    return out


_ABI_HEADERS = [os.path.join(os.path.dirname(HERE), "include", f) for f in ("metalchat_hip.hpp", "metalchat_hip.h")]
_PLAN_HEADERS = [os.path.join(CSRC, "gemv_plan.h"), os.path.join(CSRC, "decoder_options.h"), _ABI_HEADERS[1]]


def build_shim_test(force: bool = False) -> str:
    """tests/cpp/test_shim: a plain g++ program over include/metalchat_hip.hpp -- host code above the C ABI needs no HIP headers."""
    return _build_cpp_test("test_shim", _ABI_HEADERS, force, True)


def build_model_io_test(force: bool = False) -> str:
    """tests/cpp/test_model_io: host-only C++ test of the document / options part of the ABI."""
    return _build_cpp_test("test_model_io", _ABI_HEADERS, force, True)


def build_text_test(force: bool = False) -> str:
    """tests/cpp/test_text: host-only C++ test of the text / interpreter-framing classes of the shim."""
    return _build_cpp_test("test_text", _ABI_HEADERS, force, True)


# The eight plan programs are no part of build_all(): nothing of the package needs them, their CPU tests build them (a second or two) when they run.
def build_gemv_plan_test(force: bool = False) -> str:
    """tests/cpp/test_gemv_plan: plan_gemv() (csrc/gemv_plan.h) from the command line -- no HIP and no host library."""
    return _build_cpp_test("test_gemv_plan", _PLAN_HEADERS, force, False)


def build_block_plan_test(force: bool = False) -> str:
    """tests/cpp/test_block_plan: plan_block() (csrc/block_plan.h) from the command line -- no HIP and no host library."""
    return _build_cpp_test("test_block_plan", [os.path.join(CSRC, "block_plan.h"), *_PLAN_HEADERS], force, False)


def build_token_plan_test(force: bool = False) -> str:
    """tests/cpp/test_token_plan: plan_token() (csrc/token_plan.h) from the command line -- no HIP and no host library."""
    headers = [os.path.join(CSRC, f) for f in ("token_plan.h", "block_plan.h", "sampler_plan.h")] + [os.path.join(CSRC, "kernels", "abi.h"), *_PLAN_HEADERS]
    return _build_cpp_test("test_token_plan", headers, force, False)


def build_prefill_plan_test(force: bool = False) -> str:
    """tests/cpp/test_prefill_plan: the prompt plan (csrc/prefill_plan.h) from the command line -- no HIP and no host library."""
    return _build_cpp_test("test_prefill_plan", [os.path.join(CSRC, "prefill_plan.h"), *_PLAN_HEADERS], force, False)


def build_rows_plan_test(force: bool = False) -> str:
    """tests/cpp/test_rows_plan: the tables of the rows passes (csrc/rows_plan.h) from the command line -- no HIP and no host library."""
    return _build_cpp_test("test_rows_plan", [os.path.join(CSRC, "rows_plan.h"), os.path.join(CSRC, "kernels", "abi.h")], force, False)


def build_batch_plan_test(force: bool = False) -> str:
    """tests/cpp/test_batch_plan: what a batch launches (csrc/batch_plan.h, in order: batch_call_plan.h) from the command line -- no HIP and no host library."""
    headers = [os.path.join(CSRC, f) for f in ("batch_plan.h", "batch_call_plan.h", "rows_plan.h", "bf16_host.h", "sampler_plan.h")] + [os.path.join(CSRC, "kernels", "abi.h"), _ABI_HEADERS[1]]
    return _build_cpp_test("test_batch_plan", headers, force, False)


def build_draw_plan_test(force: bool = False) -> str:
    """tests/cpp/test_draw_plan: the pick of a batch with MC_SAMPLER_DRAW rows (csrc/batch_plan.h plan_head) -- no HIP and no host library."""
    headers = [os.path.join(CSRC, f) for f in ("batch_plan.h", "batch_call_plan.h", "rows_plan.h", "bf16_host.h", "sampler_plan.h")] + [os.path.join(CSRC, "kernels", "abi.h"), _ABI_HEADERS[1]]
    return _build_cpp_test("test_draw_plan", headers, force, False)


def build_verify_settings_plan_test(force: bool = False) -> str:
    """tests/cpp/test_verify_settings_plan: the head of a verify call whose rows carry settings (csrc/batch_plan.h plan_verify_pick /
    plan_verify_logits) -- no HIP and no host library."""
    headers = [os.path.join(CSRC, f) for f in ("batch_plan.h", "batch_call_plan.h", "rows_plan.h", "bf16_host.h", "sampler_plan.h")] + [os.path.join(CSRC, "kernels", "abi.h"), _ABI_HEADERS[1]]
    return _build_cpp_test("test_verify_settings_plan", headers, force, False)


def build_logprob_plan_test(force: bool = False) -> str:
    """tests/cpp/test_logprob_plan: the two launches behind a pick of a batch with log-probabilities on (csrc/batch_plan.h plan_logprobs) -- no HIP
    and no host library."""
    headers = [os.path.join(CSRC, f) for f in ("batch_plan.h", "batch_call_plan.h", "rows_plan.h", "bf16_host.h", "sampler_plan.h")] + [os.path.join(CSRC, "kernels", "abi.h"), _ABI_HEADERS[1]]
    return _build_cpp_test("test_logprob_plan", headers, force, False)


def build_all(force: bool = False):
    r = build_kernels(force), build_host(force)
    build_shim_test(force)
    build_model_io_test(force)
    build_text_test(force)
    return r


if __name__ == "__main__":
    print(build_all("--force" in sys.argv))
