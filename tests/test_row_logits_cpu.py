"""Row logit processors (include/metalchat_hip.h Part 2l) without a GPU: the eight calls are declared, exported and bound, a null
batch is refused by each with its prefix, the two kernels are in the code object and keep nothing in private memory, and the
rule (tests/logits_rule.py) itself: the identity of the neutral setting, hand-computed cases, and that a masked row never samples
a banned token through the oracle's default sampler."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import logits_rule as lr
from metalchat_amd import build as b
from oracle import mc_oracle as mo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
READELF = "/opt/rocm/lib/llvm/bin/llvm-readelf"
BF16 = 0
CALLS = ["mc_row_mask_set", "mc_row_mask_get", "mc_row_penalty_set", "mc_row_penalty_get", "mc_row_penalty_count",
         "mc_row_penalty_counts", "mc_row_penalty_clear", "mc_row_logits_reset"]
KERNELS = ["mc_b_logits_process_bfloat", "mc_b_logits_process_rows_bfloat"]


def bf(x):
    return mo.to_bf16(np.asarray(x, np.float32))


def f(bits):
    return mo.from_bf16(bits)


def test_the_calls_are_declared_exported_and_bound():
    from metalchat_amd import runtime
    import metalchat_amd as mc

    b.build_all()
    text = open(os.path.join(ROOT, "include", "metalchat_hip.h")).read()
    part = text[text.index("Part 2l"):]
    code = re.sub(r"/\*.*?\*/", "", "/*" + part, flags=re.S)
    so = C.CDLL(os.path.join(ROOT, "metalchat_amd", "lib", "libmetalchat_hip.so"))
    lib = runtime.capi()
    for name in CALLS:
        assert re.search(r"\bmc_status\s+" + name + r"\s*\(", code), name
        assert hasattr(so, name), name
        assert name in lib._prototypes, name
    assert "Not covered:" in part
    for method in ("set_row_mask", "row_mask", "set_row_penalties", "row_penalties", "count_row_tokens", "row_token_counts",
                   "clear_row_counts", "reset_row_logits"):
        assert callable(getattr(mc.Batch, method)), method


def test_a_null_batch_is_refused_by_each_call():
    from metalchat_amd import runtime

    b.build_all()
    lib = runtime.capi()
    words, one, x = (C.c_uint32 * 4)(1, 0, 0, 0), C.c_int32(5), C.c_float(7.0)
    ids = (C.c_int32 * 2)(1, 2)
    calls = {
        "mc_row_mask_set": (None, 0, words, 4),
        "mc_row_mask_get": (None, 0, C.byref(one), None, 0),
        "mc_row_penalty_set": (None, 0, 1.2, 0.1, 0.1),
        "mc_row_penalty_get": (None, 0, C.byref(x), None, None),
        "mc_row_penalty_count": (None, 0, ids, 2),
        "mc_row_penalty_counts": (None, 0, ids),
        "mc_row_penalty_clear": (None, 0),
        "mc_row_logits_reset": (None,),
    }
    assert sorted(calls) == sorted(CALLS)
    for name, args in calls.items():
        assert getattr(lib, name)(*args) == 1, name
        assert lib.mc_last_error().decode().startswith(name + ": "), (name, lib.mc_last_error())
    assert one.value == 5 and x.value == 7.0 and list(ids) == [1, 2]


def test_the_kernels_are_in_the_code_object_and_keep_nothing_in_private_memory():
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
    for k in KERNELS:
        assert k in fields, k
        assert fields[k] == {".max_flat_workgroup_size": 256, ".private_segment_fixed_size": 0, ".vgpr_spill_count": 0,
                             ".sgpr_spill_count": 0}, (k, fields[k])


def random_bits(rng, n):
    """random bfloat16 rows of both signs with zeros and -0.0 planted"""
    bits = bf(rng.normal(0, 3, n))
    bits[rng.integers(0, n, n // 16)] = 0x0000
    bits[rng.integers(0, n, n // 16)] = 0x8000
    return bits


def test_the_neutral_setting_is_the_identity():
    rng = np.random.default_rng(21)
    for n in (130, 2056):
        bits = random_bits(rng, n)
        assert (bits == 0x8000).any() and (bits == 0).any() and (f(bits) > 0).any() and (f(bits) < 0).any()
        counts = rng.integers(0, 4, n)
        assert np.array_equal(lr.process(bits), bits)
        assert np.array_equal(lr.process(bits, counts), bits)
        assert np.array_equal(lr.process(bits, counts, None, 1.0, 0.0, 0.0), bits)
        assert np.array_equal(lr.process(bits, counts, np.ones(n, bool), 1.0, 0.0, 0.0), bits)
        # penalties with no counts touch nothing either
        assert np.array_equal(lr.process(bits, np.zeros(n, np.int32), None, 1.5, 0.25, 0.5), bits)


def test_hand_computed_cases():
    # rep = 2 (inv_rep = 0.5), freq = 0.25, pres = 0.5: all exact in bfloat16
    x = bf([4.0, -4.0, 0.0, 4.0, -4.0, 0.0, 4.0, -0.0])
    c = np.array([1, 1, 1, 3, 3, 3, 0, 0])
    #   4 * 0.5 - (0.25 + 0.5) = 1.25      -4 * 2 - 0.75 = -8.75       0 * 2 - 0.75 = -0.75
    #   4 * 0.5 - (0.75 + 0.5) = 0.75      -4 * 2 - 1.25 = -9.25       0 * 2 - 1.25 = -1.25      uncounted: untouched
    want = bf([1.25, -8.75, -0.75, 0.75, -9.25, -1.25, 4.0, -0.0])
    got = lr.process(x, c, None, 2.0, 0.25, 0.5)
    assert np.array_equal(got, want), (f(got), f(want))
    assert got[7] == 0x8000
    # each penalty alone
    assert np.array_equal(lr.process(x, c, None, 2.0, 0.0, 0.0), bf([2.0, -8.0, 0.0, 2.0, -8.0, 0.0, 4.0, -0.0]))
    assert np.array_equal(lr.process(x, c, None, 1.0, 0.25, 0.0), bf([3.75, -4.25, -0.25, 3.25, -4.75, -0.75, 4.0, -0.0]))
    assert np.array_equal(lr.process(x, c, None, 1.0, 0.0, 0.5), bf([3.5, -4.5, -0.5, 3.5, -4.5, -0.5, 4.0, -0.0]))
    # a mask: a banned token is -inf whatever its count, an allowed one follows the penalties
    allowed = np.array([1, 0, 1, 0, 1, 1, 0, 1], bool)
    got = lr.process(x, c, allowed, 2.0, 0.25, 0.5)
    assert np.array_equal(got, np.where(allowed, want, 0xFF80))
    assert np.isneginf(f(got)[~allowed]).all()
    # ties of bfloat16 (8 bits of significand: steps of 2^-7 in [1, 2)): 1 + 2^-8 lies between 1 and 1 + 2^-7 and goes to the even
    # 1; 1 + 3 * 2^-8 lies between 1 + 2^-7 (odd) and 1 + 2^-6 (even) and goes up
    y = bf([1.0, 1.0])
    for pres, want_v in ((-2.0 ** -8, 1.0), (-3 * 2.0 ** -8, 1.0 + 2.0 ** -6)):
        got = lr.process(y, np.array([1, 0]), None, 1.0, 0.0, pres)
        exact = np.float32(1.0) - np.float32(pres)
        assert f(bf([exact]))[0] != exact   # (half way between two bfloat16 values)
        assert f(got)[0] == np.float32(want_v) and got[1] == y[1], (pres, f(got))


def test_a_masked_row_never_samples_a_banned_token():
    """200 random cases through the oracle's make_default_sampler: N = 2056, 1 to 500 allowed tokens, top_k 1 to 128, temperature 0.25 to
    4, top_p 0 to 1.  With at least one token allowed no banned token (-inf) may be returned."""
    rng = np.random.default_rng(2056)
    N, banned_picks = 2056, 0
    for case in range(200):
        bits = bf(np.clip(rng.normal(0, 2, N), -9.0, 9.0))
        allowed = np.zeros(N, bool)
        allowed[rng.choice(N, int(rng.integers(1, 501)), replace=False)] = True
        y = lr.process(bits, None, allowed)
        tok = mo.sample_default(BF16, y, top_k=int(rng.integers(1, 129)), temperature=float(rng.uniform(0.25, 4.0)),
                                top_p=float(rng.uniform(0.0, 1.0)), init_state=int(rng.integers(0, 2 ** 31)),
                                init_seq=int(rng.integers(0, 2 ** 31)))
        banned_picks += 0 if 0 <= tok < N and allowed[tok] else 1
    assert banned_picks == 0, f"{banned_picks} of 200 picks were banned tokens"


def test_mask_words_place_token_t_at_bit_t_mod_32():
    allowed = np.zeros(130, bool)
    allowed[[0, 31, 32, 129]] = True
    w = lr.mask_words(allowed)
    assert w.shape == (5,) and list(w) == [0x80000001, 1, 0, 0, 2]
