"""Which kernel a decode GEMV takes, with its grid, workgroup size and LDS bytes, pinned without a GPU: plan_gemv() (csrc/gemv_plan.h) is pure
integer arithmetic, so tests/cpp/test_gemv_plan -- a plain g++ program over that header -- is asked every decision recorded in
tests/golden/decode_gemv_plans.json and has to give the recorded answer in every field.  The recording is of the gemv() of the commit the file
names, the one in front of plan_gemv, on the device it names (test_gemv_plan_gpu.py `record`): an edit of the priority list, of the one-workgroup-per-CU
grid or of an LDS size shows up here as a diff, not as a timing or a wrong sum on one model shape."""
import json
import os
import re
import subprocess

import pytest

from metalchat_amd import build as b

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "decode_gemv_plans.json")
with open(GOLDEN) as f:
    G = json.load(f)
assert G["plan_fields"] == ["fmt", "out", "in", "group", "lora_cols", "pro", "epi", "tb", "qmode", "cus", "name", "wgs", "block", "lds"]
SUFFIX = re.compile(r"^mc_gemv_(?:i4|i8|w)_(?:bfloat|float)(?:_(fast|m4d|m4|lin\d+k4|lin3s|lin\d+|ling\d+))?(?:_dbg[a-z]+)?_p\d_e\d$")


def family(name):
    """the family a recorded kernel name belongs to (gemv_plan.h gemv_family), by the suffix the host writes"""
    s = SUFFIX.match(name).group(1)
    if s is None or s in ("fast", "m4", "m4d"):
        return s or "classic"
    return "lin_k4" if s.endswith("k4") else "lin_split" if s == "lin3s" else "ling" if s.startswith("ling") else "lin"


def ask(lines):
    exe = b.build_gemv_plan_test()
    out = subprocess.run([exe], input="".join(line + "\n" for line in lines), capture_output=True, text=True, check=True).stdout
    answers = out.split("\n")[:-1]
    assert len(answers) == len(lines)
    return answers


@pytest.fixture(scope="module")
def answers():
    """{case: [the program's line for each recorded plan of the case]}: one run over the whole golden"""
    lines, owner = [], []
    for case, c in sorted(G["cases"].items()):
        switches = " ".join(f"{k}={v}" for k, v in sorted(c["options"].items()))
        for p in c["plans"]:
            lines.append(" ".join(str(x) for x in p[:10]) + " " + switches)
            owner.append(case)
    out = {case: [] for case in G["cases"]}
    for case, a in zip(owner, ask(lines)):
        out[case].append(a)
    return out


@pytest.mark.parametrize("case", sorted(G["cases"]))
def test_plan_is_the_recorded_one(answers, case):
    plans = G["cases"][case]["plans"]
    assert plans and len(answers[case]) == len(plans)
    # every name the case launched or named is a recorded plan
    names = {p[10] for p in plans}
    assert set(G["cases"][case].get("step", [])) <= names and set(G["cases"][case]["which"].values()) <= names
    for p, got in zip(plans, answers[case]):
        name, wgs, block, lds = p[10:]
        assert got == f"{name} {wgs} {block} {lds} {family(name)}", (case, p, "recorded from", G["recorded_from"])


def test_recording_covers_every_family_and_the_grid_rules():
    """what the recording is there for, asked of the golden itself: a re-recording that lost a family or a grid rule fails here"""
    plans = {case: c["plans"] for case, c in G["cases"].items()}
    seen = {family(p[10]) for ps in plans.values() for p in ps}
    assert seen == {"classic", "fast", "m4", "m4d", "lin", "lin_k4", "lin_split", "ling"}, seen
    cus = G["cus"]

    def wgs(case, pattern):
        got = {p[11] for p in plans[case] if re.search(pattern, p[10])}
        assert len(got) == 1, (case, pattern, got)
        return got.pop()

    # plain bfloat wo / w2 (2048 rows = 1024 pairs, fewer than half the waves of a full grid): one ROW per wave unless MC_LING_HALF=0
    for k in (r"_ling4_p3_e1$", r"_ling11_p0_e1$"):
        assert wgs("bf16", k) == 2 * wgs("bf16-nohalf", k) == min(cus, 2048 // 8), k
    # the K-split kernel runs on every CU; the kernel it replaces on one pair per wave
    assert wgs("i4-k4", r"_lin12k4_p0_e1$") == cus and wgs("i4-k4-off", r"_lin12_p0_e1$") == 1024 // 8
    # the switches that only move the grid or the workgroup
    assert {p[12] for p in plans["i4-lin-gemv_block512"]} == {512} and {p[12] for p in plans["i4-lin"]} == {512}
    assert {p[12] for p in plans["i4-lin-gemv_lin0"]} == {256}


def test_partial_sum_prologue_without_a_linear_order_kernel_is_an_error():
    # int8 w2 of 14 KiB rows under MC_GEMV_LING=0, asked with the partial-sum prologue
    assert ask([f"1 4096 14336 32 0 3 1 2 0 {G['cus']} gemv_ling=0"]) == ["error: gemv: the partial-sum prologue exists for the linear-order kernels only"]
