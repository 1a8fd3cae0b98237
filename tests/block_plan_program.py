"""tests/cpp/test_block_plan -- plan_block() of csrc/block_plan.h as a plain g++ program -- asked every decision recorded in
tests/golden/decode_block_plans.json: shared by test_block_plan_cpu.py (the answers) and test_kernel_names_cpu.py (the names)."""
import functools
import json
import os
import subprocess

from metalchat_amd import build as b

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "decode_block_plans.json")
with open(GOLDEN) as f:
    G = json.load(f)
FIELDS = ["form", "name", "tiles", "vsh", "ns", "grid", "fast", "chain_f", "chain_p", "qkv_gemv", "rope_kv", "wo_gemv", "pv_fold", "pv_ranges", "pv_block",
          "pv_reduce", "uses_handoffs"]
assert G["answer_fields"] == FIELDS
assert G["record_fields"] == ["shape (index)", "model (index)", "env (index)", "state", "options (index)", "answer (index)", "source (index)"]


def line(r):
    """the program's input for one record"""
    ints = G["shapes"][r[0]] + G["models"][r[1]] + G["envs"][r[2]] + [r[3] & 1, r[3] >> 1]
    return " ".join(str(x) for x in ints) + " " + G["options"][r[4]]


def recorded(r):
    return dict(zip(FIELDS, G["answers"][r[5]].split()))


@functools.lru_cache(maxsize=None)
def answers():
    """the program's line for every record of the golden, in its order: one run"""
    exe = b.build_block_plan_test()
    text = "".join(line(r) + "\n" for r in G["records"])
    out = subprocess.run([exe], input=text, capture_output=True, text=True, check=True).stdout.split("\n")[:-1]
    assert len(out) == len(G["records"])
    return out
