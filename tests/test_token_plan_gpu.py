"""The decode token as launched, pinned: for every case of tests/golden/decode_token_plans.json -- the smallest models at which each GEMV family is
taken, one block of every BASELINE shape at four contexts, and on a llama and a gemma3 decoder the taps, the switches that change the sequence, the
three samplers, an int8 embedding and the stages of a split -- the launch logs of step(1, 0), step(-1, 1) and generate(3, 0, 4) name the kernels, in
the order, that the commit the golden names launched; the generate's tokens and the logits behind it are the same bits.  What the plan says without a
device (csrc/token_plan.h): test_token_plan_cpu.py.

The cases with `recorded_under` were recorded with MC_LAZY_PICK=0 added (test_token_plan_cpu.py says why); here they run under their own switches."""
import pytest

from token_plan_observe import observe
from token_plan_program import G

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", sorted(G["cases"]))
def test_token_launches_tokens_and_logits_are_the_recorded_ones(acc, case):
    if G["cus"] != acc.compute_units():
        pytest.skip(f"the golden was recorded on {G['cus']} compute units, this device has {acc.compute_units()}: the grids, and with them the forms, differ")
    c = G["cases"][case]
    got = observe(acc, c)
    assert got.pop("handoff_fallbacks") == 0
    for k in ("step0", "step1", "generate", "tokens", "logits_sha256"):
        assert got.get(k) == c.get(k), (case, k, "recorded from", G["recorded_from"], "under", c["recorded_under"])
