"""The decode attention block as launched, pinned: for every BASELINE shape at max_seq_len 1024, 2048, 4096 and 8192 -- decoders of one block (gemma3:
two) and a vocabulary of 512 -- the mc_attn_* launches of one eager token and what gemv_kernel_name("attn") answers are the ones recorded on the device
from the build of the commit tests/golden/decode_block_plans.json names, the one in front of csrc/block_plan.h (tools/experiments/block_plan_record.py
`device`).  An edit of plan_block's priority list shows up as a diff of kernel names on the model it moves; form, ranges, grid and flags of the
same recording are pinned without a GPU by test_block_plan_cpu.py.  No numeric comparison: the parity suite holds every one of these kernels to the oracle."""
import json
import os

import pytest

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "decode_block_plans.json")
with open(GOLDEN) as f:
    G = json.load(f)


@pytest.mark.parametrize("case", sorted(G["device_cases"]))
def test_attention_block_launches_are_the_recorded_ones(acc, case):
    import metalchat_amd as mc

    if G["cus"] != acc.compute_units():
        pytest.skip(f"the golden was recorded on {G['cus']} compute units, this device has {acc.compute_units()}: the grids, and with them the forms, differ")
    c = G["device_cases"][case]
    dec = mc.Decoder(acc, **c["cfg"])
    try:
        dec.init_synthetic(7)
        named = dec.gemv_kernel_name("attn")
        dec.launch_log(True)
        dec.step(1, 0)
        names = [n for n in dec.launched() if n.startswith("mc_attn_")]
        dec.launch_log(False)
        fallbacks = dec.handoff_fallbacks()
    finally:
        dec.release()
    print(case, named, names)
    assert fallbacks == 0, "a hand-off gave up (the device is shared?): the launches are the fall-back's"
    assert names == [launch[0] for launch in c["attn_launches"]], (case, "recorded from", G["recorded_from"])
    assert named == c["attn_name"], (case, "recorded from", G["recorded_from"])
    assert named.split(" + ")[0] == names[0]
