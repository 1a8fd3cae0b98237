"""What the decode launches for the attention half of a block -- one of nine forms and five attention tails, with its kernel, ranges, grid, hand-off
mode and the GEMVs around it -- pinned without a GPU: plan_block() (csrc/block_plan.h) is integer arithmetic and string building, so
tests/cpp/test_block_plan, a plain g++ program over that header, is asked every decision recorded in tests/golden/decode_block_plans.json and has to
give the recorded answer in every field.  The recording is of the MEMBER mc_decoder::plan_block of the commit the file names, the one in front of
block_plan.h, asked without a device through tools/experiments/block_plan_record.patch with the occupancy answers real decoders got on the device
it names: an edit of the priority list shows up here as a diff, not as a timing or a wrong kernel on one model shape.

The finding the recording made: the step's retry asks `attn_fused() || attn_fused_t2()` -- block_uses_handoffs() -- as a
stand-in for "the form has a hand-off".  It is not one.  The forms gated by handoffs_ok() alone, whose ranges need only fit one workgroup per CU, are
taken where neither holds: 102 of the 1568 records, among them Gemma-7B at max_seq_len 4096 under the default switches (64 x 16 ranges of 64 slots
are more than two workgroups per CU, head_dim 256 has no mc_attn_fused_t2).  test_the_retry_proxy_is_what_was_recorded pins exactly that set."""
import collections
import re

import pytest

from block_plan_program import FIELDS, G, answers, recorded

FORMS = ["qkv_wo_w13_w", "qkv_wo_w", "qkv_wo_i8", "qkv_wo_i4", "qkv_only", "qkv_wo_qkn", "wo_qkn", "wo_i4", "fused", "fused_qkn", "fused_t2", "scores_pv"]
TAILS = {"a": {"wo_qkn"}, "b": {"wo_i4"}, "c": {"fused", "fused_qkn"}, "d": {"fused_t2"}, "e": {"scores_pv"}}
# the forms whose gate is attn_fused() itself (64-slot ranges, up to two 256-thread workgroups per CU) or attn_fused_t2()
GATED_BY_THE_PROXY = {"qkv_wo_w13_w", "qkv_only", "wo_i4", "fused", "fused_qkn", "fused_t2"}
BY_SOURCE = collections.defaultdict(list)
for i, r in enumerate(G["records"]):
    BY_SOURCE[G["sources"][r[6]].split(":")[0]].append(i)


@pytest.mark.parametrize("source", sorted(BY_SOURCE))
def test_plan_is_the_recorded_one(source):
    got = answers()
    assert BY_SOURCE[source]
    for i in BY_SOURCE[source]:
        r = G["records"][i]
        assert got[i] == G["answers"][r[5]], (G["sources"][r[6]], G["options"][r[4]], G["models"][r[1]], dict(zip(FIELDS, got[i].split())), recorded(r),
                                               "recorded from", G["recorded_from"])


def test_recording_covers_every_form_and_every_tail():
    seen = {recorded(r)["form"] for r in G["records"]}
    assert seen == set(FORMS), set(FORMS) - seen
    for tail, forms in TAILS.items():
        rows = [recorded(r) for r in G["records"] if recorded(r)["form"] in forms]
        assert rows and all(a["qkv_gemv"] == "1" for a in rows), tail
    # ... the sweep the issue names: every BASELINE shape at the four contexts, the partial ranges, the other CU counts, the states
    assert {m[5] for m in G["models"]} == {1024, 2048, 4096, 8192, 2040, 4040}
    assert {e[2] for e in G["envs"]} == {192, 256, 304} and G["cus"] == 256
    assert {e[0] for e in G["envs"]} == {2, 4} and {e[4] for e in G["envs"]} == {1, 2, 255}
    assert {r[3] for r in G["records"]} == {0, 1, 2, 3}
    assert len(G["device_cases"]) == 24 and all(c["attn_launches"] for c in G["device_cases"].values())


def test_wide_ranges_only_over_whole_ranges():
    """_t2 / _t4: 128- / 256-slot ranges only where the cache is whole ranges long"""
    wide = 0
    for r in G["records"]:
        a, S = recorded(r), G["models"][r[1]][5]
        t = re.search(r"_t([24])$", a["name"])
        if t:
            wide += 1
            assert a["form"] != "fused_t2" or a["tiles"] == "2"
            assert int(a["tiles"]) == int(t.group(1)) and S % (64 * int(t.group(1))) == 0, (a, S)
        else:
            assert a["tiles"] == ("2" if a["form"] == "fused_t2" else "1"), a
        if a["form"] == "fused_t2":
            assert S % 128 == 0, (a, S)
    assert wide > 100


def test_the_retry_proxy_is_what_was_recorded():
    """Every case whose form is not scores_pv SHOULD have block_uses_handoffs() true: the retry of mc_decoder_step / mc_decoder_generate keeps the
    state in front of a step only then.  The recording shows where it does not hold (the module's docstring); the behaviour is left alone, and pinned:
    the proxy holds for every form it gates itself, never holds for scores_pv's opposite -- a fallen-back decoder -- and the cases it misses are the
    one-workgroup-per-CU forms whose 64-slot ranges are too many for attn_fused() and whose shape has no mc_attn_fused_t2."""
    missed = collections.Counter()
    for r in G["records"]:
        a, (_, _, KV, hd, _, _), e = recorded(r), G["models"][r[1]], G["envs"][r[2]]
        opts = dict(kv.split("=") for kv in G["options"][r[4]].split())
        if a["form"] == "scores_pv":
            continue
        assert r[3] & 1 and e[5] == 1 and e[0] == 2 and e[4] <= 254, (a, "a form with a hand-off on a decoder that may not take one")
        if a["uses_handoffs"] == "1":
            continue
        assert a["form"] not in GATED_BY_THE_PROXY, a
        # ... and why: more 64-slot workgroups than attn_fused() admits, and no 128-slot attention for this shape (or switched off, or still too many)
        per_cu = min(int(opts.get("attn_fused_max_wgs_per_cu", 2)), e[7] if e[7] >= 0 else 4)
        assert e[3] * KV > per_cu * e[2], (a, e)
        assert opts.get("attn_t2_on") == "0" or e[3] % 2 or hd not in (64, 128) or KV % 8 or e[3] // 2 * KV > per_cu * e[2], (a, e)
        missed[(G["sources"][r[6]], G["options"][r[4]], G["models"][r[1]][5], a["form"])] += 1
    assert sum(missed.values()) == 102, sum(missed.values())
    # under the default switches, on the recording device: Gemma-7B at 4096 slots, both of its blocks' forms
    default = {k: n for k, n in missed.items() if k[0] in ("baseline",) and not k[1]}
    assert default == {("baseline", "", 4096, "qkv_wo_qkn"): 2}, default
