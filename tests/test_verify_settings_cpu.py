"""Verify calls for sampling, masked and penalised rows (include/metalchat_hip.h Part 2m) without a GPU: the two calls are declared,
exported and bound; a null batch and values other than 0 / 1 are refused with the call's prefix; the four kernels are in the code
object and keep nothing in private memory; and the plan (csrc/batch_plan.h plan_verify_pick / plan_verify_logits, in order csrc/batch_call_plan.h
plan_verify_call, through tests/cpp/test_verify_settings_plan, a plain g++ program): the per-packed-row table and the seed indices of segments on rows
(5, 0, 2) of B = 8 with lens (2, 16, 5), the chain and tree `anc` words, a greedy-only call planning exactly plan_verify_head's
launches, the kpad of a call as the largest among the rows IN the call, and with log-probabilities on the two launches between the pick and the
acceptance of a chain and of a tree."""
import ctypes as C
import json
import os
import re
import subprocess

import pytest

import tree_rule as tr
from metalchat_amd import build as b

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
READELF = "/opt/rocm/lib/llvm/bin/llvm-readelf"
CALLS = ["mc_settings_verify_set", "mc_settings_verify_enabled"]
KERNELS = {"mc_vs_topk_candidates_mixed_bfloat": 64, "mc_vs_pick_mixed_bfloat": 1024, "mc_vs_logits_process_bfloat": 256, "mc_vs_count_accepted": 64}
GREEDY, DEFAULT, DRAW, INHERIT = 0, 1, 2, -1
B, LENS, N_PAIRS = 8, [16, 0, 5, 0, 0, 2, 0, 0], 5
CFG = dict(vocab=1312, n_kv_heads=2, head_dim=64, n_layers=3)
NOTHING, NEUTRAL = (INHERIT, 0, 0.0, 0.0), (0, 1.0, 0.0, 0.0)


def ask(lines):
    exe = b.build_verify_settings_plan_test()
    out = subprocess.run([exe], input="".join(line + "\n" for line in lines), capture_output=True, text=True, check=True).stdout
    answers = [json.loads(a) for a in out.split("\n")[:-1]]
    assert len(answers) == len(lines)
    return answers


def call(lens, samplers, logit_rows, *, dec=(GREEDY, 50, 0.6, 0.9), n_pairs=N_PAIRS, parents=None, cfg=CFG, logprobs=None, head_fmt=0):
    """logprobs: the top_n of a batch with log-probabilities on; head_fmt: the weight format of the head (0: plain)"""
    words = [cfg["vocab"], cfg["n_kv_heads"], cfg["head_dim"], cfg["n_layers"], n_pairs, int(parents is not None), int(logprobs is not None), logprobs or 0, head_fmt,
             *dec,
             len(lens), *lens]
    for s in samplers:
        words += list(s)
    for r in logit_rows:
        words += list(r)
    if parents is not None:
        words += [int(p) for row in parents for p in row]
    return "call " + " ".join(repr(float(w)) if isinstance(w, float) else str(int(w)) for w in words)


def test_the_calls_are_declared_exported_and_bound():
    from metalchat_amd import runtime
    import metalchat_amd as mc

    b.build_all()
    text = open(os.path.join(ROOT, "include", "metalchat_hip.h")).read()
    part = text[text.index("Part 2m --"):]
    code = re.sub(r"/\*.*?\*/", "", "/*" + part, flags=re.S)
    so = C.CDLL(os.path.join(ROOT, "metalchat_amd", "lib", "libmetalchat_hip.so"))
    lib = runtime.capi()
    assert re.search(r"\bmc_status\s+mc_settings_verify_set\s*\(\s*mc_batch\s*\*\s*b\s*,\s*int32_t\s+enable\s*\)", code)
    assert re.search(r"\bint32_t\s+mc_settings_verify_enabled\s*\(\s*const\s+mc_batch\s*\*\s*b\s*\)", code)
    i32 = C.c_int32
    for name in CALLS:
        assert hasattr(so, name), name
        assert name in lib._prototypes, name
    assert lib._prototypes["mc_settings_verify_set"] == (i32, [C.c_void_p, i32])
    assert lib._prototypes["mc_settings_verify_enabled"] == (i32, [C.c_void_p])
    assert "Not covered:" in part
    for method in ("set_verify_settings", "verify_settings"):
        assert callable(getattr(mc.Batch, method)), method


def test_a_null_batch_and_other_values_are_refused():
    from metalchat_amd import runtime

    b.build_all()
    lib = runtime.capi()
    assert lib.mc_settings_verify_set(None, 1) == 1
    assert lib.mc_last_error() == b"mc_settings_verify_set: null argument"
    assert lib.mc_settings_verify_enabled(None) == 0
    fake = C.c_void_p(1)   # never dereferenced: the value is checked first
    for bad in (2, -1, 7):
        assert lib.mc_settings_verify_set(fake, bad) == 1
        assert lib.mc_last_error() == b"mc_settings_verify_set: enable must be 0 or 1"
    a = ask(["switch 0", "switch 1", "switch 2", "switch -1"])
    assert a[0] == a[1] == {"ok": True}
    assert a[2] == a[3] == {"refused": "mc_settings_verify_set: enable must be 0 or 1"}


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
    for k, threads in KERNELS.items():
        assert k in fields, k
        assert fields[k] == {".max_flat_workgroup_size": threads, ".private_segment_fixed_size": 0, ".vgpr_spill_count": 0,
                             ".sgpr_spill_count": 0}, (k, fields[k])


def mixed_rows():
    samplers = [NOTHING] * B
    samplers[0] = (DRAW, 50, 0.8, 0.9)
    samplers[2] = (GREEDY, 0, 0.0, 0.0)
    samplers[5] = (DEFAULT, 20, 0.25, 1.0)
    samplers[3] = (DRAW, 128, 1.0, 1.0)   # not in the call
    logit_rows = [NEUTRAL] * B
    logit_rows[2] = (1, 1.0, 0.0, 0.0)
    logit_rows[5] = (0, 1.5, 0.25, 0.5)
    return samplers, logit_rows


def test_the_table_of_segments_on_rows_5_0_2():
    samplers, logit_rows = mixed_rows()
    a, = ask([call(LENS, samplers, logit_rows)])
    table = a["table"]
    assert len(table) == 23
    want = []
    for r, off in ((0, 0), (2, 16), (5, 21)):   # packed in row order
        kind, k = {0: (DRAW, 50), 2: (GREEDY, 0), 5: (DEFAULT, 20)}[r]
        want += [[kind, k, (j * B + r) % N_PAIRS, (2 << j) - 1, r, off] for j in range(LENS[r])]
    assert table == want
    # the seed index is (j * B + r) % n_pairs: not the packed row's, not j's alone, not r's alone
    seeds = [t[2] for t in table]
    assert seeds != [m % N_PAIRS for m in range(23)]
    assert seeds != [j % N_PAIRS for r in (0, 2, 5) for j in range(LENS[r])] and seeds != [r % N_PAIRS for r in (0, 2, 5) for j in range(LENS[r])]
    # the chain anc words: bits 0 .. j
    assert [t[3] for t in table[:16]] == [1, 3, 7, 15, 31, 63, 127, 255, 511, 1023, 2047, 4095, 8191, 16383, 32767, 65535]
    # the launches: process (row 2's mask, row 5's penalties), the two pick launches in place of the argmax, accept, count
    head = a["head"]
    assert [l[0] for l in head] == ["mc_b_rmsnorm_bfloat", "mc_v_head_w_bfloat", "mc_v_argmax_bfloat", "mc_v_accept"]
    assert a["greedy"] is False and a["any"] is True and a["count"] is True
    # the kpad of the call: rows 0 (top_k 50) and 5 (top_k 20) sample -- row 3's 128 is not in the call
    assert a["kpad"] == 64 and a["chunk"] == 512 and a["nlists"] == 3 and a["cap"] == 4096
    assert a["launches"] == [head[0], head[1], ["mc_vs_logits_process_bfloat", 1, 23, 1, 256, 0],
                             ["mc_vs_topk_candidates_mixed_bfloat", 3, 23, 1, 64, 0], ["mc_vs_pick_mixed_bfloat", 1, 23, 1, 1024, 4096 * 8],
                             head[3], ["mc_vs_count_accepted", 3, 1, 1, 64, 0]]
    # without seed pairs every index is 0
    a0, = ask([call(LENS, samplers, logit_rows, n_pairs=0)])
    assert [t[2] for t in a0["table"]] == [0] * 23


def test_a_greedy_only_call_plans_exactly_the_head_of_before():
    greedy_rows = [NOTHING] * B
    greedy_rows[3] = (DRAW, 128, 1.0, 1.0)          # a sampling row outside the call
    logit_rows = [NEUTRAL] * B
    logit_rows[1] = (1, 1.3, 0.0, 0.0)              # a processed row outside the call
    for parents in (None, [tr.chain(16), tr.chain(5), tr.chain(2)]):
        a, = ask([call(LENS, greedy_rows, logit_rows, parents=parents)])
        assert a["greedy"] is True and a["any"] is False and a["count"] is False
        assert a["launches"] == a["head"]
        assert len(a["head"]) == (5 if parents else 4)
    # ... and under a sampling decoder with the rows in the call set to greedy
    rows = [(GREEDY, 0, 0.0, 0.0) if LENS[r] else NOTHING for r in range(B)]
    a, = ask([call(LENS, rows, [NEUTRAL] * B, dec=(DEFAULT, 50, 0.6, 0.9))])
    assert a["greedy"] is True and a["launches"] == a["head"]
    # an inheriting row in the call follows the decoder: the call samples
    a, = ask([call(LENS, [NOTHING] * B, [NEUTRAL] * B, dec=(DRAW, 50, 0.6, 0.9))])
    assert a["greedy"] is False and a["kpad"] == 64 and {t[0] for t in a["table"]} == {DRAW}


def test_kpad_is_the_largest_among_the_rows_in_the_call():
    for top_ks, kpad, chunk in (((1, 3), 4, 512), ((50, 128), 128, 512), ((128, 1), 128, 512), ((33, 64), 64, 512)):
        rows = [NOTHING] * B
        rows[0] = (DRAW, top_ks[0], 0.8, 0.9)
        rows[5] = (DEFAULT, top_ks[1], 0.8, 0.9)
        rows[1] = (DEFAULT, 128, 0.8, 0.9)          # not in the call
        a, = ask([call(LENS, rows, [NEUTRAL] * B)])
        assert (a["kpad"], a["chunk"]) == (kpad, chunk), (top_ks, a["kpad"], a["chunk"])
        assert a["launches"][2] == ["mc_vs_topk_candidates_mixed_bfloat", 3, 23, 1, 64, 0]
    # masks alone: one process launch, the argmax stays, nothing is counted
    lrows = [NEUTRAL] * B
    lrows[0] = (1, 1.0, 0.0, 0.0)
    a, = ask([call(LENS, [NOTHING] * B, lrows)])
    assert [l[0] for l in a["launches"]] == ["mc_b_rmsnorm_bfloat", "mc_v_head_w_bfloat", "mc_vs_logits_process_bfloat", "mc_v_argmax_bfloat", "mc_v_accept"]


def test_a_tree_takes_depths_for_the_seed_and_the_nodes_anc_words():
    #   0 - 1 - 3 - 5
    #     \ 2 - 4          (siblings 1 | 2 share a pair, as 3 | 4 do)
    parents = [[-1, 0, 0, 1, 2, 3], tr.chain(5), [-1, 0]]
    lens = [6, 0, 5, 0, 0, 2, 0, 0]
    samplers, logit_rows = mixed_rows()
    a, = ask([call(lens, samplers, logit_rows, parents=parents)])
    depths, anc = tr.depths(parents[0]), tr.anc_masks(parents[0])
    assert depths == [0, 1, 1, 2, 2, 3] and anc == [1, 3, 5, 11, 21, 43]
    assert [t[2:] for t in a["table"][:6]] == [[(d * B + 0) % N_PAIRS, m, 0, 0] for d, m in zip(depths, anc)]
    assert [t[2:] for t in a["table"][6:11]] == [[(j * B + 2) % N_PAIRS, (2 << j) - 1, 2, 6] for j in range(5)]
    assert [l[0] for l in a["launches"]] == ["mc_b_rmsnorm_bfloat", "mc_v_head_w_bfloat", "mc_vs_logits_process_bfloat", "mc_vs_topk_candidates_mixed_bfloat",
                                             "mc_vs_pick_mixed_bfloat", "mc_tv_accept", "mc_vs_count_accepted", "mc_tv_compact_bfloat"]


def test_log_probabilities_sit_between_the_pick_and_the_accept():
    """vocab 1312: one chunk of 2048 logits (abi.h LOGPROB_CHUNK), a part per (chunk, packed row), then one workgroup per packed row; 256 threads"""
    parents = [[-1, 0, 0, 1, 2, 3], tr.chain(5), [-1, 0]]
    lens = [6, 0, 5, 0, 0, 2, 0, 0]
    samplers, logit_rows = mixed_rows()
    lp = [["mc_logprob_parts_bfloat", 1, 13, 1, 256, 0], ["mc_logprob_finish_bfloat", 1, 13, 1, 256, 0]]
    for top_n in (0, 3):
        chain, tree, greedy, off = ask([call(lens, samplers, logit_rows, logprobs=top_n), call(lens, samplers, logit_rows, parents=parents, logprobs=top_n),
                                        call(lens, [NOTHING] * B, [NEUTRAL] * B, logprobs=top_n), call(lens, samplers, logit_rows)])
        names = [l[0] for l in chain["launches"]]
        assert names == ["mc_b_rmsnorm_bfloat", "mc_v_head_w_bfloat", "mc_vs_logits_process_bfloat", "mc_vs_topk_candidates_mixed_bfloat", "mc_vs_pick_mixed_bfloat",
                         "mc_logprob_parts_bfloat", "mc_logprob_finish_bfloat", "mc_v_accept", "mc_vs_count_accepted"]
        assert chain["launches"][5:7] == lp
        names = [l[0] for l in tree["launches"]]
        assert names == ["mc_b_rmsnorm_bfloat", "mc_v_head_w_bfloat", "mc_vs_logits_process_bfloat", "mc_vs_topk_candidates_mixed_bfloat", "mc_vs_pick_mixed_bfloat",
                         "mc_logprob_parts_bfloat", "mc_logprob_finish_bfloat", "mc_tv_accept", "mc_vs_count_accepted", "mc_tv_compact_bfloat"]
        assert tree["launches"][5:7] == lp
        # a greedy call: behind the argmax
        assert greedy["launches"] == greedy["head"][:3] + lp + greedy["head"][3:]
        # ... and every other launch is the one of the call without them
        assert [l for l in chain["launches"] if l not in lp] == off["launches"]
