"""What a batch launches (metalchat_amd/csrc/batch_plan.h, in order: batch_call_plan.h) without a GPU, through tests/cpp/test_batch_plan (batch_plan_program.py):

  (a) every launch -- name, grid, block, LDS bytes -- of the cases recorded from the commit in front of the header
      (tests/golden/batch_plans.json: mc_decoder::launch wrote them down on an MI355X; the header is never recorded against itself);
  (b) the tile rule of the wide GEMV at real widths, worked from the rule;
  (c) every reason of the admission, reached from an admitted shape by one change, with its text; the shapes of the GPU tests admitted;
  (d) every refusal of a ragged call, the two of a verify call and the lockstep bounds, with their texts;
  (e) every kernel name any of these answers contains, or the plans form over a sweep of their inputs, is a FUNC symbol of the code object.
(a) pins what each launch holds, the order of a call's launches and which plan sits at which place: the lists are batch_call_plan.h's
(plan_batch_token, plan_rows_tail), the ones the batch's one executor walks; that it walks them is what tests/test_batch_call_plan_gpu.py sees.
  (f) with log-probabilities on, the two launches are the last of a token in every pick form, and the process launch sits between the head and the pick.
The texts below are the ones batch.cc carried before its checks moved into the header."""
import json
import os
import struct
import subprocess

import numpy as np

import batch_plan_program as bp
from batch_plan_program import WFMT_I4, WFMT_I8, WFMT_T
from metalchat_amd import build as b

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
READELF = ["/opt/rocm/lib/llvm/bin/llvm-readelf", "/usr/bin/readelf"]
SMALL = dict(dim=1024, n_heads=8, n_kv_heads=2, head_dim=128, ffn_dim=2048, n_layers=1, vocab=2048, max_seq_len=256)
LLAMA32_1B = dict(dim=2048, n_heads=32, n_kv_heads=8, head_dim=64, ffn_dim=8192, n_layers=2, vocab=2048, max_seq_len=256)
LLAMA3_8B = dict(dim=4096, n_heads=32, n_kv_heads=8, head_dim=128, ffn_dim=14336, n_layers=1, vocab=2048, max_seq_len=2048)
SEEN = set()   # the kernel names of the answers asked through ask(): (e) asks (a) to (d) again and looks them up


def ask(lines):
    answers = bp.ask(lines)
    for a in answers:
        SEEN.update(bp.names_in(a))
    return answers


def bf16(x):
    """x rounded to the nearest bfloat16 (ties to even), as a float"""
    u = struct.unpack("<I", struct.pack("<f", x))[0]
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return struct.unpack("<f", struct.pack("<I", u))[0]


# ------------------------------------------------------------------------------------------ (a) the recording
def recorded():
    with open(os.path.join(ROOT, "tests", "golden", "batch_plans.json")) as f:
        return json.load(f)["cases"]


def planned(c):
    """the launches the header plans for a recorded case, from the case's own request"""
    if c["call"] in ("step", "ragged"):
        one = bp.token_launches(c["cfg"], c["linears"], c["B"], cus=c["cus"], tiles_env=c["tiles_env"], ragged_call=c["call"] == "ragged",
                                rolling=bool(c["rolling"]), dec_sampler=c["dec_sampler"], row_samplers=c["row_samplers"], row_logits=c["row_logits"])
        return one * c["n"]
    if c["call"] in ("rows_prefill", "rows_extend"):
        return bp.head_launches(c["cfg"], c["linears"], c["B"], cus=c["cus"], tiles_env=c["tiles_env"])
    assert c["call"] == "verify", c["call"]
    return bp.ask([bp.verify(c["linears"]["output"], c["cfg"], c["M"], c["nseg"], c["tree"])])[0]["launches"]


def test_the_plans_are_the_recorded_launches_field_for_field():
    cases = recorded()
    assert len(cases) == 55
    for c in cases:
        got = planned(c)
        SEEN.update(x[0] for x in got)
        assert len(got) == len(c["launches"]), (c["name"], len(got), len(c["launches"]))
        for i, (g, r) in enumerate(zip(got, c["launches"])):
            assert g == r, (c["name"], i, g, r)


def test_the_recording_covers_the_forms():
    names = {c["name"]: [x[0] for x in c["launches"]] for c in recorded()}
    assert any(n.startswith("mc_wb_gemv_") for n in names["plain-B17-wide-lockstep-step"]) and \
        not any(n.startswith("mc_wb_gemv_") for n in names["plain-B16-wide-lockstep-step"])                 # the threshold between the two GEMVs
    assert "mc_b_rows_begin_rolling" in names["shared-B64-rolling-generate-3"] and "mc_b_rows_begin" in names["shared-B64-ragged-generate-3"]
    assert names["shared-B64-pick-greedy-lockstep"][-1] == "mc_b_argmax_bfloat"
    assert names["shared-B64-pick-decoder-sampler-ragged"][-2:] == ["mc_b_topk_candidates_bfloat", "mc_b_sample_rows_bfloat"]
    for case in ("two-top-k", "one-greedy-row"):
        assert names[f"shared-B64-pick-{case}-lockstep"][-2:] == ["mc_b_topk_candidates_mixed_bfloat", "mc_b_pick_mixed_bfloat"]
    assert "mc_b_logits_process_rows_bfloat" in names["shared-B64-logits-mask-ragged"] and \
        not any("logits_process" in n for n in names["shared-B64-logits-none-ragged"])
    assert "mc_vhead_i8_bfloat" in names["rows-verify-int8-head-B64"] and "mc_tv_compact_bfloat" in names["rows-tree-5-nodes"]


# ------------------------------------------------------------------------------------------ (b) the tile rule
def tiles_by_the_rule(out, most, cus=256):
    """the most of 8, 4, 2 tiles that still gives every CU a workgroup, else 1; at most `most`"""
    for t in (8, 4, 2):
        if t <= most and -(-(out // 16) // t) >= cus:
            return t
    return 1


def test_the_tile_rule_at_real_widths():
    table = [(4096, WFMT_I4, 0, 1), (4096, WFMT_T, 0, 1), (6144, WFMT_I4, 0, 1), (6144, WFMT_T, 0, 1), (14336, WFMT_I4, 0, 2), (14336, WFMT_T, 0, 2),
             (28672, WFMT_I4, 0, 4), (28672, WFMT_T, 0, 4), (128256, WFMT_I4, 0, 8), (128256, WFMT_T, 0, 8), (128256, WFMT_I8, 0, 4),
             (128256, WFMT_I8, 8, 4)]
    lines = [bp.gemv(bp.linear(fmt, out, 4096, 128 if fmt != WFMT_T else 0), 0, 64, 256, env) for out, fmt, env, _ in table]
    for (out, fmt, env, tiles), a in zip(table, ask(lines)):
        assert tiles == tiles_by_the_rule(out, 4 if fmt == WFMT_I8 else 8), (out, fmt)            # the table is the rule's
        name, gx, gy, gz, block, lds = a["launches"][-1]
        assert a["wide"] and name.startswith("mc_wb_gemv_") and (gx, gy, gz, block, lds) == (-(-(out // 16) // tiles), 1, 1, 512, 0), (out, fmt, env, a)
    # an adaptor caps the tiles at 4 as int8 does; the adaptor's own launch is a plain matrix of lora_cols rows
    a = ask([bp.gemv(bp.linear(WFMT_I4, 128256, 4096, 32, 16), 0, 64)])[0]
    assert [x[:2] for x in a["launches"]] == [["mc_wb_gemv_w_bfloat_e0", 1], ["mc_wb_gemv_i4_bfloat_e0_l", -(-(128256 // 16) // 4)]], a
    # up to 16 rows: the one-tile kernel, a workgroup per 16 weight rows, whatever the format and MC_WB_TILES
    for fmt in (WFMT_T, WFMT_I8, WFMT_I4):
        for env in (0, 8):
            a = ask([bp.gemv(bp.linear(fmt, 4096, 4096, 128 if fmt != WFMT_T else 0), 1, 16, 256, env)])[0]
            assert not a["wide"] and a["launches"] == [[f"mc_b_gemv_{'w i8 i4'.split()[fmt]}_bfloat_e1", 4096 // 16, 1, 1, 512, 0]], a


# ------------------------------------------------------------------------------------------ (c) admission
def test_the_shapes_of_the_gpu_tests_are_admitted():
    lines = []
    for cfg in (SMALL, LLAMA32_1B, LLAMA3_8B):
        lines += [bp.admit(cfg, bp.linears_of(cfg), wide) for wide in (False, True)]
        lines += [bp.admit(cfg, bp.linears_of(cfg, WFMT_I4, 128), wide) for wide in (False, True)]
    qlora = bp.linears_of(SMALL, WFMT_I4, 32, 16, head_fmt=WFMT_I8, head_group=0)
    lines += [bp.admit(SMALL, qlora, True, emb_fmt=WFMT_I8), bp.admit(SMALL, bp.linears_of(SMALL, WFMT_I8, 32), True)]
    assert ask(lines) == [{"admitted": True}] * len(lines)


def test_every_reason_of_the_admission_is_reached_by_one_change():
    cfg, base = SMALL, bp.linears_of(SMALL, WFMT_I4, 128)

    def changed(name, **fields):
        lin = {k: dict(v) for k, v in base.items()}
        lin[name].update(fields)
        return lin

    head_text = "the batched GEMV needs out_features % 16 == 0 and in_features % 1024 == 0"
    both = [  # (the request's change, the text) for wide False and True alike
        (dict(family=1), "only llama3 decoders can be batched"),
        (dict(dtype=1), "only bfloat16 decoders can be batched"),
        (dict(layer_end=0), "the decoder must own every layer (a pipeline stage cannot be batched)"),
        (dict(qmode=1), "only the exact quantised arithmetic (MC_QMODE_EXACT) can be batched"),
        (dict(head_dim=32), "head_dim must be 128 or 64"),
        (dict(n_kv_heads=3), "n_heads must be a multiple of n_kv_heads, at most 16 per kv head"),
        (dict(max_seq_len=32), "max_seq_len must be at least 64"),
        (dict(emb_fmt=WFMT_I4), "unsupported embedding format"),
        (dict(linears=changed("wo", out=1024 + 8)), "wo: " + head_text),
        (dict(linears=changed("w2", **{"in": 2048 + 512})), "w2: " + head_text),
        (dict(dim=2048), "layer shapes do not chain"),
        (dict(vocab=4096), "output head shape"),
    ]
    narrow = [
        (dict(weight_format=WFMT_I8), "only int4 (group % 128 == 0) and plain bfloat16 weights can be batched"),
        (dict(group_size=32), "int4 weights need a group size that is a multiple of 128"),
        (dict(linears=changed("wo", lora=1, lora_cols=16)), "LoRA adaptors are not supported (wo)"),
        (dict(linears=changed("w13", fmt=WFMT_T)), "mixed weight formats (w1|w3)"),
        (dict(linears=changed("qkv", group=32), group_size=128), "wq|wk|wv: int4 group size must be a multiple of 128"),   # (the config's stays)
    ]
    wide = [
        (dict(linears=changed("w2", fmt=3)), "w2: only int4, int8 and plain bfloat16 weights can be batched"),
        (dict(linears=changed("output", lora=1, lora_cols=16)), "LoRA adaptors are not supported (output)"),
        (dict(linears=changed("wo", lora=1, lora_cols=8)), "wo: LoRA rank must be a multiple of 16"),
        (dict(linears=changed("qkv", group=48)), "wq|wk|wv: the group size of quantised weights must be a multiple of 32 (or 0: one scale per row)"),
    ]
    lines, texts = [], []
    for w, reasons in ((False, both + narrow), (True, both + wide)):
        assert ask([bp.admit(cfg, base, w)]) == [{"admitted": True}]
        for change, text in reasons:
            change = dict(change)
            lin = change.pop("linears", base)
            shape = dict(cfg)
            for k in ("head_dim", "n_kv_heads", "max_seq_len", "dim", "vocab"):
                if k in change:
                    shape[k] = change.pop(k)
            lines.append(bp.admit(shape, lin, w, **change))
            texts.append(text)
    assert len(lines) == 2 * 12 + 5 + 4
    for line, text, a in zip(lines, texts, ask(lines)):
        assert a == {"refused": text}, (line, a)


# ------------------------------------------------------------------------------------------ (d) the checks of a call
def test_every_refusal_of_a_ragged_call():
    S, V, I32 = 256, 2048, 2 ** 31 - 1
    kw = dict(max_seq_len=S, vocab=V)
    who = "mc_ragged_step"
    cases = [
        (bp.ragged(who, [0, 3], [1, 2], [0, 3], **kw), None),
        (bp.ragged(who, [0, -2], [1, 2], [0, 3], **kw), "row 1: position below -1 (-1 = idle)"),
        (bp.ragged(who, [0, S], [1, 2], [0, S], **kw), f"row 1: position {S} must be below max_seq_len (a batch's cache does not roll)"),
        (bp.ragged(who, [0, S], [1, 2], [0, S], rolling=True, **kw), None),
        (bp.ragged(who, [I32 - 1, 0], [1, 2], [I32, 0], rolling=True, n=2, **kw), f"row 0: position {I32 - 1} + n leaves the range of positions"),
        (bp.ragged(who, [0, 4], [1, 2], [0, 3], **kw), "row 1: position 4 is past the row's length 3 (its cache has no slots written beyond it)"),
        (bp.ragged(who, [0, 10], [1, 2], [0, 300], rolling=True, **kw), "row 1: position 10 lies below the row's length 300 and the row has rolled"),
        (bp.ragged(who, [0, 300], [1, 2], [0, 300], rolling=True, **kw), None),
        (bp.ragged(who, [0, 3], [1, V], [0, 3], **kw), "row 1: token id outside the vocabulary"),
        (bp.ragged(who, [0, 3], [-1, 2], [0, 3], **kw), "row 0: token id outside the vocabulary"),
        (bp.ragged(who, [-1, -1], [1, 2], [0, 3], **kw), "no active row (every position is -1)"),
        (bp.ragged("mc_ragged_generate", [-1, -1], [1, 2], [0, 3], n=4, **kw), "no active row (every position is -1)"),
    ]
    for (line, text), a in zip(cases, ask([c[0] for c in cases])):
        caller = line.split()[1]
        assert a == ({"ok": True} if text is None else {"refused": f"{caller}: {text}"}), (line, a)


def test_the_refusals_of_a_verify_call_and_the_lockstep_bounds():
    why = "(accepting sampled drafts needs the draft's probabilities)"
    mask, pen, none = (1, 1.0, 0.0, 0.0), (0, 1.0, 0.5, 0.0), (0, 1.0, 0.0, 0.0)
    cases = [
        (bp.settings("mc_verify_rows", [2, 0, 3]), None),
        (bp.settings("mc_verify_rows", [2, 0, 3], dec_kind=1), f"mc_verify_rows: the decoder's sampler is not greedy {why}"),
        (bp.settings("mc_tree_verify", [2, 0, 3], dec_kind=1, kinds=[0, 1, 0]), None),                    # the sampling row is not in the call
        (bp.settings("mc_tree_verify", [2, 0, 3], dec_kind=1, kinds=[0, -1, -1]), f"mc_tree_verify: row 2: the row's sampler is not greedy {why}"),
        (bp.settings("mc_verify_rows", [2, 0, 3], kinds=[-1, -1, 1]), f"mc_verify_rows: row 2: the row's sampler is not greedy {why}"),
        (bp.settings("mc_verify_rows", [2, 0, 3], logit_rows=[none, mask, none]), None),
        (bp.settings("mc_verify_rows", [2, 0, 3], logit_rows=[mask, none, none]),
         "mc_verify_rows: row 0: the row has a token mask or penalties (a verify call would need them per chunk row)"),
        (bp.settings("mc_tree_verify", [2, 0, 3], logit_rows=[none, none, pen]),
         "mc_tree_verify: row 2: the row has a token mask or penalties (a verify call would need them per chunk row)"),
        ("bounds step 255 256", None),
        ("bounds step 256 256", "mc_batch_step: start_pos + 1 must not exceed max_seq_len (a batch's cache does not roll)"),
        ("bounds step -1 256", "mc_batch_step: start_pos + 1 must not exceed max_seq_len (a batch's cache does not roll)"),
        ("bounds generate 252 4 256", None),
        ("bounds generate 253 4 256", "mc_batch_generate: start_pos + n must not exceed max_seq_len (a batch's cache does not roll)"),
        ("bounds generate -1 4 256", "mc_batch_generate: start_pos + n must not exceed max_seq_len (a batch's cache does not roll)"),
        ("bounds generate 2147483647 2147483647 256", "mc_batch_generate: start_pos + n must not exceed max_seq_len (a batch's cache does not roll)"),
        ("bounds tokens 3 2048 0 2047 5", None),
        ("bounds tokens 3 2048 0 2048 5", "mc_batch: token id outside the vocabulary"),
        ("bounds tokens 3 2048 0 5 -1", "mc_batch: token id outside the vocabulary"),
    ]
    for (line, text), a in zip(cases, ask([c[0] for c in cases])):
        assert a == ({"ok": True} if text is None else {"refused": text}), (line, a)


def test_the_pick_forms_and_the_tables():
    B, V = 4, 2048
    inherit, dec = (-1, 0, 0.0, 0.0), (1, 50, 0.6, 0.9)
    greedy, uniform, own, mixed, one_greedy = ask([
        bp.head(V, False, (0, 50, 0.6, 0.9), [inherit] * B), bp.head(V, True, dec, [inherit] * B), bp.head(V, False, (0, 50, 0.6, 0.9), [dec] * B),
        bp.head(V, True, dec, [inherit, (1, 100, 0.6, 0.9), inherit, inherit]), bp.head(V, False, dec, [inherit, (0, 0, 0.0, 0.0), inherit, inherit])])
    assert greedy["form"] == "greedy" and greedy["launches"] == [["mc_b_argmax_bfloat", 1, B, 1, 1024, 0]]
    # top_k 50: lists of 64 keys from chunks of 512 logits; T(1 / T(0.6)) and T(0.9) in bfloat16
    inv_temp, top_p = bf16(float(np.float32(1.0) / np.float32(bf16(0.6)))), bf16(0.9)
    sp = dict(k=50, ncand=4 * 64, cap=4096, inv_temp=inv_temp, top_p=top_p, nlists=4, kpad=64)
    assert uniform["form"] == "uniform" and uniform["sp"] == sp and uniform["chunk"] == 512
    assert uniform["launches"] == [["mc_b_topk_candidates_bfloat", 4, B, 1, 64, 0], ["mc_b_sample_rows_bfloat", 1, B, 1, 128, 4096 * 8]]
    assert own["form"] == "uniform" and own["sp"] == sp and own["launches"][1][0] == "mc_b_sample_bfloat"      # rows with equal settings of their own
    assert mixed["form"] == "mixed" and mixed["sp"]["kpad"] == 128 and mixed["sp"]["k"] == 100                   # one kpad for the call: the largest top_k's
    assert mixed["launches"] == [["mc_b_topk_candidates_mixed_bfloat", 4, B, 1, 64, 0], ["mc_b_pick_mixed_rows_bfloat", 1, B, 1, 1024, 4096 * 8]]
    assert mixed["table"] == [[1, 50, inv_temp, top_p], [1, 100, inv_temp, top_p]] + [[1, 50, inv_temp, top_p]] * 2
    assert one_greedy["form"] == "mixed" and one_greedy["table"][1] == [0, 0, 0, 0] and one_greedy["launches"][1][0] == "mc_b_pick_mixed_bfloat"
    none, some = ask([bp.logits(V, False, [(0, 1.0, 0.0, 0.0)] * B), bp.logits(V, True, [(0, 1.0, 0.0, 0.0), (1, 1.0, 0.0, 0.0), (0, 2.0, 0.5, 0.25), (1, 1.0, 0.0, 0.0)])])
    assert none == {"any": False, "launches": [], "table": [[0, 0, 0, 0, 0]] * B}
    assert some["launches"] == [["mc_b_logits_process_rows_bfloat", 1, B, 1, 256, 0]]
    assert some["table"] == [[0, 0, 0, 0, 0], [1, 0, 0, 0, 0], [2, 2.0, 0.5, 0.5, 0.25], [1, 0, 0, 0, 0]]


# ------------------------------------------------------------------------------------------ (f) log-probabilities in the ordered list
def test_the_log_probability_launches_are_the_last_of_a_token():
    B, V = 4, SMALL["vocab"]
    lin = bp.linears_of(SMALL)
    sampling = (1, 50, 0.6, 0.9)
    picks = {"greedy": (dict(), ["mc_b_argmax"]), "uniform": (dict(dec_sampler=sampling), ["mc_b_topk_candidates_bfloat", "mc_b_sample"]),
             "mixed": (dict(dec_sampler=sampling, row_samplers=[(1, 1, 20, 0.7, 0.8)]), ["mc_b_topk_candidates_mixed_bfloat", "mc_b_pick_mixed"])}
    masked = [(2, 1, 1.0, 0.0, 0.0)]
    for ragged in (False, True):
        sfx = "_rows_bfloat" if ragged else "_bfloat"
        # vocab 2048: one chunk of 2048 logits per row (abi.h LOGPROB_CHUNK), 256 threads
        lp = [["mc_logprob_parts" + sfx, 1, B, 1, 256, 0], ["mc_logprob_finish" + sfx, 1, B, 1, 256, 0]]
        for form, (kw, pick) in picks.items():
            pick = [n if n.endswith("_bfloat") else n + sfx for n in pick]
            off, = ask([bp.token(SMALL, lin, B, cus=256, ragged_call=ragged, row_logits=masked, **kw)])
            for top_n in (0, 3):
                on, tail = ask([bp.token(SMALL, lin, B, cus=256, ragged_call=ragged, row_logits=masked, logprobs=top_n, **kw),
                                bp.token(SMALL, lin, B, cus=256, row_logits=masked, logprobs=top_n, tail=True, **kw)])
                assert on["launches"] == off["launches"] + lp and on["lp_slots"] == B and off["lp_slots"] == 0, (ragged, form, top_n)
                names = [l[0] for l in on["launches"]]
                process = "mc_b_logits_process" + sfx
                assert names[-len(pick) - 4:] == ["mc_b_gemv_w_bfloat_e0", process] + pick + [l[0] for l in lp], (ragged, form, top_n, names)
                assert names[-len(pick) - 5] == "mc_b_rmsnorm_bfloat" and names.count(process) == 1
                # behind a prompt pass: the ragged list from the final norm on, whatever `ragged` of the request says
                if ragged:
                    assert tail["launches"] == on["launches"][-len(pick) - 5:], (form, top_n)
    # the process launch of a step counts, the one behind a prompt pass does not: two op tags for one launch
    on, tail = ask([bp.token(SMALL, lin, B, cus=256, ragged_call=True, row_logits=masked), bp.token(SMALL, lin, B, cus=256, row_logits=masked, tail=True)])
    assert on["launches"][-2] == tail["launches"][-2] and on["ops"][-2] != tail["ops"][-2] and on["ops"][-1] == tail["ops"][-1]
    # a vocabulary of more chunks than the finish launch folds is the call's refusal
    big = dict(SMALL, vocab=2048 * 257)
    a, = ask([bp.token(big, bp.linears_of(big), B, cus=256, logprobs=0)])
    assert a["refused"].startswith("mc_logprobs: the vocabulary has 257 chunks of 2048"), a


# ------------------------------------------------------------------------------------------ (e) the names exist
def test_every_kernel_the_plans_name_exists():
    """the names of every answer of (a) to (d) -- asked again here, so that the check is the same whichever tests ran before it --, of the sweep
    and of the recording"""
    SEEN.clear()
    for asks in (test_the_plans_are_the_recorded_launches_field_for_field, test_the_tile_rule_at_real_widths, test_the_shapes_of_the_gpu_tests_are_admitted,
                 test_every_reason_of_the_admission_is_reached_by_one_change, test_every_refusal_of_a_ragged_call,
                 test_the_refusals_of_a_verify_call_and_the_lockstep_bounds, test_the_pick_forms_and_the_tables,
                 test_the_log_probability_launches_are_the_last_of_a_token):
        asks()
    assert len(SEEN) >= 40, sorted(SEEN)
    names = set(SEEN) | set(bp.formed_names())
    for c in recorded():
        names |= {x[0] for x in c["launches"]}
    assert len(names) >= 65, sorted(names)
    hsaco, _ = b.build_all()
    tool = next((t for t in READELF if os.path.exists(t)), None)
    assert tool is not None, "no readelf available"
    out = subprocess.check_output([tool, "--symbols", "--wide", hsaco], text=True)
    symbols = {line.split()[-1] for line in out.splitlines() if " FUNC " in line}
    missing = sorted(n for n in names if n not in symbols)
    assert not missing, missing
