"""The launches of one decode token -- the embed, every block's GEMVs around its attention launch, gemma3's post-norms folded or not, the taps, the
head and the pick -- pinned without a GPU: plan_token() (csrc/token_plan.h) is integer arithmetic and string building on symbolic operands, so
tests/cpp/test_token_plan, a plain g++ program over that header, is asked the tokens of every case in tests/golden/decode_token_plans.json and has to
name, in order, the kernels the commit that file names launched for step(1, 0), step(-1, 1) and generate(3, 0, 4) (its launch log, recorded by
tools/experiments/token_plan_record.py).  The program itself holds every GEMV step against plan_gemv and every block against plan_block; the
structure of a plan -- rows are written before they are read, a post-norm is applied exactly once, a deferred pick has a head that made one -- is
checked here over all cases.

The finding behind the last test: the recorded commit asked "does the head make the pick?" twice, inside the token with the pending post-norm in
view and outside it without, and for a gemma3 decoder whose head takes a linear-order kernel the answers differed -- mc_decoder_generate deferred a
fold of keys that the head, behind its post-norm prologue, never wrote.  Those cases are recorded under MC_LAZY_PICK=0, which is what one answer
yields for them."""
import pytest

from token_plan_program import AROUND, G, planned_names, plans, token_launches

CASES = sorted(G["cases"])
GEMVS = ("qkv_gemv", "wo_gemv", "w13_gemv", "w2_gemv", "head_gemv")


def all_tokens():
    for name in CASES:
        for t in plans()[name]:
            yield name, t


def test_the_cases_are_the_ones_to_record():
    kinds = {k: [n for n in CASES if n.startswith(k + ":")] for k in ("model", "device", "variant")}
    assert len(kinds["model"]) == 11 and len(kinds["device"]) == 24 and len(kinds["variant"]) == 2 * 14
    assert G["cus"] == 256
    for name in CASES:
        c = G["cases"][name]
        single = c["cfg"]["layer_begin"] == 0 and c["cfg"]["layer_end"] == c["cfg"]["n_layers"]
        assert ("generate" in c) == single and ("tokens" in c) == single, name
        assert c["step0"] and c["step1"], name
        assert any(n in AROUND for n in c["step0"]), name  # (the log is the whole call's)


@pytest.mark.parametrize("case", CASES)
def test_planned_names_are_the_recorded_launches(case):
    c, planned = G["cases"][case], planned_names(case)
    assert all(t.error == "" for t in plans()[case])
    for call, names in planned.items():
        assert names == token_launches(c[call]), (case, call, "recorded from", G["recorded_from"], "under", c["recorded_under"])


def test_no_step_reads_a_row_nobody_wrote():
    for name, t in all_tokens():
        first = G["cases"][name]["cfg"]["layer_begin"] == 0
        written = set() if first else {"in"}  # (a later stage's inbound row is the caller's)
        for i, s in enumerate(t.steps):
            reads = {s["x"]} | ({s["res_row"]} if s["res"] == "row" else set())
            writes = {s["y"]}
            if s["op"] in ("post_norm_attn", "post_norm_ffn"):
                reads.add("proj")
            if s["res"] == "pn_attn":    # hidden_b = hidden + norm(proj) w
                reads |= {"proj", "hidden"}
                writes.add("hidden_b")
            if s["res"] == "pn_ffn":     # hidden = hidden_b + norm(proj) w
                reads |= {"proj", "hidden_b"}
                writes.add("hidden")
            if s["res"] == "qkv_epi":    # the rope epilogue leaves the rotated queries
                writes.add("q_rot")
            if s["op"] == "attn" and "_w13_w_" in s["name"]:
                writes.add("gate")
            reads.discard("-")
            assert reads <= written, (name, i, s["op"], s["layer"], sorted(reads - written))
            written |= writes - {"-"}


def test_a_post_norm_is_applied_exactly_once():
    seen = 0
    for name, t in all_tokens():
        cfg = G["cases"][name]["cfg"]
        if cfg.get("family", 0) != 1:
            assert not [s for s in t.steps if s["res"] in ("pn_attn", "pn_ffn") or s["op"].startswith("post_norm")], name
            continue
        n_own, last = cfg["layer_end"] - cfg["layer_begin"], cfg["layer_end"] == cfg["n_layers"]
        main = [s for s in t.steps if s["adaptor"] == "0" and s["op"] != "tap"]
        for li in range(n_own):
            layer = str(li)
            for half, row, takers in (("pn_attn", "post_norm_attn", ("w13_gemv",)), ("pn_ffn", "post_norm_ffn", ("qkv_gemv", "attn", "head_gemv"))):
                appliers = [s for s in main if (s["res"] == half and s["res_layer"] == layer) or (s["op"] == row and s["layer"] == layer)]
                assert len(appliers) == 1, (name, li, half, [s["op"] for s in appliers])
                a = appliers[0]
                # ... by the step right behind the one that left the row in `proj`: the next pre-norm launch, or the row launch
                writer = [i for i, s in enumerate(main) if s["layer"] == layer and s["y"] == "proj" and s["op"] in (("attn", "wo_gemv") if half == "pn_attn" else ("w2_gemv",))]
                assert len(writer) == 1 and main[writer[0] + 1] is a, (name, li, half)
                assert a["op"] == row or (a["op"] in takers and a["x"] == "proj"), (name, li, half, a["op"])
                if a["op"] == "post_norm_ffn" and a["x"] == "hidden_b":  # folded, but the row leaves the stage: materialised at its end only
                    assert li == n_own - 1 and not last, (name, li)
                seen += 1
    assert seen


def test_a_lazy_token_has_a_head_that_left_keys():
    lazy_seen = 0
    for name in CASES:
        p = plans()[name]
        for t in p:
            heads = [s for s in t.steps if s["op"] == "head_gemv" and s["adaptor"] == "0"]
            folds = [s for s in t.steps if s["op"] == "fold_pick"]
            per_wg = bool(heads) and heads[0]["res"] == "pick_per_wg"
            if t.lazy:
                assert per_wg and not folds and not t.head_behind_post_norm, name
                lazy_seen += 1
            else:
                assert len(folds) == (1 if per_wg else 0), name
            if heads and t.head_behind_post_norm:
                assert heads[0]["pro"] == "2" and heads[0]["epi"] == "0" and heads[0]["res"] == "pn_ffn", name
        # ... and only a chained token behind a lazy one folds keys in its embed
        for t in p:
            for s in t.steps:
                if s["op"] == "embed":
                    assert (s["fold_keys"] == "1") == (s["advance"] == "1" and p[1].lazy), name
    assert lazy_seen


DEFECT = [n for n in CASES if G["cases"][n]["recorded_under"]]


def test_the_two_answers_of_the_recorded_commit_differ_where_one_answer_now_stands():
    """gemma3, one stage, folded post-norms, greedy, MC_HEAD_PICK=2, a head lin_ok() takes: asked without the pending post-norm the pick is deferred
    (what mc_decoder_generate did), asked with it the head makes none (what run_head did).  One answer: not lazy, the MC_LAZY_PICK=0 sequence."""
    assert "model:gemma" in DEFECT and all(":gemma" in n for n in DEFECT)
    for name in CASES:
        first, chained = plans()[name][1:] if len(plans()[name]) > 1 else (None, None)
        if first is None:
            continue
        differed = first.lazy_if_nothing_pending and first.head_behind_post_norm
        assert differed == (name in DEFECT), name
        if not differed:
            continue
        assert G["cases"][name]["recorded_under"] == {"MC_LAZY_PICK": "0"}
        assert not first.lazy and not chained.lazy
        names = planned_names(name)["generate"]
        assert "mc_argmax_keys" not in names and names.count("mc_argmax_bfloat") == 4
        assert not [s for s in chained.steps if s["fold_keys"] == "1"]
        assert names == token_launches(G["cases"][name]["generate"])
