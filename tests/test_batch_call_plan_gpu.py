"""The calls on a batch as launched, against their plans: for one call of every kind on the suite's small one-layer model (dim 1024, vocab 2048,
max_seq_len 256, int4 g128) the decoder's launch log names the kernels, in the order, of the list that csrc/batch_call_plan.h plans for the same
inputs (through tests/cpp/test_batch_plan and test_verify_settings_plan, the programs of the CPU tests) -- the list mc_batch::run walks.  A rows
pass is compared behind its prompt pass (the gather of the segments' last rows).  Names and order only: what the launches compute is held bit for
bit by the suites of each call."""
import numpy as np
import pytest

import batch_plan_program as bp
import modelgen as mg
from test_batch_gpu import SMALL, small_decoder
from test_verify_settings_cpu import ask as ask_verify, call as verify_call

pytestmark = pytest.mark.gpu
GREEDY, DEFAULT, DRAW, INHERIT = 0, 1, 2, -1
GATHER = "mc_pp_gather_last_bfloat"
LINEARS = bp.linears_of(SMALL, bp.WFMT_I4, 128)
PAIRS = [(3 + 2 * i, 11 + 7 * i) for i in range(5)]
DEC_SAMPLER = (DEFAULT, 50, 0.6, 0.9)
OWN = (DEFAULT, 20, 0.7, 0.8)
PENALTIES = (1.3, 0.25, 0.5)


@pytest.fixture(scope="module")
def dec(acc):
    d = small_decoder(acc, SMALL, mg.make_model(SMALL, seed=11, quant="i4", group=128))
    yield d
    d.release()


def batch_of(dec, B, wide=False):
    import metalchat_amd as mc

    b = mc.Batch(dec, B, wide=wide)
    b.set_seeds(PAIRS)
    return b


def logged(dec, call):
    dec.launch_log(True)
    call()
    names = dec.launched()
    dec.launch_log(False)
    return names


def planned(acc, B, n=1, **kw):
    return [l[0] for l in bp.ask([bp.token(SMALL, LINEARS, B, cus=acc.compute_units(), **kw)])[0]["launches"]] * n


def planned_verify(lens, samplers, logit_rows, **kw):
    a, = ask_verify([verify_call(lens, samplers, logit_rows, cfg=SMALL, n_pairs=len(PAIRS), head_fmt=bp.WFMT_I4, **kw)])
    return [l[0] for l in a["launches"]]


def behind_the_prompt_pass(names):
    assert names.count(GATHER) == 1, names
    return names[names.index(GATHER) + 1:]


def tokens(B):
    return [5 + 3 * r for r in range(B)]


def test_a_lockstep_step(acc, dec):
    b = batch_of(dec, 2)
    assert logged(dec, lambda: b.step(tokens(2), 0)) == planned(acc, 2)
    b.release()


@pytest.mark.parametrize("rolling", [False, True])
def test_a_ragged_generate_of_two_tokens_with_an_idle_row(acc, dec, rolling):
    b = batch_of(dec, 2)
    b.set_rolling(rolling)
    want = planned(acc, 2, n=2, ragged_call=True, rolling=rolling)
    assert ("mc_b_rows_begin_rolling" in want) == rolling
    assert logged(dec, lambda: b.generate_rows(tokens(2), [0, -1], 2)) == want
    b.release()


def test_a_wide_batch(acc, dec):
    b = batch_of(dec, 17, wide=True)
    want = planned(acc, 17)
    assert any(n.startswith("mc_wb_gemv_") for n in want)
    assert logged(dec, lambda: b.step(tokens(17), 0)) == want
    b.release()


def test_the_decoder_sampler_is_the_uniform_pick(acc, dec):
    b = batch_of(dec, 2)
    dec.set_sampler(*DEC_SAMPLER)
    try:
        want = planned(acc, 2, dec_sampler=DEC_SAMPLER)
        assert want[-2:] == ["mc_b_topk_candidates_bfloat", "mc_b_sample_bfloat"]
        assert logged(dec, lambda: b.step(tokens(2), 0)) == want
    finally:
        dec.set_sampler(GREEDY)
    b.release()


def test_a_row_with_its_own_sampler_is_the_mixed_pick(acc, dec):
    b = batch_of(dec, 2)
    b.set_row_sampler(1, *OWN)
    want = planned(acc, 2, row_samplers=[(1, *OWN)])
    assert want[-2:] == ["mc_b_topk_candidates_mixed_bfloat", "mc_b_pick_mixed_bfloat"]
    assert logged(dec, lambda: b.step(tokens(2), 0)) == want
    b.release()


def test_a_masked_and_penalised_row(acc, dec):
    b = batch_of(dec, 2)
    b.set_row_mask(0, np.arange(SMALL["vocab"]) % 4 != 1)
    b.set_row_penalties(0, *PENALTIES)
    want = planned(acc, 2, ragged_call=True, row_logits=[(0, 1, *PENALTIES)])
    assert want[-2:] == ["mc_b_logits_process_rows_bfloat", "mc_b_argmax_rows_bfloat"]
    assert logged(dec, lambda: b.step_rows(tokens(2), [0, 0])) == want
    b.release()


def test_log_probabilities_with_the_top_three(acc, dec):
    b = batch_of(dec, 2)
    b.set_logprobs(3)
    want = planned(acc, 2, ragged_call=True, logprobs=3)
    assert want[-2:] == ["mc_logprob_parts_rows_bfloat", "mc_logprob_finish_rows_bfloat"]
    assert logged(dec, lambda: b.step_rows(tokens(2), [0, 0])) == want
    b.release()


@pytest.mark.parametrize("call", ["prefill_rows", "extend_rows"])
def test_the_tail_of_a_rows_pass(acc, dec, call):
    b = batch_of(dec, 2)
    want = planned(acc, 2, tail=True)
    assert want == ["mc_b_rmsnorm_bfloat", "mc_b_gemv_i4_bfloat_e0", "mc_b_argmax_rows_bfloat"]
    names = logged(dec, lambda: getattr(b, call)([[7, 8, 9], [4, 5]], [0, 0]))
    assert behind_the_prompt_pass(names) == want
    b.release()


def test_a_verify_call_with_lens_two_and_zero(acc, dec):
    b = batch_of(dec, 2)
    want = planned_verify([2, 0], [(INHERIT, 0, 0.0, 0.0)] * 2, [(0, 1.0, 0.0, 0.0)] * 2)
    assert want == ["mc_b_rmsnorm_bfloat", "mc_v_head_i4_bfloat", "mc_v_argmax_bfloat", "mc_v_accept"]
    assert behind_the_prompt_pass(logged(dec, lambda: b.verify_rows([[7, 8], None], [0, 0]))) == want
    b.release()


def test_a_tree_of_three_nodes(acc, dec):
    b = batch_of(dec, 2)
    parents = [-1, 0, 0]
    want = planned_verify([3, 0], [(INHERIT, 0, 0.0, 0.0)] * 2, [(0, 1.0, 0.0, 0.0)] * 2, parents=[parents])
    assert want == ["mc_b_rmsnorm_bfloat", "mc_v_head_i4_bfloat", "mc_v_argmax_bfloat", "mc_tv_accept", "mc_tv_compact_bfloat"]
    assert behind_the_prompt_pass(logged(dec, lambda: b.verify_tree([[7, 8, 9], None], [parents, None], [0, 0]))) == want
    b.release()


def test_a_verify_call_with_row_settings_and_log_probabilities(acc, dec):
    b = batch_of(dec, 2)
    b.set_verify_settings(True)
    b.set_row_sampler(0, DRAW, 40, 0.9, 0.95)
    b.set_row_penalties(1, *PENALTIES)
    b.set_logprobs(3)
    want = planned_verify([3, 2], [(DRAW, 40, 0.9, 0.95), (INHERIT, 0, 0.0, 0.0)], [(0, 1.0, 0.0, 0.0), (0, *PENALTIES)], logprobs=3)
    assert want == ["mc_b_rmsnorm_bfloat", "mc_v_head_i4_bfloat", "mc_vs_logits_process_bfloat", "mc_vs_topk_candidates_mixed_bfloat", "mc_vs_pick_mixed_bfloat",
                    "mc_logprob_parts_bfloat", "mc_logprob_finish_bfloat", "mc_v_accept", "mc_vs_count_accepted"]
    assert behind_the_prompt_pass(logged(dec, lambda: b.verify_rows([[7, 8, 9], [4, 5]], [0, 0]))) == want
    b.release()
