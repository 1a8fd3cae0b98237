"""tests/cpp/test_token_plan -- plan_token() of csrc/token_plan.h as a plain g++ program -- asked the tokens of every case recorded in
tests/golden/decode_token_plans.json: shared by test_token_plan_cpu.py (the sequences, the structure) and test_kernel_names_cpu.py (the names).

A case holds a decoder's configuration, not the plan's inputs (the recorder has no more than the launch log to go by), so the inputs are worked out here
as mc_decoder_create and the loaders fill them: the fused shapes, the range count, and the occupancy answers the MI355X gave for the kernels
query_occupancy asks about (tests/golden/decode_block_plans.json holds them per head_dim; a float decoder never asks)."""
import collections
import functools
import json
import os
import subprocess

from metalchat_amd import build as b

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "decode_token_plans.json")
with open(GOLDEN) as f:
    G = json.load(f)
FIELDS = ["op", "layer", "name", "gx", "gy", "gz", "block", "lds", "pro", "epi", "adaptor", "pn_by_value", "x", "y", "res", "res_row", "res_layer", "norm",
          "advance", "fold_keys"]
# the switches of the cases and the decoder_options fields they set (csrc/decoder_options.h read_options)
SWITCHES = {
    "MC_ATTN_FUSED": lambda v: {"attn_fused": int(v)},
    "MC_GEMMA_UNFUSED": lambda v: {"gemma_fuse": 1 - int(v)},
    "MC_HEAD_PICK": lambda v: {"head_pick_mode": int(v), "head_pick_on": int(int(v) != 0)},
    "MC_LAZY_PICK": lambda v: {"lazy_pick_on": int(v)},
}
SAMPLERS = {"greedy": 0, "default": 1, "draw": 2}
# (head_dim, K of Wo in 2048s) of the built mc_attn_wo_i4_bfloat_* kernels
WO_BUILT = {(64, 1), (128, 2), (256, 2)}


def occupancy(cfg):
    """fused wo wo_w wo_i8 wo_qkn qkv_qkn qkv_only wo_i4_wide w13 (mc_decoder::query_occupancy on the recording device)"""
    if cfg["dtype"] != 0:
        return [-1] * 9
    hd = cfg["head_dim"]
    wo = 2 if (hd, cfg["n_heads"] * hd // 2048) in WO_BUILT else 0
    return [4, wo, 2 * (hd == 64), 1 * (hd == 128), 2 * (hd == 256), 1 * (hd == 256), 1 * (hd == 128), 2 * (hd == 128), 1 * (hd == 64)]


def shapes(case):
    """fmt out in group lora_cols of the head and of wq|wk|wv, Wo, w1|w3, w2 (every owned block has the same)"""
    c, w = case["cfg"], case["weights"] or {}
    fmt, group = c.get("weight_format", 0), c.get("group_size", 0)
    dim, H, KV, hd, ffn = c["dim"], c["n_heads"], c["n_kv_heads"], c["head_dim"], c["ffn_dim"]
    rank, only = w.get("lora_rank", 0), w.get("lora_only")

    def cols(names):  # adaptors of a fused matrix share its columns: one block of `rank` per fused segment once any of them is adapted
        return rank * len(names) if rank and (only is None or any(n in only for n in names)) else 0

    head = [fmt, c["vocab"], dim, group, 0]
    layer = [fmt, (H + 2 * KV) * hd, dim, group, cols(("wq", "wk", "wv")), fmt, dim, H * hd, group, cols(("wo",)),
             fmt, 2 * ffn, dim, group, cols(("w1", "w3")), fmt, dim, ffn, group, cols(("w2",))]
    return head, layer


def line(case, lazy=0, advance=0):
    """the program's input for one token of a case"""
    c = case["cfg"]
    S, tb = c["max_seq_len"], 2 if c["dtype"] == 0 else 4
    first, last, n_own = c["layer_begin"] == 0, c["layer_end"] == c["n_layers"], c["layer_end"] - c["layer_begin"]
    opts = {}
    for k, v in case["env"].items():
        opts.update(SWITCHES[k](v))
    model = [c.get("family", 0), c["n_heads"], c["n_kv_heads"], c["head_dim"], c["dim"], S]
    env = [tb, c.get("qmode", 0), G["cus"], (S + 63) // 64, n_own, int(tb == 2), min(16, S // 2048) if S >= 8192 else 1] + occupancy(c)
    emb_i8 = bool((case["weights"] or {}).get("emb_quant"))
    fixed = [int(first), int(last), 1 if emb_i8 else 0, c["vocab"], 50]
    state = [opts.get("attn_fused", 1), int(case["taps"]), SAMPLERS[case["sampler"]], lazy, advance, 0]
    head, layer = shapes(case)
    ints = model + env + fixed + state + head + [n_own] + layer * n_own
    return " ".join(str(x) for x in ints) + "".join(f" {k}={v}" for k, v in sorted(opts.items()))


def tokens_of(case):
    """the lines of a case: [a single step's token, a generate's first token, its chained tokens] (the last two for a single stage only)"""
    c = case["cfg"]
    single = c["layer_begin"] == 0 and c["layer_end"] == c["n_layers"]
    return [line(case)] + ([line(case, lazy=1), line(case, lazy=1, advance=1)] if single else [])


# one planned token: its steps (dicts over FIELDS); is it lazy; is a post-norm pending in front of its head; would lazy_pick_ok say yes if asked as
# though none were; the refusal, "" = none
Token = collections.namedtuple("Token", "steps lazy head_behind_post_norm lazy_if_nothing_pending error")


@functools.lru_cache(maxsize=None)
def plans():
    """{case: [Token per line of tokens_of(case)]}: one run of the program"""
    exe = b.build_token_plan_test()
    names = list(G["cases"])
    text = "".join(t + "\n" for n in names for t in tokens_of(G["cases"][n]))
    out = subprocess.run([exe], input=text, capture_output=True, text=True, check=True).stdout.split("\n")[:-1]
    answers, steps = [], []
    for ln in out:
        if ln.startswith("end "):
            lazy, behind, unasked, error = ln[4:].split(" ", 3)
            answers.append(Token(steps, lazy == "lazy=1", behind.endswith("=1"), unasked.endswith("=1"), error[len("error="):]))
            steps = []
        else:
            steps.append(dict(zip(FIELDS, ln.split())))
    it = iter(answers)
    got = {n: [next(it) for _ in tokens_of(G["cases"][n])] for n in names}
    assert next(it, None) is None
    return got


def launches(steps):
    """the kernel names of a token's steps (the copies launch nothing)"""
    return [s["name"] for s in steps if s["name"] != "-"]


def planned_names(case_name):
    """what the plan says the three recorded calls launch, the launches around the token left out: {"step0": [...], "step1": [...], "generate": [...]}"""
    p = plans()[case_name]
    out = {"step0": launches(p[0].steps), "step1": launches(p[0].steps)}  # (the plan does not depend on the position)
    if len(p) > 1:  # the first token, three chained ones, and the caller's fold behind the last lazy token
        out["generate"] = launches(p[1].steps) + 3 * launches(p[2].steps) + (["mc_argmax_keys"] if p[1].lazy else [])
    return out


# the launches of a call that are not the token's: the step state and the rope table (mc_decoder_step / mc_decoder_generate, ensure_rope)
AROUND = ("mc_step_set", "mc_step_rope", "mc_step_advance", "mc_rope_table")


def token_launches(log):
    return [n for n in log if n not in AROUND]
