"""MC_SAMPLER_DRAW in the device-free pick plan (metalchat_amd/csrc/batch_plan.h plan_head, through tests/cpp/test_draw_plan) and in the built
code object, without a GPU:

  * the names, grids, block sizes and LDS bytes of an all-draw batch, of draw + greedy and of draw + default, lockstep and ragged; the table of
    effective settings the mixed launches read; kinds 0 and 1 keep their plans;
  * the four new kernels are FUNC symbols of the code object;
  * the code object's notes report a zero private segment and no spills for them and for both mc_b_pick_mixed*."""
import json
import os
import re
import struct
import subprocess

import numpy as np

import batch_plan_program as bp
from metalchat_amd import build as b

READELF = ["/opt/rocm/lib/llvm/bin/llvm-readelf", "/opt/rocm/llvm/bin/llvm-readelf"]
GREEDY, DEFAULT, DRAW, INHERIT = 0, 1, 2, -1
NEW = ["mc_draw_bfloat", "mc_draw_float", "mc_draw_b_bfloat", "mc_draw_b_rows_bfloat"]
MIXED = ["mc_b_pick_mixed_bfloat", "mc_b_pick_mixed_rows_bfloat"]


def bf16(x):
    u = struct.unpack("<I", struct.pack("<f", x))[0]
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return struct.unpack("<f", struct.pack("<I", u))[0]


def rounded(k, t, p):
    """(top_k, T(1 / T(temperature)), T(top_p)) in bfloat16, as the host keeps a sampling row's settings"""
    return [k, bf16(float(np.float32(1.0) / np.float32(bf16(t)))), bf16(p)]


def ask(lines):
    exe = b.build_draw_plan_test()
    out = subprocess.run([exe], input="".join(line + "\n" for line in lines), capture_output=True, text=True, check=True).stdout
    answers = [json.loads(a) for a in out.split("\n")[:-1]]
    assert len(answers) == len(lines)
    return answers


def test_the_plans_of_batches_with_draw_rows():
    B, V = 4, 2048
    a, c = (40, 0.9, 0.95), (5, 1.5, 0.5)
    inherit, greedy_dec = (INHERIT, 0, 0.0, 0.0), (GREEDY, 50, 0.6, 0.9)
    # top_k 40: lists of 64 keys from chunks of 512 logits; the LDS of the second launch: SAMPLE_CAP keys of 8 bytes
    sp = dict(k=40, ncand=4 * 64, cap=4096, inv_temp=rounded(*a)[1], top_p=rounded(*a)[2], nlists=4, kpad=64)
    for ragged, sfx in ((False, "_bfloat"), (True, "_rows_bfloat")):
        own, inherited, with_greedy, with_default, same_numbers, default_only, greedy_only = ask([
            bp.head(V, ragged, greedy_dec, [(DRAW, *a)] * B),                                   # every row set to the same draw
            bp.head(V, ragged, (DRAW, *a), [inherit] * B),                                      # the decoder's, inherited
            bp.head(V, ragged, greedy_dec, [(GREEDY, 0, 0.0, 0.0), (DRAW, *a), (DRAW, *a), (DRAW, *a)]),
            bp.head(V, ragged, (DEFAULT, *c), [(DRAW, *a), inherit, (DRAW, *c), inherit]),
            bp.head(V, ragged, (DEFAULT, *a), [(DRAW, *a), inherit, inherit, inherit]),         # equal numbers, the kind alone differs
            bp.head(V, ragged, (DEFAULT, *a), [inherit] * B),
            bp.head(V, ragged, greedy_dec, [inherit] * B)])
        for u in (own, inherited):
            assert u["form"] == "uniform" and u["sp"] == sp and u["chunk"] == 512, u
            assert u["launches"] == [["mc_b_topk_candidates_bfloat", 4, B, 1, 64, 0], ["mc_draw_b" + sfx, 1, B, 1, 128, 4096 * 8]], u
            assert u["table"] == [[DRAW] + rounded(*a)] * B
        mixed = [["mc_b_topk_candidates_mixed_bfloat", 4, B, 1, 64, 0], ["mc_b_pick_mixed" + sfx, 1, B, 1, 1024, 4096 * 8]]
        assert with_greedy["form"] == "mixed" and with_greedy["launches"] == mixed
        # (the mixed launches take nlists, kpad and cap from sp; the rows' own k, temperature and top_p from the table)
        assert [with_greedy["sp"][w] for w in ("nlists", "kpad", "cap", "ncand")] == [4, 64, 4096, 256]
        assert with_greedy["table"] == [[GREEDY, 0, 0, 0]] + [[DRAW] + rounded(*a)] * 3
        assert with_default["form"] == "mixed" and with_default["launches"] == mixed and with_default["sp"]["kpad"] == 64 and with_default["sp"]["k"] == 40
        assert with_default["table"] == [[DRAW] + rounded(*a), [DEFAULT] + rounded(*c), [DRAW] + rounded(*c), [DEFAULT] + rounded(*c)]
        assert same_numbers["form"] == "mixed" and same_numbers["launches"] == mixed
        assert same_numbers["table"] == [[DRAW] + rounded(*a)] + [[DEFAULT] + rounded(*a)] * 3
        # kinds 0 and 1: what they were
        assert default_only["form"] == "uniform" and default_only["sp"] == sp and default_only["table"] == [[DEFAULT] + rounded(*a)] * B
        assert default_only["launches"] == [["mc_b_topk_candidates_bfloat", 4, B, 1, 64, 0], ["mc_b_sample" + sfx, 1, B, 1, 128, 4096 * 8]]
        assert greedy_only["form"] == "greedy" and greedy_only["launches"] == [["mc_b_argmax" + sfx, 1, B, 1, 1024, 0]]
    # a real vocabulary, the widest top-k, a wide batch: 251 lists of 128 keys
    wide = ask([bp.head(128256, True, (DRAW, 128, 0.7, 1.0), [inherit] * 64)])[0]
    assert wide["launches"] == [["mc_b_topk_candidates_bfloat", 251, 64, 1, 64, 0], ["mc_draw_b_rows_bfloat", 1, 64, 1, 128, 4096 * 8]]
    assert wide["sp"]["kpad"] == 128 and wide["sp"]["ncand"] == 251 * 128 and wide["chunk"] == 512


def code_object_tool():
    tool = next((t for t in READELF if os.path.exists(t)), None)
    assert tool is not None, "no llvm-readelf available"
    return tool


def test_the_new_kernels_exist():
    hsaco, _ = b.build_all()
    out = subprocess.check_output([code_object_tool(), "--symbols", "--wide", hsaco], text=True)
    symbols = {line.split()[-1] for line in out.splitlines() if " FUNC " in line}
    assert not [n for n in NEW + MIXED if n not in symbols], sorted(n for n in NEW + MIXED if n not in symbols)


def test_nothing_of_them_lives_in_private_memory():
    hsaco, _ = b.build_all()
    notes = subprocess.check_output([code_object_tool(), "--notes", hsaco], text=True)
    kernels = {}
    for block in re.split(r"\n\s+- \.agpr_count:", notes)[1:]:
        name = re.search(r"\.name:\s+(\S+)", block).group(1)
        kernels[name] = {k: int(re.search(r"\.%s:\s+(\d+)" % k, block).group(1))
                         for k in ("private_segment_fixed_size", "sgpr_spill_count", "vgpr_spill_count", "group_segment_fixed_size")}
    for name in NEW + MIXED:
        k = kernels[name]
        assert (k["private_segment_fixed_size"], k["sgpr_spill_count"], k["vgpr_spill_count"]) == (0, 0, 0), (name, k)
    # the switch of the last phase adds no LDS: the drawing kernels hold what their default forms hold
    for new, old in zip(NEW, ["mc_sample_bfloat", "mc_sample_float", "mc_b_sample_bfloat", "mc_b_sample_rows_bfloat"]):
        assert kernels[new]["group_segment_fixed_size"] == kernels[old]["group_segment_fixed_size"], (new, kernels[new], kernels[old])
