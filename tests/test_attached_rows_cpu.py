"""Packed chunks and verify on attached rows (include/metalchat_hip.h Part 2t) without a GPU: the header declares the two calls, a null batch
gets the specified answers, the code object holds exactly the four mc_ax_* kernels without a private segment or spills, and the plan of a call
(csrc/rows_plan.h, asked through tests/cpp/test_attached_plan) lists the attached rows' tiles behind the others in units, and is today's when
no attached row is named."""
import os
import re
import subprocess

import pytest

import rows_tables as rt
from metalchat_amd import build as b
from metalchat_amd import runtime

KERNELS = {f"mc_ax_{k}_bfloat_hd{hd}" for k in ("sums", "pv") for hd in (64, 128)}


def test_the_header_declares_the_two_calls_once_each():
    with open(os.path.join(os.path.dirname(b.HERE), "include", "metalchat_hip.h")) as fh:
        declared = re.findall(r"^(?:mc_status|int32_t)\s+(mc_attached_\w+)\(", fh.read(), re.M)
    assert sorted(declared) == ["mc_attached_packed_enabled", "mc_attached_packed_set"]


def test_a_null_batch():
    api = runtime.capi()
    assert api.mc_attached_packed_enabled(None) == 0
    assert api.mc_attached_packed_set(None, 1) == 1
    assert "mc_attached_packed_set: null argument" in api.mc_last_error().decode()


def test_the_code_object_holds_the_kernels_and_none_keeps_private_memory():
    out = subprocess.check_output(["/opt/rocm/lib/llvm/bin/llvm-readelf", "--notes", b.build_all()[0]], text=True)
    kernels = {m.group(1): k for k in out.split(".agpr_count")[1:] if (m := re.search(r"\.name:\s+(mc_ax_\w*)", k))}
    assert set(kernels) == KERNELS
    for k in kernels.values():
        assert [int(v) for v in re.findall(r"\.(?:private_segment_fixed_size|[sv]gpr_spill_count):\s+(\d+)", k)] == [0, 0, 0], k


def ask(H, KV, hd, keys, mask, rows):
    out = subprocess.check_output([b.build_attached_plan_test(), *map(str, (H, KV, hd, keys, mask)), *(str(x) for r in rows for x in r)], text=True)
    lines = [line.split() for line in out.splitlines()]
    pick = lambda tag: [tuple(int(x) if x.lstrip("-").isdigit() else x for x in rest) for t, *rest in lines if t == tag]
    return pick("T")[0][0], pick("range"), pick("unit"), pick("launch")


@pytest.mark.parametrize("hd,n_rep,T", [(128, 4, 3), (64, 4, 3), (128, 1, 4)])
def test_tiles_per_unit(hd, n_rep, T):
    assert ask(4 * n_rep, 4, hd, -1, 0, [(2, 0)])[0] == T


ROWS = [(16, 200), (0, 0), (20, 70), (5, 230)]   # (len, pos) of B = 4: rows 0 and 3 attached behind 192 shared slots, row 2 ordinary


def test_attached_tiles_go_behind_the_others_in_units():
    _, ranges, units, launches = ask(8, 2, 128, 128, 0b1001, ROWS)
    assert ranges == [(1, 0, 0, 86, 0, 1), (1, 16, 0, 90, 1, 1),                                # row 2's two tiles, one range each
                      (0, 0, 0, 128, 2, 2), (0, 0, 128, 216, 2, 2), (2, 0, 0, 128, 4, 2), (2, 0, 128, 235, 4, 2)]
    assert units == [(2, 2, 4), (2, 3, 5)]                                                      # one unit of two tiles: ordinal 0, ordinal 1
    assert launches == [("mc_px_sums2_bfloat_hd128", 4, 2), ("mc_px_pv2_bfloat_hd128", 4, 2),
                        ("mc_ax_sums_bfloat_hd128", 4, 2), ("mc_ax_pv_bfloat_hd128", 4, 2), ("mc_px_reduce_bfloat_hd128", 8, 4)]
    # seven attached tiles of one long chunk and a short one at T = 4: units of 4 and 3 tiles, every tile one range under the rule
    _, ranges, units, _ = ask(4, 4, 128, -1, 0b11, [(80, 64), (17, 128)])
    assert units == [(4, 0, 1, 2, 3), (3, 4, 5, 6)] and [e[4:] for e in ranges] == [(i, 1) for i in range(7)]


@pytest.mark.parametrize("keys", [-1, 128])
def test_a_call_without_an_attached_row_plans_what_it_planned(keys):
    segs = rt.segments(*zip(*ROWS))
    want = rt.ranges(segs, rt.tiles(segs), rt.default_keys if keys < 0 else rt.keys_of(keys))
    for mask in (0, 0b0010):   # no row attached; the attached row is not in the call
        _, ranges, units, launches = ask(8, 2, 128, keys, mask, ROWS)
        assert ranges == [e[:6] for e in want] and units == []
        assert launches == [("mc_px_sums2_bfloat_hd128", 4, len(want)), ("mc_px_pv2_bfloat_hd128", 4, len(want))] + \
            ([("mc_px_reduce_bfloat_hd128", 8, len(want))] if keys > 0 else [])
