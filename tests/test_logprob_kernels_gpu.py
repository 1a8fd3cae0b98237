"""Kernel-level check of the two log-probability launches (logprob_kernels.hip: mc_logprob_parts_* / mc_logprob_finish_*;
include/metalchat_hip.h Part 2n), launched BY NAME through the Part-1 seam on hand-made bfloat16 logits [8][N] against the rule of
tests/logprob_rule.py under the part's condition (never more than 1 float32 ulp, bit-equal on at least 999 of 1000 finite values,
the same -inf; ids and order exact):

  * N = 2056: one whole chunk of 2048 and a second of 8.  N = 130: less than one chunk, 260-byte rows, so rows 1, 2, 3, 5, 6, 7 start
    off a 16-byte boundary and have elements in front of their first whole piece and behind their last.  N = 4104: three chunks, in
    rows 5 and 6 the middle one entirely -inf;
  * top_n = 0, 1, 5 and 20;
  * planted: the maximum at index N - 1 (row 0), equal maxima on both sides of index 2048 (row 1; N = 130: of index 64), -0.0 / +0.0
    on top (row 2), a row with one finite logit (row 3: its token has exactly 0.0), a row with three finite logits (row 4: the tail
    of its top n is -inf in index order, and its token is banned: -inf);
  * both slot forms: the rows' states (token and step_index, the slots permuted inside a buffer of 16) -- plain and ragged, with
    one row idle -- and picks[m] with slot m;
  * the idle row's slots and the slots no row writes keep the fill, the guard words around every buffer, the logits and the rows'
    states are untouched."""
import numpy as np
import pytest

import logprob_rule as lpr
import parity
from test_batch_kernels_gpu import ST_POS, ST_STEP, ST_TOKEN, bf, states
from test_row_logits_kernels_gpu import GUARD, guarded

pytestmark = pytest.mark.gpu
B = 8
NAN, WGUARD = 0x7FC0, 0xA5A5A5A5
FILL = 0xFFFFFFFF
NEG = -np.inf
SLOTS = 8 + np.array([3, 0, 6, 1, 7, 2, 5, 4])   # step_index of row r: a permutation, the first 8 slots of 16 stay empty


def inputs(N):
    rng = np.random.default_rng(N)
    x = np.clip(rng.normal(0, 3, (B, N)), -9.0, 9.0).astype(np.float32)
    x[rng.random((B, N)) < 0.2] = NEG
    side = 2048 if N > 2049 else 64
    x[0, N - 1] = 12.0
    x[1, [side - 1, side + 1, 5]] = 11.0
    x[2] = np.minimum(x[2], -1.0)
    x[2, [9, 3, 77]] = [0.0, -0.0, 0.0]
    x[3] = NEG
    x[3, N - 2] = -3.5
    x[4] = NEG
    x[4, [N - 1, 17, 40]] = [1.0, 2.0, 1.0]
    if N == 4104:
        x[5:7, 2048:4096] = NEG
    bits = bf(x)
    assert bits[2, 3] == 0x8000
    tokens = np.array([N - 1, 5, 3, N - 2, 18, 1, N - 4, 7], np.int32)    # row 4's is banned
    for r in (5, 6, 7):
        x[r, tokens[r]] = 1.5   # (finite)
    bits = bf(x)
    return bits, tokens


def buffer_of(acc, words, value, dtype):
    """a device buffer of `words` elements filled with `value` between guards"""
    return guarded(acc, np.full(words, value, dtype), dtype.type(WGUARD) if dtype != np.uint64 else np.uint64(WGUARD))


# form: (kernel suffix, the slots come from the rows' states, idle row or None)
FORMS = [("_bfloat", True, None), ("_rows_bfloat", True, 6), ("_bfloat", False, None)]


@pytest.mark.parametrize("N", [2056, 130, 4104])
def test_records_equal_the_rule(acc, N):
    import metalchat_amd as mc

    bits, tokens = inputs(N)
    nchunk = -(-N // 2048)
    want_lp = np.stack([lpr.logprobs(bits[r]) for r in range(B)])
    compared = differing = 0
    for top_n in (0, 1, 5, 20):
        want_top = [lpr.top(bits[r], top_n) for r in range(B)]
        for sfx, from_rows, idle in FORMS:
            what = f"N {N} top_n {top_n} {sfx} {'rows' if from_rows else 'picks'} idle {idle}"
            nslots = 16 if from_rows else B
            slot_of = SLOTS if from_rows else np.arange(B)
            lb, lhost, loff = guarded(acc, bits, np.uint16(NAN))
            parts, phost, poff = buffer_of(acc, B * nchunk * 4, FILL, np.dtype(np.uint32))
            keys, khost, koff = buffer_of(acc, B * nchunk * max(top_n, 1), FILL, np.dtype(np.uint64))
            o_lp, lp_host, lp_off = buffer_of(acc, nslots, FILL, np.dtype(np.uint32))
            o_ids, ids_host, ids_off = buffer_of(acc, nslots * max(top_n, 1), FILL, np.dtype(np.uint32))
            o_top, top_host, top_off = buffer_of(acc, nslots * max(top_n, 1), FILL, np.dtype(np.uint32))
            rows = states(B)
            rows[:, ST_POS] = np.arange(B)
            rows[:, ST_TOKEN] = tokens
            rows[:, ST_STEP] = SLOTS
            if idle is not None:
                rows[idle, ST_POS] = -1
            rb = acc.to_device(rows.reshape(-1))
            pb = acc.to_device(tokens)
            state = rb if from_rows else None
            mc.KernelTask(acc.load("mc_logprob_parts" + sfx), (nchunk * 256, B, 1), (256, 1, 1),
                          [(lb, loff), np.uint32(N), np.uint32(top_n), (parts, poff), (keys, koff), state])()
            mc.KernelTask(acc.load("mc_logprob_finish" + sfx), (256, B, 1), (256, 1, 1),
                          [(lb, loff), np.uint32(N), np.uint32(top_n), np.uint32(nchunk), (parts, poff), (keys, koff), state, None if from_rows else pb,
                           np.uint32(nslots), (o_lp, lp_off), (o_ids, ids_off) if top_n else None, (o_top, top_off) if top_n else None])()
            acc.wait()
            # untouched: the logits and their guards, the rows' states, the picks, the guards of the scratch
            parity.exact(lb.download(np.uint16, lhost.size), lhost, f"{what}: the logits and their guards")
            parity.exact(rb.download(np.int32, B * 12).reshape(B, 12), rows, f"{what}: the rows' states")
            parity.exact(pb.download(np.int32, B), tokens, f"{what}: the picks")
            for buf, host, name in ((parts, phost, "parts"), (keys, khost, "keys")):
                got = buf.download(host.dtype, host.size)
                parity.exact(got[:GUARD], host[:GUARD], f"{what}: the guard in front of the {name}")
                parity.exact(got[-GUARD:], host[-GUARD:], f"{what}: the guard behind the {name}")
            g_lp = o_lp.download(np.uint32, lp_host.size)
            g_ids = o_ids.download(np.uint32, ids_host.size)
            g_top = o_top.download(np.uint32, top_host.size)
            # what is expected: the fill everywhere, the records in the active rows' slots
            e_lp, e_ids = lp_host.copy(), ids_host.copy()
            written = np.zeros(nslots, bool)
            for r in range(B):
                if r == idle:
                    continue
                s = slot_of[r]
                written[s] = True
                e_ids[GUARD + s * top_n:GUARD + (s + 1) * top_n] = want_top[r][0].view(np.uint32) if top_n else []
                n, k = lpr.check(g_lp[GUARD + s:GUARD + s + 1].view(np.float32), want_lp[r, tokens[r]:tokens[r] + 1], f"{what}: row {r}'s token", share=False)
                compared, differing = compared + n, differing + k
                if top_n:
                    n, k = lpr.check(g_top[GUARD + s * top_n:GUARD + (s + 1) * top_n].view(np.float32), want_top[r][1], f"{what}: row {r}'s top", share=False)
                    compared, differing = compared + n, differing + k
            if top_n == 0:
                parity.exact(g_ids, ids_host, f"{what}: no ids are written at top_n 0")
                parity.exact(g_top, top_host, f"{what}: no top values are written at top_n 0")
            else:
                parity.exact(g_ids, e_ids, f"{what}: the ids, the fill of the other slots and the guards")
            body = slice(GUARD, GUARD + nslots)
            assert (g_lp[body][~written] == FILL).all(), f"{what}: a slot without a record lost its fill"
            parity.exact(g_lp[:GUARD], lp_host[:GUARD], f"{what}: the guard in front of the token values")
            parity.exact(g_lp[GUARD + nslots:], lp_host[GUARD + nslots:], f"{what}: the guard behind the token values")
            if top_n:
                keep = np.ones(g_top.size, bool)
                keep[GUARD:GUARD + nslots * top_n] = ~np.repeat(written, top_n)
                parity.exact(g_top[keep], top_host[keep], f"{what}: the top values' fill and guards")
            # the planted rows
            tok = {r: g_lp[GUARD + slot_of[r]:GUARD + slot_of[r] + 1].view(np.float32)[0] for r in range(B) if r != idle}
            assert tok[3] == 0.0 and not np.signbit(tok[3]), f"{what}: the one finite logit"
            assert np.isneginf(tok[4]), f"{what}: a banned token"
            if top_n >= 5:
                ids = {r: g_ids[GUARD + slot_of[r] * top_n:GUARD + (slot_of[r] + 1) * top_n].view(np.int32) for r in range(B) if r != idle}
                side = 2048 if N > 2049 else 64
                assert ids[0][0] == N - 1
                assert ids[1][:3].tolist() == [5, side - 1, side + 1]
                assert ids[2][:3].tolist() == [3, 9, 77]
                assert ids[3][:3].tolist() == [N - 2, 0, 1]
                assert ids[4][:5].tolist() == [17, 40, N - 1, 0, 1]
    assert compared > 100
    lpr.check_share(compared, differing, f"N {N}")
