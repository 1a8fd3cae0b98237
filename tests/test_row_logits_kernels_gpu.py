"""Kernel-level check of the row logit processors' launch (logit_kernels.hip: mc_b_logits_process_bfloat / _rows_bfloat;
include/metalchat_hip.h Part 2l), launched BY NAME through the Part-1 seam on hand-made bfloat16 logits [8][N] against the rule of
tests/logits_rule.py, bit for bit:

  * N = 2056: one whole chunk of 2048 and a second of 8, rows of whole 16-byte pieces, a last mask word of 8 bits; the input token
    N - 1 lies in a 16-byte piece.  N = 130: less than one chunk, 260-byte rows, so rows 1, 2, 3, 5, 6, 7 start off a 16-byte
    boundary and have elements in front of their first whole piece and behind their last; the input token lies among the latter.
    N = 130 once more with the counts one word off the logits' alignment: the whole row takes the element path;
  * rows 0 and 4 have nothing set; mask only, penalties only, both, and each of the three penalties alone; in the `_rows` form one
    row with settings is idle;
  * planted: counts on a positive, a negative, a zero and a -0.0 logit, a count on a banned token, the input token in the last,
    partial mask word, the maximum on a banned token, results half way between two bfloat16 values;
  * every processed row equals the rule; rows with nothing set and the idle row keep every bit; the guard elements in front of and
    behind the logits, the counts and the masks are untouched, as are the rows' states and the masks; counts change only at the
    input token of the active rows with penalties, by exactly 1, and not at all with count = 0;
  * mc_b_argmax_bfloat on the result picks the first allowed maximum."""
import numpy as np
import pytest

import logits_rule as lr
import parity
from oracle import mc_oracle as mo
from test_batch_kernels_gpu import ST_POS, ST_TOKEN, bf, f, states

pytestmark = pytest.mark.gpu
B, GUARD = 8, 64
NAN, CGUARD, MGUARD = 0x7FC0, -77, 0xA5A5A5A5
MASK, PENALTY = 1, 2
RL = np.dtype([("flags", np.uint32), ("rep", np.float32), ("inv_rep", np.float32), ("freq", np.float32), ("pres", np.float32),
               ("pad", np.uint32, (3,))])   # kernels/abi.h row_logits
# row: (masked, rep, freq, pres).  2^-8 puts 2.0 - freq * c - pres half way between two bfloat16 values for c = 1 and 3
SETTINGS = [(False, 1.0, 0.0, 0.0), (True, 1.0, 0.0, 0.0), (False, 1.5, 0.25, 0.5), (True, 1.25, 2.0 ** -8, 2.0 ** -8),
            (False, 1.0, 0.0, 0.0), (False, 1.5, 0.0, 0.0), (False, 1.0, 2.0 ** -8, 0.0), (False, 1.0, 0.0, 2.0 ** -8)]
P_POS, P_NEG, P_ZERO, P_NZERO, P_TIE1, P_TIE3, P_TIEREP, P_BANNED, P_BANNED_MAX, P_NZERO_FREE = 3, 5, 7, 9, 11, 13, 15, 17, 19, 21


def penalised(s):
    return not (s[1] == 1.0 and s[2] == 0.0 and s[3] == 0.0)


def inputs(N):
    rng = np.random.default_rng(N)
    x = bf(np.clip(rng.normal(0, 3, (B, N)), -9.0, 9.0))
    counts = np.where(rng.random((B, N)) < 0.1, rng.integers(1, 5, (B, N)), 0).astype(np.int32)
    allowed = rng.random((B, N)) < 0.5
    for p, v, c in ((P_POS, 4.0, 1), (P_NEG, -4.0, 2), (P_ZERO, 0.0, 1), (P_NZERO, -0.0, 3), (P_TIE1, 2.0, 1), (P_TIE3, 2.0, 3),
                    (P_TIEREP, -1.0078125, 1), (P_BANNED, 1.0, 2), (P_BANNED_MAX, 20.0, 0), (P_NZERO_FREE, -0.0, 0)):
        x[:, p] = bf(np.float32(v))
        counts[:, p] = c
        allowed[:, p] = p not in (P_BANNED, P_BANNED_MAX)
    assert (x[:, P_NZERO] == 0x8000).all()
    # the input token: the last token, in the last (partial) mask word; rows start with 0 or 1 of it
    allowed[:, N - 1] = True
    counts[:, N - 1] = np.arange(B) % 2
    return x, counts, allowed


def table():
    t = np.zeros(B, RL)
    for r, s in enumerate(SETTINGS):
        t[r]["flags"] = (MASK if s[0] else 0) | (PENALTY if penalised(s) else 0)
        if penalised(s):
            t[r]["rep"], t[r]["inv_rep"], t[r]["freq"], t[r]["pres"] = s[1], np.float32(1.0) / np.float32(s[1]), s[2], s[3]
    return t


def guarded(acc, body, guard_value, guard=GUARD):
    g = np.full(guard, guard_value, body.dtype)
    host = np.concatenate([g, body.reshape(-1), np.full(GUARD, guard_value, body.dtype)])
    return acc.to_device(host), host, guard * body.dtype.itemsize


# form: (kernel suffix, count argument or None, idle row or None)
FORMS = [("_bfloat", None, None), ("_rows_bfloat", 1, 3), ("_rows_bfloat", 0, 6)]


@pytest.mark.parametrize("N,cguard", [(2056, GUARD), (130, GUARD), (130, GUARD + 1)])
def test_processed_rows_equal_the_rule(acc, N, cguard):
    import metalchat_amd as mc

    x, counts, allowed = inputs(N)
    words = np.stack([lr.mask_words(allowed[r]) for r in range(B)])
    tab = table()
    assert N % 32 != 0 and words.shape[1] == (N + 31) // 32
    for sfx, count, idle in FORMS:
        what = f"N {N} counts guard {cguard} {sfx} count {count} idle {idle}"
        lb, lhost, loff = guarded(acc, x, np.uint16(NAN))
        cb, chost, coff = guarded(acc, counts, np.int32(CGUARD), cguard)
        mb, mhost, moff = guarded(acc, words, np.uint32(MGUARD))
        rows = states(B)
        rows[:, ST_POS] = np.arange(B)
        rows[:, ST_TOKEN] = N - 1
        if idle is not None:
            rows[idle, ST_POS] = -1
        rb = acc.to_device(rows.reshape(-1))
        tb = acc.to_device(tab.view(np.uint8))
        args = [(lb, loff), np.uint32(N), tb, (mb, moff), (cb, coff), rb]
        if count is not None:
            args.append(np.int32(count))
        gx = -(-N // 2048)
        mc.KernelTask(acc.load("mc_b_logits_process" + sfx), (gx * 256, B, 1), (256, 1, 1), args)()
        acc.wait()
        got_l = lb.download(np.uint16, lhost.size)
        got_c = cb.download(np.int32, chost.size)
        got_m = mb.download(np.uint32, mhost.size)
        parity.exact(rb.download(np.int32, B * 12).reshape(B, 12), rows, f"{what}: the rows' states")
        parity.exact(got_m, mhost, f"{what}: the masks and their guards")
        # the counts: + 1 at the input token of the active rows with penalties
        exp_c = counts.copy()
        for r, s in enumerate(SETTINGS):
            if penalised(s) and r != idle and count != 0:
                exp_c[r, N - 1] += 1
        exp_chost = chost.copy()
        exp_chost[cguard:cguard + B * N] = exp_c.reshape(-1)
        parity.exact(got_c, exp_chost, f"{what}: the counts and their guards")
        # the logits
        exp = x.copy()
        for r, s in enumerate(SETTINGS):
            if r == idle:
                continue
            exp[r] = lr.process(x[r], exp_c[r] if penalised(s) else None, allowed[r] if s[0] else None, *s[1:])
        parity.exact(got_l[:GUARD], lhost[:GUARD], f"{what}: the guard in front of the logits")
        parity.exact(got_l[GUARD + B * N:], lhost[GUARD + B * N:], f"{what}: the guard behind the logits")
        got = got_l[GUARD:GUARD + B * N].reshape(B, N)
        for r, s in enumerate(SETTINGS):
            parity.exact(got[r], exp[r], f"{what}: row {r} {s}")
            if not (s[0] or penalised(s)) or r == idle:
                parity.exact(got[r], x[r], f"{what}: row {r} keeps every bit")
        # what the planted values became (row 3: mask, rep 1.25, freq = pres = 2^-8; row 5: rep 1.5 alone)
        if idle != 3:
            assert np.isneginf(f(got[3, [P_BANNED, P_BANNED_MAX]])).all()
            assert got[3, P_NZERO_FREE] == 0x8000   # an uncounted, allowed -0.0 stays -0.0
        assert f(got[6])[P_TIE1] == 2.0 or idle == 6   # 2 - 2^-8: half way, to the even 2.0
        assert f(got[6])[P_TIE3] == 1.984375 or idle == 6   # 2 - 3 * 2^-8: half way, to the even 2 - 2^-6
        assert f(got[5])[P_TIEREP] == -1.515625   # -(1 + 2^-7) * 1.5 = -(1.5 + 1.5 * 2^-7): half way, to the even 1.5 + 2^-6
        # the greedy pick on the result: the first allowed maximum
        tout = acc.to_device(np.full(B, -1, np.int32))
        prow = states(B)
        prow[:, 5] = np.arange(B)   # step_index: the slot of tokens_out
        pb = acc.to_device(prow.reshape(-1))
        mc.KernelTask(acc.load("mc_b_argmax_bfloat"), (1024, B, 1), (1024, 1, 1), [(lb, loff), np.uint32(N), pb, tout])()
        acc.wait()
        picks = tout.download(np.int32, B)
        for r, s in enumerate(SETTINGS):
            assert picks[r] == lr.first_max(exp[r]), f"{what}: row {r} picked {picks[r]}"
            if s[0] and r != idle:
                assert allowed[r, picks[r]] and picks[r] != P_BANNED_MAX, f"{what}: row {r} picked the banned {picks[r]}"
            elif not penalised(s) or r == idle:
                assert picks[r] == P_BANNED_MAX   # (no mask: the planted maximum)
