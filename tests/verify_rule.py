"""The acceptance rule of mc_verify_rows (include/metalchat_hip.h Part 2f), restated in Python for the CPU and GPU tests.

A row's chunk is c[0 .. n): c[0] the row's last accepted token, c[1 .. n) its drafted tokens; pick[i] is the target's greedy pick
after chunk row i.  Draft i + 1 is accepted when it IS that pick and every draft before it was accepted:

    a = the largest a <= n - 1 with c[i + 1] == pick[i] for all i < a

and the token to feed next is pick[a].  A match behind the first mismatch does not count: the picks there were conditioned on a
token the target did not produce.

This is a RESTATEMENT of kernels/verify_kernels.hip mc_v_accept; test_verify_kernels_gpu.py binds the kernel to it on the device."""
import numpy as np


def accept(chunk, picks):
    """(a, next token) of one row"""
    chunk, picks = [int(t) for t in chunk], [int(t) for t in picks]
    assert len(chunk) == len(picks) >= 1
    a = 0
    while a < len(chunk) - 1 and chunk[a + 1] == picks[a]:
        a += 1
    return a, picks[a]


def accept_rows(chunks, picks):
    """per batch row (None: not in the call) -> accepted[B], next_tokens[B], -1 for a row not in the call"""
    acc, nxt = np.full(len(chunks), -1, np.int32), np.full(len(chunks), -1, np.int32)
    for r, (c, p) in enumerate(zip(chunks, picks)):
        if c is not None:
            acc[r], nxt[r] = accept(c, p)
    return acc, nxt
