"""The rule of the row logit processors (include/metalchat_hip.h Part 2l) in numpy float32 -- the one reference every test of the
part compares with, bit for bit.  T is bfloat16, x the float value of a logit, every operation one float32 operation in the order
written:

    c  = counts[t]                                  (the step's input token counted already)
    x1 = c > 0 ? (x > 0 ? x * inv_rep : x * rep) : x        inv_rep = float32(1) / float32(rep)
    x2 = c > 0 ? x1 - (freq * float32(c) + pres) : x
    y  = allowed[t] ? T(x2) : -inf                  (an untouched x keeps its bits)
"""
import numpy as np

from oracle import mc_oracle as mo

NEG_INF = np.uint16(0xFF80)


def process(bits, counts=None, allowed=None, rep=1.0, freq=0.0, pres=0.0):
    """bits: bfloat16 bits [n] (uint16); counts: int [n] or None (all zero); allowed: bool [n] or None (no mask).
    Returns the processed row's bits."""
    bits = np.ascontiguousarray(bits, dtype=np.uint16)
    y = bits.copy()
    rep, freq, pres = np.float32(rep), np.float32(freq), np.float32(pres)
    if counts is not None and not (rep == 1 and freq == 0 and pres == 0):
        c = np.asarray(counts)
        x = mo.from_bf16(bits)
        inv_rep = np.float32(1.0) / rep
        with np.errstate(over="ignore", invalid="ignore"):
            x1 = np.where(x > 0, x * inv_rep, x * rep).astype(np.float32)
            x2 = (x1 - (freq * c.astype(np.float32) + pres).astype(np.float32)).astype(np.float32)
        y = np.where(c > 0, mo.to_bf16(x2), bits).astype(np.uint16)
    if allowed is not None:
        y = np.where(np.asarray(allowed, dtype=bool), y, NEG_INF).astype(np.uint16)
    return y


def mask_words(allowed):
    """bool [n] -> the uint32 words of mc_row_mask_set: bit t % 32 of word t / 32"""
    allowed = np.asarray(allowed, dtype=bool)
    nw = (allowed.size + 31) // 32
    padded = np.zeros(nw * 32, np.uint8)
    padded[: allowed.size] = allowed
    return np.packbits(padded, bitorder="little").view("<u4").astype(np.uint32)


def first_max(bits):
    """the greedy pick: the first index of the maximum of a row of bfloat16 bits"""
    return int(np.argmax(mo.from_bf16(np.asarray(bits, np.uint16))))
