"""MC_SAMPLER_DRAW's rule (include/metalchat_hip.h Part 2, DESIGN.md s.4 "A sampler that draws") in numpy float32: the ONE reference of the
draw tests.  It sits on top of the oracle's make_default_sampler chain -- mo.sample_default(..., taps=True), whose seven taps the device
reproduces bit for bit -- and the oracle's own PCG32; only the last phase is written here, one float32 operation per step, in the order the
header gives:

    m[j]  = masked[j] (tap 5), j = 0 .. k-1            sorted order, the zeros are a suffix
    total = ((0 + m[0]) + m[1]) + .. + m[k-1]          sequential, ascending j
    u     = the first uniform() of pcg32(seed0, seed1)
    t     = u * total
    c_j   = c_{j-1} + m[j] (c_{-1} = 0);  pos = the smallest j with c_j > t
    none (t rounded up to total; total is 0 or NaN): pos = the largest j with m[j] > 0, else 0
    token = ids[sidx[pos]] (tap 6)"""
import numpy as np

from oracle import mc_oracle as mo

F = np.float32


def position(m, u):
    """the rule's last phase on the masked row m (float32 [k]) and the uniform u -> pos"""
    m = np.asarray(m, F)
    total = F(0.0)
    for x in m:
        total = F(total + x)
    t = F(F(u) * total)
    c = F(0.0)
    for j, x in enumerate(m):
        c = F(c + x)
        if c > t:
            return j
    positive = np.flatnonzero(m > 0)
    return int(positive[-1]) if positive.size else 0


def uniform(seed0, seed1):
    return F(mo.pcg32_uniform(int(seed0), int(seed1)))


def draw(dt, logits, top_k=50, temperature=0.6, top_p=0.9, seed0=0, seed1=0, taps=False, with_pos=False):
    """one row of logits (storage array of element type dt) -> the vocabulary id MC_SAMPLER_DRAW picks with the pair (seed0, seed1);
    taps: also the chain's [7, k] table (the oracle's, untouched); with_pos: also the position in sorted order"""
    _, t = mo.sample_default(dt, logits, top_k=top_k, temperature=temperature, top_p=top_p, init_state=int(seed0), init_seq=int(seed1), taps=True)
    with np.errstate(all="ignore"):
        pos = position(t[5], uniform(seed0, seed1))
    out = (int(t[6][pos]),)
    if taps:
        out += (t,)
    if with_pos:
        out += (pos,)
    return out[0] if len(out) == 1 else out


def draw_many(dt, logits, pairs, top_k=50, temperature=0.6, top_p=0.9):
    """the picks and positions of one row under every pair of `pairs` (the chain runs once: it does not read the seeds) -> (tokens, positions, taps)"""
    _, t = mo.sample_default(dt, logits, top_k=top_k, temperature=temperature, top_p=top_p, taps=True)
    with np.errstate(all="ignore"):
        pos = np.array([position(t[5], uniform(a, b)) for a, b in pairs], np.int64)
    return t[6][pos].astype(np.int64), pos, t
