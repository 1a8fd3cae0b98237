"""The rule of row log-probabilities (include/metalchat_hip.h Part 2n) in numpy float64 -- the one reference every test of the part
compares with.  For one row, y[0..V) the bfloat16 logits the pick read (after the row's mask and penalties, before temperature and
truncation):

    M      = max y
    S      = sum over t of exp(double(y[t]) - double(M))        exp(-inf) = 0
    lse    = double(M) + log(S)
    lp[t]  = float32(double(y[t]) - lse)                         one rounding; a banned token's lp is -inf
    top n  = the n largest y by the sampler's key order (value descending, -0 == +0, then LOWER index), each with its lp

The model's distribution over the processed logits at temperature 1; not the sampler's truncated nucleus.

The order of a float64 sum can move a result across a float32 rounding boundary only, hence the condition every comparison of a
device (or chunked) evaluation with this one uses (check): never more than 1 float32 ulp apart, bit-equal on at least 999 of every
1000 finite values compared, and the same -inf."""
import numpy as np

CHUNK = 2048   # kernels/abi.h LOGPROB_CHUNK


def values(bits):
    """bfloat16 bits (uint16) -> float64"""
    b = np.ascontiguousarray(bits, dtype=np.uint16)
    return (b.astype(np.uint32) << 16).view(np.float32).astype(np.float64)


def lse(bits):
    d = values(bits)
    m = d.max()
    with np.errstate(divide="ignore"):
        return m + np.log(np.exp(d - m).sum())


def logprobs(bits):
    """lp[t] for the whole row, float32"""
    with np.errstate(invalid="ignore"):
        return (values(bits) - lse(bits)).astype(np.float32)


def order(bits):
    """every index of the row in the sampler's key order: value descending, -0 == +0, then lower index"""
    d = values(bits) + 0.0   # (-0.0 + 0.0 = +0.0: the two zeros compare equal anyway, this only documents it)
    return np.lexsort((np.arange(d.size), -d))


def top(bits, n):
    """(ids [n] int32, lp [n] float32) of the n most likely tokens"""
    ids = order(bits)[:n].astype(np.int32)
    return ids, logprobs(bits)[ids]


def lse_chunked(bits, chunk=CHUNK, threads=256):
    """The rule in the order the device evaluates it: per chunk of `chunk` logits its maximum m_c and s_c = sum exp(y - m_c) from
    per-thread partial sums (thread i of `threads` owns elements 8 i .. 8 i + 7 of the chunk), a xor-tree over each wave of 64, the
    waves in order; then M = max m_c and S = sum of s_c exp(m_c - M) in chunk order, chunks whose maximum is -inf skipped."""
    d = values(bits)
    per = chunk // threads
    ms, ss = [], []
    for c in range(0, d.size, chunk):
        ch = d[c:c + chunk]
        mc = ch.max()
        ms.append(mc)
        if mc == -np.inf:
            ss.append(0.0)
            continue
        e = np.zeros(chunk)
        e[:ch.size] = np.exp(ch - mc)
        t = np.zeros(threads)
        for j in range(per):                      # a thread adds its elements in index order
            t = t + e.reshape(threads, per)[:, j]
        s = t.reshape(threads // 64, 64)
        for off in (32, 16, 8, 4, 2, 1):
            s = s + s[:, np.arange(64) ^ off]
        acc = 0.0
        for w in range(threads // 64):
            acc = acc + s[w, 0]
        ss.append(acc)
    M = max(ms)
    S = 0.0
    for s, m in zip(ss, ms):
        if m > -np.inf:
            S = S + s * np.exp(m - M)
    return M + np.log(S)


def ulps(a, b):
    """distance in float32 ulps of two finite float32 arrays"""
    def key(x):
        i = np.ascontiguousarray(x, dtype=np.float32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)
    return np.abs(key(a) - key(b))


def check_share(compared, differing, what=""):
    """bit-equal on at least 999 of every 1000 finite values compared"""
    assert differing * 1000 <= compared, f"{what}: {differing} of {compared} finite values differ from the rule"


def check(got, want, what="", share=True):
    """the condition of the part: `got` against the rule's `want` (float32 arrays of one shape).  Returns (compared, differing);
    share=False leaves the 999-in-1000 condition to the caller, who adds up the counts of several calls (check_share)."""
    got, want = np.asarray(got, np.float32).reshape(-1), np.asarray(want, np.float32).reshape(-1)
    assert got.shape == want.shape, what
    assert not np.isnan(want).any() and not np.isnan(got).any(), f"{what}: NaN"
    fin = np.isfinite(want)
    assert (np.isfinite(got) == fin).all() and (got[~fin] == want[~fin]).all(), f"{what}: the infinite values differ"
    u = ulps(got[fin], want[fin])
    assert (u <= 1).all(), f"{what}: {int(u.max())} ulp from the rule"
    differing = int((u != 0).sum())
    if share:
        check_share(int(fin.sum()), differing, what)
    return int(fin.sum()), differing
