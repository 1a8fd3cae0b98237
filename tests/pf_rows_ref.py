"""The references of test_pf_row_kernels_gpu.py (the row kernels of the one-prompt pass: kernels/prefill_kernels.hip mc_pf_embed*,
mc_pf_rmsnorm*, mc_pf_act_mul*, mc_pf_rope_cache*, mc_pf_scores* / mc_pf_pv*), without a device: each is the oracle's own kernel where the
operation is one, and plain float64 / float32 numpy with the project's roundings to T written out where it is not.
test_pf_rows_ref_cpu.py holds every one of them to the oracle at the GPU tests' shapes, with the GPU tests' caps, so that a cap is
known to be met by the reference alone before a kernel is held to it."""
import numpy as np

from oracle import mc_oracle as mo
from test_batch_kernels_gpu import bf, bf16_rne64, f, packed_partners
from test_rows_kernels_gpu import unpartner

BF16, F32 = 0, 1
L = mo.layout
THETA = 500000.0
NORM_REL = 2.0 ** -20     # the relative distance from the float64 normed value inside which the fp32 kernels' value lies (norm_span)


def rt(dt, x):
    """float32 values rounded to T (as float32 values)"""
    x = np.asarray(x, np.float32)
    return f(bf(x)) if dt == BF16 else x


def storage(dt, x):
    return mo.encode(dt, np.asarray(x, np.float32))


def values(dt, x):
    return mo.decode(dt, x)


# ------------------------------------------------------------------------------------------ A: embedding
def embed(dt, table, tokens, scale=None):
    """mo.embedding of the rows `tokens`, then (gemma) mo.scalar_mul by T(sqrt(dim)); storage of type dt"""
    tokens = np.asarray(tokens, np.int32).reshape(1, -1)
    dim = table.shape[1]
    out = np.zeros((1, tokens.size, dim), mo.np_dtype(dt))
    mo.embedding(dt, L(out.shape), out, L(tokens.shape), tokens, L(table.shape), table)
    out = out.reshape(tokens.size, dim)
    if scale is None:
        return out
    scaled = np.zeros_like(out)
    mo.scalar_mul(dt, L(out.shape), scaled, L(out.shape), out, float(scale))
    return scaled


def embed_q8(dt, q, s, tokens, scale=None):
    """the int8 table: T(T(q * T(s)) [* scale]) in float32 -- the first product is an 8-bit by 8-bit (bfloat) or 8-bit by 24-bit
    significand product rounded once, every step one IEEE multiply"""
    tokens = np.asarray(tokens, np.int64)
    v = rt(dt, q[tokens].astype(np.float32) * rt(dt, s[tokens])[:, None])
    if scale is not None:
        v = rt(dt, v * np.float32(scale))
    return storage(dt, v)


def embed_scale(dt, dim):
    """prefill.cc run_prefill: T(sqrt(dim))"""
    return np.float32(rt(dt, np.array([np.sqrt(np.float32(dim))], np.float32))[0])


# ------------------------------------------------------------------------------------------ B: rmsnorm
def rmsnorm64(x, w, eps, mu):
    """float64 rows (mu + w) x / sqrt(mean(x^2) + eps) of the float values x [M][dim], w [dim]"""
    x, w = np.asarray(x, np.float64), np.asarray(w, np.float64)
    inv = 1.0 / np.sqrt(np.mean(x * x, axis=1, keepdims=True) + float(eps))
    return (float(mu) + w) * x * inv


def bf16_neighbours(bits):
    """the bf16 values one step below and above (by ordinal; across zero the step is to the smallest value of the other sign)"""
    o = bits_ordinal(bits)
    return ordinal_bits(o - 1), ordinal_bits(o + 1)


def bits_ordinal(bits):
    b = np.asarray(bits).astype(np.int32)
    return np.where(b & 0x8000, -(b & 0x7FFF), b & 0x7FFF)


def ordinal_bits(o):
    o = np.asarray(o, np.int32)
    return np.where(o < 0, 0x8000 | (-o), o).astype(np.uint16)


def residual_span(res, v64):
    """bf16 rows with a residual: the kernel writes T(res + v), v = T(normed) within one step of T(v64).  Returns the ordinals
    (lo, hi) of T(res + v_lo) and T(res + v_hi), v_lo / v_hi the neighbours of T(v64): the sum in float32, monotone in v"""
    v_lo, v_hi = bf16_neighbours(bf16_rne64(v64))
    a, b = bits_ordinal(bf(f(res) + f(v_lo))), bits_ordinal(bf(f(res) + f(v_hi)))
    return np.minimum(a, b), np.maximum(a, b)


def outside(got, lo, hi):
    """bf16 steps by which `got` (bits) lies outside the ordinal span [lo, hi]"""
    g = bits_ordinal(got)
    return np.maximum(np.maximum(lo - g, g - hi), 0)


def oracle_rmsnorm(dt, x, w, eps, mu):
    out = np.zeros_like(x)
    mo.rmsnorm(dt, L(x.shape), out, L(x.shape), x, L(w.shape), w, float(eps), float(mu))
    return out


def norm_inputs(dt, M, dim, mu, seed):
    """rows scaled by logspace(-3, 3, M) (test_b_rmsnorm_rows), a residual of the rows' size, and a weight: U(0.5, 1.5) for mu = 0,
    U(-0.25, 0.25) for mu = 1 (as modelgen draws a gemma norm); storage of type dt"""
    rng = np.random.default_rng([seed, dim, int(mu)])
    x = storage(dt, rng.normal(0, 1, (M, dim)) * np.logspace(-3, 3, M)[:, None])
    res = storage(dt, rng.normal(0, 1, (M, dim)))
    w = storage(dt, rng.uniform(-0.25, 0.25, dim) if mu else rng.uniform(0.5, 1.5, dim))
    return x, res, w


# ------------------------------------------------------------------------------------------ C: activation
def silu64(a):
    a = np.asarray(a, np.float64)
    with np.errstate(over="ignore"):
        return a / (1.0 + np.exp(-a))


def gelu64(a):
    """the tanh form (kernel/gelu: 0.5 x (1 + tanh(sqrt(2 / pi) (x + 0.044715 x^3))))"""
    a = np.asarray(a, np.float64)
    return 0.5 * a * (1.0 + np.tanh(np.sqrt(2.0 / np.pi) * (a + 0.044715 * a ** 3)))


def oracle_silu_mul(dt, a, b):
    """mo.silu followed by mo.hadamard"""
    s, out = np.zeros_like(a), np.zeros_like(a)
    mo.silu(dt, L(a.shape), s, L(a.shape), a)
    mo.hadamard(dt, L(a.shape), out, L(a.shape), s, L(a.shape), b)
    return out


def all_bf16():
    return np.arange(65536, dtype=np.uint32).astype(np.uint16)


def is_nan16(bits):
    return (np.asarray(bits) & 0x7FFF) > 0x7F80


def interleave(a, b):
    """rows (2j, 2j + 1) of the fused w1|w3 output = (a_j, b_j)"""
    out = np.empty(a.shape[:-1] + (2 * a.shape[-1],), a.dtype)
    out[..., 0::2], out[..., 1::2] = a, b
    return out


# ------------------------------------------------------------------------------------------ D: rope and cache write
class RopeRef:
    """one prompt chunk of M rows behind wq|wk|wv: row r goes to cache slot start_pos + r and is rotated by table row rope_row0 + r.
    fused rows [M][(H + 2 KV) hd]: q heads, k heads (rotation partners adjacent: test_batch_kernels_gpu.packed_partners), v heads"""

    def __init__(self, dt, H, KV, hd, M, max_seq, start_pos, rope_row0, table_rows=64):
        self.dt, self.H, self.KV, self.hd, self.M, self.max_seq = dt, H, KV, hd, M, max_seq
        self.start_pos, self.rope_row0, self.table_rows = start_pos, rope_row0, table_rows
        self.NQ, self.nb = (H + 2 * KV) * hd, (H + KV) * hd
        assert start_pos + M <= max_seq and rope_row0 + M <= table_rows
        half = hd // 2
        self.rc, self.rs = np.zeros((table_rows, half), np.float32), np.zeros((table_rows, half), np.float32)
        mo.rope_freqs(L(self.rc.shape), self.rc, L(self.rs.shape), self.rs, hd, 0, THETA)

    def rope(self, x, heads, pos):
        """mo.rope of natural rows [heads][hd] at table row pos"""
        o = np.zeros((heads, self.hd), mo.np_dtype(self.dt))
        mo.rope(self.dt, L(o.shape), o, L(o.shape), np.ascontiguousarray(x), L(self.rc.shape), self.rc, L(self.rs.shape), self.rs, 1, heads, pos)
        return o

    def split_row(self, row):
        """a fused row [NQ] -> natural q [H][hd], natural k [KV][hd], v [KV][hd]"""
        H, KV, hd = self.H, self.KV, self.hd
        return unpartner(row[:H * hd].reshape(H, hd)), unpartner(row[H * hd:self.nb].reshape(KV, hd)), row[self.nb:].reshape(KV, hd)

    def expect(self, x, kc0, vt0):
        """fused rows [M][NQ] (normed already where a norm applies) -> the q rows [M][H][hd] and the whole K [KV][max_seq][hd] and
        V [KV][hd][max_seq]: the initial content with exactly the call's slots replaced"""
        q = np.zeros((self.M, self.H, self.hd), mo.np_dtype(self.dt))
        kc, vt = kc0.copy(), vt0.copy()
        for r in range(self.M):
            qn, kn, vn = self.split_row(x[r])
            q[r] = self.rope(qn, self.H, self.rope_row0 + r)
            kc[:, self.start_pos + r] = self.rope(kn, self.KV, self.rope_row0 + r)
            vt[:, :, self.start_pos + r] = vn
        return q, kc, vt

    def normed64(self, x, q_w, k_w, eps, mu):
        """the q / k norm in float64, in the fused layout: [M][NQ] float64 with the heads of a norm that is None (and v) left as they
        are, and the mask of the elements a norm applies to.  The norm's weight is indexed by the NATURAL element: fused [2j] takes
        w[j], fused [2j + 1] takes w[j + hd / 2]"""
        H, KV, hd = self.H, self.KV, self.hd
        v = values(self.dt, x).astype(np.float64)
        out, on = v.copy(), np.zeros(v.shape, bool)
        for w, first, heads in ((q_w, 0, H), (k_w, H, KV)):
            if w is None:
                continue
            wf = values(self.dt, packed_partners(w.reshape(1, hd))[0]).astype(np.float64)
            cols = slice(first * hd, (first + heads) * hd)
            hv = v[:, cols].reshape(-1, hd)
            out[:, cols] = rmsnorm64(hv, wf, eps, mu).reshape(self.M, heads * hd)
            on[:, cols] = True
        return out, on

    def norm_span(self, x, q_w, k_w, eps, mu):
        """bf16: the normed rows the rope may see.  The kernel's fp32 value of (mu + w) x inv lies within relative NORM_REL = 2^-20
        of the float64 one (at most ~ 12 roundings of 2^-24: the squares and the butterfly over a head, the mean, eps, the root, the
        quotient, mu + w and two products), so T of it is T(lo) or T(hi) or between: returns the fused rows (lo, hi) as bf16 bits --
        equal where every value that close rounds to the same bfloat16 -- and the mask of the ambiguous elements"""
        assert self.dt == BF16
        xn, on = self.normed64(x, q_w, k_w, eps, mu)
        d = np.abs(xn) * NORM_REL
        lo, hi = np.where(on, bf16_rne64(xn - d), x), np.where(on, bf16_rne64(xn + d), x)
        return lo.astype(np.uint16), hi.astype(np.uint16), lo != hi

    def corners(self, lo, hi, kc0, vt0):
        """the ropes of the four corners (lo / hi of a pair's first and of its second element): ordinals (min, max) per output of
        (q rows, K, V).  The rope's fp32 operations and T are monotone in each input, so the rope of any pair inside the span lies
        inside the span of the corners; where lo == hi for a whole pair the span is one value: T(xn64) roped by mo.rope"""
        first = (np.arange(self.NQ) % 2 == 0) | (np.arange(self.NQ) >= self.nb)
        cands = [self.expect(np.where(first, a, b), kc0, vt0) for a in (lo, hi) for b in (lo, hi)]
        out = []
        for gi in range(3):
            o = np.stack([bits_ordinal(c[gi]) for c in cands])
            out.append((o.min(axis=0), o.max(axis=0)))
        return out

    def inputs(self, seed, norms=False):
        """fused rows N(0, 1), caches N(0, 30), and (norms) the two weights U(-0.25, 0.25); storage of type dt"""
        rng = np.random.default_rng([seed, self.H, self.hd])
        x = storage(self.dt, rng.normal(0, 1, (self.M, self.NQ)))
        kc0 = storage(self.dt, rng.normal(0, 30, (self.KV, self.max_seq, self.hd)))
        vt0 = storage(self.dt, rng.normal(0, 30, (self.KV, self.hd, self.max_seq)))
        qw = storage(self.dt, rng.uniform(-0.25, 0.25, self.hd))
        kw = storage(self.dt, rng.uniform(-0.25, 0.25, self.hd))
        return (x, kc0, vt0, qw, kw) if norms else (x, kc0, vt0)


# the shapes of section D: M = 37 rows whose last one is the cache's last slot, behind a turned ring (rope_row0 != start_pos)
ROPE_M, ROPE_MAX_SEQ, ROPE_START, ROPE_ROW0 = 37, 56, 19, 3
ROPE_SHAPES = [(8, 2, 32), (16, 4, 64), (6, 2, 128), (4, 1, 256)]
NORM_EPS, NORM_MU = 1e-6, 1.0
NORM_SEED = 11


def rope_ref(dt, H, KV, hd):
    return RopeRef(dt, H, KV, hd, ROPE_M, ROPE_MAX_SEQ, ROPE_START, ROPE_ROW0)


# ------------------------------------------------------------------------------------------ E: two-pass attention
def prob_sum_bound(dt, S):
    """|sum of a row's probabilities - 1|: p_i = T(e_i inv), inv = 1 / sum_fp32(e), every e_i > 0.  The fp32 sum of at most S positive
    terms, the quotient and each product are within (S + 2) 2^-24 relative together, and each T() moves its p_i by at most u_T
    relative -- the unit roundoff of bfloat16's 8 significant bits, 2^-8: half a step of 2^-7 at the bottom of a binade; nothing
    more for float: |sum - 1| <= u_T (1 + eta) + eta, eta = (S + 2) 2^-24.  (All of a row's p_i can round the same way: a row of n
    equal scores is n times T(1 / n).)"""
    eta = (S + 2) * 2.0 ** -24
    u = 2.0 ** -8 if dt == BF16 else 0.0
    return u * (1 + eta) + eta
