"""Kernel-level parity of the batched and ragged decode kernels (metalchat_amd/csrc/kernels/batch_kernels.hip), each launched BY NAME
through the Part-1 seam and compared with a plain float64 / oracle restatement of the same operation, with the project's roundings
to T written out:

  * the B-row GEMV `mc_b_gemv_{i4,w}_bfloat_e{0,1,2}` at every B from 1 to 8, at in_features whose per-wave slice (K / 8) runs the
    main loop alone, the tail loop alone and both, at int4 groups of 128, 256, 1024, K and 0 (one scale per row), and its three
    epilogues as exact compositions with its own e0, written at a row stride wider than the row;
  * the per-row rmsnorm, step state (mc_b_rows_begin), embedding (bfloat and int8 tables), RoPE + cache write, attention and picks,
    lockstep and `_rows`, each row in a cache of its own with a NaN guard behind it, idle rows left alone word for word.

The tests use the decoder only as the host-side packer of weights (mc_decoder_weight_ptrs), so the GEMV reads exactly the HBM layout
a batch reads.  NaN logits are out of scope: no reference semantics exist for them."""
import numpy as np
import pytest

import modelgen as mg
import parity
from oracle import mc_oracle as mo
from test_attn_kernels_gpu import oracle_attention
from test_sampler_gpu import SP, fused_sample

pytestmark = pytest.mark.gpu
BF16 = 0
PB = 64
NAN = 0x7FC0
GUARD = 512               # bf16 NaN elements between two rows' caches (and behind the last one)
BG_THREADS = 512          # mc_b_gemv_*: 8 waves


# ------------------------------------------------------------------------------------------ helpers
def bf(x):
    return mo.to_bf16(np.asarray(x, np.float32))


def f(bits):
    return mo.from_bf16(bits)


def bf16_rne64(y):
    """float64 -> bf16 bits, rounded ONCE (nearest, ties to even): the float32 rounding can be off by a step at ties"""
    y = np.asarray(y, np.float64)
    b = bf(y).astype(np.int32)
    best, bd = b.copy(), np.abs(f(b.astype(np.uint16)).astype(np.float64) - y)
    for d in (-1, 1):
        c = b + d
        ok = (c & 0x7FFF) != 0x7FFF
        ok &= ((c ^ b) & 0x8000) == 0                 # do not cross the sign
        c = np.where(ok, c, b)
        cd = np.abs(f(c.astype(np.uint16)).astype(np.float64) - y)
        take = (cd < bd) | ((cd == bd) & ((c & 1) == 0) & (c != best))
        best, bd = np.where(take, c, best), np.where(take, cd, bd)
    return best.astype(np.uint16)


def ulp_bf16(v):
    """one bf16 step at the binade of v (float values); the smallest step for 0"""
    a = np.abs(np.asarray(v, np.float64))
    _, e = np.frexp(a)
    return np.where(a == 0, 2.0 ** -133, np.maximum(np.ldexp(1.0, e - 8), 2.0 ** -133))


def steps(a, b):
    return np.abs(parity.bf16_ordinal(a) - parity.bf16_ordinal(b))


def states(n):
    """n step_state records (kernels/abi.h: 12 words, pinned by its static_assert), every word a distinct value so that a stray write shows"""
    return (np.arange(n * 12, dtype=np.int32).reshape(n, 12) + 1000)


ST_TOKEN, ST_POS, ST_KV, ST_SLOT, ST_STEP, ST_ROPE = 0, 1, 2, 3, 5, 6


def state_at(n_kv):
    st = np.zeros(12, np.int32)
    st[ST_POS], st[ST_KV], st[ST_SLOT], st[ST_ROPE], st[9] = n_kv - 1, n_kv, n_kv - 1, n_kv - 1, 1
    return st


# ------------------------------------------------------------------------------------------ B-row GEMV
# K slices (kslice = K / 8 per wave, 128-weight chunks; int4 rounds of U = 4 chunks, bfloat rounds of U = 2):
#   int4   K = 1024: 1 chunk, tail alone      K = 2048: 2 chunks, tail alone    K = 4096: 4 chunks, main alone (1 round)
#          K = 5120: 5 chunks, 1 round + 1    K = 14336: 14 chunks, 3 rounds + 2
#   bfloat K = 1024: 1 chunk, tail alone      K = 2048: 2 chunks, main alone    K = 4096 / 14336: 4 / 14 chunks, main alone
#          K = 5120: 5 chunks, 2 rounds + 1
I4, W = "i4", "w"
GEMV_CASES = [
    # fmt, K, group, out_features.  The loader takes int4 groups that are powers of two dividing K, or 0: one scale per row
    # (ngroups = 1), which is how a K of 5120 or 14336 gets a single group
    (I4, 1024, 128, 48), (I4, 1024, 1024, 16), (I4, 2048, 256, 336), (I4, 2048, 0, 48),
    (I4, 4096, 128, 6144), (I4, 4096, 1024, 48), (I4, 4096, 4096, 16),
    (I4, 5120, 256, 336), (I4, 5120, 0, 16), (I4, 5120, 1024, 48), (I4, 2048, 2048, 48),
    (I4, 14336, 128, 48), (I4, 14336, 1024, 336), (I4, 14336, 0, 16),
    (W, 1024, 0, 48), (W, 2048, 0, 336), (W, 4096, 0, 6144), (W, 5120, 0, 16), (W, 14336, 0, 48),
    pytest.param(I4, 14336, 256, 6144, marks=pytest.mark.slow), pytest.param(W, 14336, 0, 6144, marks=pytest.mark.slow),
]
XMAG = [1.0, 1e-2, 30.0, 0.0, 1e2, 0.1, 3.0, 1e-3]   # activation row r ~ N(0, XMAG[r]); row 3 all zero


class Packed:
    """one out x K matrix packed by a decoder (its `output` linear) as the batch reads it, and its dequantised rows"""

    def __init__(self, acc, fmt, K, group, out, seed):
        import metalchat_amd as mc

        rng = np.random.default_rng(seed)
        self.fmt, self.K, self.group, self.out = fmt, K, group, out
        cfg = mg.tiny_cfg(BF16, dim=K, n_heads=4, n_kv_heads=2, head_dim=64, ffn_dim=256, n_layers=1, vocab=out, max_seq_len=16)
        if fmt == I4:
            self.dec = mc.Decoder(acc, **mg.decoder_kwargs(cfg, weight_format=mc.WFMT_I4, group_size=128))
            ng = K // group if group else 1
            q = rng.integers(-8, 8, size=(out, K), dtype=np.int8)          # all 16 nibble values
            q[0, :16] = np.arange(-8, 8)
            # scales of both signs over 8 binades, bfloat values (T(s) = s), all normal
            s = (rng.choice([-1.0, 1.0], (out, ng)) * np.exp2(rng.uniform(-9, -1, (out, ng)))).astype(np.float32)
            s = f(bf(s))
            self.dec.load_linear(-1, "output", mc.WFMT_I4, q, s, group)
            self.q, self.s = q, s
        else:
            self.dec = mc.Decoder(acc, **mg.decoder_kwargs(cfg))
            w = rng.normal(0, 1, (out, K)) * np.exp2(rng.integers(-4, 4, (out, 1))) / np.sqrt(K)
            self.w = bf(w)
            self.dec.load_linear(-1, "output", mc.WFMT_T, self.w)
        self.wptr, self.sptr, rows, inf, self.ng = self.dec.weight_ptrs(-1, "output")
        assert (rows, inf) == (out, K)

    def rows(self, r0, r1):
        """Wd[r0:r1] as float64: int4 dequantised as T(T(q - 8) T(s)) -- exact in float32, rounded once to bfloat"""
        if self.fmt == W:
            return f(self.w[r0:r1]).astype(np.float64)
        G = self.group or self.K
        srep = np.repeat(self.s[r0:r1], G, axis=1)
        return f(bf(self.q[r0:r1].astype(np.float32) * srep)).astype(np.float64)

    def reference(self, x):
        """y64 = Wd . x and sum_k |Wd_k x_k| per (row of x, output), in blocks of rows"""
        xf = f(x).astype(np.float64)
        y = np.zeros((x.shape[0], self.out))
        a = np.zeros_like(y)
        for r0 in range(0, self.out, 512):
            wd = self.rows(r0, min(self.out, r0 + 512))
            y[:, r0:r0 + wd.shape[0]] = (wd @ xf.T).T
            a[:, r0:r0 + wd.shape[0]] = (np.abs(wd) @ np.abs(xf).T).T
        return y, a

    def launch(self, acc, x, epi=0, ldy=None, y_init=None, y_rows=None):
        """mc_b_gemv_* as batch.cc launches it (batch_plan.h plan_batch_gemv): out / 16 workgroups of 512 threads; B = rows of x; y rows at stride ldy"""
        import metalchat_amd as mc

        B = x.shape[0]
        width = self.out // 2 if epi == 2 else self.out
        ldy = ldy or width
        y_rows = y_rows or B
        yb = acc.to_device(y_init.reshape(-1) if y_init is not None else np.zeros(y_rows * ldy, np.uint16))
        wrap = lambda p: acc.wrap(p, 1 << 40) if p else None
        mc.KernelTask(acc.load(f"mc_b_gemv_{self.fmt}_bfloat_e{epi}"), (self.out // 16 * BG_THREADS, 1, 1), (BG_THREADS, 1, 1),
                      [wrap(self.wptr), wrap(self.sptr), acc.to_device(np.ascontiguousarray(x).reshape(-1)), yb, np.uint32(self.K),
                       np.uint32(self.ng), np.uint32(self.group), np.uint32(B), np.uint32(ldy)])()
        acc.wait()
        return yb.download(np.uint16, y_rows * ldy).reshape(y_rows, ldy)

    def release(self):
        self.dec.release()


def activations(K, seed):
    rng = np.random.default_rng(seed)
    return bf(rng.normal(0, 1, (8, K)) * np.array(XMAG)[:, None])


def acc_bound(K, a):
    """worst case of the fp32 accumulation: a wave sums its K / 8 exact bf16 x bf16 products into one fp32 accumulator (the MFMA
    adds each product with at most one rounding), then the 8 wave partials are added in order -- at most K / 8 + 7 roundings of
    relative size 2^-24 on partial sums bounded by sum_k |Wd_k x_k|, so |acc - y64| <= gamma_{K/8+7} * sum |.|, and
    gamma_n = n u / (1 - n u) <= (n + 1) u for n u < 2^-10"""
    return (K / 8 + 8) * 2.0 ** -24 * a


def check_e0(got, y64, a, K, what):
    """got: bf16 bits [B, out] = T(acc)"""
    g = f(got).astype(np.float64)
    assert np.all(np.isfinite(g)), what
    err = np.abs(g - y64)
    bound = 0.5 * ulp_bf16(g) + acc_bound(K, a)
    worst = np.unravel_index(np.argmax(err - bound), err.shape)
    assert np.all(err <= bound), f"{what}: |got - y64| {err[worst]:.4g} > bound {bound[worst]:.4g} at {worst}"
    ty = bf16_rne64(y64)
    frac = float(np.mean(got != ty))
    assert frac <= 0.01, f"{what}: {frac:.4f} of the outputs differ from T(y64) (allowed 0.01)"
    # normwise, as parity.check measures it: against the correctly rounded result T(y64).  (Against y64 itself even T(y64)
    # reaches 2.1e-3 > 2^-9 on these rows, where a few large outputs carry the norm: one rounding to bfloat is up to 2^-8
    # relative, so that comparison gets the bound 2^-8 plus the accumulation's share.)
    tyf = f(ty).astype(np.float64)
    nrm = np.linalg.norm(g - tyf) / max(np.linalg.norm(tyf), 1e-300)
    assert nrm <= 2.0 ** -9, f"{what}: normwise relative error against T(y64) {nrm:.3g}"
    nrm64 = np.linalg.norm(g - y64) / max(np.linalg.norm(y64), 1e-300)
    lim64 = 2.0 ** -8 + 1.01 * np.linalg.norm(acc_bound(K, a)) / max(np.linalg.norm(y64), 1e-300)
    assert nrm64 <= lim64, f"{what}: normwise relative error against y64 {nrm64:.3g} > {lim64:.3g}"
    return frac


@pytest.mark.parametrize("fmt,K,group,out", GEMV_CASES)
def test_b_gemv_store_matches_float64_at_every_batch_size(acc, fmt, K, group, out):
    P = Packed(acc, fmt, K, group, out, seed=K + out + group)
    x = activations(K, seed=K + 1)
    y64, a = P.reference(x)
    got8 = P.launch(acc, x)
    check_e0(got8, y64, a, K, f"e0 {fmt} K{K} g{group} out{out} B8")
    assert np.all(got8[3] == 0), "the all-zero row gives +0.0"
    for B in range(1, 8):   # the first B rows of a B-row launch are the B = 8 launch's rows, bit for bit
        parity.exact(P.launch(acc, x[:B]), got8[:B], f"e0 {fmt} K{K} B{B} rows against B8")
    # row independence: row r alone (B = 1) and row r at index 7 of a B = 8 launch (the rows rotated) give the same bits
    rot = np.roll(x, -1, axis=0)                  # rot[i] = x[(i + 1) % 8]: x[0] sits at index 7
    got_rot = P.launch(acc, rot)
    parity.exact(got_rot, np.roll(got8, -1, axis=0), f"e0 {fmt} K{K}: rows moved to other indices")
    for r in (0, 2, 5):
        parity.exact(P.launch(acc, x[r:r + 1])[0], got8[r], f"e0 {fmt} K{K}: row {r} alone")
    P.release()


EPI_CASES = [(I4, 5120, 256, 336), (I4, 14336, 128, 48), (I4, 2048, 0, 64), (W, 5120, 0, 336), (W, 1024, 0, 48)]


def silu_T32(x):
    """gemv.h silu_T in float32: T(x / T(1 + T(exp(-x))))"""
    x = np.asarray(x, np.float32)
    with np.errstate(over="ignore"):
        e = f(bf(np.exp(-x.astype(np.float64)).astype(np.float32)))
    d = f(bf(np.float32(1.0) + e))
    return f(bf(x / d))


@pytest.mark.parametrize("fmt,K,group,out", EPI_CASES)
def test_b_gemv_epilogues_and_placement(acc, fmt, K, group, out):
    P = Packed(acc, fmt, K, group, out, seed=7 * K + out)
    x = activations(K, seed=K + 2)
    y64, a = P.reference(x)
    rng = np.random.default_rng(out)
    for B in (8, 5):
        xb = x[:B]
        e0 = P.launch(acc, xb)
        check_e0(e0, y64[:B], a[:B], K, f"e0 {fmt} K{K} B{B}")
        e0f = f(e0)
        # ---- placement: rows at stride ldy = out + 32 in a buffer of 8 rows of NaN; columns [out, ldy) and rows >= B keep NaN
        ldy = out + 32
        buf = np.full((8, ldy), NAN, np.uint16)
        got = P.launch(acc, xb, ldy=ldy, y_init=buf, y_rows=8)
        parity.exact(got[:B, :out], e0, f"e0 {fmt} K{K} B{B} at ldy {ldy}")
        parity.exact(got[:B, out:], buf[:B, out:], f"e0 {fmt} B{B}: the columns past out")
        parity.exact(got[B:], buf[B:], f"e0 {fmt} B{B}: the rows past B")
        # ---- e1: y preloaded with the residual R; T(R + T(acc)) in float32, bit for bit
        R = bf(rng.normal(0, 1, (B, out)) * np.abs(e0f).mean(axis=1, keepdims=True).clip(1e-3) * 4)
        buf1 = buf.copy()
        buf1[:B, :out] = R
        got1 = P.launch(acc, xb, epi=1, ldy=ldy, y_init=buf1, y_rows=8)
        ref1 = bf(f(R) + e0f)
        parity.exact(got1[:B, :out], ref1, f"e1 {fmt} K{K} B{B}: T(R + e0)")
        parity.exact(got1[:B, out:], buf1[:B, out:], f"e1 {fmt} B{B}: the columns past out")
        parity.exact(got1[B:], buf1[B:], f"e1 {fmt} B{B}: the rows past B")
        # e1 against float64: the roundings T(acc), then R + . in float32 and T(.) (together <= (1/2 + 2^-16) of a step of the
        # result), and the accumulation bound of e0
        g1 = f(got1[:B, :out]).astype(np.float64)
        b1 = (0.5 + 2.0 ** -16) * ulp_bf16(g1) + 0.5 * ulp_bf16(e0f) + acc_bound(K, a[:B])
        assert np.all(np.abs(g1 - (f(R) + y64[:B])) <= b1), f"e1 {fmt} K{K} B{B}: against float64"
        # ---- e2: rows (2j, 2j + 1) as w1 | w3 pairs into ldy = out / 2
        got2 = P.launch(acc, xb, epi=2)
        ga, gb = e0f[:, 0::2], e0f[:, 1::2]
        ref2 = bf(silu_T32(ga) * gb)
        # the device exp and numpy's may differ in the last float place, which can move T(exp(-x)) and so the result by one
        # bfloat step; nothing else differs
        d = steps(got2, ref2)
        assert d.max() <= 1, f"e2 {fmt} K{K} B{B}: {d.max()} bf16 steps from silu_T(e0[2j]) * e0[2j+1]"
        assert np.mean(d != 0) <= 0.01, f"e2 {fmt} K{K} B{B}: {np.mean(d != 0):.4f} of outputs off by one step"
        # e2 against float64: silu(a) b with a, b each within the e0 bound, then the T roundings of silu_T and of the product
        a64, b64 = y64[:B, 0::2], y64[:B, 1::2]
        ea = 0.5 * ulp_bf16(ga) + acc_bound(K, a[:B, 0::2])
        eb = 0.5 * ulp_bf16(gb) + acc_bound(K, a[:B, 1::2])
        with np.errstate(over="ignore"):
            sil = a64 / (1 + np.exp(-a64))
        g2 = f(got2).astype(np.float64)
        b2 = 1.1 * np.abs(b64) * ea + (np.abs(sil) + 1.1 * ea) * eb + 4 * ulp_bf16(np.abs(sil * b64)) + 2 * ulp_bf16(g2)
        assert np.all(np.abs(g2 - sil * b64) <= b2), f"e2 {fmt} K{K} B{B}: against float64"
    P.release()


# ------------------------------------------------------------------------------------------ rmsnorm
@pytest.mark.parametrize("dim", [2048, 4096])
def test_b_rmsnorm_rows(acc, dim):
    import metalchat_amd as mc

    rng = np.random.default_rng(dim)
    B, eps = 8, np.float32(1e-5)
    scales = np.logspace(-3, 3, B)
    x = bf(rng.normal(0, 1, (B, dim)) * scales[:, None])
    w = bf(rng.uniform(0.5, 1.5, dim))
    k = acc.load("mc_b_rmsnorm_bfloat")

    def run(xs):
        out = acc.to_device(np.full(xs.size, NAN, np.uint16))
        mc.KernelTask(k, (1024, xs.shape[0], 1), (1024, 1, 1), [acc.to_device(xs.reshape(-1)), acc.to_device(w), out, np.uint32(dim), eps])()
        acc.wait()
        return out.download(np.uint16, xs.size).reshape(xs.shape)

    got = run(x)
    xf = f(x).astype(np.float64)
    inv = 1.0 / np.sqrt(np.mean(xf * xf, axis=1, keepdims=True) + float(eps))
    ref = bf16_rne64(f(w).astype(np.float64) * xf * inv)   # rmsnorm_row_body: T(w x inv), one rounding to T
    d = steps(got, ref)
    assert d.max() <= 1, f"rmsnorm dim {dim}: {d.max()} bf16 steps from float64"
    for r in (0, 3, 7):
        parity.exact(run(x[r:r + 1])[0], got[r], f"rmsnorm row {r} alone")


# ------------------------------------------------------------------------------------------ step state
def begin_ref(rows, stop, max_seq, B, advance):
    rows = rows.copy()
    for r in range(B):
        pos = int(rows[r, ST_POS])
        if pos < 0:
            continue
        if advance:
            if pos >= max_seq - 1 or int(rows[r, ST_TOKEN]) in stop:
                rows[r, ST_POS] = -1
                continue
            pos += 1
            rows[r, ST_POS] = pos
            rows[r, ST_STEP] += B
        rows[r, ST_KV], rows[r, ST_SLOT], rows[r, ST_ROPE] = pos + 1, pos, pos
    return rows


def test_b_rows_begin_table(acc):
    import metalchat_amd as mc

    B, S = 8, 256
    rows = states(10)
    # token 0 of a call: row 0 at 0, a row at max_seq - 1, an idle row (3), rows across a 64-slot boundary
    for r, (tok, pos) in enumerate([(5, 0), (6, 10), (7, S - 1), (8, -1), (9, 63), (10, 5), (11, 100), (12, 7)]):
        rows[r, ST_TOKEN], rows[r, ST_POS], rows[r, ST_STEP] = tok, pos, r
    stop = [2, 128001, 77]
    buf = acc.to_device(rows.reshape(-1))
    k = acc.load("mc_b_rows_begin")

    def launch(stop_ids, advance):
        sb = acc.to_device(np.array(stop_ids or [0], np.int32))
        mc.KernelTask(k, (64, 1, 1), (64, 1, 1), [buf, sb, np.int32(len(stop_ids)), np.int32(S), np.int32(B), np.int32(advance)])()
        acc.wait()
        return buf.download(np.int32, 120).reshape(10, 12)

    exp = begin_ref(rows, stop, S, B, 0)
    parity.exact(launch(stop, 0), exp, "token 0 of a call (advance = 0)")
    # the picks of step 0: a stop id (rows 0, 4), picks that are not stop ids (1, 5, 6, 7), the row at max_seq - 1 (2)
    for r, tok in zip(range(8), [2, 99, 99, 2, 128001, 0, 1, 78]):
        exp[r, ST_TOKEN] = tok
    buf.upload(exp.reshape(-1))
    exp = begin_ref(exp, stop, S, B, 1)
    parity.exact(launch(stop, 1), exp, "a chained step with stops")
    for r, tok in zip(range(8), [2, 77, 99, 2, 3, 4, 5, 6]):
        exp[r, ST_TOKEN] = tok
    buf.upload(exp.reshape(-1))
    exp = begin_ref(exp, stop, S, B, 1)
    got = launch(stop, 1)
    parity.exact(got, exp, "a second chained step")
    assert [int(p) for p in got[:8, ST_POS]] == [-1, -1, -1, -1, -1, 7, 102, 9]
    # no stop ids: only the end of the cache stops a row
    for r, tok in zip(range(8), [2, 77, 99, 2, 128001, 77, 2, 128001]):
        exp[r, ST_TOKEN] = tok
    buf.upload(exp.reshape(-1))
    exp = begin_ref(exp, [], S, B, 1)
    parity.exact(launch([], 1), exp, "a chained step without stop ids")
    parity.exact(exp[8:], states(10)[8:], "rows 8 and 9 (past B)")


# ------------------------------------------------------------------------------------------ embedding
@pytest.mark.parametrize("q8", [False, True])
def test_b_embed_lockstep_and_rows(acc, q8):
    import metalchat_amd as mc

    B, dim, vocab = 8, 4096, 64
    rng = np.random.default_rng(3 + q8)
    if q8:
        tq = rng.integers(-128, 128, size=(vocab, dim), dtype=np.int8)
        ts = (rng.uniform(0.5, 1.5, vocab) * np.exp2(rng.integers(-12, -4, vocab))).astype(np.float32)
        ts[vocab - 1] = np.nan                                 # the idle row's token: a read of it shows as NaN
        table = lambda t: bf(tq[t].astype(np.float32) * f(bf(ts[t])))   # T(q T(s)): the product is exact in float32
        args = [None, acc.to_device(ts), acc.to_device(tq.reshape(-1))]
    else:
        tb = bf(rng.normal(0, 1, (vocab, dim)))
        tb[vocab - 1] = NAN
        table = lambda t: tb[t]
        args = [acc.to_device(tb.reshape(-1)), None, None]
    toks = np.array([0, 5, 63 - 1, 17, 17, 1, 40, vocab - 1], np.int32)
    out = acc.alloc(B * dim * 2)
    # lockstep: every row reads its token (the last row's too: NaN there is the table's); advance moves step_index by B once
    rows = states(B)
    rows[:, ST_TOKEN], rows[:, ST_STEP] = toks, np.arange(B)
    for advance in (0, 1):
        rb = acc.to_device(rows.reshape(-1))
        mc.KernelTask(acc.load("mc_b_embed_bfloat"), ((dim + 255) // 256 * 256, B, 1), (256, 1, 1),
                      args + [out, rb, np.uint32(dim), np.int32(advance), np.uint32(B)])()
        acc.wait()
        got = out.download(np.uint16, B * dim).reshape(B, dim)
        for r in range(B - 1):
            parity.exact(got[r], table(toks[r]), f"embed row {r} token {toks[r]} (q8 {q8})")
        exp = rows.copy()
        exp[:, ST_STEP] += B * advance
        parity.exact(rb.download(np.int32, B * 12).reshape(B, 12), exp, f"embed advance {advance}: the step state")
    # _rows: the last row idle (its token is valid, its table row all NaN): +0.0 bits, nothing read
    rows = states(B)
    rows[:, ST_TOKEN], rows[:, ST_POS] = toks, np.arange(B) * 3
    rows[B - 1, ST_POS] = -1
    rb = acc.to_device(rows.reshape(-1))
    out.upload(np.full(B * dim, NAN, np.uint16))
    mc.KernelTask(acc.load("mc_b_embed_rows_bfloat"), ((dim + 255) // 256 * 256, B, 1), (256, 1, 1), args + [out, rb, np.uint32(dim)])()
    acc.wait()
    got = out.download(np.uint16, B * dim).reshape(B, dim)
    for r in range(B - 1):
        parity.exact(got[r], table(toks[r]), f"embed_rows row {r}")
    parity.exact(got[B - 1], np.zeros(dim, np.uint16), "embed_rows: the idle row is +0.0")
    parity.exact(rb.download(np.int32, B * 12).reshape(B, 12), rows, "embed_rows leaves the step state alone")


# ------------------------------------------------------------------------------------------ RoPE + cache write
def rope_table(acc, S, hd, theta):
    import metalchat_amd as mc

    half = hd // 2
    cb, sb = acc.alloc(S * half * 4), acc.alloc(S * half * 4)
    mc.KernelTask(acc.load("mc_rope_table"), ((half + 63) // 64 * 64, S, 1), (64, 1, 1),
                  [cb, sb, np.uint32(S), np.uint32(hd), np.uint32(0), np.float32(theta)])()
    acc.wait()
    return cb, sb, cb.download(np.float32, S * half).reshape(S, half), sb.download(np.float32, S * half).reshape(S, half)


def guarded(per_row, B):
    """B rows' caches in one buffer, each followed by GUARD NaN: cache_stride = per_row[0].size + GUARD"""
    g = np.full(GUARD, NAN, np.uint16)
    return np.concatenate([np.concatenate([per_row[r].reshape(-1), g]) for r in range(B)])


def packed_partners(x):
    """natural [heads, hd] -> the GEMV's q / k layout: packed [2j] = natural [j], [2j + 1] = natural [j + hd / 2]"""
    h, hd = x.shape
    return np.ascontiguousarray(x.reshape(h, 2, hd // 2).transpose(0, 2, 1)).reshape(h, hd)


@pytest.mark.parametrize("H,KV,hd", [(16, 4, 64), (32, 2, 64), (16, 4, 128), (32, 2, 128)])
def test_b_rope_kv_lockstep_and_rows(acc, H, KV, hd):
    import metalchat_amd as mc

    S, theta = 200, 500000.0
    half = hd // 2
    cb, sb, fcos, fsin = rope_table(acc, S, hd, theta)
    rc, rs = np.zeros((S, half), np.float32), np.zeros((S, half), np.float32)
    L = mo.layout
    mo.rope_freqs(L(rc.shape), rc, L(rs.shape), rs, hd, 0, theta)
    # both evaluate the same double expressions, rounded to float
    parity.exact(fcos, rc, "mc_rope_table cos against rope_freqs")
    parity.exact(fsin, rs, "mc_rope_table sin against rope_freqs")
    positions = [0, 1, 63, 64, 65, S - 1, -1]   # -1: idle
    B = len(positions)
    rng = np.random.default_rng(H + hd)
    qn = bf(rng.normal(0, 1, (B, H, hd)))
    kn = bf(rng.normal(0, 1, (B, KV, hd)))
    vn = bf(rng.normal(0, 1, (B, KV, hd)))
    qkv = np.concatenate([np.stack([packed_partners(qn[r]) for r in range(B)]).reshape(B, -1),
                          np.stack([packed_partners(kn[r]) for r in range(B)]).reshape(B, -1), vn.reshape(B, -1)], axis=1)
    kc0 = bf(rng.normal(0, 30, (B, KV, S, hd)))
    vt0 = bf(rng.normal(0, 30, (B, KV, hd, S)))
    cstride = KV * S * hd + GUARD

    def expect(r, pos):
        q1, k1 = np.zeros((H, hd), np.uint16), np.zeros((KV, hd), np.uint16)
        mo.rope(BF16, L((H, hd)), q1, L((H, hd)), qn[r], L(rc.shape), rc, L(rs.shape), rs, 1, H, pos)
        mo.rope(BF16, L((KV, hd)), k1, L((KV, hd)), kn[r], L(rc.shape), rc, L(rs.shape), rs, 1, KV, pos)
        kc, vt = kc0[r].copy(), vt0[r].copy()
        kc[:, pos] = k1
        vt[:, :, pos] = vn[r]
        return q1, kc, vt

    def run(name, st, Bn):
        kb, vb = acc.to_device(guarded(kc0, Bn)), acc.to_device(guarded(vt0, Bn))
        qo = acc.to_device(np.full(Bn * H * hd, NAN, np.uint16))
        mc.KernelTask(acc.load(name), ((H + 2 * KV) * half, Bn, 1), (half, 1, 1),
                      [acc.to_device(np.ascontiguousarray(qkv[:Bn]).reshape(-1)), qo, kb, vb, cb, sb, acc.to_device(st.reshape(-1)),
                       np.uint32(H), np.uint32(KV), np.uint32(hd), np.uint32(S), np.uint64(cstride)])()
        acc.wait()
        return (qo.download(np.uint16, Bn * H * hd).reshape(Bn, H, hd), kb.download(np.uint16, Bn * cstride).reshape(Bn, cstride),
                vb.download(np.uint16, Bn * cstride).reshape(Bn, cstride))

    def check_row(q, kc, vt, r, pos, what):
        guard = np.full(GUARD, NAN, np.uint16)
        parity.exact(kc[r, -GUARD:], guard, f"{what}: the guard behind row {r}'s K cache")
        parity.exact(vt[r, -GUARD:], guard, f"{what}: the guard behind row {r}'s V cache")
        if pos < 0:
            parity.exact(kc[r, :-GUARD], kc0[r].reshape(-1), f"{what}: idle row {r}'s K cache")
            parity.exact(vt[r, :-GUARD], vt0[r].reshape(-1), f"{what}: idle row {r}'s V cache")
            assert np.all(q[r] == NAN), f"{what}: idle row {r}'s q written"
            return
        q1, ke, ve = expect(r, pos)
        parity.exact(q[r], q1, f"{what}: row {r} q at {pos}")
        parity.exact(kc[r, :-GUARD], ke.reshape(-1), f"{what}: row {r} K cache (slot {pos} only)")
        parity.exact(vt[r, :-GUARD], ve.reshape(-1), f"{what}: row {r} V cache (slot {pos} only)")

    for pos in (0, 64, S - 1):   # lockstep: every row at one position
        q, kc, vt = run("mc_b_rope_kv_bfloat", state_at(pos + 1), B - 1)
        for r in range(B - 1):
            check_row(q, kc, vt, r, pos, f"lockstep at {pos}")
    rows = states(B)
    for r, pos in enumerate(positions):
        rows[r] = state_at(pos + 1) if pos >= 0 else rows[r]
        rows[r, ST_POS] = pos
    q, kc, vt = run("mc_b_rope_kv_rows_bfloat", rows, B)
    for r, pos in enumerate(positions):
        check_row(q, kc, vt, r, pos, "rows")


# ------------------------------------------------------------------------------------------ attention
ATTN_SHAPES = [(2048, 32, 8, 128), (1000, 32, 4, 64), (104, 16, 1, 128)]   # S, H, KV, hd (n_rep 4, 8, 16)


def attn_rows(S, H, KV, hd, lens, seed):
    rng = np.random.default_rng(seed)
    B = len(lens)
    q = bf(rng.normal(0, 1, (B, H, hd)))
    kc = bf(rng.normal(0, 30, (B, KV, S, hd)))       # slots past a row's kv_len: garbage that must not matter
    vt = bf(rng.normal(0, 30, (B, KV, hd, S)))
    ks, vs = [], []
    for r, n in enumerate(lens):
        n = max(n, 0)
        k = bf(rng.normal(0, 0.4, (n, KV, hd)))
        v = bf(rng.normal(0, 0.5, (n, KV, hd)))
        kc[r, :, :n] = k.transpose(1, 0, 2)
        vt[r, :, :, :n] = v.transpose(1, 2, 0)
        ks.append(k)
        vs.append(v)
    return q, kc, vt, ks, vs


def attn_single(acc, qb, kb, vb, r, H, KV, hd, S, n, scale, cstride):
    """the batch-1 two-launch form on row r's cache: mc_attn_scores_bfloat + mc_attn_pv_bfloat with 1024 threads and one range"""
    import metalchat_amd as mc

    nsplit = (S + PB - 1) // PB
    st = acc.to_device(state_at(n))
    expv, psum = acc.alloc(H * S * 4), acc.alloc(H * nsplit * 4)
    out = acc.to_device(np.zeros(H * hd, np.uint16))
    mc.KernelTask(acc.load("mc_attn_scores_bfloat"), (nsplit * 256, KV, 1), (256, 1, 1),
                  [(qb, r * H * hd * 2), (kb, r * cstride * 2), expv, psum, None, st, np.uint32(H // KV), np.uint32(hd), np.uint32(S),
                   np.float32(scale), np.uint32(nsplit)])()
    mc.KernelTask(acc.load("mc_attn_pv_bfloat"), (hd // 16 * 1024, KV, 1), (1024, 1, 1),
                  [expv, psum, (vb, r * cstride * 2), out, st, np.uint32(H // KV), np.uint32(hd), np.uint32(S), np.uint32(nsplit),
                   acc.alloc(H * hd * 4), np.uint32(H)])()
    acc.wait()
    return out.download(np.uint16, H * hd).reshape(H, hd)


@pytest.mark.parametrize("ragged", [False, True])
@pytest.mark.parametrize("S,H,KV,hd", ATTN_SHAPES)
def test_b_attention_per_row(acc, S, H, KV, hd, ragged):
    import metalchat_amd as mc

    nsplit, n_rep = (S + PB - 1) // PB, H // KV
    scale = float(f(bf(np.array([hd ** -0.5])))[0])
    cstride = KV * S * hd + GUARD
    sfx = "_rows_bfloat" if ragged else "_bfloat"
    lens_all = [1, 63, 64, 65, S - 1, S]
    # ragged: one launch, every row at its own kv_len and an idle row; lockstep: two rows at each kv_len in turn
    runs = [lens_all + [-1]] if ragged else [[n, n] for n in lens_all]
    for i, lens in enumerate(runs):
        B = len(lens)
        q, kc, vt, ks, vs = attn_rows(S, H, KV, hd, lens, seed=S + i + 10 * ragged)
        qb, kb, vb = acc.to_device(q.reshape(-1)), acc.to_device(guarded(kc, B)), acc.to_device(guarded(vt, B))
        if ragged:
            st = states(B)
            for r, n in enumerate(lens):
                if n > 0:
                    st[r] = state_at(n)
                st[r, ST_POS] = n - 1 if n > 0 else -1
        else:
            st = state_at(lens[0])
        sentinel = np.full(B * H * S, -7.0, np.float32)
        expv, psum = acc.to_device(sentinel), acc.to_device(np.zeros(B * H * nsplit, np.float32))
        out = acc.to_device(np.full(B * H * hd, NAN, np.uint16))
        sb = acc.to_device(st.reshape(-1))
        mc.KernelTask(acc.load("mc_b_attn_scores" + sfx), (nsplit * 256, KV, B), (256, 1, 1),
                      [qb, kb, expv, psum, sb, np.uint32(n_rep), np.uint32(hd), np.uint32(S), np.float32(scale), np.uint32(nsplit),
                       np.uint64(cstride)])()
        mc.KernelTask(acc.load("mc_b_attn_pv" + sfx), (hd // 16 * 1024, KV, B), (1024, 1, 1),
                      [expv, psum, vb, out, sb, np.uint32(n_rep), np.uint32(hd), np.uint32(S), np.uint32(nsplit), np.uint64(cstride)])()
        acc.wait()
        got = out.download(np.uint16, B * H * hd).reshape(B, H, hd)
        ev = expv.download(np.float32, B * H * S).reshape(B, H * S)
        for r, n in enumerate(lens):
            what = f"{'rows' if ragged else 'lockstep'} S{S} row {r} kv_len {n}"
            if n < 0:
                parity.exact(got[r], np.zeros((H, hd), np.uint16), f"{what}: the idle row's output is +0.0")
                parity.exact(ev[r], sentinel[:H * S], f"{what}: the idle row's expv slice")
                continue
            parity.check(BF16, got[r], oracle_attention(q[r], ks[r], vs[r], n_rep, scale), rel=2e-3, max_ulp=1, max_frac=0.03,
                         scale_aware=True, what=what)
            parity.exact(got[r], attn_single(acc, qb, kb, vb, r, H, KV, hd, S, n, scale, cstride), f"{what}: against batch 1")
        guard = np.full(GUARD, NAN, np.uint16)
        for buf, name in ((kb, "K"), (vb, "V")):
            allb = buf.download(np.uint16, B * cstride).reshape(B, cstride)
            for r in range(B):
                parity.exact(allb[r, -GUARD:], guard, f"S{S}: the guard behind row {r}'s {name} cache")


# ------------------------------------------------------------------------------------------ picks
VOCABS = [2048, 2032, 128256]


def pick_rows(n, seed):
    """8 rows of bf16 logits: repeated maxima, a maximum of 0 first as -0 then +0 (and the reverse), a row of -inf, the maximum in
    the last element, ties everywhere, plain"""
    rng = np.random.default_rng(seed)
    x = rng.normal(0, 2, (8, n)).astype(np.float32)
    x[0, [n // 3, 7, n - 1, n // 2]] = 12.5                   # repeated maxima (6 sigma): the first is index 7
    x[1] = -np.abs(x[1]) - 0.5
    x[1, [n // 5, n // 2]] = [-0.0, 0.0]                       # max 0 first as -0
    x[2] = -np.inf
    x[3, n - 1] = 20.0                                         # in the last element, the last partial list
    x[4] = -np.abs(x[4]) - 0.5
    x[4, [11, n - 2]] = [0.0, -0.0]                            # max 0 first as +0
    x[5] = np.round(x[5] * 2) / 2                              # coarse: long runs of equal logits
    x[6, [0, n - 1]] = 15.0                                    # tie between the first and the last
    return bf(x)


def first_max(row):
    v = f(row).astype(np.float64)
    return int(np.flatnonzero(v == v.max())[0])                # -0 == +0 in float compare


@pytest.mark.parametrize("ragged", [False, True])
@pytest.mark.parametrize("n", VOCABS)
def test_b_argmax_rows(acc, n, ragged):
    import metalchat_amd as mc

    B = 8
    logits = pick_rows(n, n)
    rows = states(B)
    rows[:, ST_POS] = np.arange(B)
    rows[:, ST_STEP] = 3 * B + np.arange(B)[::-1]              # tokens_out slot of row r
    if ragged:
        rows[7, ST_POS] = -1
    lb = acc.to_device(logits.reshape(-1))
    rb = acc.to_device(rows.reshape(-1))
    tout = acc.to_device(np.full(5 * B, -1, np.int32))
    mc.KernelTask(acc.load("mc_b_argmax" + ("_rows_bfloat" if ragged else "_bfloat")), (1024, B, 1), (1024, 1, 1),
                  [lb, np.uint32(n), rb, tout])()
    acc.wait()
    got_rows = rb.download(np.int32, B * 12).reshape(B, 12)
    got_t = tout.download(np.int32, 5 * B)
    exp_t = np.full(5 * B, -1, np.int32)
    for r in range(B):
        if ragged and r == 7:
            parity.exact(got_rows[r], rows[r], "argmax_rows: the idle row's state")
            continue
        pick = first_max(logits[r])
        st1 = acc.to_device(np.zeros(12, np.int32))
        mc.KernelTask(acc.load("mc_argmax_bfloat"), (1024, 1, 1), (1024, 1, 1), [(lb, r * n * 2), np.uint32(n), st1, None])()
        acc.wait()
        one = int(st1.download(np.int32, 12)[0])
        assert got_rows[r, ST_TOKEN] == pick == one, f"vocab {n} row {r}: {got_rows[r, ST_TOKEN]} (first max {pick}, batch 1 {one})"
        exp_row = rows[r].copy()
        exp_row[ST_TOKEN] = pick
        parity.exact(got_rows[r], exp_row, f"argmax row {r}: only the token word changes")
        exp_t[rows[r, ST_STEP]] = pick
    parity.exact(got_t, exp_t, f"vocab {n}: tokens_out")


SEEDS = np.array([[0, 0], [123456789, 987654321], [5, 6]], np.uint64)


@pytest.mark.parametrize("ragged", [False, True])
@pytest.mark.parametrize("top_k", [1, 40, 128])
@pytest.mark.parametrize("n", VOCABS)
def test_b_default_sampler_rows(acc, n, top_k, ragged):
    import metalchat_amd as mc

    B, cap = 8, 4096
    x = pick_rows(n, n + top_k)
    x[2] = bf(np.random.default_rng(1).normal(0, 1, n))       # (a row of -inf has no distribution)
    x[7] = bf(np.random.default_rng(2).normal(0, 3, n))
    lb = acc.to_device(x.reshape(-1))
    kpad = 1
    while kpad < top_k:
        kpad *= 2
    chunk = max(512, kpad)
    while chunk < 2048 and -(-n // chunk) > 1024:
        chunk *= 2
    lists = -(-n // chunk)
    assert lists == {2048: 4, 2032: 4, 128256: 251}[n]        # 2032 and 128256: the last list partial
    cand = acc.alloc(B * lists * kpad * 8)
    mc.KernelTask(acc.load("mc_b_topk_candidates_bfloat"), (lists * 64, B, 1), (64, 1, 1),
                  [lb, np.uint32(n), np.uint32(kpad), cand, np.uint32(chunk)])()
    rt = lambda v: float(f(bf(np.array([v])))[0])
    seeds = acc.to_device(SEEDS.reshape(-1))
    for temperature, top_p in ((0.6, 0.95), (1.3, 1.0), (0.6, 1.0), (1.3, 0.95)):
        p = np.zeros(1, SP)
        p["k"], p["ncand"], p["cap"], p["nlists"], p["kpad"] = min(top_k, n), lists * kpad, cap, lists, kpad
        p["inv_temp"], p["top_p"] = rt(1.0 / rt(temperature)), rt(top_p)   # as mc_decoder_set_sampler forms them
        rows = states(B)
        rows[:, ST_POS] = np.arange(B)
        rows[:, ST_STEP] = 2 * B + np.arange(B)
        if ragged:
            rows[5, ST_POS] = -1
        rb = acc.to_device(rows.reshape(-1))
        tout = acc.to_device(np.full(3 * B, -1, np.int32))
        mc.KernelTask(acc.load("mc_b_sample" + ("_rows_bfloat" if ragged else "_bfloat")), (128, B, 1), (128, 1, 1),
                      [cand, p, seeds, np.uint32(len(SEEDS)), rb, tout], lds_bytes=cap * 8)()
        acc.wait()
        got_rows = rb.download(np.int32, B * 12).reshape(B, 12)
        got_t = tout.download(np.int32, 3 * B)
        exp_t = np.full(3 * B, -1, np.int32)
        for r in range(B):
            what = f"vocab {n} top_k {top_k} T {temperature} p {top_p} row {r}"
            if ragged and r == 5:
                parity.exact(got_rows[r], rows[r], f"{what}: the idle row's state")
                continue
            s0, s1 = (int(v) for v in SEEDS[rows[r, ST_STEP] % len(SEEDS)])
            otok = mo.sample_default(BF16, x[r], top_k=top_k, temperature=temperature, top_p=top_p, init_state=s0, init_seq=s1)
            one, _ = fused_sample(acc, BF16, x[r], top_k=top_k, temperature=temperature, top_p=top_p, seed=(s0, s1))
            assert got_rows[r, ST_TOKEN] == otok == one, f"{what}: {got_rows[r, ST_TOKEN]} (oracle {otok}, batch 1 {one})"
            exp_row = rows[r].copy()
            exp_row[ST_TOKEN] = otok
            parity.exact(got_rows[r], exp_row, f"{what}: only the token word changes")
            exp_t[rows[r, ST_STEP]] = otok
        parity.exact(got_t, exp_t, f"vocab {n} top_k {top_k}: tokens_out")
