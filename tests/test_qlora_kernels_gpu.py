"""Kernel-level tests of what a QLoRA decoder adds to the batched weight kernels (include/metalchat_hip.h Part 2i), each kernel
launched BY NAME through the Part-1 seam over weights packed by a decoder, as test_batch_kernels_gpu.Packed packs them:

  * int8 weights, `mc_b_gemv_i8_bfloat_e{0,1,2}`: e0 against float64 with Wd = T(T(q) T(s)) written out, at in_features that run the
    tail loop alone, the main loop alone and both, in groups of 0 (one scale per row), 32, 128 and K, q over all of [-128, 127];
    every B from 1 to 8 and rows moved to other indices bit for bit;
  * two zero-tolerance ties to the tested paths: an int8 matrix of values in [-8, 7] is its int4 twin bit for bit, and an int4 matrix
    in groups of 32 / 64 whose scales are equal within every 128 is its group-128 twin bit for bit; then groups of 32 with
    independent scales against float64;
  * adaptors, `mc_b_gemv_{i4,i8,w}_bfloat_e{0,1,2}_l`: every output inside the interval [f(p64 - d), f(p64 + d)] of the monotone
    f(p) = T(base + T(T(p) T(scale))) around the float64 adaptor sum, e1 / e2 as exact compositions with the kernel's own e0,
    no-op adaptors, NaN guards around a and y;
  * the wide forms `mc_wb_gemv_*` (int8, group 32, _l) at M up to 64 and every tile count, and the head `mc_vhead_i8_bfloat` at M up
    to 128: every row bit for bit the narrow kernel's on 8-row slices."""
import numpy as np
import pytest

import modelgen as mg
import parity
from test_batch_kernels_gpu import BG_THREADS, I4, NAN, W, XMAG, Packed, activations, bf, bf16_rne64, check_e0, f, silu_T32, steps
from test_verify_kernels_gpu import VH_ROWS, activations128
from test_wide_kernels_gpu import activations64, launch_wide

pytestmark = pytest.mark.gpu
BF16 = 0
I8 = "i8"


class QPacked(Packed):
    """Packed for int8 as well, and with the integer values and the scales given: q [out][K] int8, s [out][K / group or 1] bfloat values"""

    def __init__(self, acc, fmt, K, group, out, seed, q=None, s=None):
        import metalchat_amd as mc

        rng = np.random.default_rng(seed)
        self.fmt, self.K, self.group, self.out = fmt, K, group, out
        cfg = mg.tiny_cfg(BF16, dim=K, n_heads=4, n_kv_heads=2, head_dim=64, ffn_dim=256, n_layers=1, vocab=out, max_seq_len=16)
        wf = mc.WFMT_I4 if fmt == I4 else mc.WFMT_I8
        self.dec = mc.Decoder(acc, **mg.decoder_kwargs(cfg, weight_format=wf, group_size=128))
        ng = K // group if group else 1
        if q is None:
            lo, hi = (-8, 8) if fmt == I4 else (-128, 128)
            q = rng.integers(lo, hi, size=(out, K), dtype=np.int8)
            q[0, :hi - lo] = np.arange(lo, hi)                          # every value present
        if s is None:
            # Packed's draw: both signs over 8 binades, bfloat values (T(s) = s), all normal
            s = f(bf((rng.choice([-1.0, 1.0], (out, ng)) * np.exp2(rng.uniform(-9, -1, (out, ng)))).astype(np.float32)))
        assert q.shape == (out, K) and s.shape == (out, ng)
        self.dec.load_linear(-1, "output", wf, q, s, group)
        self.q, self.s = q, s
        self.wptr, self.sptr, rows, inf, self.ng = self.dec.weight_ptrs(-1, "output")
        assert (rows, inf, self.ng) == (out, K, ng)

    def rows(self, r0, r1):
        """Wd[r0:r1] as float64: T(T(q) T(s)) -- (float)q * s is exact in float32 (8 x 8 significant bits), rounded once to bfloat"""
        G = self.group or self.K
        srep = np.repeat(self.s[r0:r1], G, axis=1)
        return f(bf(self.q[r0:r1].astype(np.float32) * srep)).astype(np.float64)


def packed(acc, fmt, K, group, out, seed):
    return Packed(acc, W, K, 0, out, seed) if fmt == W else QPacked(acc, fmt, K, group, out, seed)


# ------------------------------------------------------------------------------------------ int8, e0 against float64
# kslice = K / 8 per wave in 128-weight chunks, rounds of 4: K = 1024 one chunk (tail alone), 2048 two (tail alone), 4096 four (main
# alone), 5120 five (both).  The loader takes groups that are powers of two: group K only where K is one
I8_CASES = [(K, g) for K in (1024, 2048, 4096, 5120) for g in (0, 32, 128, K) if g & (g - 1) == 0]


@pytest.mark.parametrize("K,group", I8_CASES)
def test_b_gemv_i8_store_matches_float64_at_every_batch_size(acc, K, group):
    x = activations(K, seed=K + 1)
    for out in (48, 336):
        P = QPacked(acc, I8, K, group, out, seed=K + out + group)
        assert set(np.unique(P.q)) == set(range(-128, 128))
        y64, a = P.reference(x)
        got8 = P.launch(acc, x)
        what = f"e0 i8 K{K} g{group} out{out}"
        frac = check_e0(got8, y64, a, K, what + " B8")
        print(f"{what}: {frac:.5f} of the outputs differ from T(y64)")
        assert np.all(got8[3] == 0), "the all-zero row gives +0.0"
        for B in range(1, 8):
            parity.exact(P.launch(acc, x[:B]), got8[:B], f"{what} B{B} rows against B8")
        parity.exact(P.launch(acc, np.roll(x, -1, axis=0)), np.roll(got8, -1, axis=0), f"{what}: rows moved to other indices")
        for r in (0, 5):
            parity.exact(P.launch(acc, x[r:r + 1])[0], got8[r], f"{what}: row {r} alone")
        P.release()


@pytest.mark.parametrize("K,group,out", [(5120, 32, 336), (1024, 0, 48), (4096, 128, 336)])
def test_b_gemv_i8_epilogues_and_placement(acc, K, group, out):
    """the int8 e1 / e2 over the full range of q as exact compositions of the kernel's own e0 (test_batch_kernels_gpu's statements),
    written at a row stride wider than the row into NaN"""
    P = QPacked(acc, I8, K, group, out, seed=11 * K + out)
    x = activations(K, seed=K + 8)
    rng = np.random.default_rng(out + K)
    for B in (8, 5):
        xb = x[:B]
        e0 = P.launch(acc, xb)
        e0f = f(e0)
        ldy = out + 32
        buf = np.full((8, ldy), NAN, np.uint16)
        got = P.launch(acc, xb, ldy=ldy, y_init=buf, y_rows=8)
        parity.exact(got[:B, :out], e0, f"e0 i8 K{K} B{B} at ldy {ldy}")
        assert np.all(got[:B, out:] == NAN) and np.all(got[B:] == NAN), f"e0 i8 K{K} B{B}: y outside [B][out] written"
        R = bf(rng.normal(0, 1, (B, out)) * np.abs(e0f).mean(axis=1, keepdims=True).clip(1e-3) * 4)
        buf1 = buf.copy()
        buf1[:B, :out] = R
        got1 = P.launch(acc, xb, epi=1, ldy=ldy, y_init=buf1, y_rows=8)
        parity.exact(got1[:B, :out], bf(f(R) + e0f), f"e1 i8 K{K} B{B}: T(R + e0)")
        assert np.all(got1[:B, out:] == NAN) and np.all(got1[B:] == NAN), f"e1 i8 K{K} B{B}: y outside [B][out] written"
        got2 = P.launch(acc, xb, epi=2)
        d = steps(got2, bf(silu_T32(e0f[:, 0::2]) * e0f[:, 1::2]))
        assert d.max() <= 1 and np.mean(d != 0) <= 0.01, f"e2 i8 K{K} B{B}: {d.max()} steps, {np.mean(d != 0):.4f} of outputs off"
    P.release()


# ------------------------------------------------------------------------------------------ the two ties
@pytest.mark.parametrize("K,group", [(1024, 32), (1024, 0), (4096, 128), (5120, 32), (5120, 256)])
def test_int8_of_int4_values_is_the_int4_kernel(acc, K, group):
    """both dequantise to the same bfloat and feed the same MFMAs"""
    out = 336
    P4 = QPacked(acc, I4, K, group, out, seed=K + group + 3)
    P8 = QPacked(acc, I8, K, group, out, seed=0, q=P4.q, s=P4.s)
    x = activations(K, seed=K + 4)
    R = bf(np.random.default_rng(K).normal(0, 1, (8, out)))
    for epi in (0, 1, 2):
        init = R.copy() if epi == 1 else None
        parity.exact(P8.launch(acc, x, epi=epi, y_init=init), P4.launch(acc, x, epi=epi, y_init=init),
                     f"mc_b_gemv_i8 e{epi} K{K} g{group} against mc_b_gemv_i4 on the same values")
    P4.release()
    P8.release()


@pytest.mark.parametrize("K", [1024, 4096, 5120])
@pytest.mark.parametrize("group", [32, 64])
def test_int4_small_groups_with_equal_scales_are_group_128(acc, K, group):
    out = 336
    P128 = QPacked(acc, I4, K, 128, out, seed=K + group + 5)
    Pg = QPacked(acc, I4, K, group, out, seed=0, q=P128.q, s=np.repeat(P128.s, 128 // group, axis=1))
    x = activations(K, seed=K + 6)
    for epi in (0, 2):
        parity.exact(Pg.launch(acc, x, epi=epi), P128.launch(acc, x, epi=epi), f"int4 e{epi} K{K}: groups of {group} against groups of 128")
    P128.release()
    Pg.release()


@pytest.mark.parametrize("K", [1024, 4096, 5120])
def test_int4_groups_of_32_match_float64(acc, K):
    x = activations(K, seed=K + 7)
    for out in (48, 336):
        P = QPacked(acc, I4, K, 32, out, seed=K + out)
        y64, a = P.reference(x)
        got8 = P.launch(acc, x)
        frac = check_e0(got8, y64, a, K, f"e0 i4 K{K} g32 out{out}")
        print(f"e0 i4 K{K} g32 out{out}: {frac:.5f} of the outputs differ from T(y64)")
        for B in (1, 3, 7):
            parity.exact(P.launch(acc, x[:B]), got8[:B], f"e0 i4 K{K} g32 B{B} rows against B8")
        P.release()


# ------------------------------------------------------------------------------------------ adaptors
class Adaptor:
    """a [rows][lda] with `cols` columns used and NaN everywhere else (the padding columns, and the rows past `live`); lora_b
    [out][cols] with all-zero 16-column blocks per row, as a fused matrix has outside a row's own adaptor, and an all-zero row"""

    def __init__(self, acc, out, cols, rows, live, seed, lda=None):
        rng = np.random.default_rng(seed)
        self.cols, self.lda = cols, lda or cols + 8
        self.a = np.full((rows, self.lda), NAN, np.uint16)
        self.a[:live, :cols] = bf(rng.normal(0, 1, (live, cols)) * np.array(XMAG)[np.arange(live) % 8, None])
        b = rng.uniform(-1, 1, (out, cols)) * (0.25 / np.sqrt(16))
        nblk = cols // 16
        if nblk > 1:   # row r keeps block r % nblk only
            keep = (np.arange(cols)[None, :] // 16) == (np.arange(out)[:, None] % nblk)
            b = np.where(keep, b, 0.0)
        b[5] = 0.0
        self.b = bf(b)
        self.upload(acc)

    def upload(self, acc):
        self.ab, self.bb = acc.to_device(self.a.reshape(-1)), acc.to_device(self.b.reshape(-1))

    def sums(self, n):
        """p64 [n][out] and sum_c |a_c b_c|"""
        af, bfl = f(self.a[:n, :self.cols]).astype(np.float64), f(self.b).astype(np.float64)
        return af @ bfl.T, np.abs(af) @ np.abs(bfl).T


def launch_l(acc, P, x, A, scale, epi=0, ldy=None, y_init=None, y_rows=None):
    """mc_b_gemv_*_l as batch.cc launches it: the plain kernel's arguments, then (a, lda, lora_b, lora_cols, lora_scale)"""
    import metalchat_amd as mc

    B = x.shape[0]
    width = P.out // 2 if epi == 2 else P.out
    ldy = ldy or width
    y_rows = y_rows or B
    yb = acc.to_device(y_init.reshape(-1) if y_init is not None else np.zeros(y_rows * ldy, np.uint16))
    wrap = lambda p: acc.wrap(p, 1 << 40) if p else None
    mc.KernelTask(acc.load(f"mc_b_gemv_{P.fmt}_bfloat_e{epi}_l"), (P.out // 16 * BG_THREADS, 1, 1), (BG_THREADS, 1, 1),
                  [wrap(P.wptr), wrap(P.sptr), acc.to_device(np.ascontiguousarray(x).reshape(-1)), yb, np.uint32(P.K), np.uint32(P.ng),
                   np.uint32(P.group), np.uint32(B), np.uint32(ldy), A.ab, np.uint32(A.lda), A.bb, np.uint32(A.cols), np.float32(scale)])()
    acc.wait()
    return yb.download(np.uint16, y_rows * ldy).reshape(y_rows, ldy)


def f_of_p(base_bits, p64, scale):
    """f(p) = T(base + T(T(p) T(scale))) as the kernel evaluates it: p rounded once to bfloat, the product exact in float32 and
    rounded to bfloat, the sum formed in float32 and rounded to bfloat (scale is a bfloat value)"""
    tp = f(bf16_rne64(p64))
    prod = f(bf(tp * np.float32(scale)))
    return bf(f(base_bits) + prod)


def in_interval(got, base, p64, d, scale, what):
    """f is monotone in p (rising for scale > 0, falling for scale < 0): got between f(p64 - d) and f(p64 + d)"""
    e0, e1 = parity.bf16_ordinal(f_of_p(base, p64 - d, scale)), parity.bf16_ordinal(f_of_p(base, p64 + d, scale))
    lo, hi = np.minimum(e0, e1), np.maximum(e0, e1)
    g = parity.bf16_ordinal(got)
    bad = (g < lo) | (g > hi)
    assert not bad.any(), f"{what}: {int(bad.sum())} outputs outside [f(p64 - d), f(p64 + d)], first at {np.argwhere(bad)[0]}"


LORA_CASES = [(fmt, K, cols) for fmt in (I4, I8, W) for K in (1024, 4096) for cols in (16, 48, 96)]


@pytest.mark.parametrize("fmt,K,cols", LORA_CASES)
def test_b_gemv_l_adaptor_term(acc, fmt, K, cols):
    out = 336 if K == 1024 else 48
    P = packed(acc, fmt, K, 32, out, seed=K + cols + 9)
    x = activations(K, seed=K + cols)
    rng = np.random.default_rng(cols)
    for B in (8, 5):
        xb = x[:B]
        A = Adaptor(acc, out, cols, 8, B, seed=K + cols + B)
        base = P.launch(acc, xb)                                       # the plain e0 on the same x: T(v), exact
        p64, pabs = A.sums(B)
        d = cols * 2.0 ** -24 * pabs                                   # cols fp32 additions on partial sums bounded by sum |a_c b_c|
        ldy = out + 32
        buf = np.full((8, ldy), NAN, np.uint16)
        for scale in (2.0, -0.5):
            what = f"{fmt} K{K} cols{cols} B{B} scale {scale}"
            got = launch_l(acc, P, xb, A, scale, ldy=ldy, y_init=buf, y_rows=8)
            e0l = got[:B, :out]
            in_interval(e0l, base, p64, d, scale, f"e0_l {what}")
            assert not np.array_equal(e0l, base), f"e0_l {what}: the adaptor changed nothing"
            parity.exact(f(e0l[:, 5]), f(base[:, 5]), f"e0_l {what}: an all-zero lora_b row returns base")
            assert np.all(got[:B, out:] == NAN) and np.all(got[B:] == NAN), f"e0_l {what}: y outside [B][out] written"
            # e1: T(R + e0_l) in float32, bit for bit; e2: silu_T(e0_l[2j]) * e0_l[2j + 1], test_batch_kernels_gpu's statement of e2
            R = bf(rng.normal(0, 1, (B, out)) * np.abs(f(e0l)).mean(axis=1, keepdims=True).clip(1e-3) * 4)
            buf1 = buf.copy()
            buf1[:B, :out] = R
            got1 = launch_l(acc, P, xb, A, scale, epi=1, ldy=ldy, y_init=buf1, y_rows=8)
            parity.exact(got1[:B, :out], bf(f(R) + f(e0l)), f"e1_l {what}: T(R + e0_l)")
            assert np.all(got1[:B, out:] == NAN) and np.all(got1[B:] == NAN), f"e1_l {what}: y outside [B][out] written"
            buf2 = np.full((8, out // 2 + 16), NAN, np.uint16)
            got2 = launch_l(acc, P, xb, A, scale, epi=2, ldy=out // 2 + 16, y_init=buf2, y_rows=8)
            e0f = f(e0l)
            dd = steps(got2[:B, :out // 2], bf(silu_T32(e0f[:, 0::2]) * e0f[:, 1::2]))
            assert dd.max() <= 1 and np.mean(dd != 0) <= 0.01, f"e2_l {what}: {dd.max()} steps, {np.mean(dd != 0):.4f} off"
            assert np.all(got2[:B, out // 2:] == NAN) and np.all(got2[B:] == NAN), f"e2_l {what}: y outside [B][out / 2] written"
        # a no-op adaptor: a = 0 returns base as a value (T(base + T(0 * scale)))
        A.a[:B, :cols] = 0
        A.upload(acc)
        parity.exact(f(launch_l(acc, P, xb, A, -0.5)), f(base), f"e0_l {fmt} K{K} cols{cols} B{B}: a = 0 returns base")
    P.release()


# ------------------------------------------------------------------------------------------ the wide forms
WIDE_MS = [1, 16, 17, 33, 64]
WIDE_OUT = {0: 2064, 1: 2064, 2: 2080}
# fmt, K, group, lora_cols (0: the plain kernel)
WIDE_CASES = [(I8, 1024, 32, 0), (I8, 4096, 0, 0), (I4, 1024, 32, 0), (I4, 4096, 32, 0),
              (I4, 1024, 32, 48), (I8, 4096, 128, 16), (W, 1024, 0, 96)]


def launch_wide_l(acc, P, xb, M, epi, tiles, y_init, A, scale):
    import metalchat_amd as mc

    rows, ldy = y_init.shape
    yb = acc.to_device(y_init.reshape(-1))
    wrap = lambda p: acc.wrap(p, 1 << 40) if p else None
    groups = (P.out // 16 + tiles - 1) // tiles
    mc.KernelTask(acc.load(f"mc_wb_gemv_{P.fmt}_bfloat_e{epi}_l"), (groups * BG_THREADS, 1, 1), (BG_THREADS, 1, 1),
                  [wrap(P.wptr), wrap(P.sptr), xb, yb, np.uint32(P.K), np.uint32(P.ng), np.uint32(P.group), np.uint32(M), np.uint32(P.out),
                   np.uint32(ldy), A.ab, np.uint32(A.lda), A.bb, np.uint32(A.cols), np.float32(scale)])()
    acc.wait()
    return yb.download(np.uint16, rows * ldy).reshape(rows, ldy)


@pytest.mark.parametrize("epi", [0, 1, 2])
@pytest.mark.parametrize("fmt,K,group,cols", WIDE_CASES)
def test_wb_gemv_rows_are_the_batch_gemv_rows(acc, fmt, K, group, cols, epi):
    out = WIDE_OUT[epi]
    width = out // 2 if epi == 2 else out
    ldy, rows, scale = width + 16, 66, -0.5
    P = packed(acc, fmt, K, group, out, seed=5 * K + group + epi + cols)
    x = activations64(K, seed=K + group + 13)
    R = bf(np.random.default_rng(K + epi).normal(0, 1, (64, out)))
    full = Adaptor(acc, out, cols, 64, 64, seed=K + cols) if cols else None

    def narrow8(r):
        init = R[r:r + 8].copy() if epi == 1 else None
        if not cols:
            return P.launch(acc, x[r:r + 8], epi=epi, y_init=init)
        A8 = Adaptor(acc, out, cols, 8, 8, seed=0, lda=full.lda)
        A8.a, A8.b = full.a[r:r + 8].copy(), full.b
        A8.upload(acc)
        return launch_l(acc, P, x[r:r + 8], A8, scale, epi=epi, y_init=init)

    narrow = np.concatenate([narrow8(r) for r in range(0, 64, 8)])
    if not cols and epi == 0:
        y64, a = P.reference(x)
        check_e0(narrow, y64, a, K, f"mc_b_gemv e0 {fmt} K{K} g{group}")
    for M in WIDE_MS:
        xm = x.copy()
        xm[M:] = NAN                                  # the activation rows at and past M must reach nothing
        xb = acc.to_device(xm.reshape(-1))
        init = np.full((rows, ldy), NAN, np.uint16)
        if epi == 1:
            init[:M, :out] = R[:M]
        if cols:
            A = Adaptor(acc, out, cols, 66, 64, seed=0, lda=full.lda)
            A.a[:64], A.b = full.a, full.b
            A.a[M:] = NAN                             # and so must the rows of a
            A.upload(acc)
        for tiles in (1, 2, 4, 8):
            what = f"mc_wb_gemv_{fmt}_bfloat_e{epi}{'_l' if cols else ''} K{K} g{group} M{M} tiles{tiles}"
            got = launch_wide_l(acc, P, xb, M, epi, tiles, init, A, scale) if cols else launch_wide(acc, P, xb, M, epi, tiles, init)
            parity.exact(got[:M, :width], narrow[:M], f"{what}: every row against the narrow kernel")
            assert np.all(got[:M, width:] == NAN), f"{what}: columns past the result written"
            assert np.all(got[M:] == NAN), f"{what}: rows at or past M written"
    P.release()


# ------------------------------------------------------------------------------------------ the head
def launch_head_i8(acc, P, x, M, ldy, rows):
    """mc_vhead_i8_bfloat as test_verify_kernels_gpu.launch_head launches mc_v_head_*: the first M rows of x into a NaN buffer"""
    import metalchat_amd as mc

    yb = acc.to_device(np.full(rows * ldy, NAN, np.uint16))
    wrap = lambda p: acc.wrap(p, 1 << 40) if p else None
    groups = (P.out + VH_ROWS - 1) // VH_ROWS
    mc.KernelTask(acc.load("mc_vhead_i8_bfloat"), (groups * BG_THREADS, 1, 1), (BG_THREADS, 1, 1),
                  [wrap(P.wptr), wrap(P.sptr), acc.to_device(np.ascontiguousarray(x[:M]).reshape(-1)), yb, np.uint32(P.K), np.uint32(P.ng),
                   np.uint32(P.group), np.uint32(M), np.uint32(P.out), np.uint32(ldy)])()
    acc.wait()
    return yb.download(np.uint16, rows * ldy).reshape(rows, ldy)


@pytest.mark.parametrize("K", [1024, 4096])
@pytest.mark.parametrize("group", [0, 32])
def test_v_head_i8_rows_are_the_batch_gemv_rows(acc, K, group):
    out = 2064
    P = QPacked(acc, I8, K, group, out, seed=3 * K + group + 2)
    x = activations128(K, seed=K + group + 5)
    y64, a = P.reference(x)
    gemv = np.concatenate([P.launch(acc, x[r:r + 8]) for r in range(0, 128, 8)])
    check_e0(gemv, y64, a, K, f"mc_b_gemv i8 K{K} g{group}")
    for M in (1, 17, 128):
        what = f"mc_v_head i8 K{K} g{group} M{M}"
        rows = min(M + 2, 130)
        got = launch_head_i8(acc, P, x, M, out + 16, rows)
        parity.exact(got[:M, :out], gemv[:M], f"{what}: every row against mc_b_gemv_i8_bfloat_e0")
        assert np.all(got[:M, out:] == NAN), f"{what}: columns past out written"
        assert np.all(got[M:] == NAN), f"{what}: rows at or past M written"
    P.release()
