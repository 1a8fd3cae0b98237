"""Kernel-level parity of the tiled prompt GEMMs below the ping-pong GEMM (metalchat_amd/csrc/kernels/prefill_kernels.hip), each
launched BY NAME through the Part-1 seam on weights packed by a decoder (mc_decoder_load_linear + mc_decoder_weight_ptrs), against a
float64 product of the dequantised rows:

  * `mc_pf_gemm128_*` (one and two chunks in flight), `mc_pf_gemm256_*_d2` and the 64 x 64 tile `mc_pf_gemm_*` (bfloat and float),
    epilogues e0 (store), e1 (+ residual), e2 (fp32 partial sums of a K range), e3 (silu * mul) and the QLoRA term;
  * `mc_pf2_repack_i4` + `mc_pf2_gemm_i4_bfloat` (int4 g128, <= 64 rows) at several K ranges per launch;
  * `mc_pf_splitk_reduce_bfloat` and `mc_pf_dequant_rows_{i4,i8}_bfloat`.

Reference: Wd = T(T(q) T(s)) by the oracle's hadamard_broadcast, Y64 = X Wd^T in float64.  A bfloat output is within one bf16 step
(at max(|got|, |Y64|)) plus K 2^-23 sum |x||w| of Y64, normwise within 2^-8; a float output within (K + 2) 2^-24 sum |x||w|.  What the
code fixes to the bit is checked to the bit: unit rows (X = e_k returns Wd[n][k] through every family and every K split, the K tail
of a K that is 32 past a multiple of 64 included), e1 against T(res + e0) of the kernel's own e0, the QLoRA term, the reduce in z
order, the families against each other (same MFMA, same k order per output, same operand), and empty K ranges (exact zeros).
Every output buffer is poisoned with NaN and followed by a NaN guard: a tile never written, or a store past the output, shows."""
import numpy as np
import pytest

import modelgen as mg
import parity
from oracle import mc_oracle as mo
from test_batch_kernels_gpu import bf16_rne64, silu_T32, ulp_bf16

pytestmark = pytest.mark.gpu
BF16, F32 = 0, 1
NAN16 = 0x7FC0
GUARD = 1024
PFB_K = 64

# fmt -> (quant, weight format code, group)
FMTS = {"i4g32": ("i4", 2, 32), "i4g128": ("i4", 2, 128), "i4g0": ("i4", 2, 0), "i8g32": ("i8", 1, 32), "w": (None, 0, 0)}
# K = 1024 / 2048 for every format, K = 1056 / 2080 (32 past a multiple of 64) where the loader takes them
KCASES = [(f, K) for K in (1024, 2048) for f in FMTS] + [(f, K) for K in (1056, 2080) for f in ("i8g32", "i4g32", "w")]
MS = [1, 2, 15, 16, 17, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 300, 513]
ROWS = 288                   # 2 tiles of 128 + 32
NS = [288, 256, 192]         # the full matrix, a multiple of 128, 64 past one (rows are addressed independently of N)
ZS = [2, 3, 4, 16]


def f(bits):
    return mo.from_bf16(bits)


def dequant(dt, q, s, group):
    """Wd = T(T(q) T(s)) (hadamard_broadcast, as test_gemm8_gpu.oracle_rows forms it)"""
    L = mo.layout
    out_f, in_f = q.shape
    G = group or in_f
    ng = in_f // G
    wd = np.zeros((out_f, in_f), dtype=mo.np_dtype(dt))
    mo.hadamard_broadcast(dt, F32, L((out_f * ng, G)), wd, L((out_f * ng, G)), np.ascontiguousarray(q), L((out_f * ng,)),
                          np.ascontiguousarray(s.reshape(-1), dtype=np.float32))
    return wd


class Mat:
    """One rows x K matrix in layer 0 of a decoder, packed by it: slot "w2" ([dim][ffn]), "wo" ([dim][H hd]) or "w13" (w1 | w3 fused,
    rows (2j, 2j + 1) = (w1 row j, w3 row j)).  wd64: its dequantised rows as float64."""

    def __init__(self, acc, fmt, K, rows, slot, dt=BF16, seed=0):
        import metalchat_amd as mc

        quant, code, group = FMTS[fmt]
        self.fmt, self.K, self.rows, self.group, self.dt = fmt, K, rows, group, dt
        self.f = {"i4": "i4", "i8": "i8", None: "w"}[quant]
        if slot == "w2":
            cfg = mg.tiny_cfg(dt, dim=rows, ffn_dim=K, n_heads=2, n_kv_heads=1, head_dim=32, n_layers=1, vocab=64, max_seq_len=16)
        elif slot == "wo":
            cfg = mg.tiny_cfg(dt, dim=rows, ffn_dim=256, n_heads=K // 128, n_kv_heads=2, head_dim=128, n_layers=1, vocab=64, max_seq_len=16)
        else:
            cfg = mg.tiny_cfg(dt, dim=K, ffn_dim=rows // 2, n_heads=2, n_kv_heads=1, head_dim=32, n_layers=1, vocab=64, max_seq_len=16)
        self.dec = mc.Decoder(acc, **mg.decoder_kwargs(cfg, weight_format=code, group_size=group))
        rng = np.random.default_rng(seed + 7919 * K + rows + sum(map(ord, fmt + slot)))
        parts = []
        for name in (("w1", "w3") if slot == "w13" else (slot,)):
            out = rows // 2 if slot == "w13" else rows
            if quant is None:
                w = rng.normal(0, 1, (out, K)) * np.exp2(rng.integers(-3, 3, (out, 1))) / np.sqrt(K)
                w = mo.encode(dt, w.astype(np.float32))
                self.dec.load_linear(0, name, code, w)
                parts.append(f(w) if dt == BF16 else w)
                continue
            lo, hi = (-8, 8) if quant == "i4" else (-128, 128)
            q = rng.integers(lo, hi, size=(out, K), dtype=np.int8)
            q[0, :16] = np.arange(-8, 8)
            ng = K // group if group else 1
            # scales of both signs over a few binades, bfloat values (T(s) = s)
            s = rng.choice([-1.0, 1.0], (out, ng)) * np.exp2(rng.uniform(-4, 0, (out, ng))) / (np.sqrt(K) * (hi // 2))
            s = f(mo.to_bf16(s.astype(np.float32)))
            self.dec.load_linear(0, name, code, q, s, group)
            wd = dequant(dt, q, s, group)
            parts.append(f(wd) if dt == BF16 else wd)
        if slot == "w13":
            wd = np.empty((rows, K), np.float32)
            wd[0::2], wd[1::2] = parts
        else:
            wd = parts[0]
        self.wd32 = np.ascontiguousarray(wd, dtype=np.float32)   # every value is exact in float32
        self.wd64 = self.wd32.astype(np.float64)
        self.wptr, self.sptr, r, inf, _ = self.dec.weight_ptrs(0, slot)
        assert (r, inf) == (rows, K)
        self.refs = {}

    def wd_bits(self):
        return mo.to_bf16(self.wd32) if self.dt == BF16 else self.wd32

    def x(self, M, seed=0):
        rng = np.random.default_rng(1000 * M + self.K + seed)
        return mo.encode(self.dt, rng.normal(0, 1, (M, self.K)).astype(np.float32))

    def ref(self, M, N=None):
        """X (device form), Y64 = X Wd[:N]^T and sum |x||w| (N: all rows by default): cached per (M, N)"""
        N = N or self.rows
        if (M, N) not in self.refs:
            X = self.x(M)
            x64 = (f(X) if self.dt == BF16 else X).astype(np.float64)
            self.refs[M, N] = (X, x64 @ self.wd64[:N].T, np.abs(x64) @ np.abs(self.wd64[:N]).T)
        return self.refs[M, N]

    def release(self):
        self.dec.release()


class Mats:
    def __init__(self, acc):
        self.acc, self.made = acc, {}

    def get(self, fmt, K, rows=ROWS, slot=None, dt=BF16):
        slot = slot or ("wo" if K == 1024 else "w2")
        key = (fmt, K, rows, slot, dt)
        if key not in self.made:
            for m in self.made.values():   # (one at a time: the float64 references of a matrix are not small)
                m.release()
            self.made = {key: Mat(self.acc, fmt, K, rows, slot, dt)}
        return self.made[key]

    def close(self):
        for m in self.made.values():
            m.release()


@pytest.fixture(scope="module")
def mats(acc):
    m = Mats(acc)
    yield m
    m.close()


# ------------------------------------------------------------------------------------------ launches
# family -> (kernel name, rows of X per workgroup, rows of W per workgroup, threads)
FAMILIES = {
    "g128": ("mc_pf_gemm128_{f}_bfloat_e{e}", 128, 128, 256),
    "g128d2": ("mc_pf_gemm128_{f}_bfloat_d2_e{e}", 128, 128, 256),
    "g256": ("mc_pf_gemm256_{f}_bfloat_d2_e{e}", 256, 128, 512),
    "g64": ("mc_pf_gemm_{f}_bfloat_e{e}", 64, 64, 256),
    "g64f": ("mc_pf_gemm_{f}_float_e{e}", 64, 64, 256),
}


def wrap(acc, p):
    return acc.wrap(p, 1 << 40) if p else None


def poisoned(acc, n, dtype):
    return acc.to_device(np.full(n + GUARD, NAN16 if dtype == np.uint16 else np.nan, dtype))


def read_guarded(buf, n, dtype, what):
    """the n outputs, after checking that the guard behind them is intact and that every output was written"""
    y = buf.download(dtype, n + GUARD)
    if dtype == np.uint16:
        assert np.all(y[n:] == NAN16), f"{what}: the NaN guard behind the output was written"
        assert not np.any(np.isnan(f(y[:n]))), f"{what}: {int(np.isnan(f(y[:n])).sum())} outputs never written"
    else:
        assert np.all(np.isnan(y[n:])), f"{what}: the NaN guard behind the output was written"
        assert not np.any(np.isnan(y[:n])), f"{what}: {int(np.isnan(y[:n]).sum())} outputs never written"
    return y[:n]


def gemm(acc, fam, mat, xb, M, N, epi, z=1, res=None, lora=None):
    """one launch of a tile GEMM as prefill.cc gemm() forms it; returns [M][N] (e0 / e1: T bits or floats), [z][M][N] fp32 (e2),
    [M][N / 2] (e3)"""
    import metalchat_amd as mc

    tmpl, bm, bn, threads = FAMILIES[fam]
    name = tmpl.format(f=mat.f, e=epi)
    dtype = np.float32 if (epi == 2 or mat.dt == F32) else np.uint16
    n = z * M * N if epi == 2 else (M * N // 2 if epi == 3 else M * N)
    yb = poisoned(acc, n, dtype)
    la = lb = None
    rank, scale = 0, 0.0
    if lora is not None:
        A, B, scale = lora
        la, lb, rank = acc.to_device(A.reshape(-1)), acc.to_device(B.reshape(-1)), A.shape[1]
    mc.KernelTask(acc.load(name), ((N + bn - 1) // bn * threads, (M + bm - 1) // bm, z), (threads, 1, 1),
                  [wrap(acc, mat.wptr), wrap(acc, mat.sptr), xb, yb, res, np.uint32(M), np.uint32(N), np.uint32(mat.K),
                   np.uint32(mat.group), la, lb, np.uint32(rank), np.float32(scale)])()
    acc.wait()
    y = read_guarded(yb, n, dtype, f"{name} M {M} N {N} z {z}")
    return y.reshape(z, M, N) if epi == 2 else y.reshape(M, -1)


def kranges(K, z):
    """pf_gemm_big_body's K ranges: ceil(K / 64) chunks over z workgroups"""
    kper = ((K + PFB_K - 1) // PFB_K + z - 1) // z * PFB_K
    return [(min(K, i * kper), min(K, (i + 1) * kper)) for i in range(z)]


# ------------------------------------------------------------------------------------------ bounds
def check_bf16(got, y64, a, K, what):
    g = f(got).astype(np.float64)
    err = np.abs(g - y64)
    bound = ulp_bf16(np.maximum(np.abs(g), np.abs(y64))) + K * 2.0 ** -23 * a
    worst = np.unravel_index(np.argmax(err - bound), err.shape)
    assert np.all(err <= bound), f"{what}: |got - y64| {err[worst]:.4g} > bound {bound[worst]:.4g} at {worst}"
    nrm = np.linalg.norm(g - y64) / max(np.linalg.norm(y64), 1e-300)
    assert nrm <= 2.0 ** -8, f"{what}: normwise relative error {nrm:.3g} > 2^-8"


def check_f32(got, y64, a, K, what):
    err = np.abs(got.astype(np.float64) - y64)
    bound = (K + 2) * 2.0 ** -24 * a
    worst = np.unravel_index(np.argmax(err - bound), err.shape)
    assert np.all(err <= bound), f"{what}: |got - y64| {err[worst]:.4g} > bound {bound[worst]:.4g} at {worst}"


def sum_z(part):
    """fp32 sum over z, in z order (mc_pf_splitk_reduce_bfloat)"""
    t = np.zeros(part.shape[1:], np.float32)
    for p in part:
        t = t + p
    return t


def plus_res(res, e0):
    """e1 = T(f32(res) + f32(e0)): one rounding of the float sum"""
    return mo.to_bf16(f(res) + f(e0))


# ------------------------------------------------------------------------------------------ store, residual, K ranges
@pytest.mark.parametrize("fmt,K", KCASES)
def test_tiles_match_float64_and_each_other(acc, mats, fmt, K):
    """every M edge of the 64 / 128 / 256-row tiles; N the full row count, 256 and 192 in turn; e2 at 2, 3, 4 and 16 ranges in turn"""
    mat = mats.get(fmt, K)
    rng = np.random.default_rng(K)
    for i, M in enumerate(MS):
        N, z = NS[i % len(NS)], ZS[i % len(ZS)]
        X, y64, a = mat.ref(M)
        y64, a = y64[:, :N], a[:, :N]
        xb = acc.to_device(X.reshape(-1))
        what = f"{fmt} K {K} M {M} N {N}"
        e0 = gemm(acc, "g128d2", mat, xb, M, N, 0)
        check_bf16(e0, y64, a, K, f"{what} gemm128_d2 e0")
        # the same MFMA over the same k order per output on the same dequantised operand: the same bits
        parity.exact(gemm(acc, "g128", mat, xb, M, N, 0), e0, f"{what}: gemm128 (one chunk in flight) against _d2")
        parity.exact(gemm(acc, "g256", mat, xb, M, N, 0), e0, f"{what}: gemm256 against gemm128")
        parity.exact(gemm(acc, "g64", mat, xb, M, N, 0), e0, f"{what}: the 64 x 64 tile against gemm128")
        # e1: T(res + e0), the kernel's own e0
        res = mo.to_bf16((rng.normal(0, 1, (M, N)) * np.abs(f(e0)).mean()).astype(np.float32))
        rb = acc.to_device(res.reshape(-1))
        want = plus_res(res, e0)
        for fam in ("g128d2", "g128", "g256", "g64"):
            parity.exact(gemm(acc, fam, mat, xb, M, N, 1, res=rb), want, f"{what}: {fam} e1 = T(res + e0)")
        # e2: the partial of every K range against its own float64 product; ranges past K store zeros
        x64 = f(X).astype(np.float64)
        for fam in ("g128d2", "g256"):
            part = gemm(acc, fam, mat, xb, M, N, 2, z=z)
            for j, (k0, k1) in enumerate(kranges(K, z)):
                if k0 == k1:
                    parity.exact(part[j], np.zeros((M, N), np.float32), f"{what}: {fam} e2 x{z}: range {j} starts past K")
                    continue
                yz = x64[:, k0:k1] @ mat.wd64[:N, k0:k1].T
                az = np.abs(x64[:, k0:k1]) @ np.abs(mat.wd64[:N, k0:k1]).T
                err = np.abs(part[j] - yz)
                assert np.all(err <= (k1 - k0) * 2.0 ** -23 * az), f"{what}: {fam} e2 x{z} range {j} [{k0}, {k1}) off by {err.max():.3g}"
            check_bf16(mo.to_bf16(sum_z(part)), y64, a, K, f"{what}: {fam} e2 x{z}, summed in z order")


@pytest.mark.parametrize("fmt,K", KCASES)
def test_one_hot_rows_return_every_dequantised_weight(acc, mats, fmt, K):
    """X = e_k (M = K rows): Y[k][n] = Wd[n][k] to the bit through every family and every K split -- the columns of the last 64-chunk
    that a K 32 past a multiple of 64 half fills included; and the dequantised copy is Wd to the bit"""
    import metalchat_amd as mc

    mat = mats.get(fmt, K)
    N = ROWS
    X = mo.to_bf16(np.eye(K, dtype=np.float32))
    xb = acc.to_device(X.reshape(-1))
    # (q = 0 under a negative scale dequantises to -0; the sum +0 + (-0) of the products is +0)
    want = mo.to_bf16(np.ascontiguousarray(mat.wd32[:N].T) + np.float32(0.0))
    for fam in ("g128d2", "g128", "g256", "g64"):
        parity.exact(gemm(acc, fam, mat, xb, K, N, 0), want, f"{fmt} K {K}: one-hot rows through {fam} e0")
    for fam, zs in (("g128d2", (2, 3, 16)), ("g256", (2, 4, 16)), ("g128", (3,))):
        for z in zs:
            part = gemm(acc, fam, mat, xb, K, N, 2, z=z)
            parity.exact(mo.to_bf16(sum_z(part)), want, f"{fmt} K {K}: one-hot rows through {fam} e2 x{z}, summed over z")
    if mat.f != "w":
        name = f"mc_pf_dequant_rows_{mat.f}_bfloat"
        ob = poisoned(acc, ROWS * K, np.uint16)
        mc.KernelTask(acc.load(name), ((K // 16 + 255) // 256 * 256, ROWS, 1), (256, 1, 1),
                      [wrap(acc, mat.wptr), wrap(acc, mat.sptr), ob, np.uint32(ROWS), np.uint32(K), np.uint32(mat.group)])()
        acc.wait()
        parity.exact(read_guarded(ob, ROWS * K, np.uint16, name).reshape(ROWS, K), mat.wd_bits(), f"{fmt} K {K}: {name}")


# ------------------------------------------------------------------------------------------ the XCD tile order
# (nx ny) % 8 != 0 is every case above (nx = 3 at N = 288); here ny in {1, 2, 4} with nx % (8 / ny) == 0, and ny % 8 == 0
GRIDS = [("g128d2", 128, 1024), ("g128d2", 256, 512), ("g128d2", 512, 256), ("g256", 512, 512), ("g256", 1024, 256),
         ("g128d2", 1024, 128), ("g256", 2048, 128), ("g128", 1024, 128)]


@pytest.mark.parametrize("fmt", ["i4g128", "i8g32", "w"])
def test_xcd_tile_order_writes_every_tile_once(acc, mats, fmt):
    mat = mats.get(fmt, 1024, rows=1024, slot="w13")
    rng = np.random.default_rng(5)
    for fam, M, N in GRIDS:
        bm = FAMILIES[fam][1]
        nx, ny = N // 128, (M + bm - 1) // bm
        assert (nx * ny) % 8 == 0 and (ny % 8 == 0 or (8 % ny == 0 and nx % (8 // ny) == 0))
        X, y64, a = mat.ref(M, N)
        xb = acc.to_device(X.reshape(-1))
        what = f"{fmt} {fam} M {M} N {N} (grid {nx} x {ny})"
        e0 = gemm(acc, fam, mat, xb, M, N, 0)
        check_bf16(e0, y64[:, :N], a[:, :N], 1024, what)
        res = mo.to_bf16(rng.normal(0, 0.1, (M, N)).astype(np.float32))
        parity.exact(gemm(acc, fam, mat, xb, M, N, 1, res=acc.to_device(res.reshape(-1))), plus_res(res, e0), f"{what} e1")
        part = gemm(acc, fam, mat, xb, M, N, 2, z=2)
        check_bf16(mo.to_bf16(sum_z(part)), y64[:, :N], a[:, :N], 1024, f"{what} e2 x2")


# ------------------------------------------------------------------------------------------ the activation epilogue
def silu64(v):
    return v / (1.0 + np.exp(-v))


@pytest.mark.parametrize("fmt", list(FMTS))
def test_activation_epilogue_matches_float64(acc, mats, fmt):
    """mc_pf_gemm256_*_d2_e3 on w1 | w3: out[m][j] = T(silu_T(T(w1 x)) * T(w3 x)) -- within two steps of float64 silu(T(w1 x)) T(w3 x),
    and (at most 3 % of the outputs differing at all) the same composition with the roundings of silu_T on T(float64) operands"""
    import metalchat_amd as mc

    mat = mats.get(fmt, 1024, rows=576, slot="w13")
    etab = acc.alloc(65536 * 4)
    mc.KernelTask(acc.load("mc_exp_table_bfloat"), (256 * 256, 1, 1), (256, 1, 1), [etab])()
    acc.wait()
    for M in (17, 256, 300, 513):
        X, y64, _ = mat.ref(M)
        xb = acc.to_device(X.reshape(-1))
        got = gemm(acc, "g256", mat, xb, M, mat.rows, 3, res=etab)
        g1, g3 = f(bf16_rne64(y64[:, 0::2])).astype(np.float64), f(bf16_rne64(y64[:, 1::2])).astype(np.float64)
        ref = bf16_rne64(silu64(g1) * g3)
        parity.check(BF16, got.reshape(-1), ref.reshape(-1), rel=2.0 ** -7, max_ulp=2, max_frac=1.0, scale_aware=True,
                     what=f"{fmt} w1|w3 e3 M {M} against float64")
        comp = mo.to_bf16(silu_T32(g1.astype(np.float32)) * g3.astype(np.float32))
        parity.check(BF16, got.reshape(-1), comp.reshape(-1), rel=2e-3, max_ulp=2, max_frac=0.03, scale_aware=True,
                     what=f"{fmt} w1|w3 e3 M {M} against silu_T")


# ------------------------------------------------------------------------------------------ the QLoRA term
def lora_inputs(M, N, rank, seed):
    rng = np.random.default_rng(seed)
    A = mo.to_bf16(rng.normal(0, 1, (M, rank)).astype(np.float32))
    B = mo.to_bf16(rng.normal(0, 0.05, (N, rank)).astype(np.float32))
    return A, B


def lora_term(base, A, B, rank, scale):
    """pf_lora: T(base + T(T(p) T(scale))), p = sum over i = 0 .. rank - 1 of a_i b_i in fp32, in that order (each product exact)"""
    af, bf_ = f(A), f(B)
    p = np.zeros((A.shape[0], B.shape[0]), np.float32)
    for i in range(rank):
        p = p + af[:, i:i + 1] * bf_[:, i][None, :]
    ts = f(mo.to_bf16(np.array([scale], np.float32)))[0]
    t = f(mo.to_bf16(f(mo.to_bf16(p)) * ts))
    return mo.to_bf16(f(base) + t)


@pytest.mark.parametrize("rank", [8, 16])
@pytest.mark.parametrize("fmt", ["i4g32", "i8g32", "w"])
def test_lora_epilogue_is_the_reference_composition(acc, mats, fmt, rank):
    mat = mats.get(fmt, 1056)
    rng = np.random.default_rng(rank)
    for M, N in ((17, 288), (129, 192), (300, 256)):
        X, _, _ = mat.ref(M)
        xb = acc.to_device(X.reshape(-1))
        A, B = lora_inputs(M, N, rank, M + rank)
        scale = 0.7
        for fam in ("g128d2", "g256", "g64"):
            base = gemm(acc, fam, mat, xb, M, N, 0)
            want = lora_term(base, A, B, rank, scale)
            got = gemm(acc, fam, mat, xb, M, N, 0, lora=(A, B, scale))
            parity.exact(got, want, f"{fmt} {fam} M {M} rank {rank}: e0 with the adaptor")
            assert np.mean(got != base) > 0.3, "the adaptor term moved too few outputs to test anything"
            res = mo.to_bf16(rng.normal(0, 0.1, (M, N)).astype(np.float32))
            got1 = gemm(acc, fam, mat, xb, M, N, 1, res=acc.to_device(res.reshape(-1)), lora=(A, B, scale))
            parity.exact(got1, plus_res(res, want), f"{fmt} {fam} M {M} rank {rank}: e1 with the adaptor")


# ------------------------------------------------------------------------------------------ the split-K reduce
@pytest.mark.parametrize("splits", [1, 2, 3, 16])
def test_splitk_reduce_adds_in_z_order_then_adaptor_then_residual(acc, splits):
    import metalchat_amd as mc

    M, N, rank, scale = 37, 300, 16, 1.3
    rng = np.random.default_rng(splits)
    # partials of mixed magnitudes and signs; in every other column the first two are +-B, B ~ 2^16 times the rest, so that the order
    # of the additions moves the ROUNDED sum
    part = (rng.normal(0, 1, (splits, M, N)) * np.exp2(rng.integers(-12, 12, (splits, M, N)))).astype(np.float32)
    if splits > 2:   # (two partials: a + b = b + a)
        part[2:, :, 0::2] = rng.normal(0, 1, (splits - 2, M, (N + 1) // 2))
        part[0, :, 0::2] = rng.normal(0, 1, (M, (N + 1) // 2)) * 2.0 ** 16
        part[1, :, 0::2] = -part[0, :, 0::2]
        rev = np.zeros((M, N), np.float32)
        for p in part[::-1]:
            rev = rev + p
        assert np.mean(mo.to_bf16(rev) != mo.to_bf16(sum_z(part))) > 0.05, "partials whose rounded sum does not depend on the order"
    base = mo.to_bf16(sum_z(part))
    res = mo.to_bf16(rng.normal(0, 100, (M, N)).astype(np.float32))
    A, B = lora_inputs(M, N, rank, 3)
    pb = acc.to_device(part.reshape(-1))
    for with_res in (False, True):
        for with_lora in (False, True):
            yb = poisoned(acc, M * N, np.uint16)
            la, lb = (acc.to_device(A.reshape(-1)), acc.to_device(B.reshape(-1))) if with_lora else (None, None)
            mc.KernelTask(acc.load("mc_pf_splitk_reduce_bfloat"), ((N + 255) // 256 * 256, M, 1), (256, 1, 1),
                          [pb, yb, acc.to_device(res.reshape(-1)) if with_res else None, np.uint32(M), np.uint32(N), np.uint32(splits),
                           la, lb, np.uint32(rank if with_lora else 0), np.float32(scale)])()
            acc.wait()
            got = read_guarded(yb, M * N, np.uint16, "mc_pf_splitk_reduce_bfloat").reshape(M, N)
            want = lora_term(base, A, B, rank, scale) if with_lora else base
            if with_res:
                want = plus_res(res, want)
            parity.exact(got, want, f"reduce x{splits} (residual {with_res}, adaptor {with_lora})")


# ------------------------------------------------------------------------------------------ the weight-streaming GEMM (pf2)
def pf2_launch(acc, mat, wq2, xb, M, N, ktper):
    import metalchat_amd as mc

    KT = mat.K // 128
    z = (KT + ktper - 1) // ktper
    n = z * M * N
    pb = poisoned(acc, n, np.float32)
    mc.KernelTask(acc.load("mc_pf2_gemm_i4_bfloat"), ((N + 127) // 128 * 512, 1, z), (512, 1, 1),
                  [wq2, wrap(acc, mat.sptr), xb, pb, np.uint32(M), np.uint32(N), np.uint32(mat.K), np.uint32(ktper)])()
    acc.wait()
    return read_guarded(pb, n, np.float32, f"pf2 M {M} N {N} ktper {ktper}").reshape(z, M, N)


def pf2_repack(acc, mat, N):
    import metalchat_amd as mc

    wq2 = acc.alloc((N + 15) // 16 * (mat.K // 128) * 1024)
    mc.KernelTask(acc.load("mc_pf2_repack_i4"), (2048 * 256, 1, 1), (256, 1, 1),
                  [wrap(acc, mat.wptr), wq2, np.uint32(N), np.uint32(mat.K)])()
    acc.wait()
    return wq2


@pytest.mark.parametrize("K", [256, 1024, 2048])
def test_weight_streaming_gemm_matches_float64(acc, mats, K):
    """int4 g128 prompts of <= 64 rows: MT = 1 / 2 / 4 row tiles, K ranges of 2, 3, 5 and all K steps (a short last range: the steps
    past it add zero-scaled weights), N a multiple of 16 and not (the waves past the last 16-row tile store nothing)"""
    mat = mats.get("i4g128", K)
    KT = K // 128
    for N in (ROWS, 200):
        wq2 = pf2_repack(acc, mat, N)
        for i, M in enumerate((1, 16, 17, 32, 33, 64)):
            X, y64, a = mat.ref(M)
            y64, a = y64[:, :N], a[:, :N]
            xb = acc.to_device(X.reshape(-1))
            x64 = f(X).astype(np.float64)
            for ktper in sorted({2, 3, 5, KT}):
                if ktper > KT:
                    continue
                part = pf2_launch(acc, mat, wq2, xb, M, N, ktper)
                what = f"pf2 K {K} N {N} M {M} ktper {ktper}"
                for j in range(part.shape[0]):
                    k0, k1 = 128 * j * ktper, min(K, 128 * (j + 1) * ktper)
                    yz = x64[:, k0:k1] @ mat.wd64[:N, k0:k1].T
                    az = np.abs(x64[:, k0:k1]) @ np.abs(mat.wd64[:N, k0:k1]).T
                    err = np.abs(part[j] - yz)
                    assert np.all(err <= (k1 - k0) * 2.0 ** -23 * az), f"{what}: range {j} [{k0}, {k1}) off by {err.max():.3g}"
                check_bf16(mo.to_bf16(sum_z(part)), y64, a, K, f"{what}, summed in z order")
    # one-hot rows, 64 at a time: every weight of every K range comes back to the bit
    N = 200
    wq2 = pf2_repack(acc, mat, N)
    want = mo.to_bf16(mat.wd32[:N] + np.float32(0.0))   # (-0 weights come back as +0: see the one-hot test above)
    for ktper in (3, KT):
        got = np.zeros((K, N), np.uint16)
        for k0 in range(0, K, 64):
            X = np.zeros((64, K), np.float32)
            X[np.arange(64), k0 + np.arange(64)] = 1.0
            part = pf2_launch(acc, mat, wq2, acc.to_device(mo.to_bf16(X).reshape(-1)), 64, N, ktper)
            got[k0:k0 + 64] = mo.to_bf16(sum_z(part))
        parity.exact(got.T, want, f"pf2 K {K} ktper {ktper}: one-hot rows summed over the K ranges")


# ------------------------------------------------------------------------------------------ T = float: the 64 x 64 tile
@pytest.mark.parametrize("fmt", ["i4g32", "i8g32", "w"])
@pytest.mark.parametrize("K", [1024, 1056])
def test_float_tile_matches_float64(acc, mats, fmt, K):
    mat = mats.get(fmt, K, slot="w2", dt=F32)
    rng = np.random.default_rng(K + 1)
    for i, M in enumerate((1, 17, 64, 65, 129)):
        N = NS[i % len(NS)]
        X, y64, a = mat.ref(M)
        xb = acc.to_device(X.reshape(-1))
        e0 = gemm(acc, "g64f", mat, xb, M, N, 0)
        check_f32(e0, y64[:, :N], a[:, :N], K, f"{fmt} K {K} M {M} N {N} float e0")
        res = rng.normal(0, 1, (M, N)).astype(np.float32)
        parity.exact(gemm(acc, "g64f", mat, xb, M, N, 1, res=acc.to_device(res.reshape(-1))), res + e0, f"{fmt} K {K} M {M} float e1")
    X = np.eye(K, dtype=np.float32)
    parity.exact(gemm(acc, "g64f", mat, acc.to_device(X.reshape(-1)), K, ROWS, 0), np.ascontiguousarray(mat.wd32.T),
                 f"{fmt} K {K}: one-hot rows through the float tile")
