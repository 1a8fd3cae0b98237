"""The references of pf_rows_ref.py against the oracle's own kernels, at the shapes and with the caps of test_pf_row_kernels_gpu.py: a cap
the reference alone does not meet is a wrong cap or a wrong reference, and shows here, without a GPU.  Prints the measured shares."""
import numpy as np
import pytest

import parity
import pf_rows_ref as ref
from oracle import mc_oracle as mo
from test_batch_kernels_gpu import bf, bf16_rne64, f, silu_T32, steps

BF16, F32 = 0, 1
BF_DIMS, F_DIMS = [256, 2048, 2056, 8192, 8200, 1004], [256, 4096, 4100, 1002]


@pytest.fixture(scope="module", autouse=True)
def _oracle(oracle):
    return oracle


def test_embedding_references():
    """the int8 chain against the oracle's dequantising product (hadamard_broadcast) and scalar_mul; the plain table is the oracle"""
    rng = np.random.default_rng(1)
    tokens = [0, 49, 7, 7, 49]
    for dt in (BF16, F32):
        for dim in (256, 1000):
            q = rng.integers(-128, 128, (50, dim), dtype=np.int8)
            s = rng.uniform(1e-3, 3e-2, 50).astype(np.float32)
            sc = ref.embed_scale(dt, dim)
            plain = ref.values(dt, ref.embed_q8(dt, q, s, tokens))
            want = ref.rt(dt, q[tokens].astype(np.float64) * ref.rt(dt, s[tokens]).astype(np.float64)[:, None])
            parity.exact(plain, want, f"int8 rows dt {dt} dim {dim}: the float32 product rounds as the exact product does")
            got = ref.embed_q8(dt, q, s, tokens, sc)
            table = ref.storage(dt, plain)
            full = np.zeros((50, dim), table.dtype)
            full[tokens] = table
            parity.exact(got, ref.embed(dt, full, tokens, sc), f"int8 rows dt {dt} dim {dim}: the scale step is mo.scalar_mul")
            assert sc == ref.rt(dt, np.array([np.sqrt(dim)], np.float32))[0]


@pytest.mark.parametrize("dim", BF_DIMS)
def test_rmsnorm_float64_against_the_oracle_bfloat(dim):
    for mu in (0.0, 1.0):
        x, res, w = ref.norm_inputs(BF16, 3, dim, mu, seed=2)
        v64 = ref.rmsnorm64(f(x), f(w), 1e-5, mu)
        o = ref.oracle_rmsnorm(BF16, x, w, 1e-5, mu)
        d = steps(o, bf16_rne64(v64))
        print(f"rmsnorm bfloat dim {dim} mu {mu}: oracle against T(float64): at most {int(d.max())} steps, {float(np.mean(d != 0)):.5f} differ")
        assert d.max() <= 1
        # with the residual: T(res + oracle's row) inside the span of the neighbours (or one step outside)
        lo, hi = ref.residual_span(res, v64)
        out = ref.outside(bf(f(res) + f(o)), lo, hi)
        print(f"  with the residual: at most {int(out.max())} steps outside the span, {float(np.mean(out != 0)):.5f} outside")
        assert out.max() <= 1


@pytest.mark.parametrize("dim", F_DIMS)
def test_rmsnorm_float64_against_the_oracle_float(dim):
    for mu in (0.0, 1.0):
        x, res, w = ref.norm_inputs(F32, 3, dim, mu, seed=2)
        v64 = ref.rmsnorm64(x, w, 1e-5, mu)
        st = parity.check(F32, ref.oracle_rmsnorm(F32, x, w, 1e-5, mu), v64, rel=2e-5, what=f"rmsnorm float dim {dim} mu {mu}")
        print(f"rmsnorm float dim {dim} mu {mu}: oracle against float64 {st}")


def test_silu_T32_against_the_oracle_over_every_bfloat16():
    a = ref.all_bf16()
    ok = ~ref.is_nan16(a)
    rng = np.random.default_rng(3)
    for name, b in (("b = 1", np.full(65536, 0x3F80, np.uint16)), ("b random", bf(rng.normal(0, 2, 65536)))):
        with np.errstate(invalid="ignore", over="ignore"):
            mine = bf(silu_T32(f(a)) * f(b))
        theirs = ref.oracle_silu_mul(BF16, a.reshape(1, -1), b.reshape(1, -1))[0]
        both = ok & ~ref.is_nan16(mine) & ~ref.is_nan16(theirs)
        assert np.array_equal(ref.is_nan16(mine)[ok], ref.is_nan16(theirs)[ok]), name
        d = steps(mine[both], theirs[both])
        print(f"silu_T32 against mo.silu + mo.hadamard, {name}: at most {int(d.max())} steps, share {float(np.mean(d != 0)):.5f} of {int(both.sum())}")
        assert d.max() <= 1 and np.mean(d != 0) <= 0.01


def test_float_activations_against_the_oracle():
    rng = np.random.default_rng(4)
    for ffn in (1000, 1001):
        a, b = (rng.normal(0, 2, (3, ffn)).astype(np.float32) for _ in range(2))
        st = parity.check(F32, ref.oracle_silu_mul(F32, a, b), ref.silu64(a) * b.astype(np.float64), rel=2e-5, what=f"silu float ffn {ffn}")
        g = np.zeros_like(a)
        mo.gelu(F32, mo.layout(a.shape), g, mo.layout(a.shape), a)
        st2 = parity.check(F32, g, ref.gelu64(a), rel=2e-5, what=f"gelu float ffn {ffn}")
        print(f"float activations ffn {ffn}: silu {st}, gelu {st2}")


@pytest.mark.parametrize("H,KV,hd", ref.ROPE_SHAPES)
def test_rope_reference_without_norms_is_the_oracle_per_row(H, KV, hd):
    """RopeRef.expect: exactly the call's slots change, and a row's q is mo.rope of its un-partnered heads at table row rope_row0 + r"""
    for dt in ((BF16, F32) if hd <= 64 else (BF16,)):
        rr = ref.rope_ref(dt, H, KV, hd)
        assert rr.M % 16 != 0 and ((H + KV) * rr.M) % (2048 // hd) != 0
        x, kc0, vt0 = rr.inputs(seed=5)
        q, kc, vt = rr.expect(x, kc0, vt0)
        slots = np.arange(rr.start_pos, rr.start_pos + rr.M)
        keep = np.ones(rr.max_seq, bool)
        keep[slots] = False
        assert slots[-1] == rr.max_seq - 1
        parity.exact(kc[:, keep], kc0[:, keep], "K slots outside the call")
        parity.exact(vt[:, :, keep], vt0[:, :, keep], "V slots outside the call")
        parity.exact(vt[:, :, slots].transpose(2, 0, 1).reshape(rr.M, -1), x[:, rr.nb:], "V columns are the v heads")
        # a q row is the rotation of its un-partnered heads by the table row rope_row0 + r, in float64 within a rounding to T
        r = rr.M - 1
        qn = ref.values(dt, rr.split_row(x[r])[0]).astype(np.float64)
        c, s = rr.rc[rr.rope_row0 + r].astype(np.float64), rr.rs[rr.rope_row0 + r].astype(np.float64)
        half = hd // 2
        want = np.concatenate([c * qn[:, :half] - s * qn[:, half:], s * qn[:, :half] + c * qn[:, half:]], axis=1)
        err = np.abs(ref.values(dt, q[r]).astype(np.float64) - want)
        assert np.all(err <= (2.0 ** -8 if dt == BF16 else 2.0 ** -22) * (np.abs(want) + np.abs(qn).max())), f"dt {dt} hd {hd}: the last row's rotation"


@pytest.mark.parametrize("H,KV,hd", ref.ROPE_SHAPES)
def test_norm_then_rope_reference_against_the_oracle(H, KV, hd):
    """mo.rmsnorm + mo.rope of every head against the span method: exact where the normed value has one rounding, within a step of
    the corners' span elsewhere; the ambiguous share under 1e-2 for the seeds the GPU tests use (expected near 2 * 2^-20 / 2^-8)"""
    rr = ref.rope_ref(BF16, H, KV, hd)
    x, kc0, vt0, qw, kw = rr.inputs(seed=ref.NORM_SEED, norms=True)
    for q_w, k_w, name in ((qw, kw, "q and k"), (qw, None, "q only"), (None, kw, "k only")):
        lo, hi, amb = rr.norm_span(x, q_w, k_w, ref.NORM_EPS, ref.NORM_MU)
        on = rr.normed64(x, q_w, k_w, ref.NORM_EPS, ref.NORM_MU)[1]
        share = float(amb.sum() / on.sum())
        print(f"H {H} KV {KV} hd {hd} {name}: {int(amb.sum())} of {int(on.sum())} normed values have two roundings (share {share:.5f}; "
              f"expected near {2 * 2.0 ** -20 / 2.0 ** -8:.5f})")
        assert share < 1e-2
        # the oracle's composition on the fused rows: norm every head in its natural order, re-partner, rope
        xo = x.copy()
        for w, first, heads in ((q_w, 0, H), (k_w, H, KV)):
            if w is None:
                continue
            nat = np.stack([ref.unpartner(x[r, first * hd:(first + heads) * hd].reshape(heads, hd)) for r in range(rr.M)]).reshape(-1, hd)
            nn = ref.oracle_rmsnorm(BF16, nat, w, ref.NORM_EPS, ref.NORM_MU).reshape(rr.M, heads, hd)
            xo[:, first * hd:(first + heads) * hd] = np.stack([ref.packed_partners(nn[r]) for r in range(rr.M)]).reshape(rr.M, -1)
        got = rr.expect(xo, kc0, vt0)
        for g, (omin, omax), what in zip(got, rr.corners(lo, hi, kc0, vt0), ("q rows", "K", "V")):
            d = ref.outside(g, omin, omax)
            print(f"  {what}: at most {int(d.max())} steps outside the span, {float(np.mean(d != 0)):.5f} outside, {float(np.mean(omin != omax)):.5f} have a span")
            assert d.max() <= 1
            assert np.all(d[omin == omax] == 0), f"{what}: a value with one correct rounding differs from the oracle"


def test_probability_sum_bound_holds_for_the_oracles_softmax():
    rng = np.random.default_rng(6)
    for dt in (BF16, F32):
        for S in (5, 17, 37, 48):
            s = ref.storage(dt, rng.normal(0, 2, (8, S)))
            p = np.zeros_like(s)
            mo.softmax(dt, mo.layout(s.shape), p, mo.layout(s.shape), s)
            err = np.abs(ref.values(dt, p).astype(np.float64).sum(axis=1) - 1.0)
            print(f"softmax dt {dt} S {S}: |sum - 1| at most {err.max():.3g}, bound {ref.prob_sum_bound(dt, S):.3g}")
            assert np.all(err <= ref.prob_sum_bound(dt, S))
