"""Kernel-level tests of the ROW kernels of the one-prompt pass (kernels/prefill_kernels.hip), the kernels that sit between the GEMMs and
the attention in prefill.cc mc_decoder::run_prefill: every one launched BY NAME through the Part-1 seam on buffers the test owns, with
the grid, block and argument order of its launch site, against the references of pf_rows_ref.py (the oracle's kernel where the operation
is one, float64 / float32 numpy with the roundings to T written out where it is not; test_pf_rows_ref_cpu.py holds them to the oracle):

  A  mc_pf_embed_{bfloat,float}, mc_pf_embed_q8_{bfloat,float}: exact, a partial last workgroup, gemma's scale;
  B  mc_pf_rmsnorm_{bfloat,float} on both sides of every edge of the packet path (idle lanes, one round, one packet into the second
     round, the last size, the scalar path by size and by alignment), with and without the residual, mu 0 and 1, every row alone bit for
     bit its row of the launch; mc_pf_rmsnorm_parts_bfloat and mc_pf_rmsnorm2_parts_bfloat bit for bit the launches they fold;
  C  mc_pf_act_mul_bfloat over every bfloat16 value, mc_pf_act_mul_{bfloat,float} at a size with a scalar tail,
     mc_pf_act_mul_parts_bfloat bit for bit mc_pf_splitk_reduce_bfloat + mc_pf_act_mul_bfloat;
  D  mc_pf_rope_cache_{bfloat,float}, _v4_bfloat, _parts_bfloat, _parts_v4_bfloat at head_dim 32 .. 256 with both tails of the four-pair
     grid, the chunk's last row in the cache's last slot, with and without q / k norms (the 16- and 32-thread workgroups of the one-pair
     launch at head_dim 32 / 64; the butterfly of the four-pair launch at 128 / 256);
  E  mc_pf_scores_T + mc_pf_pv_T, the attention of a float decoder and of MC_PF_TWO_PASS: the probabilities' zeros and sums, every row
     against the oracle over exactly its visible keys.

Every output buffer is longer than what the kernel may write and starts as a pattern of NaNs (bfloat16) or NaN (float), and every test
holds the excess to the initial bits: rows past M, cache slots other than the call's, the guard behind a cache."""
import sys

import numpy as np
import pytest

import parity
import pf_attn_rule as pr
import pf_rows_ref as ref
from test_attn_kernels_gpu import oracle_attention
from test_batch_kernels_gpu import GUARD, NAN, bf, bf16_rne64, f, guarded, rope_table, silu_T32, steps
from test_pf_gemm_gpu import poisoned, read_guarded
from test_rows_kernels_gpu import etab, pattern, scale_of  # noqa: F401  (etab: a fixture)

pytestmark = pytest.mark.gpu
BF16, F32 = 0, 1
TN = {BF16: "bfloat", F32: "float"}
u32, i32, f32 = np.uint32, np.int32, np.float32
EXCESS = 64               # elements behind every row buffer
LAUNCHED = set()          # the names this module has launched (test_every_row_kernel_of_the_table_was_launched)


# ------------------------------------------------------------------------------------------ helpers
def launch(acc, name, blocks, threads, args):
    """one launch as prefill.cc launch(name, gx, gy, 1, block, 0, args): `blocks` = (gx, gy) workgroups of `threads` threads"""
    import metalchat_amd as mc

    LAUNCHED.add(name)
    mc.KernelTask(acc.load(name), (blocks[0] * threads, blocks[1], 1), (threads, 1, 1), args)()


def bits(a):
    """the storage as unsigned words: NaNs compare by their bits"""
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def fresh(dt, n):
    """n elements no kernel has written: the pattern of NaNs (bfloat16), NaN (float)"""
    return pattern(n) if dt == BF16 else np.full(n, np.nan, np.float32)


def same(got, want, what):
    parity.exact(bits(got), bits(want), what)


class Out:
    """an output buffer of n elements and EXCESS more; take() returns the n and holds the excess to its initial bits"""

    def __init__(self, acc, dt, n, excess=EXCESS):
        self.dt, self.n, self.host = dt, n, fresh(dt, n + excess)
        self.buf = acc.to_device(self.host)

    def take(self, what, shape=None):
        y = self.buf.download(ref.mo.np_dtype(self.dt), self.host.size)
        same(y[self.n:], self.host[self.n:], f"{what}: the elements behind the output")
        return y[:self.n].reshape(shape or (self.n,))

    def untouched(self, what):
        same(self.buf.download(ref.mo.np_dtype(self.dt), self.host.size), self.host, f"{what}: a buffer the launch must not write")


def with_guard(dt, a):
    """a cache followed by GUARD NaNs"""
    if dt == BF16:
        return guarded([a], 1)
    return np.concatenate([a.reshape(-1), np.full(GUARD, np.nan, np.float32)])


def reduce_rows(acc, partb, splits, M, N, res=None):
    """mc_pf_splitk_reduce_bfloat as prefill.cc gemm_run launches it behind a split GEMM: grid ((N + 255) / 256, M), 256 threads;
    arguments part, Y, res, M, N, splits, la, lb, lora_rank, lora_scale"""
    yb = poisoned(acc, M * N, np.uint16)
    resb = acc.to_device(res.reshape(-1)) if res is not None else None
    launch(acc, "mc_pf_splitk_reduce_bfloat", ((N + 255) // 256, M), 256, [partb, yb, resb, u32(M), u32(N), u32(splits), None, None, u32(0), f32(0.0)])
    acc.wait()
    return read_guarded(yb, M * N, np.uint16, f"split-K reduce M {M} N {N} splits {splits}").reshape(M, N)


def parts_buffer(rng, splits, M, N, tail="finite"):
    """fp32 partial sums [splits][M][N], generic N(0, 1), and one more split's worth behind them that no sum may take in"""
    p = rng.normal(0, 1, (splits + 1, M, N)).astype(np.float32)
    if tail == "nan":
        p[splits] = np.nan
    return p


# ------------------------------------------------------------------------------------------ A: embedding
TOKENS = np.array([0, 49, 7, 7, 49], np.int32)
VOCAB = 50


@pytest.mark.parametrize("dim", [256, 1000])
@pytest.mark.parametrize("dt", [BF16, F32])
def test_embed_rows(acc, dt, dim):
    """prefill.cc run_prefill: mc_pf_embed_T, grid ((dim + 255) / 256, M), 256 threads, arguments table, tokens, out, dim, scale,
    use_scale; mc_pf_embed_q8_T the same with the scales behind the table"""
    rng = np.random.default_rng([dim, dt])
    M = TOKENS.size
    table = ref.storage(dt, rng.normal(0, 1, (VOCAB, dim)))
    q = rng.integers(-128, 128, (VOCAB, dim), dtype=np.int8)
    q[0, :256] = np.arange(-128, 128)                      # every int8 value
    s = rng.uniform(1e-3, 3e-2, VOCAB).astype(np.float32)
    sc = ref.embed_scale(dt, dim)
    tb, qb, sb, tokb = acc.to_device(table.reshape(-1)), acc.to_device(q.reshape(-1)), acc.to_device(s), acc.to_device(TOKENS)
    blocks = ((dim + 255) // 256, M)
    for use in (0, 1):
        what = f"{TN[dt]} dim {dim} use_scale {use}"
        out = Out(acc, dt, M * dim, excess=2 * dim)
        launch(acc, f"mc_pf_embed_{TN[dt]}", blocks, 256, [tb, tokb, out.buf, u32(dim), sc, i32(use)])
        acc.wait()
        same(out.take(f"mc_pf_embed {what}", (M, dim)), ref.embed(dt, table, TOKENS, sc if use else None), f"mc_pf_embed {what} against mo.embedding")
        out = Out(acc, dt, M * dim, excess=2 * dim)
        launch(acc, f"mc_pf_embed_q8_{TN[dt]}", blocks, 256, [qb, sb, tokb, out.buf, u32(dim), sc, i32(use)])
        acc.wait()
        same(out.take(f"mc_pf_embed_q8 {what}", (M, dim)), ref.embed_q8(dt, q, s, TOKENS, sc if use else None), f"mc_pf_embed_q8 {what} against the float32 chain")


# ------------------------------------------------------------------------------------------ B: rmsnorm
EPS = f32(1e-5)
NORM_M = 3


def rmsnorm(acc, dt, x, w, res, mu, y=None, what=""):
    """prefill.cc norm_rows: mc_pf_rmsnorm_T, grid M, 256 threads, arguments x, w, res, y, dim, eps, mu"""
    M, dim = x.shape
    out = Out(acc, dt, M * dim)
    xb, wb = acc.to_device(x.reshape(-1)), acc.to_device(w)
    rb = acc.to_device(res.reshape(-1)) if res is not None else None
    launch(acc, f"mc_pf_rmsnorm_{TN[dt]}", (M, 1), 256, [xb, wb, rb, out.buf, u32(dim), EPS, f32(mu)])
    acc.wait()
    return out.take(f"mc_pf_rmsnorm_{TN[dt]} {what}", (M, dim))


# bfloat16: 256 most lanes clamp; 2048 exactly one round; 2056 one packet into the second round; 8192 the last size of the packet path;
# 8200 the scalar path by size; 1004 the scalar path with rows that are not 16-byte aligned.  float: the same edges at 4 elements a packet
@pytest.mark.parametrize("dt,dim", [(BF16, d) for d in (256, 2048, 2056, 8192, 8200, 1004)] + [(F32, d) for d in (256, 4096, 4100, 1002)])
def test_rmsnorm_rows(acc, dt, dim):
    for mu in (0.0, 1.0):
        x, res, w = ref.norm_inputs(dt, NORM_M, dim, mu, seed=2)
        v64 = ref.rmsnorm64(ref.values(dt, x), ref.values(dt, w), EPS, mu)
        for r_ in (None, res):
            what = f"dim {dim} mu {mu} res {'given' if r_ is not None else 'null'}"
            got = rmsnorm(acc, dt, x, w, r_, mu, what=what)
            if dt == F32:
                want = v64 + (r_.astype(np.float64) if r_ is not None else 0.0)
                st = parity.check(F32, got, want, rel=2e-5, what=f"mc_pf_rmsnorm_float {what}")
                print(f"mc_pf_rmsnorm_float {what}: {st}")
            elif r_ is None:
                d = steps(got, bf16_rne64(v64))
                print(f"mc_pf_rmsnorm_bfloat {what}: at most {int(d.max())} bf16 steps from T(float64), {float(np.mean(d != 0)):.5f} differ")
                assert not np.any(ref.is_nan16(got)) and d.max() <= 1, f"{what}: {int(d.max())} bf16 steps from float64"
            else:
                lo, hi = ref.residual_span(r_, v64)
                d = ref.outside(got, lo, hi)
                print(f"mc_pf_rmsnorm_bfloat {what}: at most {int(d.max())} bf16 steps outside [T(res + v_lo), T(res + v_hi)], {float(np.mean(d != 0)):.5f} outside")
                assert not np.any(ref.is_nan16(got)) and d.max() <= 1, f"{what}: {int(d.max())} bf16 steps outside the span"
            for r in range(NORM_M):
                alone = rmsnorm(acc, dt, x[r:r + 1], w, r_[r:r + 1] if r_ is not None else None, mu, what=f"{what} row {r} alone")
                same(alone[0], got[r], f"mc_pf_rmsnorm_{TN[dt]} {what}: row {r} alone against row {r} of the {NORM_M}-row launch")


PARTS_DIMS = [256, 2048, 2056, 8192]
PARTS_SPLITS = [1, 2, 3, 4, 5, 8]


@pytest.mark.parametrize("dim", PARTS_DIMS)
def test_rmsnorm_parts_is_the_reduce_and_the_norm(acc, dim):
    """prefill.cc gemm_residual: mc_pf_rmsnorm_parts_bfloat, grid M, 256 threads, arguments part, splits, M, res, h_out, w, y, dim, eps,
    mu -- bit for bit mc_pf_splitk_reduce_bfloat with the residual and mc_pf_rmsnorm_bfloat on its output"""
    M, mu = NORM_M, 0.0
    rng = np.random.default_rng([3, dim])
    _, res, w = ref.norm_inputs(BF16, M, dim, mu, seed=3)
    resb, wb = acc.to_device(res.reshape(-1)), acc.to_device(w)

    def folded(p, splits):
        pb = acc.to_device(p.reshape(-1))
        h, y = Out(acc, BF16, M * dim), Out(acc, BF16, M * dim)
        launch(acc, "mc_pf_rmsnorm_parts_bfloat", (M, 1), 256, [pb, u32(splits), u32(M), resb, h.buf, wb, y.buf, u32(dim), EPS, f32(mu)])
        acc.wait()
        return pb, h.take(f"rmsnorm_parts dim {dim} splits {splits}: h_out", (M, dim)), y.take(f"rmsnorm_parts dim {dim} splits {splits}: y", (M, dim))

    for splits in PARTS_SPLITS:
        what = f"mc_pf_rmsnorm_parts_bfloat dim {dim} splits {splits}"
        p = parts_buffer(rng, splits, M, dim)
        pb, h, y = folded(p, splits)
        h_ref = reduce_rows(acc, pb, splits, M, dim, res)
        same(h, h_ref, f"{what}: h_out against the reduce with the residual")
        same(y, rmsnorm(acc, BF16, h_ref, w, None, mu), f"{what}: y against mc_pf_rmsnorm_bfloat of the reduce's rows")
        assert not np.any(ref.is_nan16(y))
        if splits in (3, 5):   # pf_part_sum8 walks the splits in fours: nothing past splits * M * dim is read into a sum
            p[splits] = np.nan
            _, h2, y2 = folded(p, splits)
            same(h2, h, f"{what}: h_out with NaN behind the last split")
            same(y2, y, f"{what}: y with NaN behind the last split")


@pytest.mark.parametrize("dim", PARTS_DIMS)
def test_rmsnorm2_parts_is_the_reduce_and_two_norms(acc, dim):
    """prefill.cc gemm_residual with a post norm (gemma3): mc_pf_rmsnorm2_parts_bfloat, grid M, 256 threads, arguments part, splits, M,
    res, h_out, w_post, w_next, y, dim, eps, mu -- bit for bit the reduce without a residual, mc_pf_rmsnorm_bfloat with w_post and the
    residual into h_out, mc_pf_rmsnorm_bfloat with w_next into y"""
    M, mu = NORM_M, 1.0
    rng = np.random.default_rng([4, dim])
    _, res, w_post = ref.norm_inputs(BF16, M, dim, mu, seed=4)
    w_next = ref.norm_inputs(BF16, M, dim, mu, seed=5)[2]
    resb, wpb, wnb = acc.to_device(res.reshape(-1)), acc.to_device(w_post), acc.to_device(w_next)

    def folded(p, splits, next_b):
        pb = acc.to_device(p.reshape(-1))
        h, y = Out(acc, BF16, M * dim), Out(acc, BF16, M * dim)
        launch(acc, "mc_pf_rmsnorm2_parts_bfloat", (M, 1), 256, [pb, u32(splits), u32(M), resb, h.buf, wpb, next_b, y.buf, u32(dim), EPS, f32(mu)])
        acc.wait()
        return pb, h, y

    for splits in PARTS_SPLITS:
        what = f"mc_pf_rmsnorm2_parts_bfloat dim {dim} splits {splits}"
        p = parts_buffer(rng, splits, M, dim)
        pb, hb, yb = folded(p, splits, wnb)
        h, y = hb.take(f"{what}: h_out", (M, dim)), yb.take(f"{what}: y", (M, dim))
        proj = reduce_rows(acc, pb, splits, M, dim)
        h_ref = rmsnorm(acc, BF16, proj, w_post, res, mu)
        same(h, h_ref, f"{what}: h_out against the reduce and the post norm with the residual")
        same(y, rmsnorm(acc, BF16, h_ref, w_next, None, mu), f"{what}: y against the next norm of h_out")
        assert not np.any(ref.is_nan16(y))
        _, hb0, yb0 = folded(p, splits, None)   # the last block: no next norm
        same(hb0.take(f"{what}, w_next null: h_out", (M, dim)), h, f"{what}: h_out without a next norm")
        yb0.untouched(f"{what}, w_next null: y")
        if splits in (3, 5):
            p[splits] = np.nan
            _, hb2, yb2 = folded(p, splits, wnb)
            same(hb2.take(what, (M, dim)), h, f"{what}: h_out with NaN behind the last split")
            same(yb2.take(what, (M, dim)), y, f"{what}: y with NaN behind the last split")


# ------------------------------------------------------------------------------------------ C: activation
@pytest.fixture(scope="module")
def gtab(acc):
    """mc_gelu_table_bfloat: T(gelu) of every bfloat16 value, as the decoder builds it for a gemma prompt"""
    t = acc.alloc(65536 * 4)
    launch(acc, "mc_gelu_table_bfloat", (256, 1), 256, [t])
    acc.wait()
    return t


def act_mul(acc, dt, rows, ffn, gelu, tab, what):
    """prefill.cc run_prefill: mc_pf_act_mul_T, grid ((ffn / PP + 255) / 256 + 1, M), 256 threads, PP = 4 (bfloat16) or 2 (float) pairs a
    thread; arguments in, out, ffn, gelu (, the table: bfloat16)"""
    M = rows.shape[0]
    pp = 4 if dt == BF16 else 2
    out = Out(acc, dt, M * ffn)
    inb = acc.to_device(rows.reshape(-1))
    launch(acc, f"mc_pf_act_mul_{TN[dt]}", ((ffn // pp + 255) // 256 + 1, M), 256, [inb, out.buf, u32(ffn), i32(gelu)] + ([tab] if dt == BF16 else []))
    acc.wait()
    return out.take(f"mc_pf_act_mul_{TN[dt]} {what}", (M, ffn))


def check_silu_bfloat(got, a, b, what):
    """exact against T(silu_T32(a) * b) for every a that is no NaN -- the table of exponentials is the rounded double exp, the rest is
    IEEE float32 rounded to T -- and within one bf16 step of mo.silu + mo.hadamard, at most 0.01 of the elements differing (the cap of
    test_b_gemv_epilogues_and_placement for the same function)"""
    ok = ~ref.is_nan16(a)
    with np.errstate(invalid="ignore", over="ignore"):
        mine = bf(silu_T32(f(a)) * f(b))
    nan_ref = ref.is_nan16(mine)
    assert np.array_equal(ref.is_nan16(got)[ok], nan_ref[ok]), f"{what}: NaN where the float32 chain has none (or the reverse)"
    cmp_ = ok & ~nan_ref
    bad = int(np.sum(got[cmp_] != mine[cmp_]))
    print(f"{what}: {bad} of {int(cmp_.sum())} elements differ from T(silu_T32(a) * b)")
    same(got[cmp_], mine[cmp_], f"{what}: against T(silu_T32(a) * b)")
    theirs = ref.oracle_silu_mul(BF16, a, b)
    both = cmp_ & ~ref.is_nan16(theirs)
    d = steps(got[both], theirs[both])
    print(f"{what}: against mo.silu + mo.hadamard at most {int(d.max())} bf16 steps, share {float(np.mean(d != 0)):.5f} of {int(both.sum())}")
    assert d.max() <= 1 and np.mean(d != 0) <= 0.01, f"{what}: {int(d.max())} steps, share {float(np.mean(d != 0)):.5f} against the oracle"


def test_silu_over_every_bfloat16(acc, etab):
    a = ref.all_bf16().reshape(1, -1)
    rng = np.random.default_rng(6)
    for name, b in (("b = 1", np.full(a.shape, 0x3F80, np.uint16)), ("b random", bf(rng.normal(0, 2, a.shape)))):
        got = act_mul(acc, BF16, ref.interleave(a, b), 65536, 0, etab, f"every bfloat16, {name}")
        check_silu_bfloat(got, a, b, f"mc_pf_act_mul_bfloat silu over every bfloat16, {name}")


@pytest.mark.parametrize("ffn", [1000, 1002])   # 1002: the scalar tail path (ffn % 4 != 0)
def test_act_mul_bfloat_rows(acc, etab, ffn):
    rng = np.random.default_rng(ffn)
    a, b = bf(rng.normal(0, 2, (3, ffn))), bf(rng.normal(0, 2, (3, ffn)))
    got = act_mul(acc, BF16, ref.interleave(a, b), ffn, 0, etab, f"ffn {ffn}")
    check_silu_bfloat(got, a, b, f"mc_pf_act_mul_bfloat silu ffn {ffn}")


@pytest.mark.parametrize("ffn", [1000, 1001])   # 1001: the scalar tail path (ffn % 2 != 0)
def test_act_mul_float_rows(acc, ffn):
    rng = np.random.default_rng(ffn)
    a, b = (rng.normal(0, 2, (3, ffn)).astype(np.float32) for _ in range(2))
    for gelu, fn in ((0, ref.silu64), (1, ref.gelu64)):
        what = f"mc_pf_act_mul_float {'gelu' if gelu else 'silu'} ffn {ffn}"
        got = act_mul(acc, F32, ref.interleave(a, b), ffn, gelu, None, what)
        st = parity.check(F32, got, fn(a) * b.astype(np.float64), rel=2e-5, what=what)
        print(f"{what}: {st}")


def test_act_mul_parts_is_the_reduce_and_the_activation(acc, etab, gtab):
    """prefill.cc run_prefill: mc_pf_act_mul_parts_bfloat, grid ((ffn / 4 + 255) / 256 + 1, M), 256 threads, arguments part, splits, M,
    out, ffn, gelu, table -- bit for bit mc_pf_splitk_reduce_bfloat followed by mc_pf_act_mul_bfloat"""
    M, ffn = 3, 1000
    rng = np.random.default_rng(7)
    for splits in (1, 2, 3, 4, 5):
        p = parts_buffer(rng, splits, M, 2 * ffn, tail="nan")
        pb = acc.to_device(p.reshape(-1))
        rows = reduce_rows(acc, pb, splits, M, 2 * ffn)
        for gelu, tab, name in ((0, etab, "silu"), (1, gtab, "gelu from the table"), (1, None, "gelu without a table")):
            what = f"mc_pf_act_mul_parts_bfloat {name} splits {splits}"
            out = Out(acc, BF16, M * ffn)
            launch(acc, "mc_pf_act_mul_parts_bfloat", ((ffn // 4 + 255) // 256 + 1, M), 256, [pb, u32(splits), u32(M), out.buf, u32(ffn), i32(gelu), tab])
            acc.wait()
            got = out.take(what, (M, ffn))
            assert not np.any(ref.is_nan16(got)), what
            same(got, act_mul(acc, BF16, rows, ffn, gelu, tab, what), f"{what}: against the reduce and mc_pf_act_mul_bfloat")


# ------------------------------------------------------------------------------------------ D: rope and cache write
class RopeDev:
    """the device side of one pf_rows_ref.RopeRef: the table of 64 rows, and the launches of the five kernels in the forms and grids of
    prefill_plan.h plan_rope with the arguments of prefill.cc qkv_rope_cache"""

    def __init__(self, acc, rr):
        self.rr = rr
        self.cb, self.sb, fcos, fsin = rope_table(acc, rr.table_rows, rr.hd, ref.THETA)
        parity.exact(fcos, rr.rc, "mc_rope_table cos against rope_freqs")
        parity.exact(fsin, rr.rs, "mc_rope_table sin against rope_freqs")
        per = 2048 // rr.hd
        # both tails of the four-pair grid are present: a last V tile of fewer than 16 rows, a last workgroup of fewer than `per` units
        assert rr.M % 16 != 0 and ((rr.H + rr.KV) * rr.M) % per != 0
        self.gx = ((rr.H + rr.KV) * rr.M + per - 1) // per + rr.KV * ((rr.M + 15) // 16)    # plan_rope: q / k units, then v tiles of 16 rows

    def launch(self, acc, form, rows, kc0, vt0, splits=0, q_w=None, k_w=None, what=""):
        """form "pair": plan_rope's rope_form::pair, grid (H + 2 KV, M), hd / 2 threads; "v4": rope_form::v4, grid gx, 256 threads.
        rows: [M][NQ] of T, or (splits > 0) the fp32 parts [splits + 1][M][NQ].  Returns the q rows and the whole K / V buffers, guards
        included; the q rows past M are held to their pattern"""
        rr = self.rr
        dt, H, KV, hd, M = rr.dt, rr.H, rr.KV, rr.hd, rr.M
        q = Out(acc, dt, M * H * hd, excess=16 * H * hd)
        k_host, v_host = with_guard(dt, kc0), with_guard(dt, vt0)
        kb, vb = acc.to_device(k_host), acc.to_device(v_host)
        rb = acc.to_device(np.ascontiguousarray(rows).reshape(-1))
        qwb = acc.to_device(q_w) if q_w is not None else None
        kwb = acc.to_device(k_w) if k_w is not None else None
        shape = [u32(H), u32(KV), u32(hd), u32(rr.max_seq), u32(rr.start_pos), u32(rr.rope_row0)]
        norms = [qwb, kwb]
        tail = [f32(ref.NORM_EPS), f32(ref.NORM_MU)]
        front = [rb, u32(splits), u32(M), q.buf] if splits else [rb, q.buf]
        name = f"mc_pf_rope_cache_{'parts_' if splits else ''}{'v4_' if form == 'v4' else ''}{TN[dt]}"
        if form == "pair":
            launch(acc, name, (H + 2 * KV, M), hd // 2, front + [kb, vb, self.cb, self.sb] + norms + shape + tail)
        else:
            launch(acc, name, (self.gx, 1), 256, front + [kb, vb, self.cb, self.sb] + shape + ([] if splits else [u32(M)]) + norms + tail)
        acc.wait()
        npd = ref.mo.np_dtype(dt)
        return q.take(f"{name} {what}: q rows", (M, H, hd)), kb.download(npd, k_host.size), vb.download(npd, v_host.size)

    def expect(self, x, kc0, vt0):
        q, kc, vt = self.rr.expect(x, kc0, vt0)
        return q, with_guard(self.rr.dt, kc), with_guard(self.rr.dt, vt)


WHAT3 = ("q rows", "K cache (every slot, the guard included)", "V cache (every slot, the guard included)")


@pytest.mark.parametrize("H,KV,hd", ref.ROPE_SHAPES)
def test_rope_cache_without_norms(acc, H, KV, hd):
    """mo.rope of the un-partnered q and k heads at table row rope_row0 + r; exactly the call's slots of K and V replaced"""
    for dt, form in [(BF16, "pair"), (BF16, "v4")] + ([(F32, "pair")] if hd <= 64 else []):
        rd = RopeDev(acc, ref.rope_ref(dt, H, KV, hd))
        x, kc0, vt0 = rd.rr.inputs(seed=5)
        got = rd.launch(acc, form, x, kc0, vt0)
        for g, e, name in zip(got, rd.expect(x, kc0, vt0), WHAT3):
            same(g, e, f"{TN[dt]} {form} H {H} KV {KV} hd {hd}: {name} against mo.rope")


@pytest.mark.parametrize("H,KV,hd", ref.ROPE_SHAPES)
def test_rope_cache_with_q_and_k_norms(acc, H, KV, hd):
    """The one-pair launch with norms -- workgroups of hd / 2 = 16 and 32 threads at head_dim 32 and 64, where wave_sum shuffles across
    lanes the workgroup does not have -- against the float64 norm: where every value within 2^-20 of it rounds to the same bfloat16
    the result is mo.rope of T(xn64) exactly, elsewhere within one step of the span of the ropes of the four corners (the method of
    test_pp_rope_cache_parts_sums_in_front_of_the_rope).  The four-pair launch (head_dim 128 / 256: rope_v4_ok) bit for bit the one-pair"""
    rd = RopeDev(acc, ref.rope_ref(BF16, H, KV, hd))
    rr = rd.rr
    x, kc0, vt0, qw, kw = rr.inputs(seed=ref.NORM_SEED, norms=True)
    for q_w, k_w, name in ((qw, kw, "q and k norm"), (qw, None, "q norm only"), (None, kw, "k norm only")):
        what = f"H {H} KV {KV} hd {hd} {name}"
        lo, hi, amb = rr.norm_span(x, q_w, k_w, ref.NORM_EPS, ref.NORM_MU)
        on = rr.normed64(x, q_w, k_w, ref.NORM_EPS, ref.NORM_MU)[1]
        share = float(amb.sum() / on.sum())
        print(f"{what}: {int(amb.sum())} of {int(on.sum())} normed values have more than one correct rounding (share {share:.5f})")
        assert share < 1e-2
        got = rd.launch(acc, "pair", x, kc0, vt0, q_w=q_w, k_w=k_w, what=what)
        for g, (omin, omax), n3 in zip(got, rr.corners(lo, hi, kc0, vt0), WHAT3):
            if g.ndim == 1:   # a cache: the guard behind it first
                assert np.all(g[-GUARD:] == NAN), f"{what}: {n3}: the guard was written"
                g = g[:-GUARD].reshape(omin.shape)
            assert not np.any(ref.is_nan16(g)), f"{what}: {n3}: a NaN"
            d = ref.outside(g, omin, omax)
            print(f"mc_pf_rope_cache_bfloat {what}: {n3}: at most {int(d.max())} bf16 steps outside the span, {float(np.mean(d != 0)):.5f} outside, "
                  f"{float(np.mean(omin != omax)):.5f} have a span")
            assert np.all(d[omin == omax] == 0), f"{what}: {n3}: {int(np.sum(d[omin == omax] != 0))} values differ from mo.rope of T(xn64)"
            assert d.max() <= 1, f"{what}: {n3}: {int(d.max())} bf16 steps outside the span of the four corners"
        if hd in (128, 256):
            for g, p, n3 in zip(rd.launch(acc, "v4", x, kc0, vt0, q_w=q_w, k_w=k_w, what=what), got, WHAT3):
                same(g, p, f"mc_pf_rope_cache_v4_bfloat {what}: {n3} against mc_pf_rope_cache_bfloat")


@pytest.mark.parametrize("H,KV,hd", ref.ROPE_SHAPES)
def test_rope_cache_parts_are_the_reduce_and_the_plain_kernel(acc, H, KV, hd):
    rd = RopeDev(acc, ref.rope_ref(BF16, H, KV, hd))
    rr = rd.rr
    _, kc0, vt0, qw, kw = rr.inputs(seed=8, norms=True)
    rng = np.random.default_rng([9, hd])
    for splits in (1, 2, 3, 4, 5):
        p = parts_buffer(rng, splits, rr.M, rr.NQ, tail="nan")
        pb = acc.to_device(p.reshape(-1))
        x = reduce_rows(acc, pb, splits, rr.M, rr.NQ)
        del pb
        for q_w, k_w, name in ((None, None, "no norms"), (qw, kw, "q and k norms")):
            what = f"H {H} KV {KV} hd {hd} splits {splits} {name}"
            plain = rd.launch(acc, "pair", x, kc0, vt0, q_w=q_w, k_w=k_w, what=what)
            parts = rd.launch(acc, "pair", p, kc0, vt0, splits=splits, q_w=q_w, k_w=k_w, what=what)
            for g, e, n3 in zip(parts, plain, WHAT3):
                same(g, e, f"mc_pf_rope_cache_parts_bfloat {what}: {n3} against the reduce and mc_pf_rope_cache_bfloat")
            if q_w is None or hd in (128, 256):   # rope_v4_ok
                plain4 = rd.launch(acc, "v4", x, kc0, vt0, q_w=q_w, k_w=k_w, what=what)
                parts4 = rd.launch(acc, "v4", p, kc0, vt0, splits=splits, q_w=q_w, k_w=k_w, what=what)
                for g, e4, e, n3 in zip(parts4, plain4, parts, WHAT3):
                    same(g, e4, f"mc_pf_rope_cache_parts_v4_bfloat {what}: {n3} against the reduce and mc_pf_rope_cache_v4_bfloat")
                    same(g, e, f"mc_pf_rope_cache_parts_v4_bfloat {what}: {n3} against mc_pf_rope_cache_parts_bfloat")


# ------------------------------------------------------------------------------------------ E: two-pass attention
ATT_H, ATT_KV = 4, 2
# M, S, window, max_seq
ATT_CASES = [(5, 5, 0, 8), (17, 17, 0, 24),
             (37, 48, 0, 48),     # a context in front whose columns the reference's mask hides
             (37, 37, 4, 40),
             (37, 45, 20, 48),    # S % 8 != 0: the element-wise probability load
             (40, 40, 0, 40)]     # S = max_seq, no multiple of 32: the V load is guarded by c + 8 <= max_seq


@pytest.mark.parametrize("M,S,window,max_seq", ATT_CASES)
@pytest.mark.parametrize("dt,hd", [(BF16, 64), (F32, 64), (F32, 32)])
def test_two_pass_attention(acc, dt, hd, M, S, window, max_seq):
    """prefill.cc run_prefill: mc_pf_scores_T, grid ((M + 15) / 16, H), 256 threads, arguments Q, kc, probs, M, S, H, n_rep, hd, max_seq,
    scale, window; mc_pf_pv_T the same grid, arguments probs, vt, out, M, S, H, n_rep, hd, max_seq, window"""
    H, KV, n_rep = ATT_H, ATT_KV, ATT_H // ATT_KV
    what = f"{TN[dt]} hd {hd} M {M} S {S} window {window} max_seq {max_seq}"
    rng = np.random.default_rng([hd, M, S])
    q = ref.storage(dt, rng.normal(0, 1, (M, H, hd)))
    k = ref.storage(dt, rng.normal(0, 0.4, (S, KV, hd)))        # the magnitudes of test_pf_attn_kernels_gpu.Data
    v = ref.storage(dt, rng.normal(0, 0.5, (S, KV, hd)))
    kc = ref.storage(dt, rng.normal(0, 30, (KV, max_seq, hd)))  # N(0, 30) behind S
    vt = ref.storage(dt, rng.normal(0, 30, (KV, hd, max_seq)))
    kc[:, :S], vt[:, :, :S] = k.transpose(1, 0, 2), v.transpose(1, 2, 0)
    k_host, v_host = with_guard(dt, kc), with_guard(dt, vt)
    kb, vb = acc.to_device(k_host), acc.to_device(v_host)
    q_host = fresh(dt, (M + 16) * H * hd)
    q_host[:q.size] = q.reshape(-1)
    qb = acc.to_device(q_host)
    probs, out = Out(acc, dt, H * M * S), Out(acc, dt, M * H * hd, excess=16 * H * hd)
    scale = scale_of(hd) if dt == BF16 else f32(hd ** -0.5)
    blocks = ((M + 15) // 16, H)
    launch(acc, f"mc_pf_scores_{TN[dt]}", blocks, 256, [qb, kb, probs.buf, u32(M), u32(S), u32(H), u32(n_rep), u32(hd), u32(max_seq), scale, u32(window)])
    launch(acc, f"mc_pf_pv_{TN[dt]}", blocks, 256, [probs.buf, vb, out.buf, u32(M), u32(S), u32(H), u32(n_rep), u32(hd), u32(max_seq), u32(window)])
    acc.wait()
    p = probs.take(f"{what}: probs", (H, M, S))
    got = out.take(f"{what}: out rows at and past M", (M, H, hd))
    npd = ref.mo.np_dtype(dt)
    same(kb.download(npd, k_host.size), k_host, f"{what}: K cache and guard")
    same(vb.download(npd, v_host.size), v_host, f"{what}: V cache and guard")
    same(qb.download(npd, q_host.size), q_host, f"{what}: Q")
    # ---- the probabilities: +0 bit for bit outside the visible keys, a sum of 1 inside
    lo, hi = pr.visible(np.arange(M), M, S, window)
    cols = np.arange(S)
    vis = (cols[None, :] >= lo[:, None]) & (cols[None, :] <= hi[:, None])          # [M][S]
    assert np.all(bits(p)[:, ~vis] == 0), f"{what}: a probability outside the visible keys is not +0"
    pv_ = ref.values(dt, p).astype(np.float64)
    assert np.all(np.isfinite(pv_)) and np.all(pv_ >= 0)
    err = np.abs(pv_.sum(axis=2) - 1.0)
    print(f"{what}: |sum of a row's probabilities - 1| at most {err.max():.3g} (bound {ref.prob_sum_bound(dt, S):.3g})")
    assert np.all(err <= ref.prob_sum_bound(dt, S)), f"{what}: a row's probabilities sum to 1 -+ {err.max():.3g}"
    # ---- every output row against the oracle over exactly its visible keys
    worst, fails, differ = {}, [], 0
    for r in range(M):
        want = oracle_attention(q[r], k[lo[r]:hi[r] + 1], v[lo[r]:hi[r] + 1], n_rep, float(scale), dt)
        differ += int(np.sum(bits(got[r]) != bits(want)))
        try:
            if dt == BF16:   # the bound of test_rows_kernels_gpu.check_against
                st = parity.check(BF16, got[r], want, rel=2e-3, max_ulp=1, max_frac=0.03, scale_aware=True, what=f"{what} row {r}")
            else:
                st = parity.check(F32, got[r], want, rel=1e-4, what=f"{what} row {r}")
            worst = {key: max(worst.get(key, 0), val) for key, val in st.items()}
        except AssertionError as e:
            fails.append(str(e))
    print(f"{what}: worst over the rows {worst}; {differ / got.size:.4f} of all elements differ; {len(fails)} rows outside the bound")
    assert not fails, fails[:5]


# ------------------------------------------------------------------------------------------ the table
ROW_KERNELS = [
    "mc_pf_embed_bfloat", "mc_pf_embed_float", "mc_pf_embed_q8_bfloat", "mc_pf_embed_q8_float",
    "mc_pf_rmsnorm_bfloat", "mc_pf_rmsnorm_float", "mc_pf_rmsnorm_parts_bfloat", "mc_pf_rmsnorm2_parts_bfloat",
    "mc_pf_act_mul_bfloat", "mc_pf_act_mul_float", "mc_pf_act_mul_parts_bfloat",
    "mc_pf_rope_cache_bfloat", "mc_pf_rope_cache_float", "mc_pf_rope_cache_parts_bfloat", "mc_pf_rope_cache_v4_bfloat", "mc_pf_rope_cache_parts_v4_bfloat",
    "mc_pf_scores_bfloat", "mc_pf_scores_float", "mc_pf_pv_bfloat", "mc_pf_pv_float",
]


def test_every_row_kernel_of_the_table_was_launched(acc, request):
    """every name exists in the code object, and -- where the whole module ran -- occurs in the module's own launches: a rename that drops
    one from the tests above shows here"""
    for name in ROW_KERNELS:
        acc.load(name)
    module = sys.modules[__name__]
    mine = {item.function.__name__ for item in request.session.items if getattr(item, "module", None) is module}
    if mine == {n for n in dir(module) if n.startswith("test_")}:
        missing = [n for n in ROW_KERNELS if n not in LAUNCHED]
        assert not missing, f"never launched by this module: {missing}"
