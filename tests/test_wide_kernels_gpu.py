"""Kernel-level tests of the wide batch's GEMV (metalchat_amd/csrc/kernels/wide_kernels.hip), `mc_wb_gemv_{i4,w}_bfloat_e{0,1,2}`
launched BY NAME at M from 1 to 64 activation rows and at every tile count a grid can ask for (1, 2, 4, 8 weight tiles per workgroup):

  * every row bit for bit what `mc_b_gemv_*_eE` writes for that activation row, run over the same activations eight rows at a time
    (e1: both from the same prefilled y);
  * within check_e0's bound of the float64 product, so the test does not only compare two kernels with each other: e0 directly, e1
    on a residual of +0.0 (T(0 + T(acc)) is T(acc)), e2 as the composition of its own e0 that test_batch_kernels_gpu states for
    mc_b_gemv_*_e2;
  * the activation rows at and past M hold NaN and reach no output bit; y outside [M][N] (e2: [M][N / 2]) keeps its NaN."""
import numpy as np
import pytest

import parity
from test_batch_kernels_gpu import BG_THREADS, I4, NAN, W, XMAG, Packed, bf, f, silu_T32, steps
from test_verify_kernels_gpu import check_e0

pytestmark = pytest.mark.gpu
ROWS = 64                              # abi.h MC_WIDE_BATCH_MAX
MS = [1, 16, 17, 32, 33, 48, 63, 64]   # the ends of each 16-column group, and one row into the next
TILES = [1, 2, 4, 8]
# K = 1024: one 128-weight chunk per wave, the loop runs once (the tail form alone); K = 4096: four (the rounds of the main loop at
# 1, 2 and 4 tiles, four single chunks at 8).  int4 groups of 128 and of K
SHAPES = [(I4, 1024, 128), (I4, 1024, 1024), (I4, 4096, 128), (I4, 4096, 4096), (W, 1024, 0), (W, 4096, 0)]
OUT = {0: 2064, 1: 2064, 2: 2080}      # 129 / 130 weight tiles: no multiple of 2, 4 or 8 of them (e2: out % 32 == 0)


def activations64(K, seed):
    """64 activation rows: test_batch_kernels_gpu.activations' magnitudes (an all-zero row among every eight)"""
    rng = np.random.default_rng(seed)
    return bf(rng.normal(0, 1, (ROWS, K)) * np.tile(np.array(XMAG), ROWS // 8)[:, None])


def launch_wide(acc, P, xb, M, epi, tiles, y_init):
    """mc_wb_gemv_* over the first M of the 64 rows in xb, ceil(out / 16 / tiles) workgroups, into a copy of y_init [rows][ldy]"""
    import metalchat_amd as mc

    rows, ldy = y_init.shape
    yb = acc.to_device(y_init.reshape(-1))
    wrap = lambda p: acc.wrap(p, 1 << 40) if p else None
    groups = (P.out // 16 + tiles - 1) // tiles
    mc.KernelTask(acc.load(f"mc_wb_gemv_{P.fmt}_bfloat_e{epi}"), (groups * BG_THREADS, 1, 1), (BG_THREADS, 1, 1),
                  [wrap(P.wptr), wrap(P.sptr), xb, yb, np.uint32(P.K), np.uint32(P.ng), np.uint32(P.group), np.uint32(M), np.uint32(P.out),
                   np.uint32(ldy)])()
    acc.wait()
    return yb.download(np.uint16, rows * ldy).reshape(rows, ldy)


@pytest.mark.parametrize("epi", [0, 1, 2])
@pytest.mark.parametrize("fmt,K,group", SHAPES)
def test_wb_gemv_rows_are_the_batch_gemv_rows(acc, fmt, K, group, epi):
    out = OUT[epi]
    width = out // 2 if epi == 2 else out
    ldy, rows = width + 16, ROWS + 2
    P = Packed(acc, fmt, K, group, out, seed=5 * K + group + epi + 1)
    x = activations64(K, seed=K + group + 11)
    y64, a = P.reference(x)
    rng = np.random.default_rng(K + epi)
    # the narrow kernel, eight rows at a time: e0 (the float64 check's subject and the residual's scale), and the epilogue
    e0 = np.concatenate([P.launch(acc, x[r:r + 8]) for r in range(0, ROWS, 8)])
    check_e0(e0, y64, a, K, f"mc_b_gemv e0 {fmt} K{K} g{group}")
    R = bf(rng.normal(0, 1, (ROWS, out)) * np.abs(f(e0)).mean(axis=1, keepdims=True).clip(1e-3) * 4)
    if epi == 0:
        narrow = e0
    elif epi == 1:
        narrow = np.concatenate([P.launch(acc, x[r:r + 8], epi=1, y_init=R[r:r + 8].copy()) for r in range(0, ROWS, 8)])
    else:
        narrow = np.concatenate([P.launch(acc, x[r:r + 8], epi=2) for r in range(0, ROWS, 8)])
    assert narrow.shape == (ROWS, width)

    for M in MS:
        xm = x.copy()
        xm[M:] = NAN                                  # the rows at and past M must reach nothing
        xb = acc.to_device(xm.reshape(-1))
        init = np.full((rows, ldy), NAN, np.uint16)
        if epi == 1:
            init[:M, :out] = R[:M]
        for tiles in TILES:
            what = f"mc_wb_gemv_{fmt}_bfloat_e{epi} K{K} g{group} M{M} tiles{tiles}"
            got = launch_wide(acc, P, xb, M, epi, tiles, init)
            parity.exact(got[:M, :width], narrow[:M], f"{what}: every row against mc_b_gemv_{fmt}_bfloat_e{epi}")
            assert np.all(got[:M, width:] == NAN), f"{what}: columns past the result written"
            assert np.all(got[M:] == NAN), f"{what}: rows at or past M written"
        # against float64, once per M (the tile counts agree bit for bit by the comparison above)
        if epi == 2:
            w0 = launch_wide(acc, P, xb, M, 0, 8, np.full((rows, out), NAN, np.uint16))[:M]
        else:
            z = np.full((rows, ldy), NAN, np.uint16)
            z[:M, :out] = 0                           # e1 on +0.0: T(0 + T(acc))
            w0 = launch_wide(acc, P, xb, M, epi, 4, z)[:M, :out]
        frac = check_e0(w0, y64[:M], a[:M], K, f"mc_wb_gemv e{min(epi, 1)} {fmt} K{K} g{group} M{M}")
        print(f"mc_wb_gemv_{fmt} e{epi} K{K} g{group} M{M}: {frac:.5f} of the outputs differ from T(y64)")
        if epi == 2:
            # silu_T(e0[2j]) * e0[2j + 1]: the device exp and numpy's may differ in the last float place, which can move the
            # result by one bfloat step; nothing else differs (test_batch_kernels_gpu's statement of e2)
            got2 = launch_wide(acc, P, xb, M, 2, 8, np.full((rows, ldy), NAN, np.uint16))[:M, :width]
            w0f = f(w0)
            d = steps(got2, bf(silu_T32(w0f[:, 0::2]) * w0f[:, 1::2]))
            assert d.max() <= 1, f"e2 {fmt} K{K} M{M}: {d.max()} bf16 steps from silu_T(e0[2j]) * e0[2j+1]"
            assert np.mean(d != 0) <= 0.01, f"e2 {fmt} K{K} M{M}: {np.mean(d != 0):.4f} of outputs off by one step"
    # a row's bits do not depend on its index: rows 40..63 as rows 0..23
    moved = np.full((ROWS, K), NAN, np.uint16)
    moved[:24] = x[40:]
    init = np.full((rows, ldy), NAN, np.uint16)
    if epi == 1:
        init[:24, :out] = R[40:]
    got = launch_wide(acc, P, acc.to_device(moved.reshape(-1)), 24, epi, 4, init)
    parity.exact(got[:24, :width], narrow[40:], f"mc_wb_gemv_{fmt} e{epi} K{K}: rows moved to other columns")
    P.release()
