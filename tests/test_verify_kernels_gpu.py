"""Kernel-level tests of speculative verify (metalchat_amd/csrc/kernels/verify_kernels.hip), each kernel launched BY NAME:

  * the head over M rows `mc_v_head_{i4,w}_bfloat`, M from 1 to 128: every row bit for bit what `mc_b_gemv_*_e0` writes for that
    activation row (run over the same activations eight rows at a time) AND within check_e0's bound of the float64 product, so the
    test does not only compare two kernels with each other; rows at or past M and everything outside [M][out] stay NaN;
  * the pick per packed row `mc_v_argmax_bfloat` against first_max on pick_rows' tables;
  * the acceptance `mc_v_accept` against verify_rule.py on random tables with planted matches and mismatches."""
import numpy as np
import pytest

import parity
import rows_tables as rt
import verify_rule as vr
from test_batch_kernels_gpu import BG_THREADS, I4, NAN, W, XMAG, Packed, bf, check_e0, first_max, pick_rows

pytestmark = pytest.mark.gpu
VH_ROWS = 64    # weight rows of one mc_v_head_* workgroup (abi.h VH_TILES x 16)
OUT = 2048 + 16  # not a multiple of VH_ROWS: the last workgroup owns one 16-row tile
MS = [1, 7, 8, 9, 16, 17, 40, 128]
HEAD_CASES = [(I4, 1024, 128), (I4, 2048, 128), (I4, 4096, 128), (I4, 1024, 1024), (I4, 2048, 512), (I4, 4096, 1024),
              (W, 1024, 0), (W, 2048, 0), (W, 4096, 0)]


def activations128(K, seed):
    """128 activation rows: test_batch_kernels_gpu.activations' magnitudes (an all-zero row among every eight), fresh values per group"""
    rng = np.random.default_rng(seed)
    return bf(rng.normal(0, 1, (128, K)) * np.tile(np.array(XMAG), 16)[:, None])


def launch_head(acc, P, x, M, ldy, rows):
    """mc_v_head_* over the first M rows of x into a NaN buffer of `rows` rows at stride ldy"""
    import metalchat_amd as mc

    yb = acc.to_device(np.full(rows * ldy, NAN, np.uint16))
    wrap = lambda p: acc.wrap(p, 1 << 40) if p else None
    groups = (P.out + VH_ROWS - 1) // VH_ROWS
    mc.KernelTask(acc.load(f"mc_v_head_{P.fmt}_bfloat"), (groups * BG_THREADS, 1, 1), (BG_THREADS, 1, 1),
                  [wrap(P.wptr), wrap(P.sptr), acc.to_device(np.ascontiguousarray(x[:M]).reshape(-1)), yb, np.uint32(P.K), np.uint32(P.ng),
                   np.uint32(P.group), np.uint32(M), np.uint32(P.out), np.uint32(ldy)])()
    acc.wait()
    return yb.download(np.uint16, rows * ldy).reshape(rows, ldy)


@pytest.mark.parametrize("fmt,K,group", HEAD_CASES)
def test_v_head_rows_are_the_batch_gemv_rows(acc, fmt, K, group):
    P = Packed(acc, fmt, K, group, OUT, seed=3 * K + group + 1)
    x = activations128(K, seed=K + group + 5)
    y64, a = P.reference(x)
    gemv = np.concatenate([P.launch(acc, x[r:r + 8]) for r in range(0, 128, 8)])   # mc_b_gemv_*_e0, eight rows at a time
    check_e0(gemv, y64, a, K, f"mc_b_gemv {fmt} K{K} g{group}")
    ldy = OUT + 16
    for M in MS:
        what = f"mc_v_head {fmt} K{K} g{group} M{M}"
        rows = min(M + 2, 130)
        got = launch_head(acc, P, x, M, ldy, rows)
        parity.exact(got[:M, :OUT], gemv[:M], f"{what}: every row against mc_b_gemv_{fmt}_bfloat_e0")
        frac = check_e0(got[:M, :OUT], y64[:M], a[:M], K, what)
        print(f"{what}: {frac:.5f} of the outputs differ from T(y64)")
        assert np.all(got[:M, OUT:] == NAN), f"{what}: columns past out written"
        assert np.all(got[M:] == NAN), f"{what}: rows at or past M written"
    # a row's bits do not depend on its index: rows 100..127 as rows 0..27
    moved = launch_head(acc, P, x[100:], 28, OUT, 28)
    parity.exact(moved, gemv[100:], f"mc_v_head {fmt} K{K}: rows moved to other columns")
    P.release()


@pytest.mark.parametrize("n", [2048, 2032, 128256])
def test_v_argmax_rows(acc, n):
    import metalchat_amd as mc

    logits = np.concatenate([pick_rows(n, n + 17 * i) for i in range(16)])    # 128 rows: ties, the last index, -inf rows
    lb = acc.to_device(logits.reshape(-1))
    for M in (1, 37, 128):
        picks = acc.to_device(np.full(130, -7, np.int32))
        mc.KernelTask(acc.load("mc_v_argmax_bfloat"), (1024, M, 1), (1024, 1, 1), [lb, np.uint32(n), picks])()
        acc.wait()
        got = picks.download(np.int32, 130)
        exp = np.full(130, -7, np.int32)
        exp[:M] = [first_max(logits[r]) for r in range(M)]
        parity.exact(got, exp, f"mc_v_argmax vocab {n} M {M}")


ACCEPT_CASES = [
    # lens[B] (0: the row is not in the call), vocab
    ([16] * 8, 2056), ([2, 0, 16, 5, 0, 9, 3, 0], 2056), ([0, 0, 0, 7], 128256), ([4, 8, 16, 2, 3, 16, 11, 6], 4096), ([2], 2048),
]


@pytest.mark.parametrize("lens,vocab", ACCEPT_CASES)
def test_v_accept_against_the_rule(acc, lens, vocab):
    import metalchat_amd as mc

    B = len(lens)
    rng = np.random.default_rng(sum(lens) + vocab)
    segs = rt.segments(lens, [int(p) for p in rng.integers(0, 100, B)])
    M = sum(lens)
    for trial in range(4):
        tokens = rng.integers(0, vocab, M).astype(np.int32)
        picks = rng.integers(0, vocab, M).astype(np.int32)
        chunks, prow, want = [None] * B, [None] * B, {}
        for row, _, off, n in segs:
            # trial 0: everything accepted; 1: nothing; else a random count.  Matches are planted behind the mismatch as well
            a = {0: n - 1, 1: 0}.get(trial, int(rng.integers(0, n)))
            picks[off:off + n - 1] = tokens[off + 1:off + n]
            if a < n - 1:
                picks[off + a] = (tokens[off + a + 1] + 1 + int(rng.integers(0, vocab - 1))) % vocab
            chunks[row], prow[row], want[row] = tokens[off:off + n], picks[off:off + n], a
        exp_acc, exp_next = vr.accept_rows(chunks, prow)
        assert all(exp_acc[r] == a for r, a in want.items())
        logits = rng.integers(0, 0x7F80, (M, vocab)).astype(np.uint16)
        ab, nb = acc.to_device(np.full(B + 2, -1, np.int32)), acc.to_device(np.full(B + 2, -1, np.int32))
        lo = acc.to_device(np.full((B + 1) * vocab, NAN, np.uint16))
        gx = min(64, (vocab // 8 + 255) // 256)
        mc.KernelTask(acc.load("mc_v_accept"), (gx * 256, len(segs), 1), (256, 1, 1),
                      [acc.to_device(rt.words(segs, 4).reshape(-1)), acc.to_device(tokens), acc.to_device(picks), acc.to_device(logits.reshape(-1)),
                       np.uint32(vocab), ab, nb, lo])()
        acc.wait()
        what = f"mc_v_accept lens {lens} vocab {vocab} trial {trial}"
        parity.exact(ab.download(np.int32, B + 2), np.concatenate([exp_acc, [-1, -1]]).astype(np.int32), f"{what}: accepted")
        parity.exact(nb.download(np.int32, B + 2), np.concatenate([exp_next, [-1, -1]]).astype(np.int32), f"{what}: next tokens")
        got = lo.download(np.uint16, (B + 1) * vocab).reshape(B + 1, vocab)
        for row, _, off, n in segs:
            parity.exact(got[row], logits[off + want[row]], f"{what}: row {row}'s logits are those of chunk row {want[row]}")
        for r in range(B + 1):
            if r >= B or lens[r] == 0:
                assert np.all(got[r] == NAN), f"{what}: logits row {r} written"
