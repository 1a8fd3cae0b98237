"""The one-prompt attention kernels (kernels/prefill_kernels.hip mc_pf_attn*, chosen by prefill.cc plan_attention) restated without a
device for test_pf_attn_kernels_gpu.py: which keys a chunk row sees, the grid and block each of the eleven names is launched with and
the preconditions its host rule checks, and a probe whose expected output bits are fixed by the SET of visible keys alone.

This is a RESTATEMENT.  `visible` is written from the reference's mask text (nn/attention.h:283-321), not from the kernels'
pf_visible: make_causal_mask fills [M][S] with -inf and clears, inside the LAST M columns, the part at and below the diagonal
(triu(..., 1) keeps the -inf strictly above it); make_sliding_causal_mask adds a second matrix whose last M columns, transposed,
keep -inf from diagonal `window` on, i.e. where row - column >= window.  Columns of an earlier context stay -inf in both.
(The reference builds no mask at all for a chunk of ONE row, size0 > 1; the tests here use chunks of two rows and more.)
test_pf_attn_rule_cpu.py holds `visible` to a literal mask matrix and `mask_expected` to the oracle."""
import functools

import numpy as np

from oracle import mc_oracle as mo

# name -> (head_dim, query heads per workgroup NH, rows per row tile RT, threads, row tiles may be dealt in pairs)
KERNELS = {
    "mc_pf_attn_bfloat_hd32": (32, 1, 16, 256, False), "mc_pf_attn_bfloat_hd64": (64, 1, 16, 256, False),
    "mc_pf_attn_bfloat_hd128": (128, 1, 16, 256, False), "mc_pf_attn_bfloat_hd256": (256, 1, 16, 256, False),
    "mc_pf_attn2_bfloat_hd32": (32, 2, 16, 256, False), "mc_pf_attn2_bfloat_hd64": (64, 2, 16, 256, False),
    "mc_pf_attn2_bfloat_hd128": (128, 2, 16, 256, False),
    "mc_pf_attn4_bfloat_hd128": (128, 4, 16, 256, False),
    "mc_pf_attn8_bfloat_hd128": (128, 4, 32, 512, True),      # 8 waves = 4 heads x 2 blocks of 16 rows
    "mc_pf_attn8_bfloat_hd64_h8": (64, 8, 16, 512, True),     # 8 heads x 1 block
    "mc_pf_attn8_bfloat_hd64_h4": (64, 4, 32, 512, True),     # 4 heads x 2 blocks
    "mc_pf_attn8_bfloat_hd256": (256, 1, 64, 256, True),      # 4 waves = 1 head x 4 blocks
}


def head_dim(kernel):
    return KERNELS[kernel][0]


def row_tile(kernel):
    return KERNELS[kernel][2]


def pairable(kernel):
    return KERNELS[kernel][4]


def visible(r, M, S, window):
    """the inclusive key range (lo, hi) of chunk row r (an int or an array of rows) of M rows whose last row sits at slot S - 1;
    window == 0: no window"""
    assert np.all(0 <= np.asarray(r)) and np.all(np.asarray(r) < M) and M <= S and window >= 0
    first = S - M                                                 # the causal square is the last M columns
    lo = np.maximum(0, r + 1 - window) if window else 0 * r       # row - column < window
    return first + lo, first + r                                  # column <= row


def launch_shape(kernel, M, H, pair, *, n_rep, max_seq, S):
    """((grid.x, grid.y) in workgroups, threads) as plan_attention launches `kernel`, and the conditions under which it does: a launch
    outside them reads outside Q or the caches, so they are asserted here and every test launches through this function"""
    hd, nh, rt, threads, can_pair = KERNELS[kernel]
    assert 1 <= M <= S <= max_seq, (M, S, max_seq)
    assert max_seq % 8 == 0, max_seq                           # 16-byte V loads / LDS-DMA chunks of a transposed cache row
    assert H % nh == 0 and n_rep >= 1 and H % n_rep == 0 and n_rep % nh == 0, (H, n_rep, nh)   # a workgroup's heads share ONE kv head
    assert can_pair or not pair, kernel
    ntl = -(-M // rt)
    return ((ntl + 1) // 2 if pair else ntl, H // nh), threads


def _bf(x):
    return mo.to_bf16(np.asarray(x, np.float32))


@functools.lru_cache(maxsize=None)
def _pool(hd, H, KV, max_seq):
    """the random material of the probes of one shape, drawn once: queries, context keys / values, and N(0, 30) for behind S"""
    rng = np.random.default_rng([hd, H, KV, max_seq])
    return (_bf(rng.normal(0, 1, (max_seq, H, hd))), _bf(rng.normal(0, 0.4, (KV, max_seq, hd))), _bf(rng.normal(0, 0.5, (KV, hd, max_seq))),
            _bf(rng.normal(0, 30, (KV, max_seq, hd))), _bf(rng.normal(0, 30, (KV, hd, max_seq))))


def mask_probe(hd, H, KV, max_seq, start, M):
    """Q [M][H][hd], K [KV][max_seq][hd], V^T [KV][hd][max_seq] (bf16 bits) of a chunk of M rows at slots [start, start + M):
    K = 0 in the chunk's slots (every visible score is exactly 0, every exp exactly 1), V[key][d] = 1.0 where key % hd == d;
    the context slots in front hold ordinary keys and values (one let in changes bits), the slots behind hold N(0, 30)"""
    S = start + M
    assert S <= max_seq
    q, k_ctx, v_ctx, k_big, v_big = _pool(hd, H, KV, max_seq)
    kc, vt = np.zeros((KV, max_seq, hd), np.uint16), np.zeros((KV, hd, max_seq), np.uint16)
    kc[:, :start], vt[:, :, :start] = k_ctx[:, :start], v_ctx[:, :, :start]
    kc[:, S:], vt[:, :, S:] = k_big[:, S:], v_big[:, :, S:]
    keys = np.arange(start, S)
    vt[:, keys % hd, keys] = 0x3F80
    return q[:M].copy(), kc, vt


@functools.lru_cache(maxsize=None)
def mask_expected(hd, M, S, window):
    """[M][hd] bf16 bits (read-only), the same for every head: row r with n visible keys, c_d of them congruent to d, gives
    out[d] = T(T(1 / n) c_d) -- the row sum n is exact, p = T(exp(0) (1 / n)) with the fp32 quotient, and c_d <= 14 copies of an
    8-bit value add up exactly in fp32 in any order"""
    lo, hi = visible(np.arange(M), M, S, window)
    d = np.arange(hd)
    c = (hi[:, None] - d) // hd - (lo[:, None] - 1 - d) // hd       # keys of [lo, hi] congruent to d
    p = mo.from_bf16(_bf(np.float32(1.0) / (hi - lo + 1).astype(np.float32)))
    out = _bf(p[:, None] * c.astype(np.float32))
    out.setflags(write=False)
    return out
