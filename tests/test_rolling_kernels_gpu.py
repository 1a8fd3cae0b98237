"""Kernel-level test of rolling rows (mc_b_rows_begin_rolling, metalchat_amd/csrc/kernels/batch_kernels.hip), the kernel launched BY
NAME on buffers the test owns:

  * the rope row it writes for a row at position p is, bit for bit, the row mc_rope_table writes with start_pos = p -- positions 0, 1,
    S - 1, S, S + 57, 3 S and 100000, head_dim 64 and 128;
  * the state it derives is rolling_rule.state(p); an idle row's state and rope row are not touched;
  * advance: the row moves on by one position and its step_index by B; a row whose token is a stop id turns idle and nothing else
    of it is written; no row stops for the end of its cache."""
import numpy as np
import pytest

import rolling_rule as rr

pytestmark = pytest.mark.gpu
THETA = 500000.0
WORDS = 12   # step_state: token, pos, kv_len, write_slot, ring_base, step_index, rope_row, rolled, rope_start, epoch, err, pad
TOKEN, POS, KV_LEN, WRITE_SLOT, RING_BASE, STEP_INDEX, ROPE_ROW = range(7)


def table_row(acc, hd, p):
    """mc_rope_table's one row at start_pos = p"""
    import metalchat_amd as mc

    half = hd // 2
    cb, sb = acc.alloc(half * 4), acc.alloc(half * 4)
    mc.KernelTask(acc.load("mc_rope_table"), ((half + 63) // 64 * 64, 1, 1), (64, 1, 1),
                  [cb, sb, np.uint32(1), np.uint32(hd), np.uint32(p), np.float32(THETA)])()
    acc.wait()
    return cb.download(np.float32, half), sb.download(np.float32, half)


def rows_begin(acc, rows, S, hd, advance, stop=()):
    """one launch over `rows` ([B][12] int32); returns (rows afterwards, rcos, rsin), the rope rows NaN where nothing was written"""
    import metalchat_amd as mc

    B, half = rows.shape[0], hd // 2
    rb = acc.to_device(rows)
    cb, sb = acc.to_device(np.full((B, half), np.nan, np.float32)), acc.to_device(np.full((B, half), np.nan, np.float32))
    stopb = acc.to_device(np.asarray(stop, np.int32)) if len(stop) else None
    i32 = np.int32
    mc.KernelTask(acc.load("mc_b_rows_begin_rolling"), (B * 64, 1, 1), (64, 1, 1),
                  [rb, stopb, i32(len(stop)), i32(S), i32(rr.pre_len(S)), i32(advance), cb, sb, np.uint32(hd), np.float32(THETA)])()
    acc.wait()
    return (rb.download(np.int32, B * WORDS).reshape(B, WORDS), cb.download(np.float32, B * half).reshape(B, half),
            sb.download(np.float32, B * half).reshape(B, half))


def fresh_rows(positions, tokens):
    rows = np.zeros((len(positions), WORDS), np.int32)
    rows[:, 2:] = -7   # what the kernel must derive or leave alone
    rows[:, POS], rows[:, TOKEN], rows[:, STEP_INDEX] = positions, tokens, np.arange(len(positions))
    return rows


@pytest.mark.parametrize("hd,S", [(128, 64), (64, 64), (128, 256)])
def test_rope_rows_are_the_tables_rows_and_the_state_follows_the_position(acc, hd, S):
    positions = [0, 1, S - 1, S, -1, S + 57, 3 * S, 100000]   # -1: idle
    B = len(positions)
    rows0 = fresh_rows(positions, 100 + np.arange(B))
    rows, rcos, rsin = rows_begin(acc, rows0, S, hd, advance=0)
    for r, p in enumerate(positions):
        if p < 0:
            assert np.array_equal(rows[r], rows0[r]), "an idle row's state is not touched"
            assert np.isnan(rcos[r]).all() and np.isnan(rsin[r]).all(), "an idle row's rope row is not written"
            continue
        tc, ts = table_row(acc, hd, p)
        assert np.array_equal(rcos[r].view(np.uint32), tc.view(np.uint32)), (hd, S, p, "cos")
        assert np.array_equal(rsin[r].view(np.uint32), ts.view(np.uint32)), (hd, S, p, "sin")
        ring_base, write_slot, kv_len = rr.state(p, S)
        want = rows0[r].copy()
        want[[KV_LEN, WRITE_SLOT, RING_BASE, ROPE_ROW]] = kv_len, write_slot, ring_base, r
        assert np.array_equal(rows[r], want), (hd, S, p, rows[r], want)


@pytest.mark.parametrize("hd,S", [(128, 64), (64, 256)])
def test_advance_moves_a_row_on_and_a_stop_id_turns_it_idle(acc, hd, S):
    before = [0, S - 2, S - 1, -1, S + 56, 3 * S - 1, 99999, 17]   # one step later: the positions of the test above, and 18
    B = len(before)
    tokens = 100 + np.arange(B)
    stop = [999, int(tokens[-1])]                                  # the last row's previous pick is a stop id
    rows0 = fresh_rows(before, tokens)
    rows, rcos, rsin = rows_begin(acc, rows0, S, hd, advance=1, stop=stop)
    for r, q in enumerate(before):
        if q < 0:
            assert np.array_equal(rows[r], rows0[r]) and np.isnan(rcos[r]).all() and np.isnan(rsin[r]).all()
            continue
        want = rows0[r].copy()
        if tokens[r] in stop:
            want[POS] = -1
            assert np.array_equal(rows[r], want), (r, rows[r], want)
            assert np.isnan(rcos[r]).all() and np.isnan(rsin[r]).all(), "a stopped row's rope row is not written"
            continue
        p = q + 1                                                  # S - 1 -> S: no stop for the end of the cache
        ring_base, write_slot, kv_len = rr.state(p, S)
        want[[POS, KV_LEN, WRITE_SLOT, RING_BASE, STEP_INDEX, ROPE_ROW]] = p, kv_len, write_slot, ring_base, r + B, r
        assert np.array_equal(rows[r], want), (hd, S, p, rows[r], want)
        tc, ts = table_row(acc, hd, p)
        assert np.array_equal(rcos[r].view(np.uint32), tc.view(np.uint32)), (hd, S, p, "cos")
        assert np.array_equal(rsin[r].view(np.uint32), ts.view(np.uint32)), (hd, S, p, "sin")
