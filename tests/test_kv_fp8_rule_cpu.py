"""The fp8 KV cache rule (tests/kv_fp8_rule.py; include/metalchat_hip.h Part 2o) on its own: deq is a bfloat16, e sits where the
format's maximum puts it, and the bytes are torch's e4m3fn conversion of the scaled values."""
import numpy as np
import pytest

import kv_fp8_rule as kr


def bf16_bits(v):
    """exact float values -> bfloat16 bits (asserts that nothing is lost)"""
    v = np.asarray(v, np.float32)
    bits = v.view(np.uint32)
    assert np.all((bits & 0xFFFF) == 0)
    return (bits >> 16).astype(np.uint16)


def test_deq_is_a_normal_bfloat16_or_zero_for_every_byte_and_exponent():
    table = kr.e4m3_table()
    ok = ~np.isnan(table)
    assert ok.sum() == 254
    for e in range(kr.E_MIN, kr.E_MAX + 1):
        v64 = np.ldexp(table[ok], e)
        v32 = v64.astype(np.float32)
        assert np.all(v32.astype(np.float64) == v64), e
        assert np.all((v32.view(np.uint32) & 0xFFFF) == 0), f"e {e}: more than 8 significant bits"
        mag = np.abs(v64[v64 != 0])
        assert mag.min() >= 2.0 ** -126 and np.all(np.isfinite(v32)), f"e {e}: a subnormal or an overflow"
        bits = kr.deq(np.arange(256, dtype=np.uint8)[ok], np.int8(e))
        assert np.all(kr.from_bf16(bits).astype(np.float64) == v64), e


@pytest.mark.parametrize("k", [-120, -109, -108, -30, 0, 7, 110, 111, 118])
def test_exponent_at_the_edges(k):
    edge = np.float32(448.0 * 2.0 ** k)                      # amax exactly 448 2^k: e = k
    at = bf16_bits([edge])[0]
    below, above = at - 1, at + 1                             # one bfloat16 step (positive values: the bits are ordered)
    clip = lambda e: min(max(e, kr.E_MIN), kr.E_MAX)
    for bits, e in ((at, k), (below, k), (above, k + 1)):
        x = np.zeros(64, np.uint16)
        x[5] = bits | 0x8000                                  # the amax may be negative
        x[9] = bf16_bits([edge / 4])[0]
        b, got = kr.quant(x)
        assert int(got) == clip(e), (k, hex(bits))
        if clip(e) == e:
            scaled = np.abs(kr.from_bf16(x).astype(np.float64)) * 2.0 ** -e
            assert scaled.max() <= 448 < 2 * scaled.max()     # the smallest such e
        assert not np.any((b & 0x7F) == 0x7F), "a finite vector never makes a NaN byte"
    assert int(kr.quant(np.zeros(64, np.uint16))[1]) == kr.E_MIN
    assert np.all(kr.quant(np.array([0x8000, 0], np.uint16))[0] == [0x80, 0])


def test_bytes_are_torchs_e4m3fn_conversion():
    torch = pytest.importorskip("torch")
    if not hasattr(torch, "float8_e4m3fn"):
        pytest.skip("this torch has no float8_e4m3fn")
    rng = np.random.default_rng(8)
    table = kr.e4m3_table()
    grid = np.sort(table[~np.isnan(table)])
    ties = (grid[:-1] + grid[1:]) / 2                         # every midpoint of two neighbours (exact in float32)
    y = np.concatenate([rng.normal(0, 1, 4000) * np.exp2(rng.integers(-12, 9, 4000)), ties, grid, [448.0, -448.0, 2.0 ** -10, -2.0 ** -10]])
    y = np.clip(y, -448, 448).astype(np.float32)
    ref = torch.from_numpy(y).to(torch.float8_e4m3fn).view(torch.uint8).numpy()
    got = kr.e4m3_bytes(y.astype(np.float64))
    zero = (ref & 0x7F) == 0                                  # (the sign of a zero result: the rule keeps the value's)
    assert np.array_equal(got[~zero], ref[~zero])
    assert np.all((got[zero] & 0x7F) == 0)
    # and through quant(): the bytes of a vector are the conversion of x 2^-e
    xf = (rng.normal(0, 1, (64, 128)) * np.exp2(rng.integers(-20, 20, (64, 1)))).astype(np.float32)
    x = (xf.view(np.uint32) >> 16).astype(np.uint16)      # (truncated to bfloat16)
    b, e = kr.quant(x)
    scaled = np.ldexp(kr.from_bf16(x), -e.astype(np.int32)[:, None]).astype(np.float32)
    ref = torch.from_numpy(scaled).to(torch.float8_e4m3fn).view(torch.uint8).numpy()
    assert np.array_equal(b[(ref & 0x7F) != 0], ref[(ref & 0x7F) != 0])
