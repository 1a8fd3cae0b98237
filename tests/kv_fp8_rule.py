"""The fp8 KV cache format of include/metalchat_hip.h Part 2o, in numpy alone.  For one cache vector x of head_dim bfloat16 values:

    amax    = max |x|                                            (float32)
    e       = the smallest integer with amax 2^-e <= 448, clamped to [E_MIN, E_MAX]; E_MIN for amax = 0
    byte[i] = e4m3(x[i] 2^-e)      OCP e4m3 ("e4m3fn"), nearest, ties to even, saturating at +-448 (reached only where e was clamped at E_MAX)
    deq[i]  = e4m3(byte[i]) 2^e    exactly a normal bfloat16 or a zero

Vectors lie along the LAST axis.  bfloat16 values travel as uint16 bits, as everywhere in the tests."""
import numpy as np

E_MIN, E_MAX = -100, 119
E4M3_MAX = 448.0


def e4m3_table():
    """the float64 value of each of the 256 bytes: sign, 4 exponent bits (bias 7), 3 mantissa bits; 0x7f and 0xff are NaN"""
    b = np.arange(256)
    ex, m = (b >> 3) & 15, b & 7
    v = np.where(ex == 0, m * 2.0 ** -9, (8 + m) * np.exp2(ex.astype(np.float64) - 10))
    v = np.where((b & 0x7F) == 0x7F, np.nan, v)
    return np.where(b & 0x80, -v, v)


def from_bf16(bits):
    return (np.asarray(bits, np.uint16).astype(np.uint32) << 16).view(np.float32)


def exponent(amax):
    """e for amax >= 0 (any shape): frexp gives amax = f 2^x with f in [1/2, 1), and 448 = (7/8) 2^9"""
    amax = np.asarray(amax, np.float64)
    f, x = np.frexp(amax)
    e = x - 9 + (f > 0.875)
    return np.clip(np.where(amax == 0, E_MIN, e), E_MIN, E_MAX).astype(np.int8)


def e4m3_bytes(y):
    """float64 y -> bytes: |y| saturated at 448, rounded to the format's grid (steps of 2^-9 below 2^-6, else 8 steps a binade) to
    nearest, ties to even -- np.rint on the exact quotient --, the sign kept (a negative that rounds to zero is 0x80)"""
    y = np.asarray(y, np.float64)
    a = np.minimum(np.abs(y), E4M3_MAX)
    _, x = np.frexp(a)                                   # a in [2^(x-1), 2^x)
    q = np.maximum(x - 1, -6) - 3                        # the grid's step is 2^q
    n = np.rint(np.ldexp(a, -q)).astype(np.int64)        # a / 2^q is exact; n <= 16 (16: the next binade's first value)
    ex = np.where(n >= 8, q + 3 + 7, 0)                  # biased exponent; n < 8 only on the subnormal grid
    code = np.where(n >= 16, (ex + 1) << 3, np.where(n >= 8, (ex << 3) | (n - 8), n))
    return (code | np.where(np.signbit(y), 0x80, 0)).astype(np.uint8)


def quant(x_bits):
    """bfloat16 bits [..., hd] -> (bytes uint8 [..., hd], e int8 [...])"""
    x = from_bf16(x_bits).astype(np.float64)
    e = exponent(np.max(np.abs(x), axis=-1))
    return e4m3_bytes(np.ldexp(x, -e.astype(np.int64)[..., None])), e


def deq(bytes_, e):
    """(bytes [..., hd], e [...]) -> bfloat16 bits [..., hd]; exact, so the float32 bits' upper half"""
    v = np.ldexp(e4m3_table()[np.asarray(bytes_, np.uint8)], np.asarray(e, np.int64)[..., None]).astype(np.float32)
    return (v.view(np.uint32) >> 16).astype(np.uint16)


def roundtrip(x_bits):
    return deq(*quant(x_bits))
