// The packet arithmetic of the rmsnorm prologues (kernel/rmsnorm.metal:52-95, y = T((mu + w) * x * rsqrt(mean(x^2) + eps))) -- the one
// definition; four places still carry a written-out copy, listed below.
// A packet is the 16 bytes of the activation row one thread stages: HIP's uint4 (the classic prologue, gemv.h stage_x) or a
// native vector of four dwords (the build-time prologues of the linear-order kernels in gemv.h and of the attention-block
// kernels; why not uint4 there: gemv.h, the int4 linear-order prologue); eight bfloats, or -- classic kernels only -- four floats.
//
// THE ORDER OF ADDITIONS IS PART OF THE CONTRACT.  Every prologue that normalises a row must produce the bits of the stand-alone
// rmsnorm: one sum per packet (elements in order, low half of a dword before its high half), a thread's packets added in the
// order it holds them -- a packet the thread does not have counts as `live(i) ? s1 : 0.0f`, never skipped -- then wave_sum_dpp,
// then the waves' sums in wave order.  The callers own the last three steps; the first is packet_sumsq.
//
// Who uses these, and who still writes the arithmetic out.  Through the helpers: stage_x (all three), the int4 linear-order
// prologue's normalise (gemv.h normalise_l) and the three prologues of attn_block_kernels.hip.  Written out, each with a comment at
// the place: the sum of squares and the normalise of the generic linear-order prologue (gemv.h, LGEN), the sum of squares and the
// T-add of the int4 linear-order prologue (gemv.h sumsq_l and the PRO_POSTNORM branch).  With the helper called there hipcc emits
// different code for those kernels (tools/code_object_diff.py against the build before), so the copies stay until that is understood;
// they must keep the arithmetic and the order above, addition for addition.
#pragma once
// MC_ABL_NORM_NOXWAVE = 1 is an ablation build (wrong numbers, timing only): the rmsnorm prologues of the int4 linear-order kernels
// (gemv.h) and of the attention block multiply one wave's sum of squares by the number of waves instead of exchanging the waves'
// sums through LDS -- what the prologue would cost without that exchange.  The numbers are at its use in gemv.h.
#ifndef MC_ABL_NORM_NOXWAVE
#define MC_ABL_NORM_NOXWAVE 0
#endif

#include "common.h"

#include <type_traits>

namespace mc {
namespace gemv {

template <typename V>
__device__ __forceinline__ V
packet_of(uint32_t a, uint32_t b, uint32_t c, uint32_t d)
{
    if constexpr (std::is_same<V, uint4>::value) return make_uint4(a, b, c, d);
    else return V{a, b, c, d};
}

// sum of squares of the packet's elements
template <typename T, typename V>
__device__ __forceinline__ float
packet_sumsq(const V& v)
{
    const uint32_t vv[4] = {v.x, v.y, v.z, v.w};
    float ss = 0.0f;
#pragma unroll
    for (int i = 0; i < 4; i++) {
        if (T::bytes == 2) {
            const float a = __uint_as_float(vv[i] << 16), b = __uint_as_float(vv[i] & 0xFFFF0000u);
            ss += a * a;
            ss += b * b;
        } else {
            const float a = __uint_as_float(vv[i]);
            ss += a * a;
        }
    }
    return ss;
}

// T((mu + w) * v * inv) per element
template <typename T, typename V>
__device__ __forceinline__ V
packet_normalise(const V& v, const V& wv, float mu, float inv)
{
    const uint32_t vv[4] = {v.x, v.y, v.z, v.w};
    const uint32_t ww[4] = {wv.x, wv.y, wv.z, wv.w};
    uint32_t o[4];
#pragma unroll
    for (int i = 0; i < 4; i++) {
        if (T::bytes == 2) {
            const float a = (mu + __uint_as_float(ww[i] << 16)) * __uint_as_float(vv[i] << 16) * inv;
            const float b = (mu + __uint_as_float(ww[i] & 0xFFFF0000u)) * __uint_as_float(vv[i] & 0xFFFF0000u) * inv;
            o[i] = pack_bf16x2(a, b);
        } else {
            o[i] = __float_as_uint((mu + __uint_as_float(ww[i])) * __uint_as_float(vv[i]) * inv);
        }
    }
    return packet_of<V>(o[0], o[1], o[2], o[3]);
}

// elementwise T(a + b) (the residual add of a block, evaluated in T)
template <typename T, typename V>
__device__ __forceinline__ V
packet_add_T(const V& a, const V& b)
{
    const uint32_t aa[4] = {a.x, a.y, a.z, a.w}, bb[4] = {b.x, b.y, b.z, b.w};
    uint32_t o[4];
#pragma unroll
    for (int i = 0; i < 4; i++) {
        if (T::bytes == 2)
            o[i] = pack_bf16x2(__uint_as_float(aa[i] << 16) + __uint_as_float(bb[i] << 16), __uint_as_float(aa[i] & 0xFFFF0000u) + __uint_as_float(bb[i] & 0xFFFF0000u));
        else
            o[i] = __float_as_uint(__uint_as_float(aa[i]) + __uint_as_float(bb[i]));
    }
    return packet_of<V>(o[0], o[1], o[2], o[3]);
}

} // namespace gemv
} // namespace mc
