// Round-to-nearest-even float -> bfloat16 and back on the host, as the kernels round (a NaN stays one): the ONE definition, for the decoder's
// units (scales, attn_scale, sampler settings) and the batch's.  No HIP.
#pragma once

#include <cstdint>
#include <cstring>

namespace mcimpl {

inline uint16_t
f2bf_host(float f)
{
    uint32_t u;
    memcpy(&u, &f, 4);
    if ((u & 0x7f800000u) == 0x7f800000u && (u & 0x007fffffu)) return (uint16_t)((u >> 16) | 0x40u);
    u += 0x7fffu + ((u >> 16) & 1u);
    return (uint16_t)(u >> 16);
}

inline float
bf2f_host(uint16_t b)
{
    uint32_t u = (uint32_t)b << 16;
    float f;
    memcpy(&f, &u, 4);
    return f;
}

// T(v) for T = bfloat16, as a float
inline float
round_bf_host(float v)
{
    return bf2f_host(f2bf_host(v));
}

} // namespace mcimpl
