// make_default_sampler's two launches, planned without a device: ONE definition for the decoder's own sampler (decoder.cc) and the pick of a
// batch (batch_plan.h plan_head).  Pure arithmetic over kernels/abi.h constants, no HIP.
#pragma once

#include <algorithm>
#include <cstdint>
#include <string>

#include "kernels/abi.h"

namespace mcimpl {

// Over a row of `vocab` logits (sampler_kernels.hip): the candidate lists come from chunks of 512 logits (1024 / 2048 where that would be
// more than MC_SAMPLE_LISTS_MAX lists), each sorted by ONE wave in registers, kpad = top_k rounded up to a power of two keys per list; the
// second launch finds the k best of the sorted lists.  Fills the second launch's parameters and the chunk of the first (its grid is
// p->nlists); "" = fine, else the refusal (MC_ERR_RUNTIME) where the row is too long for the second.
constexpr const char* SAMPLER_ROW_TOO_LONG = "sampler: the fused sampler handles rows of up to 2048 * 1024 logits";
inline std::string
sampler_plan(int top_k, int vocab, float inv_temp_T, float top_p_T, mc::abi::sampler_params* p, uint32_t* chunk)
{
    using namespace mc::abi;
    uint32_t kpad = 1;
    while (kpad < (uint32_t)top_k) kpad *= 2;
    const uint32_t k = (uint32_t)std::min(top_k, vocab);
    *chunk = std::max(512u, kpad);
    while (*chunk < 2048u && ((uint32_t)vocab + *chunk - 1) / *chunk > MC_SAMPLE_LISTS_MAX) *chunk *= 2;
    const uint32_t lists = ((uint32_t)vocab + *chunk - 1) / *chunk;
    if (lists > MC_SAMPLE_LISTS_MAX) return SAMPLER_ROW_TOO_LONG;
    *p = sampler_params{k, lists * kpad, SAMPLE_CAP, inv_temp_T, top_p_T, lists, kpad};
    return "";
}

} // namespace mcimpl
