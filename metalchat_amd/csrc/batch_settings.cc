// What a batch's row slots carry between calls (the map of the whole: batch_impl.h): the seeds, the row samplers (Part 2k), the row logit
// processors (Part 2l) and the batch's log-probability switch with its records (Part 2n).  The calls store what the caller set; plan_head / plan_logits (batch_plan.h) resolve it at the next step.
// Every batch call drains the stream before it returns, so the synchronous copies below meet an idle stream.
#include "batch_impl.h"

using namespace mcimpl;

namespace {

mc_status
ensure_masks(mc_batch* b)
{
    b->masks_host.resize((size_t)b->B * b->mask_words(), 0u);
    return b->ensure(b->masks_dev, sizeof(uint32_t) * b->B * b->mask_words());
}

mc_status
ensure_counts(mc_batch* b)
{
    return b->ensure(b->counts_dev, sizeof(int32_t) * (size_t)b->B * b->p.cfg.vocab);
}

} // namespace

extern "C" {

mc_status
mc_batch_set_seeds(mc_batch* b, const uint64_t* seeds, int32_t n_pairs)
{
    if (!b || (n_pairs > 0 && !seeds) || n_pairs < 0) return fail(MC_ERR_INVALID_ARGUMENT, "mc_batch_set_seeds: bad argument");
    MC_HIP(hipSetDevice(b->p.ordinal));
    mc_status s = b->reserve(b->seeds, b->seed_cap, n_pairs, n_pairs, 2 * sizeof(uint64_t));
    if (s != MC_OK) return s;
    if (n_pairs > 0) {
        MC_HIP(hipStreamSynchronize(b->p.stream));
        MC_HIP(hipMemcpy(b->seeds, seeds, sizeof(uint64_t) * 2 * n_pairs, hipMemcpyHostToDevice));
    }
    b->n_seed_pairs = n_pairs;
    return MC_OK;
}

// ---- Part 2k: row samplers ----

mc_status
mc_row_sampler_set(mc_batch* b, int32_t row, int32_t kind, int32_t top_k, float temperature, float top_p)
{
    if (mc_status s = find_row(b, "mc_row_sampler_set", row); s != MC_OK) return s;
    if (kind != MC_SAMPLER_INHERIT && kind != MC_SAMPLER_GREEDY && kind != MC_SAMPLER_DEFAULT && kind != MC_SAMPLER_DRAW)
        return fail(MC_ERR_INVALID_ARGUMENT, "mc_row_sampler_set: unknown sampler");
    row_setting rs;
    if (kind == MC_SAMPLER_DEFAULT || kind == MC_SAMPLER_DRAW) {
        // mc_decoder_set_sampler's checks and texts (nn/sampling.h:165-174), and its rounding (a batch is bfloat16)
        if (!(temperature > 0.0f)) return fail(MC_ERR_INVALID_ARGUMENT, "nucleus_sampler: temperature must be positive");
        if (top_p < 0.0f || top_p > 1.0f) return fail(MC_ERR_INVALID_ARGUMENT, "nucleus_sampler: probability must be in [0.0, 1.0]");
        if (top_k < 1 || top_k > 128) return fail(MC_ERR_INVALID_ARGUMENT, "topk_sampler: the fused sampler keeps 1..128 candidates");
        rs.inv_temp_T = round_bf_host(1.0f / round_bf_host(temperature)); // T temp = T(1) / _M_temperature  (sampling.h:190)
        rs.top_p_T = round_bf_host(top_p);
    }
    rs.kind = kind;
    rs.top_k = top_k;
    rs.temperature = temperature;
    rs.top_p = top_p;
    b->row_samplers[row] = rs;
    return MC_OK;
}

mc_status
mc_row_sampler_get(const mc_batch* b, int32_t row, int32_t* kind, int32_t* top_k, float* temperature, float* top_p)
{
    if (!b || !kind) return fail(MC_ERR_INVALID_ARGUMENT, "mc_row_sampler_get: null argument");
    if (mc_status s = find_row(b, "mc_row_sampler_get", row); s != MC_OK) return s;
    const row_setting& rs = b->row_samplers[row];
    *kind = rs.kind;
    if (rs.kind == MC_SAMPLER_INHERIT) return MC_OK;
    if (top_k) *top_k = rs.top_k;
    if (temperature) *temperature = rs.temperature;
    if (top_p) *top_p = rs.top_p;
    return MC_OK;
}

mc_status
mc_row_sampler_reset(mc_batch* b)
{
    if (!b) return fail(MC_ERR_INVALID_ARGUMENT, "mc_row_sampler_reset: null argument");
    b->row_samplers.assign(b->B, row_setting{});
    return MC_OK;
}

// ---- Part 2l: row logit processors ----

mc_status
mc_row_mask_set(mc_batch* b, int32_t row, const uint32_t* allowed, int32_t n_words)
{
    if (mc_status s = find_row(b, "mc_row_mask_set", row); s != MC_OK) return s;
    if (!allowed) {
        b->row_logit_set[row].masked = false;
        return MC_OK;
    }
    const int nw = b->mask_words(), vocab = b->p.cfg.vocab;
    if (n_words != nw) return fail(MC_ERR_INVALID_ARGUMENT, "mc_row_mask_set: n_words must be (vocab + 31) / 32 = " + std::to_string(nw));
    // bits at and above vocab are ignored: the device's words hold zeros there
    std::vector<uint32_t> words(allowed, allowed + nw);
    if (vocab % 32) words[nw - 1] &= (1u << (vocab % 32)) - 1u;
    if (std::all_of(words.begin(), words.end(), [](uint32_t w) { return w == 0; }))
        return fail(MC_ERR_INVALID_ARGUMENT, "mc_row_mask_set: the mask allows no token");
    if (mc_status s = ensure_masks(b); s != MC_OK) return s;
    MC_HIP(hipSetDevice(b->p.ordinal));
    MC_HIP(hipMemcpyAsync(b->masks_dev + (size_t)row * nw, words.data(), sizeof(uint32_t) * nw, hipMemcpyHostToDevice, b->p.stream));
    MC_HIP(hipStreamSynchronize(b->p.stream));
    std::copy(words.begin(), words.end(), b->masks_host.begin() + (size_t)row * nw);
    b->row_logit_set[row].masked = true;
    return MC_OK;
}

mc_status
mc_row_mask_get(const mc_batch* b, int32_t row, int32_t* is_set, uint32_t* allowed, int32_t n_words)
{
    if (mc_status s = find_row(b, "mc_row_mask_get", row); s != MC_OK) return s;
    if (!is_set) return fail(MC_ERR_INVALID_ARGUMENT, "mc_row_mask_get: null argument");
    const int nw = b->mask_words();
    if (allowed && n_words != nw) return fail(MC_ERR_INVALID_ARGUMENT, "mc_row_mask_get: n_words must be (vocab + 31) / 32 = " + std::to_string(nw));
    *is_set = b->row_logit_set[row].masked ? 1 : 0;
    if (*is_set && allowed) std::copy_n(b->masks_host.begin() + (size_t)row * nw, nw, allowed);
    return MC_OK;
}

mc_status
mc_row_penalty_set(mc_batch* b, int32_t row, float repetition, float frequency, float presence)
{
    if (mc_status s = find_row(b, "mc_row_penalty_set", row); s != MC_OK) return s;
    if (!std::isfinite(repetition) || !(repetition > 0.0f))
        return fail(MC_ERR_INVALID_ARGUMENT, "mc_row_penalty_set: repetition must be finite and positive");
    if (!std::isfinite(frequency)) return fail(MC_ERR_INVALID_ARGUMENT, "mc_row_penalty_set: frequency must be finite");
    if (!std::isfinite(presence)) return fail(MC_ERR_INVALID_ARGUMENT, "mc_row_penalty_set: presence must be finite");
    if (mc_status s = ensure_counts(b); s != MC_OK) return s;
    row_logit_setting& rs = b->row_logit_set[row];
    rs.rep = repetition;
    rs.freq = frequency;
    rs.pres = presence;
    return MC_OK;
}

mc_status
mc_row_penalty_get(const mc_batch* b, int32_t row, float* repetition, float* frequency, float* presence)
{
    if (mc_status s = find_row(b, "mc_row_penalty_get", row); s != MC_OK) return s;
    const row_logit_setting& rs = b->row_logit_set[row];
    if (repetition) *repetition = rs.rep;
    if (frequency) *frequency = rs.freq;
    if (presence) *presence = rs.pres;
    return MC_OK;
}

mc_status
mc_row_penalty_count(mc_batch* b, int32_t row, const int32_t* tokens, int32_t n)
{
    if (mc_status s = find_row(b, "mc_row_penalty_count", row); s != MC_OK) return s;
    if (n < 0) return fail(MC_ERR_INVALID_ARGUMENT, "mc_row_penalty_count: n must not be negative");
    if (n > 0 && !tokens) return fail(MC_ERR_INVALID_ARGUMENT, "mc_row_penalty_count: null argument");
    const int vocab = b->p.cfg.vocab;
    for (int32_t i = 0; i < n; i++)
        if (tokens[i] < 0 || tokens[i] >= vocab)
            return fail(MC_ERR_INVALID_ARGUMENT, "mc_row_penalty_count: token " + std::to_string(i) + " (id " + std::to_string(tokens[i]) +
                                                     ") is outside the vocabulary");
    if (mc_status s = ensure_counts(b); s != MC_OK) return s;
    if (n == 0) return MC_OK;
    MC_HIP(hipSetDevice(b->p.ordinal));
    std::vector<int32_t> counts(vocab);
    int32_t* dev = b->counts_dev + (size_t)row * vocab;
    MC_HIP(hipMemcpy(counts.data(), dev, sizeof(int32_t) * vocab, hipMemcpyDeviceToHost));
    for (int32_t i = 0; i < n; i++) counts[tokens[i]]++;
    MC_HIP(hipMemcpyAsync(dev, counts.data(), sizeof(int32_t) * vocab, hipMemcpyHostToDevice, b->p.stream));
    MC_HIP(hipStreamSynchronize(b->p.stream));
    return MC_OK;
}

mc_status
mc_row_penalty_counts(mc_batch* b, int32_t row, int32_t* counts)
{
    if (mc_status s = find_row(b, "mc_row_penalty_counts", row); s != MC_OK) return s;
    if (!counts) return fail(MC_ERR_INVALID_ARGUMENT, "mc_row_penalty_counts: null argument");
    const int vocab = b->p.cfg.vocab;
    if (!b->counts_dev) {
        std::fill_n(counts, vocab, 0);
        return MC_OK;
    }
    MC_HIP(hipSetDevice(b->p.ordinal));
    MC_HIP(hipMemcpy(counts, b->counts_dev + (size_t)row * vocab, sizeof(int32_t) * vocab, hipMemcpyDeviceToHost));
    return MC_OK;
}

mc_status
mc_row_penalty_clear(mc_batch* b, int32_t row)
{
    if (mc_status s = find_row(b, "mc_row_penalty_clear", row); s != MC_OK) return s;
    if (!b->counts_dev) return MC_OK;
    MC_HIP(hipSetDevice(b->p.ordinal));
    MC_HIP(hipMemsetAsync(b->counts_dev + (size_t)row * b->p.cfg.vocab, 0, sizeof(int32_t) * b->p.cfg.vocab, b->p.stream));
    MC_HIP(hipStreamSynchronize(b->p.stream));
    return MC_OK;
}

mc_status
mc_row_logits_reset(mc_batch* b)
{
    if (!b) return fail(MC_ERR_INVALID_ARGUMENT, "mc_row_logits_reset: null argument");
    b->row_logit_set.assign(b->B, row_logit_setting{});
    if (!b->counts_dev) return MC_OK;
    MC_HIP(hipSetDevice(b->p.ordinal));
    MC_HIP(hipMemsetAsync(b->counts_dev, 0, sizeof(int32_t) * (size_t)b->B * b->p.cfg.vocab, b->p.stream));
    MC_HIP(hipStreamSynchronize(b->p.stream));
    return MC_OK;
}

// ---- Part 2n: row log-probabilities ----

mc_status
mc_logprobs_set(mc_batch* b, int32_t enable, int32_t top_n)
{
    if (!b) return fail(MC_ERR_INVALID_ARGUMENT, "mc_logprobs_set: null argument");
    if (mc_status s = refuse(check_logprobs(enable, top_n, b->p.cfg.vocab)); s != MC_OK) return s;
    for (logprob_records* r : {&b->records, &b->vs.records}) r->forget(top_n != b->logprobs_top);
    b->logprobs_on = enable == 1;
    b->logprobs_top = top_n;
    return MC_OK;
}

int32_t
mc_logprobs_enabled(const mc_batch* b, int32_t* top_n)
{
    if (!b) return 0;
    if (top_n) *top_n = b->logprobs_top;
    return b->logprobs_on ? 1 : 0;
}

mc_status
mc_logprobs_get(mc_batch* b, int32_t n, float* token_logprobs, int32_t* top_ids, float* top_logprobs)
{
    if (!b || !token_logprobs) return fail(MC_ERR_INVALID_ARGUMENT, "mc_logprobs_get: null argument");
    if (!b->logprobs_on) return fail(MC_ERR_INVALID_ARGUMENT, "mc_logprobs_get: log-probabilities are switched off (mc_logprobs_set)");
    if (!b->records.count) return fail(MC_ERR_INVALID_ARGUMENT, "mc_logprobs_get: no step, generate or packed call with log-probabilities on this batch yet");
    if (n != b->records.count) return fail(MC_ERR_INVALID_ARGUMENT, "mc_logprobs_get: n must be the last call's n = " + std::to_string(b->records.count));
    if (b->logprobs_top == 0 && (top_ids || top_logprobs)) return fail(MC_ERR_INVALID_ARGUMENT, "mc_logprobs_get: top_n is 0, the top arrays must be null");
    return b->copy_records(b->records, (size_t)n * b->B, token_logprobs, top_ids, top_logprobs);
}

} // extern "C"
