// Part 2b of include/metalchat_hip.h: batched decode -- B sequences in lockstep over one decoder's weights (B <= 8 from
// mc_batch_create, B <= 64 from Part 2h's mc_wide_batch_create, which since Part 2i also admits QLoRA decoders: int4 / int8 linears in
// groups of 32, each linear in a format of its own, LoRA adaptors on the layer linears).
//
// The reference's layers carry the batch dimension already: nn::attention::operator() takes input[bs, len, dim]
// (include/metalchat/nn/attention.h:163-206) and nn::sink_cache holds [max_batch_size, max_seq_len, n_kv_heads, head_dim],
// writing cache[0:bs, start_pos:start_pos+len] at ONE start_pos for the whole batch (nn/cache.h:154-215); only nn::llama3 pins
// max_batch_size = 1 (nn/llama.h:86).  A batch here shares the decoder's weights (read through decoder_batch.h, never copied)
// and owns B caches per layer.  Per token and layer it enqueues a fixed sequence of launches (batch_kernels.hip), none of which
// waits for another workgroup:
//   rmsnorm, wq|wk|wv, rope + cache write, scores, softmax + P.V, Wo + residual, rmsnorm, w1|w3 + SiLU.mul, w2 + residual
// then the final norm, the head and the pick (greedy, or the decoder's default sampler) per row.  Every GEMV streams each
// weight once for all B rows: plan_batch_gemv() (batch_plan.h) picks the launch by B, and nothing else knows where that line runs.
// Part 2c (mc_ragged_*) runs the same sequence with every row at a position of its own: the per-row launches read rows[r]
// instead of the shared state, one small launch (mc_b_rows_begin) starts each step in place of mc_step_set, and a row whose
// position is -1, or which stopped on a stop id or at the end of its cache, is idle.
// Part 2j (mc_rolling_set): the ragged rows of a batch decode past max_seq_len on nn::sink_cache's ring (nn/cache.h:187-204).
// A row's ring state is a function of its position -- rows get past the end by single steps only -- so the batch keeps its lengths
// and nothing else: mc_b_rows_begin_rolling derives the state and writes the row's rope row, every other launch is the ragged one.
// Part 2k (mc_row_sampler_*): a row slot may pick with settings of its own in place of the decoder's; plan_head() resolves every row's
// effective sampler and keeps the uniform launches wherever the rows agree.
// Part 2l (mc_row_mask_*, mc_row_penalty_*, mc_row_logits_reset): a row slot may carry a token mask and repetition / frequency /
// presence penalties; the plan then puts ONE launch (logit_kernels.hip) between the head GEMV and the pick, which rewrites the logits
// of those rows in place.  A batch on which no row has either launches what it launched before.
// Part 2m (mc_settings_verify_set): opt-in per batch, the two verify calls take rows that sample or carry a mask or penalties;
// the head of the call then runs process -> pick -> accept -> count over the packed rows (plan_verify_pick, plan_verify_logits).
// Part 2n (mc_logprobs_set): opt-in per batch, two launches (logprob_kernels.hip) behind every pick -- a token's three forms and a verify call's --
// record the pick's log-probability and the top_n most likely tokens.  With the switch off a batch launches and holds what it did before.
//
// WHAT is launched -- names, grids, blocks, LDS bytes, the admission and every check of a call that needs no device -- is decided in
// batch_plan.h, and IN WHICH ORDER in batch_call_plan.h: an entry point plans its whole call once (plan_batch_token, plan_rows_tail,
// plan_verify_call), prepare() reserves and uploads what the plan names in front of the first launch, and run() -- one switch over the op tag, the
// only place that packs a batch launch's arguments -- executes the list (the n tokens of a generate call: the same list n times).  Both headers are
// without HIP.  This header is struct mc_batch as its four units see it: the state, the allocator, the launch path and the small helpers every
// unit calls inline.  Which unit defines what:
//   batch.cc           creation and release, prepare and run, the log-probability records, the lockstep and ragged entry points
//   batch_rows.cc      the rows passes: rows_pass (check, tables, plan, prepare, prompt pass, run, read back) behind mc_rows_prefill /
//                      mc_extend_rows / mc_verify_rows / mc_tree_verify
//   batch_cache.cc     a row's cache: fork, import, the exports, mc_rolling_*
//   batch_settings.cc  what a row slot carries between calls: seeds, row samplers, row logit processors; the log-probability switch and mc_logprobs_get
#pragma once

#include "bf16_host.h"
#include "batch_call_plan.h"
#include "decoder_batch.h"

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstring>
#include <memory>

namespace mcimpl {

// Part 2n: the log-probability records of a call on the device -- tok [slots], ids / top [slots][top_n] -- with their capacities in slots
struct logprob_records {
    float *tok = nullptr, *top = nullptr;
    int32_t* ids = nullptr;
    int tok_cap = 0, top_cap = 0, ids_cap = 0;
    int count = 0; // of the last call with records: its n (a step, generate or packed call) or its packed rows (a verify call); 0: none yet
    // mc_logprobs_set: what an earlier setting recorded is gone; the records are laid out by top_n, so another one reserves them anew
    void
    forget(bool layout_changed)
    {
        if (layout_changed) ids_cap = top_cap = 0;
        count = 0;
    }
};

// mc_verify_rows and mc_tree_verify, all reserved at the first call that needs it: the normed rows [128][dim], their logits [128][vocab], and the
// call's results on the device: accepted[B], next_tokens[B], picks[M], then (mc_tree_verify) paths[B][MC_VERIFY_MAX_LEN]; with row settings
// (Part 2m) the per-packed-row table and the candidate keys [MC_VERIFY_MAX_ROWS][cand_per_row]; with log-probabilities a record per packed row
struct verify_state {
    void *xn = nullptr, *logits = nullptr;
    int32_t* out = nullptr;
    int xn_cap = 0, logits_cap = 0, out_cap = 0;
    int rows = 0; // packed rows of the last mc_verify_rows / mc_tree_verify call (0: none yet)
    std::vector<int32_t> host;
    verify_row* tab = nullptr;
    std::vector<verify_row> tab_sent;
    int tab_cap = 0;
    uint64_t* cand = nullptr;
    int cand_cap = 0; // (packed rows)
    logprob_records records;
};

// what changes between the launches of one plan: the lockstep position and the advance word of a token; of a verify call the packed rows behind
// the last layer, the call's ids and (a tree) its node table, all on the device
struct call_args {
    const batch_call_plan& plan;
    int pos = 0;
    bool advance = false;
    const void* xrows = nullptr;
    const int32_t* ids = nullptr;
    const tv_node* nodes = nullptr;
};

} // namespace mcimpl

struct mc_batch {
    mcimpl::decoder_parts p;
    mc_decoder* d = nullptr;
    int B = 0;
    size_t cache_elems = 0; // one row's cache of one layer: n_kv * max_seq * hd
    std::vector<void*> allocs;
    void *kc = nullptr, *vt = nullptr;    // [layer][B][n_kv][max_seq][hd], [layer][B][n_kv][hd][max_seq]
    void *x = nullptr, *xn = nullptr;     // [B][dim]
    void *qkv = nullptr;                  // [B][(H + 2 KV) hd]
    void *q = nullptr, *att = nullptr;    // [B][H hd]
    void *gate = nullptr;                 // [B][ffn]
    void *lora_vec = nullptr;             // [B][lora_ld]: a = T(A x) of the linear in flight; only when some linear has an adaptor.  ONE
                                          // scratch for all linears: every launch goes to the decoder's one stream, in order
    int lora_ld = 0;                      // the most lora_cols of any linear
    void *logits = nullptr;               // [B][vocab]
    float *expv = nullptr, *psum = nullptr; // [B][H][max_seq], [B][H][fx.nsplit]
    float *fcos = nullptr, *fsin = nullptr; // rope table rows [0, max_seq)
    float *rcos = nullptr, *rsin = nullptr; // [B][hd / 2]: a rolling batch's rope row of each row, written by every step's first launch
    bool rolling = false;                   // mc_rolling_set
    mcimpl::step_state* st = nullptr;     // the shared position
    mcimpl::step_state* rows = nullptr;   // [B]: token and step_index of each row (ragged calls: the whole state of each row)
    uint64_t* cand = nullptr;             // [B][fx.cand_per_row]
    uint64_t* seeds = nullptr;
    int n_seed_pairs = 0, seed_cap = 0;   // (capacity in pairs)
    int32_t* tokens_dev = nullptr;
    int tokens_cap = 0;
    std::vector<mcimpl::step_state> rows_host;
    std::vector<int32_t> lengths;         // [B]: valid cache positions of each row
    int32_t* stop_dev = nullptr;          // the stop ids of a ragged call
    int stop_cap = 0;
    std::vector<int32_t> stop_host;
    char* pp_tab = nullptr;               // a packed prompt pass (mc_rows_prefill): pp_seg[MC_WIDE_BATCH_MAX], then the pp_tile table,
                                          // then (mc_tree_verify) one tv_node per packed row
    int pp_tab_cap = 0;                   // (bytes)
    std::vector<char> pp_host;            // the same bytes on the host: one upload
    mcimpl::px_range* px_tab = nullptr;   // mc_extend_rows: the range table
    int px_tab_cap = 0;
    std::vector<mcimpl::px_range> px_host;
    std::vector<mcimpl::px_group> px_groups;
    float *px_sums = nullptr, *px_part = nullptr; // scratch of one launch group: [px_slots][H][16], [px_slots][H][16][hd]
    int px_slots = 0;
    // mc_verify_rows and mc_tree_verify (verify_state above); Part 2m's switch (mc_settings_verify_set): the two calls take sampling, masked and
    // penalised rows
    mcimpl::verify_state vs;
    bool verify_settings_on = false;
    // Part 2k: the sampler of each row slot as mc_row_sampler_set took it, the table of effective settings the mixed launches read
    // (plan_head resolves it), and what of it the device holds
    std::vector<mcimpl::row_setting> row_samplers; // [B]
    mcimpl::row_sampler* samplers_dev = nullptr;   // [B]
    std::vector<mcimpl::row_sampler> samplers_sent;
    // Part 2l: the logit processor of each row slot as the caller set it, and what of the table plan_logits resolves from it the
    // device holds.  The mask words [B][mask_words()] (and their copy on the host), the counts [B][vocab] and the table are
    // allocated at the first call that needs them: a batch that uses neither holds what it held
    std::vector<mcimpl::row_logit_setting> row_logit_set; // [B]
    uint32_t* masks_dev = nullptr;
    std::vector<uint32_t> masks_host;
    int32_t* counts_dev = nullptr;
    mcimpl::row_logits* logits_tab_dev = nullptr;
    std::vector<mcimpl::row_logits> logits_tab_sent;
    // Part 2n (mc_logprobs_set): with the switch on, two launches behind every pick record the pick's log-probability and the top_n most
    // likely tokens (plan_logprobs): `records` beside tokens_dev and indexed like it, vs.records per packed row of a verify call; the parts and chunk keys
    // of the launches in flight.  All reserved at the first call that needs them: a batch that never asks holds what it held
    bool logprobs_on = false;
    int logprobs_top = 0;
    mcimpl::logprob_records records;         // count: n of the last step, generate or packed call with records
    mcimpl::logprob_part* lp_parts = nullptr;
    uint64_t* lp_keys = nullptr;
    int lp_parts_cap = 0, lp_keys_cap = 0; // (rows)
    // The plans fixed at creation (batch_call_plan.h batch_fixed): B, the device's compute units and MC_WB_TILES, both read once there; the GEMV
    // of every matrix; the launches of a step, lockstep / ragged / ragged on a rolling batch.  The plan of a call is the entry point's own
    // (plan_batch_token, plan_rows_tail, plan_verify_call with settings()) and goes down by const&: the settings cannot change inside a call
    mcimpl::batch_fixed fx;

    ~mc_batch()
    {
        (void)hipSetDevice(p.ordinal);
        (void)hipStreamSynchronize(p.stream);
        for (void* a : allocs) (void)hipFree(a);
    }

    template <typename P> mc_status
    alloc(P** ptr, size_t bytes)
    {
        void* v = nullptr;
        hipError_t e = hipMalloc(&v, bytes ? bytes : 16);
        if (e != hipSuccess)
            return mcimpl::fail(MC_ERR_ALLOC, std::string("hardware_memory_allocator: failed to allocate ") + std::to_string(bytes) +
                                                  " bytes: " + hipGetErrorString(e));
        allocs.push_back(v);
        MC_HIP(hipMemsetAsync(v, 0, bytes ? bytes : 16, p.stream));
        *ptr = static_cast<P*>(v);
        return MC_OK;
    }
    void
    free_one(void* v)
    {
        auto it = std::find(allocs.begin(), allocs.end(), v);
        if (it != allocs.end()) allocs.erase(it);
        (void)hipFree(v);
    }
    // a buffer that only grows: `need` elements of `elem` bytes fit in `have`, or the stream drains and a zeroed buffer of `cap`
    // elements takes its place (nothing in flight reads the old one then)
    template <typename P> mc_status
    reserve(P*& ptr, int& have, int need, int cap, size_t elem = sizeof(P))
    {
        if (need <= have) return MC_OK;
        MC_HIP(hipStreamSynchronize(p.stream));
        if (ptr) free_one(ptr);
        ptr = nullptr;
        have = 0;
        mc_status s = alloc(&ptr, elem * (size_t)cap);
        if (s != MC_OK) return s;
        have = cap;
        return MC_OK;
    }
    // a buffer made at the first call that needs it (the stream drains behind the allocation: the synchronous copies of the mc_row_*
    // calls must find its zeros in place)
    template <typename P> mc_status
    ensure(P*& ptr, size_t bytes)
    {
        if (ptr) return MC_OK;
        MC_HIP(hipSetDevice(p.ordinal));
        mc_status s = alloc(&ptr, bytes);
        if (s != MC_OK) return s;
        MC_HIP(hipStreamSynchronize(p.stream));
        return MC_OK;
    }
    // a per-row table goes up when it differs from what the device holds: once per call, and every call drains the stream before it
    // returns, so `sent` is not touched while a copy reads it
    template <typename T> mc_status
    send_if_changed(T* dev, std::vector<T>& sent, const std::vector<T>& now)
    {
        if (sent.size() == now.size() && memcmp(sent.data(), now.data(), sizeof(T) * now.size()) == 0) return MC_OK;
        sent = now;
        MC_HIP(hipMemcpyAsync(dev, sent.data(), sizeof(T) * sent.size(), hipMemcpyHostToDevice, p.stream));
        return MC_OK;
    }

    mc_status
    launch(const std::string& name, unsigned gx, unsigned gy, unsigned gz, unsigned bx, unsigned lds, mcimpl::arg_pack&& a)
    {
        return mcimpl::decoder_launch(d, name, gx, gy, gz, bx, lds, std::move(a));
    }
    mc_status
    launch(const mcimpl::launch_plan& l, mcimpl::arg_pack&& a)
    {
        return mcimpl::decoder_launch(d, l.name, l.gx, l.gy, l.gz, l.block, l.lds, std::move(a));
    }

    int mask_words() const { return (p.cfg.vocab + 31) / 32; }
    char* kc_of(int layer, int row) const { return (char*)kc + ((size_t)layer * B + row) * cache_elems * 2; }
    char* vt_of(int layer, int row) const { return (char*)vt + ((size_t)layer * B + row) * cache_elems * 2; }
    mc_status ensure_tokens(int n) { return reserve(tokens_dev, tokens_cap, n * B, n * B); }

    // the shared step state at position `pos` (slot = pos: a batch's cache never turns)
    mc_status
    set_pos(int pos)
    {
        return launch(fx.steps[0].begin, mcimpl::pack(st, (int32_t)-1, (int32_t)pos, (int32_t)p.cfg.max_seq_len, (int32_t)p.pre_len, (int32_t)0, (int32_t)1));
    }

    mcimpl::call_settings
    settings() const
    {
        return {rolling, verify_settings_on, logprobs_on, logprobs_top, n_seed_pairs, mcimpl::decoder_sampler_of(d), row_samplers, row_logit_set};
    }

    // ---------------------------------------------------------------- one call (batch.cc)
    // everything of a planned call in front of its first launch: its refusal, the n x B tokens, the log-probability records and scratch, the
    // packed rows' buffers of a verify call, the tables sent
    mc_status prepare(const mcimpl::batch_call_plan& c, int n);
    // ONE launch of the plan: the op's arguments bound (the only place that packs them), and the list from front to back
    mc_status run(const mcimpl::batch_launch& l, const mcimpl::call_args& a);
    mc_status gemv(const mcimpl::launch_plan& l, bool adaptor, const mcimpl::batch_linear& L, const void* xin, void* y, uint32_t ldy);
    mc_status run_all(const mcimpl::call_args& a);
    // Part 2n: `slots` records, reserved and filled with 0xFF (a slot no pick reaches reads as NaN bits, id -1); the records copied out
    mc_status begin_records(mcimpl::logprob_records& r, int slots, int cap);
    mc_status copy_records(const mcimpl::logprob_records& r, size_t slots, float* tok, int32_t* ids, float* top);
};

namespace mcimpl {

// fail() for a refusal of batch_plan.h ("" = none)
inline mc_status
refuse(const std::string& why, mc_status code = MC_ERR_INVALID_ARGUMENT)
{
    return why.empty() ? MC_OK : fail(code, why);
}

// the batch, row and (with_layer) layer of the call `who`: one check, the caller's name in front of its text
inline mc_status
find_row(const mc_batch* b, const char* who, int32_t row, bool with_layer = false, int32_t layer = 0)
{
    return refuse(check_row(who, b ? b->B : -1, row, b && with_layer ? (int)b->p.layers.size() : -1, layer));
}

} // namespace mcimpl
