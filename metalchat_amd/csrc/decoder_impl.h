// The decoder behind Part 2 of include/metalchat_hip.h, as its five translation units see it: the fused weights (linear_w, layer_w), the
// greedy pick's descriptors (pick_block) and struct mc_decoder -- its state, the small helpers every unit calls inline, and the
// declarations of everything else.  Which unit defines what:
//   decoder.cc         the per-token decode -- it launches what token_plan.h plans, step by step -- the hand-off fall-back, the C ABI of a step
//   weights.cc         allocation and upload of the fused matrices, the synthetic model
//   prefill.cc         the prompt pass (run_prefill): it launches what prefill_plan.h plans -- GEMM family, attention, rope form, folds; no HIP there
//   prefill_blaslt.cc  the library GEMM of long prompts -- the only unit that sees hipBLASLt's header
//   pipeline.cc        the layer pipeline (RCCL / local); it holds decoders, it is not part of one
// The batch's units (batch_impl.h) do not include this header: they read a decoder through decoder_batch.h.  Six headers beside the units need no
// device and are pinned on the CPU by plain g++ programs (tests/cpp): gemv_plan.h (the decode GEMV), block_plan.h (the decode attention block),
// token_plan.h (the whole decode token), prefill_plan.h (the prompt pass), rows_plan.h (the admission and the tables of the batch's rows passes) and batch_plan.h (what a batch launches);
// sampler_plan.h plans the default sampler's two launches for the decoder and the batch alike.
#pragma once

#include "backend_impl.h"
#include "bf16_host.h" // f2bf_host / bf2f_host
#include "decoder_batch.h"
#include "sampler_plan.h" // the two launches of the default sampler
#include "gemv_plan.h" // decoder_options / read_options (decoder_options.h) and plan_gemv
#include "block_plan.h" // plan_block: form, kernel and grid of the decode attention block
#include "token_plan.h" // plan_token: every launch of one decode token, in order, on symbolic operands
#include "prefill_plan.h" // plan_gemm, plan_attention, plan_rope and the fold predicates of the prompt pass

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <string>
#include <unordered_map>
#include <vector>

struct blaslt_state; // prefill_blaslt.cc

namespace mcimpl {

// more kernel arguments behind a pack() whose head depends on the form of a launch
template <typename... A> inline void
push_all(arg_pack& p, const A&... a)
{
    (p.push(a), ...);
}

struct linear_w {
    int fmt = MC_WFMT_T;
    int out = 0, in = 0, group = 0; // group 0 = one scale per row
    void* w = nullptr;
    void* scales = nullptr;
    size_t w_bytes = 0, s_bytes = 0;
    size_t row_bytes = 0;
    int ngroups = 1;
    bool allocated = false;
    std::vector<uint8_t> scales_host; // shadow of the quad-interleaved scale buffer (load path only)
    void* wq2 = nullptr;      // int4: the quad-interleaved copy short prompts multiply from (prefill_kernels.hip mc_pf2_*), built on demand
    uint64_t wq2_gen = 0;     // ... from the weights of this generation (mc_decoder::weights_gen)
    void* wd = nullptr;       // int4 / int8: the dequantised bfloat16 copy [out][in] long prompts multiply by in the library GEMM (gemm_lib), built on demand
    uint64_t wd_gen = 0;
    // quantization::lora_adaptor(s) of the matrices fused here (quantization/lora.h:17-53): the A
    // matrices stacked [nseg*rank][in] (a T-format GEMV of its own), B in fused row order
    // [out][nseg*rank] with zeros outside each row's own adaptor columns, a = T(A x) in lora_vec
    std::unique_ptr<linear_w> lora_a;
    void* lora_b = nullptr;
    std::vector<uint8_t> lora_b_host; // load path only
    void* lora_vec = nullptr;
    int lora_rank = 0;      // rank of one adaptor
    int lora_cols = 0;      // nseg * rank
    float lora_scale = 0.0f;
};

// EPI_STORE_PICK's two descriptors (kernels/gemv.h) and the words the first points at, as they lie in mc_decoder::pick_desc
struct pick_block {
    pick_epilogue atomic;   // key + ticket: the last workgroup of the head's launch finishes the pick
    pick_epilogue per_wg;   // one key per workgroup (pick_keys), no ticket: folded by mc_argmax_keys behind the launch
    unsigned long long key; // 0 between launches
    uint32_t ticket;
};

struct layer_w {
    linear_w qkv, wo, w13, w2;
    void* qkv_epi = nullptr; // device qkv_epilogue
    void* pn_attn = nullptr; // device postnorm_args: attention post-norm, residual = layer input, h_out = hidden_b
    void* pn_ffn = nullptr;  // device postnorm_args: ffn post-norm, residual = hidden_b, h_out = hidden
    void* attention_norm = nullptr;
    void* ffn_norm = nullptr;
    void* q_norm = nullptr;
    void* k_norm = nullptr;
    void* attention_post_norm = nullptr;
    void* ffn_post_norm = nullptr;
    void* kc = nullptr;
    void* vt = nullptr;
    int rope_table = 0;
};

inline int
bit_width(uint32_t v)
{
    int n = 0;
    while (v) {
        n++;
        v >>= 1;
    }
    return n;
}

// (weights.cc)
size_t linear_bytes(const linear_w& L);
// (decoder.cc) the owned layer of a global layer index; is every weight of the stage loaded (and gemma3's post-norm descriptors made)?
mc_status find_layer(mc_decoder* d, int32_t layer, layer_w** out);
mc_status check_ready(mc_decoder* d);
// (prefill_blaslt.cc) the end of mc_decoder::blas
void blaslt_release(blaslt_state* st);

} // namespace mcimpl

using namespace mcimpl;

struct mc_decoder {
    mc_decoder_config cfg;
    decoder_options opt; // the MC_* switches, read once (read_options)
    mc_device* dev = nullptr;
    mc_library* lib = nullptr;
    mc_queue* q = nullptr;
    hipStream_t stream = nullptr;
    int tb = 2; // sizeof(T)
    int pre_len = 0;
    int nsplit = 1;
    int n_own = 0;
    bool first_stage = true, last_stage = true;
    std::string tname; // "bfloat" / "float"

    std::map<std::string, hipFunction_t> fns;
    std::vector<layer_w> layers;
    // embedding
    int emb_fmt = MC_WFMT_T;
    void* emb_table = nullptr;
    float* emb_scales = nullptr;
    linear_w output;
    void* final_norm = nullptr;

    // arena
    void* hidden = nullptr;     // T[dim]   running hidden row (h)
    void* hidden_in = nullptr;  // T[dim]   inbound row for non-first stages
    void* hidden_b = nullptr;   // T[dim]   gemma3: the row between the attention and the ffn half of a block
    uint64_t weights_gen = 1;  // bumped whenever weight rows change: the derived copies (linear_w::wq2) are rebuilt
    bool pf_plain_on = false;  // ... resolved when the first long prompt arrives (plain_copy_ok)
    bool pf_plain_known = false;
    bool pf_lib_on = false;    // opt.pf_lib until the library fails (gemm_lib)
    struct blaslt_state* blas = nullptr; // the library's handle, workspace and per-shape plans: made by gemm_lib on first use (prefill_blaslt.cc)
    int lt_calls = 0; // library multiplications issued (mc_decoder_launch_log names them "hipblasLtMatmul")
    bool lazy_pick = false;    // inside mc_decoder_generate: the pick of a token is folded by the NEXT token's embedding launch
    bool graph_lazy = false;   // the captured token was recorded with lazy_pick
    std::unordered_map<const void*, postnorm_args> pn_host; // the same descriptors on the host (the linear-order kernels take the three pointers as arguments)
    void* qkv = nullptr;        // T[(H+2KV)*hd]
    void* q_rot = nullptr;      // T[H*hd]
    void* attn_out = nullptr;   // T[H*hd]
    void* proj = nullptr;       // T[dim]   (gemma: pre-post-norm outputs)
    void* gate = nullptr;       // T[ffn]
    void* logits = nullptr;     // T[vocab]
    float* expv = nullptr;      // [H][max_seq]
    float* psum = nullptr;      // [H][nsplit]
    float* pv_parts = nullptr;  // [pv_ranges][H*hd] fp32 partial P.V sums (long contexts)
    int pv_ranges = 1;
    // decode attention in one launch (mc_attn_fused_bfloat): {value, tag} granules of its two in-launch hand-offs
    unsigned long long* attn_psum_g = nullptr; // [H][nsplit]            partial softmax denominators
    unsigned long long* attn_slab_g = nullptr; // [KV][nsplit][n_rep][hd] fp32 partial P.V sums
    unsigned long long* attn_row_g = nullptr;  // [H * hd / 2]          the finished attention row, two bf16 per granule (mc_attn_wo_*)
    unsigned long long* attn_hid_g = nullptr;  // [dim / 2]             the hidden row behind Wo, for the w1|w3 phase of mc_attn_qkv_wo_w13_w_* (hand-off D)
    unsigned long long* attn_qkv_g = nullptr;  // [KV][(n_rep + 2) hd / 2] the step's rotated queries and K / V row, two bf16 per granule (mc_attn_qkv_wo_*)
    // ---- what happens when an in-launch hand-off gives up (its workgroups were not resident together: another stream or process
    // holds part of the chip).  The launch sets state.err and completes; the host then LATCHES the decoder onto the launches
    // that need no co-residency (attn_fused_on = false: scores, P.V and the GEMVs as launches of their own), drops the captured
    // graph and -- where the step can be repeated exactly -- runs it again (mc_decoder_step; mc_decoder_generate while the
    // ring has not turned inside the call).  handoff_fallbacks counts those events (mc_decoder_handoff_fallbacks).
    step_state* state_bak = nullptr; // the step state in front of the call that may have to be repeated
    uint32_t* err_host = nullptr;      // pinned: state.err of a step nobody waited for (a non-last stage, next_token == NULL)
    hipEvent_t err_evt = nullptr;
    bool err_pending = false;
    int handoff_fallbacks = 0;
    // ... and the fall-back is TEMPORARY (round 6): one transient stall (another stream holding CUs for 50 ms, a profiler pass) must not cost every
    // later token the one-launch blocks.  After `rearm_after` tokens without a hand-off launch the decoder takes them again (mc_decoder_handoff_rearms counts);
    // every further fall-back doubles the distance (a chip that is shared for good settles on the launches that need no co-residency), MC_HANDOFF_REARM=0: never
    int rearm_after = 256, clean_tokens = 0, handoff_rearms = 0;
    void
    note_clean_tokens(int n)
    {
        if (attn_fused_on || !opt.attn_fused || rearm_after <= 0) return;
        clean_tokens += n;
        if (clean_tokens < rearm_after) return;
        attn_fused_on = true;
        clean_tokens = 0;
        handoff_rearms++;
        drop_graph(); // (captured with the launches that need no co-residency)
    }
    bool attn_fused_on = true;   // opt.attn_fused, until a hand-off gives up (handoff_failed) and again after rearm_after clean tokens (note_clean_tokens)
    void* taps = nullptr;       // T[(n_own+1)*dim]
    step_state* state = nullptr;
    int32_t* tokens_dev = nullptr;
    // the greedy pick inside the output head's launch (gemv.h EPI_STORE_PICK): two descriptors {key*, ticket*, state*, tokens_out*}
    // -- [0, 32) with the atomic key at [64, 72) and the ticket at [72, 76), both zero between launches; [32, 64) with pick_keys
    // and no ticket
    char* pick_desc = nullptr;
    unsigned long long* pick_keys = nullptr; // MC_HEAD_PICK=2: one key per workgroup of the head's launch, folded by mc_argmax_keys
    static constexpr unsigned pick_slots = 1024;
    int tokens_cap = 0;
    // sampler (nn/sampling.h:303-313); kind 0 = greedy argmax, 1 = topk -> nucleus -> multinomial
    int sampler_kind = MC_SAMPLER_GREEDY;
    int top_k = 50;
    float inv_temp_T = 0.0f, top_p_T = 0.0f;
    uint64_t* cand = nullptr;      // [chunks][kpad] candidate keys
    uint64_t* seeds = nullptr;     // [n_seed_pairs][2]
    int n_seed_pairs = 0, seed_cap = 0;
    float* sampler_taps = nullptr; // [7][128]
    // prompt pass (prefill_kernels.hip): row buffers for up to pf_cap rows
    int pf_cap = 0;
    size_t pf_probs_elems = 0;
    void *pf_x = nullptr, *pf_xn = nullptr, *pf_h = nullptr, *pf_proj = nullptr, *pf_qkv = nullptr,
         *pf_q = nullptr, *pf_att = nullptr, *pf_g2 = nullptr, *pf_g = nullptr, *pf_probs = nullptr;
    int32_t* pf_tokens = nullptr;
    float* pf_etab = nullptr; // exp_precise of every bfloat16 value (prefill_kernels.hip mc_exp_table_bfloat), 256 KiB
    float* pf_gtab = nullptr; // gemma: T(gelu) of every bfloat16 value (mc_gelu_table_bfloat), 256 KiB; MC_PF_GELU_TABLE=0: none (the fp64 tanh per element)
    void* pf_lora = nullptr;
    size_t pf_lora_elems = 0;
    float* pf_part = nullptr; // split-K partial sums [splits][M][N]
    size_t pf_part_elems = 0;
    bool ring_turned = false;
    void *rot_k = nullptr, *rot_v = nullptr; // scratch of mc_kv_rotate (one layer's K and Vt)
    hipEvent_t pf_e0 = nullptr, pf_e1 = nullptr;
    std::map<std::string, double> pf_ms;

    template <typename F> mc_status
    timed(const char* cat, F&& f)
    {
        if (!opt.pf_timing) return f();
        if (!pf_e0) {
            MC_HIP(hipEventCreate(&pf_e0));
            MC_HIP(hipEventCreate(&pf_e1));
        }
        MC_HIP(hipEventRecord(pf_e0, stream));
        mc_status s = f();
        if (s != MC_OK) return s;
        MC_HIP(hipEventRecord(pf_e1, stream));
        MC_HIP(hipEventSynchronize(pf_e1));
        float ms = 0.0f;
        MC_HIP(hipEventElapsedTime(&ms, pf_e0, pf_e1));
        pf_ms[cat] += ms;
        return MC_OK;
    }
    float* rope_cos[2] = {nullptr, nullptr};
    float* rope_sin[2] = {nullptr, nullptr};
    int rope_rows = 0;
    int rope_start = 0;
    bool rope_valid = false;
    int last_pos = -1;
    bool want_taps = false;

    hipGraph_t graph = nullptr;
    hipGraphExec_t graph_exec = nullptr;

    std::vector<void*> allocs;
    bool pn_ready = false;
    // test / measurement aids: the names of the kernels launched eagerly since the log was switched on (a replayed graph
    // launches what was logged when it was captured)
    bool log_on = false;
    std::vector<std::string> launch_log;

    ~mc_decoder();

    mc_status
    alloc(void** p, size_t bytes, bool zero = true)
    {
        hipError_t e = hipMalloc(p, bytes ? bytes : 16);
        if (e != hipSuccess)
            return fail(MC_ERR_ALLOC, std::string("hardware_memory_allocator: failed to allocate ") +
                                          std::to_string(bytes) + " bytes: " + hipGetErrorString(e));
        allocs.push_back(*p);
        if (zero) {
            // complete before alloc returns: callers fill some of these buffers with synchronous copies on the null
            // stream, which is not ordered against this (non-blocking, or adopted) stream
            MC_HIP(hipMemsetAsync(*p, 0, bytes ? bytes : 16, stream));
            MC_HIP(hipStreamSynchronize(stream));
        }
        return MC_OK;
    }

    // give a buffer of the arena back (the caller has synchronised the stream)
    void
    release(void** p)
    {
        if (!*p) return;
        auto it = std::find(allocs.begin(), allocs.end(), *p);
        if (it != allocs.end()) allocs.erase(it);
        (void)hipFree(*p);
        *p = nullptr;
    }

    void
    drop_graph()
    {
        if (graph_exec) (void)hipGraphExecDestroy(graph_exec);
        if (graph) (void)hipGraphDestroy(graph);
        graph_exec = nullptr;
        graph = nullptr;
    }

    mc_status
    fn(const std::string& name, hipFunction_t* out)
    {
        auto it = fns.find(name);
        if (it != fns.end()) {
            *out = it->second;
            return MC_OK;
        }
        hipFunction_t f = nullptr;
        hipError_t e = hipModuleGetFunction(&f, lib->module, name.c_str());
        if (e != hipSuccess || !f)
            return fail(MC_ERR_INVALID_ARGUMENT, "hardware_accelerator: function " + name +
                                                     " not found in a shader library");
        fns[name] = f;
        *out = f;
        return MC_OK;
    }

    mc_status
    launch(const std::string& name, unsigned gx, unsigned gy, unsigned gz, unsigned bx, unsigned lds,
           arg_pack&& a)
    {
        hipFunction_t f;
        mc_status s = fn(name, &f);
        if (s != MC_OK) return s;
        size_t n = a.buf.size();
        void* extra[] = {HIP_LAUNCH_PARAM_BUFFER_POINTER, a.buf.data(), HIP_LAUNCH_PARAM_BUFFER_SIZE,
                         &n, HIP_LAUNCH_PARAM_END};
        mcimpl::launch_range range(name.c_str(), gx, gy, gz, bx, 1, 1);
        if (log_on) launch_log.push_back(name);
        hipError_t e = hipModuleLaunchKernel(f, gx, gy, gz, bx, 1, 1, lds, stream, nullptr, extra);
        if (e != hipSuccess) return hip_fail(e, name.c_str());
        return MC_OK;
    }

    // ---------------------------------------------------------------- weights (weights.cc)
    size_t row_bytes(int fmt, int in) const;
    mc_status alloc_linear(linear_w& L, int fmt, int out, int in, int group);
    mc_status upload_rows(linear_w& L, int dst_row0, int dst_stride, int rows, const void* weight, const float* scales, int perm_hd = 0);

    // ---------------------------------------------------------------- launches
    // Which kernel a decode GEMV takes is decided in gemv_plan.h (plan_gemv), what the attention block launches in block_plan.h (plan_block), the
    // token's whole sequence in token_plan.h (plan_token): all over this view of the decoder -- benv.g is the GEMV's part of it -- fixed at create time but for the occupancy answers (query_occupancy).
    block_env benv{};
    static gemv_shape
    shape_of(const linear_w& L) { return {L.fmt, L.out, L.in, L.group, L.lora_cols}; }
    block_model
    model() const { return {(int)cfg.family, cfg.n_heads, cfg.n_kv_heads, cfg.head_dim, cfg.dim, cfg.max_seq_len}; }
    // (in front of a stage's first block no post-norm is pending; a later block's flag is a value of the token's plan -- token_plan.h)
    block_state
    block_now() const { return {attn_fused_on, false}; }
    block_plan
    plan_block(const layer_w& L) const { return ::plan_block({shape_of(L.qkv), shape_of(L.wo), shape_of(L.w13)}, model(), benv, block_now()); }
    // may a hand-off of the next launches give up?  (the step in front of them is then kept for the retry)
    bool
    uses_handoffs() const { return block_uses_handoffs(model(), benv, block_now()); }
    // (decoder.cc, like every member declared from here to run_token)
    void query_occupancy();
    void handoff_failed();

    // ---------------------------------------------------------------- the hand-off reporting and the per-token decode (decoder.cc)
    mc_status check_handoffs(const step_state& st);
    mc_status report_handoff(uint32_t code);
    mc_status check_err_synced();
    mc_status poll_pending_err();
    void note_err_async();
    mc_status gemv(const linear_w& L, int pro, int epi, const void* x, void* y, const void* res, const void* norm_w, float mu);
    mc_status gemv_launch(const linear_w& L, const std::string& name, unsigned wgs, unsigned block, unsigned lds, bool pn_by_value, const void* x, void* y,
                          const void* res, const void* norm_w, float mu);
    mc_status ensure_rope(int pos, int len = 1);
    // what plan_token (token_plan.h) sees of this decoder, and of this moment
    token_fixed token_fixed_now() const;
    token_state
    token_now(bool advance, bool in_hidden) const { return {attn_fused_on, want_taps, sampler_kind, lazy_pick, advance, in_hidden}; }
    mc_status fold_pick();
    mc_status attn_launch(const layer_w& L, const block_plan& P, const void* x, void* y, const void* res, const void* pn);
    mc_status run_step(const token_plan& P, const token_step& s, const void* in);
    mc_status run_head();
    mc_status run_token(const void* hidden_src, bool advance = false);

    // ---------------------------------------------------------------- prompt pass (prefill.cc; gemm_lib: prefill_blaslt.cc)
    // what the prompt pass launches is decided in prefill_plan.h, over this view of the decoder; the members here touch the device
    prefill_env
    penv() const
    {
        return {tb, (int)cfg.qmode, (int)cfg.family, (unsigned)dev->prop.multiProcessorCount, cfg.dim, cfg.ffn_dim, cfg.n_heads, cfg.n_kv_heads, cfg.head_dim,
                cfg.max_seq_len, pf_lib_on, &opt};
    }
    gemm_plan
    plan_gemm(const linear_w& L, int M, int epi) const { return ::plan_gemm(shape_of(L), penv(), M, epi); }
    mc_status grow(void** p, size_t* have, size_t need, size_t elem_bytes);
    mc_status ensure_prefill(int M, int S);
    mc_status ensure_pf2(const linear_w& Lc);
    bool plain_copy_ok();
    mc_status ensure_wd(const linear_w& Lc, const void** wd);
    bool gemm_lib(const linear_w& L, const void* X, void* Y, int M, bool f32_out);
    // One plan, one launch per family, one reduce.  epi 2 stops at the partial sums in pf_part ([splits][M][out]); the answer's `splits`
    // is then how many the consumer adds up, 0 when this matrix at this M leaves none (nothing was launched: the caller takes gemm()).
    struct gemm_done {
        mc_status st;
        unsigned splits;
    };
    gemm_done gemm_run(const linear_w& L, int epi, const void* X, void* Y, const void* res, int M);
    gemm_done gemm_to_parts(const linear_w& L, const void* X, int M);
    mc_status gemm(const linear_w& L, int epi, const void* X, void* Y, const void* res, int M);
    mc_status norm_rows(const void* x, const void* w, const void* res, void* y, int M, float mu);
    mc_status qkv_rope_cache(const layer_w& L, void* kc, void* vt, int M, int start_pos, int rope_pos, float mu, const packed_prefill* pk);
    mc_status gemm_residual(const linear_w& W, const void* X, const void* res, void* out, const void* post_w, const void* next_w, const char* label, int M, float mu, bool* xn_done);
    mc_status run_prefill(int M, int cache_pos, int rope_pos, int window, const void* rows_in, const packed_prefill* pk = nullptr);
};
