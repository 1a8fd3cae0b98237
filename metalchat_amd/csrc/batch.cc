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
// weight once for all B rows: mc_batch::gemv() picks the launch by B, and nothing else here knows where that line runs.
// Part 2c (mc_ragged_*) runs the same sequence with every row at a position of its own: the per-row launches read rows[r]
// instead of the shared state, one small launch (mc_b_rows_begin) starts each step in place of mc_step_set, and a row whose
// position is -1, or which stopped on a stop id or at the end of its cache, is idle.
// Part 2j (mc_rolling_set): the ragged rows of a batch decode past max_seq_len on nn::sink_cache's ring (nn/cache.h:187-204).
// A row's ring state is a function of its position -- rows get past the end by single steps only -- so the batch keeps its lengths
// and nothing else: mc_b_rows_begin_rolling derives the state and writes the row's rope row, every other launch is the ragged one.
// Part 2k (mc_row_sampler_*): a row slot may pick with settings of its own in place of the decoder's; head() resolves every row's
// effective sampler and keeps the uniform launches wherever the rows agree.
// Part 2l (mc_row_mask_*, mc_row_penalty_*, mc_row_logits_reset): a row slot may carry a token mask and repetition / frequency /
// presence penalties; head() then puts ONE launch (logit_kernels.hip) between the head GEMV and the pick, which rewrites the logits
// of those rows in place.  A batch on which no row has either launches what it launched before.
#include "decoder_batch.h"

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstring>
#include <memory>

using namespace mcimpl;

static_assert(ROW_SAMPLER_GREEDY == MC_SAMPLER_GREEDY && ROW_SAMPLER_DEFAULT == MC_SAMPLER_DEFAULT, "row_sampler::kind carries the public kinds");

struct mc_batch {
    mc_decoder* d = nullptr;
    decoder_parts p;
    int B = 0;
    int nsplit = 0;
    int wb_cus = 0;         // compute units of the device, and MC_WB_TILES (0: by wb_tiles' rule), both read once at creation
    int wb_tiles_env = 0;
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
    float *expv = nullptr, *psum = nullptr; // [B][H][max_seq], [B][H][nsplit]
    float *fcos = nullptr, *fsin = nullptr; // rope table rows [0, max_seq)
    float *rcos = nullptr, *rsin = nullptr; // [B][hd / 2]: a rolling batch's rope row of each row, written by every step's first launch
    bool rolling = false;                   // mc_rolling_set
    step_state* st = nullptr;             // the shared position
    step_state* rows = nullptr;           // [B]: token and step_index of each row (ragged calls: the whole state of each row)
    uint64_t* cand = nullptr;             // [B][lists * kpad]
    size_t cand_per_row = 0;
    uint64_t* seeds = nullptr;
    int n_seed_pairs = 0, seed_cap = 0;   // (capacity in pairs)
    int32_t* tokens_dev = nullptr;
    int tokens_cap = 0;
    std::vector<step_state> rows_host;
    std::vector<int32_t> lengths;         // [B]: valid cache positions of each row
    int32_t* stop_dev = nullptr;          // the stop ids of a ragged call
    int stop_cap = 0;
    std::vector<int32_t> stop_host;
    char* pp_tab = nullptr;               // a packed prompt pass (mc_rows_prefill): pp_seg[MC_WIDE_BATCH_MAX], then the pp_tile table,
                                          // then (mc_tree_verify) one tv_node per packed row
    int pp_tab_cap = 0;                   // (bytes)
    std::vector<char> pp_host;            // the same bytes on the host: one upload
    px_range* px_tab = nullptr;           // mc_extend_rows: the range table
    int px_tab_cap = 0;
    std::vector<px_range> px_host;
    std::vector<px_group> px_groups;
    float *px_sums = nullptr, *px_part = nullptr; // scratch of one launch group: [px_slots][H][16], [px_slots][H][16][hd]
    int px_slots = 0;
    // mc_verify_rows and mc_tree_verify, reserved at the first call: the normed rows [128][dim], their logits [128][vocab], and the
    // call's results on the device: accepted[B], next_tokens[B], picks[M], then (mc_tree_verify) paths[B][MC_VERIFY_MAX_LEN]
    void *v_xn = nullptr, *v_logits = nullptr;
    int32_t* v_out = nullptr;
    int v_xn_cap = 0, v_logits_cap = 0, v_out_cap = 0;
    int v_rows = 0;                       // packed rows of the last mc_verify_rows / mc_tree_verify call (0: none yet)
    std::vector<int32_t> v_host;
    // Part 2k: the sampler of each row slot as mc_row_sampler_set took it (the caller's values, and rounded as the decoder rounds its
    // own); the table of effective settings the mixed launches read, and what of it the device holds
    struct row_setting {
        int32_t kind = MC_SAMPLER_INHERIT, top_k = 0;
        float temperature = 0.0f, top_p = 0.0f;
        float inv_temp_T = 0.0f, top_p_T = 0.0f;
    };
    std::vector<row_setting> row_samplers; // [B]
    row_sampler* samplers_dev = nullptr;   // [B]
    std::vector<row_sampler> samplers_host, samplers_sent;
    // Part 2l: the logit processor of each row slot as the caller set it, the table head() resolves from it and what of that the
    // device holds.  The mask words [B][mask_words()] (and their copy on the host), the counts [B][vocab] and the table are
    // allocated at the first call that needs them: a batch that uses neither holds what it held
    struct row_logit_setting {
        bool masked = false;
        float rep = 1.0f, freq = 0.0f, pres = 0.0f;
        bool penalised() const { return !(rep == 1.0f && freq == 0.0f && pres == 0.0f); }
    };
    std::vector<row_logit_setting> row_logit_set; // [B]
    uint32_t* masks_dev = nullptr;
    std::vector<uint32_t> masks_host;
    int32_t* counts_dev = nullptr;
    row_logits* logits_tab_dev = nullptr;
    std::vector<row_logits> logits_tab_host, logits_tab_sent;

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
            return fail(MC_ERR_ALLOC, std::string("hardware_memory_allocator: failed to allocate ") + std::to_string(bytes) +
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

    mc_status
    launch(const std::string& name, unsigned gx, unsigned gy, unsigned gz, unsigned bx, unsigned lds, arg_pack&& a)
    {
        return decoder_launch(d, name, gx, gy, gz, bx, lds, std::move(a));
    }


    int mask_words() const { return (p.cfg.vocab + 31) / 32; }
    // (the stream drains behind the allocation: the synchronous copies of the mc_row_* calls must find its zeros in place)
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
    mc_status ensure_masks()
    {
        masks_host.resize((size_t)B * mask_words(), 0u);
        return ensure(masks_dev, sizeof(uint32_t) * B * mask_words());
    }
    mc_status ensure_counts() { return ensure(counts_dev, sizeof(int32_t) * (size_t)B * p.cfg.vocab); }

    char* kc_of(int layer, int row) const { return (char*)kc + ((size_t)layer * B + row) * cache_elems * 2; }
    char* vt_of(int layer, int row) const { return (char*)vt + ((size_t)layer * B + row) * cache_elems * 2; }

    // the shared step state at position `pos` (slot = pos: a batch's cache never turns)
    mc_status
    set_pos(int pos)
    {
        return launch("mc_step_set", 1, 1, 1, 64, 0,
                      pack(st, (int32_t)-1, (int32_t)pos, (int32_t)p.cfg.max_seq_len, (int32_t)p.pre_len, (int32_t)0, (int32_t)1));
    }

    // 16-row weight tiles per workgroup of mc_wb_gemv_* for the matrix L: the most of 8, 4, 2 that still brings a workgroup to
    // every compute unit, else 1 (measured: DESIGN.md "Wide batches").  MC_WB_TILES is the experiment's handle.  At most 4 for an
    // int8 matrix or one with an adaptor: those kernels run 8 tiles as two passes of 4 (wide_kernels.hip), which only fetches x twice.
    int
    wb_tiles(const batch_linear& L) const
    {
        const int most = L.fmt == MC_WFMT_I8 || L.lora ? 4 : 8;
        if (wb_tiles_env) return std::min(wb_tiles_env, most);
        for (int t = most; t > 1; t /= 2)
            if ((L.out / 16 + t - 1) / t >= wb_cus) return t;
        return 1;
    }

    static const char* fmt_name(int fmt) { return fmt == MC_WFMT_I4 ? "i4" : (fmt == MC_WFMT_I8 ? "i8" : "w"); }

    // y[r] = epi(W x[r]) for the B rows.  The ONE place that chooses a launch: the format from L.fmt; up to 16 rows are the columns of
    // mc_b_gemv_*'s single MFMA tile (it masks with m < B), more go through mc_wb_gemv_*, whose rows carry the same bits
    // (wide_kernels.hip); a linear with an adaptor takes two launches -- a = T(A x) for all rows, an ordinary T-format GEMV over the
    // stacked A into lora_vec, then the main launch in its _l form, which adds T(T(B a) scale) in front of its epilogue
    mc_status
    gemv(const batch_linear& L, int epi, const void* xin, void* y, uint32_t ldy)
    {
        if (L.lora) {
            batch_linear A; // plain T, no scales and no adaptor of its own: the recursion ends after this one level
            A.out = L.lora_cols;
            A.in = L.in;
            A.w = L.lora_a;
            mc_status s = gemv(A, 0, xin, lora_vec, (uint32_t)lora_ld);
            if (s != MC_OK) return s;
        }
        const std::string tail = std::string(fmt_name(L.fmt)) + "_bfloat_e" + std::to_string(epi) + (L.lora ? "_l" : "");
        const bool wide = B > 16;
        const int tiles = wide ? wb_tiles(L) : 1;
        arg_pack a = wide ? pack(L.w, L.scales, xin, y, (uint32_t)L.in, (uint32_t)L.ngroups, (uint32_t)L.group, (uint32_t)B, (uint32_t)L.out, ldy)
                          : pack(L.w, L.scales, xin, y, (uint32_t)L.in, (uint32_t)L.ngroups, (uint32_t)L.group, (uint32_t)B, ldy);
        if (L.lora) {
            a.push((const void*)lora_vec);
            a.push((uint32_t)lora_ld);
            a.push(L.lora_b);
            a.push((uint32_t)L.lora_cols);
            a.push(L.lora_scale);
        }
        return launch(std::string(wide ? "mc_wb_gemv_" : "mc_b_gemv_") + tail, (unsigned)(L.out / 16 + tiles - 1) / tiles, 1, 1, BG_THREADS, 0,
                      std::move(a));
    }
    mc_status
    rmsnorm(const void* xin, const void* w, void* out)
    {
        return launch("mc_b_rmsnorm_bfloat", 1, B, 1, 1024, 0, pack(xin, w, out, (uint32_t)p.cfg.dim, p.cfg.norm_eps));
    }

    // one lockstep token at `pos` for every row; advance: a chained step (row r's step_index moves by B).
    // ragged: every row at its own rows[r].pos instead, the same launches with the per-row kernels; `pos` is not used, and
    // mc_b_rows_begin starts the step (advance: retires the rows that stopped, moves the others on).
    mc_status
    enqueue_token(int pos, bool advance, bool ragged = false)
    {
        const mc_decoder_config& c = p.cfg;
        const int H = c.n_heads, KV = c.n_kv_heads, hd = c.head_dim, n_rep = H / KV;
        const float scale_T = [&] {
            // T(attn_scale): the scalar_mul of attention.h:196 is evaluated in T
            float f = c.attn_scale;
            uint32_t u;
            memcpy(&u, &f, 4);
            u += 0x7fffu + ((u >> 16) & 1u);
            u &= 0xFFFF0000u;
            memcpy(&f, &u, 4);
            return f;
        }();
        const uint64_t cstride = cache_elems;
        const bool q8 = p.emb_fmt != MC_WFMT_T;
        const void* emb = q8 ? nullptr : p.emb_table;
        const void* emb_q8 = q8 ? p.emb_table : nullptr;
        mc_status s;
        const bool roll = ragged && rolling;
        if (ragged) {
            if (roll)
                s = launch("mc_b_rows_begin_rolling", B, 1, 1, 64, 0,
                           pack(rows, (const int32_t*)stop_dev, (int32_t)stop_host.size(), (int32_t)c.max_seq_len, (int32_t)p.pre_len,
                                (int32_t)(advance ? 1 : 0), rcos, rsin, (uint32_t)hd, c.rope_theta));
            else
                s = launch("mc_b_rows_begin", 1, 1, 1, 64, 0,
                           pack(rows, (const int32_t*)stop_dev, (int32_t)stop_host.size(), (int32_t)c.max_seq_len, (int32_t)B,
                                (int32_t)(advance ? 1 : 0)));
            if (s != MC_OK) return s;
            s = launch("mc_b_embed_rows_bfloat", (c.dim + 255) / 256, B, 1, 256, 0, pack(emb, p.emb_scales, emb_q8, x, rows, (uint32_t)c.dim));
        } else {
            if ((s = set_pos(pos)) != MC_OK) return s;
            s = launch("mc_b_embed_bfloat", (c.dim + 255) / 256, B, 1, 256, 0,
                       pack(emb, p.emb_scales, emb_q8, x, rows, (uint32_t)c.dim, (int32_t)(advance ? 1 : 0), (uint32_t)B));
        }
        if (s != MC_OK) return s;
        // the per-row launches: the lockstep kernel reads the shared state, its _rows form row r's own
        const std::string sfx = ragged ? "_rows_bfloat" : "_bfloat";
        const step_state* state = ragged ? rows : st;
        for (size_t li = 0; li < p.layers.size(); li++) {
            const batch_layer& L = p.layers[li];
            const int l = (int)li;
            if ((s = rmsnorm(x, L.attention_norm, xn)) != MC_OK) return s;
            if ((s = gemv(L.qkv, 0, xn, qkv, (uint32_t)L.qkv.out)) != MC_OK) return s;
            s = launch("mc_b_rope_kv" + sfx, H + 2 * KV, B, 1, hd / 2, 0,
                       pack(qkv, q, (void*)kc_of(l, 0), (void*)vt_of(l, 0), roll ? rcos : fcos, roll ? rsin : fsin, state, (uint32_t)H,
                            (uint32_t)KV, (uint32_t)hd, (uint32_t)c.max_seq_len, cstride));
            if (s != MC_OK) return s;
            s = launch("mc_b_attn_scores" + sfx, nsplit, KV, B, 256, 0,
                       pack(q, (void*)kc_of(l, 0), expv, psum, state, (uint32_t)n_rep, (uint32_t)hd, (uint32_t)c.max_seq_len, scale_T,
                            (uint32_t)nsplit, cstride));
            if (s != MC_OK) return s;
            s = launch("mc_b_attn_pv" + sfx, hd / 16, KV, B, 1024, 0,
                       pack(expv, psum, (void*)vt_of(l, 0), att, state, (uint32_t)n_rep, (uint32_t)hd, (uint32_t)c.max_seq_len,
                            (uint32_t)nsplit, cstride));
            if (s != MC_OK) return s;
            if ((s = gemv(L.wo, 1, att, x, (uint32_t)c.dim)) != MC_OK) return s;
            if ((s = rmsnorm(x, L.ffn_norm, xn)) != MC_OK) return s;
            if ((s = gemv(L.w13, 2, xn, gate, (uint32_t)(L.w13.out / 2))) != MC_OK) return s;
            if ((s = gemv(L.w2, 1, gate, x, (uint32_t)c.dim)) != MC_OK) return s;
        }
        return head(sfx, true);
    }

    // row r's effective sampler: its own (mc_row_sampler_set), or the decoder's while it inherits
    decoder_sampler
    sampler_of_row(int r, const decoder_sampler& dec) const
    {
        const row_setting& rs = row_samplers[r];
        if (rs.kind == MC_SAMPLER_INHERIT) return dec;
        decoder_sampler e;
        e.kind = rs.kind;
        e.top_k = rs.top_k;
        e.inv_temp_T = rs.inv_temp_T;
        e.top_p_T = rs.top_p_T;
        return e;
    }

    // the final norm of x, the head and the pick per row, each row with its effective sampler; sfx "_rows_bfloat": rows whose
    // rows[r].pos is -1 get no pick.  The pick takes the cheapest of three forms, chosen from the settings of ALL B rows (which
    // rows go idle inside a chained call is not known here):
    //   1  no row samples               mc_b_argmax
    //   2  all sample, settings equal   mc_b_topk_candidates_bfloat + mc_b_sample with the plan of those settings
    //   3  anything else                the two mixed launches over the table of effective settings
    // 1 and 2 are what a batch without row samplers launches for the decoder's sampler, argument for argument.
    // Part 2l: with a mask or penalties on any row, mc_b_logits_process_* rewrites those rows' logits between the head and the pick;
    // count: the rows with penalties count their input token first (a step; the packed passes count nothing)
    mc_status
    head(const std::string& sfx, bool count)
    {
        const mc_decoder_config& c = p.cfg;
        mc_status s;
        if ((s = rmsnorm(x, p.final_norm, xn)) != MC_OK) return s;
        if ((s = gemv(p.output, 0, xn, logits, (uint32_t)c.vocab)) != MC_OK) return s;
        if ((s = process_logits(sfx, count)) != MC_OK) return s;
        const decoder_sampler dec = decoder_sampler_of(d);
        const decoder_sampler sm = sampler_of_row(0, dec);
        int sampling = 0, top_k_max = 0;
        bool alike = true;
        samplers_host.resize(B);
        for (int r = 0; r < B; r++) {
            const decoder_sampler e = sampler_of_row(r, dec);
            const bool samples = e.kind != MC_SAMPLER_GREEDY;
            samplers_host[r] = samples ? row_sampler{ROW_SAMPLER_DEFAULT, (uint32_t)std::min(e.top_k, c.vocab), e.inv_temp_T, e.top_p_T}
                                       : row_sampler{ROW_SAMPLER_GREEDY, 0u, 0.0f, 0.0f};
            if (r > 0 && memcmp(&samplers_host[r], &samplers_host[0], sizeof(row_sampler)) != 0) alike = false;
            if (!samples) continue;
            sampling++;
            top_k_max = std::max(top_k_max, e.top_k);
        }
        if (!sampling) return launch("mc_b_argmax" + sfx, 1, B, 1, 1024, 0, pack(logits, (uint32_t)c.vocab, rows, tokens_dev));
        // make_default_sampler per row (sampler_kernels.hip): per-chunk candidates, then one workgroup per row
        const bool mixed = !alike;
        sampler_params sp;
        uint32_t chunk;
        if ((s = sampler_plan(mixed ? top_k_max : sm.top_k, c.vocab, sm.inv_temp_T, sm.top_p_T, &sp, &chunk)) != MC_OK) return s;
        if ((size_t)sp.nlists * sp.kpad > cand_per_row)
            return fail(MC_ERR_RUNTIME, "sampler: the fused sampler handles rows of up to 2048 * 1024 logits");
        if (!mixed) {
            s = launch("mc_b_topk_candidates_bfloat", sp.nlists, B, 1, 64, 0, pack(logits, (uint32_t)c.vocab, sp.kpad, cand, chunk));
            if (s != MC_OK) return s;
            return launch("mc_b_sample" + sfx, 1, B, 1, 128, sp.cap * 8,
                          pack(cand, sp, seeds, (uint32_t)n_seed_pairs, rows, tokens_dev));
        }
        // the table goes up when it differs from what the device holds: once per call (the settings cannot change inside one), and
        // every call drains the stream before it returns, so samplers_sent is not touched while a copy reads it
        if (samplers_sent.size() != samplers_host.size() ||
            memcmp(samplers_sent.data(), samplers_host.data(), sizeof(row_sampler) * B) != 0) {
            samplers_sent = samplers_host;
            MC_HIP(hipMemcpyAsync(samplers_dev, samplers_sent.data(), sizeof(row_sampler) * B, hipMemcpyHostToDevice, p.stream));
        }
        const bool ragged = sfx == "_rows_bfloat";
        s = launch("mc_b_topk_candidates_mixed_bfloat", sp.nlists, B, 1, 64, 0,
                   pack(logits, (uint32_t)c.vocab, sp.kpad, cand, chunk, (const row_sampler*)samplers_dev, (const step_state*)rows,
                        (int32_t)(ragged ? 1 : 0)));
        if (s != MC_OK) return s;
        return launch("mc_b_pick_mixed" + sfx, 1, B, 1, 1024, sp.cap * 8,
                      pack(logits, (uint32_t)c.vocab, (const uint64_t*)cand, (const row_sampler*)samplers_dev, sp.nlists, sp.kpad, sp.cap,
                           (const uint64_t*)seeds, (uint32_t)n_seed_pairs, rows, tokens_dev));
    }

    // the table of the rows' logit processors, resolved as the samplers' is and sent when it differs from what the device holds;
    // no launch (and no table) while no row has anything set
    mc_status
    process_logits(const std::string& sfx, bool count)
    {
        const mc_decoder_config& c = p.cfg;
        bool any = false;
        logits_tab_host.assign(B, row_logits{});
        for (int r = 0; r < B; r++) {
            const row_logit_setting& rs = row_logit_set[r];
            row_logits& t = logits_tab_host[r];
            t.flags = (rs.masked ? ROW_LOGITS_MASK : 0u) | (rs.penalised() ? ROW_LOGITS_PENALTY : 0u);
            if (!t.flags) continue;
            any = true;
            if (!rs.penalised()) continue;
            t.rep = rs.rep;
            t.inv_rep = 1.0f / rs.rep;
            t.freq = rs.freq;
            t.pres = rs.pres;
        }
        if (!any) return MC_OK;
        mc_status s;
        if ((s = ensure(logits_tab_dev, sizeof(row_logits) * B)) != MC_OK) return s;
        if (logits_tab_sent.size() != logits_tab_host.size() ||
            memcmp(logits_tab_sent.data(), logits_tab_host.data(), sizeof(row_logits) * B) != 0) {
            logits_tab_sent = logits_tab_host;
            MC_HIP(hipMemcpyAsync(logits_tab_dev, logits_tab_sent.data(), sizeof(row_logits) * B, hipMemcpyHostToDevice, p.stream));
        }
        const unsigned gx = ((unsigned)c.vocab + LP_CHUNK - 1) / LP_CHUNK;
        arg_pack a = pack(logits, (uint32_t)c.vocab, (const row_logits*)logits_tab_dev, (const uint32_t*)masks_dev, counts_dev, (const step_state*)rows);
        if (sfx == "_rows_bfloat") a.push((int32_t)(count ? 1 : 0));
        return launch("mc_b_logits_process" + sfx, gx, B, 1, LP_THREADS, 0, std::move(a));
    }

    // mc_verify_rows / mc_tree_verify (`who`): a row in the call with a mask or penalties is refused (its chunk rows would each
    // need them)
    mc_status
    verify_logit_rows(const char* who, const int32_t* lens) const
    {
        for (int r = 0; r < B; r++)
            if (lens[r] > 0 && (row_logit_set[r].masked || row_logit_set[r].penalised()))
                return fail(MC_ERR_INVALID_ARGUMENT, std::string(who) + ": row " + std::to_string(r) +
                                                         ": the row has a token mask or penalties (a verify call would need them per chunk row)");
        return MC_OK;
    }

    // mc_verify_rows / mc_tree_verify (`who`): every row in the call must pick greedily.  A batch without row samplers keeps the
    // decoder-wide refusal and its text
    mc_status
    verify_samplers(const char* who, const int32_t* lens) const
    {
        const decoder_sampler dec = decoder_sampler_of(d);
        const bool any_set = std::any_of(row_samplers.begin(), row_samplers.end(), [](const row_setting& r) { return r.kind != MC_SAMPLER_INHERIT; });
        if (!any_set) {
            if (dec.kind == MC_SAMPLER_GREEDY) return MC_OK;
            return fail(MC_ERR_INVALID_ARGUMENT, std::string(who) + ": the decoder's sampler is not greedy (accepting sampled drafts needs the draft's probabilities)");
        }
        for (int r = 0; r < B; r++)
            if (lens[r] > 0 && sampler_of_row(r, dec).kind != MC_SAMPLER_GREEDY)
                return fail(MC_ERR_INVALID_ARGUMENT, std::string(who) + ": row " + std::to_string(r) +
                                                         ": the row's sampler is not greedy (accepting sampled drafts needs the draft's probabilities)");
        return MC_OK;
    }

    // mc_verify_rows: the final norm, the head and a greedy pick for each of the M packed rows `xrows` of a call, then per segment
    // the acceptance of its drafts (`tokens`: the call's ids on the device) and the accepted row's logits into logits[row].
    // nodes (mc_tree_verify): the chunks are trees -- the walk in place of the prefix rule, then the accepted path's K / V
    // moved into place in every layer, both reading the device's own results
    mc_status
    verify_head(const void* xrows, const int32_t* tokens, int M, int nseg, const tv_node* nodes = nullptr)
    {
        const mc_decoder_config& c = p.cfg;
        const batch_linear& L = p.output;
        mc_status s = launch("mc_b_rmsnorm_bfloat", 1, M, 1, 1024, 0, pack(xrows, p.final_norm, v_xn, (uint32_t)c.dim, c.norm_eps));
        if (s != MC_OK) return s;
        s = launch(std::string(L.fmt == MC_WFMT_I8 ? "mc_vhead_" : "mc_v_head_") + fmt_name(L.fmt) + "_bfloat", (unsigned)(L.out / 16 + VH_TILES - 1) / VH_TILES, 1, 1,
                   BG_THREADS, 0,
                   pack(L.w, L.scales, (const void*)v_xn, v_logits, (uint32_t)L.in, (uint32_t)L.ngroups, (uint32_t)L.group, (uint32_t)M,
                        (uint32_t)L.out, (uint32_t)c.vocab));
        if (s != MC_OK) return s;
        int32_t* picks = v_out + 2 * B;
        if ((s = launch("mc_v_argmax_bfloat", 1, M, 1, 1024, 0, pack((const void*)v_logits, (uint32_t)c.vocab, picks))) != MC_OK) return s;
        const unsigned gx = std::min(64u, ((unsigned)c.vocab / 8 + 255) / 256);
        if (!nodes)
            return launch("mc_v_accept", gx, nseg, 1, 256, 0,
                          pack((const pp_seg*)pp_segs(pp_tab), tokens, (const int32_t*)picks, (const void*)v_logits, (uint32_t)c.vocab, v_out, v_out + B,
                               logits));
        int32_t* paths = picks + M;
        s = launch("mc_tv_accept", gx, nseg, 1, 256, 0,
                   pack((const pp_seg*)pp_segs(pp_tab), tokens, nodes, (const int32_t*)picks, (const void*)v_logits, (uint32_t)c.vocab, v_out,
                        v_out + B, paths, logits));
        if (s != MC_OK) return s;
        return launch("mc_tv_compact_bfloat", ((unsigned)(c.n_kv_heads * c.head_dim) + 255) / 256, nseg, (unsigned)p.layers.size(), 256, 0,
                      pack((const pp_seg*)pp_segs(pp_tab), (const int32_t*)v_out, (const int32_t*)paths, kc, vt, (uint64_t)cache_elems,
                           (uint32_t)B, (uint32_t)c.n_kv_heads, (uint32_t)c.head_dim, (uint32_t)c.max_seq_len));
    }

    // rows' tokens and step indices for token 0 of a call (step_index = r: seed pair r % n_pairs, tokens_out[0][r]); a ragged
    // call: their positions too (mc_b_rows_begin derives the rest), an idle row has no token
    mc_status
    start_rows(const int32_t* tokens, const int32_t* positions = nullptr)
    {
        rows_host.assign(B, step_state{});
        for (int r = 0; r < B; r++) {
            if (positions) rows_host[r].pos = positions[r];
            rows_host[r].token = positions && positions[r] < 0 ? -1 : tokens[r];
            rows_host[r].step_index = r;
        }
        MC_HIP(hipMemcpyAsync(rows, rows_host.data(), sizeof(step_state) * B, hipMemcpyHostToDevice, p.stream));
        return MC_OK;
    }

    mc_status ensure_tokens(int n) { return reserve(tokens_dev, tokens_cap, n * B, n * B); }

    mc_status
    check_tokens(const int32_t* tokens) const
    {
        for (int r = 0; r < B; r++)
            if (tokens[r] < 0 || tokens[r] >= p.cfg.vocab)
                return fail(MC_ERR_INVALID_ARGUMENT, "mc_batch: token id outside the vocabulary");
        return MC_OK;
    }

    // (rows_plan.h: a row that has rolled is continued at its length or restarted at 0)
    std::string
    rolled_rewind(int r, int64_t pos) const { return mcimpl::rolled_rewind(lengths[r], p.cfg.max_seq_len, pos); }

    // a ragged call's positions and tokens: -1 = idle, else 0 <= pos <= the row's length and pos < max_seq_len (a rolling batch:
    // any pos, as long as the n steps of the call stay inside int32), with a token of the vocabulary; at least one row active
    mc_status
    check_ragged(const char* what, const int32_t* tokens, const int32_t* positions, int32_t n) const
    {
        int active = 0;
        for (int r = 0; r < B; r++) {
            const int32_t pos = positions[r];
            const std::string row = std::string(what) + ": row " + std::to_string(r) + ": ";
            if (pos == -1) continue;
            if (pos < -1) return fail(MC_ERR_INVALID_ARGUMENT, row + "position below -1 (-1 = idle)");
            if (!rolling && pos >= p.cfg.max_seq_len)
                return fail(MC_ERR_INVALID_ARGUMENT, row + "position " + std::to_string(pos) + " must be below max_seq_len (a batch's cache does not roll)");
            if (rolling && (int64_t)pos + n > INT32_MAX)
                return fail(MC_ERR_INVALID_ARGUMENT, row + "position " + std::to_string(pos) + " + n leaves the range of positions");
            if (pos > lengths[r])
                return fail(MC_ERR_INVALID_ARGUMENT, row + "position " + std::to_string(pos) + " is past the row's length " +
                                                         std::to_string(lengths[r]) + " (its cache has no slots written beyond it)");
            if (const std::string why = rolled_rewind(r, pos); !why.empty()) return fail(MC_ERR_INVALID_ARGUMENT, row + why);
            if (tokens[r] < 0 || tokens[r] >= p.cfg.vocab) return fail(MC_ERR_INVALID_ARGUMENT, row + "token id outside the vocabulary");
            active++;
        }
        if (!active) return fail(MC_ERR_INVALID_ARGUMENT, std::string(what) + ": no active row (every position is -1)");
        return MC_OK;
    }

    // token 0 of a ragged call: the rows, the stop ids, and -1 in every slot of tokens_out
    mc_status
    start_ragged(const int32_t* tokens, const int32_t* positions, const int32_t* stop_ids, int n_stop, int n)
    {
        mc_status s = start_rows(tokens, positions);
        if (s != MC_OK) return s;
        stop_host.assign(stop_ids, stop_ids + n_stop);
        if ((s = reserve(stop_dev, stop_cap, n_stop, n_stop)) != MC_OK) return s;
        if (n_stop > 0)
            MC_HIP(hipMemcpyAsync(stop_dev, stop_host.data(), sizeof(int32_t) * n_stop, hipMemcpyHostToDevice, p.stream));
        MC_HIP(hipMemsetAsync(tokens_dev, 0xFF, sizeof(int32_t) * (size_t)n * B, p.stream));
        return MC_OK;
    }
};

namespace {

// the admission predicate: "" = admitted, else the reason.  mc_batch_create (wide = false) takes one weight format for the whole
// decoder, int4 in groups that are multiples of 128 or plain T, and no adaptors.  mc_wide_batch_create (wide = true, Part 2i) judges
// every linear on its own: T, int4 or int8, quantised in groups that are multiples of 32 or one scale per row, and on the seven
// layer linears adaptors whose fused columns are a multiple of 16.  The conditions both share keep one text.
std::string
refusal(const decoder_parts& p, bool wide)
{
    const mc_decoder_config& c = p.cfg;
    if (c.family != MC_FAMILY_LLAMA3) return "only llama3 decoders can be batched";
    if (c.dtype != MC_DTYPE_BF16) return "only bfloat16 decoders can be batched";
    if (c.layer_begin != 0 || c.layer_end != c.n_layers) return "the decoder must own every layer (a pipeline stage cannot be batched)";
    if (!wide && c.weight_format != MC_WFMT_I4 && c.weight_format != MC_WFMT_T)
        return "only int4 (group % 128 == 0) and plain bfloat16 weights can be batched";
    if (!wide && c.weight_format == MC_WFMT_I4 && c.group_size % 128 != 0) return "int4 weights need a group size that is a multiple of 128";
    if (c.qmode != MC_QMODE_EXACT) return "only the exact quantised arithmetic (MC_QMODE_EXACT) can be batched";
    if (c.head_dim != 128 && c.head_dim != 64) return "head_dim must be 128 or 64";
    if (c.n_kv_heads <= 0 || c.n_heads % c.n_kv_heads != 0 || c.n_heads / c.n_kv_heads > 16)
        return "n_heads must be a multiple of n_kv_heads, at most 16 per kv head";
    if (c.max_seq_len < 64) return "max_seq_len must be at least 64";
    if (p.emb_fmt != MC_WFMT_T && p.emb_fmt != MC_WFMT_I8) return "unsupported embedding format";
    auto bad = [&](const batch_linear& L, const char* name, bool head) -> std::string {
        if (!wide) {
            if (L.lora) return std::string("LoRA adaptors are not supported (") + name + ")";
            if (L.fmt != c.weight_format) return std::string("mixed weight formats (") + name + ")";
        } else {
            if (L.fmt != MC_WFMT_T && L.fmt != MC_WFMT_I4 && L.fmt != MC_WFMT_I8)
                return std::string(name) + ": only int4, int8 and plain bfloat16 weights can be batched";
            if (L.lora && head) return std::string("LoRA adaptors are not supported (") + name + ")";
            if (L.lora && L.lora_cols % 16 != 0) return std::string(name) + ": LoRA rank must be a multiple of 16";
        }
        if (L.out % 16 != 0 || L.in % (int)BG_K_UNIT != 0)
            return std::string(name) + ": the batched GEMV needs out_features % 16 == 0 and in_features % 1024 == 0";
        if (!wide && L.fmt == MC_WFMT_I4 && L.group % 128 != 0) return std::string(name) + ": int4 group size must be a multiple of 128";
        if (wide && L.fmt != MC_WFMT_T && L.group % 32 != 0)
            return std::string(name) + ": the group size of quantised weights must be a multiple of 32 (or 0: one scale per row)";
        return "";
    };
    const int H = c.n_heads, KV = c.n_kv_heads, hd = c.head_dim;
    for (const batch_layer& L : p.layers) {
        for (auto [lin, name] : {std::pair<const batch_linear*, const char*>{&L.qkv, "wq|wk|wv"}, {&L.wo, "wo"}, {&L.w13, "w1|w3"},
                                 {&L.w2, "w2"}}) {
            std::string r = bad(*lin, name, false);
            if (!r.empty()) return r;
        }
        if (L.qkv.out != (H + 2 * KV) * hd || L.qkv.in != c.dim || L.wo.in != H * hd || L.wo.out != c.dim ||
            L.w13.out % 32 != 0 || L.w13.in != c.dim || L.w2.in != L.w13.out / 2 || L.w2.out != c.dim)
            return "layer shapes do not chain";
    }
    std::string r = bad(p.output, "output", true);
    if (!r.empty()) return r;
    if (p.output.out != c.vocab || p.output.in != c.dim) return "output head shape";
    return "";
}

mc_status
find_row(mc_batch* b, int32_t row, int32_t layer, const char* what)
{
    if (!b) return fail(MC_ERR_INVALID_ARGUMENT, std::string(what) + ": null argument");
    if (row < 0 || row >= b->B) return fail(MC_ERR_INVALID_ARGUMENT, std::string(what) + ": row out of range");
    if (layer < 0 || layer >= (int)b->p.layers.size()) return fail(MC_ERR_INVALID_ARGUMENT, std::string(what) + ": layer out of range");
    return MC_OK;
}

// mc_batch_export_kv and mc_ragged_export_kv: row `row`'s cache of `layer` through mc_kv_export_bfloat, which takes kv_len (and
// the ring) from the device step state `state`, into staging buffers of `cap` positions; then n positions to the host.
// n < 0: n = that kv_len, read back behind the launch and reported in *n_out.
mc_status
export_kv(mc_batch* b, const char* what, int32_t row, int32_t layer, const step_state* state, int32_t cap, int32_t n, int32_t* n_out,
          void* keys, void* values)
{
    const mc_decoder_config& c = b->p.cfg;
    const size_t per_pos = (size_t)c.n_kv_heads * c.head_dim * 2;
    device_tmp kt, vtmp;
    hipError_t e = kt.alloc(cap * per_pos);
    if (e == hipSuccess) e = vtmp.alloc(cap * per_pos);
    if (e != hipSuccess) return hip_fail(e, what);
    mc_status s = b->launch("mc_kv_export_bfloat", 512, 1, 1, 256, 0,
                            pack((const void*)b->kc_of(layer, row), (const void*)b->vt_of(layer, row), kt.ptr, vtmp.ptr, (const void*)state,
                                 (uint32_t)c.n_kv_heads, (uint32_t)c.head_dim, (uint32_t)c.max_seq_len, (uint32_t)b->p.pre_len));
    e = hipStreamSynchronize(b->p.stream);
    if (s == MC_OK && e == hipSuccess && n < 0) {
        step_state st{};
        e = hipMemcpy(&st, state, sizeof st, hipMemcpyDeviceToHost);
        n = st.kv_len;
        if (n_out) *n_out = n;
    }
    if (s == MC_OK && e == hipSuccess && keys) e = hipMemcpy(keys, kt.ptr, n * per_pos, hipMemcpyDeviceToHost);
    if (s == MC_OK && e == hipSuccess && values) e = hipMemcpy(values, vtmp.ptr, n * per_pos, hipMemcpyDeviceToHost);
    if (e != hipSuccess) return hip_fail(e, what);
    return s;
}

// mc_ragged_export_kv (and mc_batch_export_kv for a row that has rolled): row `row`'s own logical view, min(length, max_seq_len)
// positions -- the sink rows, then the ring unrolled.  The export kernel reads kv_len and the ring from a state of its own, made
// from the row's length: the row last wrote position length - 1, which fixes its ring (mc_b_rows_begin_rolling)
mc_status
export_row(mc_batch* b, const char* what, int32_t row, int32_t layer, void* keys, void* values, int32_t* n_valid)
{
    const int32_t len = b->lengths[row], S = b->p.cfg.max_seq_len, n = std::min(len, S);
    if (n_valid) *n_valid = n;
    if (n == 0) return MC_OK;
    MC_HIP(hipSetDevice(b->p.ordinal));
    step_state st{};
    st.kv_len = n;
    st.ring_base = len > S ? (len - S) % (S - b->p.pre_len) : 0;
    device_tmp stv;
    hipError_t e = stv.alloc(sizeof st);
    if (e == hipSuccess) e = hipMemcpyAsync(stv.ptr, &st, sizeof st, hipMemcpyHostToDevice, b->p.stream);
    if (e != hipSuccess) return hip_fail(e, what);
    return export_kv(b, what, row, layer, static_cast<const step_state*>(stv.ptr), n, n, nullptr, keys, values);
}

} // namespace

extern "C" {

// mc_batch_create and mc_wide_batch_create: `who` names the caller in the texts, `cap` is its largest batch, `wide` its admission
static mc_status
batch_create(const std::string& who, int cap, bool wide, mc_decoder* d, int32_t batch, mc_batch** out)
{
    if (!d || !out) return fail(MC_ERR_INVALID_ARGUMENT, who + ": null argument");
    if (batch < 1 || batch > cap) return fail(MC_ERR_INVALID_ARGUMENT, who + ": batch must lie in [1, " + std::to_string(cap) + "]");
    *out = nullptr;
    decoder_parts parts;
    mc_status s = decoder_parts_of(d, &parts);
    if (s != MC_OK) return s;
    const std::string why = refusal(parts, wide);
    if (!why.empty()) return fail(MC_ERR_INVALID_ARGUMENT, who + ": " + why);
    MC_HIP(hipSetDevice(parts.ordinal));
    std::unique_ptr<mc_batch> b(new mc_batch);
    MC_HIP(hipDeviceGetAttribute(&b->wb_cus, hipDeviceAttributeMultiprocessorCount, parts.ordinal));
    if (const char* e = getenv("MC_WB_TILES")) {
        const int t = atoi(e);
        if (t == 1 || t == 2 || t == 4 || t == 8) b->wb_tiles_env = t;
    }
    b->d = d;
    b->p = parts;
    b->B = batch;
    b->lengths.assign(batch, 0);
    b->row_samplers.assign(batch, mc_batch::row_setting{});
    b->row_logit_set.assign(batch, mc_batch::row_logit_setting{});
    const mc_decoder_config& c = parts.cfg;
    const int H = c.n_heads, KV = c.n_kv_heads, hd = c.head_dim, L = (int)parts.layers.size();
    b->nsplit = (c.max_seq_len + PB - 1) / PB;
    b->cache_elems = (size_t)KV * c.max_seq_len * hd;
    const size_t cache_bytes = (size_t)L * batch * b->cache_elems * 2;
    const int ffn = parts.layers.empty() ? 0 : parts.layers[0].w13.out / 2;
    const uint32_t lists512 = ((uint32_t)c.vocab + 511) / 512;
    b->cand_per_row = (size_t)std::max(lists512, 1u) * 128;
    if ((s = b->alloc(&b->kc, cache_bytes)) != MC_OK || (s = b->alloc(&b->vt, cache_bytes)) != MC_OK ||
        (s = b->alloc(&b->x, (size_t)batch * c.dim * 2)) != MC_OK || (s = b->alloc(&b->xn, (size_t)batch * c.dim * 2)) != MC_OK ||
        (s = b->alloc(&b->qkv, (size_t)batch * (H + 2 * KV) * hd * 2)) != MC_OK ||
        (s = b->alloc(&b->q, (size_t)batch * H * hd * 2)) != MC_OK || (s = b->alloc(&b->att, (size_t)batch * H * hd * 2)) != MC_OK ||
        (s = b->alloc(&b->gate, (size_t)batch * ffn * 2)) != MC_OK ||
        (s = b->alloc(&b->logits, (size_t)batch * c.vocab * 2)) != MC_OK ||
        (s = b->alloc(&b->expv, sizeof(float) * batch * H * c.max_seq_len)) != MC_OK ||
        (s = b->alloc(&b->psum, sizeof(float) * batch * H * b->nsplit)) != MC_OK ||
        (s = b->alloc(&b->fcos, sizeof(float) * c.max_seq_len * (hd / 2))) != MC_OK ||
        (s = b->alloc(&b->fsin, sizeof(float) * c.max_seq_len * (hd / 2))) != MC_OK ||
        (s = b->alloc(&b->rcos, sizeof(float) * batch * (hd / 2))) != MC_OK ||
        (s = b->alloc(&b->rsin, sizeof(float) * batch * (hd / 2))) != MC_OK ||
        (s = b->alloc(&b->st, sizeof(step_state))) != MC_OK || (s = b->alloc(&b->rows, sizeof(step_state) * batch)) != MC_OK ||
        (s = b->alloc(&b->cand, sizeof(uint64_t) * batch * b->cand_per_row)) != MC_OK ||
        (s = b->alloc(&b->samplers_dev, sizeof(row_sampler) * batch)) != MC_OK)
        return s;
    for (const batch_layer& l : parts.layers)
        for (const batch_linear* lin : {&l.qkv, &l.wo, &l.w13, &l.w2}) b->lora_ld = std::max(b->lora_ld, lin->lora_cols);
    if (b->lora_ld && (s = b->alloc(&b->lora_vec, (size_t)batch * b->lora_ld * 2)) != MC_OK) return s;
    // nn::rope's table for positions [0, max_seq_len) (a row depends on the absolute position only, nn/embedding.h:159-165)
    s = b->launch("mc_rope_table", (hd / 2 + 63) / 64, c.max_seq_len, 1, 64, 0,
                  pack(b->fcos, b->fsin, (uint32_t)c.max_seq_len, (uint32_t)hd, (uint32_t)0, c.rope_theta));
    if (s != MC_OK) return s;
    MC_HIP(hipStreamSynchronize(parts.stream));
    *out = b.release();
    return MC_OK;
}

mc_status
mc_batch_create(mc_decoder* d, int32_t batch, mc_batch** out)
{
    return batch_create("mc_batch_create", BATCH_MAX, false, d, batch, out);
}

// ---- Part 2h: wide batches ----

mc_status
mc_wide_batch_create(mc_decoder* d, int32_t batch, mc_batch** out)
{
    return batch_create("mc_wide_batch_create", MC_WIDE_BATCH_MAX, true, d, batch, out);
}

void
mc_batch_release(mc_batch* b)
{
    delete b;
}

int32_t
mc_batch_size(const mc_batch* b)
{
    return b ? b->B : 0;
}

mc_status
mc_batch_fork(mc_batch* b, int32_t row, int32_t n_valid)
{
    mc_status s = find_row(b, row, 0, "mc_batch_fork");
    if (s != MC_OK) return s;
    const mc_decoder_config& c = b->p.cfg;
    if (n_valid < 1 || n_valid > c.max_seq_len) return fail(MC_ERR_INVALID_ARGUMENT, "mc_batch_fork: n_valid must lie in [1, max_seq_len]");
    int kv_len = 0;
    bool rolled = false;
    if ((s = decoder_cache_state(b->d, &kv_len, &rolled)) != MC_OK) return s;
    if (rolled) return fail(MC_ERR_INVALID_ARGUMENT, "mc_batch_fork: the decoder's cache has rolled (sink ring turned)");
    if (n_valid > kv_len) return fail(MC_ERR_INVALID_ARGUMENT, "mc_batch_fork: the decoder's cache holds fewer than n_valid positions");
    MC_HIP(hipSetDevice(b->p.ordinal));
    const int KV = c.n_kv_heads, hd = c.head_dim, S = c.max_seq_len;
    for (size_t l = 0; l < b->p.layers.size(); l++) {
        const batch_layer& L = b->p.layers[l];
        // K [kv][pos][hd]: n_valid * hd elements per kv head; Vt [kv * hd][pos]: n_valid elements per row
        MC_HIP(hipMemcpy2DAsync(b->kc_of((int)l, row), (size_t)S * hd * 2, L.kc, (size_t)S * hd * 2, (size_t)n_valid * hd * 2, KV,
                                hipMemcpyDeviceToDevice, b->p.stream));
        MC_HIP(hipMemcpy2DAsync(b->vt_of((int)l, row), (size_t)S * 2, L.vt, (size_t)S * 2, (size_t)n_valid * 2, (size_t)KV * hd,
                                hipMemcpyDeviceToDevice, b->p.stream));
    }
    if ((s = b->set_pos(n_valid - 1)) != MC_OK) return s;
    MC_HIP(hipStreamSynchronize(b->p.stream));
    b->lengths[row] = n_valid;
    return MC_OK;
}

mc_status
mc_batch_import_kv(mc_batch* b, int32_t row, int32_t layer, const void* keys, const void* values, int32_t n_valid)
{
    mc_status s = find_row(b, row, layer, "mc_batch_import_kv");
    if (s != MC_OK) return s;
    if (!keys || !values) return fail(MC_ERR_INVALID_ARGUMENT, "mc_batch_import_kv: null argument");
    const mc_decoder_config& c = b->p.cfg;
    if (n_valid < 1 || n_valid > c.max_seq_len)
        return fail(MC_ERR_INVALID_ARGUMENT, "mc_batch_import_kv: n_valid must lie in [1, max_seq_len]");
    MC_HIP(hipSetDevice(b->p.ordinal));
    const size_t nb = (size_t)n_valid * c.n_kv_heads * c.head_dim * 2;
    device_tmp kt, vtmp;
    MC_HIP(kt.alloc(nb));
    hipError_t e = vtmp.alloc(nb);
    if (e == hipSuccess) e = hipMemcpy(kt.ptr, keys, nb, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(vtmp.ptr, values, nb, hipMemcpyHostToDevice);
    if (e == hipSuccess) {
        s = b->launch("mc_kv_import_bfloat", 512, 1, 1, 256, 0,
                      pack((void*)b->kc_of(layer, row), (void*)b->vt_of(layer, row), (const void*)kt.ptr, (const void*)vtmp.ptr,
                           (uint32_t)n_valid, (uint32_t)c.n_kv_heads, (uint32_t)c.head_dim, (uint32_t)c.max_seq_len));
        if (s == MC_OK) s = b->set_pos(n_valid - 1);
        e = hipStreamSynchronize(b->p.stream);
    }
    if (e != hipSuccess) return hip_fail(e, "mc_batch_import_kv");
    if (s == MC_OK) b->lengths[row] = n_valid;
    return s;
}

mc_status
mc_batch_export_kv(mc_batch* b, int32_t row, int32_t layer, void* keys, void* values, int32_t* n_valid)
{
    mc_status s = find_row(b, row, layer, "mc_batch_export_kv");
    if (s != MC_OK) return s;
    // a row that has rolled has no lockstep view: its own (Part 2j)
    if (b->lengths[row] > b->p.cfg.max_seq_len) return export_row(b, "mc_batch_export_kv", row, layer, keys, values, n_valid);
    MC_HIP(hipSetDevice(b->p.ordinal));
    // kv_len of the batch's shared state: the position of the last lockstep step, fork or import, whichever row that was for
    return export_kv(b, "mc_batch_export_kv", row, layer, b->st, b->p.cfg.max_seq_len, -1, n_valid, keys, values);
}

mc_status
mc_batch_step(mc_batch* b, const int32_t* tokens, int32_t start_pos, int32_t* next_tokens)
{
    if (!b || !tokens) return fail(MC_ERR_INVALID_ARGUMENT, "mc_batch_step: null argument");
    if (start_pos < 0 || start_pos + 1 > b->p.cfg.max_seq_len)
        return fail(MC_ERR_INVALID_ARGUMENT, "mc_batch_step: start_pos + 1 must not exceed max_seq_len (a batch's cache does not roll)");
    mc_status s = b->check_tokens(tokens);
    if (s != MC_OK) return s;
    MC_HIP(hipSetDevice(b->p.ordinal));
    if ((s = b->ensure_tokens(1)) != MC_OK || (s = b->start_rows(tokens)) != MC_OK || (s = b->enqueue_token(start_pos, false)) != MC_OK)
        return s;
    MC_HIP(hipStreamSynchronize(b->p.stream));
    b->lengths.assign(b->B, start_pos + 1);
    if (next_tokens) MC_HIP(hipMemcpy(next_tokens, b->tokens_dev, sizeof(int32_t) * b->B, hipMemcpyDeviceToHost));
    return MC_OK;
}

mc_status
mc_batch_generate(mc_batch* b, const int32_t* first_tokens, int32_t start_pos, int32_t n, int32_t* tokens_out)
{
    if (!b || !first_tokens || !tokens_out) return fail(MC_ERR_INVALID_ARGUMENT, "mc_batch_generate: null argument");
    if (n < 1) return fail(MC_ERR_INVALID_ARGUMENT, "mc_batch_generate: n must be positive");
    if (start_pos < 0 || (int64_t)start_pos + n > b->p.cfg.max_seq_len)
        return fail(MC_ERR_INVALID_ARGUMENT, "mc_batch_generate: start_pos + n must not exceed max_seq_len (a batch's cache does not roll)");
    mc_status s = b->check_tokens(first_tokens);
    if (s != MC_OK) return s;
    MC_HIP(hipSetDevice(b->p.ordinal));
    if ((s = b->ensure_tokens(n)) != MC_OK || (s = b->start_rows(first_tokens)) != MC_OK) return s;
    for (int i = 0; i < n; i++)
        if ((s = b->enqueue_token(start_pos + i, i > 0)) != MC_OK) return s;
    MC_HIP(hipStreamSynchronize(b->p.stream));
    b->lengths.assign(b->B, start_pos + n);
    MC_HIP(hipMemcpy(tokens_out, b->tokens_dev, sizeof(int32_t) * (size_t)n * b->B, hipMemcpyDeviceToHost));
    return MC_OK;
}

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

mc_status
mc_batch_get_logits(mc_batch* b, void* logits_T)
{
    if (!b || !logits_T) return fail(MC_ERR_INVALID_ARGUMENT, "mc_batch_get_logits: null argument");
    MC_HIP(hipSetDevice(b->p.ordinal));
    MC_HIP(hipStreamSynchronize(b->p.stream));
    MC_HIP(hipMemcpy(logits_T, b->logits, (size_t)b->B * b->p.cfg.vocab * 2, hipMemcpyDeviceToHost));
    return MC_OK;
}

// ---- Part 2d: the packed prompt pass ----

namespace {

// what mc_verify_rows adds to the pass: a pick after every chunk row and the acceptance (next_tokens is the pass's own argument)
struct verify_out {
    int32_t* accepted; // [B]
    int32_t* picks;    // [M], may be null
    // mc_tree_verify: the chunks are trees
    const int32_t* parents = nullptr; // [M], packed like the tokens
    int32_t* paths = nullptr;         // [B][MC_VERIFY_MAX_LEN], may be null
};

// mc_rows_prefill, mc_extend_rows, mc_verify_rows and mc_tree_verify: one body, `extend` selects the attention (and `who` the
// texts), `v` the head over every packed row in place of the head over each row's last, v->parents the tree form of that
mc_status
rows_pass(mc_batch* b, const char* who, bool extend, const int32_t* tokens, const int32_t* lens, const int32_t* positions, int32_t* next_tokens,
          const verify_out* v = nullptr)
{
    const mc_decoder_config& c = b->p.cfg;
    const int B = b->B;
    // check (rows_plan.h: the admission, the tables and the scratch sizes are plain arithmetic there), tables, upload, prompt pass, head
    const bool tree = v && v->parents;
    const rows_counts n = rows_check(who, tokens, lens, positions, b->lengths.data(), B, c.max_seq_len, c.vocab, v != nullptr);
    if (!n.refusal.empty()) return fail(MC_ERR_INVALID_ARGUMENT, n.refusal);
    if (tree)
        if (const std::string why = tree_check(who, v->parents, lens, B); !why.empty()) return fail(MC_ERR_INVALID_ARGUMENT, why);
    const int M = n.M, nseg = n.nseg, ntiles = n.ntiles;
    // MC_PX_KEYS, the experiment's handle on the key ranges, is read at the call (the tests set it between calls on a live batch)
    const char* keys_env = getenv("MC_PX_KEYS");
    const int keys_override = keys_env ? std::max(atoi(keys_env), 0) : PX_KEYS_RULE;
    const rows_scratch sc = rows_scratch_of(c.max_seq_len, c.n_heads, c.head_dim, keys_override);
    mc_status s;
    MC_HIP(hipSetDevice(b->p.ordinal));
    rows_tables(lens, positions, B, ntiles, b->rows_host, b->pp_host);
    if (tree) tree_nodes(v->parents, lens, B, ntiles, M, b->pp_host);
    if ((s = b->reserve(b->pp_tab, b->pp_tab_cap, (int)b->pp_host.size(), (int)sc.tab_bytes())) != MC_OK) return s;
    MC_HIP(hipMemcpyAsync(b->pp_tab, b->pp_host.data(), b->pp_host.size(), hipMemcpyHostToDevice, b->p.stream));
    packed_prefill pk;
    pk.segs = pp_segs(b->pp_tab);
    pk.nseg = nseg;
    pk.tiles = pp_tiles(b->pp_tab);
    pk.ntiles = ntiles;
    if (tree) pk.nodes = tv_nodes(b->pp_tab, ntiles);
    MC_HIP(hipMemcpyAsync(b->rows, b->rows_host.data(), sizeof(step_state) * B, hipMemcpyHostToDevice, b->p.stream));
    if ((s = b->ensure_tokens(1)) != MC_OK) return s;
    MC_HIP(hipMemsetAsync(b->tokens_dev, 0xFF, sizeof(int32_t) * B, b->p.stream));
    pk.kc = b->kc;
    pk.vt = b->vt;
    pk.B = B;
    pk.cache_stride = b->cache_elems;
    pk.fcos = b->fcos;
    pk.fsin = b->fsin;
    pk.x_out = b->x;
    if (extend) {
        // scratch for one launch group, sized once (rows_scratch_of)
        int sums_slots = b->px_slots;
        if ((s = b->reserve(b->px_sums, sums_slots, sc.per_tile, sc.slots, sizeof(float) * c.n_heads * PP_TILE_ROWS)) != MC_OK ||
            (s = b->reserve(b->px_part, b->px_slots, sc.per_tile, sc.slots, sc.per_slot)) != MC_OK)
            return s;
        rows_ranges(b->pp_host, ntiles, b->px_slots, keys_override, b->px_host, b->px_groups);
        if ((s = b->reserve(b->px_tab, b->px_tab_cap, (int)b->px_host.size(), sc.tiles_max * sc.per_tile)) != MC_OK) return s;
        MC_HIP(hipMemcpyAsync(b->px_tab, b->px_host.data(), sizeof(px_range) * b->px_host.size(), hipMemcpyHostToDevice, b->p.stream));
        pk.extend = true;
        pk.ranges = b->px_tab;
        pk.groups = b->px_groups.data();
        pk.ngroups = (int)b->px_groups.size();
        pk.sums = b->px_sums;
        pk.part = b->px_part;
    }
    const void* rows_all = nullptr;
    const int32_t* ids = nullptr;
    if (v) {
        // (M <= 128 here; the scratch is sized for any call)
        if ((s = b->reserve(b->v_xn, b->v_xn_cap, M, MC_VERIFY_MAX_ROWS, (size_t)c.dim * 2)) != MC_OK ||
            (s = b->reserve(b->v_logits, b->v_logits_cap, M, MC_VERIFY_MAX_ROWS, (size_t)c.vocab * 2)) != MC_OK ||
            (s = b->reserve(b->v_out, b->v_out_cap, 2 * B + M + MC_VERIFY_MAX_LEN * B, 2 * MC_WIDE_BATCH_MAX + MC_VERIFY_MAX_ROWS + MC_VERIFY_MAX_LEN * MC_WIDE_BATCH_MAX)) !=
                MC_OK)
            return s;
        MC_HIP(hipMemsetAsync(b->v_out, 0xFF, sizeof(int32_t) * 2 * B, b->p.stream)); // -1: a row not in the call
        if (tree) MC_HIP(hipMemsetAsync(b->v_out + 2 * B + M, 0xFF, sizeof(int32_t) * MC_VERIFY_MAX_LEN * B, b->p.stream)); // ... its path
        pk.rows_all = &rows_all;
        pk.tokens_dev = &ids;
    }
    if ((s = decoder_prefill_packed(b->d, tokens, M, pk)) != MC_OK) return s;
    if ((s = v ? b->verify_head(rows_all, ids, M, nseg, pk.nodes) : b->head("_rows_bfloat", false)) != MC_OK) return s;
    MC_HIP(hipStreamSynchronize(b->p.stream)); // (`tokens` is the caller's buffer; the tables are read by the launches)
    if (v) {
        b->v_rows = M;
        b->v_host.resize(2 * B + M + (tree ? MC_VERIFY_MAX_LEN * B : 0));
        MC_HIP(hipMemcpy(b->v_host.data(), b->v_out, sizeof(int32_t) * b->v_host.size(), hipMemcpyDeviceToHost));
        std::copy_n(b->v_host.begin(), B, v->accepted);
        if (next_tokens) std::copy_n(b->v_host.begin() + B, B, next_tokens);
        if (v->picks) std::copy_n(b->v_host.begin() + 2 * B, M, v->picks);
        if (v->paths) std::copy_n(b->v_host.begin() + 2 * B + M, MC_VERIFY_MAX_LEN * B, v->paths);
        // the rejected drafts' slots stay written past the length: the rewound state every rows call handles
        for (int r = 0; r < B; r++)
            if (lens[r] > 0) b->lengths[r] = positions[r] + v->accepted[r] + 1;
        return MC_OK;
    }
    for (int r = 0; r < B; r++)
        if (lens[r] > 0) b->lengths[r] = positions[r] + lens[r];
    if (next_tokens) MC_HIP(hipMemcpy(next_tokens, b->tokens_dev, sizeof(int32_t) * B, hipMemcpyDeviceToHost));
    return MC_OK;
}

} // namespace

mc_status
mc_rows_prefill(mc_batch* b, const int32_t* tokens, const int32_t* lens, const int32_t* positions, int32_t* next_tokens)
{
    if (!b || !tokens || !lens || !positions) return fail(MC_ERR_INVALID_ARGUMENT, "mc_rows_prefill: null argument");
    return rows_pass(b, "mc_rows_prefill", false, tokens, lens, positions, next_tokens);
}

// ---- Part 2e: chunks that see their row's context ----

mc_status
mc_extend_rows(mc_batch* b, const int32_t* tokens, const int32_t* lens, const int32_t* positions, int32_t* next_tokens)
{
    if (!b || !tokens || !lens || !positions) return fail(MC_ERR_INVALID_ARGUMENT, "mc_extend_rows: null argument");
    return rows_pass(b, "mc_extend_rows", true, tokens, lens, positions, next_tokens);
}

// ---- Part 2f: speculative verify ----

mc_status
mc_verify_rows(mc_batch* b, const int32_t* tokens, const int32_t* lens, const int32_t* positions, int32_t* accepted, int32_t* next_tokens,
               int32_t* picks)
{
    if (!b || !tokens || !lens || !positions || !accepted) return fail(MC_ERR_INVALID_ARGUMENT, "mc_verify_rows: null argument");
    if (mc_status s = b->verify_samplers("mc_verify_rows", lens); s != MC_OK) return s;
    if (mc_status s = b->verify_logit_rows("mc_verify_rows", lens); s != MC_OK) return s;
    const verify_out v{accepted, picks};
    return rows_pass(b, "mc_verify_rows", true, tokens, lens, positions, next_tokens, &v);
}

// ---- Part 2g: speculative verify over a draft tree per row ----

mc_status
mc_tree_verify(mc_batch* b, const int32_t* tokens, const int32_t* parents, const int32_t* lens, const int32_t* positions, int32_t* accepted,
               int32_t* next_tokens, int32_t* paths, int32_t* picks)
{
    if (!b || !tokens || !parents || !lens || !positions || !accepted) return fail(MC_ERR_INVALID_ARGUMENT, "mc_tree_verify: null argument");
    if (mc_status s = b->verify_samplers("mc_tree_verify", lens); s != MC_OK) return s;
    if (mc_status s = b->verify_logit_rows("mc_tree_verify", lens); s != MC_OK) return s;
    const verify_out v{accepted, picks, parents, paths};
    return rows_pass(b, "mc_tree_verify", true, tokens, lens, positions, next_tokens, &v);
}

mc_status
mc_verify_get_logits(mc_batch* b, void* logits_T)
{
    if (!b || !logits_T) return fail(MC_ERR_INVALID_ARGUMENT, "mc_verify_get_logits: null argument");
    if (!b->v_rows) return fail(MC_ERR_INVALID_ARGUMENT, "mc_verify_get_logits: no mc_verify_rows call on this batch yet");
    MC_HIP(hipSetDevice(b->p.ordinal));
    MC_HIP(hipStreamSynchronize(b->p.stream));
    MC_HIP(hipMemcpy(logits_T, b->v_logits, (size_t)b->v_rows * b->p.cfg.vocab * 2, hipMemcpyDeviceToHost));
    return MC_OK;
}

// ---- Part 2c: ragged rows ----

mc_status
mc_ragged_step(mc_batch* b, const int32_t* tokens, const int32_t* positions, int32_t* next_tokens)
{
    if (!b || !tokens || !positions) return fail(MC_ERR_INVALID_ARGUMENT, "mc_ragged_step: null argument");
    mc_status s = b->check_ragged("mc_ragged_step", tokens, positions, 1);
    if (s != MC_OK) return s;
    MC_HIP(hipSetDevice(b->p.ordinal));
    if ((s = b->ensure_tokens(1)) != MC_OK || (s = b->start_ragged(tokens, positions, nullptr, 0, 1)) != MC_OK ||
        (s = b->enqueue_token(0, false, true)) != MC_OK)
        return s;
    MC_HIP(hipStreamSynchronize(b->p.stream));
    for (int r = 0; r < b->B; r++)
        if (positions[r] >= 0) b->lengths[r] = positions[r] + 1;
    if (next_tokens) MC_HIP(hipMemcpy(next_tokens, b->tokens_dev, sizeof(int32_t) * b->B, hipMemcpyDeviceToHost));
    return MC_OK;
}

mc_status
mc_ragged_generate(mc_batch* b, const int32_t* first_tokens, const int32_t* positions, int32_t n, const int32_t* stop_ids,
                   int32_t n_stop, int32_t* tokens_out, int32_t* lengths)
{
    if (!b || !first_tokens || !positions || !tokens_out || !lengths || (n_stop > 0 && !stop_ids))
        return fail(MC_ERR_INVALID_ARGUMENT, "mc_ragged_generate: null argument");
    if (n < 1) return fail(MC_ERR_INVALID_ARGUMENT, "mc_ragged_generate: n must be positive");
    if (n_stop < 0) return fail(MC_ERR_INVALID_ARGUMENT, "mc_ragged_generate: n_stop must not be negative");
    mc_status s = b->check_ragged("mc_ragged_generate", first_tokens, positions, n);
    if (s != MC_OK) return s;
    MC_HIP(hipSetDevice(b->p.ordinal));
    if ((s = b->ensure_tokens(n)) != MC_OK || (s = b->start_ragged(first_tokens, positions, stop_ids, n_stop, n)) != MC_OK) return s;
    for (int i = 0; i < n; i++)
        if ((s = b->enqueue_token(0, i > 0, true)) != MC_OK) return s;
    MC_HIP(hipStreamSynchronize(b->p.stream));
    const int B = b->B;
    MC_HIP(hipMemcpy(tokens_out, b->tokens_dev, sizeof(int32_t) * (size_t)n * B, hipMemcpyDeviceToHost));
    // a row's tokens are a prefix of its column: -1 from the step after it stopped (an idle row: none)
    for (int r = 0; r < B; r++) {
        int32_t produced = 0;
        while (produced < n && tokens_out[(size_t)produced * B + r] >= 0) produced++;
        lengths[r] = produced;
        if (positions[r] >= 0) b->lengths[r] = positions[r] + produced;
    }
    return MC_OK;
}

mc_status
mc_ragged_lengths(const mc_batch* b, int32_t* lengths)
{
    if (!b || !lengths) return fail(MC_ERR_INVALID_ARGUMENT, "mc_ragged_lengths: null argument");
    std::copy(b->lengths.begin(), b->lengths.end(), lengths);
    return MC_OK;
}

mc_status
mc_ragged_export_kv(mc_batch* b, int32_t row, int32_t layer, void* keys, void* values, int32_t* n_valid)
{
    mc_status s = find_row(b, row, layer, "mc_ragged_export_kv");
    if (s != MC_OK) return s;
    return export_row(b, "mc_ragged_export_kv", row, layer, keys, values, n_valid);
}

// ---- Part 2j: rolling rows ----

mc_status
mc_rolling_set(mc_batch* b, int32_t enable)
{
    if (!b) return fail(MC_ERR_INVALID_ARGUMENT, "mc_rolling_set: null argument");
    if (enable != 0 && enable != 1) return fail(MC_ERR_INVALID_ARGUMENT, "mc_rolling_set: enable must be 0 or 1");
    b->rolling = enable == 1;
    return MC_OK;
}

int32_t
mc_rolling_enabled(const mc_batch* b)
{
    return b && b->rolling ? 1 : 0;
}

mc_status
mc_rolling_fork_row(mc_batch* b, int32_t dst, int32_t src)
{
    if (!b) return fail(MC_ERR_INVALID_ARGUMENT, "mc_rolling_fork_row: null argument");
    if (dst < 0 || dst >= b->B || src < 0 || src >= b->B) return fail(MC_ERR_INVALID_ARGUMENT, "mc_rolling_fork_row: row out of range");
    if (dst == src) return fail(MC_ERR_INVALID_ARGUMENT, "mc_rolling_fork_row: dst and src are the same row");
    const mc_decoder_config& c = b->p.cfg;
    const int KV = c.n_kv_heads, hd = c.head_dim, S = c.max_seq_len;
    // the physical slots as they lie: a rolled row's ring follows from its length, which the copy takes along
    const int n = std::min(b->lengths[src], S);
    MC_HIP(hipSetDevice(b->p.ordinal));
    for (int l = 0; n > 0 && l < (int)b->p.layers.size(); l++) {
        // K [kv][slot][hd]: n * hd elements per kv head; Vt [kv * hd][slot]: n elements per row
        MC_HIP(hipMemcpy2DAsync(b->kc_of(l, dst), (size_t)S * hd * 2, b->kc_of(l, src), (size_t)S * hd * 2, (size_t)n * hd * 2, KV,
                                hipMemcpyDeviceToDevice, b->p.stream));
        MC_HIP(hipMemcpy2DAsync(b->vt_of(l, dst), (size_t)S * 2, b->vt_of(l, src), (size_t)S * 2, (size_t)n * 2, (size_t)KV * hd,
                                hipMemcpyDeviceToDevice, b->p.stream));
    }
    MC_HIP(hipStreamSynchronize(b->p.stream));
    b->lengths[dst] = b->lengths[src];
    return MC_OK;
}

// ---- Part 2k: row samplers ----

mc_status
mc_row_sampler_set(mc_batch* b, int32_t row, int32_t kind, int32_t top_k, float temperature, float top_p)
{
    if (!b) return fail(MC_ERR_INVALID_ARGUMENT, "mc_row_sampler_set: null argument");
    if (row < 0 || row >= b->B) return fail(MC_ERR_INVALID_ARGUMENT, "mc_row_sampler_set: row out of range");
    if (kind != MC_SAMPLER_INHERIT && kind != MC_SAMPLER_GREEDY && kind != MC_SAMPLER_DEFAULT)
        return fail(MC_ERR_INVALID_ARGUMENT, "mc_row_sampler_set: unknown sampler");
    mc_batch::row_setting rs;
    if (kind == MC_SAMPLER_DEFAULT) {
        // mc_decoder_set_sampler's checks and texts (nn/sampling.h:165-174), and its rounding (a batch is bfloat16)
        if (!(temperature > 0.0f)) return fail(MC_ERR_INVALID_ARGUMENT, "nucleus_sampler: temperature must be positive");
        if (top_p < 0.0f || top_p > 1.0f) return fail(MC_ERR_INVALID_ARGUMENT, "nucleus_sampler: probability must be in [0.0, 1.0]");
        if (top_k < 1 || top_k > 128) return fail(MC_ERR_INVALID_ARGUMENT, "topk_sampler: the fused sampler keeps 1..128 candidates");
        auto rt = [](float v) {
            uint32_t u;
            memcpy(&u, &v, 4);
            if ((u & 0x7f800000u) == 0x7f800000u && (u & 0x007fffffu)) u |= 0x400000u; // (a NaN stays one)
            else u += 0x7fffu + ((u >> 16) & 1u);
            u &= 0xFFFF0000u;
            memcpy(&v, &u, 4);
            return v;
        };
        rs.inv_temp_T = rt(1.0f / rt(temperature)); // T temp = T(1) / _M_temperature  (sampling.h:190)
        rs.top_p_T = rt(top_p);
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
    if (row < 0 || row >= b->B) return fail(MC_ERR_INVALID_ARGUMENT, "mc_row_sampler_get: row out of range");
    const mc_batch::row_setting& rs = b->row_samplers[row];
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
    b->row_samplers.assign(b->B, mc_batch::row_setting{});
    return MC_OK;
}

// ---- Part 2l: row logit processors ----
// Every batch call drains the stream before it returns, so the synchronous copies below meet an idle stream.

static mc_status
logit_row(const mc_batch* b, int32_t row, const char* who)
{
    if (!b) return fail(MC_ERR_INVALID_ARGUMENT, std::string(who) + ": null argument");
    if (row < 0 || row >= b->B) return fail(MC_ERR_INVALID_ARGUMENT, std::string(who) + ": row out of range");
    return MC_OK;
}

mc_status
mc_row_mask_set(mc_batch* b, int32_t row, const uint32_t* allowed, int32_t n_words)
{
    if (mc_status s = logit_row(b, row, "mc_row_mask_set"); s != MC_OK) return s;
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
    if (mc_status s = b->ensure_masks(); s != MC_OK) return s;
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
    if (mc_status s = logit_row(b, row, "mc_row_mask_get"); s != MC_OK) return s;
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
    if (mc_status s = logit_row(b, row, "mc_row_penalty_set"); s != MC_OK) return s;
    if (!std::isfinite(repetition) || !(repetition > 0.0f))
        return fail(MC_ERR_INVALID_ARGUMENT, "mc_row_penalty_set: repetition must be finite and positive");
    if (!std::isfinite(frequency)) return fail(MC_ERR_INVALID_ARGUMENT, "mc_row_penalty_set: frequency must be finite");
    if (!std::isfinite(presence)) return fail(MC_ERR_INVALID_ARGUMENT, "mc_row_penalty_set: presence must be finite");
    if (mc_status s = b->ensure_counts(); s != MC_OK) return s;
    mc_batch::row_logit_setting& rs = b->row_logit_set[row];
    rs.rep = repetition;
    rs.freq = frequency;
    rs.pres = presence;
    return MC_OK;
}

mc_status
mc_row_penalty_get(const mc_batch* b, int32_t row, float* repetition, float* frequency, float* presence)
{
    if (mc_status s = logit_row(b, row, "mc_row_penalty_get"); s != MC_OK) return s;
    const mc_batch::row_logit_setting& rs = b->row_logit_set[row];
    if (repetition) *repetition = rs.rep;
    if (frequency) *frequency = rs.freq;
    if (presence) *presence = rs.pres;
    return MC_OK;
}

mc_status
mc_row_penalty_count(mc_batch* b, int32_t row, const int32_t* tokens, int32_t n)
{
    if (mc_status s = logit_row(b, row, "mc_row_penalty_count"); s != MC_OK) return s;
    if (n < 0) return fail(MC_ERR_INVALID_ARGUMENT, "mc_row_penalty_count: n must not be negative");
    if (n > 0 && !tokens) return fail(MC_ERR_INVALID_ARGUMENT, "mc_row_penalty_count: null argument");
    const int vocab = b->p.cfg.vocab;
    for (int32_t i = 0; i < n; i++)
        if (tokens[i] < 0 || tokens[i] >= vocab)
            return fail(MC_ERR_INVALID_ARGUMENT, "mc_row_penalty_count: token " + std::to_string(i) + " (id " + std::to_string(tokens[i]) +
                                                     ") is outside the vocabulary");
    if (mc_status s = b->ensure_counts(); s != MC_OK) return s;
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
    if (mc_status s = logit_row(b, row, "mc_row_penalty_counts"); s != MC_OK) return s;
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
    if (mc_status s = logit_row(b, row, "mc_row_penalty_clear"); s != MC_OK) return s;
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
    b->row_logit_set.assign(b->B, mc_batch::row_logit_setting{});
    if (!b->counts_dev) return MC_OK;
    MC_HIP(hipSetDevice(b->p.ordinal));
    MC_HIP(hipMemsetAsync(b->counts_dev, 0, sizeof(int32_t) * (size_t)b->B * b->p.cfg.vocab, b->p.stream));
    MC_HIP(hipStreamSynchronize(b->p.stream));
    return MC_OK;
}

} // extern "C"
