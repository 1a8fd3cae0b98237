// The prompt pass of a decoder: M > 1 rows through every owned block with GEMMs instead of GEMVs (kernels/prefill_kernels.hip, pf_gemm8.h; the
// packed, extend and tree forms of the batch: packed_kernels.hip, extend_kernels.hip, tree_kernels.hip).  What is launched -- each GEMM's family, tiles and
// K ranges, the attention kernel, the rope form, the folds -- is decided in prefill_plan.h, without a device; run_prefill is the one launch sequence; the
// library GEMM the plan may choose is prefill_blaslt.cc.
#include "decoder_impl.h"

using namespace mcimpl;

    // ---------------------------------------------------------------- prompt pass

// a scratch buffer that only grows (pf_part, pf_lora, pf_probs): the stream has finished with the old one before it is given back
mc_status
mc_decoder::grow(void** p, size_t* have, size_t need, size_t elem_bytes)
{
    if (need <= *have) return MC_OK;
    MC_HIP(hipStreamSynchronize(stream));
    release(p);
    *have = 0;
    mc_status s = alloc(p, need * elem_bytes, false);
    if (s == MC_OK) *have = need;
    return s;
}

mc_status
mc_decoder::ensure_prefill(int M, int S)
{
    const int H = cfg.n_heads, KV = cfg.n_kv_heads, hd = cfg.head_dim;
    mc_status s;
    if (M > pf_cap) {
        // grow geometrically in whole 128-row tiles and give the superseded buffers back: a chat whose prompts
        // grow a little every turn must not strand a set of row buffers per turn
        const int cap = std::min(std::max({M, 2 * pf_cap, 128}), std::max(M, cfg.max_seq_len)) + 127 & ~127;
        MC_HIP(hipStreamSynchronize(stream));
#define A(ptr, bytes)                         \
release((void**)&(ptr));                  \
s = alloc((void**)&(ptr), (bytes), true); \
if (s != MC_OK) return s;
        A(pf_x, (size_t)cap * cfg.dim * tb);
        A(pf_xn, (size_t)cap * cfg.dim * tb);
        A(pf_h, (size_t)cap * cfg.dim * tb);
        A(pf_proj, (size_t)cap * cfg.dim * tb);
        A(pf_qkv, (size_t)cap * (H + 2 * KV) * hd * tb);
        A(pf_q, (size_t)cap * H * hd * tb);
        A(pf_att, (size_t)cap * H * hd * tb);
        A(pf_g2, (size_t)cap * 2 * cfg.ffn_dim * tb);
        A(pf_g, (size_t)cap * cfg.ffn_dim * tb);
        A(pf_tokens, (size_t)cap * 4);
#undef A
        pf_cap = cap;
    }
    if (tb == 2 && !pf_etab) {
        s = alloc((void**)&pf_etab, 65536 * sizeof(float), false);
        if (s != MC_OK) return s;
        s = launch("mc_exp_table_bfloat", 256, 1, 1, 256, 0, pack(pf_etab));
        if (s != MC_OK) return s;
    }
    if (tb == 2 && cfg.family == MC_FAMILY_GEMMA3 && !pf_gtab && opt.pf_gelu_table) {
        s = alloc((void**)&pf_gtab, 65536 * sizeof(float), false);
        if (s != MC_OK) return s;
        s = launch("mc_gelu_table_bfloat", 256, 1, 1, 256, 0, pack(pf_gtab));
        if (s != MC_OK) return s;
    }
    const size_t need = (tb == 2 && !opt.pf_two_pass) ? 0 : (size_t)H * M * S;
    return grow(&pf_probs, &pf_probs_elems, need, tb);
}

// Y[M, L.out] = T(X[M, L.in] Wd^T) (+ res): the fused matrices of the decode GEMV, same HBM layout.  Which kernel multiplies, with what tiles and K
// ranges, is decided in prefill_plan.h (plan_gemm); here are the derived copies of a matrix the plan may multiply from: the quad-interleaved int4
// copy of short prompts ...
mc_status
mc_decoder::ensure_pf2(const linear_w& Lc)
{
    linear_w& L = const_cast<linear_w&>(Lc);
    if (L.wq2 && L.wq2_gen == weights_gen) return MC_OK;
    const size_t bytes = (size_t)((L.out + 15) / 16) * (size_t)(L.in / 128) * 1024;
    if (!L.wq2) {
        mc_status s = alloc(&L.wq2, bytes, false);
        if (s != MC_OK) return s;
    }
    mc_status s = launch("mc_pf2_repack_i4", 2048, 1, 1, 256, 0, pack((const void*)L.w, L.wq2, (uint32_t)L.out, (uint32_t)L.in));
    if (s != MC_OK) return s;
    L.wq2_gen = weights_gen;
    return MC_OK;
}

// ... and the quantised matrices of long prompts as dequantised bfloat16 copies (opt.pf_plain_mode)
bool
mc_decoder::plain_copy_ok()
{
    if (!pf_plain_known) {
        pf_plain_known = true;
        if (opt.pf_plain_mode >= 0) pf_plain_on = opt.pf_plain_mode != 0;
        else {
            size_t need = 0;
            auto one = [&](const linear_w& L) {
                if (L.fmt != MC_WFMT_T) need += (size_t)L.out * L.in * 2;
            };
            for (const layer_w& L : layers) {
                one(L.qkv);
                one(L.wo);
                one(L.w13);
                one(L.w2);
            }
            size_t free_b = 0, total_b = 0;
            if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) free_b = 0;
            pf_plain_on = need > 0 && need <= dev->prop.totalGlobalMem / 8 && need <= free_b / 2; // (and half of what is free NOW: other decoders share the device)
        }
    }
    return pf_plain_on;
}

mc_status
mc_decoder::ensure_wd(const linear_w& Lc, const void** wd)
{
    linear_w& L = const_cast<linear_w&>(Lc);
    if (L.fmt == MC_WFMT_T) {
        *wd = L.w;
        return MC_OK;
    }
    if (!(L.wd && L.wd_gen == weights_gen)) {
        if (!L.wd) {
            mc_status s = alloc(&L.wd, (size_t)L.out * L.in * 2, false);
            if (s != MC_OK) return s;
        }
        mc_status s = launch(L.fmt == MC_WFMT_I4 ? "mc_pf_dequant_rows_i4_bfloat" : "mc_pf_dequant_rows_i8_bfloat", (L.in / 16 + 255) / 256,
                             L.out, 1, 256, 0, pack((const void*)L.w, (const void*)L.scales, L.wd, (uint32_t)L.out, (uint32_t)L.in, (uint32_t)L.group));
        if (s != MC_OK) return s;
        L.wd_gen = weights_gen;
    }
    *wd = L.wd;
    return MC_OK;
}

mc_decoder::gemm_done
mc_decoder::gemm_run(const linear_w& L, int epi, const void* X, void* Y, const void* res, int M)
{
    const bool stop = epi == 2;
    gemm_plan P = plan_gemm(L, M, epi);
    if (P.fam == gemm_family::lib) {
        // (the library GEMM leaves its fp32 sums as the ONE partial the consumers add up)
        mc_status s = stop ? grow((void**)&pf_part, &pf_part_elems, (size_t)M * L.out, 4) : MC_OK;
        if (s != MC_OK) return {s, 1};
        if (gemm_lib(L, X, stop ? (void*)pf_part : Y, M, stop)) return {MC_OK, 1};
        P = plan_gemm(L, M, epi); // (pf_lib_on went false for good: the prompt kernels take over)
    }
    if (stop && P.splits < 2) return {MC_OK, 0};
    const bool parts = P.writes_partials();
    mc_status s = parts ? grow((void**)&pf_part, &pf_part_elems, (size_t)P.splits * M * L.out, 4) : MC_OK;
    if (s != MC_OK) return {s, P.splits};
    // the kernel writes T rows with the caller's epilogue, or fp32 partials (e2: no residual, no adaptor -- the reduce carries them)
    void* dst = parts ? (void*)pf_part : Y;
    const void* kres = parts ? nullptr : res;
    const bool lora = L.lora_cols != 0;
    const void *la = lora ? (const void*)pf_lora : nullptr, *lb = lora ? (const void*)L.lora_b : nullptr;
    const float lscale = lora ? L.lora_scale : 0.0f;
    const void *kla = parts ? nullptr : la, *klb = parts ? nullptr : lb;
    const uint32_t kcols = parts ? 0u : (uint32_t)L.lora_cols;
    const float kscale = parts ? 0.0f : lscale;
    switch (P.fam) {
    case gemm_family::stream:
        s = ensure_pf2(L);
        if (s != MC_OK) break;
        s = launch(P.kernel(parts), P.gx, P.gy, P.splits, P.block, 0,
                   pack((const void*)L.wq2, (const void*)L.scales, X, dst, (uint32_t)M, (uint32_t)L.out, (uint32_t)L.in, P.ktper));
        break;
    case gemm_family::g8: {
        // (round 6) the quantised matrices of long prompts as dequantised bfloat16 copies where memory allows (plain_copy_ok)
        const void *w = L.w, *sc = L.scales, *wd = nullptr;
        uint32_t group = (uint32_t)L.group;
        if (L.fmt != MC_WFMT_T && plain_copy_ok()) {
            if (ensure_wd(L, &wd) == MC_OK) {
                w = wd;
                sc = nullptr;
                group = 0;
            } else {
                pf_plain_on = false; // (no memory for the copy: the quantised rows from here on)
                (void)hipGetLastError(); // (the failed allocation's residue: RCCL reads it between its own calls)
            }
        }
        s = launch(P.kernel(parts, wd != nullptr), P.gx, P.gy, P.splits, P.block, 0,
                   pack(w, sc, X, dst, kres, (uint32_t)M, (uint32_t)L.out, (uint32_t)L.in, group, (const void*)nullptr, (const void*)nullptr,
                        (uint32_t)0, 0.0f));
        break;
    }
    default: // tiled, tile64
        s = launch(P.kernel(parts), P.gx, P.gy, P.splits, P.block, 0,
                   pack(L.w, L.scales, X, dst, kres, (uint32_t)M, (uint32_t)L.out, (uint32_t)L.in, (uint32_t)L.group, kla, klb, kcols, kscale));
    }
    if (s != MC_OK || stop || !parts) return {s, P.splits};
    s = launch("mc_pf_splitk_reduce_" + tname, (L.out + 255) / 256, M, 1, 256, 0,
               pack((const void*)pf_part, Y, epi == 1 ? res : (const void*)nullptr, (uint32_t)M, (uint32_t)L.out, P.splits, la, lb,
                    (uint32_t)L.lora_cols, lscale));
    return {s, P.splits};
}

// A prompt GEMM that splits K, stopped at its fp32 partial sums: the kernel that consumes the rows adds them itself
// (prefill_kernels.hip mc_pf_*_parts_bfloat) and the reduce launch is saved.  splits 0: this matrix at this M does not split
// (or carries an adaptor, or T = float): the caller takes gemm().
mc_decoder::gemm_done
mc_decoder::gemm_to_parts(const linear_w& L, const void* X, int M)
{
    if (!fold_parts_ok(shape_of(L), penv())) return {MC_OK, 0};
    return gemm_run(L, 2, X, nullptr, nullptr, M);
}

mc_status
mc_decoder::gemm(const linear_w& L, int epi, const void* X, void* Y, const void* res, int M)
{
    if (L.lora_cols) {
        // la = T(X A^T): the stacked adaptor inputs, [M][nseg * rank]
        mc_status s = grow(&pf_lora, &pf_lora_elems, (size_t)M * L.lora_cols, tb);
        if (s != MC_OK) return s;
        s = gemm(*L.lora_a, 0, X, pf_lora, nullptr, M);
        if (s != MC_OK) return s;
    }
    return gemm_run(L, epi, X, Y, res, M).st;
}

mc_status
mc_decoder::norm_rows(const void* x, const void* w, const void* res, void* y, int M, float mu)
{
    return launch("mc_pf_rmsnorm_" + tname, M, 1, 1, 256, 0,
                  pack(x, w, res, y, (uint32_t)cfg.dim, cfg.norm_eps, mu));
}

// wq|wk|wv of the M rows in pf_xn, then rope + cache write (q rows into pf_q, k and v into kc / vt) in the one form that fits -- packed / tree (pk), four
// pairs per thread, one pair -- reading the GEMM's rows (pf_qkv) or, where it split K, its partial sums
mc_status
mc_decoder::qkv_rope_cache(const layer_w& L, void* kc, void* vt, int M, int start_pos, int rope_pos, float mu, const packed_prefill* pk)
{
    const int H = cfg.n_heads, KV = cfg.n_kv_heads, hd = cfg.head_dim;
    const gemm_done g = gemm_to_parts(L.qkv, pf_xn, M);
    if (g.st != MC_OK) return g.st;
    const bool parts = g.splits > 0;
    if (!parts) {
        mc_status s = timed("gemm_qkv", [&] { return gemm(L.qkv, 0, pf_xn, pf_qkv, nullptr, M); });
        if (s != MC_OK) return s;
    }
    // rope + cache write in the form and grid prefill_plan.h plan_rope gives
    const rope_plan R = plan_rope(penv(), M, parts, pk ? (pk->nodes ? 2 : 1) : 0, L.q_norm || L.k_norm);
    arg_pack a = parts ? pack((const void*)pf_part, g.splits, (uint32_t)M, pf_q) : (pk ? pack((const void*)pf_qkv, (uint32_t)M, pf_q) : pack(pf_qkv, pf_q));
    switch (R.form) {
    case rope_form::packed:
    case rope_form::tree: // (kc, vt: this layer of every batch row)
        push_all(a, pk->segs, (uint32_t)pk->nseg, kc, vt, pk->cache_stride, pk->fcos, pk->fsin, (uint32_t)H, (uint32_t)KV, (uint32_t)hd,
                 (uint32_t)cfg.max_seq_len);
        if (pk->nodes) a.push(pk->nodes);
        break;
    case rope_form::v4:
        push_all(a, kc, vt, rope_cos[L.rope_table], rope_sin[L.rope_table], (uint32_t)H, (uint32_t)KV, (uint32_t)hd, (uint32_t)cfg.max_seq_len,
                 (uint32_t)start_pos, (uint32_t)(rope_pos - rope_start));
        if (!parts) a.push((uint32_t)M);
        push_all(a, L.q_norm, L.k_norm, cfg.norm_eps, mu);
        break;
    case rope_form::pair:
        push_all(a, kc, vt, rope_cos[L.rope_table], rope_sin[L.rope_table], L.q_norm, L.k_norm, (uint32_t)H, (uint32_t)KV, (uint32_t)hd,
                 (uint32_t)cfg.max_seq_len, (uint32_t)start_pos, (uint32_t)(rope_pos - rope_start), cfg.norm_eps, mu);
    }
    return timed("rope_cache", [&] { return launch(R.name, R.gx, R.gy, 1, R.block, 0, std::move(a)); });
}

// Wo and w2: out = T(res + y), y = T(X W^T) or gemma3's post norm of it (post_w; null: llama) -- and where the GEMM splits K its
// reduce, the residual and the NEXT rmsnorm (next_w) of out into pf_xn are the one launch that consumes the partial sums.
// *xn_done: pf_xn was written.  label: the timed() category of the GEMM where it is a launch of its own.
mc_status
mc_decoder::gemm_residual(const linear_w& W, const void* X, const void* res, void* out, const void* post_w, const void* next_w, const char* label, int M, float mu,
              bool* xn_done)
{
    const int dim = cfg.dim;
    *xn_done = false;
    // the reduce of a split Wo / w2, the residual and the norm(s) behind it in one launch where prefill_plan.h fold_norm_ok allows:
    // llama: h = T(x + T(sum of the partials)) -> out, rmsnorm(h) -> pf_xn; gemma3: the post norm in front of the residual too
    const bool fold = fold_norm_ok(penv(), post_w != nullptr, next_w != nullptr);
    const gemm_done g = fold ? gemm_to_parts(W, X, M) : gemm_done{MC_OK, 0};
    if (g.st != MC_OK) return g.st;
    if (g.splits) {
        *xn_done = next_w != nullptr;
        arg_pack a = pack((const void*)pf_part, g.splits, (uint32_t)M, res, out);
        if (post_w) a.push(post_w);
        push_all(a, next_w, pf_xn, (uint32_t)dim, cfg.norm_eps, mu);
        return timed("norm", [&] { return launch(post_w ? "mc_pf_rmsnorm2_parts_bfloat" : "mc_pf_rmsnorm_parts_" + tname, M, 1, 1, 256, 0, std::move(a)); });
    }
    if (!post_w) return timed(label, [&] { return gemm(W, 1, X, out, res, M); });
    mc_status s = timed(label, [&] { return gemm(W, 0, X, pf_proj, nullptr, M); });
    if (s != MC_OK) return s;
    return norm_rows(pf_proj, post_w, res, out, M, mu);
}

// nn::llama3 / nn::gemma3 operator() on M > 1 rows (llama.h:113-134, gemma.h:110-137)
// cache_pos: first cache row (= logical column) the M rows are written to; rope_pos: their sequence position
// (they differ for a chunk behind a full cache: rows max_seq_len - M .., positions start_pos ..);
// rows_in: hidden rows [M][dim] from the previous pipeline stage (device), null on the first stage
// pk (mc_rows_prefill): the M rows are the chunks of several batch rows (decoder_batch.h packed_prefill) -- the rope + cache
// write and the attention take the packed kernels (kernels/packed_kernels.hip) on the batch's caches and rope table, the
// taps and the head are skipped, and the last row of each chunk is gathered into pk->x_out.  cache_pos, rope_pos and window
// are not used then.
mc_status
mc_decoder::run_prefill(int M, int cache_pos, int rope_pos, int window, const void* rows_in, const packed_prefill* pk)
{
    const int dim = cfg.dim, H = cfg.n_heads, KV = cfg.n_kv_heads, hd = cfg.head_dim;
    const int start_pos = cache_pos;
    const int S = start_pos + M;
    const bool gemma = cfg.family == MC_FAMILY_GEMMA3;
    const float mu = gemma ? 1.0f : 0.0f;
    const float scale_T = tb == 2 ? bf2f_host(f2bf_host(cfg.attn_scale)) : cfg.attn_scale;
    float sc = std::sqrt((float)dim);
    if (tb == 2) sc = bf2f_host(f2bf_host(sc));
    mc_status s;
    const unsigned gd = (dim + 255) / 256;
    if (!first_stage) {
        MC_HIP(hipMemcpyAsync(pf_x, rows_in, (size_t)M * dim * tb, hipMemcpyDeviceToDevice, stream));
        s = MC_OK;
    } else if (emb_fmt == MC_WFMT_T)
        s = launch("mc_pf_embed_" + tname, gd, M, 1, 256, 0,
                   pack(emb_table, pf_tokens, pf_x, (uint32_t)dim, sc, (int32_t)(gemma ? 1 : 0)));
    else
        s = launch("mc_pf_embed_q8_" + tname, gd, M, 1, 256, 0,
                   pack(emb_table, emb_scales, pf_tokens, pf_x, (uint32_t)dim, sc, (int32_t)(gemma ? 1 : 0)));
    if (s != MC_OK) return s;
    const size_t last = (size_t)(M - 1) * dim * tb;
    const bool taps_on = want_taps && !pk;
    if (taps_on) MC_HIP(hipMemcpyAsync(taps, (char*)pf_x + last, (size_t)dim * tb, hipMemcpyDeviceToDevice, stream));
    // (round 4) a GEMM that splits K hands its fp32 partial sums straight to the kernel that consumes its rows -- rope + cache
    // write, the next rmsnorm (with the residual), act * mul -- instead of to a reduce launch: gemm_to_parts
    bool xn_ready = false; // pf_xn already holds this block's normalised input (the previous block's w2 consumer wrote it)
    for (int li = 0; li < n_own; li++) {
        layer_w& L = layers[li];
        if (!xn_ready) {
            s = timed("norm", [&] { return norm_rows(pf_x, L.attention_norm, nullptr, pf_xn, M, mu); });
            if (s != MC_OK) return s;
        }
        xn_ready = false;
        // packed rows: layer li of every batch row's caches
        void* pk_kc = pk ? (char*)pk->kc + (size_t)li * pk->B * pk->cache_stride * tb : nullptr;
        void* pk_vt = pk ? (char*)pk->vt + (size_t)li * pk->B * pk->cache_stride * tb : nullptr;
        s = qkv_rope_cache(L, pk ? pk_kc : L.kc, pk ? pk_vt : L.vt, M, start_pos, rope_pos, mu, pk);
        if (s != MC_OK) return s;
        const uint32_t win = (gemma && L.rope_table == 1) ? (uint32_t)window : 0u;
        if (pk && pk->extend) {
            // chunks that see their context (mc_extend_rows, kernels/extend_kernels.hip): the exp sums of every key range, then
            // p V over the ranges, then the ranges of a tile added in order (names and heads per workgroup: prefill_plan.h
            // plan_extend_attention).  A group is as many whole tiles as the scratch holds (one group unless the call is huge).
            // Chunks that are trees (mc_tree_verify, pk->nodes): the mc_tv_* forms of the first two, the node table behind their arguments.
            s = timed("attention", [&] {
                const extend_plan E = plan_extend_attention(penv(), pk->nodes != nullptr);
                for (int g = 0; g < pk->ngroups; g++) {
                    const uint32_t e0 = (uint32_t)pk->groups[g].first, ne = (uint32_t)pk->groups[g].count;
                    arg_pack as = pack(pf_q, pk->segs, pk->ranges, e0, (const void*)pk_kc, pk->cache_stride, pk->sums, (uint32_t)H,
                                       (uint32_t)(H / KV), (uint32_t)cfg.max_seq_len, scale_T, (const void*)pf_etab);
                    if (pk->nodes) as.push(pk->nodes);
                    mc_status ls = launch(E.sums, E.heads, ne, 1, 256, 0, std::move(as));
                    if (ls != MC_OK) return ls;
                    arg_pack ap = pack(pf_q, pk->segs, pk->ranges, e0, (const void*)pk_kc, (const void*)pk_vt, pk->cache_stride,
                                       (const void*)pk->sums, pk->part, pf_att, (uint32_t)H, (uint32_t)(H / KV), (uint32_t)cfg.max_seq_len, scale_T,
                                       (const void*)pf_etab);
                    if (pk->nodes) ap.push(pk->nodes);
                    ls = launch(E.pv, E.heads, ne, 1, 256, 0, std::move(ap));
                    if (ls != MC_OK) return ls;
                    if (!pk->groups[g].split) continue; // no tile of the group is split: mc_px_pv wrote the outputs
                    ls = launch(E.reduce, H, ne, 1, 256, 0,
                                pack(pk->segs, pk->ranges, e0, (const void*)pk->part, pf_att, (uint32_t)H));
                    if (ls != MC_OK) return ls;
                }
                return mc_status(MC_OK);
            });
            if (s != MC_OK) return s;
        } else if (pk) {
            // (prefill_plan.h plan_packed_attention: the two-heads rule of one prompt over the tiles of all segments)
            s = timed("attention", [&] {
                const attn_plan A = plan_packed_attention(penv(), pk->ntiles);
                return launch(A.name, A.gx, A.gy, 1, A.block, 0,
                              pack(pf_q, pk->segs, pk->tiles, (const void*)pk_kc, (const void*)pk_vt, pk->cache_stride, pf_att, (uint32_t)H,
                                   (uint32_t)(H / KV), (uint32_t)cfg.max_seq_len, scale_T, (const void*)pf_etab));
            });
            if (s != MC_OK) return s;
        } else if (tb == 2 && !opt.pf_two_pass) {
            // fused: the probabilities stay on chip
            s = timed("attention", [&] {
                const attn_plan A = plan_attention(penv(), M);
                return launch(A.name, A.gx, A.gy, 1, A.block, 0,
                              pack(pf_q, L.kc, L.vt, pf_att, (uint32_t)M, (uint32_t)S, (uint32_t)H, (uint32_t)(H / KV),
                                   (uint32_t)cfg.max_seq_len, scale_T, win, (const void*)pf_etab));
            });
            if (s != MC_OK) return s;
        } else {
            s = timed("scores", [&] { return launch("mc_pf_scores_" + tname, (M + 15) / 16, H, 1, 256, 0,
                       pack(pf_q, L.kc, pf_probs, (uint32_t)M, (uint32_t)S, (uint32_t)H, (uint32_t)(H / KV),
                            (uint32_t)hd, (uint32_t)cfg.max_seq_len, scale_T, win)); });
            if (s != MC_OK) return s;
            s = timed("pv", [&] { return launch("mc_pf_pv_" + tname, (M + 15) / 16, H, 1, 256, 0,
                       pack(pf_probs, L.vt, pf_att, (uint32_t)M, (uint32_t)S, (uint32_t)H, (uint32_t)(H / KV),
                            (uint32_t)hd, (uint32_t)cfg.max_seq_len, win)); });
            if (s != MC_OK) return s;
        }
        bool xn_done;
        s = gemm_residual(L.wo, pf_att, pf_x, pf_h, L.attention_post_norm, L.ffn_norm, "gemm_wo", M, mu, &xn_done);
        if (s != MC_OK) return s;
        if (!xn_done) s = timed("norm", [&] { return norm_rows(pf_h, L.ffn_norm, nullptr, pf_xn, M, mu); });
        if (s != MC_OK) return s;
        // (act(w1 x) * (w3 x) in the GEMM's epilogue was built -- the even lane of a column pair finishing it -- and measured
        //  SLOWER: 13.60 against 13.26 ms per 512-row prompt, 52.0 against 50.6 at 2048 rows: half the lanes idle through the
        //  fp64 exponential, in the kernel that holds the matrix pipe)
        const unsigned act_pp = 8u / (unsigned)tb; // pairs per thread (one 16-byte packet)
        // the activation in the epilogue of an unsplit w1|w3 GEMM where prefill_plan.h act_epi_ok allows (the table rides in `res`)
        const gemm_plan p13 = plan_gemm(L.w13, M, 0);
        const bool act_epi = act_epi_ok(shape_of(L.w13), penv(), p13, pf_gtab != nullptr);
        const void* act_tab = gemma ? (const void*)pf_gtab : (const void*)pf_etab; // (gelu without a table: nullptr, the kernels evaluate it)
        // (the library GEMM writes bfloat16 rows for the separate activation launch: half the bytes of fp32 partials)
        const gemm_done g13 = !act_epi && cfg.ffn_dim % 4 == 0 && p13.fam != gemm_family::lib ? gemm_to_parts(L.w13, pf_xn, M) : gemm_done{MC_OK, 0};
        if (g13.st != MC_OK) return g13.st;
        if (act_epi) {
            s = timed("gemm_w13_act", [&] { return gemm(L.w13, gemma ? 4 : 3, pf_xn, pf_g, act_tab, M); });
        } else if (g13.splits) {
            s = timed("act_mul", [&] { return launch("mc_pf_act_mul_parts_" + tname, (cfg.ffn_dim / 4 + 255) / 256 + 1, M, 1, 256, 0,
                       pack((const void*)pf_part, g13.splits, (uint32_t)M, pf_g, (uint32_t)cfg.ffn_dim, (int32_t)(gemma ? 1 : 0), act_tab)); });
        } else {
            s = timed("gemm_w13", [&] { return gemm(L.w13, 0, pf_xn, pf_g2, nullptr, M); });
            if (s != MC_OK) return s;
            s = timed("act_mul", [&] { return launch("mc_pf_act_mul_" + tname, (cfg.ffn_dim / act_pp + 255) / 256 + 1, M, 1, 256, 0,
                       tb == 2 ? pack(pf_g2, pf_g, (uint32_t)cfg.ffn_dim, (int32_t)(gemma ? 1 : 0), act_tab)
                               : pack(pf_g2, pf_g, (uint32_t)cfg.ffn_dim, (int32_t)(gemma ? 1 : 0))); });
        }
        if (s != MC_OK) return s;
        // x = T(h + ...) -> pf_x (the block's output), and the NEXT block's attention norm of it -> pf_xn where the fold wrote it
        const void* wn = li + 1 < n_own ? (const void*)layers[li + 1].attention_norm : (const void*)nullptr;
        s = gemm_residual(L.w2, pf_g, pf_h, pf_x, L.ffn_post_norm, wn, "gemm_w2", M, mu, &xn_ready);
        if (s != MC_OK) return s;
        if (taps_on)
            MC_HIP(hipMemcpyAsync((char*)taps + (size_t)(li + 1) * dim * tb, (char*)pf_x + last, (size_t)dim * tb,
                                  hipMemcpyDeviceToDevice, stream));
    }
    if (pk) {
        // the batch's head follows (batch_rows.cc): the last row of each chunk into its batch row
        s = launch("mc_pp_gather_last_bfloat", gd, (unsigned)pk->nseg, 1, 256, 0, pack((const void*)pf_x, pk->segs, pk->x_out, (uint32_t)dim));
        if (pk->rows_all) *pk->rows_all = pf_x;
        if (pk->tokens_dev) *pk->tokens_dev = pf_tokens;
    } else {
        // only the last row goes through the head (llama.h:130-133); other stages hand all rows on (pf_x)
        MC_HIP(hipMemcpyAsync(hidden, (char*)pf_x + last, (size_t)dim * tb, hipMemcpyDeviceToDevice, stream));
        s = last_stage ? timed("head", [&] { return run_head(); }) : MC_OK;
    }
    if (opt.pf_timing) {
        double tot = 0;
        for (auto& kv : pf_ms) tot += kv.second;
        fprintf(stderr, "[prefill M=%d] GPU ms:", M);
        for (auto& kv : pf_ms) fprintf(stderr, " %s %.2f", kv.first.c_str(), kv.second);
        fprintf(stderr, " | total %.2f\n", tot);
        pf_ms.clear();
    }
    return s;
}

extern "C" {

mc_status
mc_decoder_prefill_stage(mc_decoder* d, const int32_t* tokens, const void* rows_in, int32_t len, int32_t start_pos,
                         int32_t sliding_window, void** rows_out, int32_t* next_token)
{
    if (!d) return fail(MC_ERR_INVALID_ARGUMENT, "mc_decoder_prefill: null argument");
    if (d->first_stage ? !tokens : !rows_in)
        return fail(MC_ERR_INVALID_ARGUMENT, "mc_decoder_prefill: the first stage takes token ids, a later stage the inbound hidden rows");
    if (len < 1 || start_pos < 0) return fail(MC_ERR_INVALID_ARGUMENT, "mc_decoder_prefill: bad length or position");
    const int S = d->cfg.max_seq_len;
    if (len > S)
        return fail(MC_ERR_INVALID_ARGUMENT, "sink_cache: requested length (" + std::to_string(len) +
                                                 ") is larger than the cache size (" + std::to_string(S) + ")"); // nn/cache.h:178-183
    // nn::sink_cache::copy (nn/cache.h:187-213): a chunk either fits behind start_pos, or -- once start_pos has
    // left the cache -- the post-sink region is rotated left by len and the chunk takes the last len rows.  A chunk
    // that starts inside the cache and ends outside has no branch there (its slice runs past the tensor).
    const bool behind_full = start_pos >= S;
    if (!behind_full && start_pos + len > S)
        return fail(MC_ERR_INVALID_ARGUMENT, "sink_cache: rows [" + std::to_string(start_pos) + ", " + std::to_string(start_pos + len) +
                                                 ") straddle the end of the cache (" + std::to_string(S) + "): the reference clamps the "
                                                 "target slice and its clone kernel rejects the element counts "
                                                 "(kernel/copy.h:38-39); split the chunk at the cache size");
    if (d->first_stage)
        for (int i = 0; i < len; i++)
            if (tokens[i] < 0 || tokens[i] >= d->cfg.vocab)
                return fail(MC_ERR_INVALID_ARGUMENT, "decoder: token id outside the vocabulary");
    mc_status s = check_ready(d);
    if (s != MC_OK) return s;
    MC_HIP(hipSetDevice(d->dev->ordinal));
    if (len == 1 && d->first_stage && d->last_stage && !behind_full)
        return mc_decoder_step(d, tokens[0], start_pos, nullptr, next_token);
    const int cache_pos = behind_full ? S - len : start_pos;
    s = d->ensure_prefill(len, cache_pos + len);
    if (s != MC_OK) return s;
    // rope rows start_pos .. start_pos + len - 1 must lie inside the table window
    s = d->ensure_rope(start_pos, len);
    if (s != MC_OK) return s;
    if (start_pos == 0) d->ring_turned = false;
    // a ring that has turned is made linear again (the rotation by len of a chunk behind a full cache included),
    // so the prompt kernels keep addressing physical slot == logical column
    const bool rotate = d->n_own > 0 && (behind_full || d->ring_turned);
    if (rotate) {
        const mc_decoder_config& c = d->cfg;
        const size_t cache_bytes = (size_t)c.n_kv_heads * c.max_seq_len * c.head_dim * d->tb;
        if (!d->rot_k) {
            s = d->alloc(&d->rot_k, cache_bytes, false);
            if (s != MC_OK) return s;
            s = d->alloc(&d->rot_v, cache_bytes, false);
            if (s != MC_OK) return s;
        }
        for (auto& L : d->layers) {
            s = d->launch("mc_kv_rotate_" + d->tname, 1024, 1, 1, 256, 0,
                          pack((const void*)L.kc, (const void*)L.vt, d->rot_k, d->rot_v, d->state, (uint32_t)c.n_kv_heads,
                               (uint32_t)c.head_dim, (uint32_t)c.max_seq_len, (uint32_t)d->pre_len, (uint32_t)(behind_full ? len : 0)));
            if (s != MC_OK) return s;
            MC_HIP(hipMemcpyAsync(L.kc, d->rot_k, cache_bytes, hipMemcpyDeviceToDevice, d->stream));
            MC_HIP(hipMemcpyAsync(L.vt, d->rot_v, cache_bytes, hipMemcpyDeviceToDevice, d->stream));
        }
    }
    if (d->first_stage) MC_HIP(hipMemcpyAsync(d->pf_tokens, tokens, (size_t)len * 4, hipMemcpyHostToDevice, d->stream));
    // the state a following mc_decoder_step / _generate continues from: last row of the prompt
    s = d->launch("mc_step_after_prompt", 1, 1, 1, 64, 0,
                  pack(d->state, d->first_stage ? tokens[len - 1] : (int32_t)-1, (int32_t)(start_pos + len - 1), (int32_t)(cache_pos + len),
                       (int32_t)d->rope_start, (int32_t)(rotate || d->n_own == 0 ? 1 : 0), (int32_t)(start_pos == 0 ? 1 : 0)));
    if (s != MC_OK) return s;
    if (rotate) d->ring_turned = false; // linear again; the next step behind a full cache turns it anew
    s = d->run_prefill(len, cache_pos, start_pos, sliding_window, rows_in);
    if (s != MC_OK) return s;
    d->last_pos = start_pos + len - 1;
    if (rows_out) *rows_out = d->pf_x;
    MC_HIP(hipStreamSynchronize(d->stream)); // `tokens` is the caller's buffer
    if (next_token && d->last_stage) MC_HIP(hipMemcpy(next_token, &d->state->token, 4, hipMemcpyDeviceToHost));
    return d->check_err_synced(); // (the prompt pass has no hand-offs of its own: a step in front of it that nobody waited for)
}

mc_status
mc_decoder_prefill(mc_decoder* d, const int32_t* tokens, int32_t len, int32_t start_pos,
                   int32_t sliding_window, int32_t* next_token)
{
    if (!d || !tokens) return fail(MC_ERR_INVALID_ARGUMENT, "mc_decoder_prefill: null argument");
    if (!d->first_stage || !d->last_stage)
        return fail(MC_ERR_INVALID_ARGUMENT, "mc_decoder_prefill: a stage of a layer pipeline takes mc_decoder_prefill_stage / mc_pipeline_prefill");
    return mc_decoder_prefill_stage(d, tokens, nullptr, len, start_pos, sliding_window, nullptr, next_token);
}

} // extern "C"

namespace mcimpl {

mc_status
decoder_prefill_packed(mc_decoder* d, const int32_t* tokens, int M, const packed_prefill& pk)
{
    mc_status s = check_ready(d);
    if (s != MC_OK) return s;
    MC_HIP(hipSetDevice(d->dev->ordinal));
    if ((s = d->ensure_prefill(M, M)) != MC_OK) return s;
    MC_HIP(hipMemcpyAsync(d->pf_tokens, tokens, (size_t)M * 4, hipMemcpyHostToDevice, d->stream));
    return d->run_prefill(M, 0, 0, 0, nullptr, &pk);
}

} // namespace mcimpl
