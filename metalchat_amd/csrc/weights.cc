// The decoder's weights: the fused matrices of a block (wq|wk|wv, wo, w1|w3 interleaved, w2) and the head as they lie in HBM -- allocation,
// the repacking upload of reference-native rows, LoRA adaptors, norm vectors, the synthetic model -- and what the ABI tells about them.
#include "decoder_impl.h"
#include "kernels/synth.h"

using namespace mcimpl;

    // ---------------------------------------------------------------- weights

size_t
mc_decoder::row_bytes(int fmt, int in) const
{
    if (fmt == MC_WFMT_I4) return (size_t)in / 2;
    if (fmt == MC_WFMT_I8) return (size_t)in;
    return (size_t)in * tb;
}

mc_status
mc_decoder::alloc_linear(linear_w& L, int fmt, int out, int in, int group)
{
    if (L.allocated) {
        if (L.fmt != fmt || L.in != in || L.group != group)
            return fail(MC_ERR_INVALID_ARGUMENT,
                        "decoder: matrices fused into one GEMV must share format, in_features "
                        "and group size");
        return MC_OK;
    }
    if (in % 32 != 0)
        return fail(MC_ERR_INVALID_ARGUMENT, "decoder: in_features must be a multiple of 32");
    if (fmt != MC_WFMT_T && group != 0 && (group < 32 || (group & (group - 1)) != 0 || in % group != 0))
        return fail(MC_ERR_INVALID_ARGUMENT,
                    "decoder: group size must be a power of two >= 32 that divides in_features");
    L.fmt = fmt;
    L.out = out;
    L.in = in;
    L.group = group;
    L.ngroups = (fmt == MC_WFMT_T) ? 0 : (group ? in / group : 1);
    L.row_bytes = row_bytes(fmt, in);
    L.w_bytes = L.row_bytes * out;
    // scales live in row quads [ceil(out/4)][ngroups][4] (gemv.h)
    L.s_bytes = (size_t)L.ngroups * ((out + 3) / 4 * 4) * (tb == 2 ? 2 : 4);
    mc_status s = alloc(&L.w, L.w_bytes, false);
    if (s != MC_OK) return s;
    if (L.s_bytes) {
        s = alloc(&L.scales, L.s_bytes, false);
        if (s != MC_OK) return s;
    }
    L.allocated = true;
    return MC_OK;
}

// repack `rows` reference-native rows into the fused buffer at destination rows
// dst_row0 + i*dst_stride
mc_status
mc_decoder::upload_rows(linear_w& L, int dst_row0, int dst_stride, int rows, const void* weight,
            const float* scales, int perm_hd)
{
    // perm_hd != 0: the source is a q or k projection; natural row head*hd + j + e*hd/2 goes to
    // packed row head*hd + 2j + e (rotation partners adjacent, gemv.h EPI_QKV_ROPE)
    auto dest = [&](int r) -> size_t {
        if (!perm_hd) return (size_t)dst_row0 + (size_t)r * dst_stride;
        const int head = r / perm_hd, w = r % perm_hd, half = perm_hd / 2;
        return (size_t)dst_row0 + (size_t)head * perm_hd + 2 * (w % half) + w / half;
    };
    weights_gen++; // (derived copies of the weights -- linear_w::wq2 -- are rebuilt when next needed)
    const int in = L.in;
    const size_t sb = tb == 2 ? 2 : 4;
    const bool contiguous = dst_stride == 1; // destination rows form one block (maybe permuted)
    std::vector<uint8_t> stage(L.row_bytes * (contiguous ? rows : 1));
    // scales of the destination rows, scattered into the quad layout on the host first
    std::vector<uint8_t> squad;
    for (int r = 0; r < rows; r++) {
        uint8_t* dst = contiguous ? stage.data() + (dest(r) - dst_row0) * L.row_bytes : stage.data();
        if (L.fmt == MC_WFMT_T) {
            memcpy(dst, (const char*)weight + (size_t)r * in * tb, (size_t)in * tb);
        } else if (L.fmt == MC_WFMT_I8) {
            memcpy(dst, (const int8_t*)weight + (size_t)r * in, in);
        } else {
            // I4: offset-binary nibbles, nibble p of each dword = weight {0,2,4,6,1,3,5,7}[p]
            static const int perm[8] = {0, 2, 4, 6, 1, 3, 5, 7};
            const int8_t* src = (const int8_t*)weight + (size_t)r * in;
            uint32_t* d32 = reinterpret_cast<uint32_t*>(dst);
            for (int c0 = 0; c0 < in; c0 += 8) {
                uint32_t v = 0;
                for (int p = 0; p < 8; p++) {
                    const int q = src[c0 + perm[p]];
                    if (q < -8 || q > 7)
                        return fail(MC_ERR_INVALID_ARGUMENT,
                                    "decoder: int4 weight outside [-8, 7]");
                    v |= (uint32_t)(q + 8) << (4 * p);
                }
                d32[c0 / 8] = v;
            }
        }
        if (!contiguous) {
            const size_t drow = dest(r);
            MC_HIP(hipMemcpy((char*)L.w + drow * L.row_bytes, stage.data(), L.row_bytes,
                             hipMemcpyHostToDevice));
        }
    }
    if (contiguous)
        MC_HIP(hipMemcpy((char*)L.w + (size_t)dst_row0 * L.row_bytes, stage.data(), stage.size(),
                         hipMemcpyHostToDevice));
    if (L.ngroups) {
        // element (row, g) of the quad layout sits at ((row/4)*ngroups + g)*4 + row%4.  Rows of
        // different source matrices share quads (w1/w3), so the layout is edited in a host
        // shadow of the whole scale buffer and the touched quad range is re-uploaded.
        if (L.scales_host.size() != L.s_bytes) L.scales_host.assign(L.s_bytes, 0);
        size_t lo = SIZE_MAX, hi = 0;
        for (int r = 0; r < rows; r++) {
            const size_t drow = dest(r);
            for (int g = 0; g < L.ngroups; g++) {
                const float sc = scales[(size_t)r * L.ngroups + g];
                const size_t idx = ((drow / 4) * L.ngroups + g) * 4 + drow % 4;
                if (tb == 2) reinterpret_cast<uint16_t*>(L.scales_host.data())[idx] = f2bf_host(sc);
                else reinterpret_cast<float*>(L.scales_host.data())[idx] = sc;
            }
            const size_t q0 = (drow / 4) * L.ngroups * 4 * sb, q1 = q0 + (size_t)L.ngroups * 4 * sb;
            lo = q0 < lo ? q0 : lo;
            hi = q1 > hi ? q1 : hi;
        }
        MC_HIP(hipMemcpy((char*)L.scales + lo, L.scales_host.data() + lo, hi - lo, hipMemcpyHostToDevice));
    }
    return MC_OK;
}

namespace mcimpl {

size_t
linear_bytes(const linear_w& L)
{
    return L.allocated ? L.w_bytes + L.s_bytes : 0;
}

} // namespace mcimpl

extern "C" {

mc_status
mc_decoder_load_linear(mc_decoder* d, int32_t layer, const char* name, int32_t fmt,
                       int32_t out_f, int32_t in_f, int32_t group, const void* weight,
                       const float* scales)
{
    if (!d || !name || !weight) return fail(MC_ERR_INVALID_ARGUMENT, "mc_decoder_load_linear: null argument");
    if (fmt != MC_WFMT_T && !scales)
        return fail(MC_ERR_INVALID_ARGUMENT, "mc_decoder_load_linear: quantised weights need scales");
    MC_HIP(hipSetDevice(d->dev->ordinal));
    const mc_decoder_config& c = d->cfg;
    const std::string n = name;
    const int H = c.n_heads, KV = c.n_kv_heads, hd = c.head_dim;
    mc_status s;
    if (layer < 0) {
        if (n == "tok_embeddings") {
            if (out_f != c.vocab || in_f != c.dim)
                return fail(MC_ERR_INVALID_ARGUMENT, "decoder: tok_embeddings shape mismatch");
            if (fmt == MC_WFMT_T) {
                d->emb_fmt = MC_WFMT_T;
                s = d->alloc(&d->emb_table, (size_t)out_f * in_f * d->tb, false);
                if (s != MC_OK) return s;
                MC_HIP(hipMemcpy(d->emb_table, weight, (size_t)out_f * in_f * d->tb, hipMemcpyHostToDevice));
            } else {
                // lora_embedding: int8 + one f32 scale per row (quantization/lora.h:133-175)
                d->emb_fmt = MC_WFMT_I8;
                s = d->alloc(&d->emb_table, (size_t)out_f * in_f, false);
                if (s != MC_OK) return s;
                s = d->alloc((void**)&d->emb_scales, (size_t)out_f * 4, false);
                if (s != MC_OK) return s;
                MC_HIP(hipMemcpy(d->emb_table, weight, (size_t)out_f * in_f, hipMemcpyHostToDevice));
                MC_HIP(hipMemcpy(d->emb_scales, scales, (size_t)out_f * 4, hipMemcpyHostToDevice));
            }
            return MC_OK;
        }
        if (n == "output") {
            if (out_f != c.vocab || in_f != c.dim)
                return fail(MC_ERR_INVALID_ARGUMENT, "decoder: output shape mismatch");
            s = d->alloc_linear(d->output, fmt, out_f, in_f, group);
            if (s != MC_OK) return s;
            return d->upload_rows(d->output, 0, 1, out_f, weight, scales);
        }
        return fail(MC_ERR_INVALID_ARGUMENT, "decoder: unknown model-level linear '" + n + "'");
    }
    layer_w* L;
    s = find_layer(d, layer, &L);
    if (s != MC_OK) return s;
    struct slot { linear_w* lin; int total, row0, stride, rows, in, perm; };
    slot sl{};
    if (n == "wq") sl = {&L->qkv, (H + 2 * KV) * hd, 0, 1, H * hd, c.dim, hd};
    else if (n == "wk") sl = {&L->qkv, (H + 2 * KV) * hd, H * hd, 1, KV * hd, c.dim, hd};
    else if (n == "wv") sl = {&L->qkv, (H + 2 * KV) * hd, (H + KV) * hd, 1, KV * hd, c.dim, 0};
    else if (n == "wo") sl = {&L->wo, c.dim, 0, 1, c.dim, H * hd, 0};
    else if (n == "w1") sl = {&L->w13, 2 * c.ffn_dim, 0, 2, c.ffn_dim, c.dim, 0};
    else if (n == "w3") sl = {&L->w13, 2 * c.ffn_dim, 1, 2, c.ffn_dim, c.dim, 0};
    else if (n == "w2") sl = {&L->w2, c.dim, 0, 1, c.dim, c.ffn_dim, 0};
    else return fail(MC_ERR_INVALID_ARGUMENT, "decoder: unknown linear '" + n + "'");
    if (out_f != sl.rows || in_f != sl.in)
        return fail(MC_ERR_INVALID_ARGUMENT, "decoder: '" + n + "' shape mismatch");
    s = d->alloc_linear(*sl.lin, fmt, sl.total, sl.in, group);
    if (s != MC_OK) return s;
    return d->upload_rows(*sl.lin, sl.row0, sl.stride, sl.rows, weight, scales, sl.perm);
}

mc_status
mc_decoder_load_lora(mc_decoder* d, int32_t layer, const char* name, int32_t rank,
                     int32_t out_f, int32_t in_f, const void* a_T, const void* b_T, float scale)
{
    if (!d || !name || !a_T || !b_T) return fail(MC_ERR_INVALID_ARGUMENT, "mc_decoder_load_lora: null argument");
    if (rank <= 0 || rank % 8 != 0 || rank > 256)
        return fail(MC_ERR_INVALID_ARGUMENT, "decoder: LoRA rank must be a multiple of 8 in [8, 256]");
    MC_HIP(hipSetDevice(d->dev->ordinal));
    const mc_decoder_config& c = d->cfg;
    const std::string n = name;
    const int H = c.n_heads, KV = c.n_kv_heads, hd = c.head_dim;
    layer_w* L;
    mc_status s = find_layer(d, layer, &L);
    if (s != MC_OK) return s;
    struct slot { linear_w* lin; int total, row0, stride, rows, in, perm, seg, nseg; };
    slot sl{};
    if (n == "wq") sl = {&L->qkv, (H + 2 * KV) * hd, 0, 1, H * hd, c.dim, hd, 0, 3};
    else if (n == "wk") sl = {&L->qkv, (H + 2 * KV) * hd, H * hd, 1, KV * hd, c.dim, hd, 1, 3};
    else if (n == "wv") sl = {&L->qkv, (H + 2 * KV) * hd, (H + KV) * hd, 1, KV * hd, c.dim, 0, 2, 3};
    else if (n == "wo") sl = {&L->wo, c.dim, 0, 1, c.dim, H * hd, 0, 0, 1};
    else if (n == "w1") sl = {&L->w13, 2 * c.ffn_dim, 0, 2, c.ffn_dim, c.dim, 0, 0, 2};
    else if (n == "w3") sl = {&L->w13, 2 * c.ffn_dim, 1, 2, c.ffn_dim, c.dim, 0, 1, 2};
    else if (n == "w2") sl = {&L->w2, c.dim, 0, 1, c.dim, c.ffn_dim, 0, 0, 1};
    else return fail(MC_ERR_INVALID_ARGUMENT, "decoder: unknown linear '" + n + "'");
    if (out_f != sl.rows || in_f != sl.in)
        return fail(MC_ERR_INVALID_ARGUMENT, "decoder: '" + n + "' adaptor shape mismatch");
    linear_w& W = *sl.lin;
    const int cols = sl.nseg * rank;
    const size_t tb = d->tb;
    if (!W.lora_cols) {
        W.lora_a.reset(new linear_w());
        s = d->alloc_linear(*W.lora_a, MC_WFMT_T, cols, sl.in, 0);
        if (s != MC_OK) return s;
        MC_HIP(hipMemset(W.lora_a->w, 0, W.lora_a->w_bytes));
        s = d->alloc(&W.lora_b, (size_t)sl.total * cols * tb, true);
        if (s != MC_OK) return s;
        s = d->alloc(&W.lora_vec, (size_t)cols * tb, true);
        if (s != MC_OK) return s;
        W.lora_rank = rank;
        W.lora_cols = cols;
        W.lora_scale = scale;
    } else if (W.lora_rank != rank || W.lora_scale != scale) {
        return fail(MC_ERR_INVALID_ARGUMENT,
                    "decoder: adaptors of matrices fused into one GEMV must share rank and scale");
    }
    // A rows of this adaptor: block `seg` of the stacked matrix
    s = d->upload_rows(*W.lora_a, sl.seg * rank, 1, rank, a_T, nullptr);
    if (s != MC_OK) return s;
    // B[o][:] -> fused row dest(o), columns [seg*rank, (seg+1)*rank)
    auto dest = [&](int r) -> size_t {
        if (!sl.perm) return (size_t)sl.row0 + (size_t)r * sl.stride;
        const int head = r / sl.perm, w = r % sl.perm, half = sl.perm / 2;
        return (size_t)sl.row0 + (size_t)head * sl.perm + 2 * (w % half) + w / half;
    };
    if (W.lora_b_host.size() != (size_t)sl.total * cols * tb) W.lora_b_host.assign((size_t)sl.total * cols * tb, 0);
    for (int o = 0; o < sl.rows; o++)
        memcpy(W.lora_b_host.data() + (dest(o) * cols + (size_t)sl.seg * rank) * tb,
               (const char*)b_T + (size_t)o * rank * tb, (size_t)rank * tb);
    MC_HIP(hipMemcpy(W.lora_b, W.lora_b_host.data(), W.lora_b_host.size(), hipMemcpyHostToDevice));
    return MC_OK;
}

mc_status
mc_decoder_load_vector(mc_decoder* d, int32_t layer, const char* name, int32_t n, const void* data)
{
    if (!d || !name || !data) return fail(MC_ERR_INVALID_ARGUMENT, "mc_decoder_load_vector: null argument");
    MC_HIP(hipSetDevice(d->dev->ordinal));
    void** dst = nullptr;
    const std::string nm = name;
    int expect = d->cfg.dim;
    if (layer < 0) {
        if (nm == "norm") dst = &d->final_norm;
        else return fail(MC_ERR_INVALID_ARGUMENT, "decoder: unknown model-level vector '" + nm + "'");
    } else {
        layer_w* L;
        mc_status s = find_layer(d, layer, &L);
        if (s != MC_OK) return s;
        if (nm == "attention_norm") dst = &L->attention_norm;
        else if (nm == "ffn_norm") dst = &L->ffn_norm;
        else if (nm == "attention_post_norm") dst = &L->attention_post_norm;
        else if (nm == "ffn_post_norm") dst = &L->ffn_post_norm;
        else if (nm == "q_norm") { dst = &L->q_norm; expect = d->cfg.head_dim; }
        else if (nm == "k_norm") { dst = &L->k_norm; expect = d->cfg.head_dim; }
        else return fail(MC_ERR_INVALID_ARGUMENT, "decoder: unknown vector '" + nm + "'");
    }
    if (n != expect) return fail(MC_ERR_INVALID_ARGUMENT, "decoder: '" + nm + "' length mismatch");
    if (!*dst) {
        mc_status s = d->alloc(dst, (size_t)n * d->tb, false);
        if (s != MC_OK) return s;
    }
    MC_HIP(hipMemcpy(*dst, data, (size_t)n * d->tb, hipMemcpyHostToDevice));
    return MC_OK;
}

// matrix ids of the synthetic model: layer*16 + {0 wq,1 wk,2 wv,3 wo,4 w1,5 w2,6 w3,
// 8 attention_norm, 9 ffn_norm, 10 q_norm, 11 k_norm, 12 attention_post_norm, 13 ffn_post_norm};
// 0xFFFF0000 + {0 tok_embeddings, 1 output, 2 norm}
mc_status
mc_decoder_init_synthetic(mc_decoder* d, uint64_t seed)
{
    if (!d) return fail(MC_ERR_INVALID_ARGUMENT, "mc_decoder_init_synthetic: null argument");
    MC_HIP(hipSetDevice(d->dev->ordinal));
    d->weights_gen++;
    const mc_decoder_config& c = d->cfg;
    const int H = c.n_heads, KV = c.n_kv_heads, hd = c.head_dim;
    const int fmt = c.weight_format;
    const int bits = fmt == MC_WFMT_I4 ? 4 : 8;
    const int group = c.group_size;
    mc_status s;
    auto fill_linear = [&](linear_w& L, int out, int in, uint32_t m0, uint32_t map, uint32_t n0,
                           uint32_t n1) -> mc_status {
        mc_status r = d->alloc_linear(L, fmt, out, in, group);
        if (r != MC_OK) return r;
        if (fmt == MC_WFMT_T) {
            return d->launch("mc_synth_fill_T", 2048, 1, 1, 256, 0,
                             pack(L.w, seed, m0, map, n0, n1, (uint32_t)out, (uint32_t)in, (int32_t)2,
                                  (int32_t)d->tb));
        }
        r = d->launch("mc_synth_fill_q", 4096, 1, 1, 256, 0,
                      pack(L.w, seed, m0, map, n0, n1, (uint32_t)out, (uint32_t)in, (int32_t)bits));
        if (r != MC_OK) return r;
        return d->launch("mc_synth_fill_scales", 1024, 1, 1, 256, 0,
                         pack(L.scales, seed, m0, map, n0, n1, (uint32_t)out, (uint32_t)L.ngroups,
                              (uint32_t)in, (int32_t)bits, (int32_t)(d->tb == 2 ? 2 : 4)));
    };
    auto fill_vec = [&](void** p, int n, uint32_t m) -> mc_status {
        if (!*p) {
            mc_status r = d->alloc(p, (size_t)n * d->tb, false);
            if (r != MC_OK) return r;
        }
        return d->launch("mc_synth_fill_T", (n + 255) / 256, 1, 1, 256, 0,
                         pack(*p, seed, m, (uint32_t)0, (uint32_t)0, (uint32_t)0, (uint32_t)1,
                              (uint32_t)n, (int32_t)0, (int32_t)d->tb));
    };
    for (int i = 0; i < d->n_own; i++) {
        layer_w& L = d->layers[i];
        const uint32_t base = (uint32_t)(c.layer_begin + i) * 16;
        s = fill_linear(L.qkv, (H + 2 * KV) * hd, c.dim, base + 0, 1u | ((uint32_t)hd << 8), H * hd, KV * hd);
        if (s != MC_OK) return s;
        s = fill_linear(L.wo, c.dim, H * hd, base + 3, 0, 0, 0);
        if (s != MC_OK) return s;
        s = fill_linear(L.w13, 2 * c.ffn_dim, c.dim, base + 4, 2, 0, 0);
        if (s != MC_OK) return s;
        s = fill_linear(L.w2, c.dim, c.ffn_dim, base + 5, 0, 0, 0);
        if (s != MC_OK) return s;
        s = fill_vec(&L.attention_norm, c.dim, base + 8);
        if (s != MC_OK) return s;
        s = fill_vec(&L.ffn_norm, c.dim, base + 9);
        if (s != MC_OK) return s;
        if (c.family == MC_FAMILY_GEMMA3) {
            s = fill_vec(&L.q_norm, hd, base + 10);
            if (s != MC_OK) return s;
            s = fill_vec(&L.k_norm, hd, base + 11);
            if (s != MC_OK) return s;
            s = fill_vec(&L.attention_post_norm, c.dim, base + 12);
            if (s != MC_OK) return s;
            s = fill_vec(&L.ffn_post_norm, c.dim, base + 13);
            if (s != MC_OK) return s;
        }
    }
    if (d->first_stage) {
        d->emb_fmt = MC_WFMT_T;
        if (!d->emb_table) {
            s = d->alloc(&d->emb_table, (size_t)c.vocab * c.dim * d->tb, false);
            if (s != MC_OK) return s;
        }
        s = d->launch("mc_synth_fill_T", 4096, 1, 1, 256, 0,
                      pack(d->emb_table, seed, (uint32_t)0xFFFF0000u, (uint32_t)0, (uint32_t)0,
                           (uint32_t)0, (uint32_t)c.vocab, (uint32_t)c.dim, (int32_t)1, (int32_t)d->tb));
        if (s != MC_OK) return s;
    }
    if (d->last_stage) {
        s = fill_linear(d->output, c.vocab, c.dim, 0xFFFF0001u, 0, 0, 0);
        if (s != MC_OK) return s;
        s = fill_vec(&d->final_norm, c.dim, 0xFFFF0002u);
        if (s != MC_OK) return s;
    }
    MC_HIP(hipStreamSynchronize(d->stream));
    return MC_OK;
}

size_t
mc_decoder_derived_weight_bytes(const mc_decoder* d)
{
    if (!d) return 0;
    size_t n = 0;
    auto one = [&](const linear_w& L) {
        if (L.wq2) n += (size_t)((L.out + 15) / 16) * (size_t)(L.in / 128) * 1024;
        if (L.wd) n += (size_t)L.out * L.in * 2;
    };
    for (const layer_w& L : d->layers) {
        one(L.qkv);
        one(L.wo);
        one(L.w13);
        one(L.w2);
    }
    one(d->output);
    return n;
}

size_t
mc_decoder_weight_bytes(const mc_decoder* d)
{
    size_t n = 0;
    for (auto& L : d->layers) n += linear_bytes(L.qkv) + linear_bytes(L.wo) + linear_bytes(L.w13) + linear_bytes(L.w2);
    if (d->last_stage) n += linear_bytes(d->output);
    return n;
}

// tests: direct access to the fused weight buffers ("qkv","wo","w13","w2" per layer, "output")
mc_status
mc_decoder_weight_ptrs(mc_decoder* d, int32_t layer, const char* name, void** w, void** scales,
                       int32_t* rows, int32_t* in_features, int32_t* ngroups)
{
    const linear_w* L = nullptr;
    const std::string n = name;
    if (layer < 0) {
        if (n == "output") L = &d->output;
    } else {
        layer_w* lw;
        mc_status s = find_layer(d, layer, &lw);
        if (s != MC_OK) return s;
        if (n == "qkv") L = &lw->qkv;
        else if (n == "wo") L = &lw->wo;
        else if (n == "w13") L = &lw->w13;
        else if (n == "w2") L = &lw->w2;
    }
    if (!L || !L->allocated) return fail(MC_ERR_INVALID_ARGUMENT, "decoder: no such fused weight '" + n + "'");
    if (w) *w = L->w;
    if (scales) *scales = L->scales;
    if (rows) *rows = L->out;
    if (in_features) *in_features = L->in;
    if (ngroups) *ngroups = L->ngroups;
    return MC_OK;
}

int32_t
mc_synth_weight(uint64_t seed, uint32_t matrix_id, uint32_t row, uint32_t col, int32_t bits)
{
    return mcsynth::weight(seed, matrix_id, row, col, bits);
}

float
mc_synth_scale(uint64_t seed, uint32_t matrix_id, uint32_t row, uint32_t group, int32_t in_features,
               int32_t bits)
{
    return mcsynth::scale(seed, matrix_id, row, group, in_features, bits);
}

float
mc_synth_value(uint64_t seed, uint32_t matrix_id, uint32_t index, int32_t kind, uint32_t n)
{
    return mcsynth::value(seed, matrix_id, index, kind, n ? n : 1);
}

} // extern "C"
