// What the batched decode (batch_impl.h and its units, mc_batch_*) needs from a decoder (decoder.cc): the device addresses of its weights, norms,
// embedding, head and caches as they lie in HBM, its sampler settings, and its launch path (the launch log included).  Nothing
// here changes the decoder.
#pragma once

#include "backend_impl.h"
#include "kernels/abi.h"
#include "batch_plan.h" // linear_shape, decoder_sampler: what a batch launches, decided without a device
#include "rows_plan.h" // the tables of the packed prompt pass as the host builds them

namespace mcimpl {

using namespace mc::abi;

// one fused matrix as decoder.cc holds it: its shape (batch_plan.h linear_shape: all that the admission and the launch plans
// read) and where it lies -- rows [out][in] in MC_WFMT_* format, bfloat scales in row quads
struct batch_linear : linear_shape {
    const void* w = nullptr;
    const void* scales = nullptr;
    // its LoRA adaptor(s), when lora (mc_decoder_load_lora): the stacked A matrices, plain T [lora_cols][in]; B [out][lora_cols] of T in
    // fused row order, zeros outside a row's own adaptor columns; lora_cols = adaptors x rank
    const void* lora_a = nullptr;
    const void* lora_b = nullptr;
    float lora_scale = 0.0f;
};

struct batch_layer {
    batch_linear qkv, wo, w13, w2; // wq|wk|wv (q / k rows with the rotation partners adjacent), wo, w1/w3 interleaved, w2
    const void* attention_norm = nullptr;
    const void* ffn_norm = nullptr;
    const void* kc = nullptr; // the decoder's own cache: K [n_kv][max_seq][hd], V transposed [n_kv][hd][max_seq]
    const void* vt = nullptr;
};

struct decoder_parts {
    mc_decoder_config cfg{};
    int ordinal = 0;
    hipStream_t stream = nullptr;
    int pre_len = 0;
    int emb_fmt = MC_WFMT_T; // MC_WFMT_T table of T, or MC_WFMT_I8 + one f32 scale per row
    const void* emb_table = nullptr;
    const float* emb_scales = nullptr;
    batch_linear output;
    const void* final_norm = nullptr;
    std::vector<batch_layer> layers;
};

// fails with MC_ERR_RUNTIME when the decoder's weights are not all loaded
mc_status decoder_parts_of(mc_decoder* d, decoder_parts* out);
decoder_sampler decoder_sampler_of(const mc_decoder* d);
// the decoder's step state after everything enqueued so far (synchronises): valid cache rows and whether the ring has turned
mc_status decoder_cache_state(mc_decoder* d, int* kv_len, bool* rolled);
// a launch on the decoder's stream through its launch path (named ranges, mc_decoder_launch_log); args: the packed kernel arguments
mc_status decoder_launch(mc_decoder* d, const std::string& name, unsigned gx, unsigned gy, unsigned gz, unsigned bx, unsigned lds, arg_pack&& args);

// The packed prompt pass (mc_rows_prefill and mc_extend_rows, kernels/packed_kernels.hip): the chunks of several sequences as one prompt pass of
// M = sum of their lengths rows.  The tables are on the device already (uploaded on the decoder's stream).
// (px_group, a launch group of mc_extend_rows: rows_plan.h)
struct packed_prefill {
    const pp_seg* segs = nullptr;   // [nseg]: the rows in the call, offsets ascending
    int nseg = 0;
    const pp_tile* tiles = nullptr; // [ntiles]: the 16-row attention tiles of every segment
    int ntiles = 0;
    void* kc = nullptr;             // caches of layer l, batch row r at kc / vt + (l * B + r) * cache_stride elements (batch_impl.h kc_of / vt_of)
    void* vt = nullptr;
    int B = 0;
    uint64_t cache_stride = 0;
    const float* fcos = nullptr;    // the batch's rope table, rows = positions [0, max_seq_len)
    const float* fsin = nullptr;
    void* x_out = nullptr;          // [B][dim]: the last row of each segment lands in its batch row
    // mc_extend_rows (kernels/extend_kernels.hip): chunk rows see their row's whole context.  The attention then takes the
    // mc_px_* launches over the range table instead of mc_pp_attn* over the tile table.
    bool extend = false;
    const px_range* ranges = nullptr; // device: the key ranges of every tile, a tile's ranges adjacent
    const px_group* groups = nullptr; // HOST, [ngroups]: the launch groups
    int ngroups = 0;
    float* sums = nullptr;           // scratch [slots][n_heads][16]: the exp row sums of a range
    float* part = nullptr;           // scratch [slots][n_heads][16][head_dim]: the partial outputs of a range
    // mc_verify_rows: the head runs over every packed row.  When set they receive the device addresses of all M rows after the
    // last layer ([M][dim]) and of the call's M token ids -- the decoder's prompt scratch, valid until its next prompt pass.
    const void** rows_all = nullptr;
    const int32_t** tokens_dev = nullptr;
    // mc_tree_verify (kernels/tree_kernels.hip): the chunks are trees.  One tv_node per packed row, on the device; the rope + cache
    // write and the extend attention then take their mc_tv_* names, with the table as one more argument behind their own.
    const tv_node* nodes = nullptr;
};
// run_prefill over `tokens` (M ids, host) with the packed rope + cache and attention launches, then the gather into x_out; the
// decoder's cache, step state, sampler, taps and head are not touched (its prompt scratch is)
mc_status decoder_prefill_packed(mc_decoder* d, const int32_t* tokens, int M, const packed_prefill& pk);

} // namespace mcimpl
