// The packed prompt pass (mc_rows_prefill, include/metalchat_hip.h Part 2d): the prompts of several rows of an mc_batch as ONE
// prompt pass of M = sum of their lengths rows over the decoder's weights.  Embedding, norms, GEMMs, act * mul and residuals work
// row by row and run unchanged (decoder.cc run_prefill); only the two launches that know which sequence a row belongs to are
// here: rope + cache write, and the causal attention.  Both are the one-prompt kernels' device bodies (prefill_kernels.hip) with
// per-row cache bases and positions, so every value is rounded where the one-prompt pass rounds it.
//
// The segment table: one pp_seg per row in the call, in packed order (offsets ascending, lengths >= 2).  Row `row` of the batch
// owns the caches kc + row * cache_stride ([n_kv][max_seq][hd]) and vt + row * cache_stride ([n_kv][hd][max_seq]) of a layer,
// and its chunk sits at positions [pos, pos + len) -- cache slots and rope table rows alike (a batch's cache does not roll and
// its rope table starts at position 0).

// (pp_seg and pp_tile: abi.h)

// pf_rope_cache_v4_body's row map over the segment table: packed row r -> (its row's caches, slot, rope row)
struct pp_rows {
    const pp_seg* segs;
    uint32_t nseg;
    bf16_t* kc;
    bf16_t* vt;
    uint64_t cache_stride;
    __device__ __forceinline__ void
    at(uint32_t r, bf16_t*& k, bf16_t*& v, uint32_t& slot, uint32_t& rope_row) const
    {
        uint32_t s = 0;
        while (s + 1 < nseg && r >= (uint32_t)segs[s + 1].off) s++;
        const pp_seg g = segs[s];
        k = kc + (size_t)g.row * cache_stride;
        v = vt + (size_t)g.row * cache_stride;
        slot = (uint32_t)g.pos + (r - (uint32_t)g.off);
        rope_row = slot;
    }
};

// grid and rows as mc_pf_rope_cache_v4_bfloat / mc_pf_rope_cache_parts_v4_bfloat over the M packed rows; the V tiles of 16 rows may
// straddle two segments (each thread writes its own row's slot)
extern "C" __global__ void __launch_bounds__(256)
mc_pp_rope_cache_bfloat(const bf16_t* qkv, uint32_t M, bf16_t* q_out, const pp_seg* segs, uint32_t nseg, bf16_t* kc, bf16_t* vt,
                        uint64_t cache_stride, const float* fcos, const float* fsin, uint32_t H, uint32_t KV, uint32_t hd, uint32_t max_seq)
{
    pf_rope_cache_v4_body<false>(qkv, 1, M, q_out, pp_rows{segs, nseg, kc, vt, cache_stride}, fcos, fsin, H, KV, hd, max_seq, nullptr, nullptr,
                                 0.0f, 0.0f);
}
extern "C" __global__ void __launch_bounds__(256)
mc_pp_rope_cache_parts_bfloat(const float* part, uint32_t splits, uint32_t M, bf16_t* q_out, const pp_seg* segs, uint32_t nseg, bf16_t* kc,
                              bf16_t* vt, uint64_t cache_stride, const float* fcos, const float* fsin, uint32_t H, uint32_t KV, uint32_t hd,
                              uint32_t max_seq)
{
    pf_rope_cache_v4_body<true>(part, splits, M, q_out, pp_rows{segs, nseg, kc, vt, cache_stride}, fcos, fsin, H, KV, hd, max_seq, nullptr,
                                nullptr, 0.0f, 0.0f);
}

// Causal attention over segments: grid (tiles, H / NH), 256 threads.  tiles[blockIdx.x] = (segment, first row of the tile inside it):
// 16 rows of ONE segment, the tiles of a segment starting at its first row.  The tile is the one-prompt kernel's tile of a prompt of
// M = len rows at S = pos + len in the row's own cache, its Q and output rows offset by the segment's offset -- pf_visible included
// (only the chunk's own columns are visible, as in mc_decoder_prefill at start_pos = pos).
#define MC_PP_ATTN(HD)                                                                                                                     \
    extern "C" __global__ void __launch_bounds__(256)                                                                                      \
    mc_pp_attn_bfloat_hd##HD(const bf16_t* Q, const pp_seg* segs, const pp_tile* tiles, const bf16_t* kc, const bf16_t* vt, uint64_t cache_stride, \
                             bf16_t* out, uint32_t H, uint32_t n_rep, uint32_t max_seq, float scale, const float* etab)                    \
    {                                                                                                                                      \
        const pp_tile t = tiles[blockIdx.x];                                                                                               \
        const pp_seg g = segs[t.seg];                                                                                                      \
        const size_t q0 = (size_t)g.off * H * HD;                                                                                          \
        pf_attn_body<HD, 1>(Q + q0, kc + (size_t)g.row * cache_stride, vt + (size_t)g.row * cache_stride, out + q0, (uint32_t)g.len,       \
                            (uint32_t)(g.pos + g.len), H, n_rep, max_seq, scale, 0u, etab, (uint32_t)t.r0);                                \
    }                                                                                                                                      \
    extern "C" __global__ void __launch_bounds__(256)                                                                                      \
    mc_pp_attn2_bfloat_hd##HD(const bf16_t* Q, const pp_seg* segs, const pp_tile* tiles, const bf16_t* kc, const bf16_t* vt,               \
                              uint64_t cache_stride, bf16_t* out, uint32_t H, uint32_t n_rep, uint32_t max_seq, float scale,               \
                              const float* etab)                                                                                           \
    {                                                                                                                                      \
        const pp_tile t = tiles[blockIdx.x];                                                                                               \
        const pp_seg g = segs[t.seg];                                                                                                      \
        const size_t q0 = (size_t)g.off * H * HD;                                                                                          \
        pf_attn_kt_body<HD, 2>(Q + q0, kc + (size_t)g.row * cache_stride, vt + (size_t)g.row * cache_stride, out + q0, (uint32_t)g.len,    \
                               (uint32_t)(g.pos + g.len), H, n_rep, max_seq, scale, 0u, etab, (uint32_t)t.r0);                             \
    }
MC_PP_ATTN(64)
MC_PP_ATTN(128)

// the last row of every segment -> x[row] ([B][dim]: the batch head's input); grid (ceil(dim / 256), nseg), 256 threads
extern "C" __global__ void
mc_pp_gather_last_bfloat(const bf16_t* rows, const pp_seg* segs, bf16_t* x, uint32_t dim)
{
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= dim) return;
    const pp_seg g = segs[blockIdx.y];
    x[(size_t)g.row * dim + k] = rows[(size_t)(g.off + g.len - 1) * dim + k];
}
