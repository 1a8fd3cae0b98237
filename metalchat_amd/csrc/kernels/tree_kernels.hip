// Speculative verify over a draft TREE per row (mc_tree_verify, include/metalchat_hip.h Part 2g): mc_verify_rows' pass whose chunk
// rows are the nodes of a tree.  Node i of a segment is written to cache slot pos + i (its index), is rotated for position
// pos + depth(i), and attends to the keys below pos plus the slots of its ancestors and itself.  The per-packed-row table tv_node
// (abi.h; built by the host from the call's `parents`) carries depth and the ancestor-or-self bits.
//
//   mc_tv_rope_cache{,_parts}_bfloat       mc_pp_rope_cache*'s body over a row map with slot = pos + i, rope row = pos + depth(i)
//   mc_tv_sums{,2} / mc_tv_pv{,2}_hd{64,128} extend_kernels.hip's px_sums_body / px_pv_body with TREE = true: ONE select differs
//   (mc_px_reduce_* is reused as it is: range table, split rule, rounding points and sum order are mc_extend_rows')
//   mc_tv_accept                           the walk from the root along matching children; the last accepted node's logits
//   mc_tv_compact_bfloat                   the accepted path's K / V from slots pos + path[d] to pos + d, all layers in one launch
//
// The mask's contract.  A node that is not an ancestor-or-self of a row gets the score -inf, so its e = exp(s) is an exact 0 and
// its p = T(e * 1/sum) is an exact +0.  Its V row is FINITE: the slot is pos + j for a node j of this call, and this call's rope +
// cache launch wrote it one launch earlier (slots at or past pos + len are zeroed by px_pv_body's own element mask).  So its
// products p * v are +-0, and adding +-0 changes no bit of a sum that holds at least one other term (every row sees itself).  Its K
// may be anything: the score is replaced before it is used.  With chain masks (anc of node i = bits 0 .. i) the select is
// key <= pos + i for every key below pos + 16 -- the keys of the tile end at pos + len -- and the kernels compute mc_px_*'s bits.

// pf_rope_cache_v4_body's row map over the segment table and the node table: packed row r = node i of its segment
struct tv_rows {
    const pp_seg* segs;
    uint32_t nseg;
    bf16_t* kc;
    bf16_t* vt;
    uint64_t cache_stride;
    const tv_node* nodes;
    __device__ __forceinline__ void
    at(uint32_t r, bf16_t*& k, bf16_t*& v, uint32_t& slot, uint32_t& rope_row) const
    {
        uint32_t s = 0;
        while (s + 1 < nseg && r >= (uint32_t)segs[s + 1].off) s++;
        const pp_seg g = segs[s];
        k = kc + (size_t)g.row * cache_stride;
        v = vt + (size_t)g.row * cache_stride;
        slot = (uint32_t)g.pos + (r - (uint32_t)g.off);
        rope_row = (uint32_t)g.pos + (uint32_t)nodes[r].depth;
    }
};

// grids, rows and arguments as mc_pp_rope_cache_bfloat / mc_pp_rope_cache_parts_bfloat, the node table behind them
extern "C" __global__ void __launch_bounds__(256)
mc_tv_rope_cache_bfloat(const bf16_t* qkv, uint32_t M, bf16_t* q_out, const pp_seg* segs, uint32_t nseg, bf16_t* kc, bf16_t* vt,
                        uint64_t cache_stride, const float* fcos, const float* fsin, uint32_t H, uint32_t KV, uint32_t hd, uint32_t max_seq,
                        const tv_node* nodes)
{
    pf_rope_cache_v4_body<false>(qkv, 1, M, q_out, tv_rows{segs, nseg, kc, vt, cache_stride, nodes}, fcos, fsin, H, KV, hd, max_seq, nullptr,
                                 nullptr, 0.0f, 0.0f);
}
extern "C" __global__ void __launch_bounds__(256)
mc_tv_rope_cache_parts_bfloat(const float* part, uint32_t splits, uint32_t M, bf16_t* q_out, const pp_seg* segs, uint32_t nseg, bf16_t* kc,
                              bf16_t* vt, uint64_t cache_stride, const float* fcos, const float* fsin, uint32_t H, uint32_t KV, uint32_t hd,
                              uint32_t max_seq, const tv_node* nodes)
{
    pf_rope_cache_v4_body<true>(part, splits, M, q_out, tv_rows{segs, nseg, kc, vt, cache_stride, nodes}, fcos, fsin, H, KV, hd, max_seq,
                                nullptr, nullptr, 0.0f, 0.0f);
}

// grids and arguments as mc_px_sums* / mc_px_pv* (extend_kernels.hip), the node table behind them
#define MC_TV_ATTN(HD, NH, SFX)                                                                                                            \
    extern "C" __global__ void __launch_bounds__(256)                                                                                      \
    mc_tv_sums##SFX##_bfloat_hd##HD(const bf16_t* Q, const pp_seg* segs, const px_range* tab, uint32_t ebase, const bf16_t* kc,              \
                                    uint64_t cache_stride, float* sums, uint32_t H, uint32_t n_rep, uint32_t max_seq, float scale,           \
                                    const float* etab, const tv_node* nodes)                                                               \
    {                                                                                                                                      \
        px_sums_body<HD, NH, true>(Q, segs, tab, ebase, kc, cache_stride, sums, H, n_rep, max_seq, scale, etab, nodes);                      \
    }                                                                                                                                      \
    extern "C" __global__ void __launch_bounds__(256)                                                                                      \
    mc_tv_pv##SFX##_bfloat_hd##HD(const bf16_t* Q, const pp_seg* segs, const px_range* tab, uint32_t ebase, const bf16_t* kc,                \
                                  const bf16_t* vt, uint64_t cache_stride, const float* sums, float* part, bf16_t* out, uint32_t H,            \
                                  uint32_t n_rep, uint32_t max_seq, float scale, const float* etab, const tv_node* nodes)                  \
    {                                                                                                                                      \
        px_pv_body<HD, NH, true>(Q, segs, tab, ebase, kc, vt, cache_stride, sums, part, out, H, n_rep, max_seq, scale, etab, nodes);         \
    }
MC_TV_ATTN(64, 1, )
MC_TV_ATTN(64, 2, 2)
MC_TV_ATTN(128, 1, )
MC_TV_ATTN(128, 2, 2)

// grid (any, nseg), 256 threads: segment g = segs[blockIdx.y] holds the nodes [off, off + len) of its row's tree and the picks after
// each of them.  The walk: cur = 0; among cur's children in ascending node index the first j with tokens[j] == pick[cur] becomes
// cur; it stops when there is none.  Node j is a child of cur when depth(j) == depth(cur) + 1 and bit cur of anc(j) is set (its
// ancestor at that depth is its parent); children have higher indices than their parent (topological order).  Every thread walks
// the <= 15 drafts: no hand-off.  accepted[row] = depth(cur), next_tokens[row] = pick[cur], paths[row][d] = the node at depth d
// for d <= depth(cur) and -1 behind it (each may be null), and logits row off + cur into logits_out[row] (vocab % 8 == 0: rows
// are copied in 16-byte pieces).  Rows of the batch without a segment are not written.
extern "C" __global__ void __launch_bounds__(256)
mc_tv_accept(const pp_seg* segs, const int32_t* tokens, const tv_node* nodes, const int32_t* picks, const bf16_t* logits, uint32_t vocab,
             int32_t* accepted, int32_t* next_tokens, int32_t* paths, bf16_t* logits_out)
{
    const pp_seg g = segs[blockIdx.y];
    const bool writer = blockIdx.x == 0 && threadIdx.x == 0;
    int32_t* path = paths ? paths + (size_t)g.row * MC_VERIFY_MAX_LEN : nullptr;
    int32_t cur = 0, a = 0;
    if (writer && path) path[0] = 0;
    for (;;) {
        const int32_t want = picks[g.off + cur];
        int32_t next = -1;
        for (int32_t j = cur + 1; j < g.len && next < 0; j++) {
            const tv_node nj = nodes[g.off + j];
            if (nj.depth == a + 1 && ((nj.anc >> cur) & 1u) && tokens[g.off + j] == want) next = j;
        }
        if (next < 0) break;
        cur = next;
        a++;
        if (writer && path) path[a] = cur;
    }
    if (writer) {
        if (accepted) accepted[g.row] = a;
        if (next_tokens) next_tokens[g.row] = picks[g.off + cur];
        if (path)
            for (int32_t d = a + 1; d < MC_VERIFY_MAX_LEN; d++) path[d] = -1;
    }
    const uint4* src = reinterpret_cast<const uint4*>(logits + (size_t)(g.off + cur) * vocab);
    uint4* dst = reinterpret_cast<uint4*>(logits_out + (size_t)g.row * vocab);
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < vocab / 8; i += gridDim.x * blockDim.x) dst[i] = src[i];
}

// grid (ceil(KV * hd / 256), nseg, layers), 256 threads: the accepted path's K / V into place.  kc / vt are layer 0's caches,
// layer l of batch row r at + (l * B + r) * cache_stride elements: K [KV][max_seq][hd], V transposed [KV][hd][max_seq].  Thread
// (kv head, element) walks d = 1 .. accepted[row] in ascending order and moves its element from slot pos + path[d] to slot pos + d.
// path[d] >= d (a node's index is at least its depth) and the path is strictly ascending (children follow their parents), so the
// source of step d lies at or behind every slot written so far (pos + 1 .. pos + d - 1 < pos + d <= pos + path[d]): a thread that
// owns its element across all slots never reads a slot it has overwritten, and no two threads touch one address.  Nothing is
// moved where path[d] == d (a chain: the whole launch is a no-op).  accepted and paths are mc_tv_accept's, read from the device.
extern "C" __global__ void __launch_bounds__(256)
mc_tv_compact_bfloat(const pp_seg* segs, const int32_t* accepted, const int32_t* paths, bf16_t* kc, bf16_t* vt, uint64_t cache_stride,
                     uint32_t B, uint32_t KV, uint32_t hd, uint32_t max_seq)
{
    const uint32_t e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= KV * hd) return;
    const pp_seg g = segs[blockIdx.y];
    const int32_t a = accepted[g.row];
    const int32_t* path = paths + (size_t)g.row * MC_VERIFY_MAX_LEN;
    const size_t base = ((size_t)blockIdx.z * B + (uint32_t)g.row) * cache_stride;
    const uint32_t kv = e / hd, el = e % hd;
    bf16_t* k = kc + base + (size_t)kv * max_seq * hd + el;   // + slot * hd
    bf16_t* v = vt + base + ((size_t)kv * hd + el) * max_seq; // + slot
    for (int32_t d = 1; d <= a; d++) {
        const uint32_t src = (uint32_t)(g.pos + path[d]), dst = (uint32_t)(g.pos + d);
        if (src == dst) continue;
        k[(size_t)dst * hd] = k[(size_t)src * hd];
        v[dst] = v[src];
    }
}
