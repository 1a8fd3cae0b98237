// Speculative verify over a draft TREE per row on fp8 KV caches (mc_kv_tree_set, include/metalchat_hip.h Part 2q): tree_kernels.hip's pass on the byte
// and exponent planes of kv8_kernels.hip.  The contract is Part 2o's (tests/kv_fp8_rule.py): every kernel here computes bit for bit what its bfloat16
// counterpart computes on planes that hold deq(quant(K)), deq(quant(V)), and writes quant of what that counterpart would have stored.
//
//   mc_tv8_rope_cache{,_parts}_bfloat          pp8_rope_cache_body (kv8_rows_kernels.hip) with TREE = true: packed row r = node i of its segment is
//                                              written to slot pos + i and rotated with rope row pos + depth(i); the K unit's shuffle-tree amax and the
//                                              V tile's maxima through LDS are Part 2p's
//   mc_tv8_sums{,2} / mc_tv8_pv{,2}_hd{64,128} px8_sums_body / px8_pv_body with TREE = true: px_tile's select over tv_node::anc, ONE select differs; the
//                                              bytes move as in Part 2p (K 8 bytes a k-step and one exponent, one tile ahead, four
//                                              v_cvt_scalef32_pk_bf16_fp8; a V block's eight exponents once for all tiles and both heads, every V byte
//                                              requested before the block's scores).  mc_px_reduce_* follows unchanged
//   mc_tv8_compact                             the accepted path's vectors -- bytes AND exponent -- from slot pos + path[d] to pos + d, four planes, all layers
//
// The mask's contract on bytes.  A node that is not an ancestor-or-self of a row gets the score -inf: its e is an exact 0, its p an exact +0.  Its K
// bytes and exponent may be anything (a NaN byte included): the score is replaced before it is used, and load_k never leaves [0, S).  Its V slot is
// pos + j for a node j of this call, which mc_tv8_rope_cache* wrote one launch earlier: a byte of quant is never 0x7f / 0xff and an exponent of quant
// lies in [-100, 119], so deq there is finite and p * deq = +-0, which changes no bit of a sum with one other term (every row sees itself).  The slots
// at and past pos + len -- never written by this row, or a rewound tail -- are zeroed, bytes and exponents, by kv8_slot_masks before the conversion:
// its bound is px_tile::S = pos + min(r0 + 16, len), and a tree has at most 16 nodes, so r0 = 0 and S = pos + len exactly.  With chain masks the
// kernels compute mc_px8_*'s bits.
// No private segment, no spills, vector stores only.  bfloat16 decoders, head_dim 64 and 128.
// The names are mc_tv8_* beside mc_tv_*, not those names with an _f8 in them: tests/test_tree_verify_cpu.py pins the set of mc_tv_* names.

// grids, rows and arguments as mc_pp8_rope_cache_bfloat / mc_pp8_rope_cache_parts_bfloat, the node table behind them
extern "C" __global__ void __launch_bounds__(256)
mc_tv8_rope_cache_bfloat(const bf16_t* qkv, uint32_t M, bf16_t* q_out, const pp_seg* segs, uint32_t nseg, uint8_t* kq, uint8_t* vq, int8_t* kexp,
                         int8_t* vexp, uint64_t cache_stride, uint64_t exp_stride, const float* fcos, const float* fsin, uint32_t H, uint32_t KV,
                         uint32_t hd, uint32_t max_seq, const tv_node* nodes)
{
    pp8_rope_cache_body<false, true>(qkv, 1, M, q_out, segs, nseg, kq, vq, kexp, vexp, cache_stride, exp_stride, fcos, fsin, H, KV, hd, max_seq, nodes);
}
extern "C" __global__ void __launch_bounds__(256)
mc_tv8_rope_cache_parts_bfloat(const float* part, uint32_t splits, uint32_t M, bf16_t* q_out, const pp_seg* segs, uint32_t nseg, uint8_t* kq,
                               uint8_t* vq, int8_t* kexp, int8_t* vexp, uint64_t cache_stride, uint64_t exp_stride, const float* fcos,
                               const float* fsin, uint32_t H, uint32_t KV, uint32_t hd, uint32_t max_seq, const tv_node* nodes)
{
    pp8_rope_cache_body<true, true>(part, splits, M, q_out, segs, nseg, kq, vq, kexp, vexp, cache_stride, exp_stride, fcos, fsin, H, KV, hd, max_seq,
                                    nodes);
}

// grids and arguments as mc_px8_sums* / mc_px8_pv* (kv8_rows_kernels.hip), the node table behind them
#define MC_TV_ATTN_F8(HD, NH, SFX)                                                                                                                  \
    extern "C" __global__ void __launch_bounds__(256)                                                                                               \
    mc_tv8_sums##SFX##_bfloat_hd##HD(const bf16_t* Q, const pp_seg* segs, const px_range* tab, uint32_t ebase, const uint8_t* kq,                  \
                                     const int8_t* kexp, uint64_t cache_stride, uint64_t exp_stride, float* sums, uint32_t H, uint32_t n_rep,      \
                                     uint32_t max_seq, float scale, const float* etab, const tv_node* nodes)                                        \
    {                                                                                                                                               \
        px8_sums_body<HD, NH, true>(Q, segs, tab, ebase, kq, kexp, cache_stride, exp_stride, sums, H, n_rep, max_seq, scale, etab, nodes);           \
    }                                                                                                                                               \
    extern "C" __global__ void __launch_bounds__(256)                                                                                               \
    mc_tv8_pv##SFX##_bfloat_hd##HD(const bf16_t* Q, const pp_seg* segs, const px_range* tab, uint32_t ebase, const uint8_t* kq, const uint8_t* vq, \
                                   const int8_t* kexp, const int8_t* vexp, uint64_t cache_stride, uint64_t exp_stride, const float* sums,          \
                                   float* part, bf16_t* out, uint32_t H, uint32_t n_rep, uint32_t max_seq, float scale, const float* etab,          \
                                   const tv_node* nodes)                                                                                            \
    {                                                                                                                                               \
        px8_pv_body<HD, NH, true>(Q, segs, tab, ebase, kq, vq, kexp, vexp, cache_stride, exp_stride, sums, part, out, H, n_rep, max_seq, scale,      \
                                  etab, nodes);                                                                                                     \
    }
MC_TV_ATTN_F8(64, 1, )
MC_TV_ATTN_F8(64, 2, 2)
MC_TV_ATTN_F8(128, 1, )
MC_TV_ATTN_F8(128, 2, 2)

// grid (ceil(owners / 256), nseg, layers), 256 threads: the accepted path's K / V into place on the four planes.  kq / vq / kexp / vexp are layer 0's
// planes, layer l of batch row r at + (l * B + r) * cache_stride bytes (exponents: exp_stride): K bytes [KV][max_seq][hd], V bytes transposed
// [KV][hd][max_seq], kexp and vexp [KV][max_seq].  A moved vector is its hd bytes and its exponent, copied unchanged -- nothing is quantised again, so
// deq of slot pos + d afterwards is exactly deq of what mc_tv8_rope_cache* wrote for node path[d].  The owners, split as the planes lie:
//   [0, KV hd / 16)        K bytes: a slot's hd bytes are contiguous, owner (kv, w) moves the 16-byte word w of every slot (hd / 16 lanes a kv head)
//   [.., + KV hd)          V bytes: a vector lies at stride max_seq, owner (kv, el) moves one byte of every slot
//   [.., + 2 KV)           kexp, then vexp: owner (plane, kv) moves one exponent of every slot
// mc_tv_compact_bfloat's rule holds owner by owner: each address has ONE owner across all slots, the owner walks d = 1 .. accepted[row] in ascending
// order and skips path[d] == d; path[d] >= d and the path ascends strictly, so the source of step d lies at or behind every slot written so far -- no
// owner reads what it has overwritten, no two owners touch one address (a byte store touches its byte alone).  cache_stride % 16 == 0 and hd % 16 == 0:
// the K words are aligned.
extern "C" __global__ void __launch_bounds__(256)
mc_tv8_compact(const pp_seg* segs, const int32_t* accepted, const int32_t* paths, uint8_t* kq, uint8_t* vq, int8_t* kexp, int8_t* vexp,
               uint64_t cache_stride, uint64_t exp_stride, uint32_t B, uint32_t KV, uint32_t hd, uint32_t max_seq)
{
    const uint32_t kw = hd / 16, nk = KV * kw, nv = KV * hd, nx = 2 * KV;
    uint32_t o = blockIdx.x * blockDim.x + threadIdx.x;
    if (o >= nk + nv + nx) return;
    const pp_seg g = segs[blockIdx.y];
    const int32_t a = accepted[g.row];
    const int32_t* path = paths + (size_t)g.row * MC_VERIFY_MAX_LEN;
    const size_t plane = (size_t)blockIdx.z * B + (uint32_t)g.row;
    const uint32_t pos = (uint32_t)g.pos;
    if (o < nk) {
        const uint32_t kv = o / kw, w = o % kw;
        uint8_t* k = kq + plane * cache_stride + (size_t)kv * max_seq * hd + 16 * w; // + slot * hd
        for (int32_t d = 1; d <= a; d++) {
            const uint32_t src = pos + (uint32_t)path[d], dst = pos + (uint32_t)d;
            if (src == dst) continue;
            *reinterpret_cast<uint4*>(k + (size_t)dst * hd) = *reinterpret_cast<const uint4*>(k + (size_t)src * hd);
        }
        return;
    }
    o -= nk;
    // (a V byte or an exponent: one byte of every slot, the slots consecutive)
    uint8_t* p;
    if (o < nv) {
        p = vq + plane * cache_stride + (size_t)o * max_seq; // o = kv * hd + el
    } else {
        o -= nv;
        p = reinterpret_cast<uint8_t*>(o < KV ? kexp : vexp) + plane * exp_stride + (size_t)(o % KV) * max_seq;
    }
    for (int32_t d = 1; d <= a; d++) {
        const uint32_t src = pos + (uint32_t)path[d], dst = pos + (uint32_t)d;
        if (src == dst) continue;
        p[dst] = p[src];
    }
}
