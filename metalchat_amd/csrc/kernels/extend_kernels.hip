// Chunks that see their row's context (mc_extend_rows, include/metalchat_hip.h Part 2e): the packed prompt pass of
// packed_kernels.hip with ONE difference -- chunk row i of a segment (position p = pos + i) attends to cache columns c <= p of its
// row, the columns below pos included.  Rope + cache write, the gather of the last rows and everything row-wise are the packed
// pass's own launches; only the attention is here.
//
// The shape that matters is few chunk rows over many keys (a 20-token message behind 1900 tokens), so the KEYS of a 16-row tile are
// dealt over workgroups in key ranges where the tile's segment is short (rows_plan.h px_range_keys).  The softmax has no max shift and p is rounded to T with the FULL row
// sum, so the sums must be complete before any p exists -- three launches per layer, all over the range table:
//
//   mc_px_sums   (heads, ranges)  exp row sums of one key range                         -> sums[range][head][16]       fp32
//   mc_px_pv     (heads, ranges)  row sum = the tile's range sums added in range order; p = T(exp(s) * 1/sum); p V over the
//                                 range -> out, rounded to T, when the tile has one range; else -> part[range][head][16][HD] fp32
//   mc_px_reduce (heads, ranges)  a split tile's first range: its ranges' partial outputs added in range order, rounded to T -> out
//                                 (launched only for a group that holds a split tile)
//
// Rounding points are pf_attn_kt_body's (prefill_kernels.hip): s = T(T(q.k) scale), e = exp(s) from the table window,
// p = T(e * 1/sum), out = T(sum p v).  A tile's ranges are a function of its own segment alone, the waves of a workgroup
// take its 32-key blocks in a fixed deal, and ranges are added first to last: a row's bits depend on its own segment only, never
// on what else is in the call.
//
// The range table: one px_range per (tile, key range), the ranges of a tile adjacent and ascending.  `first` and `n` name the
// tile's ranges; scratch slots are range indices relative to `ebase`, the first range of the launch (a call whose ranges exceed
// the scratch is launched in groups of whole tiles).

// (px_range: abi.h)

// the scores of one range: shared by the two passes.  Lane (l15, lg) of a wave holds row r0 + l15 (S^T = K Q^T, as pf_attn_kt_body).
// TREE (tree_kernels.hip, mc_tree_verify): the chunk rows are the nodes of a draft tree, and a live row sees the keys below pos
// and, among the chunk's own slots [pos, pos + 16), those of its ancestors and itself (tv_node::anc) -- the one difference.
template <uint32_t HD, int NH, bool TREE = false>
struct px_tile {
    static constexpr uint32_t DK = HD / 32;
    const bf16_t* kbase;
    uint32_t l15, lg, kg;
    uint32_t pos_r; // the last visible key of this lane's row (pos + r), or 0 with `live` false; TREE: pos, the chunk's first slot
    uint32_t anc;   // TREE only: this lane's row's tv_node::anc
    bool live;      // this lane's row is a row of the chunk
    uint32_t S;     // keys of the row's cache that any row of the tile may see: [0, S)
    float scale;
    uint4 qa[NH][DK];

    __device__ __forceinline__ void
    load_k(uint32_t blk, uint32_t h, uint4 (&kb)[DK]) const
    {
        const uint32_t key = blk + 8 * (l15 >> 2) + 4 * h + (l15 & 3), keyc = key < S ? key : S - 1;
#pragma unroll
        for (uint32_t d = 0; d < DK; d++) kb[d] = *reinterpret_cast<const uint4*>(kbase + (size_t)keyc * HD + d * 32 + kg);
    }
    // sv[j][i] = masked, scaled score of (this lane's row, key blk + 8 lg + 4 h + i) for head j
    __device__ __forceinline__ void
    score(uint32_t blk, uint32_t h, const uint4 (&kb)[DK], float (&sv)[NH][4]) const
    {
#pragma unroll
        for (int j = 0; j < NH; j++) {
            pf_f32x4 acc = {0, 0, 0, 0};
#pragma unroll
            for (uint32_t d = 0; d < DK; d++)
                acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(pf_bf16x8, kb[d]), __builtin_bit_cast(pf_bf16x8, qa[j][d]), acc, 0, 0, 0);
#pragma unroll
            for (int i = 0; i < 4; i++) sv[j][i] = BF::rt(BF::rt(acc[i]) * scale);
        }
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const uint32_t key = blk + lg * 8 + h * 4 + i;
            const bool vis = TREE ? bool(int(live) & (int(key < pos_r) | (int(key < pos_r + 16u) & int((anc >> ((key - pos_r) & 15u)) & 1u))))
                                  : bool(int(live) & int(key <= pos_r));
#pragma unroll
            for (int j = 0; j < NH; j++) sv[j][i] = vis ? sv[j][i] : -INFINITY;
        }
    }
};

template <uint32_t HD, int NH, bool TREE = false>
__device__ __forceinline__ px_tile<HD, NH, TREE>
px_tile_of(const bf16_t* Q, const pp_seg& g, const px_range& e, const bf16_t* kc, uint64_t cache_stride, uint32_t H, uint32_t n_rep,
           uint32_t max_seq, float scale, uint32_t h0, const tv_node* nodes = nullptr)
{
    px_tile<HD, NH, TREE> t;
    const uint32_t lane = threadIdx.x & 63;
    t.l15 = lane & 15;
    t.lg = lane >> 4;
    t.kg = t.lg * 8;
    t.kbase = kc + (size_t)g.row * cache_stride + (size_t)(h0 / n_rep) * max_seq * HD;
    const uint32_t r = (uint32_t)e.r0 + t.l15, len = (uint32_t)g.len;
    t.live = r < len;
    if (TREE) {
        t.pos_r = (uint32_t)g.pos;
        t.anc = t.live ? nodes[(uint32_t)g.off + r].anc : 0u;
    } else {
        t.pos_r = t.live ? (uint32_t)g.pos + r : 0u;
    }
    t.S = (uint32_t)g.pos + min((uint32_t)e.r0 + 16u, len);
    t.scale = scale;
    const uint32_t qr = (uint32_t)g.off + min(r, len - 1);
#pragma unroll
    for (int j = 0; j < NH; j++)
#pragma unroll
        for (uint32_t d = 0; d < t.DK; d++)
            t.qa[j][d] = *reinterpret_cast<const uint4*>(Q + ((size_t)qr * H + h0 + j) * HD + d * 32 + t.kg);
    return t;
}

// grid (H / NH, ranges of the launch), 256 threads
template <uint32_t HD, int NH, bool TREE = false>
__device__ __forceinline__ void
px_sums_body(const bf16_t* Q, const pp_seg* segs, const px_range* tab, uint32_t ebase, const bf16_t* kc, uint64_t cache_stride, float* sums,
             uint32_t H, uint32_t n_rep, uint32_t max_seq, float scale, const float* etab, const tv_node* nodes = nullptr)
{
    constexpr uint32_t DK = HD / 32;
    __shared__ float wsum[NH][4][16];
    __shared__ __attribute__((aligned(16))) float ewin[2 * pf_exp_window::N];
    const pf_exp_window ew{ewin};
    ew.fill(etab);
    const px_range e = tab[ebase + blockIdx.y];
    const pp_seg g = segs[e.seg];
    const uint32_t wave = threadIdx.x >> 6, h0 = blockIdx.x * NH;
    const px_tile<HD, NH, TREE> t = px_tile_of<HD, NH, TREE>(Q, g, e, kc, cache_stride, H, n_rep, max_seq, scale, h0, nodes);
    const uint32_t b_lo = (uint32_t)e.k_lo / 32, b_end = ((uint32_t)e.k_hi + 31) / 32;
    float rsum[NH];
#pragma unroll
    for (int j = 0; j < NH; j++) rsum[j] = 0.0f;
    uint4 k0[DK], k1[DK];
    t.load_k((b_lo + wave) * 32, 0, k0);
    __syncthreads(); // the exp window is filled
    for (uint32_t b = b_lo + wave; b < b_end; b += 4) {
        float sv[NH][4];
        t.load_k(b * 32, 1, k1);
        t.score(b * 32, 0, k0, sv);
#pragma unroll
        for (int j = 0; j < NH; j++) rsum[j] += (ew(sv[j][0]) + ew(sv[j][1])) + (ew(sv[j][2]) + ew(sv[j][3]));
        t.load_k((b + 4) * 32, 0, k0); // (past the range: clamped to the tile's last key, never used)
        t.score(b * 32, 1, k1, sv);
#pragma unroll
        for (int j = 0; j < NH; j++) rsum[j] += (ew(sv[j][0]) + ew(sv[j][1])) + (ew(sv[j][2]) + ew(sv[j][3]));
    }
#pragma unroll
    for (int j = 0; j < NH; j++) {
        float s = rsum[j];
        s += __shfl_xor(s, 16, 64);
        s += __shfl_xor(s, 32, 64);
        if (t.lg == 0) wsum[j][wave][t.l15] = s;
    }
    __syncthreads();
    if (threadIdx.x < 16 * NH) {
        const uint32_t j = threadIdx.x / 16, rr = threadIdx.x % 16;
        sums[((size_t)blockIdx.y * H + h0 + j) * 16 + rr] = (wsum[j][0][rr] + wsum[j][1][rr]) + (wsum[j][2][rr] + wsum[j][3][rr]);
    }
}

// grid (H / NH, ranges of the launch), 256 threads
template <uint32_t HD, int NH, bool TREE = false>
__device__ __forceinline__ void
px_pv_body(const bf16_t* Q, const pp_seg* segs, const px_range* tab, uint32_t ebase, const bf16_t* kc, const bf16_t* vt, uint64_t cache_stride,
           const float* sums, float* part, bf16_t* out, uint32_t H, uint32_t n_rep, uint32_t max_seq, float scale, const float* etab,
           const tv_node* nodes = nullptr)
{
    constexpr uint32_t DT = HD / 16, DK = HD / 32;
    __shared__ float inv_sum[NH][16];
    // (the exp window and, behind the key loop, the waves' partial outputs share one buffer: 33 KiB, four workgroups per CU)
    constexpr uint32_t OD = HD < 128 ? HD : 128; // output columns reduced per phase
    constexpr uint32_t NW = 2 * pf_exp_window::N, NO = 4 * 16 * (OD + 1);
    __shared__ __attribute__((aligned(16))) float lds[NW > NO ? NW : NO];
    const pf_exp_window ew{lds};
    ew.fill(etab);
    float (*osum)[16][OD + 1] = reinterpret_cast<float (*)[16][OD + 1]>(lds);
    const px_range e = tab[ebase + blockIdx.y];
    const pp_seg g = segs[e.seg];
    const uint32_t wave = threadIdx.x >> 6, h0 = blockIdx.x * NH;
    const px_tile<HD, NH, TREE> t = px_tile_of<HD, NH, TREE>(Q, g, e, kc, cache_stride, H, n_rep, max_seq, scale, h0, nodes);
    const bf16_t* vbase = vt + (size_t)g.row * cache_stride + (size_t)(h0 / n_rep) * HD * max_seq;
    const uint32_t b_lo = (uint32_t)e.k_lo / 32, b_end = ((uint32_t)e.k_hi + 31) / 32;
    if (threadIdx.x < 16 * NH) {
        // the row's sum: the tile's ranges first to last.  A row of the chunk sees key 0, so its sum is positive; the rows past
        // the chunk's end have no key at all (sum 0): their p stays 0 and their outputs are never read
        const uint32_t j = threadIdx.x / 16, rr = threadIdx.x % 16;
        float s = 0.0f;
        for (int32_t i = 0; i < e.n; i++) s += sums[((size_t)((uint32_t)(e.first + i) - ebase) * H + h0 + j) * 16 + rr];
        inv_sum[j][rr] = s == 0.0f ? 0.0f : 1.0f / s;
    }
    uint4 k0[DK], k1[DK];
    t.load_k((b_lo + wave) * 32, 0, k0);
    __syncthreads(); // the exp window is filled, the sums are there
    float inv[NH];
#pragma unroll
    for (int j = 0; j < NH; j++) inv[j] = inv_sum[j][t.l15];
    pf_f32x4 oacc[NH][DT];
#pragma unroll
    for (int j = 0; j < NH; j++)
#pragma unroll
        for (uint32_t d = 0; d < DT; d++) oacc[j][d] = pf_f32x4{0, 0, 0, 0};
    constexpr uint32_t VG = DT < 8 ? DT : 8;
    for (uint32_t b = b_lo + wave; b < b_end; b += 4) {
        // V fragments of the block (keys 32 b + 8 lg .. + 7: the k slots of this lane's A operand).  Past max_seq: clamped address,
        // masked to zero (slots in [S, max_seq) may hold anything finite or not: their p is 0, and 0 * NaN must not reach a sum)
        const uint32_t c = b * 32 + t.kg;
        const bool vin = c + 8 <= max_seq;
        const bf16_t* vp = vbase + (size_t)t.l15 * max_seq + (vin ? c : max_seq - 8);
        uint4 vbs[VG];
#pragma unroll
        for (uint32_t d = 0; d < VG; d++) vbs[d] = *reinterpret_cast<const uint4*>(vp + (size_t)d * 16 * max_seq);
        uint4 pa[NH];
        {
            float sv[NH][4];
            t.load_k(b * 32, 1, k1);
            t.score(b * 32, 0, k0, sv);
#pragma unroll
            for (int j = 0; j < NH; j++) {
                pa[j].x = pack_bf16x2(BF::rt(ew(sv[j][0]) * inv[j]), BF::rt(ew(sv[j][1]) * inv[j]));
                pa[j].y = pack_bf16x2(BF::rt(ew(sv[j][2]) * inv[j]), BF::rt(ew(sv[j][3]) * inv[j]));
            }
            t.load_k((b + 4) * 32, 0, k0); // (past the range: clamped to the tile's last key, never used)
            t.score(b * 32, 1, k1, sv);
#pragma unroll
            for (int j = 0; j < NH; j++) {
                pa[j].z = pack_bf16x2(BF::rt(ew(sv[j][0]) * inv[j]), BF::rt(ew(sv[j][1]) * inv[j]));
                pa[j].w = pack_bf16x2(BF::rt(ew(sv[j][2]) * inv[j]), BF::rt(ew(sv[j][3]) * inv[j]));
            }
        }
        // the V of a slot no row of the tile sees is replaced by zero, element by element: a slot past the tile's keys was never
        // written by this row (or belongs to a rewound tail) and may hold a NaN or an infinity, and 0 * that is a NaN
        uint32_t m[4];
#pragma unroll
        for (uint32_t q = 0; q < 4; q++) {
            const uint32_t lo = (vin && c + 2 * q < t.S) ? 0x0000FFFFu : 0u, hi = (vin && c + 2 * q + 1 < t.S) ? 0xFFFF0000u : 0u;
            m[q] = lo | hi;
        }
#pragma unroll
        for (uint32_t d0 = 0; d0 < DT; d0 += VG) {
            if (d0) {
#pragma unroll
                for (uint32_t d = 0; d < VG; d++) vbs[d] = *reinterpret_cast<const uint4*>(vp + (size_t)(d0 + d) * 16 * max_seq);
            }
#pragma unroll
            for (uint32_t d = 0; d < VG; d++) {
                const uint4 vb = make_uint4(vbs[d].x & m[0], vbs[d].y & m[1], vbs[d].z & m[2], vbs[d].w & m[3]);
#pragma unroll
                for (int j = 0; j < NH; j++)
                    oacc[j][d0 + d] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(pf_bf16x8, pa[j]), __builtin_bit_cast(pf_bf16x8, vb), oacc[j][d0 + d], 0, 0, 0);
            }
        }
    }
    // the four waves' partial outputs, added in pf_attn_kt_body's order: the only range of a tile is the tile's output, one of
    // several stays fp32 in part[slot][head][16][HD] for mc_px_reduce
#pragma unroll
    for (int j = 0; j < NH; j++)
#pragma unroll
        for (uint32_t ph = 0; ph < HD / OD; ph++) {
            __syncthreads(); // (the first: every wave is through with the exp window)
#pragma unroll
            for (uint32_t d = 0; d < OD / 16; d++)
#pragma unroll
                for (int i = 0; i < 4; i++) osum[wave][t.lg * 4 + i][d * 16 + t.l15] = oacc[j][ph * (OD / 16) + d][i];
            __syncthreads();
            float* po = part + ((size_t)blockIdx.y * H + h0 + j) * 16 * HD;
            for (uint32_t x = threadIdx.x; x < 16 * OD; x += blockDim.x) {
                const uint32_t rr = x / OD, d = x % OD, ro = (uint32_t)e.r0 + rr;
                const float o = (osum[0][rr][d] + osum[1][rr][d]) + (osum[2][rr][d] + osum[3][rr][d]);
                if (e.n > 1) po[rr * HD + ph * OD + d] = o;
                else if (ro < (uint32_t)g.len) out[((size_t)((uint32_t)g.off + ro) * H + h0 + j) * HD + ph * OD + d] = BF::st(o);
            }
        }
}

// grid (H, ranges of the launch), 256 threads: the workgroup of a tile's first range adds the tile's partial outputs in range order
template <uint32_t HD>
__device__ __forceinline__ void
px_reduce_body(const pp_seg* segs, const px_range* tab, uint32_t ebase, const float* part, bf16_t* out, uint32_t H)
{
    const uint32_t ei = ebase + blockIdx.y;
    const px_range e = tab[ei];
    if ((uint32_t)e.first != ei || e.n == 1) return;
    const pp_seg g = segs[e.seg];
    const uint32_t h = blockIdx.x;
    const uint32_t rows = min(16u, (uint32_t)(g.len - e.r0));
    const float* p0 = part + ((size_t)blockIdx.y * H + h) * 16 * HD;
    bf16_t* o0 = out + ((size_t)(g.off + e.r0) * H + h) * HD;
    for (uint32_t x = threadIdx.x; x < rows * HD; x += blockDim.x) {
        float s = 0.0f;
        for (int32_t i = 0; i < e.n; i++) s += p0[(size_t)i * H * 16 * HD + x];
        o0[(size_t)(x / HD) * H * HD + x % HD] = BF::st(s);
    }
}

#define MC_PX_ATTN(HD, NH, SFX)                                                                                                            \
    extern "C" __global__ void __launch_bounds__(256)                                                                                      \
    mc_px_sums##SFX##_bfloat_hd##HD(const bf16_t* Q, const pp_seg* segs, const px_range* tab, uint32_t ebase, const bf16_t* kc,              \
                                    uint64_t cache_stride, float* sums, uint32_t H, uint32_t n_rep, uint32_t max_seq, float scale,           \
                                    const float* etab)                                                                                     \
    {                                                                                                                                      \
        px_sums_body<HD, NH>(Q, segs, tab, ebase, kc, cache_stride, sums, H, n_rep, max_seq, scale, etab);                                   \
    }                                                                                                                                      \
    extern "C" __global__ void __launch_bounds__(256)                                                                                      \
    mc_px_pv##SFX##_bfloat_hd##HD(const bf16_t* Q, const pp_seg* segs, const px_range* tab, uint32_t ebase, const bf16_t* kc,                \
                                  const bf16_t* vt, uint64_t cache_stride, const float* sums, float* part, bf16_t* out, uint32_t H,            \
                                  uint32_t n_rep, uint32_t max_seq, float scale, const float* etab)                                        \
    {                                                                                                                                      \
        px_pv_body<HD, NH>(Q, segs, tab, ebase, kc, vt, cache_stride, sums, part, out, H, n_rep, max_seq, scale, etab);                      \
    }
MC_PX_ATTN(64, 1, )
MC_PX_ATTN(64, 2, 2)
MC_PX_ATTN(128, 1, )
MC_PX_ATTN(128, 2, 2)

#define MC_PX_REDUCE(HD)                                                                                                                   \
    extern "C" __global__ void __launch_bounds__(256)                                                                                      \
    mc_px_reduce_bfloat_hd##HD(const pp_seg* segs, const px_range* tab, uint32_t ebase, const float* part, bf16_t* out, uint32_t H)          \
    {                                                                                                                                      \
        px_reduce_body<HD>(segs, tab, ebase, part, out, H);                                                                                \
    }
MC_PX_REDUCE(64)
MC_PX_REDUCE(128)
