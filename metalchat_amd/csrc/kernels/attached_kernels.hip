// Chunks and verify calls on rows attached to the shared prefix (mc_attached_packed_set, include/metalchat_hip.h Part 2t): the attention of
// extend_kernels.hip for the tiles of ATTACHED segments.  Such a row's slots [0, shared) are the prefix's planes (one copy for the batch, shared a
// multiple of 64), its slots from `shared` on its own planes at the same absolute numbers; ordinary tiles of the same call keep mc_px_sums /
// mc_px_pv, and a split attached tile is finished by mc_px_reduce as it is: sums and part are written at the slots (range index - ebase) the
// mc_px_* kernels would write.
//
// The arithmetic of every (chunk row, head) is px_sums_body's / px_pv_body's, rounding point by rounding point.  What is new is who loads what.
// Three facts of that code carry the design:
//   1. a tile's ranges depend on its own segment alone, and every range starts at a multiple of 128 keys: the wave that owns the 32-key block b
//      is b % 4 for every tile and every range, it adds its blocks in ascending order, and the waves are joined as (w0 + w1) + (w2 + w3);
//   2. the scores are S^T = K Q^T: the K fragment is one MFMA operand and the 16 chunk rows of ONE (tile, head) the other -- several (tile, head)
//      pairs against one K fragment are separate MFMAs into separate accumulators, nothing is padded and no bits are shared;
//   3. shared is a multiple of 64, so a 32-key block lies wholly in the prefix (32 (b + 1) <= shared) or wholly in the row's own slots.
// A workgroup (256 threads: four waves, one per SIMD) serves NH query heads of one kv head, a UNIT of up to T attached tiles -- of different
// rows, or of one long chunk -- and one range ordinal k: the k-th range of each of those tiles that has one (ax_unit, abi.h; the table is
// rows_plan.h's).  Wave w walks the blocks b = w (mod 4) from the smallest k_lo to the largest k_hi of these ranges.  Below shared / 32 it
// loads the K fragment (mc_ax_pv: the V fragments too) of a block ONCE from the prefix planes and runs every (tile, head) whose range holds the
// block; from shared / 32 on it loads per tile from that tile's row.  Each (tile, head, wave) keeps its own accumulator for the whole of its
// range -- the row sum, or the hd / 16 output tiles -- and receives exactly the blocks the per-row kernel gives it, in the same order; a range
// that starts in the prefix and ends in the row's slots runs through both loops in one accumulator.  The exp window, the -inf mask, the zeroing
// of V slots no row of the tile sees, inv_sum from the ranges' sums, the LDS wave sum and the choice between part and out are px_*_body's.
//
// Registers and LDS.  One wave per SIMD has 256 VGPRs + 256 AGPRs a lane.  mc_ax_pv's accumulators take T * NH * hd / 16 * 4 registers and live
// in the AGPRs -- but not in all of them: with 256 (T = 2 tiles x 4 heads at hd 128) the score MFMAs, whose results the compiler places in AGPRs
// as well, pushed accumulators out to a private segment (384 bytes, 156 spilled registers).  So the accumulators get 192 (abi.h AX_ACC_REGS), and
// heads and tiles are chosen for the most (tile, head) pairs per fragment: at hd 128 NH = 2 heads x T = 3 tiles (six pairs; four heads x one
// tile are four -- Llama-3-8B: eight attached tiles read K / V six times per kv head where mc_px_* reads them sixteen times), at hd 64 four heads
// x three tiles, and four tiles with fewer heads (abi.h ax_heads, ax_tiles).  The VGPRs hold three K fragments (the block's halves and the next
// block's first), hd / 16 V fragments, the P operand of one (tile, head) and the per-lane state of the tiles.  The Q operands of the unit would
// take T * NH * hd / 32 * 4 registers more (96), so they sit in LDS in MFMA fragment order -- [T][NH][hd / 32][64 lanes] of 16 bytes, at most
// 24 KiB, one conflict-free ds_read_b128 per MFMA -- beside the 32 KiB exp window (gfx950: 160 KiB per workgroup), and the tiles' table
// entries are read again behind the key loop rather than held in scalar registers through it.  A workgroup serves NH heads of ONE kv head, so
// n_rep 4 at hd 128 takes two workgroups per kv head and unit.

// the K fragment of (block blk, half h) in a plane `base` of one kv head: px_tile::load_k, clamped to the last of S keys
template <uint32_t HD>
__device__ __forceinline__ void
ax_load_k(const bf16_t* base, uint32_t blk, uint32_t h, uint32_t S, uint32_t l15, uint32_t kg, uint4 (&kb)[HD / 32])
{
    const uint32_t key = blk + 8 * (l15 >> 2) + 4 * h + (l15 & 3), keyc = key < S ? key : S - 1;
#pragma unroll
    for (uint32_t d = 0; d < HD / 32; d++) kb[d] = *reinterpret_cast<const uint4*>(base + (size_t)keyc * HD + d * 32 + kg);
}

// 0, which the compiler cannot see through: an LDS address formed with it inside the key loop keeps the loads of the Q fragments inside the loop
// (hoisted in front of it they are the T NH hd / 32 x 4 registers the fragments were put into LDS to save)
__device__ __forceinline__ uint32_t
ax_opaque_zero()
{
    uint32_t z = 0;
    asm volatile("" : "+v"(z));
    return z;
}

// px_tile::score for one head: qf = this lane's first Q fragment of the (tile, head) in LDS, the next 64 uint4 on
template <uint32_t HD>
__device__ __forceinline__ void
ax_score(const uint4 (&kb)[HD / 32], const uint4* qf, float scale, uint32_t blk, uint32_t h, uint32_t lg, bool live, uint32_t pos_r, float (&sv)[4])
{
    pf_f32x4 acc = {0, 0, 0, 0};
#pragma unroll
    for (uint32_t d = 0; d < HD / 32; d++)
        acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(pf_bf16x8, kb[d]), __builtin_bit_cast(pf_bf16x8, qf[d * 64]), acc, 0, 0, 0);
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const uint32_t key = blk + lg * 8 + h * 4 + i;
        const float s = BF::rt(BF::rt(acc[i]) * scale);
        sv[i] = bool(int(live) & int(key <= pos_r)) ? s : -INFINITY;
    }
}

// what a lane knows of the unit's tiles, and the Q fragments in LDS.  A tile past the unit's n has no block
template <uint32_t HD, int NH, int T>
struct ax_tiles_of {
    int32_t row[T]; // the tile's batch row
    uint32_t b_lo[T], b_end[T], pos_r[T], S[T];
    bool live[T];
    uint32_t B_lo, B_end, l15, lg, kg, lane, wave;

    __device__ __forceinline__ void
    init(const bf16_t* Q, const pp_seg* segs, const px_range* tab, const ax_unit* u, uint32_t H, uint32_t h0, uint4* qf)
    {
        constexpr uint32_t DK = HD / 32;
        lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
        l15 = lane & 15, lg = lane >> 4, kg = lg * 8;
        B_lo = 0xFFFFFFFFu, B_end = 0;
        const int32_t n = u->n;
#pragma unroll
        for (int t = 0; t < T; t++) {
            b_lo[t] = b_end[t] = pos_r[t] = 0;
            S[t] = 1;
            live[t] = false;
            row[t] = 0;
            if (t >= n) continue; // (uniform)
            const px_range e = tab[u->range[t]];
            const pp_seg g = segs[e.seg];
            row[t] = g.row;
            b_lo[t] = (uint32_t)e.k_lo / 32, b_end[t] = ((uint32_t)e.k_hi + 31) / 32;
            B_lo = min(B_lo, b_lo[t]), B_end = max(B_end, b_end[t]);
            const uint32_t r = (uint32_t)e.r0 + l15;
            live[t] = r < (uint32_t)g.len;
            pos_r[t] = live[t] ? (uint32_t)g.pos + r : 0u;
            S[t] = (uint32_t)g.pos + min((uint32_t)e.r0 + 16u, (uint32_t)g.len);
            const uint32_t qr = (uint32_t)g.off + min(r, (uint32_t)g.len - 1);
#pragma unroll
            for (int j = 0; j < NH; j++)
#pragma unroll
                for (uint32_t d = 0; d < DK; d++)
                    if (((t * NH + j) * DK + d) % 4 == wave) // (the fragments dealt over the waves)
                        qf[((t * NH + j) * DK + d) * 64 + lane] = *reinterpret_cast<const uint4*>(Q + ((size_t)qr * H + h0 + j) * HD + d * 32 + kg);
        }
        if (B_end == 0) B_lo = 0;
    }
    __device__ __forceinline__ bool has(int t, uint32_t b) const { return b >= b_lo[t] && b < b_end[t]; } // (uniform)
};

// grid (H / NH, units of the launch), 256 threads.  ewin: 2 N floats, qf: T NH hd / 32 x 64 fragments, wsum: [T NH][4][16]
template <uint32_t HD, int NH, int T>
__device__ __forceinline__ void
ax_sums_body(const bf16_t* Q, const pp_seg* segs, const px_range* tab, const ax_unit* u, uint32_t ebase, const bf16_t* kc, const bf16_t* pkc,
             uint64_t cache_stride, float* sums, uint32_t H, uint32_t n_rep, uint32_t max_seq, uint32_t shared, float scale, const float* etab,
             float* ewin, uint4* qf, float* wsum)
{
    constexpr uint32_t DK = HD / 32;
    const pf_exp_window ew{ewin};
    ew.fill(etab);
    const uint32_t h0 = blockIdx.x * NH;
    const size_t kvoff = (size_t)(h0 / n_rep) * max_seq * HD;
    ax_tiles_of<HD, NH, T> a;
    a.init(Q, segs, tab, u, H, h0, qf);
    const uint4* qfl = qf + a.lane;
    const bf16_t* pk = pkc + kvoff;
    float rsum[T][NH];
#pragma unroll
    for (int t = 0; t < T; t++)
#pragma unroll
        for (int j = 0; j < NH; j++) rsum[t][j] = 0.0f;
    auto add = [&](int t, const uint4 (&kb)[DK], uint32_t b, uint32_t h) {
        const uint4* qb = qfl + ax_opaque_zero();
#pragma unroll
        for (int j = 0; j < NH; j++) {
            float sv[4];
            ax_score<HD>(kb, qb + (t * NH + j) * DK * 64, scale, b * 32, h, a.lg, a.live[t], a.pos_r[t], sv);
            rsum[t][j] += (ew(sv[0]) + ew(sv[1])) + (ew(sv[2]) + ew(sv[3]));
        }
    };
    // the prefix's blocks of this wave: one K fragment for every tile whose range holds the block
    const uint32_t P_end = min(a.B_end, shared / 32);
    uint32_t b = a.B_lo + a.wave;
    uint4 k0[DK], k1[DK];
    if (b < P_end) ax_load_k<HD>(pk, b * 32, 0, shared, a.l15, a.kg, k0);
    __syncthreads(); // the exp window is filled, the Q fragments are there
    for (; b < P_end; b += 4) {
        ax_load_k<HD>(pk, b * 32, 1, shared, a.l15, a.kg, k1);
#pragma unroll
        for (int t = 0; t < T; t++)
            if (a.has(t, b)) add(t, k0, b, 0);
        if (b + 4 < P_end) ax_load_k<HD>(pk, (b + 4) * 32, 0, shared, a.l15, a.kg, k0);
#pragma unroll
        for (int t = 0; t < T; t++)
            if (a.has(t, b)) add(t, k1, b, 1);
    }
    // the rows' own blocks: per tile from its row's planes
    for (; b < a.B_end; b += 4) {
#pragma unroll
        for (int t = 0; t < T; t++) {
            if (!a.has(t, b)) continue;
            const bf16_t* kr = kc + (size_t)a.row[t] * cache_stride + kvoff;
            ax_load_k<HD>(kr, b * 32, 0, a.S[t], a.l15, a.kg, k0);
            ax_load_k<HD>(kr, b * 32, 1, a.S[t], a.l15, a.kg, k1);
            add(t, k0, b, 0);
            add(t, k1, b, 1);
        }
    }
#pragma unroll
    for (int t = 0; t < T; t++)
#pragma unroll
        for (int j = 0; j < NH; j++) {
            float s = rsum[t][j];
            s += __shfl_xor(s, 16, 64);
            s += __shfl_xor(s, 32, 64);
            if (a.lg == 0) wsum[((t * NH + j) * 4 + a.wave) * 16 + a.l15] = s;
        }
    __syncthreads();
    for (uint32_t x = threadIdx.x; x < (uint32_t)u->n * NH * 16; x += blockDim.x) {
        const uint32_t t = x / (NH * 16), j = x / 16 % NH, rr = x % 16;
        const float* w = wsum + (t * NH + j) * 64 + rr;
        sums[((size_t)((uint32_t)u->range[t] - ebase) * H + h0 + j) * 16 + rr] = (w[0] + w[16]) + (w[32] + w[48]);
    }
}

// grid (H / NH, units of the launch), 256 threads.  lds: the exp window and, behind the key loop, the waves' partial outputs (px_pv_body's
// buffer); qf as above; inv_sum: [T NH][16]
template <uint32_t HD, int NH, int T>
__device__ __forceinline__ void
ax_pv_body(const bf16_t* Q, const pp_seg* segs, const px_range* tab, const ax_unit* u, uint32_t ebase, const bf16_t* kc, const bf16_t* vt,
           const bf16_t* pkc, const bf16_t* pvt, uint64_t cache_stride, const float* sums, float* part, bf16_t* out, uint32_t H, uint32_t n_rep,
           uint32_t max_seq, uint32_t shared, float scale, const float* etab, float* lds, uint4* qf, float* inv_sum)
{
    constexpr uint32_t DT = HD / 16, DK = HD / 32;
    static_assert(DT <= 8, "the V fragments of a block are held at once");
    constexpr uint32_t OD = HD < 128 ? HD : 128;
    const pf_exp_window ew{lds};
    ew.fill(etab);
    float (*osum)[16][OD + 1] = reinterpret_cast<float (*)[16][OD + 1]>(lds);
    const uint32_t h0 = blockIdx.x * NH;
    const size_t kvoff = (size_t)(h0 / n_rep) * max_seq * HD;
    ax_tiles_of<HD, NH, T> a;
    a.init(Q, segs, tab, u, H, h0, qf);
    const uint4* qfl = qf + a.lane;
    const bf16_t *pk = pkc + kvoff, *pv = pvt + kvoff;
    // the rows' sums: the tile's ranges first to last (px_pv_body)
    for (uint32_t x = threadIdx.x; x < (uint32_t)u->n * NH * 16; x += blockDim.x) {
        const uint32_t t = x / (NH * 16), j = x / 16 % NH, rr = x % 16;
        const px_range et = tab[u->range[t]];
        float s = 0.0f;
        for (int32_t i = 0; i < et.n; i++) s += sums[((size_t)((uint32_t)(et.first + i) - ebase) * H + h0 + j) * 16 + rr];
        inv_sum[(t * NH + j) * 16 + rr] = s == 0.0f ? 0.0f : 1.0f / s;
    }
    const uint32_t P_end = min(a.B_end, shared / 32);
    uint32_t b = a.B_lo + a.wave;
    uint4 k0[DK], k1[DK], kn[DK];
    if (b < P_end) ax_load_k<HD>(pk, b * 32, 0, shared, a.l15, a.kg, k0);
    __syncthreads(); // the exp window is filled, the Q fragments and the sums are there
    float inv[T][NH];
    pf_f32x4 oacc[T][NH][DT];
#pragma unroll
    for (int t = 0; t < T; t++)
#pragma unroll
        for (int j = 0; j < NH; j++) {
            inv[t][j] = t < u->n ? inv_sum[(t * NH + j) * 16 + a.l15] : 0.0f;
#pragma unroll
            for (uint32_t d = 0; d < DT; d++) oacc[t][j][d] = pf_f32x4{0, 0, 0, 0};
        }
    // tile t's two score halves of block b become P, then P V into the tile's accumulators
    auto tile = [&](int t, const uint4 (&ka)[DK], const uint4 (&kb)[DK], const uint4 (&vb)[DT], uint32_t b) {
        const uint4* qb = qfl + ax_opaque_zero();
#pragma unroll
        for (int j = 0; j < NH; j++) {
            float sv[4];
            uint4 pa;
            const float iv = inv[t][j];
            ax_score<HD>(ka, qb + (t * NH + j) * DK * 64, scale, b * 32, 0, a.lg, a.live[t], a.pos_r[t], sv);
            pa.x = pack_bf16x2(BF::rt(ew(sv[0]) * iv), BF::rt(ew(sv[1]) * iv));
            pa.y = pack_bf16x2(BF::rt(ew(sv[2]) * iv), BF::rt(ew(sv[3]) * iv));
            ax_score<HD>(kb, qb + (t * NH + j) * DK * 64, scale, b * 32, 1, a.lg, a.live[t], a.pos_r[t], sv);
            pa.z = pack_bf16x2(BF::rt(ew(sv[0]) * iv), BF::rt(ew(sv[1]) * iv));
            pa.w = pack_bf16x2(BF::rt(ew(sv[2]) * iv), BF::rt(ew(sv[3]) * iv));
#pragma unroll
            for (uint32_t d = 0; d < DT; d++)
                oacc[t][j][d] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(pf_bf16x8, pa), __builtin_bit_cast(pf_bf16x8, vb[d]), oacc[t][j][d], 0, 0, 0);
        }
    };
    // the prefix's blocks: K and V fragments once (every slot of them is below every tile's S: no V element is masked)
    for (; b < P_end; b += 4) {
        uint4 vb[DT];
        const bf16_t* vp = pv + (size_t)a.l15 * max_seq + b * 32 + a.kg;
#pragma unroll
        for (uint32_t d = 0; d < DT; d++) vb[d] = *reinterpret_cast<const uint4*>(vp + (size_t)d * 16 * max_seq);
        ax_load_k<HD>(pk, b * 32, 1, shared, a.l15, a.kg, k1);
        const bool more = b + 4 < P_end;
        if (more) ax_load_k<HD>(pk, (b + 4) * 32, 0, shared, a.l15, a.kg, kn);
#pragma unroll
        for (int t = 0; t < T; t++)
            if (a.has(t, b)) tile(t, k0, k1, vb, b);
        if (more) {
#pragma unroll
            for (uint32_t d = 0; d < DK; d++) k0[d] = kn[d];
        }
    }
    // the rows' own blocks: px_pv_body's loads per tile -- the address clamped past max_seq, and the V of a slot no row of the tile sees
    // replaced by zero, element by element
    for (; b < a.B_end; b += 4) {
#pragma unroll
        for (int t = 0; t < T; t++) {
            if (!a.has(t, b)) continue;
            const size_t rowoff = (size_t)a.row[t] * cache_stride + kvoff;
            const uint32_t c = b * 32 + a.kg;
            const bool vin = c + 8 <= max_seq;
            const bf16_t* vp = vt + rowoff + (size_t)a.l15 * max_seq + (vin ? c : max_seq - 8);
            uint4 vb[DT];
#pragma unroll
            for (uint32_t d = 0; d < DT; d++) vb[d] = *reinterpret_cast<const uint4*>(vp + (size_t)d * 16 * max_seq);
            ax_load_k<HD>(kc + rowoff, b * 32, 0, a.S[t], a.l15, a.kg, k0);
            ax_load_k<HD>(kc + rowoff, b * 32, 1, a.S[t], a.l15, a.kg, k1);
            uint32_t m[4];
#pragma unroll
            for (uint32_t q = 0; q < 4; q++) {
                const uint32_t lo = (vin && c + 2 * q < a.S[t]) ? 0x0000FFFFu : 0u, hi = (vin && c + 2 * q + 1 < a.S[t]) ? 0xFFFF0000u : 0u;
                m[q] = lo | hi;
            }
#pragma unroll
            for (uint32_t d = 0; d < DT; d++) vb[d] = make_uint4(vb[d].x & m[0], vb[d].y & m[1], vb[d].z & m[2], vb[d].w & m[3]);
            tile(t, k0, k1, vb, b);
        }
    }
    // the four waves' partial outputs of every (tile, head), added in px_pv_body's order: the only range of a tile is the tile's output, one of
    // several stays fp32 in part[slot][head][16][HD] for mc_px_reduce
#pragma unroll
    for (int t = 0; t < T; t++) {
        if (t >= u->n) continue; // (uniform)
        // (the tile's table entries again: held through the key loop they are scalar registers it has no room for)
        const px_range e = tab[u->range[t]];
        const pp_seg g = segs[e.seg];
        const uint32_t slot = (uint32_t)u->range[t] - ebase;
#pragma unroll
        for (int j = 0; j < NH; j++)
#pragma unroll
            for (uint32_t ph = 0; ph < HD / OD; ph++) {
                __syncthreads(); // (the first: every wave is through with the exp window)
#pragma unroll
                for (uint32_t d = 0; d < OD / 16; d++)
#pragma unroll
                    for (int i = 0; i < 4; i++) osum[a.wave][a.lg * 4 + i][d * 16 + a.l15] = oacc[t][j][ph * (OD / 16) + d][i];
                __syncthreads();
                float* po = part + ((size_t)slot * H + h0 + j) * 16 * HD;
                for (uint32_t x = threadIdx.x; x < 16 * OD; x += blockDim.x) {
                    const uint32_t rr = x / OD, d = x % OD, ro = (uint32_t)e.r0 + rr;
                    const float o = (osum[0][rr][d] + osum[1][rr][d]) + (osum[2][rr][d] + osum[3][rr][d]);
                    if (e.n > 1) po[rr * HD + ph * OD + d] = o;
                    else if (ro < (uint32_t)g.len) out[((size_t)((uint32_t)g.off + ro) * H + h0 + j) * HD + ph * OD + d] = BF::st(o);
                }
            }
    }
}

// LDS of a workgroup: the exp window (mc_ax_pv: or the waves' partial outputs), the Q fragments, and the wave sums / the inverse row sums
constexpr uint32_t AX_QF = 3 * 2 * 4 * 64; // uint4: T NH hd / 32 fragments of 64 lanes, the most of the forms below
constexpr uint32_t AX_TH = 12;             // T NH, the most
constexpr uint32_t AX_NW = 2 * pf_exp_window::N, AX_NO = 4 * 16 * (128 + 1);

// the form of (HD, n_rep): NH = ax_heads, T = ax_tiles (abi.h)
template <uint32_t HD, int NH, typename F>
__device__ __forceinline__ void
ax_form(uint32_t n_rep, const F& f)
{
    constexpr int T = ax_tiles(HD, NH);
    static_assert(T * NH * (HD / 32) * 64 <= AX_QF && T * NH <= AX_TH, "the LDS of the form");
    if constexpr (NH > 1) {
        if (ax_heads(HD, (int)n_rep) != NH) return ax_form<HD, NH / 2>(n_rep, f);
    }
    f(std::integral_constant<int, NH>{}, std::integral_constant<int, T>{});
}

#define MC_AX_ATTN(HD)                                                                                                                     \
    extern "C" __global__ void __launch_bounds__(256)                                                                                      \
    mc_ax_sums_bfloat_hd##HD(const bf16_t* Q, const pp_seg* segs, const px_range* tab, const ax_unit* units, uint32_t ebase, uint32_t ubase, \
                             const bf16_t* kc, const bf16_t* pkc, uint64_t cache_stride, float* sums, uint32_t H, uint32_t n_rep,            \
                             uint32_t max_seq, uint32_t shared, float scale, const float* etab)                                            \
    {                                                                                                                                      \
        __shared__ __attribute__((aligned(16))) float ewin[AX_NW];                                                                         \
        __shared__ uint4 qf[AX_QF];                                                                                                        \
        __shared__ float wsum[AX_TH * 4 * 16];                                                                                             \
        const ax_unit* u = units + ubase + blockIdx.y;                                                                                     \
        ax_form<HD, ax_heads(HD, 4)>(n_rep, [&](auto nh, auto t) {                                                                         \
            ax_sums_body<HD, decltype(nh)::value, decltype(t)::value>(Q, segs, tab, u, ebase, kc, pkc, cache_stride, sums, H, n_rep, max_seq, shared, scale, etab, ewin, qf, wsum); \
        });                                                                                                                                \
    }                                                                                                                                      \
    extern "C" __global__ void __launch_bounds__(256)                                                                                      \
    mc_ax_pv_bfloat_hd##HD(const bf16_t* Q, const pp_seg* segs, const px_range* tab, const ax_unit* units, uint32_t ebase, uint32_t ubase,  \
                           const bf16_t* kc, const bf16_t* vt, const bf16_t* pkc, const bf16_t* pvt, uint64_t cache_stride, const float* sums, \
                           float* part, bf16_t* out, uint32_t H, uint32_t n_rep, uint32_t max_seq, uint32_t shared, float scale,           \
                           const float* etab)                                                                                              \
    {                                                                                                                                      \
        __shared__ __attribute__((aligned(16))) float lds[AX_NW > AX_NO ? AX_NW : AX_NO];                                                  \
        __shared__ uint4 qf[AX_QF];                                                                                                        \
        __shared__ float inv_sum[AX_TH * 16];                                                                                              \
        const ax_unit* u = units + ubase + blockIdx.y;                                                                                     \
        ax_form<HD, ax_heads(HD, 4)>(n_rep, [&](auto nh, auto t) {                                                                         \
            ax_pv_body<HD, decltype(nh)::value, decltype(t)::value>(Q, segs, tab, u, ebase, kc, vt, pkc, pvt, cache_stride, sums, part, out, H, n_rep, max_seq, shared, scale, etab, lds, qf, \
                                              inv_sum);                                                                                    \
        });                                                                                                                                \
    }
MC_AX_ATTN(64)
MC_AX_ATTN(128)

