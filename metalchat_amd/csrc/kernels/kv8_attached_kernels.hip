// Chunks and verify calls on rows attached to the shared prefix of an fp8 batch (mc_attached_packed_set with mc_kv_prefix_set and mc_kv_packed_set
// on, include/metalchat_hip.h Part 2u): attached_kernels.hip's attention on the byte and exponent planes of kv8_kernels.hip.  The prefix is one more
// set of a row's four planes -- K bytes [kv][max_seq][hd], V bytes [kv][hd][max_seq], kexp and vexp [kv][max_seq] -- and serves the slots
// [0, shared) of every attached row; a row's slots from `shared` on are its own planes.
//
// The decomposition is mc_ax_*'s and is not restated here: 256 threads, grid (H / NH, units), wave w walks the 32-key blocks b = w (mod 4) from the
// unit's smallest k_lo to its largest k_hi, one accumulator per (tile, head, wave) that receives its blocks in ascending order, the Q fragments in
// LDS (ax_tiles_of, ax_score, ax_form and the LDS sizes are attached_kernels.hip's own), sums and part at the slot (range index - ebase), so that
// mc_px_reduce finishes a split tile.  The arithmetic of every (chunk row, head) is px8_sums_body's / px8_pv_body's (kv8_rows_kernels.hip), rounding
// point by rounding point: an attached row computes bit for bit what mc_px8_* computes on a row whose planes hold a byte copy of the prefix.
//
// What is new is what is shared.  On bytes the cost of a fragment is less its load than its CONVERSION to the bfloat16 MFMA operand (four
// v_cvt_scalef32_pk_bf16_fp8 per K k-step; four v_cvt_pk_f32_fp8, eight multiplies and four packs per V tile), which mc_px8_* pays once per
// (tile, head pair).  Here a block of the prefix is converted once for every (tile, head) of the unit whose range holds it:
//   K   a lane loads the 8 bytes d = 32 ks + 8 lg + [0, 8) of its key per k-step and the key's exponent (kv8_load_k against the prefix planes).
//       The block's two halves and the next block's first half stay BYTES while in flight -- 9 registers each at hd 128 where the bfloat16 form
//       holds 16 --, and a half becomes the operand (kv8_k_operand) right in front of its scores, in the same 16 registers as the other half.
//   P   mc_ax_pv: the scores of BOTH halves of every (tile, head) come first and leave the T NH P operands, packed bfloat16, in registers (at most
//       24).  So the two converted K halves are dead before the first V tile is converted ...
//   V   ... and the block's hd / 16 V tiles are converted one at a time: 8 bytes each, one 8-byte exponent load and eight 2^e per block
//       (kv8_scales8), a tile dequantised (kv8_deq8s) into 4 registers and multiplied into the T NH accumulators oacc[t][j][d] of that d before the
//       next tile is made -- d outermost, the pairs innermost.  Consecutive MFMAs go to different accumulators, and every accumulator still sees
//       only its own blocks in ascending order.  Holding all hd / 16 converted tiles and running the pairs outermost would take 32 registers for
//       them and 32 for the two K halves at once.
//   no masks in the prefix: every prefix slot lies below every tile's S (a row's positions start at or behind `shared`), and a full mask is the
//       identity, so the bits are those of kv8_slot_masks' all-ones case.
// A row's own blocks (b >= shared / 32) are loaded per tile from that tile's row with px8_pv_body's clamps: the key index at S - 1, the V and
// exponent address at max_seq - 8, and kv8_slot_masks on bytes AND exponents before the conversion -- an unwritten slot may hold a NaN byte
// (0x7f, 0xff) or exponent -128.
// Registers: T and NH are ax_tiles / ax_heads unchanged (192 accumulator registers; rows_plan.h's unit table serves both formats).  mc_ax8_pv:
// hd 128 210 VGPRs + 256 AGPRs / 93 SGPRs, hd 64 238 + 256 / 95; mc_ax8_sums 99 and 92 VGPRs.  What was short were SCALAR registers: mc_ax8_pv
// takes twelve 64-bit arguments that its three forms (NH = 4, 2, 1 behind one entry) held from the entry on, and the compiler spilled 16 to 18
// scalar registers to vector lanes.  The kernel therefore parks them in LDS at its entry and reads each where it is needed (ax8_pv_body).  No
// private segment, no spills, vector stores only.

// the key this lane loads of (block blk, half h): px_tile::load_k's deal, clamped to the last of S keys
__device__ __forceinline__ uint32_t
ax8_key(uint32_t blk, uint32_t h, uint32_t S, uint32_t l15)
{
    const uint32_t key = blk + 8 * (l15 >> 2) + 4 * h + (l15 & 3);
    return key < S ? key : S - 1;
}

// a value every lane holds alike, back in scalar registers
__device__ __forceinline__ uint64_t
ax8_uniform(uint64_t v)
{
    // (the builtin returns int: widened as it is, a low word with bit 31 set would fill the high word with ones)
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)v), hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(v >> 32));
    return (uint64_t)lo | (uint64_t)hi << 32;
}

// grid (H / NH, units of the launch), 256 threads.  ewin, qf, wsum: ax_sums_body's
template <uint32_t HD, int NH, int T>
__device__ __forceinline__ void
ax8_sums_body(const bf16_t* Q, const pp_seg* segs, const px_range* tab, const ax_unit* u, uint32_t ebase, const uint8_t* kq, const int8_t* kexp,
              const uint8_t* pkq, const int8_t* pkexp, uint64_t cache_stride, uint64_t exp_stride, float* sums, uint32_t H, uint32_t n_rep,
              uint32_t max_seq, uint32_t shared, float scale, const float* etab, float* ewin, uint4* qf, float* wsum)
{
    constexpr uint32_t DK = HD / 32;
    const pf_exp_window ew{ewin};
    ew.fill(etab);
    const uint32_t h0 = blockIdx.x * NH;
    const size_t kvoff = (size_t)(h0 / n_rep) * max_seq * HD, xoff = (size_t)(h0 / n_rep) * max_seq;
    ax_tiles_of<HD, NH, T> a;
    a.init(Q, segs, tab, u, H, h0, qf);
    const uint4* qfl = qf + a.lane;
    const uint8_t* pk = pkq + kvoff;
    const int8_t* px = pkexp + xoff;
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
    // the prefix's blocks of this wave: a half is converted once for every tile whose range holds the block
    const uint32_t P_end = min(a.B_end, shared / 32);
    uint32_t b = a.B_lo + a.wave;
    kv8_kfrag<HD> f0, f1;
    uint4 kb[DK];
    if (b < P_end) kv8_load_k<HD>(pk, px, ax8_key(b * 32, 0, shared, a.l15), a.kg, f0);
    __syncthreads(); // the exp window is filled, the Q fragments are there
    for (; b < P_end; b += 4) {
        kv8_load_k<HD>(pk, px, ax8_key(b * 32, 1, shared, a.l15), a.kg, f1);
        kv8_k_operand<HD>(f0, kb);
#pragma unroll
        for (int t = 0; t < T; t++)
            if (a.has(t, b)) add(t, kb, b, 0);
        if (b + 4 < P_end) kv8_load_k<HD>(pk, px, ax8_key((b + 4) * 32, 0, shared, a.l15), a.kg, f0);
        kv8_k_operand<HD>(f1, kb);
#pragma unroll
        for (int t = 0; t < T; t++)
            if (a.has(t, b)) add(t, kb, b, 1);
    }
    // the rows' own blocks: per tile from its row's planes
    for (; b < a.B_end; b += 4) {
#pragma unroll
        for (int t = 0; t < T; t++) {
            if (!a.has(t, b)) continue;
            const uint8_t* kr = kq + (size_t)a.row[t] * cache_stride + kvoff;
            const int8_t* xr = kexp + (size_t)a.row[t] * exp_stride + xoff;
            kv8_load_k<HD>(kr, xr, ax8_key(b * 32, 0, a.S[t], a.l15), a.kg, f0);
            kv8_load_k<HD>(kr, xr, ax8_key(b * 32, 1, a.S[t], a.l15), a.kg, f1);
            kv8_k_operand<HD>(f0, kb);
            add(t, kb, b, 0);
            kv8_k_operand<HD>(f1, kb);
            add(t, kb, b, 1);
        }
    }
    // ax_sums_body's tail: lane groups, then the waves as (w0 + w1) + (w2 + w3)
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

// what mc_ax8_pv parks in LDS at its entry (ax8_pv_body says why): the rows' planes, the prefix's, the two strides, part and out
enum { AX8_KQ, AX8_VQ, AX8_KEXP, AX8_VEXP, AX8_PKQ, AX8_PVQ, AX8_PKEXP, AX8_PVEXP, AX8_STRIDE, AX8_XSTRIDE, AX8_PART, AX8_OUT, AX8_LATER };

// grid (H / NH, units of the launch), 256 threads.  lds, qf, inv_sum: ax_pv_body's; later: the parked arguments
template <uint32_t HD, int NH, int T>
__device__ __forceinline__ void
ax8_pv_body(const bf16_t* Q, const pp_seg* segs, const px_range* tab, const ax_unit* u, uint32_t ebase, const float* sums, uint32_t H, uint32_t n_rep,
            uint32_t max_seq, uint32_t shared, float scale, const float* etab, float* lds, uint4* qf, float* inv_sum, const uint64_t* later)
{
    constexpr uint32_t DT = HD / 16, DK = HD / 32;
    constexpr uint32_t OD = HD < 128 ? HD : 128;
    const pf_exp_window ew{lds};
    ew.fill(etab);
    float (*osum)[16][OD + 1] = reinterpret_cast<float (*)[16][OD + 1]>(lds);
    const uint32_t h0 = blockIdx.x * NH;
    const size_t kvoff = (size_t)(h0 / n_rep) * max_seq * HD, xoff = (size_t)(h0 / n_rep) * max_seq;
    ax_tiles_of<HD, NH, T> a;
    a.init(Q, segs, tab, u, H, h0, qf);
    const uint4* qfl = qf + a.lane;
    // Scalar registers.  The kernel takes eight plane pointers, two strides, part and out -- four pointers and a stride more than mc_ax_pv --,
    // and held in scalar registers from the kernel's entry through the prefix loop they made the compiler spill 16 to 18.  So the kernel parks these
    // twelve in LDS at its entry (`later`, AX8_*), and each is read -- every lane alike, back into scalar registers -- where it is needed: the
    // prefix's planes in front of the prefix loop, the rows' behind it, part and out in the tail.  The tiles' block bounds are packed two to a word.
    uint32_t span[T]; // b_lo | b_end << 16: a block index is below max_seq / 32
#pragma unroll
    for (int t = 0; t < T; t++) span[t] = a.b_lo[t] | a.b_end[t] << 16;
    auto has = [&](int t, uint32_t b) { return b >= (span[t] & 0xFFFFu) && b < span[t] >> 16; }; // (uniform)
    // the rows' sums: the tile's ranges first to last (px8_pv_body)
    for (uint32_t x = threadIdx.x; x < (uint32_t)u->n * NH * 16; x += blockDim.x) {
        const uint32_t t = x / (NH * 16), j = x / 16 % NH, rr = x % 16;
        const px_range et = tab[u->range[t]];
        float s = 0.0f;
        for (int32_t i = 0; i < et.n; i++) s += sums[((size_t)((uint32_t)(et.first + i) - ebase) * H + h0 + j) * 16 + rr];
        inv_sum[(t * NH + j) * 16 + rr] = s == 0.0f ? 0.0f : 1.0f / s;
    }
    const uint32_t P_end = min(a.B_end, shared / 32);
    uint32_t b = a.B_lo + a.wave;
    kv8_kfrag<HD> f0, f1, fn;
    __syncthreads(); // the exp window is filled, the Q fragments, the sums and `later` are there
    const uint64_t* lt = later + ax_opaque_zero();
    const uint8_t *pk = reinterpret_cast<const uint8_t*>(ax8_uniform(lt[AX8_PKQ])) + kvoff, *pv = reinterpret_cast<const uint8_t*>(ax8_uniform(lt[AX8_PVQ])) + kvoff;
    const int8_t *px = reinterpret_cast<const int8_t*>(ax8_uniform(lt[AX8_PKEXP])) + xoff, *pvx = reinterpret_cast<const int8_t*>(ax8_uniform(lt[AX8_PVEXP])) + xoff;
    if (b < P_end) kv8_load_k<HD>(pk, px, ax8_key(b * 32, 0, shared, a.l15), a.kg, f0);
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
    // half h of block b against the operand kb: the packed probabilities of tile t's NH heads, two words each
    auto probs = [&](int t, const uint4 (&kb)[DK], uint32_t b, uint32_t h, uint32_t (&lo)[NH], uint32_t (&hi)[NH]) {
        const uint4* qb = qfl + ax_opaque_zero();
#pragma unroll
        for (int j = 0; j < NH; j++) {
            float sv[4];
            const float iv = inv[t][j];
            ax_score<HD>(kb, qb + (t * NH + j) * DK * 64, scale, b * 32, h, a.lg, a.live[t], a.pos_r[t], sv);
            lo[j] = pack_bf16x2(BF::rt(ew(sv[0]) * iv), BF::rt(ew(sv[1]) * iv));
            hi[j] = pack_bf16x2(BF::rt(ew(sv[2]) * iv), BF::rt(ew(sv[3]) * iv));
        }
    };
    // the prefix's blocks: every half and every V tile converted once (every slot of them is below every tile's S: nothing is masked)
    for (; b < P_end; b += 4) {
        uint2 vbs[DT];
        const uint32_t c = b * 32 + a.kg; // c + 8 <= shared <= max_seq
        // (the tiles' addresses step by a stride held in a vector register, so that no tile wants a scalar base of its own)
        const uint8_t* vp = pv + (size_t)a.l15 * max_seq + c;
        const uint32_t vstep = 16 * max_seq + ax_opaque_zero();
#pragma unroll
        for (uint32_t d = 0; d < DT; d++, vp += vstep) vbs[d] = *reinterpret_cast<const uint2*>(vp);
        const uint2 xb = *reinterpret_cast<const uint2*>(pvx + c);
        kv8_load_k<HD>(pk, px, ax8_key(b * 32, 1, shared, a.l15), a.kg, f1);
        const bool more = b + 4 < P_end;
        if (more) kv8_load_k<HD>(pk, px, ax8_key((b + 4) * 32, 0, shared, a.l15), a.kg, fn);
        uint32_t p0[T][NH], p1[T][NH], p2[T][NH], p3[T][NH];
        {
            uint4 kb[DK];
            kv8_k_operand<HD>(f0, kb);
#pragma unroll
            for (int t = 0; t < T; t++)
                if (has(t, b)) probs(t, kb, b, 0, p0[t], p1[t]);
            kv8_k_operand<HD>(f1, kb);
#pragma unroll
            for (int t = 0; t < T; t++)
                if (has(t, b)) probs(t, kb, b, 1, p2[t], p3[t]);
        }
        float vs[8];
        kv8_scales8(xb, vs);
#pragma unroll
        for (uint32_t d = 0; d < DT; d++) {
            const pf_bf16x8 vb = __builtin_bit_cast(pf_bf16x8, kv8_deq8s(vbs[d], vs));
#pragma unroll
            for (int t = 0; t < T; t++) {
                if (!has(t, b)) continue;
#pragma unroll
                for (int j = 0; j < NH; j++)
                    oacc[t][j][d] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(pf_bf16x8, make_uint4(p0[t][j], p1[t][j], p2[t][j], p3[t][j])), vb,
                                                                            oacc[t][j][d], 0, 0, 0);
            }
        }
        if (more) f0 = fn;
    }
    // the rows' own blocks: px8_pv_body's loads per tile -- the key clamped at S - 1, the V and exponent address at max_seq - 8, bytes and
    // exponents of the slots no row of the tile sees zeroed before the conversion
    const uint64_t* lo = later + ax_opaque_zero();
    const uint8_t *kr = reinterpret_cast<const uint8_t*>(ax8_uniform(lo[AX8_KQ])) + kvoff, *vr = reinterpret_cast<const uint8_t*>(ax8_uniform(lo[AX8_VQ])) + kvoff;
    const int8_t *kxr = reinterpret_cast<const int8_t*>(ax8_uniform(lo[AX8_KEXP])) + xoff, *vxr = reinterpret_cast<const int8_t*>(ax8_uniform(lo[AX8_VEXP])) + xoff;
    const uint64_t row_stride = ax8_uniform(lo[AX8_STRIDE]), rowx_stride = ax8_uniform(lo[AX8_XSTRIDE]);
    for (; b < a.B_end; b += 4) {
#pragma unroll
        for (int t = 0; t < T; t++) {
            if (!has(t, b)) continue;
            // (the tile's row and S from its table entries again, for the same reason)
            const px_range e = tab[u->range[t]];
            const pp_seg g = segs[e.seg];
            const uint32_t S = (uint32_t)g.pos + min((uint32_t)e.r0 + 16u, (uint32_t)g.len);
            const size_t rowoff = (size_t)g.row * row_stride, rowx = (size_t)g.row * rowx_stride;
            const uint32_t c = b * 32 + a.kg, cc = c + 8 <= max_seq ? c : max_seq - 8;
            const uint8_t* vp = vr + rowoff + (size_t)a.l15 * max_seq + cc;
            uint2 vbs[DT];
#pragma unroll
            for (uint32_t d = 0; d < DT; d++) vbs[d] = *reinterpret_cast<const uint2*>(vp + (size_t)d * 16 * max_seq);
            const uint2 xb = *reinterpret_cast<const uint2*>(vxr + rowx + cc);
            kv8_load_k<HD>(kr + rowoff, kxr + rowx, ax8_key(b * 32, 0, S, a.l15), a.kg, f0);
            kv8_load_k<HD>(kr + rowoff, kxr + rowx, ax8_key(b * 32, 1, S, a.l15), a.kg, f1);
            uint32_t p0[NH], p1[NH], p2[NH], p3[NH];
            {
                uint4 kb[DK];
                kv8_k_operand<HD>(f0, kb);
                probs(t, kb, b, 0, p0, p1);
                kv8_k_operand<HD>(f1, kb);
                probs(t, kb, b, 1, p2, p3);
            }
            uint32_t mlo, mhi;
            kv8_slot_masks(c, S, max_seq, mlo, mhi);
            float vs[8];
            kv8_scales8(make_uint2(xb.x & mlo, xb.y & mhi), vs);
#pragma unroll
            for (uint32_t d = 0; d < DT; d++) {
                const pf_bf16x8 vb = __builtin_bit_cast(pf_bf16x8, kv8_deq8s(make_uint2(vbs[d].x & mlo, vbs[d].y & mhi), vs));
#pragma unroll
                for (int j = 0; j < NH; j++)
                    oacc[t][j][d] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(pf_bf16x8, make_uint4(p0[j], p1[j], p2[j], p3[j])), vb, oacc[t][j][d], 0,
                                                                            0, 0);
            }
        }
    }
    // ax_pv_body's tail: the four waves' partial outputs of every (tile, head), added in px8_pv_body's order -- the only range of a tile is the
    // tile's output, one of several stays fp32 in part[slot][head][16][HD] for mc_px_reduce
    const uint64_t* la = later + ax_opaque_zero();
    float* const part = reinterpret_cast<float*>(ax8_uniform(la[AX8_PART]));
    bf16_t* const out = reinterpret_cast<bf16_t*>(ax8_uniform(la[AX8_OUT]));
#pragma unroll
    for (int t = 0; t < T; t++) {
        if (t >= u->n) continue; // (uniform)
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

// kq / vq / kexp / vexp: this layer of every batch row (cache_stride bytes and exp_stride bytes between rows), pkq / pvq / pkexp / pvexp: the
// prefix's planes of this layer; the other arguments are mc_ax_*'s
#define MC_AX8_ATTN(HD)                                                                                                                      \
    extern "C" __global__ void __launch_bounds__(256)                                                                                        \
    mc_ax8_sums_bfloat_hd##HD(const bf16_t* Q, const pp_seg* segs, const px_range* tab, const ax_unit* units, uint32_t ebase, uint32_t ubase, \
                              const uint8_t* kq, const int8_t* kexp, const uint8_t* pkq, const int8_t* pkexp, uint64_t cache_stride,         \
                              uint64_t exp_stride, float* sums, uint32_t H, uint32_t n_rep, uint32_t max_seq, uint32_t shared, float scale,  \
                              const float* etab)                                                                                             \
    {                                                                                                                                        \
        __shared__ __attribute__((aligned(16))) float ewin[AX_NW];                                                                           \
        __shared__ uint4 qf[AX_QF];                                                                                                          \
        __shared__ float wsum[AX_TH * 4 * 16];                                                                                               \
        const ax_unit* u = units + ubase + blockIdx.y;                                                                                       \
        ax_form<HD, ax_heads(HD, 4)>(n_rep, [&](auto nh, auto t) {                                                                           \
            ax8_sums_body<HD, decltype(nh)::value, decltype(t)::value>(Q, segs, tab, u, ebase, kq, kexp, pkq, pkexp, cache_stride, exp_stride, sums, H, n_rep, max_seq, shared, \
                                                                       scale, etab, ewin, qf, wsum);                                         \
        });                                                                                                                                  \
    }                                                                                                                                        \
    extern "C" __global__ void __launch_bounds__(256)                                                                                        \
    mc_ax8_pv_bfloat_hd##HD(const bf16_t* Q, const pp_seg* segs, const px_range* tab, const ax_unit* units, uint32_t ebase, uint32_t ubase,   \
                            const uint8_t* kq, const uint8_t* vq, const int8_t* kexp, const int8_t* vexp, const uint8_t* pkq, const uint8_t* pvq, \
                            const int8_t* pkexp, const int8_t* pvexp, uint64_t cache_stride, uint64_t exp_stride, const float* sums, float* part, \
                            bf16_t* out, uint32_t H, uint32_t n_rep, uint32_t max_seq, uint32_t shared, float scale, const float* etab)      \
    {                                                                                                                                        \
        __shared__ __attribute__((aligned(16))) float lds[AX_NW > AX_NO ? AX_NW : AX_NO];                                                    \
        __shared__ uint4 qf[AX_QF];                                                                                                          \
        __shared__ float inv_sum[AX_TH * 16];                                                                                                \
        __shared__ uint64_t later[AX8_LATER];                                                                                                \
        if (threadIdx.x == 0) {                                                                                                              \
            later[AX8_KQ] = (uint64_t)kq, later[AX8_VQ] = (uint64_t)vq, later[AX8_KEXP] = (uint64_t)kexp, later[AX8_VEXP] = (uint64_t)vexp;  \
            later[AX8_PKQ] = (uint64_t)pkq, later[AX8_PVQ] = (uint64_t)pvq, later[AX8_PKEXP] = (uint64_t)pkexp;                              \
            later[AX8_PVEXP] = (uint64_t)pvexp, later[AX8_STRIDE] = cache_stride, later[AX8_XSTRIDE] = exp_stride;                           \
            later[AX8_PART] = (uint64_t)part, later[AX8_OUT] = (uint64_t)out;                                                                \
        }                                                                                                                                    \
        const ax_unit* u = units + ubase + blockIdx.y;                                                                                       \
        ax_form<HD, ax_heads(HD, 4)>(n_rep, [&](auto nh, auto t) {                                                                           \
            ax8_pv_body<HD, decltype(nh)::value, decltype(t)::value>(Q, segs, tab, u, ebase, sums, H, n_rep, max_seq, shared, scale, etab, lds, qf, inv_sum, later); \
        });                                                                                                                                  \
    }
MC_AX8_ATTN(64)
MC_AX8_ATTN(128)
