// Which kernel a decode GEMV takes, and its grid, workgroup and LDS bytes: plan_gemv().  Pure integer arithmetic on five fields of the linear, the
// (prologue, epilogue) pair, the element size, the arithmetic mode, the CU count and the MC_GEMV_* / MC_LIN* switches -- no HIP, no mc_decoder, so the
// choice can be asked without walking the launch path (mc_decoder_gemv_kernel_name) and is pinned on the CPU, grid and LDS included
// (tests/cpp/test_gemv_plan.cc against tests/golden/decode_gemv_plans.json).  mc_decoder::gemv() launches what the plan says and decides nothing.
#pragma once

#include <algorithm>
#include <cstdint>
#include <string>

#include "../../include/metalchat_hip.h" // MC_WFMT_*, MC_QMODE_*
#include "decoder_options.h"

struct gemv_shape { // of a linear_w
    int fmt, out, in, group, lora_cols;
};
struct gemv_env { // of a decoder, fixed when it is created
    int tb; // sizeof(T)
    int qmode;
    unsigned cus;        // compute units of the device
    unsigned pick_slots; // keys EPI_STORE_PICK may leave (mc_decoder::pick_slots)
    const decoder_options* opt;
};
// the suffix the host writes:  (none)   _fast  _m4  _m4d  _lin<n>  _lin12k4  _lin3s   _ling<n>
enum class gemv_family { classic, fast, m4, m4d, lin, lin_k4, lin_split, ling };
struct gemv_plan {
    gemv_family family = gemv_family::classic;
    int rows_kib = 0; // lin / lin_k4: row length in KiB (K / 2048); ling: KiB per row; 0 for the others
    std::string name;
    unsigned wgs = 1, block = 256, lds = 0;
    bool postnorm_by_value = false; // pro == 2 on lin / lin_split: the post-norm's three pointers go in the adaptor's argument slots (gemv.h)
    const char* error = nullptr;    // non-null: no kernel serves the request
};

inline size_t
gemv_row_bytes(int fmt, int in, int tb)
{
    if (fmt == MC_WFMT_I4) return (size_t)in / 2;
    if (fmt == MC_WFMT_I8) return (size_t)in;
    return (size_t)in * tb;
}
// THE int4-MFMA gate -- exact int4 on bfloat rows: dot products on the 4x4x4 MFMA (_m4) ...
inline bool
gemv_i4_mfma(const gemv_shape& L, const gemv_env& e)
{
    return L.fmt == MC_WFMT_I4 && e.tb == 2 && e.qmode == MC_QMODE_EXACT && e.opt->gemv_m4 && !e.opt->dbg_variant;
}
// ... and with scale groups that are whole 128-weight lane blocks the dequantisation can go there too (_m4d, gemv.h Q_M4D)
inline bool
gemv_m4d_ok(const gemv_shape& L, const gemv_env& e)
{
    return gemv_i4_mfma(L, e) && (L.group == 0 || L.group % 128 == 0) && L.in % 128 == 0;
}
// rows of whole KiB of int4 (K a multiple of 2048): that count, 0 = no
inline int
gemv_nch(const gemv_shape& L)
{
    return L.in % 2048 == 0 ? L.in / 2048 : 0;
}

// does this linear take the linear-order kernels (gemv.h)?  int4 on bfloat rows, exact arithmetic, scale groups of
// whole 128-weight lane blocks, rows of 1, 2, 4, 7, 12 or 14 whole KiB, whole row groups
inline bool
lin_ok(const gemv_shape& L, const gemv_env& e)
{
    const int nch = gemv_nch(L);
    return e.opt->gemv_lin && gemv_m4d_ok(L, e) && L.out % 4 == 0 && (nch == 1 || nch == 2 || nch == 4 || nch == 7 || nch == 12 || nch == 14);
}
// ... rows of 1.5 KiB (K = 3072: Gemma-7B's QKV and w1|w3), two to a 3 KiB super row (gemv.h LSPLIT, `_lin3s_`)
inline bool
lin_split_ok(const gemv_shape& L, const gemv_env& e)
{
    return e.opt->gemv_lin && e.opt->lin_split && gemv_i4_mfma(L, e) && L.group == 128 && L.in == 3072 && L.out % 4 == 0 && e.opt->lin_waves == 8 && !L.lora_cols;
}
// ... or the linear-order kernels of the VALU-dequantising formats (gemv.h LGEN): int8 / plain bfloat weights on
// bfloat rows, rows of 4 / 14 (int8) or 4 / 8 / 11 / 16 (bfloat) whole KiB; returns that count, 0 = no
inline int
ling_kib(const gemv_shape& L, const gemv_env& e)
{
    const decoder_options& opt = *e.opt;
    if (!opt.gemv_lin || !opt.gemv_ling || e.tb != 2 || opt.dbg_variant || L.out % 4 != 0) return 0;
    const size_t rb = gemv_row_bytes(L.fmt, L.in, e.tb);
    if (rb % 1024) return 0;
    const int n = (int)(rb / 1024);
    if (L.fmt == MC_WFMT_I8) {
        const bool g_ok = L.group == 0 || (L.group % 16 == 0 && (L.group & (L.group - 1)) == 0);
        return g_ok && (n == 4 || (n == 14 && opt.i8_ling14)) ? n : 0;
    }
    if (L.fmt == MC_WFMT_T) return (n == 4 || n == 8 || n == 11 || n == 16) ? n : 0;
    return 0;
}

// The grid of every linear-order kernel: ONE workgroup of opt.lin_waves (eight) waves per CU -- the activation row is staged once per CU and, with the
// raw barrier between the row requests and the first weight requests (gemv.h MC_GEMV_XBAR), always ahead of the weight stream in the CU's in-order
// memory pipe (w1|w3: 16.2 us against 17.3 with two four-wave workgroups; the kernels are built for exactly this workgroup size, gemv_kernels.hip
// MC_LIN_WAVES: no blockDim load).  A CU takes in ~25 GB/s whatever its waves do, so what matters is equal BYTES PER CU: a whole multiple of the CU
// count, at least one unit of the loop per wave (the kernel cuts the units into equal contiguous ranges).  `units` is what the loop of the family
// counts: row pairs (lin, ling), quads of rows = two super rows (lin_split).  `at_least`: the ling_half widening, in workgroups.
inline unsigned
gemv_lin_cap(const gemv_env& e)
{
    return e.cus * (e.opt->gemv_block_env ? (unsigned)e.opt->gemv_wgs_per_cu : 1u);
}
inline unsigned
gemv_grid_per_cu(unsigned units, const gemv_env& e, unsigned at_least = 0)
{
    const unsigned waves = (unsigned)e.opt->lin_waves, cap = gemv_lin_cap(e);
    unsigned wgs = std::max((units + waves - 1) / waves, at_least);
    if (wgs > cap) wgs = cap;
    if (wgs > e.cus) wgs = wgs / e.cus * e.cus;
    return wgs;
}

inline gemv_plan
plan_gemv(const gemv_shape& L, const gemv_env& e, int pro, int epi)
{
    const decoder_options& opt = *e.opt;
    const unsigned cus = e.cus;
    gemv_plan P;
    // ---- the family, in priority order: the first whose gate holds
    const int nch = gemv_nch(L);
    // 1. lin (an adapted linear behind a post-norm: the linear-order `_p2_` kernels take the post-norm's pointers in the adaptor's argument slots,
    //    gemv.h -- the classic kernels serve that combination)
    const bool lin = lin_ok(L, e) && !(pro == 2 && L.lora_cols);
    // 2. lin_split, for the (prologue, epilogue) pairs gemv_kernels.hip instantiates it with
    const int pe_code = pro * 10 + epi;
    const bool lins = !lin && lin_split_ok(L, e) &&
                      (pe_code == 0 || pe_code == 10 || pe_code == 1 || pe_code == 12 || pe_code == 13 || pe_code == 14 || pe_code == 20 || pe_code == 23);
    // 3. ling (no post-norm prologue)
    const int ling = lin || lins || pro == 2 ? 0 : ling_kib(L, e);
    if (pro == 3 && !lin && !ling) {
        P.error = "gemv: the partial-sum prologue exists for the linear-order kernels only";
        return P;
    }
    // 4. the classic kernels.  Grid: one workgroup per four row groups, capped at opt.gemv_wgs_per_cu workgroups per CU (a
    // whole multiple of the CU count: what has to balance is the work per CU -- its SIMDs
    // time-share their waves -- so 3.5 row groups per wave on every CU beats an even 4 per
    // wave on 448 workgroups, measured 19.0 vs 21.4 us on the 60 MB w1|w3 matrix).
    const unsigned classic_block = (unsigned)opt.gemv_block, classic_waves = classic_block / 64;
    const unsigned ng = ((unsigned)L.out + 3) / 4;
    unsigned classic_wgs = opt.gemv_full_grid ? ng : (ng + classic_waves - 1) / classic_waves;
    classic_wgs = std::max(1u, std::min(classic_wgs, cus * (unsigned)opt.gemv_wgs_per_cu));
    // ... of exact int4 on bfloat rows with the dot products on the MFMA (_m4), and the dequantisation too (_m4d) -- when
    // a SIMD holds more than one wave of the launch: the MFMA -> cvt_pk -> MFMA chain of a weight
    // is longer than the VALU one and a lone wave per SIMD (Wo, w2: 1024 row groups) has nobody
    // to hide it behind (8.2 vs 8.5 us per launch, profiles/r01_kernel_stats.csv).
    const bool shared_simd = std::min(classic_wgs * classic_waves, ng) > 4u * cus; // waves that own a row group
    const bool m4d = gemv_m4d_ok(L, e) && (opt.gemv_m4 >= 3 || (opt.gemv_m4 == 2 && shared_simd));
    // long rows, few of them (Gemma-7B's w2: 1536 pairs of 12 KiB rows = one pair per wave on 192 CUs): the K range of a pair over four waves of a
    // workgroup on EVERY CU (gemv_ksplit.h) -- at most eight pairs per workgroup, plain store or residual add, no adaptor
    const bool k4 = lin && opt.lin_k4_on && nch == 12 && pro == 0 && (epi == 0 || epi == 1) && !L.lora_cols && opt.lin_waves == 8 &&
                    (unsigned)L.out / 2 >= 4u * cus && ((unsigned)L.out / 2 + cus - 1) / cus <= 8u;
    const bool fast = L.fmt == MC_WFMT_I4 && e.tb == 2 && e.qmode == MC_QMODE_FAST;
    P.family = lin ? (k4 ? gemv_family::lin_k4 : gemv_family::lin)
             : lins ? gemv_family::lin_split
             : ling ? gemv_family::ling
             : gemv_i4_mfma(L, e) ? (m4d ? gemv_family::m4d : gemv_family::m4)
             : fast ? gemv_family::fast : gemv_family::classic;
    P.rows_kib = lin ? nch : ling;
    P.postnorm_by_value = pro == 2 && (lin || lins);

    // ---- grid, workgroup and LDS of that family.  LDS: the activation row zero-padded to whole chunks (64 lanes x 16 B of packed weights); where the
    // kernel reads it transposed (_m4d and the int4 linear-order kernels) 16 bytes of padding per 256; 128 bytes of scratch; and for the linear-order
    // kernels the parked row sums, 64 pairs x 8 bytes per wave (gemv.h PARKB)
    const unsigned kpl = L.fmt == MC_WFMT_I4 ? 32 : (L.fmt == MC_WFMT_I8 ? 16 : (e.tb == 2 ? 8 : 4));
    const unsigned chunk = 64 * kpl;
    const unsigned row = (unsigned)((size_t)((L.in + chunk - 1) / chunk) * chunk * e.tb);
    const unsigned lin_block = 64u * (unsigned)opt.lin_waves, parked = (unsigned)opt.lin_waves * 512u;
    const unsigned np = (unsigned)L.out / 2;
    std::string suffix;
    switch (P.family) {
    case gemv_family::lin:
    case gemv_family::lin_k4:
        suffix = "_lin" + std::to_string(nch) + (k4 ? "k4" : "");
        P.wgs = k4 ? cus : gemv_grid_per_cu(np, e);
        P.block = lin_block;
        P.lds = row / 16 * 17 + 128 + parked;
        break;
    case gemv_family::lin_split:
        suffix = "_lin3s";
        P.wgs = gemv_grid_per_cu((unsigned)L.out / 4, e);
        P.block = lin_block;
        P.lds = 3u * chunk * (unsigned)e.tb / 16 * 17 + 128 + parked; // the row twice: [x, x] = three chunks of 2048
        break;
    case gemv_family::ling: {
        suffix = "_ling" + std::to_string(ling);
        // fewer pairs than half the waves a full grid has (the 2048-row matrices of the small models) and an epilogue that
        // treats the rows of a pair separately: one ROW per wave (gemv.h LGEN, `half`)
        const unsigned waves = (unsigned)opt.lin_waves, cap = gemv_lin_cap(e);
        const bool half = opt.ling_half && (epi == 0 || epi == 1) && !L.lora_cols && 2u * np <= cap * waves && (unsigned)L.out % 2 == 0;
        P.wgs = gemv_grid_per_cu(np, e, half ? std::min(cap, ((unsigned)L.out + waves - 1) / waves) : 0u);
        P.block = lin_block;
        P.lds = row + 128 + parked;
        break;
    }
    case gemv_family::m4d:
    case gemv_family::m4:
    case gemv_family::fast:
    case gemv_family::classic:
        suffix = P.family == gemv_family::m4d ? "_m4d" : P.family == gemv_family::m4 ? "_m4" : P.family == gemv_family::fast ? "_fast" : "";
        P.wgs = classic_wgs;
        P.block = classic_block;
        P.lds = (P.family == gemv_family::m4d ? row / 16 * 17 : row) + 128;
        break;
    }
    // the tuning ablations of the classic int4 kernels (MC_GEMV_DBG: the gate above is off under it)
    if (L.fmt == MC_WFMT_I4 && e.tb == 2 && opt.dbg_variant && ((pro == 1 && epi == 2) || (pro == 0 && epi == 0)))
        suffix += opt.dbg_variant == 1 ? "_dbgstream" : "_dbgnoload";
    P.name = std::string("mc_gemv_") + (L.fmt == MC_WFMT_I4 ? "i4_" : (L.fmt == MC_WFMT_I8 ? "i8_" : "w_")) + (e.tb == 2 ? "bfloat" : "float") + suffix +
             "_p" + std::to_string(pro) + "_e" + std::to_string(epi);
    // EPI_STORE_PICK leaves one key per workgroup in pick_keys (pick_slots of them, folded by mc_argmax_keys)
    if (epi == 5 && P.wgs > e.pick_slots) P.wgs = e.pick_slots;
    return P;
}
