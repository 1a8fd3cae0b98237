// The MC_* switches of the decoder (decoder.cc): one struct, read once from the environment when a decoder is created.  Standard headers only, so that
// what depends on the switches alone -- which kernel a decode GEMV takes, gemv_plan.h -- can be compiled and tested without HIP.
#pragma once

#include <algorithm>
#include <climits>
#include <cstdlib>

// Every switch of decoder.cc: the MC_* environment variables, read ONCE when a decoder is created (read_options below holds every getenv("MC_...") of
// decoder.cc).  A switch keeps the name, default, clamp and meaning it was introduced with; the measurements behind a default stay next to its field.
struct decoder_options {
    // ---- the decode GEMVs (gemv_plan.h plan_gemv)
    int gemv_block = 256;        // MC_GEMV_BLOCK: threads of a classic GEMV workgroup (a multiple of 64 in [64, 1024], else 256)
    int gemv_wgs_per_cu = 2;     // MC_GEMV_WGS_PER_CU (at least 1, else 2)
    bool gemv_block_env = false; // MC_GEMV_BLOCK / MC_GEMV_WGS_PER_CU given: they apply to every kernel of the family
    bool gemv_lin = true;        // MC_GEMV_LIN=0: classic kernels everywhere (A/B)
    bool gemv_ling = true;       // MC_GEMV_LING=0: int8 / bfloat weights on the classic kernels (A/B)
    bool i8_ling14 = true;       // MC_I8_LING14=0: int8 rows of 14 KiB (w2 of Llama-3-8B) on the classic kernel (A/B)
    bool lin_split = true;       // MC_LIN_SPLIT=0: K = 3072 on the classic kernels (A/B)
    bool ling_half = true;       // MC_LING_HALF=0: whole row pairs per wave whatever the matrix (A/B)
    bool lin_k4_on = true;       // MC_LIN_K4=0: Gemma-7B's w2 on the one-pair-per-wave kernel (mc_gemv_i4_bfloat_lin12_*) instead of the K-split one (A/B, parity)
    int lin_waves = 8;           // MC_LIN_WAVES (1 .. 16): tuning builds of the linear-order kernels with another workgroup size
    bool gemv_full_grid = false; // MC_GEMV_FULLGRID=1: as many workgroups as CUs allow even when that leaves waves without a row group (kernels built with MC_GEMV_WAVEMAJOR)
    int dbg_variant = 0;         // MC_GEMV_DBG=1 stream-only, 2 compute-only (tuning ablations)
    int gemv_m4 = 2;             // MC_GEMV_M4: 0 = exact int4 on the VALU (v_dot2c), 1 = dot products on the 4x4x4 MFMA, 2 = dequantisation too where a SIMD holds > 1 wave, 3 = always
    int time_gemv_layers = 0;    // MC_TIME_GEMV_LAYERS=n (tuning aid of mc_decoder_time_gemv): every "layer" of the pass uses the weights of layer
                                 // i % n, so with a small n the matrices stay resident in the 256 MiB Infinity Cache; 0 = every layer its own
    // ---- the decode attention block (plan_block)
    bool attn_fused = true;      // MC_ATTN_FUSED=0: scores and P.V as two launches (A/B, parity).  What the configuration asked for: mc_decoder::attn_fused_on is
                                 // what holds now (handoff_failed, note_clean_tokens)
    // ... while the launch is at most this many 256-thread workgroups per CU (MC_ATTN_FUSED_WGS, 1 .. 4).  Measured: at S = 8192 with
    // 64-slot ranges (128 ranges x 8 kv heads = 4 per CU, every hand-off gathering from 128 producers) the one launch took 27.8 us
    // against 6.3 + 8.5 for the two -- long contexts keep the two-launch form (wider ranges were built and measured no better)
    unsigned attn_fused_max_wgs_per_cu = 2;
    bool attn_t2_on = true;      // MC_ATTN_T2
    int rearm_after = 256;       // MC_HANDOFF_REARM: tokens without a hand-off launch after which a fallen-back decoder takes the one-launch blocks again (0: never;
                                 // mc_decoder::rearm_after starts here and doubles)
    bool handoff_fast = true;    // MC_HANDOFF_FAST=0: hand-offs A and B through the fabric only (A/B; handoff.h "the XCD-local fast path")
    bool attn_wo_on = true;      // MC_ATTN_WO=0: the Wo GEMV as a launch of its own behind the one-launch attention (A/B, parity)
    bool attn_wo_k4 = false;     // MC_ATTN_WO_K4 set: mc_attn_wo_i4_*_hd128_k4 (K = 8192, Llama-3-70B: measured slower than the two launches -- attn_block_kernels.hip)
    bool attn_qkv_on = true;     // MC_ATTN_QKV=0: wq|wk|wv as a launch of its own in front of mc_attn_wo_* (A/B, parity)
    // MC_ATTN_QKV_ONLY=1: the 70B shapes' wq|wk|wv GEMV inside the attention launch (mc_attn_qkv_i4_bfloat_hd128_q4).  Built in round 5 as VERDICT r04
    // item 2 (iv) asked, bit for bit the two launches, and NOT faster: 21.25 us against 11.65 + 9.04 in the trace (profiles/r05_kernel_stats_70b_qkvin.csv),
    // 127.4 / 127.1 against 128.0 / 127.9 tokens/s alternating on one box -- 160 KB of wq|wk|wv per workgroup are 7 us of multiplication in front of
    // the first hand-off, which is what the GEMV launch lasts.  Off by default.
    bool attn_qkv_only_on = false;
    bool attn_i8_on = true;      // MC_ATTN_I8: int8 wq|wk|wv and Wo inside the attention launch (plan_block: qkv_wo_i8)
    bool attn_i4_wide_on = true; // MC_ATTN_I4_WIDE: the int4 block with 128- / 256-slot ranges at S = 4096 / 8192 (plan_block: qkv_wo_i4 with tiles > 1)
    bool kv_virtual_on = true;   // MC_KV_VIRTUAL: fewer than 8 kv heads launched as 8 virtual ones where wq|wk|wv is inside the attention launch (kv_virtual_shift)
    bool chain_w13_on = true;    // MC_CHAIN_W13=0: ffn_norm + w1|w3 + act*mul as a launch of its own behind the plain-weight attention block (A/B, parity)
    int chain_f = -1;            // MC_CHAIN_F: pairs per fetcher wave of that chain instead of the rule's (tuning: tools/ab_case_multi.sh); -1 = not given
    bool attn_qkv_qkn_on = true; // MC_ATTN_QKV_QKN=0: gemma3's wq|wk|wv GEMV as a launch of its own in front of mc_attn_wo_qkn_* (A/B, parity)
    bool attn_wo_qkn_on = true;  // MC_ATTN_WO_QKN=0: gemma3's q/k-norm + rope + cache write + attention as mc_attn_fused_qkn_T, Wo as a GEMV of its own (A/B, parity)
    bool attn_qkn_on = true;     // MC_ATTN_QKN=0: gemma3's q/k-norm + rope + cache write as a launch of their own (mc_rope_kv_T) in front of the attention (A/B, parity)
    bool gemma_fuse = true;      // MC_GEMMA_UNFUSED=1: keep the post-norms as launches of their own
    bool pv_fold_on = true;      // MC_PV_FOLD=0: P.V ranges reduced by their own launch (A/B, parity)
    int pv_block = 1024;         // MC_PV_BLOCK: threads of a P.V workgroup (16 waves: one round of loads per wave at S = 2048; a multiple of 64 in [256, 1024], else 1024)
    int pv_ranges = 0;           // MC_PV_RANGES (1 .. 64): ranges of the P.V launch; 0 = not given, by the context length (mc_decoder_create)
    // ---- the output head
    int head_pick_mode = 2;
    bool head_pick_on = true;    // MC_HEAD_PICK: 0 = mc_argmax_T behind the head (round 1); 1 = the pick wholly inside the head's launch (atomic max
                                 // + ticket per workgroup: parity-green, 1448 vs 1449 us per token -- the atomics cost what the launch costs);
                                 // 2 = one key per workgroup + mc_argmax_keys, a one-workgroup launch over 8 KB instead of 256 KB of logits
    bool lazy_pick_on = true;    // MC_LAZY_PICK
    // ---- the prompt pass
    bool pf2_on = true;          // MC_PF2: short prompts from the quad-interleaved copy
    int pf2_wgs_per_cu = 1;      // MC_PF2_WGS_PER_CU (at least 1): workgroups per CU pf2_split aims at
    bool pf_attn8_on = true;     // MC_PF_ATTN8: the prompt attention with K / V tiles through LDS, from pf_attn8_rows rows on
    int pf_attn8_rows = 1024;    // MC_PF_ATTN8_ROWS
    int pf_attn8_rows64 = 1793;  // MC_PF_ATTN8_ROWS64 (head_dim 64: mc_pf_attn8_bfloat_hd64_h{8,4}; TinyLlama 2048 rows 8.35 against 8.95 ms, Llama-3.2-1B 6.57 against 7.0; 1536 - 1792 rows equal, 1024: 5.1 against 4.9 -- profiles/r06_pf_hd64_attn8_ab.log)
    int pf_attn8_rows256 = 513;  // MC_PF_ATTN8_ROWS256 (head_dim 256: mc_pf_attn8_bfloat_hd256; Gemma-7B shapes: 2048 rows 35.5 against 44.4 ms, 1024: 19.0 against 21.3, 512: equal, 256: 9.0 against 8.85)
    int pf_attn_heads = -1;      // MC_PF_ATTN_HEADS=1 / 2 / 4 / 8: the prompt attention kernel by its query heads per workgroup instead of by the rules of prefill(); -1 = not given
    int pf_attn8_pair = -1;      // MC_PF_ATTN8_PAIR=0 / 1: row tiles of the LDS-tile attention one per workgroup / in pairs; -1 = not given, by the grid
    int pf_plain_mode = -1;      // MC_PF_PLAIN_COPY: 1 = the 256 x 256 prompt GEMM multiplies quantised matrices from their dequantised bfloat16 copy (linear_w::wd, built on
                                 // first use, 2 bytes per weight more HBM: the very values the quantised loop stages in LDS, same loop, same sums bit for bit -- without
                                 // the dequantisation that competes with the MFMAs for the issue port), 0 = from the quantised rows; unset = 1 iff the copies of every
                                 // block's matrices fit an eighth of the device's memory (Llama-3-8B: 14 of 288 GB, yes; 70B: 137 GB, no)
    bool pf_rope_pack = true;    // MC_PF_ROPE_PACK (prefill: the rope + cache launch with four rotation pairs per thread)
    bool pf_g8_on = true;        // MC_PF_GEMM8: prompts of pf_g8_rows rows and more take the 256 x 256 ping-pong GEMM (kernels/pf_gemm8.h)
    int pf_g8_max_splits = 16, pf_g8_min_ktiles = 8; // MC_PF_GEMM8_MAXSPLIT, MC_PF_GEMM8_MINKT: K ranges of a launch (g8_splits)
    int pf_g8_rows = 257;        // MC_PF_GEMM8_ROWS: from TWO row tiles on (round 5 measured 256 rows 7.42 ms with, 7.06 without -- one row of tiles leaves half the chip idle -- and 512 rows
                                 // 10.13 against 11.66, and set 384; round 6, on the dequantised copies: 256 rows 6.87 without against 7.65 with, 320 rows 11.2 against 8.95, 383: 11.3 against 9.2 --
                                 // profiles/r06_pf_rows_ab.log)
    bool pf_small_gemm = false;  // MC_PF_SMALL_GEMM set: the round-1 prompt GEMM for every matrix (A/B)
    bool pf_depth1 = false;      // MC_PF_DEPTH=1: the one-chunk build of the tiled prompt GEMM (A/B; two K chunks in flight measured best at every length)
    bool pf_bm128 = false;       // MC_PF_BM128 set: the 128-row prompt tile for every length
    bool pf_splits_old = false;  // MC_PF_SPLITS_OLD set: the plain doubling rule of gemm_splits
    bool pf_no_splitk = false;   // MC_PF_NO_SPLITK set: no prompt GEMM splits K
    bool pf_fold_on = true;      // MC_PF_FOLD: the split-K reduce of a prompt GEMM inside the kernel that consumes its rows
    bool pf_norm2 = true;        // MC_PF_NORM2=0: the split-K reduce and gemma3's two norms behind it as three launches
    bool pf_act_epi = true;      // MC_PF_ACT_EPI=0: the activation of a long prompt as a launch of its own
    bool pf_gelu_table = true;   // MC_PF_GELU_TABLE=0: no table of T(gelu) (mc_decoder::pf_gtab): the fp64 tanh per element
    bool pf_lib = false;         // MC_PF_BLASLT=1 (opt-in since round 5, a comparison aid): long prompts' large GEMMs in hipBLASLt on a dequantised bfloat16 copy of the matrix
                                 // (gemm_lib; mc_decoder::pf_lib_on is what holds now: any failure of the library switches the path off)
    bool pf_lib_force = false;   // MC_PF_BLASLT=2: every prompt GEMM that can, whatever its size
    bool pf_lib_tune = false;    // MC_PF_BLASLT_TUNE=1: the fastest of the heuristic's first eight algorithms, timed once per shape, instead of its first
                                 // (measured: inside the noise -- 512 rows 10.13 / 9.91 ms without, 10.04 / 10.00 with; 2048 rows 32.92 / 33.52, 32.55 / 32.92 --
                                 // and a timed choice would make the order of the fp32 additions differ from run to run: off)
    int pf_lib_rows = 160;       // MC_PF_BLASLT_ROWS: the shortest prompt chunk whose GEMMs may take the library (measured: 128 rows 5.01 ms without against
                                 // 5.38 with, 160 rows 6.83 / 5.96, 192: 6.91 / 6.33, 224: 7.08 / 6.44 -- profiles/r04_prefill_blaslt.log)
    int pf_lib_tiles = 48;       // MC_PF_BLASLT_TILES: the fewest 256 x 256 tiles of a launch the library takes (swept on whole prompts: profiles/r04_prefill_blaslt.log)
    bool pf_lib_verbose = false; // MC_PF_BLASLT_VERBOSE set: say on stderr why the library path switched itself off, and which algorithm a tuned shape took
    // MC_PF_TIMING=1: per-category GPU time of a prompt pass printed to stderr (tuning aid; it
    // synchronises after every launch)
    bool pf_timing = false;
    bool pf_two_pass = false;    // MC_PF_TWO_PASS=1: scores + pv kernels with the probability scratch (always for T = float)
};

// the three shapes a switch takes: on / off with a default, an integer clamped to [lo, hi], "is it set at all"
inline bool
env_set(const char* name) { return getenv(name) != nullptr; }
inline bool
env_flag(const char* name, bool dflt) { return env_set(name) ? atoi(getenv(name)) != 0 : dflt; }
inline int
env_int(const char* name, int dflt, int lo = INT_MIN, int hi = INT_MAX) { return env_set(name) ? std::max(lo, std::min(hi, atoi(getenv(name)))) : dflt; }

inline decoder_options
read_options()
{
    decoder_options o;
    o.gemv_block = env_int("MC_GEMV_BLOCK", o.gemv_block);
    o.gemv_wgs_per_cu = env_int("MC_GEMV_WGS_PER_CU", o.gemv_wgs_per_cu);
    o.gemv_block_env = env_set("MC_GEMV_BLOCK") || env_set("MC_GEMV_WGS_PER_CU");
    if (o.gemv_block % 64 || o.gemv_block < 64 || o.gemv_block > 1024) o.gemv_block = 256;
    if (o.gemv_wgs_per_cu < 1) o.gemv_wgs_per_cu = 2;
    o.gemv_lin = env_flag("MC_GEMV_LIN", o.gemv_lin);
    o.gemv_ling = env_flag("MC_GEMV_LING", o.gemv_ling);
    o.i8_ling14 = env_flag("MC_I8_LING14", o.i8_ling14);
    o.lin_split = env_flag("MC_LIN_SPLIT", o.lin_split);
    o.ling_half = env_flag("MC_LING_HALF", o.ling_half);
    o.lin_k4_on = env_flag("MC_LIN_K4", o.lin_k4_on);
    o.lin_waves = env_int("MC_LIN_WAVES", o.lin_waves, 1, 16);
    o.gemv_full_grid = env_flag("MC_GEMV_FULLGRID", o.gemv_full_grid);
    o.dbg_variant = env_int("MC_GEMV_DBG", o.dbg_variant);
    o.gemv_m4 = env_int("MC_GEMV_M4", o.gemv_m4);
    o.time_gemv_layers = env_int("MC_TIME_GEMV_LAYERS", 0, 0);

    o.attn_fused = env_flag("MC_ATTN_FUSED", o.attn_fused);
    o.attn_fused_max_wgs_per_cu = (unsigned)env_int("MC_ATTN_FUSED_WGS", (int)o.attn_fused_max_wgs_per_cu, 1, 4);
    o.attn_t2_on = env_flag("MC_ATTN_T2", o.attn_t2_on);
    o.rearm_after = env_int("MC_HANDOFF_REARM", o.rearm_after, 0);
    o.handoff_fast = env_flag("MC_HANDOFF_FAST", o.handoff_fast);
    o.attn_wo_on = env_flag("MC_ATTN_WO", o.attn_wo_on);
    o.attn_wo_k4 = env_set("MC_ATTN_WO_K4");
    o.attn_qkv_on = env_flag("MC_ATTN_QKV", o.attn_qkv_on);
    o.attn_qkv_only_on = env_flag("MC_ATTN_QKV_ONLY", o.attn_qkv_only_on);
    o.attn_i8_on = env_flag("MC_ATTN_I8", o.attn_i8_on);
    o.attn_i4_wide_on = env_flag("MC_ATTN_I4_WIDE", o.attn_i4_wide_on);
    o.kv_virtual_on = env_flag("MC_KV_VIRTUAL", o.kv_virtual_on);
    o.chain_w13_on = env_flag("MC_CHAIN_W13", o.chain_w13_on);
    o.chain_f = env_int("MC_CHAIN_F", o.chain_f, 0);
    o.attn_qkv_qkn_on = env_flag("MC_ATTN_QKV_QKN", o.attn_qkv_qkn_on);
    o.attn_wo_qkn_on = env_flag("MC_ATTN_WO_QKN", o.attn_wo_qkn_on);
    o.attn_qkn_on = env_flag("MC_ATTN_QKN", o.attn_qkn_on);
    o.gemma_fuse = !env_flag("MC_GEMMA_UNFUSED", !o.gemma_fuse);
    o.pv_fold_on = env_flag("MC_PV_FOLD", o.pv_fold_on);
    o.pv_block = env_int("MC_PV_BLOCK", o.pv_block);
    if (o.pv_block % 64 || o.pv_block < 256 || o.pv_block > 1024) o.pv_block = 1024;
    o.pv_ranges = env_int("MC_PV_RANGES", o.pv_ranges, 1, 64);

    o.head_pick_mode = env_int("MC_HEAD_PICK", o.head_pick_mode, 0, 2);
    o.head_pick_on = o.head_pick_mode != 0;
    o.lazy_pick_on = env_flag("MC_LAZY_PICK", o.lazy_pick_on);

    o.pf2_on = env_flag("MC_PF2", o.pf2_on);
    o.pf2_wgs_per_cu = env_int("MC_PF2_WGS_PER_CU", o.pf2_wgs_per_cu, 1);
    o.pf_attn8_on = env_flag("MC_PF_ATTN8", o.pf_attn8_on);
    o.pf_attn8_rows = env_int("MC_PF_ATTN8_ROWS", o.pf_attn8_rows, 1);
    o.pf_attn8_rows64 = env_int("MC_PF_ATTN8_ROWS64", o.pf_attn8_rows64, 1);
    o.pf_attn8_rows256 = env_int("MC_PF_ATTN8_ROWS256", o.pf_attn8_rows256, 1);
    o.pf_attn_heads = env_int("MC_PF_ATTN_HEADS", o.pf_attn_heads, 0);
    o.pf_attn8_pair = env_set("MC_PF_ATTN8_PAIR") ? (env_flag("MC_PF_ATTN8_PAIR", false) ? 1 : 0) : -1;
    o.pf_plain_mode = env_set("MC_PF_PLAIN_COPY") ? (env_flag("MC_PF_PLAIN_COPY", false) ? 1 : 0) : -1;
    o.pf_rope_pack = env_flag("MC_PF_ROPE_PACK", o.pf_rope_pack);
    o.pf_g8_on = env_flag("MC_PF_GEMM8", o.pf_g8_on);
    o.pf_g8_rows = env_int("MC_PF_GEMM8_ROWS", o.pf_g8_rows, 1);
    o.pf_g8_max_splits = env_int("MC_PF_GEMM8_MAXSPLIT", o.pf_g8_max_splits, 1);
    o.pf_g8_min_ktiles = env_int("MC_PF_GEMM8_MINKT", o.pf_g8_min_ktiles, 1);
    o.pf_small_gemm = env_set("MC_PF_SMALL_GEMM");
    o.pf_depth1 = env_int("MC_PF_DEPTH", 0) == 1;
    o.pf_bm128 = env_set("MC_PF_BM128");
    o.pf_splits_old = env_set("MC_PF_SPLITS_OLD");
    o.pf_no_splitk = env_set("MC_PF_NO_SPLITK");
    o.pf_fold_on = env_flag("MC_PF_FOLD", o.pf_fold_on);
    o.pf_norm2 = env_flag("MC_PF_NORM2", o.pf_norm2);
    o.pf_act_epi = env_flag("MC_PF_ACT_EPI", o.pf_act_epi);
    o.pf_gelu_table = env_flag("MC_PF_GELU_TABLE", o.pf_gelu_table);
    const int lib = env_int("MC_PF_BLASLT", 0);
    o.pf_lib = lib != 0;
    o.pf_lib_force = lib == 2;
    o.pf_lib_tune = env_flag("MC_PF_BLASLT_TUNE", o.pf_lib_tune);
    o.pf_lib_rows = env_int("MC_PF_BLASLT_ROWS", o.pf_lib_rows, 1);
    o.pf_lib_tiles = env_int("MC_PF_BLASLT_TILES", o.pf_lib_tiles, 1);
    o.pf_lib_verbose = env_set("MC_PF_BLASLT_VERBOSE");
    o.pf_timing = env_flag("MC_PF_TIMING", o.pf_timing);
    o.pf_two_pass = env_flag("MC_PF_TWO_PASS", o.pf_two_pass);
    return o;
}
