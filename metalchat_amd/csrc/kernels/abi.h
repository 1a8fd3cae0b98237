// The host/kernel ABI: every struct and constant that both the host library (../*.cc) and the kernels (*.hip) must agree on, each
// defined ONCE.  Kernels are looked up by name and their arguments are packed by hand (backend_impl.h pack()), so this header is
// the only thing the compiler can check that boundary with.  Plain C++17 and HIP alike: PODs and constants over <stdint.h>, no
// device code and no HIP types.  A layout that any code relies on by position is pinned by a static_assert below.
#pragma once

#include <stddef.h>
#include <stdint.h>

namespace mc {
namespace abi {

// ---- constants ----
constexpr int PB = 64;                         // cache slots per attention-scores workgroup (decode_kernels.hip)
constexpr int BATCH_MAX = 8;                   // rows of an mc_batch made by mc_batch_create
constexpr int MC_WIDE_BATCH_MAX = 64;          // rows of one made by mc_wide_batch_create: mc_b_rows_begin is ONE 64-thread workgroup, a
                                               // thread per row (up to 16 rows: the B columns of mc_b_gemv_*'s MFMA tile; more: mc_wb_gemv_*)
constexpr int BG_WAVES = 8;                    // mc_b_gemv_*: waves of a workgroup, each takes an equal slice of K
constexpr unsigned BG_THREADS = 64 * BG_WAVES; // ... its block size
constexpr unsigned BG_K_UNIT = 128 * BG_WAVES; // ... in_features per workgroup slice: a 128-weight chunk per wave
constexpr int PP_TILE_ROWS = 16;               // chunk rows of one attention tile of the packed prompt pass (pp_tile, px_range)
constexpr int MC_VERIFY_MAX_LEN = PP_TILE_ROWS; // tokens of one row's chunk in mc_verify_rows: one attention tile per row
constexpr int MC_VERIFY_MAX_ROWS = 128;        // packed rows of one verify call (mc_v_head_*: 8 column groups of 16)
constexpr int VH_TILES = 4;                    // 16-row weight tiles per workgroup of mc_v_head_* (verify_kernels.hip)
constexpr uint32_t SAMPLE_CAP = 4096;          // keys the sampler's dynamic LDS holds (sampler_params::cap)
constexpr uint32_t MC_SAMPLE_LISTS_MAX = 1024; // sorted candidate lists the sampler's second launch takes

// ---- the step state (handoff.h: the tag of in-launch hand-offs; decode_kernels.hip mc_step_set / mc_step_next) ----
struct step_state {
    int32_t token;      // input token of the current step
    int32_t pos;        // start_pos of the current step
    int32_t kv_len;     // valid cache slots after this step's write  = min(pos + 1, max_seq)
    int32_t write_slot; // physical slot of this step's K/V row
    int32_t ring_base;  // rotation of the post-sink ring
    int32_t step_index; // index into tokens_out for chained generation
    int32_t rope_row;   // pos - rope_table_start
    int32_t rolled;     // number of rolls so far (debug)
    int32_t rope_start; // first position of the rope table window (nn/embedding.h:190-198); moved by mc_step_rope
    uint32_t epoch;     // counts the steps since the decoder was created (never reset): the tag of in-launch hand-offs
    uint32_t err;       // set by a kernel whose in-launch hand-off gave up (mc_attn_fused_T); 0 = none
    int32_t pad[1];
};
static_assert(sizeof(step_state) == 48 && alignof(step_state) == 4, "step_state: 12 words (arrays of it: one per batch row)");
static_assert(offsetof(step_state, token) == 0 && offsetof(step_state, pos) == 4 && offsetof(step_state, kv_len) == 8 &&
                  offsetof(step_state, write_slot) == 12 && offsetof(step_state, ring_base) == 16 &&
                  offsetof(step_state, step_index) == 20 && offsetof(step_state, rope_row) == 24 && offsetof(step_state, rolled) == 28 &&
                  offsetof(step_state, rope_start) == 32 && offsetof(step_state, epoch) == 36 && offsetof(step_state, err) == 40,
              "step_state: tests and traces read its words by index");

// ---- the default sampler (sampler_kernels.hip), passed BY VALUE: its size and alignment place the arguments behind it ----
struct sampler_params {
    uint32_t k;          // top-k (<= 128)
    uint32_t ncand;      // candidate keys written by launch 1 = nlists * kpad
    uint32_t cap;        // keys the dynamic LDS holds (a power of two >= 2 * kpad)
    float inv_temp;      // T(1 / T(temperature))
    float top_p;         // T(p)
    uint32_t nlists;     // sorted candidate lists (workgroups of launch 1), <= MC_SAMPLE_LISTS_MAX
    uint32_t kpad;       // keys per list
};
static_assert(sizeof(sampler_params) == 28 && alignof(sampler_params) == 4, "sampler_params is a by-value kernel argument");

// ---- a batch row's own sampler (batch_kernels.hip mc_b_*_mixed_*; ABI Part 2k), one per row in a [B] device table ----
// the EFFECTIVE settings, resolved on the host: a row that inherits carries the decoder's
constexpr int32_t ROW_SAMPLER_GREEDY = 0;  // (= MC_SAMPLER_GREEDY) the first index of the maximum; the other words are not read
constexpr int32_t ROW_SAMPLER_DEFAULT = 1; // (= MC_SAMPLER_DEFAULT) make_default_sampler with the three words below
constexpr int32_t ROW_SAMPLER_DRAW = 2;    // (= MC_SAMPLER_DRAW) the same chain, the last phase draws with the row's seed pair
struct row_sampler {
    int32_t kind;   // ROW_SAMPLER_*
    uint32_t k;     // sampler_params::k
    float inv_temp; // sampler_params::inv_temp
    float top_p;    // sampler_params::top_p
};
static_assert(sizeof(row_sampler) == 16 && alignof(row_sampler) == 4 && offsetof(row_sampler, kind) == 0 && offsetof(row_sampler, k) == 4 &&
                  offsetof(row_sampler, inv_temp) == 8 && offsetof(row_sampler, top_p) == 12,
              "row_sampler: four words (read whole with one scalar load)");

// ---- a batch row's logit processor (logit_kernels.hip mc_b_logits_process_*; ABI Part 2l), one per row in a [B] device table ----
// resolved on the host: flags 0 = nothing set, the row's workgroups exit.  The row's mask words and counts are found from the row
// index: masks + r * ((vocab + 31) / 32), counts + r * vocab
constexpr uint32_t ROW_LOGITS_MASK = 1u;    // the row has a token mask: a cleared bit makes the logit -inf
constexpr uint32_t ROW_LOGITS_PENALTY = 2u; // the row's penalties are not (1, 0, 0): its counts are read, and its input token counted
constexpr uint32_t LP_THREADS = 256;        // mc_b_logits_process_*: threads of a workgroup ...
constexpr uint32_t LP_CHUNK = 8 * LP_THREADS; // ... and the logits of one row it streams: one 16-byte piece per thread
struct alignas(16) row_logits {
    uint32_t flags; // ROW_LOGITS_*
    float rep;      // the repetition penalty ...
    float inv_rep;  // ... and float(1.0f / rep), formed on the host: no division on the device
    float freq;     // the frequency penalty
    float pres;     // the presence penalty
    uint32_t pad[3];
};
static_assert(sizeof(row_logits) == 32 && alignof(row_logits) == 16 && offsetof(row_logits, flags) == 0 && offsetof(row_logits, rep) == 4 &&
                  offsetof(row_logits, inv_rep) == 8 && offsetof(row_logits, freq) == 12 && offsetof(row_logits, pres) == 16,
              "row_logits: eight words (read whole with one scalar load)");

// ---- row log-probabilities (logprob_kernels.hip mc_logprob_parts_* / mc_logprob_finish_*; ABI Part 2n) ----
// launch 1 writes one part per (row, chunk of LOGPROB_CHUNK logits) and the chunk's top_n best keys, launch 2 folds a row's parts
constexpr int LOGPROBS_MAX_TOP = 20;                // (= MC_LOGPROBS_MAX_TOP) the most top_n: the largest `top_logprobs` any public API takes
constexpr uint32_t LOGPROB_THREADS = 256;           // threads of a workgroup of either launch ...
constexpr uint32_t LOGPROB_CHUNK = 8 * LOGPROB_THREADS; // ... and the logits of one row a parts workgroup streams: one 16-byte piece per thread
constexpr uint32_t LOGPROB_FINISH_KEYS = 8;         // chunk keys a thread of the finish launch holds in registers
constexpr uint32_t LOGPROB_KEY_CAP = LOGPROB_FINISH_KEYS * LOGPROB_THREADS; // nchunk * top_n it can fold; nchunk <= LOGPROB_THREADS as well
struct alignas(16) logprob_part {
    double s;  // sum over the chunk of exp(double(y) - double(m)), 0 where m is -inf
    float m;   // the chunk's maximum (a bfloat16 value)
    uint32_t pad;
};
static_assert(sizeof(logprob_part) == 16 && alignof(logprob_part) == 16 && offsetof(logprob_part, s) == 0 && offsetof(logprob_part, m) == 8,
              "logprob_part: one 16-byte store and load");
static_assert(LOGPROB_CHUNK == 2048 && LOGPROB_CHUNK == LP_CHUNK, "the parts launch has the shape of mc_b_logits_process_*");
static_assert(LOGPROBS_MAX_TOP * ((128256 + LOGPROB_CHUNK - 1) / LOGPROB_CHUNK) <= LOGPROB_KEY_CAP, "Llama-3's vocabulary fits the finish launch at top_n = 20");

// ---- the descriptors a decode GEMV finds behind its `res` argument (gemv.h) ----
// PRO_POSTNORM
struct postnorm_args {
    const void* post_w; // T[in]
    const void* res;    // T[in]
    void* h_out;        // T[in]
};
static_assert(sizeof(postnorm_args) == 24, "postnorm_args: three pointers");
// EPI_STORE_PICK
struct pick_epilogue {
    unsigned long long* key; // 0 between launches
    uint32_t* ticket;        // 0 between launches; NULL: `key` has one slot per workgroup and a one-workgroup launch folds them
    step_state* state;       // the pick becomes its token, and tokens_out[its step_index]
    int32_t* tokens_out;     // may be null
};
static_assert(sizeof(pick_epilogue) == 32 && offsetof(pick_epilogue, key) == 0 && offsetof(pick_epilogue, ticket) == 8 &&
                  offsetof(pick_epilogue, state) == 16 && offsetof(pick_epilogue, tokens_out) == 24,
              "pick_epilogue: four pointers");
// EPI_QKV_ROPE
struct qkv_epilogue {
    void* q_out;        // T[H*hd]       rotated queries, natural order
    void* kc;           // T[KV][max_seq][hd]
    void* vt;           // T[KV][hd][max_seq]
    const float* fcos;  // [rows][hd/2]
    const float* fsin;
    const step_state* state; // its write_slot and rope_row
    uint32_t H, KV, hd, max_seq;
};
static_assert(sizeof(qkv_epilogue) == 64 && offsetof(qkv_epilogue, state) == 40 && offsetof(qkv_epilogue, H) == 48,
              "qkv_epilogue: six pointers and four words (read whole with scalar loads)");

// ---- the tables of the packed prompt pass (packed_kernels.hip, extend_kernels.hip) ----
// one per row in the call, in packed order: batch row, position of its chunk, offset of its first packed row, length
struct pp_seg {
    int32_t row, pos, off, len;
};
static_assert(sizeof(pp_seg) == 16, "pp_seg: four words");
// one 16-row attention tile: its segment, and its first row inside the segment
struct alignas(8) pp_tile {
    int32_t seg, r0;
};
static_assert(sizeof(pp_tile) == 8 && alignof(pp_tile) == 8 && offsetof(pp_tile, r0) == 4, "pp_tile: one 8-byte load");
// one per (tile, key range) of mc_extend_rows
struct px_range {
    int32_t seg, r0;    // segment, first chunk row of the 16-row tile inside it
    int32_t k_lo, k_hi; // keys [k_lo, k_hi) of the row's cache; k_lo a multiple of 128
    int32_t first, n;   // the tile's ranges: indices [first, first + n) of this table
    int32_t pad0, pad1;
};
static_assert(sizeof(px_range) == 32 && offsetof(px_range, k_lo) == 8 && offsetof(px_range, first) == 16, "px_range: eight words");
// one per packed row of mc_tree_verify (tree_kernels.hip): node i of its segment's draft tree
struct alignas(8) tv_node {
    int32_t depth; // edges from the root (node 0): the node sits at position pos + depth
    uint32_t anc;  // bit j: node j of the segment is an ancestor of this node, or the node itself
};
static_assert(sizeof(tv_node) == 8 && alignof(tv_node) == 8 && offsetof(tv_node, depth) == 0 && offsetof(tv_node, anc) == 4,
              "tv_node: two words, one 8-byte load");
static_assert(MC_VERIFY_MAX_LEN <= 32, "tv_node::anc holds one bit per node of a chunk");
// one per packed row of a verify call whose rows carry settings (verify_kernels.hip mc_vs_*, logit_kernels.hip mc_vs_logits_process_bfloat;
// ABI Part 2m), resolved on the host: chunk row j (tree: node j at depth d) of the segment of batch row `row`
struct alignas(16) verify_row {
    row_sampler sampler; // the batch row's EFFECTIVE sampler
    uint32_t seed;       // its seed pair: (j * B + row) % n_pairs, a tree (d * B + row) % n_pairs -- token j of the row in mc_ragged_generate; 0 without pairs
    uint32_t anc;        // bit i: chunk token i of the segment was fed up to and including this row -- a chain (2 << j) - 1, a tree tv_node::anc
    int32_t row;         // the batch row: its processor is table[row], its mask words and counts lie where the step's launch finds them
    int32_t off;         // the segment's first packed row: chunk token i is tokens[off + i]
};
static_assert(sizeof(verify_row) == 32 && alignof(verify_row) == 16 && offsetof(verify_row, sampler) == 0 && offsetof(verify_row, seed) == 16 &&
                  offsetof(verify_row, anc) == 20 && offsetof(verify_row, row) == 24 && offsetof(verify_row, off) == 28,
              "verify_row: eight words (read whole with one scalar load)");

} // namespace abi
} // namespace mc
