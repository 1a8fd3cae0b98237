/*
 * metalchat_hip.h -- C ABI of the MI355X (gfx950) backend for metalchat's decode hot path.
 *
 * This is the drop-in boundary: plain C, opaque handles, pointers and sizes only.  It exports
 * exactly what the reference's Metal seam binds for this path, one entry point per Metal call
 * site, plus the fused decode pipeline that sits behind the same handles.  Reference citations
 * are paths relative to the metalchat source tree (v1.2.1).
 *
 * Part 1 mirrors  metal::{device,library,kernel,buffer}   include/metalchat/metal.h:14-34
 *                 src/metal.cc:21-84, src/metal_impl.h:19-120
 *                 hardware_function_encoder / kernel_thread  include/metalchat/kernel_thread.h:57-294
 *                 src/kernel_thread.cc:13-223
 * Part 2 is the decode pipeline driven by nn::llama3 / nn::gemma3 / transformer<Layer>::transform
 *                 include/metalchat/nn/llama.h:113-134, nn/gemma.h:110-137, transformer.h:357-364
 *
 * Error convention: every function that can fail returns an mc_status (0 = ok).  The message of
 * the last failure on the calling thread is mc_last_error().  The C++ shim rethrows
 * MC_ERR_INVALID_ARGUMENT as std::invalid_argument, MC_ERR_RUNTIME as std::runtime_error and
 * MC_ERR_ALLOC as alloc_error with the same message text the reference uses
 * (include/metalchat/tensor/expected.h:185-193, include/metalchat/allocator.h:20-34).
 *
 * There is NO CPU fallback anywhere behind this ABI: without a HIP device every entry point that
 * needs one fails with MC_ERR_RUNTIME.
 */
#ifndef METALCHAT_HIP_H
#define METALCHAT_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef int32_t mc_status;
enum {
    MC_OK = 0,
    MC_ERR_INVALID_ARGUMENT = 1, /* std::invalid_argument */
    MC_ERR_RUNTIME = 2,          /* std::runtime_error    */
    MC_ERR_ALLOC = 3             /* alloc_error           */
};

const char* mc_last_error(void);
/* "metalchat-hip <version> gfx950" */
const char* mc_version(void);
/* 1 when every kernel launch is wrapped in a named range "name<grid,group>" (roctxRangePush / Pop; MC_TRACE_RANGES=1 and
 * libroctx64 found) -- the reference labels every encoder that way for GPU capture, src/kernel_thread.cc:109-115 */
int32_t mc_trace_ranges_enabled(void);

/* ------------------------------------------------------------------------------------------
 * Part 1 -- backend seam
 * ------------------------------------------------------------------------------------------ */
typedef struct mc_device mc_device;
typedef struct mc_library mc_library;
typedef struct mc_kernel mc_kernel;
typedef struct mc_buffer mc_buffer;
typedef struct mc_queue mc_queue;

/* MTL::CreateSystemDefaultDevice -- src/metal.cc:51-55.  ordinal < 0 selects the current HIP
 * device (LOCAL_RANK-aware callers pass their own ordinal). */
mc_status mc_device_create(int32_t ordinal, mc_device** out);
void mc_device_release(mc_device* dev);
/* HIP devices visible to this process (the reference has exactly one: MTL::CreateSystemDefaultDevice, src/metal.cc:51-55);
 * the layer pipeline puts one stage on each. */
int32_t mc_device_count(void);
/* device->name() -- src/accelerator.cc:108-113 */
const char* mc_device_name(const mc_device* dev);
/* device->maxBufferLength() -- src/accelerator.cc:73-77 */
size_t mc_device_max_buffer_size(const mc_device* dev);
int32_t mc_device_ordinal(const mc_device* dev);
int32_t mc_device_compute_units(const mc_device* dev);

/* device->newLibrary(url) -- src/metal.cc:58-84.  `path` is a gfx950 code object (.hsaco).
 * Failure message is "metal: library not found"-style: "hip: library not found" when the file
 * is absent (test/test_accelerator.cc:15-21 expects the runtime_error). */
mc_status mc_library_open(mc_device* dev, const char* path, mc_library** out);
void mc_library_release(mc_library* lib);

/* library->newFunction(name) + newComputePipelineState -- src/accelerator.cc:116-158.
 * Name format {kernel}[_{block}]_{type}[_{type}...] with types bfloat,float,int32_t,int8_t
 * (include/metalchat/accelerator.h:175-218, include/metalchat/dtype.h:83-118).
 * Missing function -> MC_ERR_INVALID_ARGUMENT "hardware_accelerator: function <name> not found
 * in a shader library". */
mc_status mc_library_get_kernel(mc_library* lib, const char* name, mc_kernel** out);
void mc_kernel_release(mc_kernel* k);
const char* mc_kernel_name(const mc_kernel* k);
/* pipeline->maxTotalThreadsPerThreadgroup() -- src/kernel.cc:75-79 */
size_t mc_kernel_max_threads_per_group(const mc_kernel* k);

/* device->newBuffer(bytes, Shared) / newBuffer(ptr, bytes, Shared) / newBuffer(ptr, bytes,
 * Shared, nil) (no-copy) -- src/allocator.cc:127-173.  HBM-resident (hipMalloc); the no-copy
 * form wraps an existing DEVICE pointer (for example torch-owned memory) without owning it. */
mc_status mc_buffer_alloc(mc_device* dev, size_t bytes, mc_buffer** out);
mc_status mc_buffer_alloc_copy(mc_device* dev, const void* host_src, size_t bytes, mc_buffer** out);
mc_status mc_buffer_wrap_nocopy(mc_device* dev, void* device_ptr, size_t bytes, mc_buffer** out);
void mc_buffer_release(mc_buffer* buf);
/* buffer->contents() / buffer->length() -- src/metal.cc:21-32.  contents() is a DEVICE address:
 * weights live in HBM, so the reference's "CPU dereferences the shared buffer" idiom becomes the
 * explicit copies below ("Unified memory assumption"). */
void* mc_buffer_contents(const mc_buffer* buf);
size_t mc_buffer_length(const mc_buffer* buf);
mc_status mc_buffer_upload(mc_buffer* buf, size_t offset, const void* host_src, size_t bytes);
mc_status mc_buffer_download(const mc_buffer* buf, size_t offset, void* host_dst, size_t bytes);
mc_status mc_buffer_fill_zero(mc_buffer* buf, size_t offset, size_t bytes);

/* device->newCommandQueue() + commandBuffer + computeCommandEncoder -- src/kernel_thread.cc:23-32.
 * One in-order HIP stream subsumes the MTL::Event chain of src/kernel_thread.cc:34-47,194 and
 * the per-argument memoryBarrier of include/metalchat/kernel_thread.h:121-124.
 * external_stream != NULL adopts a caller-owned hipStream_t (for example torch's current stream). */
mc_status mc_queue_create(mc_device* dev, void* external_stream, mc_queue** out);
void mc_queue_release(mc_queue* q);
void* mc_queue_stream(const mc_queue* q);

/* encoder->setComputePipelineState -- src/kernel_thread.cc:69-74.  Resets the argument index. */
mc_status mc_encoder_set_kernel(mc_queue* q, mc_kernel* k);
/* encoder->setBytes(data, size, index++) -- src/kernel_thread.cc:77-81.  The argument is placed at
 * the next offset aligned to min(size, 4) rounded down to a power of two (tensor_layout<N> and
 * 32-bit scalars: 4; a bfloat scalar: 2). */
mc_status mc_encoder_set_bytes(mc_queue* q, const void* data, size_t size);
/* encoder->setBuffer(buffer, offset, index++) -- src/kernel_thread.cc:84-88.  offset in BYTES. */
mc_status mc_encoder_set_buffer(mc_queue* q, mc_buffer* buf, size_t byte_offset);
/* encoder->memoryBarrier(resource) -- src/kernel_thread.cc:91-96.  A no-op on an in-order stream;
 * kept so the reference's encode() sequence maps 1:1. */
mc_status mc_encoder_memory_barrier(mc_queue* q, mc_buffer* buf);
/* encoder->dispatchThreads(grid, group) -- src/kernel_thread.cc:105-120.  grid = TOTAL threads,
 * group = threads per group; blocks = ceil(grid/group) per axis and kernels bounds-check, which is
 * how Metal's non-uniform threadgroups behave.  Validation as include/metalchat/kernel.h:119-141:
 * group.numel() <= max_threads and grid.numel() >= group.numel() else MC_ERR_INVALID_ARGUMENT. */
mc_status mc_encoder_dispatch_threads(mc_queue* q, const size_t grid[3], const size_t group[3]);
/* Same, with an explicit dynamic LDS size (fused kernels only). */
mc_status mc_encoder_dispatch_threads_lds(mc_queue* q, const size_t grid[3], const size_t group[3],
                                          size_t lds_bytes);
/* commandBuffer->addCompletedHandler -- src/kernel_thread.cc:134-144.  The callback runs on a
 * driver thread once everything submitted before it has completed; status != MC_OK carries a GPU
 * execution error (the reference delivers it through the promise). */
typedef void (*mc_completion_fn)(void* ctx, mc_status status);
mc_status mc_queue_on_completed(mc_queue* q, mc_completion_fn fn, void* ctx);
/* commandBuffer->commit() -- src/kernel_thread.cc:184-199.  Launches are asynchronous already;
 * commit only flushes.  mc_queue_wait is future_tensor::wait (include/metalchat/tensor/future.h:235-253). */
mc_status mc_queue_commit(mc_queue* q);
mc_status mc_queue_wait(mc_queue* q);

/* Timing of a region of the queue with HIP events recorded ON THE QUEUE'S STREAM (bench.py).
 * begin/end record the events, elapsed synchronises on the end event. */
mc_status mc_queue_timer_begin(mc_queue* q);
mc_status mc_queue_timer_end(mc_queue* q);
mc_status mc_queue_timer_elapsed_ms(mc_queue* q, float* ms);

/* ------------------------------------------------------------------------------------------
 * Part 2 -- fused decode pipeline (what nn::llama3::operator() does per token, behind the seam)
 * ------------------------------------------------------------------------------------------ */
enum { MC_DTYPE_BF16 = 0, MC_DTYPE_F32 = 1 };
enum { MC_FAMILY_LLAMA3 = 0, MC_FAMILY_GEMMA3 = 1 };
/* weight formats of a linear layer held in HBM */
enum {
    MC_WFMT_T = 0,   /* nn::linear: row-major [out,in] of T                                    */
    MC_WFMT_I8 = 1,  /* int8 [out,in] + per-(row,group) scale  (quantization::lora_linear)      */
    MC_WFMT_I4 = 2   /* packed int4 (two values per byte, offset-binary) + per-(row,group) scale */
};
/* quantised-GEMV arithmetic */
enum {
    MC_QMODE_EXACT = 0, /* Wd = T(T(q)*T(s)) materialised per weight exactly as
                           hadamard_broadcast does (kernel/mul.metal:78-82), then fp32 dot        */
    MC_QMODE_FAST = 1   /* y = sum_g s_g * sum_k q_k x_k : skips the per-weight rounding to T     */
};

typedef struct {
    int32_t dtype;   /* activation / KV / norm-weight type T */
    int32_t family;
    int32_t dim, n_heads, n_kv_heads, head_dim, ffn_dim, n_layers, vocab, max_seq_len;
    float rope_theta;
    float rope_sliding_theta; /* gemma3: theta of the sliding layers, 0 otherwise */
    int32_t sliding_stride;   /* gemma3: layer i is sliding iff (i+1) % stride != 0 */
    float norm_eps;
    float attn_scale;
    int32_t sink_pre_len;     /* < 0: bit_width(max_seq_len) - 1 (include/metalchat/nn/cache.h:125-127) */
    /* pipeline partition: this decoder owns layers [layer_begin, layer_end); the first stage
     * owns the embedding, the last stage owns final norm + output head. */
    int32_t layer_begin, layer_end;
    int32_t weight_format;    /* MC_WFMT_* of the seven per-layer linears and the output head */
    int32_t group_size;       /* quantisation group along `in` (per-row scale: group_size = 0)   */
    int32_t qmode;            /* MC_QMODE_* */
    int32_t use_graph;        /* capture one token step into a hipGraph and replay it */
} mc_decoder_config;

typedef struct mc_decoder mc_decoder;

mc_status mc_decoder_create(mc_device* dev, mc_library* lib, mc_queue* q,
                            const mc_decoder_config* cfg, mc_decoder** out);
void mc_decoder_release(mc_decoder* d);

/* Names of the per-layer tensors: "wq","wk","wv","wo","w1","w2","w3" (linears),
 * "attention_norm","ffn_norm","q_norm","k_norm","attention_post_norm","ffn_post_norm" (T[n]).
 * layer = -1 addresses the model-level tensors "tok_embeddings", "output" (linears) and "norm".
 *
 * mc_decoder_load_linear takes the REFERENCE-NATIVE host format and repacks it for HBM:
 *   MC_WFMT_T : weight = T[out*in]
 *   MC_WFMT_I8/I4 : weight = int8_t[out*in] (int4 range [-8,7] held one value per byte, as the
 *                   reference loads it: include/metalchat/huggingface/llama.h:159-168),
 *                   scales = float[out * in/group] (group 0: float[out])
 * For "tok_embeddings" a quantised table is always kept as int8 + per-row scale
 * (quantization::lora_embedding, include/metalchat/quantization/lora.h:133-175). */
mc_status mc_decoder_load_linear(mc_decoder* d, int32_t layer, const char* name,
                                 int32_t weight_format, int32_t out_features, int32_t in_features,
                                 int32_t group_size, const void* weight, const float* scales);
/* quantization::lora_adaptor of one projection (include/metalchat/quantization/lora.h:17-53,
 * 119-121): result = T(T(x Wd^T) + T(T(B(A x)) * scale)).  name as in mc_decoder_load_linear
 * ("wq","wk","wv","wo","w1","w3","w2"); a_T = T[rank * in_features], b_T = T[out_features * rank]
 * (nn::linear weights, row-major [out, in]).  Adaptors of projections that share a fused GEMV
 * (wq|wk|wv, w1|w3) must share rank and scale; rank is a multiple of 8. */
mc_status mc_decoder_load_lora(mc_decoder* d, int32_t layer, const char* name, int32_t rank,
                               int32_t out_features, int32_t in_features, const void* a_T,
                               const void* b_T, float scale);
mc_status mc_decoder_load_vector(mc_decoder* d, int32_t layer, const char* name, int32_t n,
                                 const void* data_T);
/* Synthetic weights generated ON THE DEVICE from a counter-based hash (bench.py at full model
 * sizes; tests regenerate any row on the host with mc_synth_* below and check it). */
mc_status mc_decoder_init_synthetic(mc_decoder* d, uint64_t seed);

/* transformer<Layer>::transform(token, start_pos) with len == 1 -- include/metalchat/transformer.h:357-364.
 * Runs the layers this decoder owns.  First stage: `token` is embedded.  Other stages: the hidden
 * row is read from hidden_in (device pointer, T[dim]).  Last stage: writes the greedy next token
 * to *next_token (after a stream sync) when next_token != NULL.  Non-last stages leave the hidden
 * row in the buffer returned by mc_decoder_hidden_out(). */
mc_status mc_decoder_step(mc_decoder* d, int32_t token, int32_t start_pos, const void* hidden_in,
                          int32_t* next_token);
/* The prompt pass: transformer<Layer>::transform(input[1, len], start_pos) with len > 1 --
 * nn::llama3 / nn::gemma3 operator() (include/metalchat/nn/llama.h:113-134, nn/gemma.h:110-137).
 * All len rows go through the layers as GEMMs (weights dequantised once per tile), the K / V rows
 * are written to cache positions [start_pos, start_pos + len), scores take the reference's mask
 * (make_causal_mask / make_sliding_causal_mask, nn/attention.h:283-321: only the LAST len columns
 * form the causal square, columns of an earlier context stay masked -- as the reference builds it),
 * and the last row goes through the head and the sampler; *next_token receives its pick.
 * sliding_window: gemma3_options.sliding_window (sliding layers only); 0 for llama3.
 * len == 1 is mc_decoder_step.  The cache follows nn::sink_cache::copy (nn/cache.h:167-216): a chunk either fits
 * behind start_pos (start_pos + len <= max_seq_len), or, once start_pos >= max_seq_len, the post-sink region is
 * rotated left by len and the chunk takes the last len rows (len <= max_seq_len, "sink_cache: requested length ... is
 * larger than the cache size" otherwise).  A chunk that starts inside the cache and ends outside is an error, as it
 * is in the reference (its cache slice runs out of range).
 * Long prompts: a GEMM launch with >= 48 tiles of 256 x 256 (MC_PF_BLASLT_TILES) multiplies a dequantised bfloat16 copy of the
 * matrix -- Wd = T(T(q) T(s)), kernel/mul.metal:78-82, 2 bytes per weight more device memory, built on first use -- in the ROCm
 * library GEMM (libhipblaslt, opened with dlopen on first use; MC_PF_BLASLT=0 or an absent library: the prompt kernels alone).
 * Same operand values, fp32 sums rounded to T once (nn/linear.h:70-81); the first such prompt of a process also pays the library's start-up.
 * mc_decoder_prefill_stage is the same pass on ONE STAGE of a layer pipeline: the first stage takes `tokens`, a later
 * stage the [len][dim] hidden rows of the previous one (`rows_in`, device memory); *rows_out (device memory, valid
 * until the next prompt pass) receives this stage's rows; the last stage runs the head and fills *next_token. */
mc_status mc_decoder_prefill(mc_decoder* d, const int32_t* tokens, int32_t len, int32_t start_pos,
                             int32_t sliding_window, int32_t* next_token);
mc_status mc_decoder_prefill_stage(mc_decoder* d, const int32_t* tokens, const void* rows_in, int32_t len,
                                   int32_t start_pos, int32_t sliding_window, void** rows_out, int32_t* next_token);
/* Enqueue `n` chained greedy steps entirely on the device (token feedback through HBM, one host
 * sync at the end); tokens_out receives the n generated ids.  Single-stage decoders only. */
mc_status mc_decoder_generate(mc_decoder* d, int32_t first_token, int32_t start_pos, int32_t n,
                              int32_t* tokens_out);
void* mc_decoder_hidden_out(mc_decoder* d);
void* mc_decoder_hidden_in(mc_decoder* d);

/* Layer pipeline over N stages: stage r owns a contiguous range of L / N layers (the first L % N
 * stages one more: mc_pipeline_layer_range) of the strict layer
 * chain include/metalchat/nn/llama.h:123-126 and their caches (nn/attention.h:122-130); per token the hidden row
 * hops stage to stage and the 4-byte pick returns to stage 0.  Everything, hops included, is enqueued on the
 * stages' streams: one host synchronisation per mc_pipeline_generate call.
 *   mc_pipeline_unique_id / _create : one process per GPU; the hop is ONE ncclSend / ncclRecv pair (RCCL over
 *       xGMI) on the decoder's own stream.  Rank 0 makes the 128-byte id, every rank passes the same bytes.
 *   mc_pipeline_create_local        : all N stages in this process (on one device or several): the hop is a
 *       device-to-device copy behind an event -- the same launches per stage, runnable on a one-GPU box.
 *   mc_pipeline_generate            : called by EVERY rank with the same arguments; tokens_out is filled on
 *       rank 0 and on the last rank (local: always).  Greedy or the last stage's sampler.
 *   mc_pipeline_allreduce_max       : barrier + device synchronise, then *value = max over ranks. */
typedef struct mc_pipeline mc_pipeline;
void mc_pipeline_layer_range(int32_t rank, int32_t world, int32_t n_layers, int32_t* layer_begin, int32_t* layer_end);
mc_status mc_pipeline_unique_id(void* id_128_bytes);
mc_status mc_pipeline_create(mc_decoder* stage, int32_t rank, int32_t world, const void* id_128_bytes, mc_pipeline** out);
mc_status mc_pipeline_create_local(mc_decoder** stages, int32_t n, mc_pipeline** out);
mc_status mc_pipeline_generate(mc_pipeline* p, int32_t first_token, int32_t start_pos, int32_t n, int32_t* tokens_out);
mc_status mc_pipeline_prefill(mc_pipeline* p, const int32_t* tokens, int32_t len, int32_t start_pos, int32_t sliding_window,
                              int32_t* next_token); /* the prompt pass: [len][dim] rows hop stage to stage */
mc_status mc_pipeline_allreduce_max(mc_pipeline* p, double* value);
/* What the transport itself reports: the communicator's size and this process's rank in it (ncclCommCount /
 * ncclCommUserRank), so a caller can verify that RCCL saw N ranks; (-1, -1) for a local pipeline. */
mc_status mc_pipeline_comm_info(mc_pipeline* p, int32_t* ranks, int32_t* rank);
void mc_pipeline_release(mc_pipeline* p);
/* Sampler of the last stage -- include/metalchat/nn/sampling.h:152-315.
 *   MC_SAMPLER_GREEDY : argmax, first maximum (the BASELINE configuration).
 *   MC_SAMPLER_DEFAULT: make_default_sampler() = topk_sampler(top_k) -> nucleus_sampler(temperature,
 *                       top_p) -> multinomial_sampler(1), run on the device in two launches with no
 *                       host synchronisation (the reference synchronises three times per token and
 *                       partial_sorts the vocabulary on the CPU).  Errors as nucleus_sampler's
 *                       constructor ("temperature must be positive", "probability must be in
 *                       [0.0, 1.0]").  top_k <= 128.  Equal logits are ordered by index
 *                       (std::partial_sort leaves them unspecified).  The reference's multinomial reads
 *                       the lower end of its draw interval at column sample_size - 1 = 0, so the
 *                       interval is empty and the pick is the head of the sorted nucleus WHATEVER the
 *                       seeds are; reproduced bit for bit.
 *   MC_SAMPLER_DRAW   : the sampler whose pick depends on its seeds (opt-in; ours, not the reference's).
 *                       MC_SAMPLER_DEFAULT's chain unchanged up to the nucleus cut -- the seven taps are
 *                       the same bits -- with its checks, texts, rounding and top_k <= 128; only the
 *                       last phase differs.  In float32, not rounded to T, one operation per step, with
 *                       m[j] = masked[j] (tap 5; sorted order, the zeros are a suffix), j = 0 .. k-1:
 *                         total = ((0 + m[0]) + m[1]) + .. + m[k-1]     sequential, ascending j
 *                         u     = the first uniform() of pcg32(seed0, seed1)
 *                         t     = u * total
 *                         c_j   = c_{j-1} + m[j] (c_{-1} = 0);  pos = the smallest j with c_j > t
 *                         none (t rounded up to total; total is 0 or NaN): pos = the largest j with
 *                               m[j] > 0, else 0
 *                         token = ids[sidx[pos]]
 *                       So: a masked entry is never picked (c does not grow there); k = 1 or top_p = 0
 *                       gives position 0, MC_SAMPLER_DEFAULT's pick; P(pos = j) = m[j] / total to within
 *                       the generator's 2^-23 step; there is no division on the device.
 *                       NOTHING IS KEPT BETWEEN CALLS: a caller who uploads no pairs, or reuses the same
 *                       pairs, gets the same u again.  A loop that samples uploads fresh pairs from the
 *                       host's generator in front of each call -- n for n tokens of a decoder call,
 *                       n * B for a batch call -- as the reference draws a new pair from its
 *                       std::mt19937 for every call.
 * mc_decoder_set_seeds: the (init_state, init_seq) pairs kernel::multinomial draws from its
 * std::mt19937 per call (include/metalchat/kernel/multinomial.h:46-55); token i of one
 * mc_decoder_generate call uses pair i % n_pairs (mc_decoder_step: pair 0); no pairs = (0, 0). */
enum { MC_SAMPLER_GREEDY = 0, MC_SAMPLER_DEFAULT = 1, MC_SAMPLER_DRAW = 2 };
mc_status mc_decoder_set_sampler(mc_decoder* d, int32_t kind, int32_t top_k, float temperature, float top_p);
mc_status mc_decoder_set_seeds(mc_decoder* d, const uint64_t* seeds, int32_t n_pairs);
/* After a step with taps enabled: [7][k] floats -- scaled logits, probabilities, sorted, cumsum,
 * cumsum - sorted, masked, vocabulary ids -- of the sampler chain, under MC_SAMPLER_DEFAULT and
 * MC_SAMPLER_DRAW alike (the chain is one); refused under greedy. */
mc_status mc_decoder_get_sampler_taps(mc_decoder* d, float* out_7xk);
/* Debug / parity taps (synchronise the queue).  mc_decoder_set_taps(1) makes every step also
 * copy the hidden row after the embedding and after each owned layer into a tap buffer. */
mc_status mc_decoder_set_taps(mc_decoder* d, int32_t enable);
mc_status mc_decoder_get_logits(mc_decoder* d, void* logits_T_vocab);
mc_status mc_decoder_get_hidden(mc_decoder* d, int32_t layer, void* hidden_T_dim);
/* Logical sink-cache view of `layer` after the last step, in the reference's layout
 * [end_pos, n_kv_heads, head_dim] (include/metalchat/nn/cache.h:209-215); *n_valid = end_pos. */
mc_status mc_decoder_export_kv(mc_decoder* d, int32_t layer, void* keys, void* values,
                               int32_t* n_valid);
/* Test aid, the inverse of mc_decoder_export_kv: fill `layer`'s cache with n_valid logical rows
 * [n_valid, n_kv_heads, head_dim] of T as if positions 0 .. n_valid-1 had been decoded (the state
 * sink_cache::copy's first branch leaves, include/metalchat/nn/cache.h:206-213; n_valid <=
 * max_seq_len, the ring is reset).  A step at start_pos = n_valid continues from there, so a parity
 * test can start at the benchmark's context length.  Every owned layer must be imported with the
 * same n_valid. */
mc_status mc_decoder_import_kv(mc_decoder* d, int32_t layer, const void* keys, const void* values,
                               int32_t n_valid);
/* Bytes of weights + scales this decoder streams per token (the roofline numerator). */
size_t mc_decoder_weight_bytes(const mc_decoder* d);
/* Per-kernel timing pass used by bench.py's roofline leg: runs the named fused GEMV of every
 * owned layer back to back between two events on the queue's stream and returns the total
 * milliseconds and the algorithmic bytes moved.  which: "qkv","wo","w13","w2","head","all". */
mc_status mc_decoder_time_gemv(mc_decoder* d, const char* which, int32_t repeats, float* total_ms,
                               double* bytes_per_pass, int32_t* launches_per_pass);
/* Host name of the kernel mc_decoder_time_gemv(which) launches -- the variant a token really runs (linear-order
 * kernels, prologue / epilogue codes, the greedy pick inside the head).  which = "attn": the decode attention kernel(s) of
 * the first owned block ("mc_attn_wo_i4_*" carries the Wo GEMV, "mc_attn_qkv_wo_i4_*" / "mc_attn_qkv_wo_w_*" (plain bfloat weights) the rmsnorm +
 * wq|wk|wv GEMV + RoPE + cache write in front of it as well: the token then launches no Wo (no QKV) GEMV of its own and time_gemv("wo") /
 * time_gemv("qkv") measure stand-alone launches).  Launches nothing. */
mc_status mc_decoder_gemv_kernel_name(mc_decoder* d, const char* which, char* buf, size_t cap);
/* How often an in-launch hand-off of the decode attention gave up (its workgroups were not resident together: another stream or
 * process held part of the chip) and the decoder fell back to the launches that need no co-residency.  A step
 * (mc_decoder_step with a token read back) and a chain that stays inside the cache (mc_decoder_generate, start_pos + n <=
 * max_seq_len) are repeated on those launches and succeed; anywhere else the call that finds the flag fails with
 * MC_ERR_RUNTIME ("... repeat the call") -- the reference delivers a GPU execution error the same way, through the future that
 * is waited for (src/kernel_thread.cc:134-144). */
int32_t mc_decoder_handoff_fallbacks(const mc_decoder* d);
/* The fall-back is temporary: after 256 tokens decoded without a hand-off launch (MC_HANDOFF_REARM=<tokens>, 0 = never) the decoder takes
 * the one-launch blocks again; every further fall-back doubles that distance, so a chip that is shared for good settles on the launches
 * that need no co-residency.  mc_decoder_handoff_rearms: how often that happened; mc_decoder_handoffs_active: 1 while the decoder uses the
 * hand-off launches, 0 while it is degraded (a caller that wants to know why its tokens got slower asks here). */
int32_t mc_decoder_handoff_rearms(const mc_decoder* d);
int32_t mc_decoder_handoffs_active(const mc_decoder* d);
/* HBM bytes this decoder holds in DERIVED copies of its weights, built on demand by the prompt pass: the quad-interleaved int4 copy
 * short prompts stream from (+ 0.5 byte per weight) and the dequantised bfloat16 copy Wd = T(T(q) T(s)) that prompts of 257 rows and
 * more multiply by (+ 2 bytes per weight; built per matrix on first use where the copies of the decoder's blocks fit an eighth of the
 * device's memory and half of what is free -- MC_PF_PLAIN_COPY=1 / 0 forces / forbids; without it the same GEMM dequantises inside its
 * loop, bit for bit the same rows).  0 until a prompt has asked for one.  The reference materialises the dequantised matrix on every
 * call (quantization/lora.h:115-117); here it is built once and rebuilt when the weights change. */
size_t mc_decoder_derived_weight_bytes(const mc_decoder* d);
/* Test aid: record the host names of every kernel the decoder launches from now on (enable = 1 clears the log and
 * drops a captured token graph, whose replay would launch without passing here; 0 stops recording).
 * mc_decoder_launch_log_read copies the newline-separated names and returns the bytes needed (terminator included).
 * The reference labels every encoder with its kernel name for the same purpose (src/kernel_thread.cc:109-115). */
mc_status mc_decoder_launch_log(mc_decoder* d, int32_t enable);
size_t mc_decoder_launch_log_read(mc_decoder* d, char* buf, size_t cap);

/* Device addresses of a fused weight matrix as it lies in HBM: per layer "qkv" (wq|wk|wv rows),
 * "wo", "w13" (w1/w3 rows interleaved), "w2"; layer -1: "output".  For kernel-level tests that
 * drive mc_gemv_* through the encoder (wrap with mc_buffer_wrap_nocopy). */
mc_status mc_decoder_weight_ptrs(mc_decoder* d, int32_t layer, const char* name, void** w,
                                 void** scales, int32_t* rows, int32_t* in_features,
                                 int32_t* ngroups);

/* ------------------------------------------------------------------------------------------
 * Part 2b -- batched decode: B <= 8 sequences in lockstep over one decoder's weights (B <= 64: Part 2h, the same handle).
 * The reference's layers carry the batch already: nn::attention::operator() takes input[bs, len, dim]
 * (include/metalchat/nn/attention.h:163-206) and nn::sink_cache holds [max_batch_size, max_seq_len, n_kv_heads, head_dim],
 * writing cache[0:bs, start_pos:start_pos+len] at ONE start_pos for the whole batch (nn/cache.h:154-215); only nn::llama3
 * pins max_batch_size = 1 (nn/llama.h:86).  A batch shares the decoder's weights (streamed once per step for all rows, never
 * copied: mc_decoder_derived_weight_bytes does not change) and owns batch x n_layers caches of its own; the decoder, its
 * cache and every mc_decoder_* call are untouched.  Launches go to the decoder's stream and its launch log
 * (mc_decoder_launch_log).  A row's results do not depend on the batch size or on the other rows, bit for bit.  The batch
 * must be released before its decoder.
 * The lockstep calls keep start_pos + n <= max_seq_len whatever mc_rolling_set says (Part 2j: only ragged rows roll; a
 * caller past the end uses ragged calls with equal positions).  mc_batch_export_kv of a row that has rolled returns that row's
 * own view, as mc_ragged_export_kv does.
 * ------------------------------------------------------------------------------------------ */
typedef struct mc_batch mc_batch;
/* 1 <= batch <= 8 (up to 64: mc_wide_batch_create, Part 2h).  The decoder must be single-stage (layer_begin = 0, layer_end = n_layers), family llama3, dtype bf16,
 * qmode exact, weight_format I4 (group % 128 == 0) or T, without LoRA adaptors, head_dim 128 or 64, every linear with
 * out_features % 16 == 0 and in_features % 1024 == 0; otherwise MC_ERR_INVALID_ARGUMENT naming the reason. */
mc_status mc_batch_create(mc_decoder* d, int32_t batch, mc_batch** out);
void mc_batch_release(mc_batch* b);
int32_t mc_batch_size(const mc_batch* b);
/* copy the decoder's cache positions [0, n_valid) of every layer into row `row` (prompt once, fork B times);
 * n_valid <= max_seq_len and <= the positions the decoder holds, and the decoder's cache must not have rolled */
mc_status mc_batch_fork(mc_batch* b, int32_t row, int32_t n_valid);
/* test aids, the reference's layout [n_valid, n_kv_heads, head_dim] of T, as mc_decoder_import_kv / export_kv; the batch's
 * position is shared, so *n_valid of export is the batch's (the last import, fork or step) */
mc_status mc_batch_import_kv(mc_batch* b, int32_t row, int32_t layer, const void* keys, const void* values, int32_t n_valid);
mc_status mc_batch_export_kv(mc_batch* b, int32_t row, int32_t layer, void* keys, void* values, int32_t* n_valid);
/* transform(input[B, 1], start_pos): tokens[B] in, next_tokens[B] out (greedy, or the decoder's sampler per row --
 * mc_decoder_set_sampler, read at every step).  start_pos + 1 <= max_seq_len: a batch's cache does not roll. */
mc_status mc_batch_step(mc_batch* b, const int32_t* tokens, int32_t start_pos, int32_t* next_tokens);
/* n chained lockstep steps on the device, token feedback through HBM, one host sync; tokens_out[n][B];
 * start_pos + n <= max_seq_len */
mc_status mc_batch_generate(mc_batch* b, const int32_t* first_tokens, int32_t start_pos, int32_t n, int32_t* tokens_out);
/* seed pair (i * B + r) % n_pairs for row r of token i of one call (mc_batch_step: i = 0); no pairs = (0, 0) */
mc_status mc_batch_set_seeds(mc_batch* b, const uint64_t* seeds, int32_t n_pairs);
/* after a step: [B][vocab] logits of T */
mc_status mc_batch_get_logits(mc_batch* b, void* logits_T);

/* ================================================================================================
 * Part 2c -- ragged rows: the rows of an mc_batch, each at a position of its own.
 * Several chats have prompts of different lengths, finish at different times and arrive at different times.  These calls
 * decode every row at its own position, stop each row on its own stop id or at the end of its cache without ending the call
 * for the others, and leave rows idle (position -1: their caches, lengths and state are not touched, their outputs are -1),
 * so that a finished row can be refilled by a fork while the other rows keep their caches.
 * The batch keeps each row's valid cache length: 0 at creation; n_valid after a fork or an import of that row; start_pos +
 * steps for every row after a lockstep step or generate; positions[r] + tokens produced after a ragged call.  An active row
 * needs 0 <= positions[r] <= its length and positions[r] < max_seq_len (a position below the length rewinds the row), and a
 * token of the vocabulary; anything else -- or no active row, n < 1, n_stop < 0, a null pointer -- is refused with
 * MC_ERR_INVALID_ARGUMENT naming the row and the reason before anything is enqueued.
 * Sampling is the decoder's sampler, read at every call; token i of row r uses seed pair (i * B + r) % n_pairs, as a
 * lockstep call does, so a ragged call whose rows all share one position computes the lockstep call's tokens, logits and
 * K/V bit for bit.  Ragged calls do not move the lockstep calls' shared position.
 * All of this is the default.  Part 2j (mc_rolling_set) lifts "positions[r] < max_seq_len" and the stop at the end of
 * the cache for a batch that opts in: its rows decode on nn::sink_cache's ring, as the batch-1 decoder does.
 * ------------------------------------------------------------------------------------------ */
/* one step of every active row at positions[r]; next_tokens[B] (may be null): the picks, -1 for an idle row */
mc_status mc_ragged_step(mc_batch* b, const int32_t* tokens, const int32_t* positions, int32_t* next_tokens);
/* up to n chained steps per row on the device, one host sync.  Row r stops after its first produced token that is one of
 * stop_ids[0, n_stop) (that token is written), or once it has written cache position max_seq_len - 1; the call itself is
 * not refused for it.  tokens_out[n][B]: -1 after a row stopped and for an idle row; lengths[B]: the tokens row r produced
 * (its cache length becomes positions[r] + lengths[r]). */
mc_status mc_ragged_generate(mc_batch* b, const int32_t* first_tokens, const int32_t* positions, int32_t n,
                             const int32_t* stop_ids, int32_t n_stop, int32_t* tokens_out, int32_t* lengths);
/* the valid cache length of every row: lengths[B] */
mc_status mc_ragged_lengths(const mc_batch* b, int32_t* lengths);
/* row `row`'s own valid positions [0, length) in the layout of the batch's export_kv; *n_valid = the row's length */
mc_status mc_ragged_export_kv(mc_batch* b, int32_t row, int32_t layer, void* keys, void* values, int32_t* n_valid);

/* ================================================================================================
 * Part 2d -- the packed prompt pass: the prompts of several rows of an mc_batch in ONE prompt pass over the decoder's weights.
 * Every weight matrix is multiplied once for all of them (M = the sum of the lengths rows); only the rope + cache write and the
 * attention know which row a prompt row belongs to.  Row r gets exactly what mc_decoder_prefill of its chunk at start_pos =
 * positions[r] does to a decoder's cache -- the reference's mask included: only the chunk's own columns form the causal square,
 * so a chunk at positions[r] > 0 does not see the row's earlier context (pf_visible) -- written to the row's own
 * cache at [positions[r], positions[r] + lens[r]); its length becomes positions[r] + lens[r] (a position below the length
 * rewinds the row, as in ragged calls).  Rows with lens[r] = 0 are not in the call: their caches, lengths and state stay.
 * The decoder's cache, step state, sampler settings and taps stay as they were; its prompt scratch and derived weight copies
 * serve the call as they serve mc_decoder_prefill.  Launches go to the decoder's stream and launch log.
 * ------------------------------------------------------------------------------------------ */
/* tokens: the chunks of the rows in the call, concatenated in row order (sum of lens ids); lens[B]: row r's chunk length, 0 =
 * not in the call; positions[B]: where row r's chunk starts in its cache.  next_tokens[B] (may be null): each row's pick after
 * its chunk's last row (the decoder's sampler read at the call, seed pair r % n_pairs), -1 for a row not in the call; the
 * batch's logits (mc_batch_get_logits) are then the last-row logits of the rows in the call.  Refused with
 * MC_ERR_INVALID_ARGUMENT naming the row and the reason, before anything is enqueued: a null pointer, no row in the call,
 * lens[r] < 0, lens[r] == 1 (a one-token chunk is a ragged step), positions[r] < 0 or past the row's length, positions[r] +
 * lens[r] > max_seq_len, a token outside the vocabulary, a sum of lens above max_seq_len (split such a call by rows). */
mc_status mc_rows_prefill(mc_batch* b, const int32_t* tokens, const int32_t* lens, const int32_t* positions, int32_t* next_tokens);

/* ================================================================================================
 * Part 2e -- chunks that see their row's context: the packed pass of Part 2d with ONE difference.  Chunk row i of row r
 * (position p = positions[r] + i) attends to cache columns c <= p of row r, ALL of them: the columns below positions[r] are
 * whatever the row's cache holds (from a fork, an import, steps, an earlier chunk or prompt pass).  Row r gets what lens[r]
 * successive decode steps over its chunk compute -- each of the reference's steps sees the whole cache -- in one pass over
 * the weights: a follow-up message fed to a live row, a long prompt fed in chunks between the other rows' steps.  At
 * positions[r] == 0 the two calls mean the same thing (their bits may differ: the softmax sums are ordered differently).
 * Everything else is Part 2d's: arguments, packing, seeds, next_tokens, the batch's logits, the lengths afterwards, the rewind
 * by a position below the length, rows with lens[r] = 0 and the decoder untouched, and the refusals (the same conditions, the
 * texts prefixed with this call's name; lens[r] == 1 stays refused: a one-token chunk is a ragged step).  A row's result does
 * not depend on which other rows are in the call.  bfloat16, head_dim 64 and 128 (what a batch admits).
 * ------------------------------------------------------------------------------------------ */
mc_status mc_extend_rows(mc_batch* b, const int32_t* tokens, const int32_t* lens, const int32_t* positions, int32_t* next_tokens);

/* ================================================================================================
 * Part 2f -- speculative verify: Part 2e's pass with a greedy pick after EVERY chunk row and the acceptance on the device.  A
 * draft (a smaller model on a second decoder, a prompt-lookup table, anything) proposes tokens for a row; the target checks all
 * of them in one pass over its weights and keeps the longest prefix it would have produced itself.  Row r's chunk is c[0 .. n),
 * n = lens[r]: c[0] is the row's last accepted token (not yet in its cache), c[1 .. n) are n - 1 drafted tokens.  The layer pass
 * is mc_extend_rows': the same launches, the same K / V written to [positions[r], positions[r] + n).  Then every packed row goes
 * through the final norm and the head -- one pass over the head's weights for all of them, each row's logits bit for bit what
 * the batch's own head gives for that hidden row -- and pick[i] is the first index of the maximum of chunk row i's logits.
 *   a_r = the largest a <= n - 1 with c[i + 1] == pick[i] for all i < a      (the drafts the target would have produced)
 * Afterwards row r's length is positions[r] + a_r + 1: the slots of the rejected drafts stay written but lie past the length,
 * the rewound state every rows call handles (a later call at the new length overwrites them).  mc_batch_get_logits then holds,
 * for each row in the call, the logits of chunk row a_r.  Feed next_tokens[r] at position positions[r] + a_r + 1.
 * Greedy only: with the decoder's sampler set to anything else the call is refused ("... greedy").  2 <= lens[r] <=
 * 16 (MC_VERIFY_MAX_LEN of the kernel ABI) for a row in the call (one attention tile per row: at most 128 packed rows); a longer chunk is refused
 * naming the row, and a one-token chunk (no drafts) stays a ragged step.  All of Part 2e's refusals apply with the texts
 * prefixed "mc_verify_rows: ", nothing enqueued.  The scratch ([128][vocab] logits and [128][dim] rows) is allocated at the first
 * call, so a batch that never verifies holds what it held.  The decoder, rows outside the call and the independence of a row's
 * bits from B, placement and company are as in Part 2e -- whose pass has one place where the call as a whole reaches a row: with
 * int4 weights the decoder multiplies a prompt pass of at most 64 rows by another GEMM than a longer one, and the two order their
 * sums differently (a few elements differ in their last bits).  Calls on one side of that line agree bit for bit.
 * ------------------------------------------------------------------------------------------ */
/* tokens / lens / positions: exactly mc_extend_rows' (Part 2e).
 * picks (sum of lens ids, packed like tokens; may be null): picks[off_r + i] = the greedy pick after chunk row i.
 * accepted[B]: a_r; -1 for a row not in the call.
 * next_tokens[B] (may be null): pick[a_r] -- the token to feed at position positions[r] + a_r + 1; -1 for a row not in the call. */
mc_status mc_verify_rows(mc_batch* b, const int32_t* tokens, const int32_t* lens, const int32_t* positions,
                         int32_t* accepted, int32_t* next_tokens, int32_t* picks);
/* test aid: the [sum of lens][vocab] logits of T of the last mc_verify_rows or (Part 2g) mc_tree_verify call on the batch,
 * packed like its tokens; refused while the batch has made neither call */
mc_status mc_verify_get_logits(mc_batch* b, void* logits_T);

/* ================================================================================================
 * Part 2g -- speculative verify over a draft TREE per row.  Part 2f spends a row's 15 drafts on one guess, and everything behind
 * the first wrong draft is lost; a tree of the same <= 16 nodes carries alternatives at the shallow depths where rejections
 * happen (several prompt-lookup matches, a small model's runner-up picks) at the same price: the same packed rows, the same one
 * pass over the weights and the head.  Row r's chunk is nodes [0, n), n = lens[r], 2 <= n <= 16 (MC_VERIFY_MAX_LEN): node 0 is the
 * row's last accepted token (not yet in its cache), nodes [1, n) are drafts, and parents[off_r + i] names node i's parent:
 * parents[off_r] == -1 and 0 <= parents[off_r + i] < i for i >= 1 -- topological order, so a node's index is at least its depth.
 *   depth(0) = 0, depth(i) = depth(parent(i)) + 1;  node i sits at position positions[r] + depth(i) (its rope position)
 *   node i attends to every cache column below positions[r], and among the chunk's nodes to its ancestors and itself -- nothing else
 *   pick[i] = the target's greedy pick after node i: what a chain of decode steps over the path root -> i computes
 * Acceptance, on the device: cur = 0; among cur's children in ascending node index the first j with tokens[j] == pick[cur]
 * becomes cur; stop when there is none.  a_r = depth(cur).  Equal tokens on two siblings are legal (the lower index wins); a match
 * under a rejected node never counts.  During the pass node i's K / V live in cache slot positions[r] + i; afterwards the accepted
 * path's K / V are moved to slots positions[r] + d, d = 0 .. a_r, in every layer (one launch, no host round trip), the row's
 * length is positions[r] + a_r + 1, and mc_batch_get_logits holds the logits of the last accepted node for each row in the call.
 * Slots past the new length may hold what the call wrote there: the rewound state every rows call handles.
 * A tree that is a chain (parents = -1, 0, 1, ...) computes Part 2f's call bit for bit: the same K / V, logits, picks, accepted.
 * Any other tree holds a path's keys in other slots than a chain would, so its sums take another order: the same values within
 * the rounding of the arithmetic, not the same bits.
 * Greedy only, refused as in Part 2f.  All of Part 2e's refusals apply with the texts prefixed "mc_tree_verify: ", and, naming the
 * row: a root whose parent is not -1, a parent outside [0, i), a chunk longer than 16; a null pointer (parents included) is
 * refused as a null argument.  MC_ERR_INVALID_ARGUMENT, nothing enqueued.  Scratch, the decoder, rows outside the call, and the
 * independence of a row's bits from B, placement and company are as in Part 2f.
 * ------------------------------------------------------------------------------------------ */
/* tokens / lens / positions: packed exactly as in Part 2f; parents: packed like tokens.
 * accepted[B]: a_r.  next_tokens[B] (may be null): pick[cur], to feed at position positions[r] + a_r + 1.
 * paths[B][MC_VERIFY_MAX_LEN] (may be null): the accepted node at each depth 0 .. a_r, -1 behind it.
 * picks (sum of lens ids, packed like tokens; may be null): the greedy pick after every node.
 * Rows not in the call: -1 in accepted, next_tokens and all of their paths row. */
mc_status mc_tree_verify(mc_batch* b, const int32_t* tokens, const int32_t* parents, const int32_t* lens, const int32_t* positions,
                         int32_t* accepted, int32_t* next_tokens, int32_t* paths, int32_t* picks);

/* ================================================================================================
 * Part 2h -- wide batches: up to 64 rows per step.  mc_batch_create's 8 rows are the columns of ONE 16-column MFMA tile; a wide
 * batch multiplies every linear layer for all of its rows in one pass over the weights with up to four such column groups
 * (mc_wb_gemv_*), so 64 chats pay the weight stream once per token and not eight times.  The row contract does not change: a
 * row's tokens, logits and K / V do not depend on the batch size, on the row's index or on the other rows, bit for bit -- across
 * the two creation calls and across the 16-row line at which the launch changes (up to 16 rows still run mc_batch_create's
 * launches).  Row r of a wide batch computes what row r % 8 of a batch of 8 computes from the same cache and tokens.
 * Everything of Parts 2b - 2g runs on the handle with B up to 64; seeds, idle rows, stop ids, lengths and refusals are as there.
 * One bound becomes reachable: a verify call (Parts 2f, 2g) holds at most 128 packed rows (MC_VERIFY_MAX_ROWS of the kernel ABI),
 * which eight rows of at most 16 tokens never exceed and 64 rows can; such a call is refused with MC_ERR_INVALID_ARGUMENT,
 *   "...: the chunks add up to N rows, more than MC_VERIFY_MAX_ROWS (128): split the call by rows"
 * nothing enqueued and no row's length changed.  mc_rows_prefill and mc_extend_rows keep their own bound, a sum of lengths no
 * greater than max_seq_len.  Memory scales with batch as in Part 2b: batch x n_layers caches and the per-row scratch.
 * ------------------------------------------------------------------------------------------ */
/* 1 <= batch <= 64 (MC_WIDE_BATCH_MAX of the kernel ABI).  Admits every decoder mc_batch_create admits, and more (Part 2i); the
 * texts are prefixed "mc_wide_batch_create: ", those of conditions both calls share are the same; a batch outside the range:
 * "mc_wide_batch_create: batch must lie in [1, 64]", checked before anything of the decoder is looked at, as mc_batch_create does.
 * For a decoder mc_batch_create admits, with batch <= 8 the call makes exactly what mc_batch_create makes.  The handle is an
 * mc_batch: every call of Parts 2b - 2g takes it, mc_batch_release frees it. */
mc_status mc_wide_batch_create(mc_decoder* d, int32_t batch, mc_batch** out);

/* ================================================================================================
 * Part 2i -- QLoRA rows: what mc_wide_batch_create admits.  mc_batch_create keeps its predicate, texts and bound; the general
 * entry also takes the one quantised checkpoint flavour the reference ships, MC_CKPT_META_LLAMA3_QLORA (int4 linears in groups of
 * 32, a rank-16 LoRA adaptor on each, an int8 embedding table, an int8 head with one scale per row), and what lies between.  A
 * decoder is admitted when
 *   - as for mc_batch_create: single stage, family llama3, dtype bf16, MC_QMODE_EXACT, head_dim 128 or 64, n_heads a multiple of
 *     n_kv_heads (at most 16 per kv head), max_seq_len >= 64, an embedding table of T or int8 with one scale per row, every linear
 *     with out_features % 16 == 0 and in_features % 1024 == 0, and layer shapes that chain;
 *   - each of the seven layer linears and the head, judged on its own, is MC_WFMT_T, MC_WFMT_I4 or MC_WFMT_I8, a quantised one in
 *     groups that are a multiple of 32 or with one scale per row (group 0); the formats may differ between linears and from
 *     cfg.weight_format (no "mixed weight formats" refusal on this entry);
 *   - LoRA adaptors (mc_decoder_load_lora) sit on layer linears only, and the adaptor columns of a fused matrix -- adaptors x rank
 *     -- are a multiple of 16, i.e. rank % 16 == 0: otherwise "<matrix>: LoRA rank must be a multiple of 16".
 * A linear with an adaptor computes T(T(x Wd^T) + T(T(B (A x)) * scale)) per row, quantization::lora_linear's arithmetic
 * (quantization/lora.h:119-121), in two launches: a = T(A x) for all rows, then the GEMV with the adaptor term in front of its
 * epilogue.  The decoder is untouched (its own adaptor scratch is not used).  The row contract of Parts 2b - 2h holds unchanged:
 * a row's tokens, logits and K / V do not depend on the batch size, its index or the other rows, bit for bit; every call of Parts
 * 2b - 2g runs on such a batch with B from 1 to 64.  Not admitted: gemma3, MC_QMODE_FAST, float32, adaptors on the head, ranks
 * that are not multiples of 16.
 * ------------------------------------------------------------------------------------------ */

/* ================================================================================================
 * Part 2j -- rolling rows: the ragged rows of a batch decode past max_seq_len, opt-in per batch.  nn::sink_cache carries the batch
 * dimension and rolls for it (nn/cache.h:154-215): once start_pos >= max_seq_len the first pre_len rows stay, the rest rotates left
 * and the new row takes the last slot.  mc_decoder_* does that on a zero-copy ring; with rolling enabled mc_ragged_step and
 * mc_ragged_generate do it per row, so a chat that outlives its cache stays in its batch.  With S = max_seq_len, post = S - pre_len:
 *   positions   an active row may sit at any positions[r] >= 0.  Below S nothing changes.  At p >= S the row is in the state the
 *               decoder reaches after p - S + 1 single-step rolls from a linear cache: ring_base = (p - S + 1) % post, the new row
 *               goes to slot pre_len + (post - 1 + ring_base) % post, and S positions are attended.  Rows get past the end by single
 *               steps only, so the state follows from p and the batch keeps nothing but the lengths.
 *   stopping    a row stops on its stop ids only, never for the end of its cache.  lengths[r] of mc_ragged_generate and
 *               mc_ragged_lengths are absolute and may exceed S.
 *   rope        cos / sin of the absolute position, bit for bit the row mc_rope_table writes for it, made on the device at the
 *               start of every step (chained steps included: no host round trip).
 *   rewinds     once a row's length exceeds S its evicted positions are gone: positions[r] must equal the length, or be 0 (a
 *               restart).  Anything between is refused with MC_ERR_INVALID_ARGUMENT,
 *                 "...: row r: position p lies below the row's length n and the row has rolled"
 *               nothing enqueued, by every rows call of Parts 2c - 2g and in either mode.  "past the row's length" stays.
 *   export      mc_ragged_export_kv (and mc_batch_export_kv for such a row) returns the logical view of min(length, S) positions:
 *               the sink rows, then the ring unrolled, as mc_decoder_export_kv does; *n_valid = min(length, S).
 *   the rest    mc_batch_import_kv, mc_batch_fork, and mc_rows_prefill / mc_extend_rows at position 0 make a rolled row linear
 *               again, as they overwrite any row.  The packed passes and both verify calls keep positions[r] + lens[r] <= S with
 *               their texts, so they refuse a rolled row: a follow-up turn on a rolled row is fed by ragged steps.  The lockstep
 *               calls keep their bound in both modes.  mc_batch_fork still refuses a decoder whose ring has turned.
 * The row contract holds unchanged: a row's tokens, logits and K / V do not depend on B, on its index or on the other rows --
 * rolled, not rolled or idle -- bit for bit, for B from 1 to 64 and every decoder mc_wide_batch_create admits.  A row that stays
 * below S computes the same bits with rolling on and off.  Not covered: chunks on rolled rows (the reference's chunk past the end
 * rotates by its length, which is not what that many steps compute), lockstep rolling, forking a rolled decoder, gemma3.
 * The calls carry a prefix of their own, mc_rolling_, as every part's do.
 * ------------------------------------------------------------------------------------------ */
/* 0 (default): rows stop at the end of their cache and positions[r] < max_seq_len.  1: ragged rows roll.  Any other value is refused.
 * Switching back to 0 keeps the rows; one whose length exceeds max_seq_len can then only be restarted at 0. */
mc_status mc_rolling_set(mc_batch* b, int32_t enable);
int32_t mc_rolling_enabled(const mc_batch* b); /* 0 for a null batch */
/* copy row src's valid cache -- the min(length, max_seq_len) physical slots of every layer -- and its length onto row dst of the same
 * batch.  Works on a rolled row, whose ring follows from its length: the one way to branch a chat that has rolled.  Refused: a null
 * batch, a row out of range, dst == src. */
mc_status mc_rolling_fork_row(mc_batch* b, int32_t dst, int32_t src);

/* ================================================================================================
 * Part 2k -- row samplers: each row of a batch picks with settings of its own.  A serving loop holds requests of different callers
 * -- one greedy, one at temperature 0.6 / top-p 0.9, one at temperature 1.0 / top-k 20 -- and one batch serves them all over one
 * pass of the weights.  A row slot is MC_SAMPLER_INHERIT (the default: it follows mc_decoder_set_sampler, read at every call, as
 * before), MC_SAMPLER_GREEDY, or MC_SAMPLER_DEFAULT or MC_SAMPLER_DRAW with its own top_k, temperature and top_p.  Only a
 * MC_SAMPLER_DRAW row's pick depends on its seed pair (Part 2: the rule, and why a loop uploads n * B fresh pairs per call).
 *   settings   belong to the row SLOT and hold until set again or reset; they are read at every call, as the decoder's sampler is.
 *              mc_batch_fork, mc_rolling_fork_row, imports and prompt passes leave them alone: a loop that refills a slot sets the
 *              slot's sampler with it.  MC_SAMPLER_DEFAULT and MC_SAMPLER_DRAW take mc_decoder_set_sampler's checks, texts and rounding.
 *   seeds      unchanged: token i of row r uses pair (i * B + r) % n_pairs (mc_batch_set_seeds).  A greedy row draws nothing; the
 *              pair index of a row does not depend on the other rows' kinds.
 *   the rows   the row contract extends to the sampler: a row's tokens, logits and K / V do not depend on B, on its index, or on
 *              the other rows OR THEIR SAMPLERS, bit for bit.  Row r with settings X computes exactly what it computes in a batch
 *              whose decoder-wide sampler is X.  Every pick of every batch call (Parts 2b - 2e, 2h - 2j) goes through it.
 *   launches   no row samples: mc_b_argmax_*; all rows sample with equal settings: mc_b_topk_candidates_bfloat + mc_b_sample_*,
 *              both as before -- a batch on which no row sampler is set (or after mc_row_sampler_reset) launches exactly what it
 *              launched before this part; all rows MC_SAMPLER_DRAW with equal settings: mc_b_topk_candidates_bfloat +
 *              mc_draw_b_*.  Anything else (any mixture with a drawing row included): mc_b_topk_candidates_mixed_bfloat + mc_b_pick_mixed_*, which read a
 *              [B] table of the effective settings and branch per row (DESIGN.md s.4 "Row samplers").
 *   verify     mc_verify_rows and mc_tree_verify look at the EFFECTIVE sampler of the rows in the call (lens[r] > 0): a sampling
 *              row outside the call no longer blocks the others, and a row set to MC_SAMPLER_GREEDY verifies under a sampling
 *              decoder.  A row in the call that is not greedy is refused, nothing enqueued:
 *                "mc_verify_rows: row r: the row's sampler is not greedy (accepting sampled drafts needs the draft's probabilities)"
 *              (mc_tree_verify: its own prefix).  With no row sampler set the decoder-wide refusal keeps its text.
 *              Part 2m lifts this refusal per batch: the pick after every chunk row is then the row's own sampler's.
 * Not covered: accepting drafts that were themselves sampled (Part 2m verifies sampling rows against drafts proposed without a draw), log-probabilities (Part 2n has them), samplers other than these three, top_k above 128, seed state kept on the device
 * between calls, the batch-1 decoder.
 * ------------------------------------------------------------------------------------------ */
enum { MC_SAMPLER_INHERIT = -1 }; /* a row that follows mc_decoder_set_sampler: the default of every row */
/* kind: MC_SAMPLER_INHERIT, MC_SAMPLER_GREEDY, MC_SAMPLER_DEFAULT or MC_SAMPLER_DRAW; top_k, temperature and top_p are checked for the
 * last two only ("nucleus_sampler: temperature must be positive", "nucleus_sampler: probability must be in [0.0, 1.0]", "topk_sampler: the
 * fused sampler keeps 1..128 candidates").  An unknown kind, a row outside [0, B) and a null batch are refused with texts prefixed
 * "mc_row_sampler_set: ".  All MC_ERR_INVALID_ARGUMENT; a refused call launches nothing and changes nothing. */
mc_status mc_row_sampler_set(mc_batch* b, int32_t row, int32_t kind, int32_t top_k, float temperature, float top_p);
/* what was set: the caller's values, not the rounded ones.  An inheriting row: *kind = MC_SAMPLER_INHERIT and the other outputs
 * untouched.  top_k, temperature and top_p may be null. */
mc_status mc_row_sampler_get(const mc_batch* b, int32_t row, int32_t* kind, int32_t* top_k, float* temperature, float* top_p);
/* every row back to MC_SAMPLER_INHERIT */
mc_status mc_row_sampler_reset(mc_batch* b);

/* ================================================================================================
 * Part 2l -- row logit processors: per-row token masks and penalties.  A serving loop must be able to shape what a row may pick: hold it
 * to a set of tokens (JSON or grammar output, a choice among N answers, a ban list, "no EOS before n tokens") and apply the
 * repetition, frequency and presence penalties that every public API exposes next to temperature and top_p -- without giving up
 * mc_ragged_generate's chained steps.  A row slot holds an optional mask (`allowed` bits, one per token), penalties (rep, freq, pres),
 * neutral at (1, 0, 0), and a count c[t] per token.
 *   the rule   T is bfloat16, x the float value of a logit, every operation one float32 operation in the order written.  For a row
 *              with anything set, every element t of its logits row becomes
 *                c  = c[t]                                   (after this step's input token has been counted, below)
 *                x1 = c > 0 ? (x > 0 ? x * inv_rep : x * rep) : x        inv_rep = float(1.0f / rep), formed once on the host
 *                x2 = c > 0 ? x1 - (freq * float(c) + pres) : x
 *                y  = allowed(t) ? T(x2) : -inf              (T: round to nearest even; an untouched x keeps its bits)
 *              y is written in place into the batch's logits, and the unchanged pick launches run on them: a processed row's pick is
 *              what its effective sampler (Part 2k) picks from y with the row's own seed pair, and mc_batch_get_logits returns y.
 *              There is no division on the device.  Neutral penalties with no mask are the identity, bit for bit, -0.0 included.
 *   counts     c[t] = how often token t was fed to the row as a step input since its counts were last cleared: mc_batch_step /
 *              _generate and mc_ragged_step / _generate, every chained step included.  The process launch of a step first counts that
 *              step's input token for each active row with (non-neutral) penalties, then penalises; the thread that owns element t
 *              increments and uses the new value (no atomics), so in a chained call every pick is counted before the next pick, with
 *              no host round trip.  Idle rows and rows that stopped count nothing.  The packed passes (mc_rows_prefill,
 *              mc_extend_rows) are processed with the counts as they stand and count nothing of their chunks: a caller that wants
 *              the prompt in the history adds it with mc_row_penalty_count.  Counts are int32 [B][vocab] on the device, allocated at
 *              the first mc_row_penalty_set or _count, as the mask words [B][(vocab + 31) / 32] are at the first mask: a batch that
 *              uses neither holds what it held.  Rewinds do not rewind counts: the caller clears and recounts.
 *   state      mask, penalties and counts belong to the row SLOT, as samplers do: mc_batch_fork, mc_rolling_fork_row, imports and
 *              prompt passes leave them alone.
 *   the rows   the row contract extends: a row's tokens, logits and K / V do not depend on B, on its index, or on the other rows,
 *              their samplers OR THEIR PROCESSORS, bit for bit (narrow, wide, QLoRA and rolling batches).  A row with nothing set
 *              computes exactly what it computed before.
 *   launches   a batch on which no row has anything set launches exactly what it launched before this part -- also after
 *              mc_row_logits_reset, or with every mask removed and every penalty neutral.  Otherwise one more launch per head,
 *              mc_b_logits_process_*, between the head GEMV and the pick (DESIGN.md s.4 "Row logit processors").
 *   verify     mc_verify_rows and mc_tree_verify refuse a row in the call (lens[r] > 0) that has a mask or non-neutral penalties,
 *              nothing enqueued:
 *                "mc_verify_rows: row r: the row has a token mask or penalties (a verify call would need them per chunk row)"
 *              (mc_tree_verify: its own prefix).  Rows outside the call do not matter.
 * Refusals: all MC_ERR_INVALID_ARGUMENT, prefixed with the call's name; nothing is launched and nothing changes.  A null batch, a row
 * outside [0, B), and what each call names below.  Uploads are synchronous (every batch call drains the stream before it returns).
 *              Part 2m lifts this refusal per batch: the slot's mask and its counts plus the chunk's tokens then apply to every chunk row.
 * Not covered: the batch-1 decoder, additive logit bias lists, masks that change per chunk row in verify calls (grammar state), log-probabilities, samplers other
 * than the two the project has.
 * ------------------------------------------------------------------------------------------ */
/* bit t % 32 of word t / 32 set = token t may be picked; n_words == (vocab + 31) / 32; bits at and above vocab are ignored;
 * allowed == NULL (n_words ignored) removes the mask.  Refused: another n_words, a mask that allows no token below vocab
 * ("mc_row_mask_set: the mask allows no token"). */
mc_status mc_row_mask_set(mc_batch* b, int32_t row, const uint32_t* allowed, int32_t n_words);
/* *is_set = 0 / 1; with a mask set and allowed != NULL (then n_words as above) its words, zeros at and above vocab */
mc_status mc_row_mask_get(const mc_batch* b, int32_t row, int32_t* is_set, uint32_t* allowed, int32_t n_words);
/* Refused: repetition not finite or <= 0, frequency or presence not finite.  (1, 0, 0) is neutral. */
mc_status mc_row_penalty_set(mc_batch* b, int32_t row, float repetition, float frequency, float presence);
/* the caller's values; each output may be null */
mc_status mc_row_penalty_get(const mc_batch* b, int32_t row, float* repetition, float* frequency, float* presence);
/* adds n tokens to the row's history.  Refused: n < 0, a null `tokens` with n > 0, a token outside the vocabulary (the text names
 * its index). */
mc_status mc_row_penalty_count(mc_batch* b, int32_t row, const int32_t* tokens, int32_t n);
/* the row's counts [vocab], read back */
mc_status mc_row_penalty_counts(mc_batch* b, int32_t row, int32_t* counts);
/* the row's counts to zero */
mc_status mc_row_penalty_clear(mc_batch* b, int32_t row);
/* every row: no mask, neutral penalties, zero counts */
mc_status mc_row_logits_reset(mc_batch* b);

/* ================================================================================================
 * Part 2m -- verify calls for sampling, masked and penalised rows, opt-in per batch.  Parts 2k and 2l let one batch serve rows
 * with different settings, and both verify calls (Parts 2f, 2g) refuse every such row.  MC_SAMPLER_DRAW is a pure function of the
 * logits row, the row's settings and one seed pair, so the pick after any chunk row can be made on the device exactly as a ragged
 * step makes it.  For a drafter that proposes a token WITHOUT drawing -- prompt lookup, a greedy draft model -- the proposal q is a
 * point mass on the draft x, and "accept x where it equals the row's own draw" is exact speculative sampling: x is accepted with
 * P(draw == x) = p(x) = min(1, p / q), and on rejection the row's own draw is emitted, which is p conditioned on != x, i.e.
 * norm(max(0, p - q)).  The draft's probabilities are not needed, and the output is what lens[r] ragged steps with the same seed
 * pairs pick from the same logits.  MC_SAMPLER_DEFAULT never draws and verifies the same way.
 * With the switch off (the default) both verify calls refuse what they refused, with the same texts.  With it on the two refusals
 * "the row's sampler is not greedy" / "the decoder's sampler is not greedy" and "the row has a token mask or penalties" are not
 * raised; every other refusal keeps its text (lengths, positions, MC_VERIFY_MAX_ROWS, rolled rows, tree shape).  Then, r a batch
 * row in the call, j a chunk row of its segment (a tree: node j at depth d):
 *   processors  a row with a mask or non-neutral penalties has the logits of each of its packed rows rewritten in place before the
 *               pick, by Part 2l's rule with allowed = the slot's mask and c[t] = the slot's count + the number of chunk tokens equal
 *               to t among tokens[0 .. j] (a tree: on the path from the root to node j, both included) -- what the ragged steps
 *               would have counted: a step counts its input, then penalises.  Nothing is written to the counts before the
 *               acceptance; behind it the counts of a row with penalties gain the accepted[r] + 1 tokens that were fed (chunk rows
 *               0 .. accepted[r], a tree's accepted path; a token fed twice counts twice).  mc_verify_get_logits and
 *               mc_batch_get_logits return the processed rows, as after a step.
 *   picks       picks[m] is what row r's effective sampler (Part 2k) picks from packed row m's processed logits with seed pair
 *               (j * B + r) % n_pairs, a tree (d * B + r) % n_pairs (siblings share a pair: they are alternatives for one draw) --
 *               the pair mc_ragged_generate uses for token j of row r.  A caller uploads MC_VERIFY_MAX_LEN * B fresh pairs in front
 *               of each call.  A greedy row takes the first index of the maximum.
 *   the rest    acceptance, the tree walk, the K / V compaction and the lengths are Parts 2f / 2g's, run on these picks.
 *   launches    a call whose rows are all greedy and unprocessed launches exactly what it launches with the switch off.  Otherwise
 *               mc_v_argmax_bfloat gives way to mc_vs_topk_candidates_mixed_bfloat + mc_vs_pick_mixed_bfloat over the packed rows
 *               (when a row in the call samples), and at most one launch in front of the pick (mc_vs_logits_process_bfloat) and one
 *               behind the acceptance (mc_vs_count_accepted) are added.  The per-packed-row table and the candidate keys are
 *               reserved at the first call that needs them.
 *   the rows    a row's picks, logits, K / V and counts do not depend on B, on its index, or on the other rows and their settings.
 * The switch belongs to the batch: mc_batch_fork, imports and the resets of Parts 2k / 2l leave it alone.
 * Not covered: drafts that were themselves sampled (a real q), masks that change per chunk row (grammar state), the batch-1
 * decoder, rolled rows in verify calls.  The calls carry a prefix of their own, mc_settings_verify_ (Part 2f's test pins the set
 * of names that begin with the verify calls' prefix).
 * ------------------------------------------------------------------------------------------ */
/* 0 (default): the verify calls refuse sampling, masked and penalised rows.  1: they take them.  A null batch and any other value
 * are refused with MC_ERR_INVALID_ARGUMENT, texts prefixed "mc_settings_verify_set: "; nothing changes. */
mc_status mc_settings_verify_set(mc_batch* b, int32_t enable);
int32_t mc_settings_verify_enabled(const mc_batch* b); /* 0 for a null batch */

/* ================================================================================================
 * Part 2n -- row log-probabilities: the pick's and the top n, opt-in per batch.  Best-of-n over forked rows is ranked by the sum of
 * each row's token log-probabilities, a choice among N masked answers is scored by the answer's, and serving APIs report `logprobs`
 * / `top_logprobs` next to the sampler settings of Parts 2k and 2l.  With the switch on, every pick of the batch leaves a record,
 * made on the device behind the pick, so chained calls keep their chain.  For one row, y[0..V) the bfloat16 logits the pick read
 * -- what mc_batch_get_logits returns: after the row's mask and penalties, before temperature and truncation:
 *   M      = max y                                        (a mask that allows no token is refused, so M is finite)
 *   S      = sum over t of exp(double(y[t]) - double(M))  in float64; exp(-inf) = 0
 *   lse    = double(M) + log(S)                           float64
 *   lp[t]  = float(double(y[t]) - lse)                    one rounding; a banned token's lp is -inf
 *   top n  = the n largest y in the sampler's key order (value descending, -0 == +0, then LOWER index), each with its lp
 * This is the model's distribution over the processed logits at temperature 1, what OpenAI-style `logprobs` report.  It is not
 * the sampler's truncated nucleus.  The device evaluates exp, log, the sums and the last subtraction in double; only the order of
 * its double sum differs from a whole-row evaluation, so a value is never more than 1 float ulp from the rule above and equals it
 * bit for bit in at least 999 of 1000 cases.
 *   records   a record is the picked token's lp and, for top_n > 0, top_n ids with their lp.  mc_batch_step / _generate,
 *             mc_ragged_step / _generate: token i of row r has its record in slot [i][r], where its token is in tokens_out.  A row
 *             that picks a stop id has that token's record; behind it, and for an idle row, the slots hold the fill: NaN bits
 *             (0xFFFFFFFF) and id -1.  mc_rows_prefill / mc_extend_rows: n = 1, the one pick of each row in the call.
 *             mc_verify_rows / mc_tree_verify: one record per packed row, for picks[m] -- every accepted token and the bonus token
 *             is one of them -- under Part 2m's settings too.
 *   launches  two per pick launch sequence, directly behind it: mc_logprob_parts_* over (chunks of 2048 logits, rows) and
 *             mc_logprob_finish_* with one workgroup per row; no atomics and no in-launch hand-offs.  With the switch off (the
 *             default) a batch launches, uploads and allocates exactly what it did before; the buffers are reserved at the first
 *             call with the switch on.
 *   the rows  a row's records do not depend on B, on its index, or on the other rows and their settings.
 * The switch belongs to the batch: mc_batch_fork, imports and the resets of Parts 2k / 2l leave it alone.
 * Not covered: the batch-1 decoder, prompt ("echo") log-probabilities of fed tokens, the sampler's truncated distribution, draft
 * probabilities.  The verify calls' getter is mc_logprobs_get_verify: it carries this part's prefix (Part 2f's test pins the set
 * of names that begin with the verify calls' prefix).
 * ------------------------------------------------------------------------------------------ */
#define MC_LOGPROBS_MAX_TOP 20 /* the largest `top_logprobs` any public API takes */
/* enable 0 (default) / 1, and the top_n of the records from the next call on; setting it drops the records of earlier calls.
 * Refused with MC_ERR_INVALID_ARGUMENT, texts prefixed "mc_logprobs_set: ": a null batch, "enable must be 0 or 1", "top_n must lie
 * in [0, 20]", "top_n (N) is above the vocabulary (V)"; nothing changes then. */
mc_status mc_logprobs_set(mc_batch* b, int32_t enable, int32_t top_n);
int32_t mc_logprobs_enabled(const mc_batch* b, int32_t* top_n); /* 0 for a null batch; top_n may be null */
/* the records of the last step, generate or packed call: token_logprobs [n][B], top_ids and top_logprobs [n][B][top_n].  n must
 * be that call's n (1 for a step or a packed pass).  The top arrays may be null, and must be null when top_n == 0.  Refused
 * (MC_ERR_INVALID_ARGUMENT, "mc_logprobs_get: ") while the switch is off, before any such call, and with another n. */
mc_status mc_logprobs_get(mc_batch* b, int32_t n, float* token_logprobs, int32_t* top_ids, float* top_logprobs);
/* the records of the last mc_verify_rows / mc_tree_verify call, packed like its tokens (as mc_verify_get_logits packs the logits):
 * pick_logprobs [M], top_ids and top_logprobs [M][top_n].  The same refusals, prefixed "mc_logprobs_get_verify: ". */
mc_status mc_logprobs_get_verify(mc_batch* b, float* pick_logprobs, int32_t* top_ids, float* top_logprobs);

/* Host-side helpers shared by tests and the synthetic initialiser. */
/* value in [-7,7] (bits = 4) or [-127,127] (bits = 8), zero mean, of element (row, col) of matrix `matrix_id` */
int32_t mc_synth_weight(uint64_t seed, uint32_t matrix_id, uint32_t row, uint32_t col, int32_t bits);
/* scale of (row, group) : U(0.5,1.5) / (sqrt(in) * 2^(bits-1)) as float */
float mc_synth_scale(uint64_t seed, uint32_t matrix_id, uint32_t row, uint32_t group,
                     int32_t in_features, int32_t bits);
/* T-typed synthetic values before rounding to T.  kind 0: U(0.5,1.5) (norm weights);
 * kind 1: ~N(0,1)*0.02 (embedding rows); kind 2: U(-1,1)/sqrt(n) (plain T linear weights, n = in) */
float mc_synth_value(uint64_t seed, uint32_t matrix_id, uint32_t index, int32_t kind, uint32_t n);
/* Matrix ids of mc_decoder_init_synthetic: layer*16 + {0 wq, 1 wk, 2 wv, 3 wo, 4 w1, 5 w2, 6 w3,
 * 8 attention_norm, 9 ffn_norm, 10 q_norm, 11 k_norm, 12 attention_post_norm, 13 ffn_post_norm};
 * 0xFFFF0000 + {0 tok_embeddings, 1 output, 2 norm}. */

/* ================================================================================================
 * Part 3 -- model files: the data format on the caller side of the decode path.
 *
 *   safetensor_document / sharded_safetensor_document
 *                                   include/metalchat/safetensor.h:534-1030, src/safetensor.cc
 *   checkpoint adaptors             include/metalchat/huggingface/llama.h:85-171,
 *                                   include/metalchat/huggingface/gemma.h:56-84,
 *                                   include/metalchat/reference.h:35-90
 *   option serializers              src/llama.cc:41-55, src/reference.cc:52-66, src/gemma.cc:20-42
 *
 * A document is an ordered list of named tensors over memory-mapped files (host memory; nothing
 * here touches the GPU until mc_decoder_load_document).  Errors follow the reference: a corrupt or
 * unreadable file is MC_ERR_RUNTIME ("safetensor_document: header is corrupted, ..."), a missing
 * name MC_ERR_INVALID_ARGUMENT.
 * ============================================================================================== */
typedef struct mc_document mc_document;

typedef struct mc_tensor_info {
    const char* name;   /* owned by the document */
    const char* dtype;  /* safetensors spelling: "BF16", "F32", "I8", "I32", ... */
    int32_t ndim;
    int64_t shape[8];
    const void* data;   /* host pointer into the mapped file (or the document's own copy) */
    size_t nbytes;
} mc_tensor_info;

enum {
    MC_CKPT_META_LLAMA3 = 0,       /* reference::llama3_safetensor_serializer (Meta names, wq/wk permuted) */
    MC_CKPT_HF_LLAMA3 = 1,         /* huggingface::llama3_safetensor_serializer (model.layers.N.self_attn...) */
    MC_CKPT_META_LLAMA3_QLORA = 2, /* huggingface::llama3_qlora_safetensor_serializer (int8-held int4 + adaptors) */
    MC_CKPT_HF_GEMMA3 = 3          /* huggingface::gemma3_safetensor_serializer */
};

mc_status mc_document_create(mc_document** out);                         /* safetensor_document() */
mc_status mc_document_open(const char* path, mc_document** out);         /* ::open(path) -- src/safetensor.cc:118-136 */
mc_status mc_document_open_sharded(const char* index_json_path, mc_document** out); /* sharded_...::open */
void mc_document_release(mc_document* d);
int32_t mc_document_size(const mc_document* d);                          /* std::distance(begin(), end()) */
/* Entries in document order (a file's tensors by ascending data offset, src/safetensor.cc:111-115). */
mc_status mc_document_tensor(const mc_document* d, int32_t index, mc_tensor_info* out);
mc_status mc_document_find(const mc_document* d, const char* name, mc_tensor_info* out);
/* insert(name, tensor): the bytes are copied.  src/safetensor.cc:182-200 */
mc_status mc_document_insert(mc_document* d, const char* name, const char* dtype, int32_t ndim,
                             const int64_t* shape, const void* data);
/* insert(name, source): a second name for the same storage.  src/safetensor.cc:203-212 */
mc_status mc_document_link(mc_document* d, const char* name, const char* source);
mc_status mc_document_set_metadata(mc_document* d, const char* key, const char* value);
const char* mc_document_metadata(const mc_document* d, const char* key); /* NULL when absent */
/* serializer.adapt(document): rename to the reference's parameter paths and link
 * "output.weight" to "tok_embeddings.weight" (tied head). */
mc_status mc_document_adapt(mc_document* d, int32_t flavour);
mc_status mc_document_save(const mc_document* d, const char* path);      /* src/safetensor.cc:264-290 */

/* options_serializer::load: fills family, head geometry, layer count, rope / norm constants,
 * attn_scale and max_seq_len (1024, as every reference serializer does) from config.json /
 * params.json text; dim / ffn_dim / vocab when the JSON carries them.  Other fields are left as
 * the caller set them. */
mc_status mc_config_from_json(const char* json_text, int32_t flavour, mc_decoder_config* cfg);
/* Widths the reference takes from the tensors themselves: vocab, dim, ffn_dim, group_size, and
 * n_layers / layer_end when still 0.  Call on an adapted document. */
mc_status mc_config_from_document(const mc_document* d, mc_decoder_config* cfg);
/* serializer.load(document): hands every tensor of the layers this decoder owns to
 * mc_decoder_load_linear / _vector / _lora (BF16 <-> F32 converted to the decoder's T). */
mc_status mc_decoder_load_document(mc_decoder* d, const mc_document* doc, int32_t flavour);
mc_status mc_decoder_get_config(const mc_decoder* d, mc_decoder_config* out);

/* ================================================================================================
 * Part 4 -- text in, text out: the callers either side of the token loop.
 *
 *   text::gpt2_codec                include/metalchat/text/gpt.h, src/gpt.cc:20-100
 *   text::byte_pair_encoder<char>   include/metalchat/text/bpe.h:82-345 (tiktoken token map)
 *   text::regexp / regexp_iterator  include/metalchat/text/regexp.h:24-92, src/regexp.cc:34-178 (PCRE2)
 *   reference::llama3_tokenizer_loader   include/metalchat/reference.h:117-165, src/reference.cc:76-127
 *   huggingface llama3_tokenizer_loader  src/llama.cc:81-112 (tokenizer.json)
 *   token scanners, interpreter     include/metalchat/interpreter.h:60-175,296-374, src/interpreter.cc:84-136
 *
 * Host code, no GPU work of its own; the interpreter drives mc_decoder_prefill / mc_decoder_step.
 * The reference's behaviour is kept where it is peculiar, because token ids are the contract:
 *   - the split pattern is compiled by PCRE2 with NO options (src/regexp.cc:38-41): the subject is
 *     bytes, \p{L} / \p{N} see Latin-1 code points, \s is the C-locale set;
 *   - a piece is cut at the PREVIOUS match end with the length of the new match (src/regexp.cc:146-155);
 *   - a piece that is not a token is merged by visiting segments in rank order and joining a segment
 *     with its right neighbour whenever the concatenation is a token; the LAST byte of the piece never
 *     gets a segment of its own and is dropped unless a merge absorbs it (bpe.h:120-168);
 *   - gpt2_codec::decode keeps the low byte of a code point that is not in its table (src/gpt.cc:92-96).
 * One deviation: a pattern that matches the empty string makes the reference loop forever; here it
 * is MC_ERR_RUNTIME "regexp_iterator: empty match".
 * The regular expressions run on the system's libpcre2-8.so.0 (the engine the reference links),
 * opened at first use; without it mc_tokenizer_* fail with MC_ERR_RUNTIME.
 * ============================================================================================== */
typedef struct mc_tokenizer mc_tokenizer;
typedef struct mc_interpreter mc_interpreter;

/* text::token kinds -- include/metalchat/text/tokenizer.h:27-38 */
enum {
    MC_TOKEN_REGULAR = 1 << 0,
    MC_TOKEN_BEGIN_TEXT = 1 << 1,
    MC_TOKEN_END_TEXT = 1 << 2,
    MC_TOKEN_RESERVED = 1 << 3,
    MC_TOKEN_FINETUNE_RIGHT_PAD = 1 << 4,
    MC_TOKEN_BEGIN_HEADER = 1 << 5,
    MC_TOKEN_END_HEADER = 1 << 6,
    MC_TOKEN_END_MESSAGE = 1 << 7,
    MC_TOKEN_END_TURN = 1 << 8,
    MC_TOKEN_IPYTHON = 1 << 9
};

/* Output convention of the byte / id producers below: up to `cap` elements are written, *n always
 * receives the full count (call again with a larger buffer when *n > cap). */

/* gpt2_codec::encode / decode: bytes <-> the printable code points of GPT-2's byte alphabet, UTF-8.
 * decode of malformed UTF-8 or of a code point above U+FFFF: MC_ERR_RUNTIME (std::range_error in the
 * reference's std::wstring_convert). */
mc_status mc_gpt2_encode(const char* bytes, size_t len, char* out, size_t cap, size_t* n);
mc_status mc_gpt2_decode(const char* utf8, size_t len, char* out, size_t cap, size_t* n);

/* The split pattern on its own (text::regexp::begin .. end): piece i occupies
 * [offsets[2i], offsets[2i+1]) of the subject, cut the way the reference's iterator cuts it. */
mc_status mc_regexp_split(const char* pattern, const char* subject, size_t len, size_t* offsets,
                          size_t cap_pairs, size_t* n_pairs);

/* byte_pair_encoder(token_regex): an empty encoder.  token_regex == NULL: the llama3 pattern
 * (reference::llama3_tokenizer_loader::default_regex). */
mc_status mc_tokenizer_create(const char* token_regex, mc_tokenizer** out);
/* reference::llama3_tokenizer_loader::load(path[, regex]): "base64 rank" lines (tiktoken), then the
 * eleven llama3 control tokens at the ids that follow (128000 .. 128010 for the published model). */
mc_status mc_tokenizer_open_tiktoken(const char* path, const char* token_regex, mc_tokenizer** out);
/* huggingface llama3_tokenizer_loader::load(path): tokenizer.json -- the Split pattern of the
 * pre_tokenizer Sequence, model.vocab with GPT-2-coded keys, then the same control tokens. */
mc_status mc_tokenizer_open_hf(const char* tokenizer_json_path, mc_tokenizer** out);
/* text::sentence_piece (include/metalchat/text/sentence_piece.h:17-104): byte-pair merging over the CODE POINTS of the whole
 * text, spaces as U+2581 on the way in and back on the way out.  _create_sentence_piece: an empty one;
 * _open_hf_gemma3: huggingface::gemma3_tokenizer_loader::load (src/gemma.cc:72-94) -- tokenizer.json's model.vocab as
 * spelled, then added_tokens, each bound to a token kind equal to its id.  One difference, where the reference does not
 * return: its ".*" stops at a line feed and its iterator then never advances; here a line is a piece and every line feed a
 * piece of its own. */
mc_status mc_tokenizer_create_sentence_piece(mc_tokenizer** out);
mc_status mc_tokenizer_open_hf_gemma3(const char* tokenizer_json_path, mc_tokenizer** out);
void mc_tokenizer_release(mc_tokenizer* t);
mc_status mc_tokenizer_insert(mc_tokenizer* t, const char* bytes, size_t len, int32_t id, int32_t kind);
mc_status mc_tokenizer_insert_back(mc_tokenizer* t, const char* bytes, size_t len, int32_t kind);
size_t mc_tokenizer_size(const mc_tokenizer* t);
/* encode(string): split, look every piece up, merge the ones that are not tokens. */
mc_status mc_tokenizer_encode(const mc_tokenizer* t, const char* text, size_t len, int32_t* ids,
                              size_t cap, size_t* n);
/* encode(tokenkind): MC_ERR_INVALID_ARGUMENT "byte_pair_encoder: unknown control token '<kind>'" */
mc_status mc_tokenizer_encode_control(const mc_tokenizer* t, int32_t kind, int32_t* id);
/* decode(id): MC_ERR_RUNTIME "byte_pair_encoder: unable to decode id '<id>'" */
mc_status mc_tokenizer_decode(const mc_tokenizer* t, const int32_t* ids, size_t n_ids, char* out,
                              size_t cap, size_t* n);

/* interpreter(transformer, tokenizer): the buffer starts with begin_text, the scanner is
 * limit_token_scanner(50), start_pos 0.  The decoder must own every layer (single stage); its sampler
 * is whatever mc_decoder_set_sampler selected.  Neither handle is owned.  d == NULL gives an interpreter
 * that frames messages (write / pending) but cannot read. */
mc_status mc_interpreter_create(mc_decoder* d, const mc_tokenizer* t, mc_interpreter** out);
void mc_interpreter_release(mc_interpreter* it);
/* set_token_scanner(composite_token_scanner<Op>{limit_token_scanner(limit), match_token_scanner(stop_ids)}):
 * generation continues while op(limit.scan(tok), match.scan(tok)) holds -- op_and != 0:
 * std::logical_and (stop at a stop id OR at the limit, the reference's test set-up), 0: std::logical_or.
 * limit == 0: no limit scanner; n_stop == 0: no match scanner; neither: the empty composite, which
 * stops at once (interpreter.h:148-152). */
mc_status mc_interpreter_set_scanner(mc_interpreter* it, size_t limit, const int32_t* stop_ids,
                                     size_t n_stop, int32_t op_and);
/* declare_variable: "{{ name }}" in later message contents is replaced by value (the reference
 * renders contents with mustache; sections, commands and tool dispatch are not provided). */
mc_status mc_interpreter_declare_variable(mc_interpreter* it, const char* name, const char* value);
/* write(basic_message(role, content)): header, content, end_turn appended to the token buffer. */
mc_status mc_interpreter_write(mc_interpreter* it, const char* role, const char* content);
/* read(): assistant header, flush the buffer through the prompt pass, then one token per step until
 * the scanner says stop; the decoded text goes to out, the ids (optionally) to ids.  sliding_window
 * as for mc_decoder_prefill. */
mc_status mc_interpreter_read(mc_interpreter* it, int32_t sliding_window, char* out, size_t cap, size_t* n,
                              int32_t* ids, size_t ids_cap, size_t* n_ids);
size_t mc_interpreter_start_pos(const mc_interpreter* it);
/* the token buffer that the next read() will flush (for tests) */
mc_status mc_interpreter_pending(const mc_interpreter* it, int32_t* ids, size_t cap, size_t* n);

#ifdef __cplusplus
}
#endif
#endif
