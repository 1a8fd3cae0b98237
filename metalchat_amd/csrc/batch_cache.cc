// A batch row's cache (the map of the whole: batch_impl.h): fork from the decoder's cache or from another row, import from and export to the host
// (the lockstep view and, Part 2j, a rolled row's own), and the rolling switch.
#include "batch_impl.h"

using namespace mcimpl;

namespace {

// the cache positions [first, n) of every kv head, one layer: K [kv][pos][hd] is hd elements a position per kv head, Vt [kv * hd][pos] one per row
mc_status
copy_cache_rows(mc_batch* b, void* k_dst, void* vt_dst, const void* k_src, const void* vt_src, int n, int first = 0)
{
    const mc_decoder_config& c = b->p.cfg;
    const int KV = c.n_kv_heads, hd = c.head_dim, S = c.max_seq_len;
    if (n <= first) return MC_OK;
    const size_t ko = (size_t)first * hd * 2, vo = (size_t)first * 2, w = (size_t)(n - first);
    MC_HIP(hipMemcpy2DAsync((char*)k_dst + ko, (size_t)S * hd * 2, (const char*)k_src + ko, (size_t)S * hd * 2, w * hd * 2, KV, hipMemcpyDeviceToDevice, b->p.stream));
    MC_HIP(hipMemcpy2DAsync((char*)vt_dst + vo, (size_t)S * 2, (const char*)vt_src + vo, (size_t)S * 2, w * 2, (size_t)KV * hd, hipMemcpyDeviceToDevice, b->p.stream));
    return MC_OK;
}

// Part 2o: the four planes of one layer of an fp8 cache -- a row's, or (Part 2s) the shared prefix's
struct kv8_planes {
    char *k, *v;
    int8_t *kx, *vx;
};
kv8_planes
row_planes(const mc_batch* b, int layer, int row)
{
    return {b->kc_of(layer, row), b->vt_of(layer, row), b->kexp_of(layer, row), b->vexp_of(layer, row)};
}
kv8_planes
prefix_planes(const mc_batch* b, int layer)
{
    return {b->pkc_of(layer), b->pvt_of(layer), b->pkexp_of(layer), b->pvexp_of(layer)};
}

// Part 2o: the positions [first, n) of the planes `dst` from the planes `src`, byte for byte
mc_status
copy_cache_rows_f8(mc_batch* b, const kv8_planes& dst, const kv8_planes& src, int n, int first = 0)
{
    const mc_decoder_config& c = b->p.cfg;
    const size_t KV = c.n_kv_heads, hd = c.head_dim, S = c.max_seq_len, o = (size_t)first;
    if (n <= first) return MC_OK;
    const size_t w = (size_t)(n - first);
    MC_HIP(hipMemcpy2DAsync(dst.k + o * hd, S * hd, src.k + o * hd, S * hd, w * hd, KV, hipMemcpyDeviceToDevice, b->p.stream));
    MC_HIP(hipMemcpy2DAsync(dst.v + o, S, src.v + o, S, w, KV * hd, hipMemcpyDeviceToDevice, b->p.stream));
    MC_HIP(hipMemcpy2DAsync(dst.kx + o, S, src.kx + o, S, w, KV, hipMemcpyDeviceToDevice, b->p.stream));
    MC_HIP(hipMemcpy2DAsync(dst.vx + o, S, src.vx + o, S, w, KV, hipMemcpyDeviceToDevice, b->p.stream));
    return MC_OK;
}

// Part 2o: bfloat16 K [kv][src_seq][hd] and Vt [kv * hd][src_seq], positions [0, n), quantised into the planes `dst` (mc_kv_quant_f8)
mc_status
quant_cache_rows(mc_batch* b, const kv8_planes& dst, const void* k_src, const void* vt_src, int src_seq, int n)
{
    const mc_decoder_config& c = b->p.cfg;
    return b->launch("mc_kv_quant_f8", (unsigned)(n + 63) / 64, (unsigned)c.n_kv_heads, 1, 256, 0,
                     pack(k_src, vt_src, (uint32_t)src_seq, (void*)dst.k, (void*)dst.v, dst.kx, dst.vx, (uint32_t)n, (uint32_t)c.head_dim, (uint32_t)c.max_seq_len));
}

// mc_prefix_attach and mc_prefix_detach: the prefix's positions [first, n) of one layer into row `row` -- the two bfloat16 planes, or (Part 2s)
// the four fp8 planes byte for byte: nothing is quantised again
mc_status
prefix_to_row(mc_batch* b, int layer, int row, int n, int first = 0)
{
    if (b->fp8()) return copy_cache_rows_f8(b, row_planes(b, layer, row), prefix_planes(b, layer), n, first);
    return copy_cache_rows(b, b->kc_of(layer, row), b->vt_of(layer, row), b->pkc_of(layer), b->pvt_of(layer), n, first);
}

// mc_batch_export_kv and mc_ragged_export_kv: row `row`'s cache of `layer` through mc_kv_export_bfloat, which takes kv_len (and
// the ring) from the device step state `state`, into staging buffers of `cap` positions; then n positions to the host.
// n < 0: n = that kv_len, read back behind the launch and reported in *n_out.  An fp8 cache (Part 2o) goes through mc_kv_dequant_f8: the same
// view, the values deq of the row's bytes.  prefix (Part 2r; Part 2s: all four planes): the shared prefix's planes in place of the row's;
// skip: only positions [skip, n) reach the host, at their place in keys / values.
mc_status
export_kv(mc_batch* b, const char* what, int32_t row, int32_t layer, const step_state* state, int32_t cap, int32_t n, int32_t* n_out,
          void* keys, void* values, bool prefix = false, int32_t skip = 0)
{
    const mc_decoder_config& c = b->p.cfg;
    const size_t per_pos = (size_t)c.n_kv_heads * c.head_dim * 2;
    device_tmp kt, vtmp;
    hipError_t e = kt.alloc(cap * per_pos);
    if (e == hipSuccess) e = vtmp.alloc(cap * per_pos);
    if (e != hipSuccess) return hip_fail(e, what);
    arg_pack args = prefix ? pack((const void*)b->pkc_of(layer), (const void*)b->pvt_of(layer)) : pack((const void*)b->kc_of(layer, row), (const void*)b->vt_of(layer, row));
    if (b->fp8()) {
        args.push((const void*)(prefix ? b->pkexp_of(layer) : b->kexp_of(layer, row)));
        args.push((const void*)(prefix ? b->pvexp_of(layer) : b->vexp_of(layer, row)));
    }
    for (const void* a : {(const void*)kt.ptr, (const void*)vtmp.ptr, (const void*)state}) args.push(a);
    for (uint32_t w : {(uint32_t)c.n_kv_heads, (uint32_t)c.head_dim, (uint32_t)c.max_seq_len, (uint32_t)b->p.pre_len}) args.push(w);
    mc_status s = b->launch(b->fp8() ? "mc_kv_dequant_f8" : "mc_kv_export_bfloat", 512, 1, 1, 256, 0, std::move(args));
    e = hipStreamSynchronize(b->p.stream);
    if (s == MC_OK && e == hipSuccess && n < 0) {
        step_state st{};
        e = hipMemcpy(&st, state, sizeof st, hipMemcpyDeviceToHost);
        n = st.kv_len;
        if (n_out) *n_out = n;
    }
    const size_t so = skip * per_pos;
    if (s == MC_OK && e == hipSuccess && keys) e = hipMemcpy((char*)keys + so, (const char*)kt.ptr + so, (n - skip) * per_pos, hipMemcpyDeviceToHost);
    if (s == MC_OK && e == hipSuccess && values) e = hipMemcpy((char*)values + so, (const char*)vtmp.ptr + so, (n - skip) * per_pos, hipMemcpyDeviceToHost);
    if (e != hipSuccess) return hip_fail(e, what);
    return s;
}

// mc_ragged_export_kv (and mc_batch_export_kv for a row that has rolled): row `row`'s own logical view, min(length, max_seq_len)
// positions -- the sink rows, then the ring unrolled.  The export kernel reads kv_len and the ring from a state of its own, made
// from the row's length: the row last wrote position length - 1, which fixes its ring (mc_b_rows_begin_rolling).  An attached row (Part 2r):
// the prefix's [0, shared), then the row's own slots
mc_status
export_row(mc_batch* b, const char* what, int32_t row, int32_t layer, void* keys, void* values, int32_t* n_valid)
{
    const int32_t len = b->lengths[row], S = b->p.cfg.max_seq_len, n = std::min(len, S);
    if (n_valid) *n_valid = n;
    if (n == 0) return MC_OK;
    MC_HIP(hipSetDevice(b->p.ordinal));
    step_state st{};
    st.kv_len = n;
    st.ring_base = len > S ? (len - S) % (S - b->p.pre_len) : 0;
    device_tmp stv;
    hipError_t e = stv.alloc(sizeof st);
    if (e == hipSuccess) e = hipMemcpyAsync(stv.ptr, &st, sizeof st, hipMemcpyHostToDevice, b->p.stream);
    if (e != hipSuccess) return hip_fail(e, what);
    const step_state* state = static_cast<const step_state*>(stv.ptr);
    if (!b->attached[row]) return export_kv(b, what, row, layer, state, n, n, nullptr, keys, values);
    const int32_t shared = b->prefix_shared(); // (n >= shared; the export kernel writes n positions of staging either way)
    const mc_status s = shared ? export_kv(b, what, row, layer, state, n, shared, nullptr, keys, values, true) : MC_OK;
    return s != MC_OK ? s : export_kv(b, what, row, layer, state, n, n, nullptr, keys, values, false, shared);
}

// mc_prefix_fork / mc_prefix_import_kv in front of their copies: the refusals, then the planes (zeroed, so finite behind n_valid)
mc_status
prefix_begin(mc_batch* b, const char* who, int32_t n_valid)
{
    mc_status s = refuse(prefix_fill_refusal(who, b->kv_format, b->rolling, b->attached, b->kv_prefix_on));
    if (s != MC_OK) return s;
    if (n_valid < 1 || n_valid > b->p.cfg.max_seq_len) return fail(MC_ERR_INVALID_ARGUMENT, std::string(who) + ": n_valid must lie in [1, max_seq_len]");
    const size_t bytes = b->p.layers.size() * b->cache_elems * b->kv_elem(), exp_bytes = b->p.layers.size() * b->exp_elems();
    if ((s = b->ensure(b->pkc, bytes)) != MC_OK || (s = b->ensure(b->pvt, bytes)) != MC_OK) return s;
    if (b->fp8() && ((s = b->ensure(b->pkexp, exp_bytes)) != MC_OK || (s = b->ensure(b->pvexp, exp_bytes)) != MC_OK)) return s;
    return b->ensure(b->sp_dev, sizeof(int32_t) * b->B);
}

} // namespace

extern "C" {

mc_status
mc_batch_fork(mc_batch* b, int32_t row, int32_t n_valid)
{
    mc_status s = find_row(b, "mc_batch_fork", row, true, 0);
    if (s == MC_OK) s = refuse(attached_row_refusal("mc_batch_fork", b->attached, row));
    if (s != MC_OK) return s;
    const mc_decoder_config& c = b->p.cfg;
    if (n_valid < 1 || n_valid > c.max_seq_len) return fail(MC_ERR_INVALID_ARGUMENT, "mc_batch_fork: n_valid must lie in [1, max_seq_len]");
    int kv_len = 0;
    bool rolled = false;
    if ((s = decoder_cache_state(b->d, &kv_len, &rolled)) != MC_OK) return s;
    if (rolled) return fail(MC_ERR_INVALID_ARGUMENT, "mc_batch_fork: the decoder's cache has rolled (sink ring turned)");
    if (n_valid > kv_len) return fail(MC_ERR_INVALID_ARGUMENT, "mc_batch_fork: the decoder's cache holds fewer than n_valid positions");
    MC_HIP(hipSetDevice(b->p.ordinal));
    for (size_t l = 0; l < b->p.layers.size(); l++) { // (an fp8 cache: a quantising copy)
        s = b->fp8() ? quant_cache_rows(b, row_planes(b, (int)l, row), b->p.layers[l].kc, b->p.layers[l].vt, c.max_seq_len, n_valid)
                     : copy_cache_rows(b, b->kc_of((int)l, row), b->vt_of((int)l, row), b->p.layers[l].kc, b->p.layers[l].vt, n_valid);
        if (s != MC_OK) return s;
    }
    if ((s = b->set_pos(n_valid - 1)) != MC_OK) return s;
    MC_HIP(hipStreamSynchronize(b->p.stream));
    b->lengths[row] = n_valid;
    return MC_OK;
}

mc_status
mc_batch_import_kv(mc_batch* b, int32_t row, int32_t layer, const void* keys, const void* values, int32_t n_valid)
{
    mc_status s = find_row(b, "mc_batch_import_kv", row, true, layer);
    if (s == MC_OK) s = refuse(attached_row_refusal("mc_batch_import_kv", b->attached, row));
    if (s != MC_OK) return s;
    if (!keys || !values) return fail(MC_ERR_INVALID_ARGUMENT, "mc_batch_import_kv: null argument");
    const mc_decoder_config& c = b->p.cfg;
    if (n_valid < 1 || n_valid > c.max_seq_len)
        return fail(MC_ERR_INVALID_ARGUMENT, "mc_batch_import_kv: n_valid must lie in [1, max_seq_len]");
    MC_HIP(hipSetDevice(b->p.ordinal));
    const size_t nb = (size_t)n_valid * c.n_kv_heads * c.head_dim * 2;
    // an fp8 cache: the import kernel fills a bfloat16 cache of exactly n_valid slots (K [kv][n][hd], Vt [kv * hd][n]), which is then quantised
    device_tmp kt, vtmp, kstage, vstage;
    MC_HIP(kt.alloc(nb));
    hipError_t e = vtmp.alloc(nb);
    if (e == hipSuccess && b->fp8()) e = kstage.alloc(nb);
    if (e == hipSuccess && b->fp8()) e = vstage.alloc(nb);
    if (e == hipSuccess) e = hipMemcpy(kt.ptr, keys, nb, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(vtmp.ptr, values, nb, hipMemcpyHostToDevice);
    if (e == hipSuccess) {
        void* k_dst = b->fp8() ? kstage.ptr : (void*)b->kc_of(layer, row);
        void* vt_dst = b->fp8() ? vstage.ptr : (void*)b->vt_of(layer, row);
        s = b->launch("mc_kv_import_bfloat", 512, 1, 1, 256, 0,
                      pack(k_dst, vt_dst, (const void*)kt.ptr, (const void*)vtmp.ptr, (uint32_t)n_valid, (uint32_t)c.n_kv_heads, (uint32_t)c.head_dim,
                           (uint32_t)(b->fp8() ? n_valid : c.max_seq_len)));
        if (s == MC_OK && b->fp8()) s = quant_cache_rows(b, row_planes(b, layer, row), kstage.ptr, vstage.ptr, n_valid, n_valid);
        if (s == MC_OK) s = b->set_pos(n_valid - 1);
        e = hipStreamSynchronize(b->p.stream);
    }
    if (e != hipSuccess) return hip_fail(e, "mc_batch_import_kv");
    if (s == MC_OK) b->lengths[row] = n_valid;
    return s;
}

mc_status
mc_batch_export_kv(mc_batch* b, int32_t row, int32_t layer, void* keys, void* values, int32_t* n_valid)
{
    mc_status s = find_row(b, "mc_batch_export_kv", row, true, layer);
    if (s == MC_OK) s = refuse(attached_row_refusal("mc_batch_export_kv", b->attached, row));
    if (s != MC_OK) return s;
    // a row that has rolled has no lockstep view: its own (Part 2j)
    if (b->lengths[row] > b->p.cfg.max_seq_len) return export_row(b, "mc_batch_export_kv", row, layer, keys, values, n_valid);
    MC_HIP(hipSetDevice(b->p.ordinal));
    // kv_len of the batch's shared state: the position of the last lockstep step, fork or import, whichever row that was for
    return export_kv(b, "mc_batch_export_kv", row, layer, b->st, b->p.cfg.max_seq_len, -1, n_valid, keys, values);
}

mc_status
mc_ragged_export_kv(mc_batch* b, int32_t row, int32_t layer, void* keys, void* values, int32_t* n_valid)
{
    mc_status s = find_row(b, "mc_ragged_export_kv", row, true, layer);
    if (s != MC_OK) return s;
    return export_row(b, "mc_ragged_export_kv", row, layer, keys, values, n_valid);
}

// ---- Part 2j: rolling rows ----

mc_status
mc_rolling_set(mc_batch* b, int32_t enable)
{
    if (!b) return fail(MC_ERR_INVALID_ARGUMENT, "mc_rolling_set: null argument");
    if (enable != 0 && enable != 1) return fail(MC_ERR_INVALID_ARGUMENT, "mc_rolling_set: enable must be 0 or 1");
    if (enable == 1 && b->prefix_n > 0) return fail(MC_ERR_INVALID_ARGUMENT, "mc_rolling_set: the batch holds a shared prefix (a shared prefix does not roll)");
    b->rolling = enable == 1;
    return MC_OK;
}

int32_t
mc_rolling_enabled(const mc_batch* b)
{
    return b && b->rolling ? 1 : 0;
}

mc_status
mc_rolling_fork_row(mc_batch* b, int32_t dst, int32_t src)
{
    if (!b) return fail(MC_ERR_INVALID_ARGUMENT, "mc_rolling_fork_row: null argument");
    if (dst < 0 || dst >= b->B || src < 0 || src >= b->B) return fail(MC_ERR_INVALID_ARGUMENT, "mc_rolling_fork_row: row out of range");
    if (dst == src) return fail(MC_ERR_INVALID_ARGUMENT, "mc_rolling_fork_row: dst and src are the same row");
    for (int32_t r : {dst, src})
        if (const mc_status s = refuse(attached_row_refusal("mc_rolling_fork_row", b->attached, r)); s != MC_OK) return s;
    // the physical slots as they lie: a rolled row's ring follows from its length, which the copy takes along
    const int n = std::min(b->lengths[src], b->p.cfg.max_seq_len);
    MC_HIP(hipSetDevice(b->p.ordinal));
    for (int l = 0; n > 0 && l < (int)b->p.layers.size(); l++) {
        const mc_status s = b->fp8() ? copy_cache_rows_f8(b, row_planes(b, l, dst), row_planes(b, l, src), n) : copy_cache_rows(b, b->kc_of(l, dst), b->vt_of(l, dst), b->kc_of(l, src), b->vt_of(l, src), n);
        if (s != MC_OK) return s;
    }
    MC_HIP(hipStreamSynchronize(b->p.stream));
    b->lengths[dst] = b->lengths[src];
    return MC_OK;
}

// ---- Part 2r: shared-prefix rows ----

mc_status
mc_prefix_fork(mc_batch* b, int32_t n_valid)
{
    if (!b) return fail(MC_ERR_INVALID_ARGUMENT, "mc_prefix_fork: null argument");
    mc_status s = prefix_begin(b, "mc_prefix_fork", n_valid);
    if (s != MC_OK) return s;
    int kv_len = 0;
    bool rolled = false;
    if ((s = decoder_cache_state(b->d, &kv_len, &rolled)) != MC_OK) return s;
    if (rolled) return fail(MC_ERR_INVALID_ARGUMENT, "mc_prefix_fork: the decoder's cache has rolled (sink ring turned)");
    if (n_valid > kv_len) return fail(MC_ERR_INVALID_ARGUMENT, "mc_prefix_fork: the decoder's cache holds fewer than n_valid positions");
    MC_HIP(hipSetDevice(b->p.ordinal));
    for (size_t l = 0; l < b->p.layers.size(); l++) { // (an fp8 prefix: a quantising copy, as mc_batch_fork's)
        s = b->fp8() ? quant_cache_rows(b, prefix_planes(b, (int)l), b->p.layers[l].kc, b->p.layers[l].vt, b->p.cfg.max_seq_len, n_valid)
                     : copy_cache_rows(b, b->pkc_of((int)l), b->pvt_of((int)l), b->p.layers[l].kc, b->p.layers[l].vt, n_valid);
        if (s != MC_OK) return s;
    }
    MC_HIP(hipStreamSynchronize(b->p.stream));
    b->prefix_n = n_valid;
    return MC_OK;
}

mc_status
mc_prefix_import_kv(mc_batch* b, int32_t layer, const void* keys, const void* values, int32_t n_valid)
{
    if (!b || !keys || !values) return fail(MC_ERR_INVALID_ARGUMENT, "mc_prefix_import_kv: null argument");
    if (layer < 0 || layer >= (int32_t)b->p.layers.size()) return fail(MC_ERR_INVALID_ARGUMENT, "mc_prefix_import_kv: layer out of range");
    mc_status s = prefix_begin(b, "mc_prefix_import_kv", n_valid);
    if (s != MC_OK) return s;
    const mc_decoder_config& c = b->p.cfg;
    MC_HIP(hipSetDevice(b->p.ordinal));
    const size_t nb = (size_t)n_valid * c.n_kv_heads * c.head_dim * 2;
    // an fp8 prefix: staged as a bfloat16 cache of exactly n_valid slots and then quantised, as mc_batch_import_kv does
    device_tmp kt, vtmp, kstage, vstage;
    MC_HIP(kt.alloc(nb));
    hipError_t e = vtmp.alloc(nb);
    if (e == hipSuccess && b->fp8()) e = kstage.alloc(nb);
    if (e == hipSuccess && b->fp8()) e = vstage.alloc(nb);
    if (e == hipSuccess) e = hipMemcpy(kt.ptr, keys, nb, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(vtmp.ptr, values, nb, hipMemcpyHostToDevice);
    if (e == hipSuccess) {
        void* k_dst = b->fp8() ? kstage.ptr : (void*)b->pkc_of(layer);
        void* vt_dst = b->fp8() ? vstage.ptr : (void*)b->pvt_of(layer);
        s = b->launch("mc_kv_import_bfloat", 512, 1, 1, 256, 0,
                      pack(k_dst, vt_dst, (const void*)kt.ptr, (const void*)vtmp.ptr, (uint32_t)n_valid, (uint32_t)c.n_kv_heads, (uint32_t)c.head_dim,
                           (uint32_t)(b->fp8() ? n_valid : c.max_seq_len)));
        if (s == MC_OK && b->fp8()) s = quant_cache_rows(b, prefix_planes(b, layer), kstage.ptr, vstage.ptr, n_valid, n_valid);
        e = hipStreamSynchronize(b->p.stream);
    }
    if (e != hipSuccess) return hip_fail(e, "mc_prefix_import_kv");
    if (s == MC_OK) b->prefix_n = n_valid;
    return s;
}

mc_status
mc_prefix_attach(mc_batch* b, int32_t row)
{
    mc_status s = find_row(b, "mc_prefix_attach", row);
    if (s != MC_OK) return s;
    if (b->prefix_n == 0) return fail(MC_ERR_INVALID_ARGUMENT, "mc_prefix_attach: the batch holds no shared prefix (mc_prefix_fork or mc_prefix_import_kv first)");
    if (b->attached[row]) return fail(MC_ERR_INVALID_ARGUMENT, "mc_prefix_attach: row " + std::to_string(row) + " is already attached");
    MC_HIP(hipSetDevice(b->p.ordinal));
    // the prefix's tail [shared, n_valid) becomes the row's own, at the same slots; [0, shared) of the row is not touched
    for (int l = 0; l < (int)b->p.layers.size(); l++)
        if ((s = prefix_to_row(b, l, row, b->prefix_n, b->prefix_shared())) != MC_OK) return s;
    MC_HIP(hipStreamSynchronize(b->p.stream));
    b->attached[row] = 1;
    b->lengths[row] = b->prefix_n;
    return MC_OK;
}

mc_status
mc_prefix_detach(mc_batch* b, int32_t row, int32_t materialise)
{
    mc_status s = find_row(b, "mc_prefix_detach", row);
    if (s != MC_OK) return s;
    if (materialise != 0 && materialise != 1) return fail(MC_ERR_INVALID_ARGUMENT, "mc_prefix_detach: materialise must be 0 or 1");
    if (!b->attached[row]) return fail(MC_ERR_INVALID_ARGUMENT, "mc_prefix_detach: row " + std::to_string(row) + " is not attached");
    MC_HIP(hipSetDevice(b->p.ordinal));
    for (int l = 0; materialise && l < (int)b->p.layers.size(); l++)
        if ((s = prefix_to_row(b, l, row, b->prefix_shared())) != MC_OK) return s;
    MC_HIP(hipStreamSynchronize(b->p.stream));
    b->attached[row] = 0;
    if (!materialise) b->lengths[row] = 0;
    return MC_OK;
}

mc_status
mc_prefix_info(const mc_batch* b, int32_t* n_valid, int32_t* shared)
{
    if (!b) return fail(MC_ERR_INVALID_ARGUMENT, "mc_prefix_info: null argument");
    if (n_valid) *n_valid = b->prefix_n;
    if (shared) *shared = b->prefix_shared();
    return MC_OK;
}

int32_t
mc_prefix_attached(const mc_batch* b, int32_t row)
{
    return b && row >= 0 && row < b->B && b->attached[row] ? 1 : 0;
}

// ---- Part 2s: shared-prefix rows on an fp8 batch ----

mc_status
mc_kv_prefix_set(mc_batch* b, int32_t on)
{
    if (!b) return fail(MC_ERR_INVALID_ARGUMENT, "mc_kv_prefix_set: null argument");
    if (on != 0 && on != 1) return fail(MC_ERR_INVALID_ARGUMENT, "mc_kv_prefix_set: on must be 0 or 1");
    if (on == 0 && b->fp8() && b->prefix_n > 0)
        return fail(MC_ERR_INVALID_ARGUMENT, "mc_kv_prefix_set: the batch holds a shared prefix (the switch stays on while it does)");
    b->kv_prefix_on = on == 1;
    return MC_OK;
}

int32_t
mc_kv_prefix_enabled(const mc_batch* b)
{
    return b && b->kv_prefix_on ? 1 : 0;
}

// ---- Part 2t: chunks and verify calls on attached rows (the admission and the launches: batch_rows.cc rows_pass) ----

mc_status
mc_attached_packed_set(mc_batch* b, int32_t on)
{
    if (!b) return fail(MC_ERR_INVALID_ARGUMENT, "mc_attached_packed_set: null argument");
    if (mc_status s = refuse(attached_packed_switch_refusal(b->kv_format, on, b->kv_prefix_on, b->kv_packed_on)); s != MC_OK) return s;
    b->attached_packed_on = on == 1;
    return MC_OK;
}

int32_t
mc_attached_packed_enabled(const mc_batch* b)
{
    return b && b->attached_packed_on ? 1 : 0;
}

} // extern "C"
