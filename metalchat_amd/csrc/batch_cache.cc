// A batch row's cache (the map of the whole: batch_impl.h): fork from the decoder's cache or from another row, import from and export to the host
// (the lockstep view and, Part 2j, a rolled row's own), and the rolling switch.
#include "batch_impl.h"

using namespace mcimpl;

namespace {

// the first n cache positions of every kv head, one layer: K [kv][pos][hd] is n * hd elements per kv head, Vt [kv * hd][pos] n elements per row
mc_status
copy_cache_rows(mc_batch* b, void* k_dst, void* vt_dst, const void* k_src, const void* vt_src, int n)
{
    const mc_decoder_config& c = b->p.cfg;
    const int KV = c.n_kv_heads, hd = c.head_dim, S = c.max_seq_len;
    MC_HIP(hipMemcpy2DAsync(k_dst, (size_t)S * hd * 2, k_src, (size_t)S * hd * 2, (size_t)n * hd * 2, KV, hipMemcpyDeviceToDevice, b->p.stream));
    MC_HIP(hipMemcpy2DAsync(vt_dst, (size_t)S * 2, vt_src, (size_t)S * 2, (size_t)n * 2, (size_t)KV * hd, hipMemcpyDeviceToDevice, b->p.stream));
    return MC_OK;
}

// mc_batch_export_kv and mc_ragged_export_kv: row `row`'s cache of `layer` through mc_kv_export_bfloat, which takes kv_len (and
// the ring) from the device step state `state`, into staging buffers of `cap` positions; then n positions to the host.
// n < 0: n = that kv_len, read back behind the launch and reported in *n_out.
mc_status
export_kv(mc_batch* b, const char* what, int32_t row, int32_t layer, const step_state* state, int32_t cap, int32_t n, int32_t* n_out,
          void* keys, void* values)
{
    const mc_decoder_config& c = b->p.cfg;
    const size_t per_pos = (size_t)c.n_kv_heads * c.head_dim * 2;
    device_tmp kt, vtmp;
    hipError_t e = kt.alloc(cap * per_pos);
    if (e == hipSuccess) e = vtmp.alloc(cap * per_pos);
    if (e != hipSuccess) return hip_fail(e, what);
    mc_status s = b->launch("mc_kv_export_bfloat", 512, 1, 1, 256, 0,
                            pack((const void*)b->kc_of(layer, row), (const void*)b->vt_of(layer, row), kt.ptr, vtmp.ptr, (const void*)state,
                                 (uint32_t)c.n_kv_heads, (uint32_t)c.head_dim, (uint32_t)c.max_seq_len, (uint32_t)b->p.pre_len));
    e = hipStreamSynchronize(b->p.stream);
    if (s == MC_OK && e == hipSuccess && n < 0) {
        step_state st{};
        e = hipMemcpy(&st, state, sizeof st, hipMemcpyDeviceToHost);
        n = st.kv_len;
        if (n_out) *n_out = n;
    }
    if (s == MC_OK && e == hipSuccess && keys) e = hipMemcpy(keys, kt.ptr, n * per_pos, hipMemcpyDeviceToHost);
    if (s == MC_OK && e == hipSuccess && values) e = hipMemcpy(values, vtmp.ptr, n * per_pos, hipMemcpyDeviceToHost);
    if (e != hipSuccess) return hip_fail(e, what);
    return s;
}

// mc_ragged_export_kv (and mc_batch_export_kv for a row that has rolled): row `row`'s own logical view, min(length, max_seq_len)
// positions -- the sink rows, then the ring unrolled.  The export kernel reads kv_len and the ring from a state of its own, made
// from the row's length: the row last wrote position length - 1, which fixes its ring (mc_b_rows_begin_rolling)
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
    return export_kv(b, what, row, layer, static_cast<const step_state*>(stv.ptr), n, n, nullptr, keys, values);
}

} // namespace

extern "C" {

mc_status
mc_batch_fork(mc_batch* b, int32_t row, int32_t n_valid)
{
    mc_status s = find_row(b, "mc_batch_fork", row, true, 0);
    if (s != MC_OK) return s;
    const mc_decoder_config& c = b->p.cfg;
    if (n_valid < 1 || n_valid > c.max_seq_len) return fail(MC_ERR_INVALID_ARGUMENT, "mc_batch_fork: n_valid must lie in [1, max_seq_len]");
    int kv_len = 0;
    bool rolled = false;
    if ((s = decoder_cache_state(b->d, &kv_len, &rolled)) != MC_OK) return s;
    if (rolled) return fail(MC_ERR_INVALID_ARGUMENT, "mc_batch_fork: the decoder's cache has rolled (sink ring turned)");
    if (n_valid > kv_len) return fail(MC_ERR_INVALID_ARGUMENT, "mc_batch_fork: the decoder's cache holds fewer than n_valid positions");
    MC_HIP(hipSetDevice(b->p.ordinal));
    for (size_t l = 0; l < b->p.layers.size(); l++)
        if ((s = copy_cache_rows(b, b->kc_of((int)l, row), b->vt_of((int)l, row), b->p.layers[l].kc, b->p.layers[l].vt, n_valid)) != MC_OK) return s;
    if ((s = b->set_pos(n_valid - 1)) != MC_OK) return s;
    MC_HIP(hipStreamSynchronize(b->p.stream));
    b->lengths[row] = n_valid;
    return MC_OK;
}

mc_status
mc_batch_import_kv(mc_batch* b, int32_t row, int32_t layer, const void* keys, const void* values, int32_t n_valid)
{
    mc_status s = find_row(b, "mc_batch_import_kv", row, true, layer);
    if (s != MC_OK) return s;
    if (!keys || !values) return fail(MC_ERR_INVALID_ARGUMENT, "mc_batch_import_kv: null argument");
    const mc_decoder_config& c = b->p.cfg;
    if (n_valid < 1 || n_valid > c.max_seq_len)
        return fail(MC_ERR_INVALID_ARGUMENT, "mc_batch_import_kv: n_valid must lie in [1, max_seq_len]");
    MC_HIP(hipSetDevice(b->p.ordinal));
    const size_t nb = (size_t)n_valid * c.n_kv_heads * c.head_dim * 2;
    device_tmp kt, vtmp;
    MC_HIP(kt.alloc(nb));
    hipError_t e = vtmp.alloc(nb);
    if (e == hipSuccess) e = hipMemcpy(kt.ptr, keys, nb, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(vtmp.ptr, values, nb, hipMemcpyHostToDevice);
    if (e == hipSuccess) {
        s = b->launch("mc_kv_import_bfloat", 512, 1, 1, 256, 0,
                      pack((void*)b->kc_of(layer, row), (void*)b->vt_of(layer, row), (const void*)kt.ptr, (const void*)vtmp.ptr,
                           (uint32_t)n_valid, (uint32_t)c.n_kv_heads, (uint32_t)c.head_dim, (uint32_t)c.max_seq_len));
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
    // the physical slots as they lie: a rolled row's ring follows from its length, which the copy takes along
    const int n = std::min(b->lengths[src], b->p.cfg.max_seq_len);
    MC_HIP(hipSetDevice(b->p.ordinal));
    for (int l = 0; n > 0 && l < (int)b->p.layers.size(); l++)
        if (mc_status s = copy_cache_rows(b, b->kc_of(l, dst), b->vt_of(l, dst), b->kc_of(l, src), b->vt_of(l, src), n); s != MC_OK) return s;
    MC_HIP(hipStreamSynchronize(b->p.stream));
    b->lengths[dst] = b->lengths[src];
    return MC_OK;
}

} // extern "C"
