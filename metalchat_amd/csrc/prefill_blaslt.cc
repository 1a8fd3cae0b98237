// The ROCm library GEMM behind the prompt pass of LONG prompts (gemm_lib below).  A plain bfloat16 GEMM with fp32 sums is what
// hipBLASLt exists for; the hand-written prompt kernels stay for everything the library is not better at (prefill_kernels.hip).

#include "decoder_impl.h"

#include <dlfcn.h>
#include <tuple>
#include <hipblaslt/hipblaslt.h> // types and prototypes only: the library is opened with dlopen when a long prompt first asks for it

using namespace mcimpl;

namespace {

struct blaslt_api {
    void* handle = nullptr;
    bool tried = false, ok = false;
    decltype(&hipblasLtCreate) Create = nullptr;
    decltype(&hipblasLtDestroy) Destroy = nullptr;
    decltype(&hipblasLtMatmulDescCreate) DescCreate = nullptr;
    decltype(&hipblasLtMatmulDescDestroy) DescDestroy = nullptr;
    decltype(&hipblasLtMatmulDescSetAttribute) DescSet = nullptr;
    decltype(&hipblasLtMatrixLayoutCreate) LayoutCreate = nullptr;
    decltype(&hipblasLtMatrixLayoutDestroy) LayoutDestroy = nullptr;
    decltype(&hipblasLtMatmulPreferenceCreate) PrefCreate = nullptr;
    decltype(&hipblasLtMatmulPreferenceDestroy) PrefDestroy = nullptr;
    decltype(&hipblasLtMatmulPreferenceSetAttribute) PrefSet = nullptr;
    decltype(&hipblasLtMatmulAlgoGetHeuristic) Heuristic = nullptr;
    decltype(&hipblasLtMatmul) Matmul = nullptr;
};
blaslt_api&
blaslt()
{
    static blaslt_api api;
    if (api.tried) return api;
    api.tried = true;
    // The copy that sits next to the libamdhip64 THIS library is linked against, first: a process that has also loaded another ROCm
    // stack (the torch wheel carries private copies of libamdhip64 / libhipblaslt: tests/ckptgen.py imports torch) would otherwise get
    // that stack's libhipblaslt by its soname -- a second HIP runtime that knows nothing of this one's streams (found in round 5: the
    // process died in hipblasLtCreate once the library stopped being loaded by the first long prompt of the test session).
    std::vector<std::string> names;
    Dl_info info;
    if (dladdr(reinterpret_cast<void*>(&hipGetDevice), &info) && info.dli_fname) {
        std::string dir(info.dli_fname);
        const size_t slash = dir.rfind('/');
        if (slash != std::string::npos) names.push_back(dir.substr(0, slash) + "/libhipblaslt.so.1");
    }
    for (const char* n : {"/opt/rocm/lib/libhipblaslt.so.1", "libhipblaslt.so.1", "libhipblaslt.so"}) names.push_back(n);
    // RTLD_DEEPBIND: the library's HIP calls bind to ITS OWN dependency chain -- the libamdhip64 of this process's first ROCm stack, found
    // by soname among the loaded objects -- before the global scope, where an `import torch` has put the wheel's private HIP runtime
    // ("no ROCm-capable device is detected" from inside hipblasLtCreate, and an exit(1), otherwise).
    for (const std::string& name : names) {
        api.handle = dlopen(name.c_str(), RTLD_NOW | RTLD_LOCAL | RTLD_DEEPBIND);
        if (api.handle) break;
    }
    if (!api.handle) return api;
    bool all = true;
#define MC_LT_SYM(field, sym) \
    api.field = reinterpret_cast<decltype(api.field)>(dlsym(api.handle, sym)); \
    all = all && api.field != nullptr;
    MC_LT_SYM(Create, "hipblasLtCreate")
    MC_LT_SYM(Destroy, "hipblasLtDestroy")
    MC_LT_SYM(DescCreate, "hipblasLtMatmulDescCreate")
    MC_LT_SYM(DescDestroy, "hipblasLtMatmulDescDestroy")
    MC_LT_SYM(DescSet, "hipblasLtMatmulDescSetAttribute")
    MC_LT_SYM(LayoutCreate, "hipblasLtMatrixLayoutCreate")
    MC_LT_SYM(LayoutDestroy, "hipblasLtMatrixLayoutDestroy")
    MC_LT_SYM(PrefCreate, "hipblasLtMatmulPreferenceCreate")
    MC_LT_SYM(PrefDestroy, "hipblasLtMatmulPreferenceDestroy")
    MC_LT_SYM(PrefSet, "hipblasLtMatmulPreferenceSetAttribute")
    MC_LT_SYM(Heuristic, "hipblasLtMatmulAlgoGetHeuristic")
    MC_LT_SYM(Matmul, "hipblasLtMatmul")
#undef MC_LT_SYM
    api.ok = all;
    return api;
}
// one multiplication shape of gemm_lib: Y[M][N] = X[M][K] Wd[N][K]^T
struct blaslt_plan {
    hipblasLtMatmulDesc_t desc = nullptr;
    hipblasLtMatrixLayout_t a = nullptr, b = nullptr, c = nullptr;
    hipblasLtMatmulHeuristicResult_t algo{};
    bool usable = false, tried = false;
};

} // namespace

// what one decoder holds of the library (mc_decoder::blas), made by its first gemm_lib
struct blaslt_state {
    hipblasLtHandle_t lt = nullptr;
    void* lt_ws = nullptr; // (of the decoder's arena: freed with it)
    static constexpr size_t lt_ws_bytes = 64u << 20;
    std::map<std::tuple<int, int, int, int>, blaslt_plan> lt_plans;
};

void
mcimpl::blaslt_release(blaslt_state* st)
{
    for (auto& kv : st->lt_plans) {
        blaslt_plan& pl = kv.second;
        if (pl.desc) (void)blaslt().DescDestroy(pl.desc);
        for (hipblasLtMatrixLayout_t l : {pl.a, pl.b, pl.c})
            if (l) (void)blaslt().LayoutDestroy(l);
    }
    if (st->lt) (void)blaslt().Destroy(st->lt);
    delete st;
}

// ---- the library GEMM of long prompts (when it is taken, and what was measured: prefill_plan.h lib_ok)
// Y[M][out] (bfloat16, or fp32 when f32_out) = X[M][in] Wd^T on the decoder's stream.  false: the library path is off now
bool
mc_decoder::gemm_lib(const linear_w& L, const void* X, void* Y, int M, bool f32_out)
{
    blaslt_api& api = blaslt();
    auto off = [&](const char* why) {
        pf_lib_on = false;
        if (opt.pf_lib_verbose) fprintf(stderr, "metalchat_hip: hipBLASLt path switched off: %s\n", why);
        return false;
    };
    if (!api.ok) return off("library or symbols not found");
    if (!blas) blas = new blaslt_state();
    if (!blas->lt && api.Create(&blas->lt) != HIPBLAS_STATUS_SUCCESS) {
        blas->lt = nullptr;
        return off("hipblasLtCreate");
    }
    if (!blas->lt_ws && alloc(&blas->lt_ws, blaslt_state::lt_ws_bytes, false) != MC_OK) return off("workspace");
    const void* wd = nullptr;
    if (ensure_wd(L, &wd) != MC_OK) return off("dequantised copy");
    blaslt_plan& pl = blas->lt_plans[std::make_tuple(L.out, L.in, M, f32_out ? 1 : 0)];
    if (!pl.tried) {
        pl.tried = true;
        // row-major Y[M][N] is column-major N x M: Y' = op(A) op(B) with A = Wd ([N][K] row-major = K x N column-major, transposed)
        // and B = X ([M][K] row-major = K x M column-major)
        const hipblasOperation_t ta = HIPBLAS_OP_T, tb_ = HIPBLAS_OP_N;
        bool good = api.DescCreate(&pl.desc, HIPBLAS_COMPUTE_32F, HIP_R_32F) == HIPBLAS_STATUS_SUCCESS;
        good = good && api.DescSet(pl.desc, HIPBLASLT_MATMUL_DESC_TRANSA, &ta, sizeof(ta)) == HIPBLAS_STATUS_SUCCESS;
        good = good && api.DescSet(pl.desc, HIPBLASLT_MATMUL_DESC_TRANSB, &tb_, sizeof(tb_)) == HIPBLAS_STATUS_SUCCESS;
        good = good && api.LayoutCreate(&pl.a, HIP_R_16BF, (uint64_t)L.in, (uint64_t)L.out, (int64_t)L.in) == HIPBLAS_STATUS_SUCCESS;
        good = good && api.LayoutCreate(&pl.b, HIP_R_16BF, (uint64_t)L.in, (uint64_t)M, (int64_t)L.in) == HIPBLAS_STATUS_SUCCESS;
        good = good && api.LayoutCreate(&pl.c, f32_out ? HIP_R_32F : HIP_R_16BF, (uint64_t)L.out, (uint64_t)M, (int64_t)L.out) == HIPBLAS_STATUS_SUCCESS;
        hipblasLtMatmulPreference_t pref = nullptr;
        good = good && api.PrefCreate(&pref) == HIPBLAS_STATUS_SUCCESS;
        const uint64_t wsb = blaslt_state::lt_ws_bytes;
        good = good && api.PrefSet(pref, HIPBLASLT_MATMUL_PREF_MAX_WORKSPACE_BYTES, &wsb, sizeof(wsb)) == HIPBLAS_STATUS_SUCCESS;
        int found = 0;
        constexpr int NCAND = 8;
        hipblasLtMatmulHeuristicResult_t cand[NCAND] = {};
        good = good && api.Heuristic(blas->lt, pl.desc, pl.a, pl.b, pl.c, pl.c, pref, opt.pf_lib_tune ? NCAND : 1, cand, &found) == HIPBLAS_STATUS_SUCCESS && found > 0;
        if (pref) (void)api.PrefDestroy(pref);
        if (good) pl.algo = cand[0];
        if (good && found > 1) {
            // the heuristic's first answer is not always the fastest kernel for a shape: each candidate multiplies THIS call's
            // operands once to warm up and three times between two events (the rows it leaves are the rows any of them leaves
            // up to the order of the fp32 additions; the last run below is the chosen one's)
            hipEvent_t e0 = nullptr, e1 = nullptr;
            if (hipEventCreate(&e0) == hipSuccess && hipEventCreate(&e1) == hipSuccess) {
                const float one = 1.0f, zero = 0.0f;
                float best = 0.0f;
                int best_i = -1;
                for (int i = 0; i < found; i++) {
                    if (cand[i].workspaceSize > blaslt_state::lt_ws_bytes) continue;
                    bool ran = true;
                    for (int r = 0; r < 4 && ran; r++) {
                        if (r == 1) (void)hipEventRecord(e0, stream);
                        ran = api.Matmul(blas->lt, pl.desc, &one, wd, pl.a, X, pl.b, &zero, Y, pl.c, Y, pl.c, &cand[i].algo, blas->lt_ws, blaslt_state::lt_ws_bytes, stream) == HIPBLAS_STATUS_SUCCESS;
                    }
                    float ms = 0.0f;
                    if (!ran || hipEventRecord(e1, stream) != hipSuccess || hipEventSynchronize(e1) != hipSuccess ||
                        hipEventElapsedTime(&ms, e0, e1) != hipSuccess)
                        continue;
                    if (best_i < 0 || ms < best) {
                        best = ms;
                        best_i = i;
                    }
                }
                if (best_i >= 0) pl.algo = cand[best_i];
                if (opt.pf_lib_verbose)
                    fprintf(stderr, "metalchat_hip: hipBLASLt %d x %d x %d%s: candidate %d of %d, %.1f us\n", M, L.out, L.in, f32_out ? " (fp32 rows)" : "",
                            best_i, found, best * 1e3f / 3.0f);
            }
            if (e0) (void)hipEventDestroy(e0);
            if (e1) (void)hipEventDestroy(e1);
        }
        pl.usable = good;
    }
    if (!pl.usable) return off("no algorithm for a shape");
    const float one = 1.0f, zero = 0.0f;
    if (api.Matmul(blas->lt, pl.desc, &one, wd, pl.a, X, pl.b, &zero, Y, pl.c, Y, pl.c, &pl.algo.algo, blas->lt_ws, blaslt_state::lt_ws_bytes, stream) != HIPBLAS_STATUS_SUCCESS)
        return off("hipblasLtMatmul");
    lt_calls++;
    if (log_on) launch_log.push_back("hipblasLtMatmul");
    return true;
}
