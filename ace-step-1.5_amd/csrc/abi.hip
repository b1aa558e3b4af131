// abi.hip — the parts of the C ABI (include/acehip.h) that belong to no model handle: the
// library's version and per-thread error state, and the stand-alone kernel entry points the
// tests and micro-benchmarks call (acehip_gemm_*, acehip_rmsnorm_bf16, acehip_attention_*,
// acehip_cross_attn_bf16, acehip_sampler_*).  The entries own their scratch memory: one buffer
// per kind and device (abi_buf), allocated on first use.
#include <map>
#include <mutex>
#include <string>
#include <utility>

#include "layer_args.h"
#include "../../include/acehip.h"

using namespace acehip;

namespace {

thread_local std::string g_err;

// Scratch of the stand-alone entries, one buffer per (kind, device) for the life of the process,
// grown on demand.  The attention workspace is zeroed once, when it is allocated (it holds
// self-resetting counters); the others are written before they are read.
enum AbiBuf { ABI_GEMM_WS, ABI_CROSS_Q, ABI_ATTN_WS };
void *abi_buf(AbiBuf kind, size_t bytes) {
    static std::mutex mu;
    static std::map<int, std::pair<void *, size_t>> by_dev[3];
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return nullptr;
    std::lock_guard<std::mutex> lk(mu);
    auto &e = by_dev[kind][dev];
    if (e.second < bytes) {
        if (e.first) {
            (void)hipDeviceSynchronize();
            (void)hipFree(e.first);
        }
        e = {nullptr, 0};
        if (hipMalloc(&e.first, bytes) != hipSuccess) return nullptr;
        if (kind == ABI_ATTN_WS && hipMemset(e.first, 0, bytes) != hipSuccess) {
            (void)hipFree(e.first);
            e.first = nullptr;
            return nullptr;
        }
        e.second = bytes;
    }
    return e.first;
}

// the split-K workspace of the production dispatch (small grids)
void use_abi_gemm_ws(GemmArgs &g) {
    g.ws = abi_buf(ABI_GEMM_WS, GEMM_WS_BYTES);
    g.ws_bytes = g.ws ? GEMM_WS_BYTES : 0;
}

int sampler_dtype(int dtype, bool *f32) {
    if (dtype != ACEHIP_BF16 && dtype != ACEHIP_F32) return fail(ACEHIP_E_ARG, "sampler: dtype");
    *f32 = dtype == ACEHIP_F32;
    return 0;
}

// residual-epilogue GemmArgs of acehip_gemm_res_bf16 / acehip_gemm_res_norm_bf16 (gate == null: EPI_RES)
int res_gemm_args(GemmArgs &g, const void *A, int lda, const void *W, int ldw, void *C, int ldc, int M, int N, int K,
                  const void *res, int ldr, const void *gate, int64_t gate_bstride, int rows_per_batch) {
    if (!A || !W || !C || !res) return fail(ACEHIP_E_ARG, "gemm_res: null argument");
    if (M <= 0 || N % 128 || K % 64 || K <= 0) return fail(ACEHIP_E_ARG, "gemm_res: shape");
    if ((lda | ldw | ldc | ldr) % 8 || lda < K || ldw < K || ldc < N || ldr < N)
        return fail(ACEHIP_E_ARG, "gemm_res: leading dimensions");
    if (gate && (rows_per_batch <= 0 || gate_bstride % 8)) return fail(ACEHIP_E_ARG, "gemm_res: gate");
    g.A = (const bf16_t *)A; g.lda = lda; g.W = (const bf16_t *)W; g.ldw = ldw;
    g.C = (bf16_t *)C; g.ldc = ldc; g.M = M; g.N = N; g.K = K;
    g.res = (const bf16_t *)res; g.ldr = ldr;
    g.epi = gate ? EPI_GATED_RES : EPI_RES;
    g.gate = (const bf16_t *)gate; g.gate_bstride = gate_bstride; g.rows_per_batch = gate ? rows_per_batch : 0;
    return 0;
}

}  // namespace

namespace acehip {
void set_error(const std::string &msg) { g_err = msg; }
int fail(int code, const std::string &msg) {
    g_err = msg;
    return code;
}
}  // namespace acehip

extern "C" {

int acehip_get_version(void) { return ACEHIP_VERSION; }
const char *acehip_last_error(void) { return g_err.c_str(); }

int acehip_sampler_apg_euler(const void *vt, void *xt, void *ra, int B, int T, int C, float guidance,
                             float dt, int apply_cfg, int first_step, int out_mode, int dtype, void *stream) {
    if (!vt || !xt || (apply_cfg > 0 && !ra)) return fail(ACEHIP_E_ARG, "null argument");
    bool f32;
    if (int rc = sampler_dtype(dtype, &f32)) return rc;
    return apg_euler(vt, xt, ra, B, T, C, guidance, dt, apply_cfg, first_step, out_mode, f32, (hipStream_t)stream);
}

int acehip_sampler_adg_euler(const void *vt, void *xt, int B, int T, int C, float guidance, float sigma,
                             float dt, int out_mode, int dtype, void *stream) {
    if (!vt || !xt) return fail(ACEHIP_E_ARG, "null argument");
    bool f32;
    if (int rc = sampler_dtype(dtype, &f32)) return rc;
    return adg_euler(vt, xt, B, T, C, guidance, sigma, dt, out_mode, f32, (hipStream_t)stream);
}

int acehip_sampler_axpy(const void *vt, void *xt, int64_t n, float s, int dtype, void *stream) {
    if (!vt || !xt) return fail(ACEHIP_E_ARG, "null argument");
    bool f32;
    if (int rc = sampler_dtype(dtype, &f32)) return rc;
    return axpy(vt, xt, n, s, f32, (hipStream_t)stream);
}

int acehip_gemm_bf16(const void *A, int lda, const void *W, int ldw, void *C, int ldc, int M, int N,
                     int K, const void *bias, void *stream) {
    GemmArgs g{};
    g.A = (const bf16_t *)A; g.lda = lda; g.W = (const bf16_t *)W; g.ldw = ldw;
    g.C = (bf16_t *)C; g.ldc = ldc; g.M = M; g.N = N; g.K = K; g.epi = EPI_STORE;
    g.bias = (const bf16_t *)bias;
    return gemm(g, (hipStream_t)stream);
}

int acehip_gemm_bf16_ex(const void *A, int lda, const void *W, int ldw, void *C, int ldc, int M, int N,
                        int K, const void *bias, int epi, int variant, void *stream) {
    GemmArgs g{};
    g.A = (const bf16_t *)A; g.lda = lda; g.W = (const bf16_t *)W; g.ldw = ldw;
    g.C = (bf16_t *)C; g.ldc = ldc; g.M = M; g.N = N; g.K = K;
    g.bias = (const bf16_t *)bias;
    if (epi == 2) { g.epi = EPI_RES; g.res = (const bf16_t *)C; g.ldr = ldc; }
    else if (epi == 3) g.epi = EPI_SWIGLU;   // W rows packed [32 gate; 32 up] per 64-row panel, C[M][N/2]
    else if (epi == 0) g.epi = EPI_STORE;
    else return fail(ACEHIP_E_ARG, "gemm_ex: epilogue");
    if (M <= 0 || N % 128 || K % 64) return fail(ACEHIP_E_ARG, "gemm_ex: shape");
    if (variant < 0) {   // production dispatch (split-K for small grids)
        use_abi_gemm_ws(g);
        return gemm(g, (hipStream_t)stream);
    }
    return gemm_variant(g, variant, (hipStream_t)stream);
}

int acehip_gemm_res_bf16(const void *A, int lda, const void *W, int ldw, void *C, int ldc, int M, int N, int K,
                         const void *res, int ldr, const void *gate, int64_t gate_bstride, int rows_per_batch,
                         int variant, void *stream) {
    GemmArgs g{};
    if (int rc = res_gemm_args(g, A, lda, W, ldw, C, ldc, M, N, K, res, ldr, gate, gate_bstride, rows_per_batch))
        return rc;
    if (variant < 0) {   // production dispatch (split-K for small grids)
        use_abi_gemm_ws(g);
        return gemm(g, (hipStream_t)stream);
    }
    return gemm_variant(g, variant, (hipStream_t)stream);
}

int acehip_gemm_res_norm_bf16(const void *A, int lda, const void *W, int ldw, void *X, int M, int D, int K,
                              const void *gate, int64_t gate_bstride, int rows_per_batch, int defer,
                              const void *w, const void *shift, const void *scale, int64_t mod_bstride, void *out,
                              int M_norm, float eps, const void *v, int from, int *deferred, void *stream) {
    if (!w || !out || !deferred) return fail(ACEHIP_E_ARG, "gemm_res_norm: null argument");
    if (M_norm < M || (v && (from < M || from > M_norm))) return fail(ACEHIP_E_ARG, "gemm_res_norm: rows");
    // what rmsnorm_mod would refuse, before the GEMM has written X
    if (D % 256 || D > 4096) return fail(ACEHIP_E_ARG, "gemm_res_norm: D must be a multiple of 256, <= 4096");
    if ((shift == nullptr) != (scale == nullptr)) return fail(ACEHIP_E_ARG, "gemm_res_norm: shift/scale");
    if ((gate || scale) && rows_per_batch <= 0) return fail(ACEHIP_E_ARG, "gemm_res_norm: rows_per_batch");
    *deferred = 0;
    GemmArgs g{};
    if (int rc = res_gemm_args(g, A, lda, W, ldw, X, D, M, D, K, X, D, gate, gate_bstride, rows_per_batch)) return rc;
    use_abi_gemm_ws(g);
    RowAdd ra{};
    if (int rc = gemm(g, (hipStream_t)stream, defer ? &ra : nullptr)) return rc;
    *deferred = ra.part != nullptr;
    if (v) {
        ra.xw = (bf16_t *)X;
        ra.v = (const bf16_t *)v;
        ra.from = from;
    }
    return rmsnorm_mod((const bf16_t *)X, (const bf16_t *)w, (const bf16_t *)shift, (const bf16_t *)scale,
                       mod_bstride, rows_per_batch, (bf16_t *)out, M_norm, D, eps, (hipStream_t)stream, ra);
}

int acehip_rmsnorm_bf16(const void *x, const void *w, const void *shift, const void *scale,
                        int64_t mod_bstride, int rows_per_batch, void *out, int M, int D, float eps,
                        int rows_per_wave, void *stream) {
    if (!x || !w || !out) return fail(ACEHIP_E_ARG, "null argument");
    if (rows_per_wave == 3 || rows_per_wave > 4 || (rows_per_wave < 0 && rows_per_wave != -2 && rows_per_wave != -4))
        return fail(ACEHIP_E_ARG, "rows_per_wave");
    return rmsnorm_mod((const bf16_t *)x, (const bf16_t *)w, (const bf16_t *)shift, (const bf16_t *)scale,
                       mod_bstride, rows_per_batch, (bf16_t *)out, M, D, eps, (hipStream_t)stream, RowAdd{},
                       rows_per_wave);
}

int acehip_gemm_headpost_bf16(const void *A, int lda, const void *W, int K, int B, int S, int nq, int nk,
                              int nv, const void *qw, const void *kw, const void *cos, const void *sin,
                              float eps, void *q, void *k, void *v, void *stream) {
    if (!A || !W) return fail(ACEHIP_E_ARG, "null argument");
    if ((nq && !q) || (nk && !k) || (nv && !v)) return fail(ACEHIP_E_ARG, "missing head output");
    if (B * S <= 0 || K % 64 || K <= 0) return fail(ACEHIP_E_ARG, "gemm_headpost: shape");
    GemmArgs g = lin_headpost((const bf16_t *)A, lda, (const bf16_t *)W, K, B, S, nq, nk, nv, (const bf16_t *)qw,
                              (const bf16_t *)kw, (const bf16_t *)cos, (const bf16_t *)sin, eps,
                              HeadDst{(bf16_t *)q, (bf16_t *)k, (bf16_t *)v, S, 0});
    use_abi_gemm_ws(g);
    return gemm(g, (hipStream_t)stream);
}

int acehip_cross_attn_bf16(const void *xn, const void *wq, const void *qnw, const void *k, const void *v, void *ao,
                           int B, int S, int H, int KV, int Lenc, int D, float eps, float scale, int force,
                           int *path, void *stream) {
    if (!xn || !wq || !qnw || !k || !v || !ao || !path) return fail(ACEHIP_E_ARG, "cross_attn: null argument");
    if (B <= 0 || S <= 0 || H <= 0 || KV <= 0 || Lenc <= 0 || D <= 0 || D % 64 || H % 2 || (int64_t)B * S > INT32_MAX)
        return fail(ACEHIP_E_ARG, "cross_attn: shape");
    if (force < -1 || force > 1) return fail(ACEHIP_E_ARG, "cross_attn: force must be -1, 0 or 1");
    *path = -1;
    hipStream_t s = (hipStream_t)stream;
    GemmArgs cq = lin_headpost((const bf16_t *)xn, D, (const bf16_t *)wq, D, B, S, H, 0, 0, (const bf16_t *)qnw, nullptr,
                               nullptr, nullptr, eps, HeadDst{nullptr, nullptr, nullptr, S, 0});
    use_abi_gemm_ws(cq);
    const int64_t qd = (int64_t)H * 128;
    const bool shape = cross_fuse_shape(cq, KV, Lenc);
    const bool planned = shape && cross_fuse_planned(cq) && attention_whole_units(B, H, KV, S, Lenc, true);
    // force = 1: fused wherever the kernel can run the shape; 0: the two launches it fuses
    // (variant 13 + whole units on attn_fwd_kernel); −1: the DiT forward's own choice
    const bool fused = shape && (force == 1 || (force < 0 && planned && knobs().cross_fuse));
    if (fused) {
        *path = 1;
        return cross_q_attention(cq, (const bf16_t *)k, (const bf16_t *)v, (bf16_t *)ao, KV, Lenc, scale, qd, s);
    }
    *path = 0;
    cq.hp.q = (bf16_t *)abi_buf(ABI_CROSS_Q, (size_t)B * S * qd * sizeof(bf16_t));   // the two-launch path's Q
    if (!cq.hp.q) return fail(ACEHIP_E_OOM, "cross_attn: Q scratch");
    if (force == 0 || planned) {
        if (H != 2 * KV) return fail(ACEHIP_E_ARG, "cross_attn: the forced two-launch path needs H = 2 KV");
        if (int rc = gemm_variant(cq, 13, s)) return rc;
        return attention_fwd_units(cq.hp.q, (const bf16_t *)k, (const bf16_t *)v, (bf16_t *)ao, B, H, KV, S, Lenc,
                                   scale, qd, s);
    }
    if (int rc = gemm(cq, s)) return rc;
    return acehip_attention_bf16(cq.hp.q, k, v, ao, B, H, KV, S, Lenc, -1, scale, stream);
}

int acehip_attention_bf16(const void *q, const void *k, const void *v, void *o, int B, int H, int KV,
                          int Sq, int Sk, int window, float scale, void *stream) {
    return acehip_attention_masked_bf16(q, k, v, o, B, H, KV, Sq, Sk, window, scale, nullptr, stream);
}

int acehip_attention_probs_bf16(const void *q, const void *k, int B, int H, int KV, int Sq, int Sk, const int *heads,
                                int n, int k0, int k1, float scale, float *out, void *stream) {
    if (!q || !k || !heads || !out) return fail(ACEHIP_E_ARG, "attention_probs: null argument");
    if (n < 1 || n > 64) return fail(ACEHIP_E_ARG, "attention_probs: n must be in [1, 64]");
    AttnProbsSel sel;
    sel.n = n;
    for (int i = 0; i < n; ++i) {
        if (heads[i] < 0 || heads[i] >= H) return fail(ACEHIP_E_ARG, "attention_probs: head index out of range");
        sel.head[i] = (int16_t)heads[i];
        sel.slot[i] = (int16_t)i;
    }
    return attention_probs((const bf16_t *)q, (const bf16_t *)k, B, H, KV, Sq, Sk, sel, k0, k1, scale, out,
                           (hipStream_t)stream);
}

int acehip_attention_masked_bf16(const void *q, const void *k, const void *v, void *o, int B, int H, int KV,
                                 int Sq, int Sk, int window, float scale, const uint8_t *kmask, void *stream) {
    // the tail-split workspace of the stand-alone entry (the runtimes own theirs, allocated at create)
    int dev = 0;
    HIP_TRY(hipGetDevice(&dev));   // reported as the HIP error it is, not as a failed allocation
    void *ws = abi_buf(ABI_ATTN_WS, attention_ws_bytes());
    if (!ws) return fail(ACEHIP_E_OOM, "attention workspace");
    return attention((const bf16_t *)q, (const bf16_t *)k, (const bf16_t *)v, (bf16_t *)o, B, H, KV, Sq,
                     Sk, window, scale, (int64_t)H * 128, ws, (hipStream_t)stream, kmask);
}

}  // extern "C"
