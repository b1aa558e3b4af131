// layer_args.h — host pieces the DiT and encoder runtimes (dit.hip, encoder.hip) and the
// stand-alone entries (abi.hip) share: the GemmArgs of a transformer layer's Linear shapes, the
// GEMM call through a handle's split-K workspace and the RoPE tables.  Weight loading: weights.h.
#pragma once
#include <algorithm>
#include <cmath>
#include <vector>

#include "kernels.h"

namespace acehip {

// ---- GemmArgs of the recurring Linear shapes: W is the nn.Linear weight [N][K], contiguous;
// every field a builder does not name stays zero
// C = bf16(A·Wᵀ + bias); bias may be null
inline GemmArgs lin_store(const bf16_t *A, int64_t lda, const bf16_t *W, bf16_t *C, int64_t ldc, int M, int N, int K,
                          const bf16_t *bias = nullptr) {
    GemmArgs g{};
    g.A = A; g.lda = lda; g.W = W; g.ldw = K; g.C = C; g.ldc = ldc;
    g.M = M; g.N = N; g.K = K; g.epi = EPI_STORE; g.bias = bias;
    return g;
}
// X = bf16(X + bf16(A·Wᵀ)), X [M][ld] both residual and output
inline GemmArgs lin_res(const bf16_t *A, int64_t lda, const bf16_t *W, bf16_t *X, int64_t ld, int M, int N, int K) {
    GemmArgs g = lin_store(A, lda, W, X, ld, M, N, K);
    g.epi = EPI_RES; g.res = X; g.ldr = ld;
    return g;
}
// X = bf16(X + bf16(bf16(A·Wᵀ)·gate[row / rows_per_batch])) (AdaLN-Zero), gate rows gate_bstride apart
inline GemmArgs lin_gated_res(const bf16_t *A, int64_t lda, const bf16_t *W, bf16_t *X, int64_t ld, int M, int N, int K,
                              const bf16_t *gate, int64_t gate_bstride, int rows_per_batch) {
    GemmArgs g = lin_res(A, lda, W, X, ld, M, N, K);
    g.epi = EPI_GATED_RES; g.gate = gate; g.gate_bstride = gate_bstride; g.rows_per_batch = rows_per_batch;
    return g;
}
// C [M][F] = silu(A·Wgᵀ)·(A·Wuᵀ), W the gate/up panels of pack_gate_up ([2F][K])
inline GemmArgs lin_swiglu(const bf16_t *A, int64_t lda, const bf16_t *W, bf16_t *C, int F, int M, int K) {
    GemmArgs g = lin_store(A, lda, W, C, F, M, 2 * F, K);
    g.epi = EPI_SWIGLU;
    return g;
}
// where a head-post projection scatters its heads: q / k / v [B][heads][S_dst][128]; S_dst_q: rows
// per head of q where they differ from k / v's (0: S_dst; see HeadPostArgs)
struct HeadDst {
    bf16_t *q, *k, *v;
    int S_dst, S_dst_q;
};
// the q|k|v projection of B·S rows (W [(nq + nk + nv)·128][K]) with q / k RMSNorm (qw, kw), RoPE
// (cos / sin rows of the first position, or null) and the head-major scatter in the epilogue
inline GemmArgs lin_headpost(const bf16_t *A, int64_t lda, const bf16_t *W, int K, int B, int S, int nq, int nk, int nv,
                             const bf16_t *qw, const bf16_t *kw, const bf16_t *cos, const bf16_t *sin, float eps,
                             const HeadDst &d) {
    GemmArgs g{};
    g.A = A; g.lda = lda; g.W = W; g.ldw = K;
    g.M = B * S; g.N = (nq + nk + nv) * 128; g.K = K; g.epi = EPI_HEADPOST;
    g.hp.B = B; g.hp.S = S; g.hp.nq = nq; g.hp.nk = nk; g.hp.nv = nv; g.hp.qw = qw; g.hp.kw = kw;
    g.hp.cos = cos; g.hp.sin = sin;
    g.hp.q = d.q; g.hp.k = d.k; g.hp.v = d.v; g.hp.S_dst = d.S_dst; g.hp.S_dst_q = d.S_dst_q; g.hp.eps = eps;
    return g;
}

// every GEMM of a runtime may use its handle's split-K workspace (small-M grids)
template <class Handle>
inline int hgemm(Handle *h, GemmArgs g, hipStream_t s, RowAdd *defer = nullptr) {
    g.ws = h->gemm_ws;
    g.ws_bytes = h->gemm_ws ? GEMM_WS_BYTES : 0;
    return gemm(g, s, defer);
}

// Qwen3RotaryEmbedding tables cos / sin [max_S][head_dim] in bf16; inv_freq from theta, or the
// caller's fp32 override ([head_dim / 2], the exact reference constant)
inline int build_rope_tables(int head_dim, int max_S, float theta, const std::vector<float> &inv_freq_override,
                             bf16_t *cos_dst, bf16_t *sin_dst) {
    const int hd = head_dim, S = max_S;
    std::vector<float> inv(hd / 2);
    for (int i = 0; i < hd / 2; ++i) {
        const float v = inv_freq_override.empty() ? 1.0f / powf(theta, (float)(2 * i) / (float)hd) : inv_freq_override[i];
        inv[i] = bf2f(f2bf(v));   // model.to(bf16) casts the inv_freq buffer (init_service_loader.py:81-89)
    }
    std::vector<bf16_t> c((size_t)S * hd), s((size_t)S * hd);
    for (int p = 0; p < S; ++p)
        for (int i = 0; i < hd; ++i) {
            const float f = (float)p * inv[i % (hd / 2)];
            c[(size_t)p * hd + i] = f2bf((float)cos((double)f));
            s[(size_t)p * hd + i] = f2bf((float)sin((double)f));
        }
    HIP_TRY(hipMemcpy(cos_dst, c.data(), c.size() * 2, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(sin_dst, s.data(), s.size() * 2, hipMemcpyHostToDevice));
    return 0;
}
}  // namespace acehip
