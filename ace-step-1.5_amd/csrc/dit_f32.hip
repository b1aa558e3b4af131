// dit_f32.hip — the fp32 parity mode of the DiT runtime (acehip_dit_cfg.fp32 = 1; SURVEY
// §8c(iii)): the reference's fp32 forward (what it runs on a non-cuda device,
// init_service_orchestrator.py:51) with fp32 weights and activations throughout, on the kernels
// of f32.hip.  No algebraic shortcuts (no CFG-row dedup, no closed-form null rows, no graphs).
// It is the oracle the bf16 path is measured against, so it is written for reading, not speed.
// The public entries are in dit.hip; they call the four functions below on a handle created
// with fp32 = 1.
#include "dit_handle.h"

using namespace acehip;

static float *falloc(acehip_dit *h, size_t elems) {
    void *p = nullptr;
    if (hipMalloc(&p, std::max<size_t>(elems, 1) * 4) != hipSuccess) return nullptr;
    h->allocs.push_back(p);
    return (float *)p;
}

int dit_create_f32(acehip_dit *h) {
    const int D = h->D, F = h->F, qd = h->qd, kvd = h->kvd, L = h->L;
    bool ok = true;
    auto A = [&](size_t n) { float *p = falloc(h, n); ok = ok && p; return p; };
    auto &f = h->f;
    f.tables = A((size_t)L * 6 * D);
    f.layers.resize(L);
    for (int i = 0; i < L && ok; ++i) {
        auto &ly = f.layers[i];
        ly.n_sa = A(D); ly.n_ca = A(D); ly.n_mlp = A(D);
        ly.wqkv = A((size_t)(qd + 2 * kvd) * D); ly.wo = A((size_t)D * qd);
        ly.qn = A(128); ly.kn = A(128); ly.cqn = A(128); ly.ckn = A(128);
        ly.wcq = A((size_t)qd * D); ly.wckv = A((size_t)2 * kvd * D); ly.wco = A((size_t)D * qd);
        ly.wg = A((size_t)F * D); ly.wu = A((size_t)F * D); ly.wdown = A((size_t)D * F);
    }
    f.sst_out = A(2 * D); f.win = A((size_t)D * 384); f.bin = A(D);
    f.wce = A((size_t)D * D); f.bce = A(D); f.norm_out = A(D);
    f.wout = A((size_t)128 * D); f.bout = A(128);
    for (int e = 0; e < 2; ++e) {
        f.te_l1[e] = A((size_t)D * 256); f.te_b1[e] = A(D);
        f.te_l2[e] = A((size_t)D * D); f.te_b2[e] = A(D);
        f.te_tp[e] = A((size_t)6 * D * D); f.te_btp[e] = A(6 * D);
    }
    // fp32: gate and up stay the reference's two matrices; each layer owns its cross k|v rows
    if (ok)
        register_dit_weights(h->weights, f, L, D, F, qd, kvd, [](const acehip_dit::F32::Layer &ly) {
            return GateUpDst<float>{ly.wg, Pack::COPY, ly.wu, Pack::COPY};
        });
    const size_t S = h->cfg.max_S, Bc = h->cfg.max_Bc, M = S * Bc, Le = h->cfg.max_Lenc;
    f.X = A(M * D); f.XN = A(M * D); f.QKV = A(M * (qd + 2 * kvd));
    f.Qh = A(M * qd); f.Kh = A(M * kvd); f.Vh = A(M * kvd); f.AO = A(M * qd);
    f.G = A(M * F); f.U = A(M * F); f.Hb = A(M * F); f.Xin = A(M * 384); f.O2 = A(M * 128);
    for (int e = 0; e < 2; ++e) { f.emb[e] = A(Bc * 256); f.temb_e[e] = A(Bc * D); f.proj_e[e] = A(Bc * 6 * D); }
    f.h1 = A(Bc * D); f.temb = A(Bc * D); f.proj = A(Bc * 6 * D);
    f.mod = A((size_t)L * Bc * 6 * D); f.mod_out = A(Bc * 2 * D);
    f.Kc = A((size_t)L * Bc * kvd * Le); f.Vc = A((size_t)L * Bc * kvd * Le);
    f.E = A(Bc * Le * D); f.KVtmp = A(Bc * Le * 2 * kvd);
    f.rope_cos = A(S * 128); f.rope_sin = A(S * 128);
    h->freqs = A(128);
    if (!ok) return fail(ACEHIP_E_OOM, "dit_create (fp32): device allocation failed");
    float fr[128];
    for (int i = 0; i < 128; ++i) fr[i] = expf((-9.210340371976184f * (float)i) / 128.0f);
    HIP_TRY(hipMemcpy(h->freqs, fr, sizeof(fr), hipMemcpyHostToDevice));
    return 0;
}

// Qwen3RotaryEmbedding in fp32: inv_freq stays fp32 (no .to(bf16) in an fp32 model),
// angle = fp32(pos · inv_freq), cos/sin of it
int dit_build_rope_f32(acehip_dit *h) {
    const int hd = h->cfg.head_dim, S = h->cfg.max_S;
    std::vector<float> inv(hd / 2);
    for (int i = 0; i < hd / 2; ++i)
        inv[i] = !h->inv_freq_override.empty() ? h->inv_freq_override[i]
                                               : 1.0f / powf(h->cfg.rope_theta, (float)(2 * i) / (float)hd);
    std::vector<float> c((size_t)S * hd), sn((size_t)S * hd);
    for (int p = 0; p < S; ++p)
        for (int i = 0; i < hd; ++i) {
            const float a = (float)p * inv[i % (hd / 2)];
            c[(size_t)p * hd + i] = (float)cos((double)a);
            sn[(size_t)p * hd + i] = (float)sin((double)a);
        }
    HIP_TRY(hipMemcpy(h->f.rope_cos, c.data(), c.size() * 4, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(h->f.rope_sin, sn.data(), sn.size() * 4, hipMemcpyHostToDevice));
    return 0;
}

int dit_set_condition_f32(acehip_dit *h, const float *enc, int Bc, int Lenc, hipStream_t s) {
    auto &f = h->f;
    const int D = h->D, kvd = h->kvd, M = Bc * Lenc;
    int rc;
    GemmF32Args g{};
    g.A = enc; g.lda = D; g.W = f.wce; g.ldw = D; g.C = f.E; g.ldc = D; g.M = M; g.N = D; g.K = D;
    g.epi = EPI_STORE; g.bias = f.bce;
    if ((rc = gemm_f32(g, s))) return rc;
    const size_t per = (size_t)Bc * kvd * Lenc;
    for (int l = 0; l < h->L; ++l) {
        GemmF32Args k{};
        k.A = f.E; k.lda = D; k.W = f.layers[l].wckv; k.ldw = D; k.C = f.KVtmp; k.ldc = 2 * kvd;
        k.M = M; k.N = 2 * kvd; k.K = D; k.epi = EPI_STORE;
        if ((rc = gemm_f32(k, s))) return rc;
        HeadPostF32Args p{};
        p.src = f.KVtmp; p.ld_src = 2 * kvd; p.B = Bc; p.S = Lenc; p.nq = 0;
        p.nk = h->cfg.kv_heads; p.nv = h->cfg.kv_heads; p.kw = f.layers[l].ckn;
        p.k = f.Kc + l * per; p.v = f.Vc + l * per; p.S_dst = Lenc; p.eps = h->cfg.eps;
        if ((rc = head_post_f32(p, s))) return rc;
    }
    h->have_cond = true;
    h->cond_Bc = Bc;
    h->cond_Lenc = Lenc;
    h->uniform_from = 1 << 30;
    return 0;
}

int dit_forward_f32(acehip_dit *h, const float *xt, const float *ctx, int Bx, const float *t, const float *t_r,
                    int t_stride, int Bc, int T, float *vt_out, hipStream_t s, const acehip_attn_capture *cap) {
    auto &f = h->f;
    const int D = h->D, F = h->F, qd = h->qd, kvd = h->kvd, L = h->L, S = (T + 1) / 2, M = Bc * S;
    const int H = h->cfg.heads, KV = h->cfg.kv_heads, Le = h->cond_Lenc;
    const float eps = h->cfg.eps, scale = 1.0f / sqrtf((float)h->cfg.head_dim);
    const int64_t mbs = 6 * D;
    const size_t cper = (size_t)Bc * kvd * Le;
    int rc;
#define RUN(x) do { if ((rc = (x))) return rc; } while (0)
    auto gemm = [&](const float *A, int lda, const float *W, float *C, int ldc, int m, int n, int k, const float *bias,
                    int epi, const float *gate = nullptr) {
        GemmF32Args g{};
        g.A = A; g.lda = lda; g.W = W; g.ldw = k; g.C = C; g.ldc = ldc; g.M = m; g.N = n; g.K = k; g.bias = bias;
        g.epi = epi; g.res = C; g.ldr = ldc; g.gate = gate; g.gate_bstride = mbs; g.rows_per_batch = S;
        return gemm_f32(g, s);
    };
    // timestep embeddings (base:225-254, :1340-1344)
    for (int e = 0; e < 2; ++e) {
        RUN(timestep_sinusoid_f32(t, t_r, t_stride, e, Bc, h->freqs, f.emb[e], s));
        RUN(gemv_f32(f.emb[e], 256, f.te_l1[e], f.te_b1[e], f.h1, D, Bc, D, 256, 0, s));
        RUN(gemv_f32(f.h1, D, f.te_l2[e], f.te_b2[e], f.temb_e[e], D, Bc, D, D, 1, s));
        RUN(gemv_f32(f.temb_e[e], D, f.te_tp[e], f.te_btp[e], f.proj_e[e], 6 * D, Bc, 6 * D, D, 1, s));
    }
    RUN(add_f32(f.temb_e[0], f.temb_e[1], f.temb, (int64_t)Bc * D, s));
    RUN(add_f32(f.proj_e[0], f.proj_e[1], f.proj, (int64_t)Bc * 6 * D, s));
    RUN(modulation_f32(f.tables, L, 6, f.proj, Bc, D, f.mod, s));
    RUN(modulation_f32(f.sst_out, 1, 2, f.temb, Bc, D, f.mod_out, s));
    // concat + pad + proj_in (base:1347-1358)
    RUN(pack_patches_f32(xt, ctx, Bx, Bc, T, S, f.Xin, s));
    RUN(gemm(f.Xin, 384, f.win, f.X, D, M, D, 384, f.bin, EPI_STORE));
    for (int l = 0; l < L; ++l) {
        const auto &ly = f.layers[l];
        const float *md = f.mod + (size_t)l * Bc * 6 * D;
        // self-attention, AdaLN-Zero (base:499-511)
        RUN(rmsnorm_f32(f.X, ly.n_sa, md + 0 * D, md + 1 * D, mbs, S, f.XN, M, D, eps, s));
        RUN(gemm(f.XN, D, ly.wqkv, f.QKV, qd + 2 * kvd, M, qd + 2 * kvd, D, nullptr, EPI_STORE));
        HeadPostF32Args p{};
        p.src = f.QKV; p.ld_src = qd + 2 * kvd; p.B = Bc; p.S = S; p.nq = H; p.nk = KV; p.nv = KV;
        p.qw = ly.qn; p.kw = ly.kn; p.cos = f.rope_cos; p.sin = f.rope_sin;
        p.q = f.Qh; p.k = f.Kh; p.v = f.Vh; p.S_dst = S; p.eps = eps;
        RUN(head_post_f32(p, s));
        AttnF32Args at{};
        at.q = f.Qh; at.k = f.Kh; at.v = f.Vh; at.o = f.AO; at.o_ld = qd; at.B = Bc; at.H = H; at.KV = KV;
        at.Sq = S; at.Sk = S; at.window = h->sliding[l] ? h->cfg.window : -1; at.scale = scale;
        RUN(attention_f32(at, s));
        RUN(gemm(f.AO, qd, ly.wo, f.X, D, M, D, qd, nullptr, EPI_GATED_RES, md + 2 * D));
        // cross-attention, plain residual (base:513-526)
        RUN(rmsnorm_f32(f.X, ly.n_ca, nullptr, nullptr, 0, S, f.XN, M, D, eps, s));
        RUN(gemm(f.XN, D, ly.wcq, f.QKV, qd, M, qd, D, nullptr, EPI_STORE));
        HeadPostF32Args cq{};
        cq.src = f.QKV; cq.ld_src = qd; cq.B = Bc; cq.S = S; cq.nq = H; cq.qw = ly.cqn; cq.q = f.Qh;
        cq.S_dst = S; cq.eps = eps;
        RUN(head_post_f32(cq, s));
        AttnProbsSel sel;
        if (cap && capture_layer(cap, l, sel)) {   // acehip_dit_forward_capture (see dit.hip forward_body)
            RUN(attention_probs_f32(f.Qh, f.Kc + l * cper, Bc, H, KV, S, Le, sel, cap->k0, cap->k1, scale, cap->out, s));
            if (cap->stop_after_last && l == capture_last_layer(cap)) return 0;
        }
        AttnF32Args ca{};
        ca.q = f.Qh; ca.k = f.Kc + l * cper; ca.v = f.Vc + l * cper; ca.o = f.AO; ca.o_ld = qd; ca.B = Bc;
        ca.H = H; ca.KV = KV; ca.Sq = S; ca.Sk = Le; ca.window = -1; ca.scale = scale;
        RUN(attention_f32(ca, s));
        RUN(gemm(f.AO, qd, ly.wco, f.X, D, M, D, qd, nullptr, EPI_RES));
        // SwiGLU MLP, AdaLN-Zero (base:528-533)
        RUN(rmsnorm_f32(f.X, ly.n_mlp, md + 3 * D, md + 4 * D, mbs, S, f.XN, M, D, eps, s));
        RUN(gemm(f.XN, D, ly.wg, f.G, F, M, F, D, nullptr, EPI_STORE));
        RUN(gemm(f.XN, D, ly.wu, f.U, F, M, F, D, nullptr, EPI_STORE));
        RUN(swiglu_f32(f.G, f.U, f.Hb, (int64_t)M * F, s));
        RUN(gemm(f.Hb, F, ly.wdown, f.X, D, M, D, F, nullptr, EPI_GATED_RES, md + 5 * D));
    }
    // norm_out AdaLN + proj_out + crop (base:1491-1501)
    RUN(rmsnorm_f32(f.X, f.norm_out, f.mod_out, f.mod_out + D, 2 * D, S, f.XN, M, D, eps, s));
    RUN(gemm(f.XN, D, f.wout, T % 2 == 0 ? vt_out : f.O2, 128, M, 128, D, f.bout, EPI_STORE));
    if (T % 2) RUN(crop_rows_f32(f.O2, Bc, 2 * S, T, 64, vt_out, s));
#undef RUN
    return 0;
}
