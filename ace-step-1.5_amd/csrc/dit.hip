// dit.hip — the DiT runtime behind acehip_dit_* (C ABI in include/acehip.h).
//
// Owns the packed bf16 weights, the cross-attention K/V cache and a
// workspace sized at create time; acehip_dit_forward enqueues one whole
// AceStepDiTModel.forward (reference base:1303-1507) on the caller's stream
// with no allocation and no host synchronisation.
//
// Weight packing (from the reference state-dict names):
//   self q|k|v rows concatenated → one QKV GEMM (N = q + 2kv)
//   cross k|v rows concatenated → one GEMM per layer at set_condition
//   gate/up interleaved in 32-row panels → one GEMM with a SwiGLU epilogue
//   proj_in  Conv1d [D][192][2]  → [D][2·192] (k-major) so the patch GEMM
//            reads [T][192] rows pairwise with no im2col copy
//   proj_out ConvT  [D][64][2]   → [2·64][D] so the GEMM output [S][128] is
//            the de-patchified [2S][64] sequence in place
//   scale_shift_tables of all layers contiguous → one modulation launch
//
// The handle and the state-dict names are in dit_handle.h, the loader in weights.h, the fp32
// parity mode in dit_f32.hip; the library's error state and the stand-alone kernel entry
// points are in abi.hip.
#include "dit_handle.h"

using namespace acehip;

static int forward_body(acehip_dit *h, int Bc, int S, bool dup, bool ts_cached, hipStream_t s,
                        const acehip_attn_capture *cap = nullptr);
static int timestep_mlps(acehip_dit *h, const bf16_t *const emb[2], int rows, bf16_t *h1, bf16_t *const temb_e[2],
                         bf16_t *const proj_e[2], bf16_t *temb, bf16_t *proj, hipStream_t s);
static int forward_bf16(acehip_dit *h, const void *xt, const void *ctx, int Bx, const float *t, const float *t_r,
                        int t_stride, int step, int Bc, int T, void *vt_out, hipStream_t s,
                        const acehip_attn_capture *cap = nullptr);

extern "C" {

int acehip_dit_create(int device, const acehip_dit_cfg *cfg, acehip_dit **out) {
    if (!cfg || !out) return fail(ACEHIP_E_ARG, "dit_create: null argument");
    if (cfg->head_dim != 128) return fail(ACEHIP_E_ARG, "dit_create: head_dim must be 128");
    if (cfg->hidden % 256 || cfg->intermediate % 64 || cfg->heads % cfg->kv_heads)
        return fail(ACEHIP_E_ARG, "dit_create: unsupported dims");
    if (cfg->patch != 2 || cfg->in_channels != 192 || cfg->out_channels != 64)
        return fail(ACEHIP_E_ARG, "dit_create: patch 2 / 192 in / 64 out required");
    if (cfg->max_Bc > 16 || cfg->max_Bc <= 0 || cfg->max_S <= 0 || cfg->max_Lenc <= 0)
        return fail(ACEHIP_E_ARG, "dit_create: max_Bc in [1,16], max_S/max_Lenc > 0");
    HIP_TRY(hipSetDevice(device));
    auto *h = new acehip_dit();
    h->device = device;
    h->cfg = *cfg;
    h->D = cfg->hidden; h->F = cfg->intermediate; h->L = cfg->layers;
    h->qd = cfg->heads * cfg->head_dim; h->kvd = cfg->kv_heads * cfg->head_dim;
    h->sliding.resize(h->L);
    for (int i = 0; i < h->L; ++i) h->sliding[i] = cfg->sliding ? cfg->sliding[i] : ((i + 1) % 2);
    h->cfg.sliding = nullptr;
    h->graph_on = knobs().dit_graph == 1;
    if (cfg->fp32) {
        h->f32 = true;
        h->graph_on = false;
        const int rc = dit_create_f32(h);
        if (rc) {
            const std::string e = acehip_last_error();
            acehip_dit_destroy(h);
            return fail(rc, e);
        }
        *out = h;
        return 0;
    }
    const int D = h->D, F = h->F, qd = h->qd, kvd = h->kvd, L = h->L;
    bool ok = true;
    auto A = [&](size_t n) { bf16_t *p = dev_alloc(h->allocs, n); ok = ok && p; return p; };

    h->tables = A((size_t)L * 6 * D);
    h->layers.resize(L);
    // the layers' cross K/V projections side by side: set_condition runs them as ONE GEMM
    // (N = L·2·kvd) instead of L small-M ones
    h->wckv_all = A((size_t)L * 2 * kvd * D);
    for (int i = 0; i < L; ++i) {
        auto &ly = h->layers[i];
        ly.n_sa = A(D); ly.n_ca = A(D); ly.n_mlp = A(D);
        ly.wqkv = A((size_t)(qd + 2 * kvd) * D); ly.wo = A((size_t)D * qd);
        ly.qn = A(128); ly.kn = A(128); ly.cqn = A(128); ly.ckn = A(128);
        ly.wcq = A((size_t)qd * D); ly.wckv = h->wckv_all ? h->wckv_all + (size_t)i * 2 * kvd * D : nullptr;
        ly.wco = A((size_t)D * qd);
        ly.wgu = A((size_t)2 * F * D); ly.wdown = A((size_t)D * F);
    }
    h->sst_out = A(2 * D); h->win = A((size_t)D * 384); h->bin = A(D);
    h->wce = A((size_t)D * D); h->bce = A(D); h->norm_out = A(D);
    h->wout = A((size_t)128 * D); h->bout = A(128);
    for (int e = 0; e < 2; ++e) {
        h->te_l1[e] = A((size_t)D * 256); h->te_b1[e] = A(D);
        h->te_l2[e] = A((size_t)D * D); h->te_b2[e] = A(D);
        h->te_tp[e] = A((size_t)6 * D * D); h->te_btp[e] = A(6 * D);
    }
    // bf16: gate and up interleaved into one SwiGLU operand; the cross k|v slots point into wckv_all
    if (ok)
        register_dit_weights(h->weights, *h, L, D, F, qd, kvd, [](const acehip_dit::Layer &ly) {
            return GateUpDst<bf16_t>{ly.wgu, Pack::GU_GATE, ly.wgu, Pack::GU_UP};
        });
    // workspace
    const size_t S = cfg->max_S, Bc = cfg->max_Bc, M = S * Bc, Le = cfg->max_Lenc;
    h->X = A(M * D); h->XN = A(M * D);
    h->Qh = A(M * qd); h->Kh = A(M * kvd); h->Vh = A(M * kvd); h->AO = A(M * qd);
    h->Hb = A(M * F); h->Xin = A(M * 384); h->O2 = A(M * 128);
    for (int e = 0; e < 2; ++e) {
        h->emb[e] = A(Bc * 256); h->temb_e[e] = A(Bc * D); h->proj_e[e] = A(Bc * 6 * D);
    }
    h->h1 = A(Bc * D); h->temb = A(Bc * D); h->proj = A(Bc * 6 * D);
    h->mod = A((size_t)L * Bc * 6 * D); h->mod_out = A(Bc * 2 * D);
    h->Kc = A((size_t)L * Bc * kvd * Le); h->Vc = A((size_t)L * Bc * kvd * Le);
    // cross K/V scratch: the layers' K/V projections run as GEMMs over groups of kv_group layers
    // (N = kv_group·2·kvd), the group sized so the scratch stays ≤ 256 MiB at max_Bc·max_Lenc
    // (all 24 layers in one GEMM for a CFG song, one layer per GEMM at the 16 × 2048 maximum)
    {
        const size_t per_layer = Bc * Le * 2 * kvd * 2;
        const size_t bound = (size_t)knobs().kv_group_kib << 10;      // 256 MiB by default
        h->kv_group = (int)std::max<size_t>(1, std::min<size_t>((size_t)L, bound / per_layer));
    }
    h->E = A(Bc * Le * D); h->KVtmp = A(Bc * Le * 2 * kvd * (size_t)h->kv_group);
    h->cnull = A((size_t)L * D); h->vnull = A(qd);
    h->gemv_act = A((size_t)16 * D);
    h->gemm_ws = A(GEMM_WS_BYTES / 2);
    h->rope_cos = A(S * 128); h->rope_sin = A(S * 128);
    h->tmp_elems = std::max<size_t>((size_t)6 * D * D, (size_t)D * 384);
    h->tmp = A(h->tmp_elems * 2);   // room for an fp32 staging copy
    {   // attention tail-split partials + self-resetting counters (zeroed once)
        const size_t wb = attention_ws_bytes();
        h->attn_ws = A((wb + 1) / 2);
        if (h->attn_ws && hipMemset(h->attn_ws, 0, wb) != hipSuccess) ok = false;
    }
    void *fr = nullptr;
    if (ok && hipMalloc(&fr, 128 * sizeof(float)) == hipSuccess) {
        h->allocs.push_back(fr);
        h->freqs = (float *)fr;
        float f[128];
        for (int i = 0; i < 128; ++i)   // torch: exp(-ln(1e4) * arange(128, f32) / 128) in fp32 (base:239-241)
            f[i] = expf((-9.210340371976184f * (float)i) / 128.0f);
        ok = hipMemcpy(h->freqs, f, sizeof(f), hipMemcpyHostToDevice) == hipSuccess;
    } else {
        ok = false;
    }
    if (!ok) {
        acehip_dit_destroy(h);
        return fail(ACEHIP_E_OOM, "dit_create: device allocation failed");
    }
    *out = h;
    return 0;
}

int acehip_dit_set_weight(acehip_dit *h, const char *name, const void *ptr, int dtype, int ndim,
                          const int64_t *shape, int on_device) {
    if (!h || !name || !ptr || !shape) return fail(ACEHIP_E_ARG, "dit_set_weight: null argument");
    HIP_TRY(hipSetDevice(h->device));
    std::string nm(name);
    if (nm.rfind("decoder.", 0) == 0) nm = nm.substr(8);
    if (nm == "_timestep_freqs" || nm == "_rope_inv_freq") {
        // optional overrides computed by the caller's torch (exact reference constants), fp32
        if (dtype != ACEHIP_F32) return fail(ACEHIP_E_ARG, nm + ": fp32 required");
        const bool freqs = nm == "_timestep_freqs";
        if (freqs && shape[0] != 128) return fail(ACEHIP_E_ARG, "_timestep_freqs must have 128 entries");
        if (!freqs && shape[0] != h->cfg.head_dim / 2) return fail(ACEHIP_E_ARG, "_rope_inv_freq size");
        std::vector<float> v;
        if (int rc = fetch_host_f32(ptr, dtype, shape[0], on_device, v)) return rc;
        if (freqs) HIP_TRY(hipMemcpy(h->freqs, v.data(), 512, hipMemcpyHostToDevice));
        else h->inv_freq_override = v;
        return 0;
    }
    if (nm == "rotary_emb.inv_freq") return 0;  // non-persistent buffer; recomputed
    WeightSlot *s = nullptr;
    if (int rc = h->weights.find_checked(nm, ndim, shape, "dit_set_weight", s)) return rc;
    return load_weight(*s, "dit_set_weight", nm, ptr, dtype, on_device, Staging{h->tmp, h->tmp_elems * 4});
}

// Buffers of acehip_dit_set_timesteps for `cap` steps: allocated at finalize for kTsCap
// steps (every schedule the reference builds: ≤ 60 base/sft steps, ≤ 20 turbo), grown only
// by a longer schedule (the header documents that exception to "no allocation in calls").
static constexpr int kTsCap = 64;
static int alloc_timesteps(acehip_dit *h, int n_steps) {
    for (bf16_t *p : {h->ts_temb, h->ts_proj, h->ts_scratch})
        if (p) (void)hipFree(p);
    h->ts_temb = h->ts_proj = h->ts_scratch = nullptr;
    h->ts_cap = h->ts_n = 0;
    const int D = h->D;
    const int cap = std::max(n_steps, kTsCap);
    // scratch: emb [2][cap][256], h1 [cap][D], temb_e [2][cap][D], proj_e [2][cap][6D]
    const size_t scratch = (size_t)cap * (2 * 256 + D + 2 * D + 2 * 6 * D);
    HIP_TRY(hipMalloc(&h->ts_temb, (size_t)cap * D * 2));
    HIP_TRY(hipMalloc(&h->ts_proj, (size_t)cap * 6 * D * 2));
    HIP_TRY(hipMalloc(&h->ts_scratch, scratch * 2));
    h->ts_cap = cap;
    return 0;
}

int acehip_dit_finalize(acehip_dit *h) {
    if (!h) return fail(ACEHIP_E_ARG, "null handle");
    HIP_TRY(hipSetDevice(h->device));
    if (h->gexec) { HIP_TRY(hipGraphExecDestroy(h->gexec)); h->gexec = nullptr; }   // re-capture
    int rc = h->weights.missing("dit_finalize");
    if (rc) return rc;
    if (h->F % 32) return fail(ACEHIP_E_ARG, "intermediate must be a multiple of 32");
    rc = h->f32 ? dit_build_rope_f32(h)
                    : build_rope_tables(h->cfg.head_dim, h->cfg.max_S, h->cfg.rope_theta, h->inv_freq_override,
                                        h->rope_cos, h->rope_sin);
    if (rc) return rc;
    if (!h->f32 && h->ts_cap < kTsCap && (rc = alloc_timesteps(h, kTsCap))) return rc;
    HIP_TRY(hipDeviceSynchronize());
    h->finalized = true;
    return 0;
}

int acehip_dit_set_condition(acehip_dit *h, const void *enc, int Bc, int Lenc, void *stream) {
    if (!h || !enc) return fail(ACEHIP_E_ARG, "null argument");
    if (!h->finalized) return fail(ACEHIP_E_STATE, "set_condition before finalize");
    if (Bc <= 0 || Bc > h->cfg.max_Bc || Lenc <= 0 || Lenc > h->cfg.max_Lenc)
        return fail(ACEHIP_E_ARG, "set_condition: Bc/Lenc out of range");
    HIP_TRY(hipSetDevice(h->device));
    hipStream_t s = (hipStream_t)stream;
    if (h->f32) return dit_set_condition_f32(h, (const float *)enc, Bc, Lenc, s);
    const int D = h->D, kvd = h->kvd, M = Bc * Lenc;
    int rc = hgemm(h, lin_store((const bf16_t *)enc, D, h->wce, h->E, D, M, D, D, h->bce), s);
    if (rc) return rc;
    const size_t per = (size_t)Bc * kvd * Lenc;
    // the layers' K/V projections in GEMMs over groups of kv_group layers: M = Bc·Lenc rows ×
    // N = kv_group·2·kvd (turbo 10 s: 641 × 49152 in one GEMM — a full-chip grid, where L
    // separate N = 2048 GEMMs were small-M split-K launches + their epilogues); the k-norm /
    // head-major scatter stays per layer
    const int G = h->kv_group;
    const int64_t ldkv = (int64_t)G * 2 * kvd;
    for (int l = 0; l < h->L; ++l) {
        const int lg = l % G;
        if (lg == 0) {
            const int nl = std::min(G, h->L - l);
            const bf16_t *wkv = h->wckv_all + (size_t)l * 2 * kvd * D;
            if ((rc = hgemm(h, lin_store(h->E, D, wkv, h->KVtmp, ldkv, M, nl * 2 * kvd, D), s))) return rc;
        }
        HeadPostArgs p{};
        p.src = h->KVtmp + (size_t)lg * 2 * kvd; p.ld_src = ldkv; p.B = Bc; p.S = Lenc;
        p.nq = 0; p.nk = h->cfg.kv_heads; p.nv = h->cfg.kv_heads;
        p.kw = h->layers[l].ckn; p.k = h->Kc + l * per; p.v = h->Vc + l * per;
        p.S_dst = Lenc; p.eps = h->cfg.eps;
        if ((rc = head_post(p, s))) return rc;
    }
    h->have_cond = true;
    h->cond_Bc = Bc;
    h->cond_Lenc = Lenc;
    h->uniform_from = 1 << 30;
    return 0;
}

int acehip_dit_set_uniform_rows(acehip_dit *h, int first_row, void *stream) {
    if (!h) return fail(ACEHIP_E_ARG, "null handle");
    if (!h->have_cond) return fail(ACEHIP_E_STATE, "set_uniform_rows before set_condition");
    if (first_row < 0 || first_row > h->cond_Bc) return fail(ACEHIP_E_ARG, "set_uniform_rows: first_row in [0, Bc]");
    HIP_TRY(hipSetDevice(h->device));
    hipStream_t s = (hipStream_t)stream;
    h->uniform_from = 1 << 30;
    if (first_row == h->cond_Bc) return 0;   // none uniform
    if (h->f32) return 0;                    // parity mode: every row computed in full
    const int D = h->D, qd = h->qd, kvd = h->kvd, Le = h->cond_Lenc;
    const size_t per = (size_t)h->cond_Bc * kvd * Le;
    for (int l = 0; l < h->L; ++l) {
        // softmax over identical keys is uniform: every query's output is V row 0 of its
        // KV head (bit-exact: Σ of Lenc equal terms and the division are exact in fp32)
        int rc = gather_head_row(h->Vc + l * per + (size_t)first_row * kvd * Le, h->cfg.kv_heads, Le, h->cfg.heads,
                                 h->vnull, s);
        if (rc) return rc;
        if ((rc = hgemm(h, lin_store(h->vnull, qd, h->layers[l].wco, h->cnull + (size_t)l * D, D, 1, D, qd), s)))
            return rc;
    }
    h->uniform_from = first_row;
    return 0;
}

int acehip_dit_forward(acehip_dit *h, const void *xt, const void *ctx, int Bx, const float *t,
                       const float *t_r, int t_stride, int Bc, int T, int dtype, void *vt_out, void *stream) {
    if (!h || !xt || !ctx || !t || !t_r || !vt_out) return fail(ACEHIP_E_ARG, "null argument");
    if (!h->finalized || !h->have_cond) return fail(ACEHIP_E_STATE, "forward before finalize/set_condition");
    if (Bc != h->cond_Bc) return fail(ACEHIP_E_ARG, "forward: Bc differs from set_condition");
    if (dtype != (h->f32 ? ACEHIP_F32 : ACEHIP_BF16))
        return fail(ACEHIP_E_ARG, h->f32 ? "forward: this handle is the fp32 parity mode (dtype ACEHIP_F32)"
                                         : "forward: this handle is bf16 (dtype ACEHIP_BF16); create with fp32=1 "
                                           "for the fp32 parity mode");
    const int S = (T + 1) / 2;
    if (T <= 0 || S > h->cfg.max_S || Bx <= 0 || Bc % Bx) return fail(ACEHIP_E_ARG, "forward: T/Bx out of range");
    HIP_TRY(hipSetDevice(h->device));
    hipStream_t s = (hipStream_t)stream;
    if (h->f32)
        return dit_forward_f32(h, (const float *)xt, (const float *)ctx, Bx, t, t_r, t_stride, Bc, T, (float *)vt_out, s);
    return forward_bf16(h, xt, ctx, Bx, t, t_r, t_stride, -1, Bc, T, vt_out, s);
}

int acehip_dit_forward_capture(acehip_dit *h, const void *xt, const void *ctx, int Bx, const float *t,
                               const float *t_r, int t_stride, int Bc, int T, int dtype, void *vt_out,
                               const acehip_attn_capture *cap, void *stream) {
    if (!h || !xt || !ctx || !t || !t_r || !cap) return fail(ACEHIP_E_ARG, "forward_capture: null argument");
    if (!h->finalized || !h->have_cond)
        return fail(ACEHIP_E_STATE, "forward_capture before finalize/set_condition");
    if (Bc != h->cond_Bc) return fail(ACEHIP_E_ARG, "forward_capture: Bc differs from set_condition");
    if (dtype != (h->f32 ? ACEHIP_F32 : ACEHIP_BF16))
        return fail(ACEHIP_E_ARG, "forward_capture: dtype must be the handle's (ACEHIP_F32 with cfg.fp32, else ACEHIP_BF16)");
    const int S = (T + 1) / 2;
    if (T <= 0 || S > h->cfg.max_S || Bx <= 0 || Bc % Bx)
        return fail(ACEHIP_E_ARG, "forward_capture: T/Bx out of range");
    if (cap->n < 1 || cap->n > 64) return fail(ACEHIP_E_ARG, "forward_capture: cap->n must be in [1, 64]");
    if (!cap->layer || !cap->head || !cap->out)
        return fail(ACEHIP_E_ARG, "forward_capture: cap->layer / head / out must be set");
    if (!vt_out && !cap->stop_after_last)
        return fail(ACEHIP_E_ARG, "forward_capture: vt_out may be NULL only with stop_after_last");
    for (int i = 0; i < cap->n; ++i) {
        if (cap->layer[i] < 0 || cap->layer[i] >= h->L)
            return fail(ACEHIP_E_ARG, "forward_capture: layer " + std::to_string(cap->layer[i]) + " outside [0, " +
                                          std::to_string(h->L) + ")");
        if (cap->head[i] < 0 || cap->head[i] >= h->cfg.heads)
            return fail(ACEHIP_E_ARG, "forward_capture: head " + std::to_string(cap->head[i]) + " outside [0, " +
                                          std::to_string(h->cfg.heads) + ")");
    }
    if (cap->k0 < 0 || cap->k0 >= cap->k1 || cap->k1 > h->cond_Lenc)
        return fail(ACEHIP_E_ARG, "forward_capture: key range must satisfy 0 <= k0 < k1 <= Lenc (" +
                                      std::to_string(h->cond_Lenc) + ")");
    if (h->uniform_from < Bc)
        return fail(ACEHIP_E_STATE, "forward_capture: uniform rows are set (acehip_dit_set_uniform_rows); their "
                                    "cross-attention maps are not computed");
    HIP_TRY(hipSetDevice(h->device));
    hipStream_t s = (hipStream_t)stream;
    if (h->f32)
        return dit_forward_f32(h, (const float *)xt, (const float *)ctx, Bx, t, t_r, t_stride, Bc, T, (float *)vt_out, s,
                           cap);
    return forward_bf16(h, xt, ctx, Bx, t, t_r, t_stride, -1, Bc, T, vt_out, s, cap);
}

int acehip_dit_set_graph(acehip_dit *h, int enable) {
    if (!h) return fail(ACEHIP_E_ARG, "null handle");
    h->graph_on = enable != 0 && !h->f32;
    return 0;
}

int acehip_dit_set_timesteps(acehip_dit *h, const float *t, const float *t_r, int n_steps, void *stream) {
    if (!h || !t || !t_r) return fail(ACEHIP_E_ARG, "null argument");
    if (!h->finalized) return fail(ACEHIP_E_STATE, "set_timesteps before finalize");
    if (h->f32) return fail(ACEHIP_E_STATE, "set_timesteps: bf16 handles only (the fp32 parity mode runs per step)");
    if (n_steps <= 0 || n_steps > 4096) return fail(ACEHIP_E_ARG, "set_timesteps: n_steps in [1, 4096]");
    HIP_TRY(hipSetDevice(h->device));
    hipStream_t s = (hipStream_t)stream;
    const int D = h->D;
    if (n_steps > h->ts_cap) {                 // only schedules longer than kTsCap steps
        HIP_TRY(hipStreamSynchronize(s));
        int rc = alloc_timesteps(h, n_steps);
        if (rc) return rc;
    }
    const size_t cap = h->ts_cap;
    bf16_t *emb[2] = {h->ts_scratch, h->ts_scratch + cap * 256};
    bf16_t *h1 = h->ts_scratch + cap * 512;
    bf16_t *temb_e[2] = {h1 + cap * D, h1 + cap * 2 * D};
    bf16_t *proj_e[2] = {h1 + cap * 3 * D, h1 + cap * 9 * D};
    int rc;
    // one sinusoid row per step (t[i], t_r[i]), then the MLPs over all steps: the MLP weights
    // are read once per schedule instead of once per step
    for (int e = 0; e < 2; ++e)
        if ((rc = timestep_sinusoid(t, t_r, 1, e, n_steps, h->freqs, emb[e], s))) return rc;
    if ((rc = timestep_mlps(h, emb, n_steps, h1, temb_e, proj_e, h->ts_temb, h->ts_proj, s))) return rc;
    h->ts_n = n_steps;
    return 0;
}

int acehip_dit_forward_step(acehip_dit *h, const void *xt, const void *ctx, int Bx, int step, int Bc, int T,
                            int dtype, void *vt_out, void *stream) {
    if (!h || !xt || !ctx || !vt_out) return fail(ACEHIP_E_ARG, "null argument");
    if (!h->finalized || !h->have_cond) return fail(ACEHIP_E_STATE, "forward_step before finalize/set_condition");
    if (h->f32 || dtype != ACEHIP_BF16) return fail(ACEHIP_E_ARG, "forward_step: bf16 handles only");
    if (step < 0 || step >= h->ts_n) return fail(ACEHIP_E_STATE, "forward_step: step outside the set_timesteps schedule");
    if (Bc != h->cond_Bc) return fail(ACEHIP_E_ARG, "forward_step: Bc differs from set_condition");
    const int S = (T + 1) / 2;
    if (T <= 0 || S > h->cfg.max_S || Bx <= 0 || Bc % Bx) return fail(ACEHIP_E_ARG, "forward_step: T/Bx out of range");
    HIP_TRY(hipSetDevice(h->device));
    return forward_bf16(h, xt, ctx, Bx, nullptr, nullptr, 0, step, Bc, T, vt_out, (hipStream_t)stream);
}

}  // extern "C"

// Everything of one forward between the input packing and proj_out: reads only handle
// buffers (emb, Xin, weights, K/V cache), so it can be captured once and replayed.
// bf16 forward; step >= 0 takes the timestep MLP outputs from the set_timesteps cache
static int forward_bf16(acehip_dit *h, const void *xt, const void *ctx, int Bx, const float *t, const float *t_r,
                        int t_stride, int step, int Bc, int T, void *vt_out, hipStream_t s,
                        const acehip_attn_capture *cap) {
    const int S = (T + 1) / 2;
    const int M = Bc * S;
    int rc;
#define RUN(x) do { if ((rc = (x))) return rc; } while (0)
    // the only reads of t / xt / ctx: sinusoid embeddings and patch packing (base:1340-1358);
    // step >= 0: the schedule's precomputed timestep MLP row (acehip_dit_set_timesteps)
    const bool ts_cached = step >= 0;
    if (ts_cached) {
        RUN(bcast_rows(h->ts_temb + (size_t)step * h->D, h->D, h->temb, Bc, s));
        RUN(bcast_rows(h->ts_proj + (size_t)step * 6 * h->D, 6 * h->D, h->proj, Bc, s));
    } else {
        for (int e = 0; e < 2; ++e) RUN(timestep_sinusoid(t, t_r, t_stride, e, Bc, h->freqs, h->emb[e], s));
    }
    RUN(pack_patches((const bf16_t *)xt, (const bf16_t *)ctx, Bx, Bc, T, S, h->Xin, s));
    // CFG: every batch row reads xt/ctx row 0 (Bx = 1) at one broadcast t, so the rows are
    // identical until the first cross-attention — proj_in and layer 0's self-attention
    // block run on row 0 only and are copied (ACEHIP_DIT_DEDUP=0 disables, for A/B)
    const bool dup = Bx == 1 && Bc > 1 && (ts_cached || t_stride == 0) && knobs().dit_dedup;
    if (cap) {   // map capture: always eager; stop_after_last ends inside the layer loop
        RUN(forward_body(h, Bc, S, dup, ts_cached, s, cap));
        if (cap->stop_after_last) return 0;
    } else if (!h->graph_on || h->prof) {
        RUN(forward_body(h, Bc, S, dup, ts_cached, s));
    } else {
        const int key[6] = {Bc, S, h->cond_Lenc, std::min(h->uniform_from, Bc), (dup ? 1 : 0) | (ts_cached ? 2 : 0),
                            (int)knobs().gen};   // a knob reload re-captures
        if (!h->gexec || memcmp(key, h->gkey, sizeof(key))) {
            if (h->gexec) { HIP_TRY(hipGraphExecDestroy(h->gexec)); h->gexec = nullptr; }
            if (!h->cap_stream) HIP_TRY(hipStreamCreateWithFlags(&h->cap_stream, hipStreamNonBlocking));
            HIP_TRY(hipStreamBeginCapture(h->cap_stream, hipStreamCaptureModeRelaxed));
            const int brc = forward_body(h, Bc, S, dup, ts_cached, h->cap_stream);
            hipGraph_t g = nullptr;
            const hipError_t ec = hipStreamEndCapture(h->cap_stream, &g);
            if (brc) { if (g) (void)hipGraphDestroy(g); return brc; }
            if (ec != hipSuccess || !g) return fail(ACEHIP_E_HIP, "forward: graph capture failed");
            const hipError_t ei = hipGraphInstantiate(&h->gexec, g, nullptr, nullptr, 0);
            (void)hipGraphDestroy(g);
            if (ei != hipSuccess) { h->gexec = nullptr; return fail(ACEHIP_E_HIP, "forward: graph instantiate failed"); }
            memcpy(h->gkey, key, sizeof(key));
        }
        HIP_TRY(hipGraphLaunch(h->gexec, s));
    }
    // proj_out (base:1491-1501) on the normed output XN
    bf16_t *po = (T % 2 == 0) ? (bf16_t *)vt_out : h->O2;
    RUN(hgemm(h, lin_store(h->XN, h->D, h->wout, po, 128, M, 128, h->D, h->bout), s));
    if (T % 2) RUN(crop_rows(h->O2, Bc, 2 * S, T, 64, (bf16_t *)vt_out, s));
#undef RUN
    return 0;
}


#define RUN(x) do { if ((rc = (x))) return rc; } while (0)
// timestep embeddings: temb = temb_t + temb_r, proj = proj_t + proj_r (base:1340-1344) for
// `rows` rows of sinusoid embeddings, in chunks of 16 rows (gemv_small computes every row
// with the same instruction sequence whatever the row count, so a row's result does not
// depend on how many rows share the launch)
static int timestep_mlps(acehip_dit *h, const bf16_t *const emb[2], int rows, bf16_t *h1, bf16_t *const temb_e[2],
                         bf16_t *const proj_e[2], bf16_t *temb, bf16_t *proj, hipStream_t s) {
    const int D = h->D;
    int rc;
    for (int r0 = 0; r0 < rows; r0 += 16) {
        const int n = std::min(16, rows - r0);
        for (int e = 0; e < 2; ++e) {
            RUN(gemv_small(emb[e] + (size_t)r0 * 256, 256, h->te_l1[e], h->te_b1[e], h1 + (size_t)r0 * D, D, n, D,
                           256, 0, s));
            RUN(gemv_small(h1 + (size_t)r0 * D, D, h->te_l2[e], h->te_b2[e], temb_e[e] + (size_t)r0 * D, D, n, D, D,
                           1, s, h->gemv_act));
            RUN(gemv_small(temb_e[e] + (size_t)r0 * D, D, h->te_tp[e], h->te_btp[e], proj_e[e] + (size_t)r0 * 6 * D,
                           6 * D, n, 6 * D, D, 1, s, h->gemv_act));
        }
    }
    RUN(add_bf16(temb_e[0], temb_e[1], temb, (int64_t)rows * D, s));
    RUN(add_bf16(proj_e[0], proj_e[1], proj, (int64_t)rows * 6 * D, s));
    return 0;
}

// cap != null (acehip_dit_forward_capture): the selected heads' softmax rows of each captured
// layer are written from the cross-Q and the cross K cache; with stop_after_last the body
// returns right after the last captured layer's maps (X is not read again, so a pending
// deferred epilogue is dropped and norm_out is not run)
static int forward_body(acehip_dit *h, int Bc, int S, bool dup, bool ts_cached, hipStream_t s,
                        const acehip_attn_capture *cap) {
    const int D = h->D, F = h->F, qd = h->qd, kvd = h->kvd, L = h->L, M = Bc * S;
    const int H = h->cfg.heads, KV = h->cfg.kv_heads, Le = h->cond_Lenc;
    const float eps = h->cfg.eps, scale = 1.0f / sqrtf((float)h->cfg.head_dim);
    int rc;
    // timestep MLPs (temb, proj), unless acehip_dit_forward_step already broadcast the
    // schedule's precomputed row into h->temb / h->proj
    if (!ts_cached) RUN(timestep_mlps(h, h->emb, Bc, h->h1, h->temb_e, h->proj_e, h->temb, h->proj, s));
    RUN(modulation(h->tables, L, 6, h->proj, Bc, D, h->mod, s));
    RUN(modulation(h->sst_out, 1, 2, h->temb, Bc, D, h->mod_out, s));

    // proj_in (base:1347-1358) over the packed patches Xin
    RUN(hgemm(h, lin_store(h->Xin, 384, h->win, h->X, D, dup ? S : M, D, 384, h->bin), s));

    const bool fuse_rowadd = knobs().fuse_rowadd != 0;
    const size_t cper = (size_t)Bc * kvd * Le;
    const int Bq = std::min(h->uniform_from, Bc), Mq = Bq * S;   // rows with a real cross-attention
    // small-M grids take gemm's split-K path; the residual epilogue of such a GEMM (O, cross-O,
    // down) is then deferred into the next norm, which reads the rows anyway: `pend` carries
    // it (gemm sets pend.part only when it deferred).  Deferral needs that norm to cover every
    // row the GEMM wrote, and no X copy in between (the layer-0 CFG dedup).
    RowAdd pend{};
    for (int l = 0; l < L; ++l) {
        const auto &ly = h->layers[l];
        const bf16_t *md = h->mod + (size_t)l * Bc * 6 * D;
        const int64_t mbs = 6 * D;
        // --- self-attention with AdaLN-Zero (base:499-511); layer 0 of identical CFG rows: row 0
        const int Bs = (dup && l == 0) ? 1 : Bc, Ms = Bs * S;
        RUN(rmsnorm_mod(h->X, ly.n_sa, md + 0 * D, md + 1 * D, mbs, S, h->XN, Ms, D, eps, s, pend));
        pend = RowAdd{};
        // QKV projection with q/k RMSNorm + RoPE + head-major scatter fused in the epilogue
        const GemmArgs q = lin_headpost(h->XN, D, ly.wqkv, D, Bs, S, H, KV, KV, ly.qn, ly.kn, h->rope_cos, h->rope_sin,
                                        eps, HeadDst{h->Qh, h->Kh, h->Vh, S, 0});
        RUN(timed(h, 2, s, [&] { return hgemm(h, q, s); }));
        RUN(timed(h, h->sliding[l] ? 5 : 4, s, [&] {
            return attention(h->Qh, h->Kh, h->Vh, h->AO, Bs, H, KV, S, S, h->sliding[l] ? h->cfg.window : -1,
                             scale, qd, h->attn_ws, s);
        }));
        const GemmArgs o = lin_gated_res(h->AO, qd, ly.wo, h->X, D, Ms, D, qd, md + 2 * D, mbs, S);
        const bool defer_o = fuse_rowadd && Bs == Bc && (Mq == M || Mq == 0);
        RUN(timed(h, 3, s, [&] { return hgemm(h, o, s, defer_o ? &pend : nullptr); }));
        for (int b = Bs; b < Bc; ++b)
            HIP_TRY(hipMemcpyAsync(h->X + (size_t)b * S * D, h->X, (size_t)S * D * 2, hipMemcpyDeviceToDevice, s));
        // --- cross-attention, plain residual (base:513-526); rows >= uniform_from (CFG null
        // rows, base:1907) get their constant cross-O output cnull[l] (set_uniform_rows)
        if (Mq > 0) {
            RUN(rmsnorm_mod(h->X, ly.n_ca, nullptr, nullptr, 0, S, h->XN, Mq, D, eps, s, pend));
            pend = RowAdd{};
            GemmArgs cq = lin_headpost(h->XN, D, ly.wcq, D, Bq, S, H, 0, 0, ly.cqn, nullptr, nullptr, nullptr, eps,
                                       HeadDst{h->Qh, nullptr, nullptr, S, 0});   // q heads only, no RoPE
            cq.ws = h->gemm_ws;
            cq.ws_bytes = h->gemm_ws ? GEMM_WS_BYTES : 0;
            AttnProbsSel sel;
            const bool captured = cap && capture_layer(cap, l, sel);
            // One launch for the projection and the attention (cross_q_attn_kernel: the Q tile stays
            // in LDS) where the projection runs on the half-chip four-wave tile, the attention as
            // whole units on attn_fwd_kernel and every 192-row tile lies in one batch element; a
            // captured layer needs Q in global memory.  Bit-identical to the two launches
            // (ACEHIP_CROSS_FUSE=0), which then take exactly those two kernels.
            const bool fusable = cross_fuse_shape(cq, KV, Le) && cross_fuse_planned(cq) &&
                                 attention_whole_units(Bq, H, KV, S, Le, h->attn_ws != nullptr);
            if (fusable && knobs().cross_fuse && !captured) {
                RUN(timed(h, 6, s, [&] {
                    return cross_q_attention(cq, h->Kc + l * cper, h->Vc + l * cper, h->AO, KV, Le, scale, qd, s);
                }));
            } else {
                RUN(fusable ? gemm_variant(cq, 13, s) : gemm(cq, s));
                if (captured) {
                    RUN(attention_probs(h->Qh, h->Kc + l * cper, Bq, H, KV, S, Le, sel, cap->k0, cap->k1, scale,
                                        cap->out, s));
                    if (cap->stop_after_last && l == capture_last_layer(cap)) return 0;
                }
                RUN(timed(h, 6, s, [&] {
                    return attention(h->Qh, h->Kc + l * cper, h->Vc + l * cper, h->AO, Bq, H, KV, S, Le, -1, scale, qd,
                                     h->attn_ws, s);
                }));
            }
            const GemmArgs co = lin_res(h->AO, qd, ly.wco, h->X, D, Mq, D, qd);
            RUN(timed(h, 3, s, [&] { return hgemm(h, co, s, fuse_rowadd ? &pend : nullptr); }));
        }
        // --- SwiGLU MLP with AdaLN-Zero (base:528-533); the null rows' constant cross-O output
        // is added inside the norm pass (ACEHIP_FUSE_ROWADD=0: separate add_row_bcast, A/B)
        RowAdd ra = pend;   // rows < ra.prows: the deferred cross-O (or O) epilogue, applied first
        pend = RowAdd{};
        if (Mq < M) {
            if (fuse_rowadd) {
                ra.xw = h->X;
                ra.v = h->cnull + (size_t)l * D;
                ra.from = Mq;
            } else {
                RUN(add_row_bcast(h->X + (size_t)Mq * D, h->cnull + (size_t)l * D, M - Mq, D, s));
            }
        }
        RUN(rmsnorm_mod(h->X, ly.n_mlp, md + 3 * D, md + 4 * D, mbs, S, h->XN, M, D, eps, s, ra));
        const GemmArgs gu = lin_swiglu(h->XN, D, ly.wgu, h->Hb, F, M, D);
        RUN(timed(h, 0, s, [&] { return hgemm(h, gu, s); }));
        const GemmArgs dn = lin_gated_res(h->Hb, F, ly.wdown, h->X, D, M, D, F, md + 5 * D, mbs, S);
        RUN(timed(h, 1, s, [&] { return hgemm(h, dn, s, fuse_rowadd ? &pend : nullptr); }));
    }
    // norm_out AdaLN (base:1491-1497); proj_out runs after the body
    RUN(rmsnorm_mod(h->X, h->norm_out, h->mod_out, h->mod_out + D, 2 * D, S, h->XN, M, D, eps, s, pend));
#undef RUN
    return 0;
}

extern "C" {

int acehip_dit_profile(acehip_dit *h, int enable) {
    if (!h) return fail(ACEHIP_E_ARG, "null handle");
    HIP_TRY(hipSetDevice(h->device));
    if (enable && h->ev.empty()) {
        h->ev.resize(2 * acehip_dit::NPAIR);
        h->ev_kind.resize(acehip_dit::NPAIR);
        for (auto &e : h->ev) HIP_TRY(hipEventCreate(&e));
    }
    h->prof = enable != 0;
    h->ev_used = 0;
    return 0;
}

int acehip_dit_profile_kinds(acehip_dit *h, unsigned mask) {
    if (!h) return fail(ACEHIP_E_ARG, "null handle");
    h->prof_mask = mask;
    return 0;
}

int acehip_dit_profile_read(acehip_dit *h, int kind, int *launches, float *total_ms) {
    if (!h || !launches || !total_ms) return fail(ACEHIP_E_ARG, "null argument");
    HIP_TRY(hipSetDevice(h->device));
    int n = 0;
    float tot = 0.f;
    for (int i = 0; i < h->ev_used; ++i) {
        if (h->ev_kind[i] != kind) continue;
        float ms = 0.f;
        HIP_TRY(hipEventSynchronize(h->ev[2 * i + 1]));
        HIP_TRY(hipEventElapsedTime(&ms, h->ev[2 * i], h->ev[2 * i + 1]));
        tot += ms;
        ++n;
    }
    *launches = n;
    *total_ms = tot;
    return 0;
}

int acehip_dit_destroy(acehip_dit *h) {
    if (!h) return 0;
    (void)hipSetDevice(h->device);
    for (auto &e : h->ev) (void)hipEventDestroy(e);
    if (h->gexec) (void)hipGraphExecDestroy(h->gexec);
    if (h->cap_stream) (void)hipStreamDestroy(h->cap_stream);
    for (void *p : h->allocs) (void)hipFree(p);
    for (bf16_t *p : {h->ts_temb, h->ts_proj, h->ts_scratch})
        if (p) (void)hipFree(p);
    delete h;
    return 0;
}

}  // extern "C"
