// encoder.hip — the condition-encoder runtime behind acehip_enc_* (C ABI in
// include/acehip.h).
//
// One handle = one stack of AceStepEncoderLayer (reference base:374-440)
// between an embed_tokens Linear and a final Qwen3RMSNorm, with an optional
// proj_out Linear.  That single shape covers the lyric encoder (base:577-731,
// 8 layers, key-padding mask), the timbre encoder (base:997-1178, 4 layers,
// no mask), the attention pooler (base:734-859) and the detokenizer
// (base:862-994); the host composes them into AceStepConditionEncoder
// (base:1509-1554).  With every layer causal (sliding[l] == 2) and no embed
// Linear it is also the Qwen3-Embedding-0.6B text encoder (Qwen3Model, the
// reference's infer_text_embeddings, conditioning_embed.py:71-74).  The layer reuses the DiT's kernels unchanged:
//
//   XN = RMSNorm(X)                              rmsnorm_mod (plain)
//   q|k|v = XN·Wqkvᵀ → q/k RMSNorm + RoPE → head-major     gemm EPI_HEADPOST
//   AO = attention(q, k, v; band or full; key-padding mask)   attention
//   X  = bf16(X + bf16(AO·Woᵀ))                  gemm EPI_RES   (base:416-427)
//   XN = RMSNorm(X);  H = silu(XN·Wgᵀ)·(XN·Wuᵀ)  gemm EPI_SWIGLU
//   X  = bf16(X + bf16(H·Wdᵀ))                   gemm EPI_RES   (base:430-433)
//
// Runs once per song (twice in the reference, service_generate_execute.py:123
// and base:1820), so it is launch-count-light rather than tuned: every GEMM
// is the DiT's MFMA GEMM, every attention the DiT's flash kernel.
//
// One layer loop (enc_run) serves the four entries that run the stack; each describes its pass
// in an EncPass: rows per sequence, first RoPE row, where head-post writes k / v, which attention
// runs and what follows the final norm.
//
//   entry     rows   k / v go to                  attention                   out
//   forward   S      Kh / Vh                      flash, or extend (below)    every row (or proj_out)
//   prefill   S      Kh / Vh, copied to cache     as forward                  last row of each sequence
//   decode    1      cache slot pos               attention_decode            every row
//   extend    n      cache slots pos .. pos+n−1   attention_extend            every row
//                    of rows row0 .. row0+B−1
//
// A causal stack with heads / kv_heads = 4 (the 4B language model) has no flash kernel (those
// take ratios 1 and 2): its forward / prefill attention is attention_extend at pos = 0 over the
// head-post buffers, the S positions as S new queries over a "cache" of S rows, which writes a
// query row without any admissible key as zeros.
#include <cmath>
#include <map>
#include <vector>

#include "layer_args.h"
#include "weights.h"
#include "../../include/acehip.h"

using namespace acehip;

struct acehip_enc {
    int device = 0;
    acehip_enc_cfg cfg{};
    std::vector<uint8_t> sliding;
    int D = 0, F = 0, qd = 0, kvd = 0, L = 0;
    bool finalized = false;
    std::vector<void *> allocs;
    acehip::WeightTable weights;   // state-dict names → the buffers below (gate / up interleaved into wgu)
    struct Layer { bf16_t *ln1, *ln2, *wqkv, *wo, *qn, *kn, *wgu, *wdown; };
    std::vector<Layer> layers;
    bf16_t *wemb = nullptr, *bemb = nullptr, *norm = nullptr, *wout = nullptr, *bout = nullptr;
    bf16_t *rope_cos = nullptr, *rope_sin = nullptr;
    std::vector<float> inv_freq_override;
    // workspace
    bf16_t *X, *XN, *Qh, *Kh, *Vh, *AO, *Hb, *O128;
    void *attn_ws = nullptr;
    void *gemm_ws = nullptr;   // split-K partials for small-M GEMMs
    // token loop (acehip_enc_kv_create): per-layer K / V caches [L][kv_B][KV][kv_cap][128] and
    // attn_decode's key-range partials
    bf16_t *Kc = nullptr, *Vc = nullptr;
    int kv_B = 0, kv_cap = 0;
    bool kv_tried = false;     // a kv_create that failed part-way keeps its buffers until destroy: no second attempt
    void *dec_ws = nullptr;
    size_t dec_ws_bytes = 0;
    // multi-token continuation (acehip_enc_extend): attn_extend's key-range partials
    void *ext_ws = nullptr;
    size_t ext_ws_bytes = 0;
};

extern "C" {

int acehip_enc_destroy(acehip_enc *h) {
    if (!h) return 0;
    (void)hipSetDevice(h->device);
    for (void *p : h->allocs) (void)hipFree(p);
    delete h;
    return 0;
}

int acehip_enc_create(int device, const acehip_enc_cfg *cfg, acehip_enc **out) {
    if (!cfg || !out) return fail(ACEHIP_E_ARG, "enc_create: null argument");
    if (cfg->head_dim != 128) return fail(ACEHIP_E_ARG, "enc_create: head_dim must be 128");
    if (cfg->hidden % 256 || cfg->intermediate % 64 || cfg->kv_heads <= 0 || cfg->heads % cfg->kv_heads ||
        (cfg->heads / cfg->kv_heads > 2 && cfg->heads / cfg->kv_heads != 4) ||
        ((cfg->heads + 2 * cfg->kv_heads) * 128) % 256)
        return fail(ACEHIP_E_ARG, "enc_create: unsupported dims");
    // heads / kv_heads == 4 (the 4B LM): attention_extend is the only kernel that stacks four
    // query heads on a KV head, and it is causal — band and full layers, and the detokenizer's
    // proj_out stack, have no kernel at that ratio
    const bool wide = cfg->heads / cfg->kv_heads == 4;
    if (wide) {
        bool causal = cfg->sliding != nullptr && !cfg->out_dim;
        for (int i = 0; causal && i < cfg->layers; ++i) causal = cfg->sliding[i] == 2;
        if (!causal) return fail(ACEHIP_E_ARG, "enc_create: unsupported dims");
    }
    if (cfg->in_dim < 0 || (cfg->in_dim && cfg->in_dim % 64) || cfg->out_dim < 0 || cfg->out_dim > 128 ||
        cfg->layers < 0 || cfg->max_tokens <= 0 || cfg->max_S <= 0)
        return fail(ACEHIP_E_ARG, "enc_create: in_dim % 64, out_dim <= 128, max_tokens/max_S > 0");
    HIP_TRY(hipSetDevice(device));
    auto *h = new acehip_enc();
    h->device = device;
    h->cfg = *cfg;
    h->D = cfg->hidden; h->F = cfg->intermediate; h->L = cfg->layers;
    h->qd = cfg->heads * 128; h->kvd = cfg->kv_heads * 128;
    h->sliding.resize(h->L);
    for (int i = 0; i < h->L; ++i) h->sliding[i] = cfg->sliding ? cfg->sliding[i] : ((i + 1) % 2);
    h->cfg.sliding = nullptr;
    const int D = h->D, F = h->F, qd = h->qd, kvd = h->kvd;
    bool ok = true;
    auto A = [&](size_t n) { bf16_t *p = dev_alloc(h->allocs, n); ok = ok && p; return p; };
    auto slot = [&](const std::string &n, bf16_t *dst, std::vector<int64_t> shape, Pack kind = Pack::COPY) {
        h->weights.add(n, dst, std::move(shape), kind);
    };
    h->layers.resize(h->L);
    for (int i = 0; i < h->L && ok; ++i) {
        auto &ly = h->layers[i];
        ly.ln1 = A(D); ly.ln2 = A(D); ly.qn = A(128); ly.kn = A(128);
        ly.wqkv = A((size_t)(qd + 2 * kvd) * D); ly.wo = A((size_t)D * qd);
        ly.wgu = A((size_t)2 * F * D); ly.wdown = A((size_t)D * F);
        if (!ok) break;
        const std::string p = "layers." + std::to_string(i);
        slot(p + ".input_layernorm.weight", ly.ln1, {D});
        slot(p + ".post_attention_layernorm.weight", ly.ln2, {D});
        slot(p + ".self_attn.q_proj.weight", ly.wqkv, {qd, D});
        slot(p + ".self_attn.k_proj.weight", ly.wqkv + (size_t)qd * D, {kvd, D});
        slot(p + ".self_attn.v_proj.weight", ly.wqkv + (size_t)(qd + kvd) * D, {kvd, D});
        slot(p + ".self_attn.o_proj.weight", ly.wo, {D, qd});
        slot(p + ".self_attn.q_norm.weight", ly.qn, {128});
        slot(p + ".self_attn.k_norm.weight", ly.kn, {128});
        slot(p + ".mlp.gate_proj.weight", ly.wgu, {F, D}, Pack::GU_GATE);
        slot(p + ".mlp.up_proj.weight", ly.wgu, {F, D}, Pack::GU_UP);
        slot(p + ".mlp.down_proj.weight", ly.wdown, {D, F});
    }
    if (ok && cfg->in_dim) {
        h->wemb = A((size_t)D * cfg->in_dim);
        slot("embed_tokens.weight", h->wemb, {D, cfg->in_dim});
        if (cfg->embed_bias) {
            h->bemb = A(D);
            slot("embed_tokens.bias", h->bemb, {D});
        }
    }
    h->norm = A(D);
    if (ok) slot("norm.weight", h->norm, {D});
    if (ok && cfg->out_dim) {
        h->wout = A((size_t)128 * D);   // rows past out_dim stay zero
        h->bout = A(128);
        if (ok) {
            HIP_TRY(hipMemset(h->wout, 0, (size_t)128 * D * 2));
            HIP_TRY(hipMemset(h->bout, 0, 256));
            slot("proj_out.weight", h->wout, {cfg->out_dim, D});
            slot("proj_out.bias", h->bout, {cfg->out_dim});
        }
    }
    const size_t M = cfg->max_tokens;
    h->X = A(M * D); h->XN = A(M * D);
    h->Qh = A(M * qd); h->Kh = A(M * kvd); h->Vh = A(M * kvd); h->AO = A(M * qd);
    h->Hb = A(M * F);
    h->O128 = cfg->out_dim ? A(M * 128) : nullptr;
    h->gemm_ws = A(GEMM_WS_BYTES / 2);
    h->rope_cos = A((size_t)cfg->max_S * 128); h->rope_sin = A((size_t)cfg->max_S * 128);
    if (ok) {
        const size_t wb = attention_ws_bytes();
        h->attn_ws = dev_alloc(h->allocs, (wb + 1) / 2);
        ok = h->attn_ws && hipMemset(h->attn_ws, 0, wb) == hipSuccess;
    }
    if (ok && wide) {   // the forward's attention is attention_extend: its partials, cache or not
        h->ext_ws_bytes = attention_extend_ws_bytes(cfg->max_tokens, cfg->heads, cfg->max_tokens);
        h->ext_ws = dev_alloc(h->allocs, h->ext_ws_bytes / 2);
        ok = h->ext_ws != nullptr;
    }
    if (!ok) {
        acehip_enc_destroy(h);
        return fail(ACEHIP_E_OOM, "enc_create: device allocation failed");
    }
    *out = h;
    return 0;
}

int acehip_enc_set_weight(acehip_enc *h, const char *name, const void *ptr, int dtype, int ndim,
                          const int64_t *shape, int on_device) {
    if (!h || !name || !ptr || !shape || ndim <= 0) return fail(ACEHIP_E_ARG, "enc_set_weight: null argument");
    HIP_TRY(hipSetDevice(h->device));
    const std::string nm(name);
    if (nm == "_rope_inv_freq") {   // the caller's torch fp32 inv_freq (exact reference constant)
        if (dtype != ACEHIP_F32 || shape[0] != 64) return fail(ACEHIP_E_ARG, "_rope_inv_freq: fp32 [64]");
        return fetch_host_f32(ptr, dtype, 64, on_device, h->inv_freq_override);
    }
    if (nm == "rotary_emb.inv_freq") return 0;   // non-persistent buffer, recomputed
    WeightSlot *s = nullptr;
    if (int rc = h->weights.find_checked(nm, ndim, shape, "enc_set_weight", s)) return rc;
    // the handle keeps no staging buffer: fp32 is cast through a temporary
    return load_weight(*s, "enc_set_weight", nm, ptr, dtype, on_device, Staging{});
}

int acehip_enc_finalize(acehip_enc *h) {
    if (!h) return fail(ACEHIP_E_ARG, "null handle");
    HIP_TRY(hipSetDevice(h->device));
    if (int rc = h->weights.missing("enc_finalize")) return rc;
    if (h->F % 32) return fail(ACEHIP_E_ARG, "intermediate must be a multiple of 32");
    const int rc = build_rope_tables(h->cfg.head_dim, h->cfg.max_S, h->cfg.rope_theta, h->inv_freq_override,
                                     h->rope_cos, h->rope_sin);
    if (rc) return rc;
    HIP_TRY(hipDeviceSynchronize());
    h->finalized = true;
    return 0;
}

int acehip_enc_embed(acehip_enc *h, const void *x, int M, void *out, void *stream) {
    if (!h || !x || !out) return fail(ACEHIP_E_ARG, "null argument");
    if (!h->finalized || !h->wemb) return fail(ACEHIP_E_STATE, "enc_embed: not finalized / no embed_tokens");
    if (M <= 0) return M == 0 ? 0 : fail(ACEHIP_E_ARG, "enc_embed: M");
    HIP_TRY(hipSetDevice(h->device));
    const int K = h->cfg.in_dim;
    return gemm(lin_store((const bf16_t *)x, K, h->wemb, (bf16_t *)out, h->D, M, h->D, K, h->bemb), (hipStream_t)stream);
}

}  // extern "C"

// One pass of the layer stack over M = B·n rows of x: what an entry hands to enc_run.
struct EncPass {
    int B, n;             // sequences, rows per sequence (S for forward / prefill, 1 for decode)
    int pos;              // first RoPE row, and with KV_CACHE the first cache position written
    int row0;             // first cache row (extend); 0 otherwise
    enum { KV_BUFFERS, KV_CACHE } kv;   // head-post writes k / v to Kh / Vh [B][KV][n][128], or into the
                                        // cache at `pos` (q compact [B][H][n][128]); the attention reads the same
    bool copy_to_cache;   // prefill: Kh / Vh → cache rows [0, n) after head-post
    enum { ATT_FLASH, ATT_EXTEND, ATT_DECODE } att;
    const uint8_t *kmask; // key-padding mask [B][mask_ld], or null
    int mask_ld;
    enum { OUT_ALL_ROWS, OUT_LAST_ROW, OUT_PROJ } tail;   // after the final norm: every row, each sequence's
                                                          // last row, or the detokenizer's proj_out
};

// forward / prefill: the flash kernels take heads / kv_heads 1 and 2; at 4 (causal by enc_create) the
// S positions are S new queries over a "cache" of S rows, the head-post buffers
static EncPass enc_buffer_pass(const acehip_enc *h, const uint8_t *kmask, int B, int S, bool prefill) {
    EncPass p{};
    p.B = B; p.n = S;
    p.kv = EncPass::KV_BUFFERS; p.copy_to_cache = prefill;
    p.att = h->cfg.heads / h->cfg.kv_heads == 4 ? EncPass::ATT_EXTEND : EncPass::ATT_FLASH;
    p.kmask = kmask; p.mask_ld = S;
    p.tail = prefill ? EncPass::OUT_LAST_ROW : h->cfg.out_dim ? EncPass::OUT_PROJ : EncPass::OUT_ALL_ROWS;
    return p;
}

static int enc_run(acehip_enc *h, const void *x, const EncPass &p, void *out, hipStream_t s) {
    const int D = h->D, F = h->F, qd = h->qd, cap = h->kv_cap, B = p.B, n = p.n, M = B * n;
    const int H = h->cfg.heads, KV = h->cfg.kv_heads;
    const float eps = h->cfg.eps, scale = 1.0f / sqrtf(128.0f);
    const bool cache = p.kv == EncPass::KV_CACHE;
    // cache layer l: [kv_B][KV][cap][128]; the pass's rows start row_off in
    const size_t per = (size_t)h->kv_B * KV * cap * 128, row_off = (size_t)p.row0 * KV * cap * 128;
    const int kv_rows = cache ? cap : n;   // rows per KV head where k / v land
    const bf16_t *rcos = h->rope_cos + (size_t)p.pos * 128, *rsin = h->rope_sin + (size_t)p.pos * 128;
    int rc;
#define RUN(e) do { if ((rc = (e))) return rc; } while (0)
    HIP_TRY(hipMemcpyAsync(h->X, x, (size_t)M * D * 2, hipMemcpyDeviceToDevice, s));
    // few rows (text / lyric encoders, the token loop): the O and down GEMMs take gemm's split-K
    // path and leave their residual epilogue to the next norm (`pend`, as in the DiT forward)
    RowAdd pend{};
    for (int l = 0; l < h->L; ++l) {
        const auto &ly = h->layers[l];
        bf16_t *Kl = cache ? h->Kc + l * per + row_off : h->Kh, *Vl = cache ? h->Vc + l * per + row_off : h->Vh;
        RUN(rmsnorm_mod(h->X, ly.ln1, nullptr, nullptr, 0, n, h->XN, M, D, eps, s, pend));
        pend = RowAdd{};
        const HeadDst dst = cache ? HeadDst{h->Qh, Kl + (size_t)p.pos * 128, Vl + (size_t)p.pos * 128, cap, n}
                                  : HeadDst{h->Qh, Kl, Vl, n, 0};
        RUN(hgemm(h, lin_headpost(h->XN, D, ly.wqkv, D, B, n, H, KV, KV, ly.qn, ly.kn, rcos, rsin, eps, dst), s));
        if (p.copy_to_cache) {   // [B·KV] blocks of n rows → the same blocks of the cache, cap rows apart
            HIP_TRY(hipMemcpy2DAsync(h->Kc + l * per, (size_t)cap * 256, h->Kh, (size_t)n * 256, (size_t)n * 256,
                                     (size_t)B * KV, hipMemcpyDeviceToDevice, s));
            HIP_TRY(hipMemcpy2DAsync(h->Vc + l * per, (size_t)cap * 256, h->Vh, (size_t)n * 256, (size_t)n * 256,
                                     (size_t)B * KV, hipMemcpyDeviceToDevice, s));
        }
        switch (p.att) {
        case EncPass::ATT_FLASH: {
            // layer kind: 0 full, 1 band |i−j| <= window, 2 causal (the Qwen3 text encoder)
            const int win = h->sliding[l] == 2 ? ATTN_CAUSAL : h->sliding[l] ? h->cfg.window : -1;
            RUN(attention(h->Qh, Kl, Vl, h->AO, B, H, KV, n, n, win, scale, qd, h->attn_ws, s, p.kmask));
            break;
        }
        case EncPass::ATT_EXTEND:
            RUN(attention_extend(h->Qh, Kl, Vl, h->AO, B, H, KV, n, p.pos, kv_rows, p.kmask, p.mask_ld, scale,
                                 h->ext_ws, h->ext_ws_bytes, s));
            break;
        case EncPass::ATT_DECODE:
            RUN(attention_decode(h->Qh, Kl, Vl, h->AO, B, H, KV, p.pos + 1, kv_rows, p.kmask, p.mask_ld, scale,
                                 h->dec_ws, h->dec_ws_bytes, s));
            break;
        }
        RUN(hgemm(h, lin_res(h->AO, qd, ly.wo, h->X, D, M, D, qd), s, &pend));
        RUN(rmsnorm_mod(h->X, ly.ln2, nullptr, nullptr, 0, n, h->XN, M, D, eps, s, pend));
        pend = RowAdd{};
        RUN(hgemm(h, lin_swiglu(h->XN, D, ly.wgu, h->Hb, F, M, D), s));
        RUN(hgemm(h, lin_res(h->Hb, F, ly.wdown, h->X, D, M, D, F), s, &pend));
    }
    bf16_t *normed = p.tail == EncPass::OUT_ALL_ROWS ? (bf16_t *)out : h->XN;
    RUN(rmsnorm_mod(h->X, h->norm, nullptr, nullptr, 0, n, normed, M, D, eps, s, pend));
    if (p.tail == EncPass::OUT_LAST_ROW) {
        HIP_TRY(hipMemcpy2DAsync(out, (size_t)D * 2, h->XN + (size_t)(n - 1) * D, (size_t)n * D * 2, (size_t)D * 2, B,
                                 hipMemcpyDeviceToDevice, s));
    }
    if (p.tail == EncPass::OUT_PROJ) {
        // detokenizer proj_out (base:991): rows padded to 128 with zeros, then the used columns
        RUN(hgemm(h, lin_store(h->XN, D, h->wout, h->O128, 128, M, 128, D, h->bout), s));
        RUN(copy_cols(h->O128, 128, (bf16_t *)out, h->cfg.out_dim, M, h->cfg.out_dim, s));
    }
#undef RUN
    return 0;
}

extern "C" {

int acehip_enc_forward(acehip_enc *h, const void *x, const uint8_t *kmask, int B, int S, void *out, void *stream) {
    if (!h || !x || !out) return fail(ACEHIP_E_ARG, "null argument");
    if (!h->finalized) return fail(ACEHIP_E_STATE, "enc_forward before finalize");
    if (B <= 0 || S <= 0 || S > h->cfg.max_S || (int64_t)B * S > h->cfg.max_tokens)
        return fail(ACEHIP_E_ARG, "enc_forward: B*S / S out of range");
    HIP_TRY(hipSetDevice(h->device));
    return enc_run(h, x, enc_buffer_pass(h, kmask, B, S, false), out, (hipStream_t)stream);
}

// ---- token loop: K/V cache, prefill, one-token decode (acestep/llm_inference.py:416-438) ----

static bool enc_all_causal(const acehip_enc *h) {
    for (uint8_t k : h->sliding)
        if (k != 2) return false;
    return true;
}

int acehip_enc_kv_create(acehip_enc *h, int max_B, int capacity) {
    if (!h) return fail(ACEHIP_E_ARG, "null handle");
    if (h->Kc) return fail(ACEHIP_E_STATE, "enc_kv_create: the handle already has a cache");
    if (h->kv_tried)
        return fail(ACEHIP_E_STATE, "enc_kv_create: an earlier attempt on this handle failed; destroy the handle "
                                    "(its partial buffers are freed there) and create a new one");
    const int G = h->cfg.heads / h->cfg.kv_heads;
    if (G != 1 && G != 2 && G != 4)
        return fail(ACEHIP_E_ARG, "enc_kv_create: heads/kv_heads must be 1, 2 or 4 (the attention kernels over "
                                  "the cache); this model stays on the PyTorch path");
    if (!enc_all_causal(h) || h->cfg.out_dim)
        return fail(ACEHIP_E_ARG, "enc_kv_create: needs a causal stack (sliding[l] == 2 for every layer) without proj_out");
    if (max_B <= 0 || max_B > 65535 || max_B > h->cfg.max_tokens || capacity <= 0 || capacity > h->cfg.max_S)
        return fail(ACEHIP_E_ARG, "enc_kv_create: need 0 < max_B <= max_tokens and 0 < capacity <= max_S (the RoPE table)");
    HIP_TRY(hipSetDevice(h->device));
    h->kv_tried = true;
    const size_t per = (size_t)max_B * h->cfg.kv_heads * capacity * 128;
    h->dec_ws_bytes = attention_decode_ws_bytes(max_B, h->cfg.heads);
    bf16_t *kc = dev_alloc(h->allocs, per * h->L), *vc = kc ? dev_alloc(h->allocs, per * h->L) : nullptr;
    void *ws = vc ? dev_alloc(h->allocs, h->dec_ws_bytes / 2) : nullptr;
    // a heads/kv_heads = 4 handle has had its extend workspace since enc_create, sized for
    // max_tokens sequences: no smaller than this bound (max_B <= max_tokens)
    void *xws = h->ext_ws;
    if (!xws) {
        h->ext_ws_bytes = attention_extend_ws_bytes(max_B, h->cfg.heads, h->cfg.max_tokens);
        xws = ws ? dev_alloc(h->allocs, h->ext_ws_bytes / 2) : nullptr;
    }
    if (!ws) xws = nullptr;
    if (!xws) return fail(ACEHIP_E_OOM, "enc_kv_create: device allocation failed");   // freed by enc_destroy
    HIP_TRY(hipMemset(kc, 0, per * h->L * 2));
    HIP_TRY(hipMemset(vc, 0, per * h->L * 2));
    h->Kc = kc; h->Vc = vc; h->dec_ws = ws; h->ext_ws = xws;
    h->kv_B = max_B; h->kv_cap = capacity;
    return 0;
}

int acehip_enc_prefill(acehip_enc *h, const void *x, const uint8_t *kmask, int B, int S, void *out, void *stream) {
    if (!h || !x || !out) return fail(ACEHIP_E_ARG, "null argument");
    if (!h->finalized) return fail(ACEHIP_E_STATE, "enc_prefill before finalize");
    if (!h->Kc) return fail(ACEHIP_E_STATE, "enc_prefill: no cache (acehip_enc_kv_create)");
    if (B <= 0 || B > h->kv_B || S <= 0 || S > h->kv_cap || (int64_t)B * S > h->cfg.max_tokens)
        return fail(ACEHIP_E_ARG, "enc_prefill: B / S / B*S out of range (cache batch, capacity, max_tokens)");
    HIP_TRY(hipSetDevice(h->device));
    return enc_run(h, x, enc_buffer_pass(h, kmask, B, S, true), out, (hipStream_t)stream);
}

// n tokens per sequence appended at cache positions [pos, pos + n) of cache rows row0 .. row0 + B − 1
static EncPass enc_cache_pass(const uint8_t *kmask, int mask_ld, int row0, int B, int pos, int n) {
    EncPass p{};
    p.B = B; p.n = n; p.pos = pos; p.row0 = row0;
    p.kv = EncPass::KV_CACHE;
    p.att = EncPass::ATT_EXTEND;
    p.kmask = kmask; p.mask_ld = mask_ld;
    p.tail = EncPass::OUT_ALL_ROWS;
    return p;
}

int acehip_enc_decode(acehip_enc *h, const void *x, const uint8_t *kmask, int mask_ld, int B, int pos, void *out,
                      void *stream) {
    if (!h || !x || !out) return fail(ACEHIP_E_ARG, "null argument");
    if (!h->finalized) return fail(ACEHIP_E_STATE, "enc_decode before finalize");
    if (!h->Kc) return fail(ACEHIP_E_STATE, "enc_decode: no cache (acehip_enc_kv_create)");
    if (B <= 0 || B > h->kv_B) return fail(ACEHIP_E_ARG, "enc_decode: B exceeds the cache's batch");
    if (pos < 0 || pos >= h->kv_cap) return fail(ACEHIP_E_ARG, "enc_decode: pos must be in [0, capacity)");
    if (kmask && mask_ld < pos + 1) return fail(ACEHIP_E_ARG, "enc_decode: mask_ld < pos + 1");
    HIP_TRY(hipSetDevice(h->device));
    EncPass p = enc_cache_pass(kmask, mask_ld, 0, B, pos, 1);   // one token, on its own attention kernel
    p.att = EncPass::ATT_DECODE;
    return enc_run(h, x, p, out, (hipStream_t)stream);
}

int acehip_enc_extend(acehip_enc *h, const void *x, const uint8_t *kmask, int mask_ld, int row0, int B, int pos, int n,
                      void *out, void *stream) {
    if (!h || !x || !out) return fail(ACEHIP_E_ARG, "null argument");
    if (!h->finalized) return fail(ACEHIP_E_STATE, "enc_extend before finalize");
    if (!h->Kc) return fail(ACEHIP_E_STATE, "enc_extend: no cache (acehip_enc_kv_create)");
    if (B <= 0 || row0 < 0 || (int64_t)row0 + B > h->kv_B)
        return fail(ACEHIP_E_ARG, "enc_extend: rows [row0, row0 + B) exceed the cache's batch");
    if (pos < 0 || n < 1 || (int64_t)pos + n > h->kv_cap)
        return fail(ACEHIP_E_ARG, "enc_extend: need pos >= 0, n >= 1, pos + n <= capacity");
    if ((int64_t)B * n > h->cfg.max_tokens) return fail(ACEHIP_E_ARG, "enc_extend: B*n exceeds max_tokens");
    if (kmask && mask_ld < pos + n) return fail(ACEHIP_E_ARG, "enc_extend: mask_ld < pos + n");
    HIP_TRY(hipSetDevice(h->device));
    return enc_run(h, x, enc_cache_pass(kmask, mask_ld, row0, B, pos, n), out, (hipStream_t)stream);
}

int acehip_fsq_quantize(const void *z, int ldz, int M, const int *levels, int n_levels, void *codes, int ldc,
                        int32_t *indices, void *stream) {
    if (!z || !codes || !levels || n_levels <= 0 || n_levels > 8 || ldz < n_levels)
        return fail(ACEHIP_E_ARG, "fsq_quantize: argument");
    FsqLevels lv{n_levels, {}};
    for (int i = 0; i < n_levels; ++i) lv.L[i] = levels[i];
    return fsq_quantize((const bf16_t *)z, ldz, M, lv, (bf16_t *)codes, ldc, indices, (hipStream_t)stream);
}

int acehip_fsq_codes_from_indices(const int32_t *indices, int M, const int *levels, int n_levels, void *codes,
                                  int ldc, void *stream) {
    if (!indices || !codes || !levels || n_levels <= 0 || n_levels > 8) return fail(ACEHIP_E_ARG, "fsq_codes: argument");
    FsqLevels lv{n_levels, {}};
    for (int i = 0; i < n_levels; ++i) lv.L[i] = levels[i];
    return fsq_codes_from_indices(indices, M, lv, (bf16_t *)codes, ldc, (hipStream_t)stream);
}

}  // extern "C"
