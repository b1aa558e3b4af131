/*
 * acehip.h — C ABI of libacehip.so, the MI355X (gfx950) implementation of the
 * ACE-Step 1.5 hot path: the DiT flow-matching denoise step and the Oobleck
 * VAE decode/encode.
 *
 * Plain C: opaque handles, plain pointers and sizes, int status codes. No
 * torch types cross this boundary.  All tensors are caller-owned, contiguous,
 * device-resident buffers (e.g. torch.Tensor.data_ptr()); the library owns the
 * packed weights, the cross-attention K/V cache and the workspace (sized at
 * create time from the max_* fields).  Nothing is allocated inside
 * forward/decode/encode calls.  Two calls allocate, once, outside the hot loop:
 *   - acehip_sampler_apg_euler keeps its norm partials in a library-owned
 *     workspace per (device, stream), allocated on the first call on that stream
 *     and grown (hipFree + hipMalloc) only when a larger B*T arrives;
 *   - acehip_dit_set_timesteps uses buffers allocated at finalize for 64 steps;
 *     a longer schedule (the reference builds <= 60) synchronises the stream and
 *     grows them once.
 * Work is enqueued on the caller's stream (hipStream_t passed as void*); apart from
 * that growth no entry point synchronises the host.
 *
 * Threading: a handle is bound to one device and is not re-entrant; every
 * entry point calls hipSetDevice(handle->device) first because callers (the
 * reference API server's ThreadPoolExecutor, reference
 * acestep/api_server.py:1291-1292) may call from any thread.
 *
 * Errors: 0 = ok; negative = error class; acehip_last_error() returns the
 * thread-local message of the last failing call.
 *
 * Each entry point names the reference interface it replaces (file:line in
 * the reference checkout).
 */
#ifndef ACEHIP_H
#define ACEHIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 100: round-1 ABI.  200: dtype argument on acehip_dit_forward and the three sampler
 * entry points, acehip_dit_cfg.fp32 (round 2).  300: acehip_vae_encode accepts any
 * N in [hop, max_T*hop] (latents = floor(N/hop) frames).  Callers check
 * acehip_get_version() == ACEHIP_VERSION before binding (acehip/_ffi.py does). */
#define ACEHIP_VERSION 400

enum acehip_status {
    ACEHIP_OK = 0,
    ACEHIP_E_ARG = -1,          /* bad argument / shape */
    ACEHIP_E_OOM = -2,          /* device allocation failed */
    ACEHIP_E_HIP = -3,          /* HIP runtime error */
    ACEHIP_E_STATE = -4,        /* not finalized / condition not set */
    ACEHIP_E_NAME = -5          /* unknown weight name */
};

enum acehip_dtype { ACEHIP_F32 = 0, ACEHIP_BF16 = 1 };

int acehip_get_version(void);
/* Re-read the ACEHIP_* A/B switches from the environment (they are read once, on first
 * use, otherwise).  Tests and A/B tools only: call while no other thread is inside the
 * library; a DiT handle re-captures its HIP graph after a reload. */
int acehip_reload_knobs(void);
const char *acehip_last_error(void);
/* Hash of what the library was built from and how: the native sources (the .hip and .h files under
 * csrc/ and include/), the Makefile and the compile flags `make` received (ARCH, EXTRA);
 * ace-step-1.5_amd/csrc/native_hash.py.  acehip/_ffi.py refuses a library whose hash differs from the
 * default build (gfx950, no EXTRA) of the sources beside it, so a shipped binary is provably the
 * tree's and no diagnostic build. */
const char *acehip_build_hash(void);

/* ---------------------------------------------------------------- DiT ---- */

/* Hyper-parameters (reference AceStepConfig,
 * acestep/models/base/configuration_acestep_v15.py:148-260). */
typedef struct acehip_dit_cfg {
    int hidden;          /* 2048 */
    int intermediate;    /* 6144 */
    int heads;           /* 16 */
    int kv_heads;        /* 8 */
    int head_dim;        /* 128 (the kernels require 128) */
    int layers;          /* 24 */
    int window;          /* 128: sliding layers attend |i-j| <= window */
    int patch;           /* 2 */
    int in_channels;     /* 192 = context 128 + latent 64 */
    int out_channels;    /* 64 */
    float eps;           /* 1e-6 */
    float rope_theta;    /* 1e6 */
    int max_S;           /* max tokens per batch row (T/patch) */
    int max_Bc;          /* max DiT batch (2x songs with CFG) */
    int max_Lenc;        /* max encoder sequence length */
    const uint8_t *sliding; /* [layers] 1 = sliding layer; NULL = even idx */
    int fp32;            /* 0: the bf16 production path; 1: the fp32 parity mode (SURVEY
                          * §8c(iii)) — fp32 weights, activations and accumulation, the
                          * reference's fp32 forward (init_service_orchestrator.py:51 runs
                          * fp32 off cuda/xpu); set_condition / forward then take fp32 */
} acehip_dit_cfg;

typedef struct acehip_dit acehip_dit;

/* replaces: AutoModel.from_pretrained(...).to(device).to(dtype)
 * (acestep/core/generation/handler/init_service_loader.py:56-89) */
int acehip_dit_create(int device, const acehip_dit_cfg *cfg, acehip_dit **out);

/* One reference state-dict tensor by its HF name without the "decoder."
 * prefix (e.g. "layers.3.mlp.gate_proj.weight").  Copies and
 * repacks; the caller keeps ownership of ptr.  dtype: ACEHIP_F32/BF16.
 * Precedent: acestep/models/mlx/dit_convert.py:11-66. */
int acehip_dit_set_weight(acehip_dit *h, const char *name, const void *ptr, int dtype,
                          int ndim, const int64_t *shape, int on_device);

/* Validates that every tensor is present; builds fused layouts. */
int acehip_dit_finalize(acehip_dit *h);

/* condition_embedder + per-layer cross-attention K/V cache.
 * replaces: the first-step branch of AceStepAttention.forward
 * (acestep/models/base/modeling_acestep_v15_base.py:310-325, :1359).
 * enc: [Bc, Lenc, hidden] in the handle's dtype (CFG: cond rows then null rows). */
int acehip_dit_set_condition(acehip_dit *h, const void *enc, int Bc, int Lenc, void *stream);

/* Declare batch rows [first_row, Bc) of the current condition uniform: their
 * encoder sequence is ONE vector repeated (the CFG null rows,
 * null_condition_emb.expand_as, base:1907).  The decoder never masks encoder
 * positions (base:1384-1385), so such a row's cross-attention softmax is
 * exactly uniform and its output is V row 0 for every query; forward then
 * skips the cross-Q projection / attention / cross-O GEMM for those rows and
 * adds the per-layer constant cross-O output (precomputed here).  first_row ==
 * Bc turns it off; set_condition resets it. */
int acehip_dit_set_uniform_rows(acehip_dit *h, int first_row, void *stream);

/* One decoder forward: AceStepDiTModel.forward
 * (acestep/models/base/modeling_acestep_v15_base.py:1303-1507).
 * xt: bf16 [Bx, T, 64]; ctx: bf16 [Bx, T, 128]; batch row b of the DiT reads
 * xt/ctx row (b % Bx) — CFG's cat([xt, xt]) without a copy (base:1929).
 * t, t_r: device fp32 [Bc] holding model-dtype values; t_stride 0
 * broadcasts element 0.  vt_out: [Bc, T, 64].  dtype is the
 * element type of xt / ctx / vt_out and must be the handle's: ACEHIP_BF16
 * (production) or ACEHIP_F32 (a handle created with cfg.fp32 = 1). */
int acehip_dit_forward(acehip_dit *h, const void *xt, const void *ctx, int Bx,
                       const float *t, const float *t_r, int t_stride, int Bc, int T,
                       int dtype, void *vt_out, void *stream);

/* Timestep MLPs of a whole schedule at once: t, t_r are device fp32 arrays of n_steps
 * entries, one broadcast timestep pair per step (the t-dependent part of
 * AceStepDiTModel.forward, base:1340-1344, evaluated for every step of the sampler loop
 * base:1936 / turbo:1968 up front).  acehip_dit_forward_step(step) is then
 * acehip_dit_forward with t = t[step], t_r = t_r[step], t_stride 0, except that the ~108 MB
 * of timestep-MLP weights are read once per schedule instead of once per step — bit-
 * identical (each MLP row is computed by the same instruction sequence).  bf16 handles. */
int acehip_dit_set_timesteps(acehip_dit *h, const float *t, const float *t_r, int n_steps, void *stream);
int acehip_dit_forward_step(acehip_dit *h, const void *xt, const void *ctx, int Bx, int step, int Bc, int T,
                            int dtype, void *vt_out, void *stream);

/* Cross-attention map capture: which softmax rows acehip_dit_forward_capture writes.
 * The lyric aligners (handler/lyric_timestamp.py:78-111, lyric_score.py:93-138) use a few
 * (layer, head) pairs of the decoder's cross-attention and only the lyric tokens of the key
 * axis; out is already in their [tokens, frames] orientation (the transpose(-1, -2) of
 * lyric_timestamp.py:100):
 *   out[i][b][j - k0][s] = softmax_j(scale · q_s · k_j) of layer[i], head[i], batch row b,
 * the softmax over all Lenc encoder positions (the decoder never masks them,
 * base:1384-1385).  A bf16 handle rounds each value to bf16 before the fp32 store (the
 * reference's eager softmax is fp32 then .to(query.dtype)); an fp32 handle stores it
 * unrounded. */
typedef struct acehip_attn_capture {
    int n;                    /* 1..64 selected (layer, head) pairs */
    const int *layer, *head;  /* host arrays [n], any order; out keeps this order */
    int k0, k1;               /* encoder positions kept, 0 <= k0 < k1 <= Lenc */
    float *out;               /* device fp32 [n][Bc][k1-k0][S], S = ceil(T / patch) */
    int stop_after_last;      /* != 0: return after the cross-attention of the highest selected
                                 layer; vt_out may be NULL and is not written */
} acehip_attn_capture;

/* acehip_dit_forward plus the capture; replaces decoder(..., output_attentions=True,
 * custom_layers_config, enable_early_exit) (base:1303-1507, :352-367).  One extra kernel
 * launch per captured layer (all of that layer's selected heads), on the cross-Q the
 * forward computes anyway; no [B, heads, S, Lenc] tensor is formed.  With
 * stop_after_last == 0, vt_out is bit-identical to acehip_dit_forward on the same
 * inputs.  Always the eager path (never the HIP-graph replay); nothing is allocated.
 * ACEHIP_E_STATE if uniform rows are set (acehip_dit_set_uniform_rows: the maps of
 * skipped rows do not exist); ACEHIP_E_ARG for a layer, head or key range out of
 * range, n outside 1..64, or vt_out == NULL without stop_after_last. */
int acehip_dit_forward_capture(acehip_dit *h, const void *xt, const void *ctx, int Bx, const float *t,
                               const float *t_r, int t_stride, int Bc, int T, int dtype, void *vt_out,
                               const acehip_attn_capture *cap, void *stream);

/* Replay the pointer-independent middle of acehip_dit_forward (timestep MLPs,
 * modulation, proj_in, the layer stack, norm_out) as one HIP graph, captured
 * once per (Bc, S, Lenc, uniform rows) and re-captured when they change or
 * after finalize.  Default off (ACEHIP_DIT_GRAPH=1 turns it on at create):
 * measured neutral on MI355X (0.600 vs 0.602 s/song, turbo 10 s 38.8 vs
 * 39.2 ms) — kernel-to-kernel gaps are not launch-bound here.  Profiling runs
 * the eager path.  Results are bit-identical either way. */
int acehip_dit_set_graph(acehip_dit *h, int enable);

int acehip_dit_destroy(acehip_dit *h);

/* Per-kernel HIP-event timing inside acehip_dit_forward (for the bench's
 * roofline numbers).  enable != 0 clears the counters and starts recording
 * an event pair around every launch of the listed kernel families on the
 * forward's stream; read after the caller synchronised that stream.
 * kind: 0 SwiGLU gate/up GEMM, 1 down GEMM, 2 QKV GEMM, 3 O/cross-O GEMMs,
 *       4 full self-attention, 5 band self-attention, 6 cross-attention. */
int acehip_dit_profile(acehip_dit *h, int enable);
int acehip_dit_profile_read(acehip_dit *h, int kind, int *launches, float *total_ms);
/* Restrict recording to the kinds whose bit is set (default 0x7f = all): the
 * bench times only the roofline kernel inside its timed region. */
int acehip_dit_profile_kinds(acehip_dit *h, unsigned mask);

/* --------------------------------------------------- condition encoders ---- */

/* One stack of AceStepEncoderLayer (reference base:374-440) with its
 * embed_tokens Linear, final Qwen3RMSNorm and optional proj_out Linear — the
 * shape shared by AceStepLyricEncoder (base:577-731), AceStepTimbreEncoder
 * (base:997-1178), AttentionPooler (base:734-859) and AudioTokenDetokenizer
 * (base:862-994).  The host composes them into AceStepConditionEncoder
 * (base:1509-1554; pack_sequences base:138-169 is index plumbing). */
typedef struct acehip_enc_cfg {
    int hidden;          /* 2048 */
    int intermediate;    /* 6144 */
    int heads;           /* 16 */
    int kv_heads;        /* 8 */
    int head_dim;        /* 128 */
    int layers;          /* lyric 8, timbre 4, pooler/detokenizer 2 */
    int window;          /* 128 (sliding layers: |i-j| <= window) */
    int in_dim;          /* embed_tokens in-features (lyric/text 1024, timbre 64, pooler 2048) */
    int embed_bias;      /* 1: embed_tokens has a bias */
    int out_dim;         /* proj_out out-features (detokenizer 64), 0 = none; <= 128 */
    float eps;           /* 1e-6 */
    float rope_theta;    /* 1e6 */
    int max_tokens;      /* max B*S per forward */
    int max_S;           /* max sequence length */
    const uint8_t *sliding; /* [layers] 1 = sliding layer, 2 = causal (Qwen3
                             * text encoder, Qwen3Model's default mask); NULL = even idx */
} acehip_enc_cfg;

typedef struct acehip_enc acehip_enc;

/* heads / kv_heads is 1 or 2 for any stack.  A ratio of 4 (the 4B language model, 32 / 8 heads) is
 * accepted for a causal stack only — sliding given and sliding[l] == 2 for every layer, out_dim
 * == 0: such a handle sends the attention of acehip_enc_forward / acehip_enc_prefill to
 * acehip_attention_extend_bf16 (the S positions as S new queries at pos = 0 over the head-post
 * buffers, cap = S), the one kernel besides the decode step's that stacks four query heads on a
 * KV head, and allocates that kernel's partials workspace here
 * (acehip_attention_extend_ws_bytes for cfg.max_tokens).  Band and full layers have no kernel
 * at that ratio: any other ratio-4 stack, and any other ratio, is ACEHIP_E_ARG ("unsupported
 * dims").  One difference follows from that kernel's rule: with a key mask, a query row without
 * any admissible key (the left padding of a batch) leaves the attention as zeros, where the flash
 * kernels give it a uniform average; such rows' outputs are never read, and their K / V stay
 * masked for every later query. */
int acehip_enc_create(int device, const acehip_enc_cfg *cfg, acehip_enc **out);
/* Names relative to the module, as in its state dict: "embed_tokens.weight",
 * "layers.3.self_attn.q_proj.weight", "layers.3.input_layernorm.weight",
 * "norm.weight", "proj_out.bias" ...  dtype ACEHIP_F32/BF16. */
int acehip_enc_set_weight(acehip_enc *h, const char *name, const void *ptr, int dtype, int ndim,
                          const int64_t *shape, int on_device);
int acehip_enc_finalize(acehip_enc *h);
/* embed_tokens: out bf16 [M, hidden] = x bf16 [M, in_dim] · Wᵀ (+ b)
 * (base:623, :1085, :766, :895). */
int acehip_enc_embed(acehip_enc *h, const void *x, int M, void *out, void *stream);
/* layers + norm (+ proj_out): x bf16 [B, S, hidden] (not modified) →
 * out bf16 [B, S, out_dim ? out_dim : hidden].  kmask: device uint8 [B, S]
 * key-padding mask (1 = attend; create_4d_mask semantics, base:56-135) or
 * NULL (no padding mask).  RoPE positions 0..S-1 per sequence. */
int acehip_enc_forward(acehip_enc *h, const void *x, const uint8_t *kmask, int B, int S, void *out,
                       void *stream);
int acehip_enc_destroy(acehip_enc *h);

/* Token loop of the 5 Hz language model (a transformers Qwen3ForCausalLM driven one token at
 * a time by the reference's _forward_pass, acestep/llm_inference.py:416-438) on a causal
 * handle (every sliding[l] == 2, no embed Linear needed, no proj_out).
 *
 * acehip_enc_kv_create allocates, once, the per-layer K / V caches
 * [layers][max_B][kv_heads][capacity][128] and the partials workspace of the decode
 * attention; acehip_enc_destroy frees them.  capacity <= cfg.max_S (the RoPE table),
 * max_B <= cfg.max_tokens.  heads / kv_heads is 1, 2 (the 0.6B and 1.7B LMs; the prefill runs on
 * the flash kernels) or 4 (the 4B LM; the prefill's attention is acehip_attention_extend_bf16, see
 * acehip_enc_create, and the handle keeps the extend workspace it allocated there);
 * ACEHIP_E_ARG otherwise. */
int acehip_enc_kv_create(acehip_enc *h, int max_B, int capacity);
/* First call of a generation: model(input_ids[B,S], attention_mask[B,S], use_cache=True).
 * The layer loop of acehip_enc_forward, causal AND key-padded when kmask (device uint8
 * [B, S], 1 = attend; the batch is left-padded) is given; each layer's K (after norm and
 * RoPE) and V of positions [0, S) also land in the cache; out bf16 [B, hidden] is the
 * final-norm row of position S - 1 of every sequence.  B <= max_B, S <= capacity,
 * B*S <= cfg.max_tokens.  Rows at padded positions stay finite (heads / kv_heads = 4: their
 * attention output is exactly zero, acehip_enc_create).  At that ratio the K / V of the prompt
 * are copied into the cache as at the others, and the attention reads the head-post buffers. */
int acehip_enc_prefill(acehip_enc *h, const void *x, const uint8_t *kmask, int B, int S, void *out, void *stream);
/* Every later call: model(input_ids[:, -1:], past_key_values, attention_mask[B, pos+1]).
 * x bf16 [B, hidden], one token per sequence at cache index pos = the number of positions
 * already cached (the same for every row of a left-padded batch); RoPE position = pos, padding
 * included, as transformers computes it when no position_ids are passed.  kmask: device uint8
 * [B, mask_ld >= pos + 1] over cache positions, or NULL.  out bf16 [B, hidden] (final norm).
 * ACEHIP_E_ARG when pos >= capacity.  Caller's stream, no allocation, no host sync. */
int acehip_enc_decode(acehip_enc *h, const void *x, const uint8_t *kmask, int mask_ld, int B, int pos, void *out,
                      void *stream);
/* Multi-token continuation: model(input_ids[:, pos:pos+n], past_key_values, attention_mask
 * [B, pos+n]) on cache rows row0 .. row0 + B - 1 (sequence b is cache row row0 + b).  x bf16
 * [B, n, hidden]; the n tokens take cache indices and RoPE positions [pos, pos + n), each layer's
 * K (normed, rotated) and V land in those cache rows, and every new query attends the cached
 * keys j <= its own position (acehip_attention_extend_bf16).  kmask: device uint8
 * [B, mask_ld >= pos + n] over cache positions, row b for sequence b, or NULL.  out bf16
 * [B, n, hidden]: the final-norm row of every new position.  pos = 0 is a prefill that returns
 * every row; n = 1 is a decode step on the other attention kernel.  The partials workspace was
 * allocated by acehip_enc_kv_create (acehip_attention_extend_ws_bytes for cfg.max_tokens; 17.3 MB
 * on 256 compute units).  Its size follows the CU count planned for at that time: with
 * ACEHIP_ATTN_CUS raised afterwards a call whose plan needs more returns ACEHIP_E_ARG.  ACEHIP_E_STATE without a cache; ACEHIP_E_ARG unless row0 >= 0,
 * row0 + B <= max_B, pos >= 0, n >= 1, pos + n <= capacity, B*n <= cfg.max_tokens and, with a
 * mask, mask_ld >= pos + n.  Caller's stream, no allocation, no host sync. */
int acehip_enc_extend(acehip_enc *h, const void *x, const uint8_t *kmask, int mask_ld, int row0, int B, int pos,
                      int n, void *out, void *stream);

/* FSQ quantizer of the audio tokenizer (ResidualFSQ, 1 quantizer, levels
 * {8,8,8,5,5,5}: base:1196-1200; vector_quantize_pytorch FSQ restated, see
 * oracle/condenc_oracle.py): z bf16 [M, ldz] (the project_in output, first
 * n_levels columns) → codes bf16 [M, ldc >= 64] (columns >= n_levels zeroed, so
 * the padded project_out GEMM can consume them) and int32 indices [M] (or NULL). */
int acehip_fsq_quantize(const void *z, int ldz, int M, const int *levels, int n_levels, void *codes, int ldc,
                        int32_t *indices, void *stream);
/* FSQ.indices_to_codes (quantizer.get_output_from_indices before project_out,
 * acestep/core/generation/handler/audio_codes.py:62). */
int acehip_fsq_codes_from_indices(const int32_t *indices, int M, const int *levels, int n_levels, void *codes,
                                  int ldc, void *stream);

/* ------------------------------------------------------------ sampler ---- */

/* One base/sft CFG step: cond/uncond split + APG (momentum -0.75, norm clip
 * 2.5 over T, float64 projection) + Euler ODE update, fused.
 * replaces: base:1943-1979 + acestep/models/base/apg_guidance.py:5-56.
 * vt: bf16 [2B, T, 64] (cond rows then uncond rows); xt: bf16 [B, T, 64]
 * updated in place; ra: bf16 [B, T, 64] momentum state (first_step != 0
 * means running_average == 0); apply_cfg == 0 → vt = cond (no momentum
 * update), apply_cfg < 0 → no CFG (vt is [B,T,64]).  dt: bf16 value.
 * out_mode 0: xt = bf16(xt − bf16(v·dt)) (ODE);  out_mode 1: xt = v (the
 * guided velocity, for the caller's SDE branch, base:1968-1973).
 * dtype: ACEHIP_BF16 (every op rounded to bf16 as torch does) or ACEHIP_F32 (the
 * fp32 parity mode: the same chain unrounded) for vt / xt / ra.
 * The norms' chunk partials live in a library-owned workspace per (device,
 * stream), allocated on first use under a lock: concurrent calls on different
 * streams are independent; calls on one stream are ordered by that stream. */
int acehip_sampler_apg_euler(const void *vt, void *xt, void *ra, int B, int T, int C,
                             float guidance, float dt, int apply_cfg, int first_step,
                             int out_mode, int dtype, void *stream);

/* One base/sft CFG step with ADG guidance (use_adg=True) + Euler, fused.
 * replaces: base:1958-1964 + adg_forward (apg_guidance.py:107-180, angle clip
 * pi/6, no norm).  vt: bf16 [2B, T, 64] cond then uncond; xt: bf16 [B, T, 64]
 * updated in place; sigma: t_curr (bf16 value).  Row-local (no reduction over
 * T).  The reference only supports B == 1 (its [N*T,1] x [N,T,C] broadcast);
 * this computes the per-row generalisation for any B.  out_mode as above. */
int acehip_sampler_adg_euler(const void *vt, void *xt, int B, int T, int C, float guidance,
                             float sigma, float dt, int out_mode, int dtype, void *stream);

/* xt = bf16(xt - bf16(vt * s)) on [n] elements — Euler ODE (turbo:1985-1991)
 * and the final x0 = xt - vt*t (turbo:1975-1977); dtype as above. */
int acehip_sampler_axpy(const void *vt, void *xt, int64_t n, float s, int dtype, void *stream);

/* ---------------------------------------------------------------- VAE ---- */

/* diffusers AutoencoderOobleck config (acestep/models/mlx/vae_model.py:251-281) */
typedef struct acehip_vae_cfg {
    int encoder_hidden;  /* 128 */
    int decoder_channels;/* 128 */
    int latent_channels; /* 64 */
    int audio_channels;  /* 2 */
    int n_blocks;        /* 5 */
    int ratios[8];       /* downsampling ratios, e.g. {2,4,4,6,10} */
    int multiples[8];    /* channel multiples, e.g. {1,2,4,8,16} */
    int max_T;           /* max latent frames per decode */
    int max_B;
    int with_encoder;
} acehip_vae_cfg;

typedef struct acehip_vae acehip_vae;

/* replaces: AutoencoderOobleck.from_pretrained (init_service_loader.py:123-144) */
int acehip_vae_create(int device, const acehip_vae_cfg *cfg, acehip_vae **out);
/* diffusers names: "decoder.block.2.res_unit1.conv1.weight_g" etc.; both the
 * weight_g/weight_v and parametrizations.weight.original{0,1} spellings. */
int acehip_vae_set_weight(acehip_vae *h, const char *name, const void *ptr, int dtype,
                          int ndim, const int64_t *shape, int on_device);
/* fuses weight_g·v/||v|| and repacks every conv into implicit-GEMM layout */
int acehip_vae_finalize(acehip_vae *h);

/* vae.decode(z).sample (acestep/core/generation/handler/vae_decode_chunks.py:42)
 * z: bf16 [B, 64, T] → wav fp32 [B, 2, T*hop]; untiled (the decoder's
 * receptive field is < the reference's 64-frame overlap). */
int acehip_vae_decode(acehip_vae *h, const void *z, int B, int T, void *wav, void *stream);
/* Test entry (block-level parity): the first launches of acehip_vae_decode for ONE song
 * (z bf16 [1, 64, T]) — conv1 and decoder blocks 0 .. n_blocks-1 — and a copy of the
 * activation they leave: channels-last bf16 [L][C] (L = T·Π strides so far), already passed
 * through the NEXT Snake (block n_blocks' snake1, or decoder.snake1 after the last block),
 * i.e. exactly the input of the next stage (vae_model.py:119-142, 190-230). */
int acehip_vae_decode_blocks(acehip_vae *h, const void *z, int T, int n_blocks, void *act, void *stream);

/* vae.encode(x).latent_dist.sample() (vae_encode.py:65) — and, untiled, the
 * handler's tiled_encode (vae_encode.py:15-82: the encoder's receptive field is
 * inside the reference's 2 s overlap, tiled == untiled).
 * wav: bf16 [B, 2, N], hop <= N <= max_T*hop; T = floor(N/hop) latent frames
 * (every strided conv maps L to floor(L/s), as AutoencoderOobleck's does);
 * eps: bf16 [B, 64, T] or NULL (NULL → the mean); z_out: bf16 [B, 64, T]. */
int acehip_vae_encode(acehip_vae *h, const void *wav, int B, int N, const void *eps,
                      void *z_out, void *stream);

int acehip_vae_destroy(acehip_vae *h);

/* Unit-level parity hooks (no reference counterpart: the per-conv checks of the
 * Oobleck layers, acestep/models/mlx/vae_model.py:24-230, against fp32
 * torch.nn.functional.conv1d / conv_transpose1d).  Both run the production weight
 * packing and kernel selection on channels-last bf16 tensors and synchronise `stream`.
 * acehip_vae_conv: kind 0 Conv1d(k, dilation dil, padding dil·(k−1)/2); kind 1
 * ConvTranspose1d(k = 2s, stride s, padding ⌈s/2⌉) (decoder blocks); kind 2 Conv1d(k = 2s,
 * stride s, padding ⌈s/2⌉) (encoder blocks).  in [L_in][Cin]; w bf16 in torch layout
 * ([Cout][Cin][k]; kind 1: [Cin][Cout][k]); bias [Cout] or NULL; res [L_out][Cout] or NULL
 * (out = bf16(res + bf16(conv + bias))); out [L_out][Cout] or NULL; alpha/beta [Cout]
 * (Snake1d, log-scale) with out_s = Snake(out) or NULL.  Cin % 64 == 0, Cout % 128 == 0.
 * acehip_vae_resunit: one C = 128 OobleckResidualUnit (vae_model.py:62-87) as the decoder
 * runs it: x, x_s = bf16(snake1(x)) [L][128] → x_out = x + conv2(snake2(conv1(x_s))) (or
 * NULL) and xs_out = bf16(snake_next(x_out)); w1 [128][128][7] (dilation dil ≤ 9), w2
 * [128][128][1]. */
int acehip_vae_conv(int kind, const void *in, int64_t L_in, int Cin, const void *w, const void *bias,
                    const void *res, int Cout, int k, int stride, int dil, void *out, const void *alpha,
                    const void *beta, void *out_s, void *stream);
int acehip_vae_resunit(const void *x, const void *x_s, int64_t L, int C, int dil, const void *w1, const void *b1,
                       const void *alpha2, const void *beta2, const void *w2, const void *b2, const void *alpha_n,
                       const void *beta_n, void *x_out, void *xs_out, void *stream);

/* The decode output guard of _decode_generate_music_pred_latents
 * (acestep/core/generation/handler/generate_music_decode.py:190-192):
 * per song, peak = max |wav|; if peak > 1 the song is divided by its peak.
 * wav fp32 [B, n] in place (n = channels·samples, n % 4 == 0); peak: device
 * scratch of B floats (receives the peaks). */
int acehip_wav_peak_normalize(float *wav, int B, int64_t n, float *peak, void *stream);

/* The guard above (guard != 0) fused with the product's loudness step,
 * normalize_audio (acestep/audio_utils.py:24-62, applied per song at
 * acestep/inference.py:674-679 when enable_normalization and normalization_db
 * <= 0): after the guard, gain = (1 / peak) * target_amp (fp32, the order torch
 * evaluates float / tensor in), wav *= gain,
 * skipped for songs whose peak < 1e-6.  target_amp = fp32(10^(normalization_db/20));
 * 0 = no normalization.  Bit-identical to the reference steps it replaces; one
 * peak pass + one scale pass. */
int acehip_wav_postprocess(float *wav, int B, int64_t n, float *peak, int guard, float target_amp,
                           void *stream);
/* The postprocess pass pair above with the output leg's sample conversion fused in (audio_utils.py
 * AudioSaver.save_audio → soundfile PCM_16, the default FLAC / WAV subtype): wav fp32 [B][C][N]
 * (C = 1 or 2, N % 4 == 0) is updated in place exactly as acehip_wav_postprocess does, and every
 * sample is also written to pcm int16 [B][N][C] (interleaved frames) as
 * rint(clamp(x, -1, 1) * 32767).  Halves the device→host bytes of the leg. */
int acehip_wav_postprocess_pcm16(float *wav, int B, int C, int64_t N, float *peak, int guard, float target_amp,
                                 int16_t *pcm, void *stream);

/* ------------------------------------------------------------ kernels ---- */
/* Single-kernel entry points used by the parity tests and the profiler
 * (same code the runtimes above launch). */

/* C[M,N] = A[M,K] · W[N,K]^T (+bias) — bf16 MFMA, fp32 accumulate. */
int acehip_gemm_bf16(const void *A, int lda, const void *W, int ldw, void *C, int ldc,
                     int M, int N, int K, const void *bias, void *stream);

/* Same with an explicit epilogue (0 store+bias, 2 residual add into C,
 * 3 SwiGLU: W rows packed [32 gate; 32 up] per 64-row panel, C is [M][N/2])
 * and tile variant (0: 128x128 2-stage, 7: 256x256 ping-pong, 8: 192x256
 * ping-pong, 9: 128x256 ping-pong (7-9: N % 256 == 0), 13: four-wave 192x128
 * + DMA helper waves (N % 128 == 0), 16: 128x64 4-stage, 17: 16 + two DMA
 * helper waves (N % 64 == 0);
 * -1: the production choice, including the tail split and split-K for grids that
 * cannot fill half the chip) — tuning and tests. */
int acehip_gemm_bf16_ex(const void *A, int lda, const void *W, int ldw, void *C, int ldc,
                        int M, int N, int K, const void *bias, int epi, int variant, void *stream);

/* The residual epilogues, for tests: C = bf16(res + bf16(acc)) with gate == NULL, else the
 * AdaLN-Zero gated form C = bf16(res + bf16(bf16(acc) · gate[m / rows_per_batch][n])), gate row b
 * at gate + b·gate_bstride (ceil(M / rows_per_batch) rows of N).  res [M][ldr] may be C itself
 * (in place) or a buffer of its own; rows >= M of C and columns >= N are not written.
 * variant as in acehip_gemm_bf16_ex (-1: the production choice with the shared split-K
 * workspace, whose epilogue then runs in the split-K reduction kernel). */
int acehip_gemm_res_bf16(const void *A, int lda, const void *W, int ldw, void *C, int ldc,
                         int M, int N, int K, const void *res, int ldr, const void *gate,
                         int64_t gate_bstride, int rows_per_batch, int variant, void *stream);

/* Host-only check, for tests (no GPU call): the ping-pong GEMM tiles (BM x 256, BM in {64, 128,
 * 192, 256}; variants 7-9 and the implicit-GEMM convs) fetch their operands by LDS-DMA from
 * addresses formed either as a 64-bit pointer per lane or as a scalar tile base plus a 32-bit
 * lane offset (ACEHIP_GEMM_SADDR).  For every row / column tile, wave, lane, piece and K-tile of
 * an [M, K] x [N, K]^T grid this forms both and returns the number of pieces whose byte address
 * differs (-1: bad arguments).  conv_cin != 0: the A-side K offset of an implicit-GEMM conv
 * (conv_cin channels per tap, dilation conv_dil, first tap at input row m + conv_a0).
 * *fits: whether the library would take the scalar form for these leading dimensions;
 * *min_a / *max_a, *max_b: the lowest / highest byte offset from A, and the highest from W,
 * that any piece touches (its last byte).  Any out pointer may be NULL. */
int64_t acehip_diag_pp_src_check(int M, int N, int K, int64_t lda, int64_t ldw, int BM, int conv_cin,
                                 int conv_dil, int conv_a0, int *fits, int64_t *min_a, int64_t *max_a,
                                 int64_t *max_b);

/* Host-only check, for tests (no GPU call): the slot-immediate K loop of the ping-pong GEMM tiles
 * (ACEHIP_GEMM_SLOTIMM) issues every LDS read as a per-lane base register, formed once before the
 * loop per operand, k-step and ring slot, plus an instruction immediate of 2048 bytes per 16-row
 * sub-tile.  With the kernel's LDS array at 32-bit LDS address lds, this walks BM in {64, 128,
 * 192, 256} x wave x lane x ring slot x k-step x operand x sub-tile, forms base + immediate in
 * 32-bit arithmetic as the kernel does, and returns the number of reads that differ from the
 * swizzled address of their row and chunk in that slot, whose immediate does not fit the 16-bit
 * offset field, or that leave the tile's LDS array.  *reads: reads walked; *max_imm: the largest
 * immediate; *max_end: the highest byte past any read, relative to lds.  Any out pointer may be
 * NULL. */
int64_t acehip_diag_pp_lds_check(uint32_t lds, int64_t *reads, int *max_imm, int64_t *max_end);

/* Host-only, for tests: whether a ping-pong launch of BM x 256 tiles with epilogue epi (0-4, 6: the
 * implicit-GEMM convs) and these leading dimensions runs the slot-immediate K loop under the current
 * ACEHIP_GEMM_SLOTIMM / ACEHIP_GEMM_SADDR (the persistent walk takes it under either SADDR value). */
int acehip_diag_pp_slotimm(int epi, int BM, int64_t lda, int64_t ldw);

/* The route acehip_gemm_bf16_ex(..., variant -1) and the runtimes' GEMMs take for a shape: the
 * value the library's dispatch plans before it launches (csrc/gemm_plan.h holds the rules).
 * Fields a route does not use are 0. */
enum {
    ACEHIP_ROUTE_TILE = 0,    /* one grid of tile variant v_head (the variants of acehip_gemm_bf16_ex) */
    ACEHIP_ROUTE_SPLITK = 1,  /* splits x kper K-tiles of fp32 partials on 128 x bn tiles, then the epilogue */
    ACEHIP_ROUTE_STAGED = 2,  /* head-post: a 128 x 128 store grid into the workspace + the head_post kernel */
    ACEHIP_ROUTE_TAIL2 = 3,   /* rows [0, M1) on v_head, then rows [M1, M) on v_tail: two launches */
    ACEHIP_ROUTE_TAIL1 = 4,   /* the same split as nmain 256 x 256 + ntail 128 x 256 tiles of one launch */
    ACEHIP_ROUTE_WALK = 5     /* SwiGLU: those nmain + ntail tiles walked by `grid` persistent workgroups */
};
typedef struct acehip_gemm_plan {
    int route;
    int v_head, v_tail;       /* tile variants (v_tail: the tail split's second grid) */
    int M1;                   /* rows of the main grid (tail splits; the walk: M without a tail) */
    int nmain, ntail;         /* tiles of the main and the tail grid (tail splits, walk) */
    int grid;                 /* workgroups of the first (or only) launch; split-K: per split */
    int splits, kper;         /* split-K: splits of kper K-tiles (the last one may be shorter) */
    int bn, stages;           /* split-K: tile width (64 / 128) and operand ring depth */
    int deferred;             /* split-K: the residual epilogue is left to the consumer norm */
    int saddr;                /* the ping-pong launches issue their LDS-DMAs in the scalar-base form under
                                 ACEHIP_GEMM_SADDR alone (the one-launch head-post grid: 0 — it takes that
                                 form only with the slot-immediate loop, acehip_diag_pp_slotimm) */
    int helpers;              /* the tile runs with LDS-DMA helper waves */
} acehip_gemm_plan;

/* Host-only, for tests (no kernel launch): the plan of an [M, K] x [N, K]^T GEMM with epilogue
 * epi (0 store, 1 gated residual, 2 residual, 3 SwiGLU, 4 head-post), ws_bytes of split-K
 * workspace (0: none) and, with defer_ok, a caller that accepts a deferred residual epilogue —
 * under the ACEHIP_* switches of the environment (ACEHIP_GEMM_CUS included) on a device of
 * device_cus compute units (0: the current device's).  Shapes the dispatch refuses return
 * ACEHIP_E_ARG. */
int acehip_diag_gemm_plan(int M, int N, int K, int64_t lda, int64_t ldw, int epi, size_t ws_bytes, int defer_ok,
                          int device_cus, acehip_gemm_plan *out);

/* The launch acehip_attention_bf16 / acehip_attention_masked_bf16 and the runtimes' attention
 * layers give a shape: the value the library's dispatch plans before it launches
 * (csrc/attn_plan.h holds the rules).  Fields a route does not use are 0. */
enum {
    ACEHIP_ATTN_SMALL = 1,    /* attn_small_kernel: one head x 32 query rows per workgroup, `parts` KV parts per unit */
    ACEHIP_ATTN_PW = 2,       /* attn_pw_kernel: a GQA pair x 128 query rows, 64 rows per wave */
    ACEHIP_ATTN_FWD = 3       /* attn_fwd_kernel<nrep>: nrep heads x 128 query rows, 32 rows per wave */
};
typedef struct acehip_attn_plan {
    int kernel;               /* ACEHIP_ATTN_* */
    int nrep;                 /* query heads per workgroup */
    int window;               /* as launched: a band at least as wide as the sequence has become -1 (full) */
    int units, unit_tiles;    /* work units (a workgroup's heads x its query rows) and KV tiles of 64 keys per unit */
    int full, nsplit;         /* pw / fwd: units [0, full) run whole, each later one as nsplit KV-range parts
                                 (tail split: 0 < full < units; short split: full 0; whole units: full = units, nsplit 1) */
    int parts;                /* small: KV parts per unit */
    int grid, block;          /* workgroups and threads per workgroup of the launch */
    int persist;              /* pw: `grid` persistent workgroups walk the units */
    int streamk;              /* fwd: `grid` workgroups share the sk_total = units x sk_nt concatenated KV tiles */
    int sk_nt, sk_total;
    int causal;               /* window is -2: keys j <= i */
    int uses_ws;              /* the launch gets the ticket and slab pointers of the split workspace */
} acehip_attn_plan;

/* Host-only, for tests (no kernel launch): the plan of q [B,H,Sq,128] x k/v [B,KV,Sk,128] with
 * `window` (as acehip_attention_bf16), with a key-padding mask if masked and with the split
 * workspace if have_ws (the standalone entries and the runtimes always pass one) — under the
 * ACEHIP_ATTN_* switches of the environment (ACEHIP_ATTN_CUS included) on a device of device_cus
 * compute units (0: the current device's).  Shapes the dispatch refuses (and empty ones, which it
 * skips) return ACEHIP_E_ARG. */
int acehip_diag_attn_plan(int B, int H, int KV, int Sq, int Sk, int window, int masked, int have_ws,
                          int device_cus, acehip_attn_plan *out);

/* A residual GEMM and the norm that consumes it, as the DiT layer issues the pair (tests):
 *   X[0:M] = residual epilogue (as above, in place, N = ldc = D) of A[M,K] · W[D,K]^T
 *   X[from:M_norm] = bf16(X + v[D])                         (v != NULL; M <= from <= M_norm)
 *   out[0:M_norm] = acehip_rmsnorm_bf16(X, w, shift, scale, mod_bstride, rows_per_batch)
 * rows_per_batch is both the gate's and the modulation's batch size (> 0 when either is given), as
 * in the DiT layer; D % 256 == 0, D <= 4096; arguments are checked before X is written.
 * With defer != 0 a GEMM that takes the split-K path leaves its epilogue to the norm kernel,
 * which then applies it from the fp32 partials in the same pass (ACEHIP_SPLITK_FUSE=0: never);
 * *deferred (host int) reports whether it did.  X [M_norm][D] is updated in place either way. */
int acehip_gemm_res_norm_bf16(const void *A, int lda, const void *W, int ldw, void *X, int M, int D, int K,
                              const void *gate, int64_t gate_bstride, int rows_per_batch, int defer,
                              const void *w, const void *shift, const void *scale, int64_t mod_bstride,
                              void *out, int M_norm, float eps, const void *v, int from, int *deferred,
                              void *stream);

/* Flash attention, head_dim 128, GQA: q [B,H,Sq,128], k/v [B,KV,Sk,128] →
 * o [B,Sq,H*128]; window -1 = full, >= 0 |i-j| <= window, -2 = causal
 * (keys j <= i; the Qwen3 text encoder's default mask). */
int acehip_attention_bf16(const void *q, const void *k, const void *v, void *o, int B, int H,
                          int KV, int Sq, int Sk, int window, float scale, void *stream);
/* Same with a key-padding mask kmask uint8 [B, Sk] (1 = attend), encoder semantics. */
int acehip_attention_masked_bf16(const void *q, const void *k, const void *v, void *o, int B,
                                 int H, int KV, int Sq, int Sk, int window, float scale,
                                 const uint8_t *kmask, void *stream);

/* Normalised attention probabilities of selected heads, head_dim 128, GQA (single-kernel
 * entry for tests and profiling; the kernel behind acehip_dit_forward_capture):
 *   out[i][b][j - k0][s] = softmax_j(scale · q[b, heads[i], s, :] · k[b, heads[i] / (H/KV), j, :])
 * for j in [k0, k1), the softmax over all Sk keys (no mask), each value rounded to bf16
 * and stored as fp32.  q bf16 [B,H,Sq,128], k bf16 [B,KV,Sk,128] (16-byte aligned);
 * heads: host array of n (1..64) head indices; out: device fp32 [n][B][k1-k0][Sq]. */
int acehip_attention_probs_bf16(const void *q, const void *k, int B, int H, int KV, int Sq, int Sk,
                                const int *heads /*host, n*/, int n, int k0, int k1, float scale,
                                float *out /* [n][B][k1-k0][Sq] */, void *stream);

/* Single-token attention over a K/V cache, head_dim 128, GQA with H/KV in {1, 2, 4} (the
 * kernel behind acehip_enc_decode): q bf16 [B, H, 128]; k, v bf16 [B, KV, cap, 128] of which
 * rows [0, n) are valid (n <= cap); kmask uint8 [B, mask_ld >= n] (1 = attend) or NULL.
 *   o[b][h·128 + :] = Σ_j softmax_j(scale · q[b,h] · k[b, h/(H/KV), j]) · v[b, h/(H/KV), j]
 * over keys j < n with kmask[b][j] != 0; rows that are masked or past n are never used,
 * whatever they hold.  A row with no admissible key gives zeros.  ws: device scratch of
 * acehip_attention_decode_ws_bytes(B, H) bytes (key ranges are folded through it in range
 * order: bit-identical results from call to call) or NULL (one range per KV head). */
size_t acehip_attention_decode_ws_bytes(int B, int H);
int acehip_attention_decode_bf16(const void *q, const void *k, const void *v, void *o, int B, int H, int KV, int n,
                                 int cap, const uint8_t *kmask, int mask_ld, float scale, void *ws, size_t ws_bytes,
                                 void *stream);

/* Causal attention of n new queries per sequence over a K/V cache, head_dim 128, GQA with H/KV in
 * {1, 2, 4} (the kernel behind acehip_enc_extend): q bf16 [B, H, n, 128]; k, v bf16
 * [B, KV, cap, 128] of which rows [0, pos + n) are valid, the new tokens' rows [pos, pos + n)
 * already in place; kmask uint8 [B, mask_ld >= pos + n] over cache positions (1 = attend) or NULL.
 *   o[b·n + i][h·128 + :] = Σ_j softmax_j(scale · q[b,h,i] · k[b, h/(H/KV), j]) · v[b, h/(H/KV), j]
 * over keys j <= pos + i with kmask[b][j] != 0; fp32 softmax, P rounded to bf16 before P·V as
 * in acehip_attention_bf16.  Rows that are masked or at [pos + n, cap) are never used, whatever
 * they hold; a query with no admissible key gives zeros (acehip_attention_decode_bf16's rules).
 * ws: device scratch of acehip_attention_extend_ws_bytes(B, H, n) bytes, through which the key
 * ranges of a small grid are folded in range order — no atomics: bit-identical results from call
 * to call, at every split count — or NULL (one range per unit).  ACEHIP_E_ARG, nothing
 * launched: a null q / k / v / o, B or n < 1, pos < 0, pos + n > cap, H/KV outside {1, 2, 4},
 * mask_ld < pos + n with a mask, a workspace smaller than the plan needs. */
size_t acehip_attention_extend_ws_bytes(int B, int H, int n);
int acehip_attention_extend_bf16(const void *q, const void *k, const void *v, void *o, int B, int H, int KV, int n,
                                 int pos, int cap, const uint8_t *kmask, int mask_ld, float scale, void *ws,
                                 size_t ws_bytes, void *stream);

/* The launch acehip_attention_extend_bf16 gives a shape (csrc/attn_plan.h attn_extend_plan). */
typedef struct acehip_attn_extend_plan {
    int unit_rows;            /* stacked rows per workgroup: the H/KV heads of a KV head x unit_queries queries */
    int unit_queries;         /* 128 / (H/KV) */
    int qblocks, units;       /* query blocks per sequence; units = B x KV x qblocks */
    int tiles;                /* 64-key tiles of the pos + n keys (the last query block's loop) */
    int parts, tiles_per_part;/* key ranges per unit and tiles per range; (parts - 1) x tiles_per_part < tiles */
    int grid, block;          /* units x parts workgroups of 256 threads */
    int uses_ws;              /* parts > 1: partials go through the workspace and a fold launch */
} acehip_attn_extend_plan;
/* Host-only, for tests (no kernel launch): the plan of that call with a workspace if have_ws, on
 * device_cus compute units (0: the current device's; ACEHIP_ATTN_CUS replaces either), and in
 * *ws_need (or NULL) the bytes of partials the plan writes.  Shapes the entry refuses return
 * ACEHIP_E_ARG. */
int acehip_diag_attn_extend_plan(int B, int H, int KV, int n, int pos, int have_ws, int device_cus,
                                 acehip_attn_extend_plan *out, size_t *ws_need);

/* Vocabulary projection of the token loop (lm_head of a bf16 Qwen3ForCausalLM):
 * y[m][n] = bf16(Σ_k x[m][k] · W[n][k]), fp32 accumulate; M <= 16, any N, K % 8 == 0,
 * ldx % 8 == 0. */
int acehip_lm_head_bf16(const void *x, int ldx, const void *W, void *y, int ldy, int M, int N, int K, void *stream);

/* Top-k / top-p logit filters of the token loop, in place:
 * LLMHandler._apply_top_k_filter (acestep/llm_inference.py:367-372) and
 * LLMHandler._apply_top_p_filter (:374-385), without a sort.  logits: B rows of V values,
 * row stride ld >= V elements, dtype ACEHIP_F32 or ACEHIP_BF16; an entry keeps its bits or
 * becomes -inf of that dtype; columns [V, ld) are never written; -inf entries stay -inf.
 *   top_k in [1, V): entries below the k-th largest value (duplicates counted) are removed,
 *     ties at it are all kept; top_k <= 0 or >= V: off.
 *   top_p in (0, 1): with p = softmax(row) in fp32 and the entries ranked by value, descending
 *     (equal values: lower index first), rank 0 is kept and rank i >= 1 is kept iff the p of
 *     ranks < i sums to <= top_p; otherwise off.  The mass is a fixed-point integer sum: the
 *     same input gives the same bits on every call.
 * Both on: top-k, then top-p over the survivors (two calls).  A row with no finite entry is
 * left as it is.  NaN / +inf inputs are outside the contract (no fault, result unspecified).
 * ws: device scratch of acehip_lm_filter_ws_bytes(B, V) bytes, 8-byte aligned.  Caller's
 * stream, no allocation, no host sync.  ACEHIP_E_ARG (nothing launched): null pointer,
 * B < 1, V < 1 or V > 2^23, ld < V, another dtype, a smaller workspace. */
size_t acehip_lm_filter_ws_bytes(int B, int V);
int acehip_lm_filter(void *logits, int dtype, int ld, int B, int V, int top_k, float top_p, void *ws, size_t ws_bytes,
                     void *stream);

/* Teacher-forced scoring head (acestep/core/scoring/lm_score.py: _calculate_log_prob,
 * _calculate_topk_recall) without a [T, V] logits matrix.  With
 * logit[r][n] = bf16(Σ_k x[r][k]·W[n][k]) (fp32 accumulate, rounded to bf16 as a bf16 lm_head
 * does), per row r in [0, T):
 *   lse[r]       = log Σ_n exp(logit[r][n])               (fp32, max-subtracted)
 *   logprob[r]   = logit[r][target[r]] − lse[r]
 *   n_greater[r] = #{n : logit[r][n] >  logit[r][target[r]]}
 *   n_equal_lower[r] = #{n < target[r] : logit[r][n] == logit[r][target[r]]}
 * so the target's rank is 1 + n_greater + n_equal_lower (equal values: lower index first, the
 * rule of acehip_lm_filter).  x bf16 [T, ldx >= K], W bf16 [V, K], both 16-byte aligned; targets
 * device int32 [T]; outputs device fp32 / int32 [T].  A target outside [0, V): nothing is read
 * out of bounds, that row gets logprob = NaN and both counts −1 (its lse is still the row's).
 * The same input gives the same bits on every call.  ws: device scratch of
 * acehip_lm_score_ws_bytes(T, V) = (2·ceil(V/128) + 1)·T·4 bytes, 4-byte aligned.  Caller's
 * stream, no allocation, no host sync.  ACEHIP_E_ARG (nothing launched): null pointer, T < 1 or
 * T > 8192, V < 1 or V > 2^23, K % 64 != 0, ldx < K or ldx % 8 != 0, a smaller workspace. */
size_t acehip_lm_score_ws_bytes(int T, int V);
int acehip_lm_score_bf16(const void *x, int ldx, const void *W, const int32_t *targets, int T, int V, int K,
                         float *logprob, float *lse, int32_t *n_greater, int32_t *n_equal_lower, void *ws,
                         size_t ws_bytes, void *stream);

/* Qwen3RMSNorm (+ AdaLN modulation when shift/scale are given) over rows of D
 * (transformers modeling_qwen3.py:59-64; reference base:499,530,1496):
 * out = bf16(bf16(bf16(w·bf16(x·rsqrt(mean x²+eps)))·bf16(1+scale[b])) + shift[b]),
 * b = row / rows_per_batch, shift/scale rows mod_bstride apart.
 * rows_per_wave: 0 = default, 1/2/4 rows per wave, -2/-4 = 2/4 waves per row (tuning, tests). */
int acehip_rmsnorm_bf16(const void *x, const void *w, const void *shift, const void *scale,
                        int64_t mod_bstride, int rows_per_batch, void *out, int M, int D, float eps,
                        int rows_per_wave, void *stream);

/* Projection GEMM with the q/k RMSNorm + RoPE + head-major scatter epilogue
 * (reference base:300-345 q_proj/k_proj/v_proj → q_norm/k_norm → apply_rotary_pos_emb):
 * rows [B·S] of A · W[N,K]ᵀ, N = (nq+nk+nv)·128, split into heads q | k | v and written
 * to q [B,nq,S,128], k [B,nk,S,128], v [B,nv,S,128]; cos/sin [S,128] or NULL (no RoPE). */
int acehip_gemm_headpost_bf16(const void *A, int lda, const void *W, int K, int B, int S, int nq,
                              int nk, int nv, const void *qw, const void *kw, const void *cos,
                              const void *sin, float eps, void *q, void *k, void *v, void *stream);

/* Cross-attention of the DiT's conditional rows from the normed hidden states (tests, tools):
 * Q = q_norm(xn · wqᵀ) per head (no RoPE), AO = softmax(scale · Q Kᵀ) V over the cached k / v
 * [B,KV,Lenc,128]; xn [B·S,D], wq [H·128,D], qnw [128], ao token-major [B·S,H·128].
 * force = 1: the fused projection + attention launch wherever that kernel can run the shape
 * (H = 2·KV, B = 1 or S % 192 = 0), whatever the CU count; 0: the two launches it fuses (the
 * four-wave projection tile, then whole units on the forward attention kernel); −1: the DiT
 * forward's own choice (ACEHIP_CROSS_FUSE and the CU-count conditions).
 * *path = 1 if the fused launch ran, 0 if two launches did. */
int acehip_cross_attn_bf16(const void *xn, const void *wq, const void *qnw, const void *k, const void *v, void *ao,
                           int B, int S, int H, int KV, int Lenc, int D, float eps, float scale, int force,
                           int *path, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* ACEHIP_H */
