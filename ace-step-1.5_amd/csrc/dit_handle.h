// dit_handle.h — private to dit.hip and dit_f32.hip: the acehip_dit handle, the registration of
// the DiT's state-dict names (written once for both precisions) and the helpers the bf16 forward
// and the fp32 parity forward share.
#pragma once
#include <cmath>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "layer_args.h"
#include "weights.h"
#include "../../include/acehip.h"

struct acehip_dit {
    int device = 0;
    acehip_dit_cfg cfg{};
    std::vector<uint8_t> sliding;
    int D = 0, F = 0, qd = 0, kvd = 0, L = 0;
    bool finalized = false, have_cond = false;
    int cond_Bc = 0, cond_Lenc = 0;

    std::vector<void *> allocs;
    acehip::WeightTable weights;

    // weights
    bf16_t *tables = nullptr;   // [L][6][D]
    struct Layer {
        bf16_t *n_sa, *n_ca, *n_mlp, *wqkv, *wo, *qn, *kn, *cqn, *ckn, *wcq, *wckv, *wco, *wgu, *wdown;
    };
    std::vector<Layer> layers;
    bf16_t *sst_out, *win, *bin, *wce, *bce, *norm_out, *wout, *bout;
    bf16_t *te_l1[2], *te_b1[2], *te_l2[2], *te_b2[2], *te_tp[2], *te_btp[2];
    float *freqs = nullptr;          // [128] sinusoid frequencies
    std::vector<float> inv_freq_override;   // optional, [hd/2]
    bf16_t *attn_ws = nullptr;  // attention tail-split workspace (attention_ws_bytes())
    bf16_t *rope_cos = nullptr, *rope_sin = nullptr;   // [max_S][hd]

    // workspace
    bf16_t *X, *XN, *Qh, *Kh, *Vh, *AO, *Hb, *Xin, *O2;
    bf16_t *emb[2], *h1, *temb_e[2], *proj_e[2], *temb, *proj, *mod, *mod_out;
    bf16_t *Kc, *Vc, *E, *KVtmp;
    int kv_group = 1;                  // layers per cross-K/V GEMM at set_condition (KVtmp holds that many)
    bf16_t *wckv_all = nullptr;        // every layer's cross K/V projection, [L][2·kvd][D] (one GEMM)
    bf16_t *gemv_act = nullptr;        // 16 × D: bf16(silu(x)) rows of the timestep MLPs (gemv_small)
    // CFG null rows (acehip_dit_set_uniform_rows): batch rows >= uniform_from have an
    // encoder sequence that is one vector repeated, so their cross-attention is the
    // constant V row and their cross-O output the per-layer constant cnull[l]
    int uniform_from = 1 << 30;
    bf16_t *cnull = nullptr, *vnull = nullptr;   // [L][D], [q_dim]
    // timestep MLP outputs of a whole schedule (acehip_dit_set_timesteps): row i = step i's
    // temb [D] and proj [6D]; ts_scratch holds the batched MLP intermediates
    int ts_n = 0, ts_cap = 0;
    bf16_t *ts_temb = nullptr, *ts_proj = nullptr, *ts_scratch = nullptr;
    bf16_t *tmp = nullptr;   // weight staging (fp32 → bf16 casts): tmp_elems floats
    void *gemm_ws = nullptr;   // split-K partials for small-M GEMMs (short songs / turbo)
    size_t tmp_elems = 0;

    // optional per-kernel event timing (acehip_dit_profile)
    static constexpr int NKIND = 7, NPAIR = 16384;
    bool prof = false;
    unsigned prof_mask = 0x7f;         // kinds recorded while profiling (acehip_dit_profile_kinds)
    std::vector<hipEvent_t> ev;        // 2·NPAIR events
    std::vector<int> ev_kind;          // kind of each recorded pair
    int ev_used = 0;

    // HIP graph of the forward's pointer-independent middle (acehip_dit_set_graph): the
    // timestep MLPs, modulation, proj_in and the layer stack read and write only handle
    // buffers, so one capture per (Bc, S, Lenc, uniform_from) replays for every step
    bool graph_on = false;
    hipStream_t cap_stream = nullptr;
    hipGraphExec_t gexec = nullptr;
    int gkey[6] = {-1, -1, -1, -1, -1, -1};

    // fp32 parity mode (acehip_dit_cfg.fp32): fp32 weights and workspace,
    // the kernels of f32.hip (dit_f32.hip); the bf16 buffers above are not allocated
    bool f32 = false;
    struct F32 {
        struct Layer {
            float *n_sa, *n_ca, *n_mlp, *wqkv, *wo, *qn, *kn, *cqn, *ckn, *wcq, *wckv, *wco, *wg, *wu, *wdown;
        };
        std::vector<Layer> layers;
        float *tables, *sst_out, *win, *bin, *wce, *bce, *norm_out, *wout, *bout;
        float *te_l1[2], *te_b1[2], *te_l2[2], *te_b2[2], *te_tp[2], *te_btp[2];
        float *rope_cos, *rope_sin;
        float *X, *XN, *QKV, *Qh, *Kh, *Vh, *AO, *G, *U, *Hb, *Xin, *O2;
        float *emb[2], *h1, *temb_e[2], *proj_e[2], *temb, *proj, *mod, *mod_out;
        float *Kc, *Vc, *E, *KVtmp;
    } f{};
};

// the parity mode (dit_f32.hip) behind the public entries of dit.hip
int dit_create_f32(acehip_dit *h);
int dit_build_rope_f32(acehip_dit *h);
int dit_set_condition_f32(acehip_dit *h, const float *enc, int Bc, int Lenc, hipStream_t s);
int dit_forward_f32(acehip_dit *h, const float *xt, const float *ctx, int Bx, const float *t, const float *t_r,
                    int t_stride, int Bc, int T, float *vt_out, hipStream_t s,
                    const acehip_attn_capture *cap = nullptr);

namespace acehip {

// where a layer's gate_proj / up_proj go.  The one difference between the precisions' tables:
// bf16 interleaves both into the SwiGLU panels of wgu, fp32 keeps the reference's two matrices.
template <class T>
struct GateUpDst {
    T *gate;
    Pack gate_kind;
    T *up;
    Pack up_kind;
};

// Every state-dict name of AceStepDiTModel (reference shapes) with its destination in `w`: the
// handle itself (bf16) or its F32 part, which name their weights alike.
template <class W, class GateUp>
void register_dit_weights(WeightTable &t, const W &w, int L, int D, int F, int qd, int kvd, GateUp gate_up) {
    for (int i = 0; i < L; ++i) {
        const auto &ly = w.layers[i];
        const std::string p = "layers." + std::to_string(i);
        t.add(p + ".scale_shift_table", w.tables + (size_t)i * 6 * D, {1, 6, D});
        t.add(p + ".self_attn_norm.weight", ly.n_sa, {D});
        t.add(p + ".cross_attn_norm.weight", ly.n_ca, {D});
        t.add(p + ".mlp_norm.weight", ly.n_mlp, {D});
        t.add(p + ".self_attn.q_proj.weight", ly.wqkv, {qd, D});
        t.add(p + ".self_attn.k_proj.weight", ly.wqkv + (size_t)qd * D, {kvd, D});
        t.add(p + ".self_attn.v_proj.weight", ly.wqkv + (size_t)(qd + kvd) * D, {kvd, D});
        t.add(p + ".self_attn.o_proj.weight", ly.wo, {D, qd});
        t.add(p + ".self_attn.q_norm.weight", ly.qn, {128});
        t.add(p + ".self_attn.k_norm.weight", ly.kn, {128});
        t.add(p + ".cross_attn.q_proj.weight", ly.wcq, {qd, D});
        t.add(p + ".cross_attn.k_proj.weight", ly.wckv, {kvd, D});
        t.add(p + ".cross_attn.v_proj.weight", ly.wckv + (size_t)kvd * D, {kvd, D});
        t.add(p + ".cross_attn.o_proj.weight", ly.wco, {D, qd});
        t.add(p + ".cross_attn.q_norm.weight", ly.cqn, {128});
        t.add(p + ".cross_attn.k_norm.weight", ly.ckn, {128});
        const auto gu = gate_up(ly);
        t.add(p + ".mlp.gate_proj.weight", gu.gate, {F, D}, gu.gate_kind);
        t.add(p + ".mlp.up_proj.weight", gu.up, {F, D}, gu.up_kind);
        t.add(p + ".mlp.down_proj.weight", ly.wdown, {D, F});
    }
    const char *te_names[2] = {"time_embed", "time_embed_r"};
    for (int e = 0; e < 2; ++e) {
        const std::string p = te_names[e];
        t.add(p + ".linear_1.weight", w.te_l1[e], {D, 256});
        t.add(p + ".linear_1.bias", w.te_b1[e], {D});
        t.add(p + ".linear_2.weight", w.te_l2[e], {D, D});
        t.add(p + ".linear_2.bias", w.te_b2[e], {D});
        t.add(p + ".time_proj.weight", w.te_tp[e], {6 * D, D});
        t.add(p + ".time_proj.bias", w.te_btp[e], {6 * D});
    }
    t.add("scale_shift_table", w.sst_out, {1, 2, D});
    t.add("proj_in.1.weight", w.win, {D, 192, 2}, Pack::PROJ_IN);
    t.add("proj_in.1.bias", w.bin, {D});
    t.add("condition_embedder.weight", w.wce, {D, D});
    t.add("condition_embedder.bias", w.bce, {D});
    t.add("norm_out.weight", w.norm_out, {D});
    t.add("proj_out.1.weight", w.wout, {D, 64, 2}, Pack::PROJ_OUT_W);
    t.add("proj_out.1.bias", w.bout, {64}, Pack::PROJ_OUT_B);
}

// record an event pair around `launch` when profiling is on
template <class F>
int timed(acehip_dit *h, int kind, hipStream_t s, F &&launch) {
    if (!h->prof || !((h->prof_mask >> kind) & 1u) || h->ev_used >= acehip_dit::NPAIR) return launch();
    const int i = h->ev_used++;
    h->ev_kind[i] = kind;
    if (kind == 0) {
        // the SwiGLU GEMM (the bench's roofline kernel, timed inside the measured song): the
        // events ride on its launches (gemm_ext_events) instead of two event packets that
        // would idle the GPU ≈ 5.6 µs each; a path without launch events drops the sample
        gemm_ext_events(h->ev[2 * i], h->ev[2 * i + 1]);
        const int rc = launch();
        if (!gemm_ext_events(nullptr, nullptr)) h->ev_kind[i] = -1;
        return rc;
    }
    HIP_TRY(hipEventRecord(h->ev[2 * i], s));
    const int rc = launch();
    HIP_TRY(hipEventRecord(h->ev[2 * i + 1], s));
    return rc;
}

// the capture's entries of layer l (heads + their output slots); returns how many
inline int capture_layer(const acehip_attn_capture *cap, int l, AttnProbsSel &sel) {
    sel.n = 0;
    for (int i = 0; i < cap->n; ++i)
        if (cap->layer[i] == l) {
            sel.head[sel.n] = (int16_t)cap->head[i];
            sel.slot[sel.n] = (int16_t)i;
            ++sel.n;
        }
    return sel.n;
}
inline int capture_last_layer(const acehip_attn_capture *cap) {
    int last = 0;
    for (int i = 0; i < cap->n; ++i) last = std::max(last, cap->layer[i]);
    return last;
}

}  // namespace acehip
