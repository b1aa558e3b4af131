"""Cross-attention map capture (``acehip_dit_forward_capture``) and the lyric-alignment
drop-ins built on it.

Goldens: ``tests/golden/lyric_attn_{float32,bfloat16}`` — the reference decoder driven as the
lyric handlers drive it (``output_attentions=True, custom_layers_config, enable_early_exit``),
its selected maps ``[n, B, k1-k0, S]`` and ``vt`` (tools/record_lyric_attn.py; full width, 4
layers, B = 2 with t = [1.0, 0.125], T = 250, Lenc = 77, keys [5, 61), selection
{1: [3, 10], 2: [0], 3: [15, 8]}).  The recorder asserts the maps are far from the uniform
1/Lenc (rel-L2 1.29 in units of the uniform map's norm), so a kernel writing a constant cannot pass.

rel-L2 over the selected maps, measured on MI355X next to its bar:
  fp32 handle: measured 1.896e-06, bar = min(10 × measured, 1e-4) = 1.896e-05
  bf16 handle: measured 7.749e-03, bar = min(2 × measured, 2.5 %) = 1.550e-02
(vt of the same runs vs the reference: 1.914e-06 fp32, 8.203e-03 bf16; the uniform 1/Lenc map
is 0.787 away from the reference maps in the same norm, 50 × the bf16 bar.)
"""
import ctypes
import json
import os
from types import SimpleNamespace

import pytest
import torch

from conftest import GOLDEN, load_golden, rel_l2

from acehip.config import DiTConfig
from acehip.weights import synth_dit_weights, synth_encoder_states, synth_null_condition

pytestmark = pytest.mark.gpu

MEASURED_FP32 = 1.896e-06      # MI355X, fp32 handle vs lyric_attn_float32
MEASURED_BF16 = 7.749e-03      # MI355X, bf16 handle vs lyric_attn_bfloat16
BAR = {"float32": min(10 * MEASURED_FP32, 1e-4), "bfloat16": min(2 * MEASURED_BF16, 0.025)}
VT_TOL = {"float32": 1e-4, "bfloat16": 0.025}      # the forward's own bars (test_gpu_fp32 / test_gpu_dit)


def _manifest():
    with open(os.path.join(GOLDEN, "lyric_attn_manifest.json")) as f:
        return json.load(f)


def _config(meta):
    return {int(k): list(v) for k, v in meta["layers_config"].items()}


@pytest.fixture(scope="module")
def weights():
    meta = _manifest()
    cfg = DiTConfig(**meta["cfg"])
    W = synth_dit_weights(cfg, seed=meta["weights_seed"], mode="parity", workers=8)
    cs = float(sum(float(v.double().abs().sum()) for v in W.values()))
    assert abs(cs - meta["weights_checksum"]) <= 1e-9 * meta["weights_checksum"], "synthetic weights drifted"
    return cfg, W


@pytest.fixture(scope="module", params=["float32", "bfloat16"])
def captured(request, gpu_device, weights):
    """One handle per dtype and every run the tests below compare, computed once."""
    from acehip.dit import DiTRuntime, config_pairs
    tag = request.param
    dtype = getattr(torch, tag)
    meta = _manifest()
    cfg, W = weights
    g = load_golden("lyric_attn_" + tag)
    enc = synth_encoder_states(cfg, meta["B"], meta["Lenc"], seed=meta["enc_seed"], gain=meta["enc_gain"]).to(dtype)
    cs = meta["fixtures"][tag]["enc_checksum"]        # summation order may differ between hosts: 1e-9 relative
    assert abs(float(enc.double().abs().sum()) - cs) <= 1e-9 * cs, "encoder input drifted"
    dev = gpu_device
    rt = DiTRuntime(cfg, dev.index or 0, max_S=128, max_Bc=meta["B"], max_Lenc=96, dtype=dtype)
    rt.load({k: v.to(dev, dtype) for k, v in W.items()})
    rt.set_condition(enc.to(dev))
    xt, ctx = g["xt"].to(dev).contiguous(), g["ctx"].to(dev).contiguous()
    t = g["t"].float().to(dev)
    pairs = config_pairs(_config(meta))
    k0, k1 = meta["k0"], meta["k1"]
    vt_plain = rt.forward(xt, ctx, t)
    maps_full, vt_cap = rt.forward_capture(xt, ctx, t, pairs, k0, k1, stop_early=False)
    maps_stop, vt_none = rt.forward_capture(xt, ctx, t, pairs, k0, k1, stop_early=True)
    vt_after = rt.forward(xt, ctx, t)
    torch.cuda.synchronize()
    assert vt_none is None
    out = SimpleNamespace(tag=tag, meta=meta, g=g, rt=rt, xt=xt, ctx=ctx, t=t, pairs=pairs,
                          vt_plain=vt_plain.cpu(), vt_cap=vt_cap.cpu(), vt_after=vt_after.cpu(),
                          maps_full=maps_full.cpu(), maps_stop=maps_stop.cpu())
    yield out
    rt.close()


def test_maps_vs_reference_golden(captured):
    c = captured
    ref = c.g["maps"].float()
    assert c.maps_stop.dtype == torch.float32 and c.maps_stop.shape == ref.shape
    r = rel_l2(c.maps_stop, ref)
    uniform = rel_l2(torch.full_like(ref, 1.0 / c.meta["Lenc"]), ref)
    print(f"lyric_attn {c.tag}: maps rel-L2 vs reference = {r:.3e} (bar {BAR[c.tag]:.3e}); "
          f"uniform 1/Lenc map = {uniform:.3f}")
    assert torch.isfinite(c.maps_stop).all()
    assert r <= BAR[c.tag], (c.tag, r)
    if c.tag == "bfloat16":           # rounded to bf16 before the fp32 store
        assert torch.equal(c.maps_stop, c.maps_stop.bfloat16().float())


def test_capture_leaves_forward_bit_identical(captured):
    c = captured
    assert torch.equal(c.vt_cap, c.vt_plain)            # stop_after_last = 0: the same vt
    assert torch.equal(c.maps_stop, c.maps_full)        # stop_after_last = 1, vt_out = NULL: the same maps
    assert torch.equal(c.vt_after, c.vt_plain)          # a following plain forward is untouched
    r = rel_l2(c.vt_after, c.g["vt"])
    print(f"lyric_attn {c.tag}: vt rel-L2 vs reference = {r:.3e}")
    assert r <= VT_TOL[c.tag], (c.tag, r)


def _raw_capture(c, layers, heads, k0, k1, stop, vt=True, n=None):
    from acehip import _ffi
    rt = c.rt
    n_real = max(len(layers), 1)
    la, ha = (ctypes.c_int * n_real)(*layers), (ctypes.c_int * n_real)(*heads)
    Bc, T = c.meta["B"], c.meta["T"]
    maps = torch.zeros(max(len(layers), 1) * Bc * 96 * 128, device=c.xt.device)
    out = torch.empty(Bc, T, 64, device=c.xt.device, dtype=rt.dtype) if vt else None
    cap = _ffi.AttnCapture(n=len(layers) if n is None else n, layer=la, head=ha, k0=k0, k1=k1,
                           out=ctypes.cast(maps.data_ptr(), ctypes.POINTER(ctypes.c_float)),
                           stop_after_last=1 if stop else 0)
    dt = _ffi.ACEHIP_F32 if rt.dtype == torch.float32 else _ffi.ACEHIP_BF16
    rc = _ffi.lib().acehip_dit_forward_capture(rt.h, _ffi.ptr(c.xt), _ffi.ptr(c.ctx), Bc, _ffi.ptr(c.t), _ffi.ptr(c.t),
                                               1, Bc, T, dt, _ffi.ptr(out), ctypes.byref(cap), _ffi.stream_ptr())
    torch.cuda.synchronize()
    return rc, (_ffi.lib().acehip_last_error() or b"").decode()


def test_capture_argument_and_state_errors(captured):
    c = captured
    Lenc, L, H = c.meta["Lenc"], 4, 16
    assert _raw_capture(c, [1], [3], 5, 61, True, vt=False)[0] == 0
    for kw in (dict(layers=[L], heads=[0]), dict(layers=[-1], heads=[0]),            # layer
               dict(layers=[1], heads=[H]), dict(layers=[1], heads=[-1]),            # head
               dict(layers=[1], heads=[0], k0=-1), dict(layers=[1], heads=[0], k0=9, k1=9),
               dict(layers=[1], heads=[0], k1=Lenc + 1),                             # key range
               dict(layers=[1], heads=[0], n=0), dict(layers=[1], heads=[0], n=65),  # n
               dict(layers=[1], heads=[0], stop=False, vt=False)):                   # NULL vt without stop
        a = dict(layers=None, heads=None, k0=5, k1=61, stop=True, vt=True, n=None)
        a.update(kw)
        rc, msg = _raw_capture(c, a["layers"], a["heads"], a["k0"], a["k1"], a["stop"], vt=a["vt"], n=a["n"])
        assert rc == -1 and msg, (kw, rc, msg)
    if c.tag == "bfloat16":      # uniform rows: the skipped rows' maps do not exist
        c.rt.set_uniform_rows(1)
        rc, msg = _raw_capture(c, [1], [3], 5, 61, True)
        assert rc == -4 and "uniform" in msg, (rc, msg)
        c.rt.set_uniform_rows(c.meta["B"])
        assert _raw_capture(c, [1], [3], 5, 61, True)[0] == 0


# ---------------------------------------------------------------- install() ----
def _small_cfg():
    return DiTConfig(hidden_size=256, intermediate_size=512, num_hidden_layers=2, num_attention_heads=2,
                     num_key_value_heads=1, head_dim=128, sliding_window=8)


def _module_tree(sd):
    root = torch.nn.Module()
    for name, t in sd.items():
        *path, leaf = name.split(".")
        m = root
        for p in path:
            if p not in m._modules:
                m.add_module(p, torch.nn.Module())
            m = m._modules[p]
        m.register_parameter(leaf, torch.nn.Parameter(t, requires_grad=False))
    return root


class _Model(torch.nn.Module):
    def __init__(self, cfg, dev):
        super().__init__()
        W = {k: v.to(dev, torch.bfloat16) for k, v in synth_dit_weights(cfg, seed=71, mode="parity").items()}
        self.decoder = _module_tree(W)
        self.null_condition_emb = torch.nn.Parameter(synth_null_condition(cfg, seed=72).to(dev, torch.bfloat16),
                                                     requires_grad=False)
        self.config = SimpleNamespace(**cfg.__dict__, is_turbo=False, model_version="base")

    def prepare_condition(self, **kw):
        raise AssertionError("prepare_condition is not part of the lyric seam")

    def generate_audio(self, **kw):
        raise AssertionError("generate_audio is not part of the lyric seam")


HEADER_LEN, N_LYRIC = 3, 9


class _Tokenizer:
    def encode(self, text, add_special_tokens=False):
        return list(range(HEADER_LEN))


class _Handler:
    """Handler-shaped fake: the helpers the drop-ins call, and originals that only report."""
    custom_layers_config = {1: [1, 0], 0: [1]}

    def __init__(self, dev):
        self.device, self.dtype = str(dev), torch.bfloat16
        self.model = _Model(_small_cfg(), dev)
        self.vae = self.text_encoder = None
        self.text_tokenizer = _Tokenizer()

    def _resolve_custom_layers_config(self, c):
        return self.custom_layers_config if c is None else c

    def _move_alignment_inputs_to_runtime(self, pred_latent, encoder_hidden_states, encoder_attention_mask,
                                          context_latents):
        return tuple(x.to(device=self.device, dtype=self.dtype)
                     for x in (pred_latent, encoder_hidden_states, encoder_attention_mask, context_latents))

    def _sample_noise_like(self, reference, seed):
        g = torch.Generator(device=reference.device).manual_seed(int(seed))
        return torch.randn(reference.shape, generator=g, device=reference.device, dtype=reference.dtype)

    def _extract_lyric_segment(self, lyric_token_ids, vocal_language):
        ids = lyric_token_ids[0].tolist()
        start = len(self.text_tokenizer.encode(vocal_language))
        return ids, ids[start:start + N_LYRIC], start, start + N_LYRIC

    def _lyric_timestamp_error(self, message):
        return {"success": False, "error": message, "lrc_text": ""}

    def _lyric_score_error(self, message):
        return {"success": False, "error": message, "lm_score": 0.0, "dit_score": 0.0}

    def get_lyric_timestamp(self, *a, **k):
        return {"original": "timestamp"}

    def get_lyric_score(self, *a, **k):
        return {"original": "score"}


class _Recorder:
    """Aligner / scorer stand-in: keeps what it was handed."""

    def __init__(self, tokenizer):
        self.calls = []

    def stamps_align_info(self, attention_matrix, lyrics_tokens, total_duration_seconds, custom_config, **kw):
        self.calls.append((attention_matrix, custom_config, lyrics_tokens))
        return {"calc_matrix": attention_matrix}

    def get_timestamps_and_lrc(self, calc_matrix, lyrics_tokens, total_duration_seconds):
        return {"lrc_text": "[00:00.00]x", "sentence_timestamps": [1], "token_timestamps": [2]}

    def lyrics_alignment_info(self, attention_matrix, token_ids, custom_config, **kw):
        self.calls.append((attention_matrix, custom_config, token_ids))
        return {"energy_matrix": attention_matrix, "type_mask": None, "path_coords": None}

    def calculate_score(self, energy_matrix, type_mask, path_coords):
        return {"lyrics_score": float(energy_matrix.sum())}


def test_install_rebinds_lyric_methods(gpu_device):
    from acehip.alignment import compact_maps
    from acehip.integration import install
    dev = gpu_device
    h = _Handler(dev)
    out = install(h, max_seconds=4.0, max_batch=2, vae=False, condition=False, text_encoder=False)
    la, dit = out["lyric_alignment"], out["dit"]
    assert h.get_lyric_timestamp == la.get_lyric_timestamp and h.get_lyric_score == la.get_lyric_score
    recs = []

    def factory(tok):
        recs.append(_Recorder(tok))
        return recs[-1]
    la.stamps_aligner = la.scorer = factory
    seen = []
    real = dit.cross_attention_maps

    def spy(xt, t, enc, ctx, layers_config, k0, k1, stop_early=True):
        seen.append(SimpleNamespace(xt=xt.clone(), t=torch.as_tensor(t).clone(), enc=enc, ctx=ctx,
                                    config=layers_config, k0=k0, k1=k1, stop=stop_early))
        return real(xt, t, enc, ctx, layers_config, k0, k1, stop_early=stop_early)
    dit.cross_attention_maps = spy

    g = torch.Generator().manual_seed(5)
    T, Lenc, steps, seed = 50, 20, 8, 42
    S = T // 2
    pred = torch.randn(1, T, 64, generator=g)
    enc = 2.0 * torch.randn(1, Lenc, 256, generator=g)
    mask = torch.ones(1, Lenc)
    ctx = torch.randn(1, T, 128, generator=g)
    ids = torch.arange(100, 100 + Lenc).reshape(1, Lenc)
    start, end = HEADER_LEN, HEADER_LEN + N_LYRIC
    cfgd = _Handler.custom_layers_config
    t_last = 1.0 / steps
    pb = pred.to(dev, torch.bfloat16)
    noise = h._sample_noise_like(pb, seed)
    xt = t_last * noise + (1.0 - t_last) * pb

    # ---- timestamps
    res = h.get_lyric_timestamp(pred, enc, mask, ctx, ids, 2.0, inference_steps=steps, seed=seed)
    assert res["success"] and res["error"] is None and res["lrc_text"] == "[00:00.00]x", res
    assert res["sentence_timestamps"] == [1] and res["token_timestamps"] == [2]
    (matrix, remapped, tokens), = recs[-1].calls
    assert matrix.dtype == torch.float32 and tuple(matrix.shape) == (2, 2, end - start, S)
    assert remapped == {0: [0, 1], 1: [0]} and list(remapped) == [0, 1]
    assert tokens == list(range(100 + start, 100 + end))
    call = seen[-1]
    assert torch.equal(call.xt, xt) and call.t.tolist() == [t_last] and call.stop and (call.k0, call.k1) == (start, end)
    assert call.config == cfgd and list(call.config) == [1, 0]
    want = real(xt, torch.tensor([t_last]), enc, ctx, cfgd, start, end)          # [3, 1, tokens, S]
    assert tuple(want.shape) == (3, 1, end - start, S)
    assert torch.equal(matrix, compact_maps(want[:, 0], cfgd))
    assert torch.equal(matrix[0, 0], want[0, 0]) and torch.equal(matrix[0, 1], want[1, 0])      # layer 1: heads 1, 0
    assert torch.equal(matrix[1, 0], want[2, 0]) and not matrix[1, 1].any()                     # layer 0: head 1, pad
    assert torch.isfinite(want).all() and float(want.max()) > 0.0

    # ---- score: rows [noise; xt] at t = [1.0, t_last]
    n_seen = len(seen)
    res = h.get_lyric_score(pred, enc, mask, ctx, ids, inference_steps=steps, seed=seed)
    assert res["success"] and res["error"] is None, res
    assert len(seen) == n_seen + 1
    call = seen[-1]
    assert call.t.tolist() == [1.0, t_last]
    assert torch.equal(call.xt[0:1], noise) and torch.equal(call.xt[1:2], xt)
    assert call.enc.shape[0] == 2 and torch.equal(call.enc[0], call.enc[1]) and torch.equal(call.ctx[0], call.ctx[1])
    (m_lm, c_lm, _), (m_dit, c_dit, _) = recs[-1].calls
    assert c_lm == c_dit == {0: [0, 1], 1: [0]}
    both = real(call.xt, call.t, call.enc, call.ctx, cfgd, start, end)           # [3, 2, tokens, S]
    assert torch.equal(m_lm, compact_maps(both[:, 0], cfgd)) and torch.equal(m_dit, compact_maps(both[:, 1], cfgd))
    assert tuple(m_lm.shape) == (2, 2, end - start, S) and not torch.equal(m_lm, m_dit)
    assert res["lm_score"] == float(m_lm.sum()) and res["dit_score"] == float(m_dit.sum())

    # ---- bsz = 2 reaches the original methods
    two = lambda x: torch.cat([x, x])       # noqa: E731
    assert h.get_lyric_timestamp(two(pred), two(enc), two(mask), two(ctx), ids, 2.0) == {"original": "timestamp"}
    assert h.get_lyric_score(two(pred), two(enc), two(mask), two(ctx), ids) == {"original": "score"}
    # ---- an error inside the path becomes the handler's error payload (no fallback)
    bad = h.get_lyric_timestamp(pred, enc, mask, ctx, ids, 2.0, inference_steps=0)
    assert bad["success"] is False and "inference_steps" in bad["error"]
    dit.rt.close()
