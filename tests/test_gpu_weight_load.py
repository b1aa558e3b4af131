"""Weight loading of the model handles (csrc/weights.h behind acehip_dit_set_weight,
acehip_enc_set_weight and acehip_vae_set_weight): what a handle stores must not depend on how
the caller hands a tensor over.  The same weights are loaded as fp32 or bf16, from the host or
the device, into otherwise identical handles, and one forward of each must agree bit for bit:
the fp32 -> bf16 rounding is the same on every route (device cast, host repack), and no route
drops, truncates or misplaces part of a tensor relative to the others.  The fp32 weights are
random draws, so they are not bf16-representable and the rounding is exercised.

What this does not show: every route shares one gate/up packing and one set of patch-conv index
maps, so a wrong map would still agree with itself here.  Where each element belongs is checked
by the parity tests against the oracle (test_gpu_dit.py, test_gpu_fp32.py, test_gpu_condenc.py,
test_vae.py).

The error cases all return before any kernel launch.  They also pin the two texts the shared
loader changed: the encoder's shape mismatch lists the got / want shapes like the DiT's, and
an unsupported dtype code is refused with the handle's prefix and the weight's name (the
three handles' earlier texts, "dtype", "enc_set_weight: dtype" and "vae_set_weight: dtype",
named no weight).  Every other assertion here also holds on the library before that change."""
import math

import pytest
import torch

from acehip import _ffi as ff
from acehip.config import DiTConfig, VAEConfig
from acehip.weights import encoder_stack_shapes, synth_dit_weights, synth_vae_weights, synth_weights

pytestmark = pytest.mark.gpu

E_ARG, E_STATE, E_NAME = -1, -4, -5


def _five_ways(W, dev):
    """fp32 / bf16 / bf16 widened back to fp32, on the host and on the device"""
    bf = {k: v.bfloat16() for k, v in W.items()}
    return {"f32_host": W, "f32_dev": {k: v.to(dev) for k, v in W.items()},
            "bf16_host": bf, "bf16_dev": {k: v.to(dev) for k, v in bf.items()},
            "bf16_as_f32_host": {k: v.float() for k, v in bf.items()}}


def _assert_all_equal(outs, int_dtype):
    names = list(outs)
    ref = outs[names[0]]
    assert bool(torch.isfinite(ref.float()).all()) and float(ref.float().abs().max()) > 0
    for n in names[1:]:
        assert outs[n].shape == ref.shape
        assert torch.equal(outs[n].view(int_dtype), ref.view(int_dtype)), f"{n} differs from {names[0]}"


def _not_bf16(W):
    return all(not torch.equal(v, v.bfloat16().float()) for v in W.values() if v.numel() >= 64)


# ------------------------------------------------------------------------------- DiT ---
DIT_CFG = DiTConfig.tiny(layers=1)
T_ODD, LENC = 47, 20


@pytest.fixture(scope="module")
def dit_w():
    W = synth_dit_weights(DIT_CFG, seed=21, mode="parity")
    assert _not_bf16(W)
    return W


@pytest.fixture(scope="module")
def dit_inputs():
    g = torch.Generator().manual_seed(9)
    return (torch.randn(1, T_ODD, 64, generator=g), torch.randn(1, T_ODD, 128, generator=g),
            torch.randn(2, LENC, DIT_CFG.hidden_size, generator=g))


def _dit_runtime(dev, dtype):
    from acehip.dit import DiTRuntime
    return DiTRuntime(DIT_CFG, dev.index or 0, max_S=64, max_Bc=2, max_Lenc=32, dtype=dtype)


def _dit_load(rt, W, skip=()):
    """DiTRuntime.load, but every second key keeps a ``decoder.`` prefix for the library to strip"""
    hd = DIT_CFG.head_dim
    rt.set_weight("_timestep_freqs", torch.exp(-math.log(10000) * torch.arange(0, 128, dtype=torch.float32) / 128))
    rt.set_weight("_rope_inv_freq", 1.0 / (DIT_CFG.rope_theta ** (torch.arange(0, hd, 2, dtype=torch.float) / hd)))
    for i, (k, v) in enumerate(W.items()):
        if k not in skip:
            rt.set_weight("decoder." + k if i % 2 else k, v)


def _dit_forward(dev, dtype, W, inputs):
    xt, ctx, enc = (x.to(dev, dtype) for x in inputs)
    rt = _dit_runtime(dev, dtype)
    _dit_load(rt, W)
    ff.check(ff.lib().acehip_dit_finalize(rt.h), "dit_finalize")
    rt.set_condition(enc)
    out = rt.forward(xt, ctx, torch.tensor([0.625], dtype=torch.float32, device=dev))
    torch.cuda.synchronize()
    out = out.cpu()
    rt.close()
    return out


def test_dit_bf16_load_routes_bit_equal(gpu_device, dit_w, dit_inputs):
    """plain copies, gate/up through the staging buffer, the patch-conv repacks; fp32 and bf16 input"""
    outs = {n: _dit_forward(gpu_device, torch.bfloat16, W, dit_inputs) for n, W in _five_ways(dit_w, gpu_device).items()}
    assert outs["f32_host"].shape == (2, T_ODD, 64)
    _assert_all_equal(outs, torch.int16)


def test_dit_fp32_load_routes_bit_equal(gpu_device, dit_w, dit_inputs):
    """the parity mode stores fp32: bf16 input and its fp32 widening are the same numbers"""
    ways = _five_ways(dit_w, gpu_device)
    ways = {"bf16_host": ways["bf16_host"], "bf16_dev": ways["bf16_dev"], "bf16_as_f32_host": ways["bf16_as_f32_host"],
            "bf16_as_f32_dev": {k: v.to(gpu_device) for k, v in ways["bf16_as_f32_host"].items()}}
    outs = {n: _dit_forward(gpu_device, torch.float32, W, dit_inputs) for n, W in ways.items()}
    _assert_all_equal(outs, torch.int32)


# --------------------------------------------------------------------------- encoder ---
ENC_CFG = DiTConfig(hidden_size=256, intermediate_size=512, num_hidden_layers=2, num_attention_heads=2,
                    num_key_value_heads=2, head_dim=128, sliding_window=8)
ENC_B, ENC_S = 2, 40


def _enc_stack():
    from acehip.condition import EncoderStack
    return EncoderStack(ENC_CFG, 2, 64, embed_bias=True, out_dim=64, device=0, max_tokens=ENC_B * ENC_S, max_S=ENC_S)


@pytest.fixture(scope="module")
def enc_w():
    W = synth_weights(encoder_stack_shapes(ENC_CFG, "s", 2, 64, True, out_dim=64), 11, "parity")
    assert _not_bf16(W)
    return W


def test_encoder_load_routes_bit_equal(gpu_device, enc_w):
    """out_dim 64 < 128: the zero rows of proj_out must survive the load"""
    g = torch.Generator().manual_seed(5)
    x = torch.randn(ENC_B, ENC_S, 64, generator=g).bfloat16().to(gpu_device)
    mask = torch.ones(ENC_B, ENC_S, dtype=torch.uint8)
    mask[1, ENC_S - ENC_S // 4:] = 0
    mask = mask.to(gpu_device)
    outs = {}
    for n, W in _five_ways(enc_w, gpu_device).items():
        st = _enc_stack()
        st.load(W, prefix="s.")
        e = st.embed(x)
        o = st.forward(e, mask)
        torch.cuda.synchronize()
        outs[n] = torch.cat([e.flatten().cpu(), o.flatten().cpu()])
        st.close()
    _assert_all_equal(outs, torch.int16)


# ------------------------------------------------------------------------------- VAE ---
def test_vae_load_routes_bit_equal(gpu_device):
    from acehip.vae import OobleckBackend
    cfg = VAEConfig.tiny()
    W = synth_vae_weights(cfg, seed=5, mode="parity", with_encoder=True)
    assert _not_bf16(W)
    bf = {k: v.bfloat16() for k, v in W.items()}
    ways = {"f32_host": W, "f32_dev": {k: v.to(gpu_device) for k, v in W.items()},
            "bf16_host": bf, "bf16_dev": {k: v.to(gpu_device) for k, v in bf.items()}}
    z = torch.randn(1, 64, 3, generator=torch.Generator().manual_seed(2)).bfloat16().to(gpu_device)
    outs = {}
    for n, Wn in ways.items():
        be = OobleckBackend(cfg, gpu_device.index or 0, max_T=8, with_encoder=True)
        be.load(Wn)
        outs[n] = be.decode_tensor(z).cpu()
        torch.cuda.synchronize()
        be.close()
    assert outs["f32_host"].shape == (1, 2, 3 * cfg.hop_length)
    _assert_all_equal(outs, torch.int32)


# ---------------------------------------------------------------------------- errors ---
def _raw_set(fn, h, name, t, dtype=None, shape=None):
    shape = tuple(t.shape) if shape is None else shape
    rc = fn(h, name.encode(), ff.ptr(t), ff.dtype_code(t) if dtype is None else dtype, len(shape), ff.shape_arg(shape),
            1 if t.is_cuda else 0)
    return rc, ff.lib().acehip_last_error().decode()


def test_dit_set_weight_errors(gpu_device, dit_w):
    rt = _dit_runtime(gpu_device, torch.bfloat16)
    fn = ff.lib().acehip_dit_set_weight
    q = "layers.0.self_attn.q_proj.weight"
    rc, msg = _raw_set(fn, rt.h, "layers.0.self_attn.r_proj.weight", dit_w[q])
    assert rc == E_NAME and msg.startswith("dit_set_weight:") and "layers.0.self_attn.r_proj.weight" in msg
    rc, msg = _raw_set(fn, rt.h, "decoder." + q, dit_w[q], shape=(256, 255))
    assert rc == E_ARG and msg.startswith("dit_set_weight:") and q in msg
    assert "got [256,255,]" in msg and "want [256,256,]" in msg
    rc, msg = _raw_set(fn, rt.h, "_timestep_freqs", torch.ones(127))
    assert rc == E_ARG and "_timestep_freqs" in msg
    rc, msg = _raw_set(fn, rt.h, "_timestep_freqs", torch.ones(128).bfloat16())
    assert rc == E_ARG and "_timestep_freqs" in msg
    rc, msg = _raw_set(fn, rt.h, "_rope_inv_freq", torch.ones(63))
    assert rc == E_ARG and "_rope_inv_freq" in msg
    rc, _ = _raw_set(fn, rt.h, "rotary_emb.inv_freq", torch.ones(3))          # accepted and ignored
    assert rc == 0
    rc, msg = _raw_set(fn, rt.h, q, dit_w[q], dtype=7)
    assert rc == E_ARG and q in msg          # (the text named no weight before the shared loader)
    # finalize lists a withheld weight, and q_proj, which only the refused calls above ever named:
    # a refusal must not count as a load
    withheld = "layers.0.mlp.up_proj.weight"
    _dit_load(rt, dit_w, skip=(withheld, q))
    rc = ff.lib().acehip_dit_finalize(rt.h)
    msg = ff.lib().acehip_last_error().decode()
    assert rc == E_STATE and msg.startswith("dit_finalize:") and withheld in msg and q in msg
    assert "layers.0.self_attn.k_proj.weight" not in msg
    rt.set_weight(withheld, dit_w[withheld])
    rt.set_weight(q, dit_w[q])
    ff.check(ff.lib().acehip_dit_finalize(rt.h), "dit_finalize")
    rt.close()


def test_enc_set_weight_errors(gpu_device, enc_w):
    st = _enc_stack()
    fn = ff.lib().acehip_enc_set_weight
    q = "layers.1.self_attn.q_proj.weight"
    wq = enc_w["s." + q]
    rc, msg = _raw_set(fn, st.h, "layers.2.self_attn.q_proj.weight", wq)
    assert rc == E_NAME and msg.startswith("enc_set_weight:") and "layers.2.self_attn.q_proj.weight" in msg
    rc, msg = _raw_set(fn, st.h, "proj_out.weight", enc_w["s.proj_out.weight"], shape=(128, 256))
    assert rc == E_ARG and msg.startswith("enc_set_weight:") and "proj_out.weight" in msg
    shape_msg = msg
    rc, msg = _raw_set(fn, st.h, "_rope_inv_freq", torch.ones(65))
    assert rc == E_ARG and "_rope_inv_freq" in msg
    rc, _ = _raw_set(fn, st.h, "rotary_emb.inv_freq", torch.ones(3))
    assert rc == 0
    rc, msg = _raw_set(fn, st.h, q, wq, dtype=7)
    assert rc == E_ARG and q in msg          # (the text named no weight before the shared loader)
    # as for the DiT: the withheld weight and the one only refused calls named are both missing
    withheld = "s.layers.0.mlp.gate_proj.weight"
    for k, v in enc_w.items():
        if k not in (withheld, "s." + q):
            st.set_weight(k[2:], v)
    rc = ff.lib().acehip_enc_finalize(st.h)
    msg = ff.lib().acehip_last_error().decode()
    assert rc == E_STATE and msg.startswith("enc_finalize:") and withheld[2:] in msg and q in msg
    assert "layers.1.self_attn.k_proj.weight" not in msg
    st.close()
    # the shape-mismatch text the shared table changes (checked last): the encoder's now lists both
    # shapes, like the DiT's
    assert "got [128,256,]" in shape_msg and "want [64,256,]" in shape_msg


def test_vae_set_weight_dtype_refused(gpu_device):
    from acehip.vae import OobleckBackend
    be = OobleckBackend(VAEConfig.tiny(), gpu_device.index or 0, max_T=8, with_encoder=False)
    rc, msg = _raw_set(ff.lib().acehip_vae_set_weight, be.h, "decoder.conv1.bias", torch.ones(128), dtype=7)
    assert rc == E_ARG and msg.startswith("vae_set_weight:") and "decoder.conv1.bias" in msg
    be.close()
