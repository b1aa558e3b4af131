"""The 5 Hz LM's token loop on the HIP path (acehip.lm.HipCausalLM: acehip_enc_prefill /
acehip_enc_decode / acehip_lm_head_bf16) against transformers' Qwen3ForCausalLM, recorded on
the CPU by tools/record_lm_decode.py on the seeded synthetic weights regenerated here.  Each
fixture's call sequence is replayed through ``__call__`` exactly as the reference's
``_forward_pass`` (acestep/llm_inference.py:416-438) makes it: the left-padded prompt with its
mask, then one token and the grown mask per step.

Bounds: the logits' rel-L2 against the reference's fp32 logits is at most twice what the
reference's own bf16 model makes against them (the manifest's ref_bf16_rel_l2), over all
calls and over the last quarter alone; the top-1 equals the fp32 top-1 on every pair the
manifest marks as clear.

The two LM widths (w06, w17) scale the synthetic embedding by the manifest's embed_gain, as
the recorder does, so that their logits have top-1 margins (tools/record_lm_decode.py).

Measured on an MI355X, rel-L2 over all calls / last quarter / bound, and cached vs recomputed
(bar 1e-2): tiny 0.01276 / 0.01323 / 0.02544, 0.00731; w06 0.01720 / 0.01708 / 0.03462, 0.00930;
w17 0.01900 / 0.01958 / 0.03812, 0.00998."""
import json

import pytest
import torch
from safetensors import safe_open

from conftest import GOLDEN, cosine, load_golden, rel_l2

from acehip.config import DiTConfig
from acehip.weights import synth_text_encoder_weights

pytestmark = pytest.mark.gpu

with open(f"{GOLDEN}/lm_decode_manifest.json") as _f:
    MANIFEST = json.load(_f)
TAGS = sorted(MANIFEST)


def _cfg(meta) -> DiTConfig:
    return DiTConfig(hidden_size=int(meta["hidden_size"]), intermediate_size=int(meta["intermediate_size"]),
                     num_hidden_layers=int(meta["num_hidden_layers"]),
                     num_attention_heads=int(meta["num_attention_heads"]),
                     num_key_value_heads=int(meta["num_key_value_heads"]), head_dim=int(meta["head_dim"]),
                     rms_norm_eps=float(meta["rms_norm_eps"]), rope_theta=float(meta["rope_theta"]))


def _fixture(tag):
    with safe_open(f"{GOLDEN}/lm_decode_{tag}.safetensors", "pt") as f:
        meta = f.metadata()
    cfg = _cfg(meta)
    W = synth_text_encoder_weights(cfg, int(meta["vocab_size"]), seed=MANIFEST[tag]["seed"], mode="parity")
    W["embed_tokens.weight"] = W["embed_tokens.weight"] * MANIFEST[tag]["embed_gain"]   # the recorder's gain
    return cfg, W, load_golden(f"lm_decode_{tag}")


def _lm(cfg, W, dev, capacity, max_batch=2):
    from acehip.lm import HipCausalLM, HipLMRuntime
    rt = HipLMRuntime(cfg, dev.index or 0, max_batch=max_batch, capacity=capacity,
                      prefill_tokens=max_batch * capacity)
    rt.load({k: v.to(dev) for k, v in W.items()})
    return HipCausalLM(rt)


def _replay(lm, ids, mask, forced):
    """_forward_pass's call sequence; logits[:, -1, :] of every call → [N + 1, B, V] and the final ids / mask."""
    out, past = [], None
    for step in range(forced.shape[1] + 1):
        if past is None:
            o = lm(input_ids=ids, attention_mask=mask, use_cache=True)
        else:
            o = lm(input_ids=ids[:, -1:], past_key_values=past, attention_mask=mask, use_cache=True)
        assert o.logits.shape[:2] == (ids.shape[0], 1) and o.logits.dtype == torch.bfloat16
        out.append(o.logits[:, -1, :])
        past = o.past_key_values
        assert past.get_seq_length() == ids.shape[1]
        if step < forced.shape[1]:
            ids = torch.cat([ids, forced[:, step:step + 1]], dim=1)
            mask = torch.cat([mask, torch.ones_like(mask[:, :1])], dim=1)
    return torch.stack(out), ids, mask


@pytest.fixture(scope="module", params=TAGS)
def replayed(request, gpu_device):
    tag = request.param
    cfg, W, g = _fixture(tag)
    n = g["ids"].shape[1] + g["forced"].shape[1]
    lm = _lm(cfg, W, gpu_device, capacity=n + 20)
    logits, ids, mask = _replay(lm, g["ids"].to(gpu_device), g["mask"].to(gpu_device), g["forced"].to(gpu_device))
    torch.cuda.synchronize()
    yield tag, lm, g, logits.float().cpu(), ids, mask
    lm.close()


def test_logits_vs_reference_fp32(replayed):
    tag, _, g, logits, _, _ = replayed
    ref, bound = g["logits_f32"], 2 * MANIFEST[tag]["ref_bf16_rel_l2"]
    assert torch.isfinite(logits).all()
    err = rel_l2(logits, ref)
    q = logits.shape[0] // 4
    err_q = rel_l2(logits[-q:], ref[-q:])
    print(f"{tag}: rel-L2 {err:.5f} (last quarter {err_q:.5f}), bound {bound:.5f}")
    assert err <= bound, f"{tag}: logits rel-L2 {err:.5f} over all calls, bound {bound:.5f}"
    assert err_q <= bound, f"{tag}: logits rel-L2 {err_q:.5f} over the last quarter, bound {bound:.5f}"


def test_top1_on_clear_pairs(replayed):
    tag, _, g, logits, _, _ = replayed
    clear = torch.tensor(MANIFEST[tag]["clear"], dtype=torch.bool)
    assert clear.shape == logits.shape[:2]
    same = logits.argmax(-1) == g["logits_f32"].argmax(-1)
    assert bool(same[clear].all()), f"{tag}: top-1 differs on clear pairs {(~same & clear).nonzero().tolist()}"


def test_cache_vs_recomputation(replayed):
    """One use_cache=False call on the whole sequence: the two paths differ only in GEMM shape
    and attention kernel."""
    tag, lm, _, logits, ids, mask = replayed
    o = lm(input_ids=ids, attention_mask=mask, use_cache=False)
    torch.cuda.synchronize()
    assert o.past_key_values is None
    err = rel_l2(o.logits[:, -1, :].float().cpu(), logits[-1])
    print(f"{tag}: cached vs recomputed rel-L2 {err:.5f}")
    assert err < 1e-2, (tag, err)


@pytest.mark.parametrize("tag", [t for t in TAGS if t != "w17"])     # the tags that store hidden_last
def test_text_encoder_attention_mask(gpu_device, tag):
    """TextEncoder with a padding mask: all ones is bit-identical to no mask; with row 1
    left-padded by 9 the hidden states at the unpadded positions meet test_textenc.py's bar
    against the reference's bf16 model."""
    from acehip.condition import TextEncoder
    TOL_REL, TOL_COS = 0.025, 0.999
    cfg, W, g = _fixture(tag)
    te = TextEncoder(cfg, device=gpu_device.index or 0, max_batch=2, max_tokens=128)
    te.load({k: v.to(gpu_device) for k, v in W.items()})
    ids, mask = g["ids"].to(gpu_device), g["mask"].to(gpu_device)
    plain = te(input_ids=ids).last_hidden_state.clone()
    ones = te(input_ids=ids, attention_mask=torch.ones_like(mask)).last_hidden_state.clone()
    padded = te(input_ids=ids, attention_mask=mask).last_hidden_state
    torch.cuda.synchronize()
    assert torch.equal(plain.view(torch.int16), ones.view(torch.int16))
    assert torch.isfinite(padded.float()).all()          # padded rows too: their K/V feed the cache
    keep = g["mask"].bool()
    out, ref = padded.float().cpu()[keep], g["hidden_last"].float()[keep]
    assert rel_l2(out, ref) <= TOL_REL, rel_l2(out, ref)
    assert cosine(out, ref) >= TOL_COS
    te.close()


def test_cache_contract_errors(gpu_device):
    """A foreign cache, two new tokens with a cache, a stale cache and pos at capacity each raise
    a ValueError; the next valid prefill works."""
    from acehip.lm import HipKVCache
    cfg, W, g = _fixture("tiny")
    ids, mask = g["ids"].to(gpu_device), g["mask"].to(gpu_device)
    S = ids.shape[1]
    lm = _lm(cfg, W, gpu_device, capacity=S + 2)
    other = _lm(cfg, W, gpu_device, capacity=S + 2)
    first = lm(input_ids=ids, attention_mask=mask)
    past = first.past_key_values
    tok = ids[:, -1:]
    with pytest.raises(ValueError, match="foreign"):
        lm(input_ids=tok, past_key_values=HipKVCache(other, 1, 2, S))
    with pytest.raises(ValueError, match="foreign"):
        lm(input_ids=tok, past_key_values=object())
    with pytest.raises(ValueError, match="new tokens"):
        lm(input_ids=ids[:, -2:], past_key_values=past)
    with pytest.raises(ValueError, match="batch"):
        lm(input_ids=tok[:1], past_key_values=past)
    m = mask
    for _ in range(2):                                   # fills the cache: S + 2 == capacity
        m = torch.cat([m, torch.ones_like(m[:, :1])], dim=1)
        past = lm(input_ids=tok, past_key_values=past, attention_mask=m).past_key_values
    with pytest.raises(ValueError, match="full"):
        lm(input_ids=tok, past_key_values=past)
    again = lm(input_ids=ids, attention_mask=mask)       # a valid prefill after the errors
    with pytest.raises(ValueError, match="stale"):
        lm(input_ids=tok, past_key_values=past)
    torch.cuda.synchronize()
    assert torch.equal(again.logits.view(torch.int16), first.logits.view(torch.int16))
    # the runtime itself refuses pos >= capacity
    from acehip import _ffi as ff
    x = torch.zeros(2, cfg.hidden_size, device=gpu_device, dtype=torch.bfloat16)
    rc = ff.lib().acehip_enc_decode(lm.rt.stack.h, ff.ptr(x), None, 0, 2, S + 2, ff.ptr(x), ff.stream_ptr())
    assert rc == -1
    lm.close()
    other.close()
