"""The LM seam on the host (no GPU): acehip.integration.install_lm on a stub handler whose ``llm``
is a tiny CPU Qwen3ForCausalLM, with HipCausalLM's runtime replaced by a small torch stand-in
injected through the constructor.  The stand-in only proves the seam (call pattern, mask
growth, cache contract, pass-throughs, fallback); it is not the product and is not shipped.
The stub handler drives a copy of the loop structure of the reference's
``_generate_with_cfg_custom`` / ``_forward_pass`` (acestep/llm_inference.py:2414-2533, :416-438)
kept here.  Also: the conditions every recorded fixture must meet."""
import json
import os

import pytest
import torch

from conftest import GOLDEN

from acehip.integration import install_lm
from acehip.lm import HipCausalLM, HipKVCache

CFG = dict(vocab_size=97, hidden_size=64, intermediate_size=128, num_hidden_layers=2, num_attention_heads=2,
           num_key_value_heads=1, head_dim=32, rms_norm_eps=1e-6, rope_theta=10000.0, max_position_embeddings=256,
           attention_bias=False, use_sliding_window=False, tie_word_embeddings=True)


def _model(**over):
    import transformers
    torch.manual_seed(0)
    return transformers.Qwen3ForCausalLM(transformers.Qwen3Config(**dict(CFG, **over))).eval()


class TorchRuntime:
    """Stand-in for acehip.lm.HipLMRuntime on the CPU: the same five calls, served by the wrapped
    module's own layers.  ``fail_at``: raise the RuntimeError an acehip call would at that decode pos."""

    def __init__(self, model, max_batch=4, capacity=64, fail_at=None, prefill_tokens=None):
        self.model, self.device = model, torch.device("cpu")
        self.prefill_tokens = prefill_tokens
        self.max_batch, self.capacity, self.fail_at = max_batch, capacity, fail_at
        self.past = None
        self.calls = []

    def embed(self, ids):
        return self.model.model.embed_tokens(ids)

    def prefill(self, x, kmask):
        self.calls.append(("prefill", tuple(x.shape[:2]), None if kmask is None else kmask.clone()))
        with torch.no_grad():
            o = self.model.model(inputs_embeds=x, attention_mask=None if kmask is None else kmask.long(), use_cache=True)
        self.past = o.past_key_values
        return o.last_hidden_state[:, -1]

    def decode(self, x, kmask, pos):
        if self.fail_at is not None and pos >= self.fail_at:
            raise RuntimeError("acehip enc_decode failed (-3): injected")
        B = x.shape[0]
        m = None if kmask is None else kmask[:B, :pos + 1].clone()
        self.calls.append(("decode", pos, m))
        assert self.past.get_seq_length() == pos
        with torch.no_grad():
            o = self.model.model(inputs_embeds=x[:, None], past_key_values=self.past,
                                 attention_mask=None if m is None else m.long(), use_cache=True)
        self.past = o.past_key_values
        return o.last_hidden_state[:, -1]

    def lm_head(self, h):
        with torch.no_grad():
            return self.model.lm_head(h)


class StubHandler:
    """The parts of LLMHandler the seam touches."""

    def __init__(self, model, backend="pt"):
        self.llm, self.llm_backend, self.device = model, backend, torch.device("cpu")

    def get_hf_model_for_scoring(self):
        return self.llm

    def _forward_pass(self, model, generated_ids, model_kwargs, past_key_values, use_cache):
        if past_key_values is None:
            return model(input_ids=generated_ids, **model_kwargs, use_cache=use_cache)
        return model(input_ids=generated_ids[:, -1:], past_key_values=past_key_values, **model_kwargs,
                     use_cache=use_cache)

    def generate_with_cfg(self, batch_input_ids, batch_attention_mask, max_new_tokens, cfg_scale=2.0):
        """Loop structure of _generate_with_cfg_custom with greedy sampling: batch = [cond, uncond]."""
        model = self.llm
        batch_size = batch_input_ids.shape[0] // 2
        generated_ids = batch_input_ids.clone()
        attention_mask = batch_attention_mask.clone()
        model_kwargs = {"attention_mask": attention_mask}
        past_key_values = None
        use_cache = hasattr(model, "generation_config") and getattr(model.generation_config, "use_cache", True)
        with torch.inference_mode():
            for _ in range(max_new_tokens):
                outputs = self._forward_pass(model, generated_ids, model_kwargs, past_key_values, use_cache)
                next_token_logits = outputs.logits[:, -1, :]
                cond, uncond = next_token_logits[:batch_size], next_token_logits[batch_size:]
                cfg_logits = uncond.float() + cfg_scale * (cond.float() - uncond.float())
                next_tokens = cfg_logits.argmax(-1)
                generated_ids = torch.cat([generated_ids, next_tokens.unsqueeze(1).repeat(2, 1)], dim=1)
                attention_mask = torch.cat([attention_mask, torch.ones((batch_size * 2, 1),
                                                                       dtype=attention_mask.dtype)], dim=1)
                model_kwargs["attention_mask"] = attention_mask
                if use_cache and hasattr(outputs, "past_key_values"):
                    past_key_values = outputs.past_key_values
        return generated_ids


def _prompt():
    g = torch.Generator().manual_seed(5)
    ids = torch.randint(1, CFG["vocab_size"], (2, 11), generator=g)
    mask = torch.ones(2, 11, dtype=torch.long)
    mask[1, :4] = 0                                   # the uncond row is shorter: left-padded
    return ids, mask


def test_install_lm_drives_the_reference_loop():
    model = _model()
    ids, mask = _prompt()
    want = StubHandler(model).generate_with_cfg(ids, mask, 9)
    h = StubHandler(model)
    rt = TorchRuntime(model)
    res = install_lm(h, runtime=rt)
    lm = res["lm"]
    assert isinstance(h.llm, HipCausalLM) and h.llm is lm and res["original"] is model
    assert h.get_hf_model_for_scoring() is model
    got = h.generate_with_cfg(ids, mask, 9)
    assert torch.equal(got, want)
    # the call pattern: one prefill with the prompt mask, then one decode per token at growing pos,
    # each seeing the prompt's padding and a one in every later column
    kinds = [c[0] for c in rt.calls]
    assert kinds == ["prefill"] + ["decode"] * 8
    assert torch.equal(rt.calls[0][2].long(), mask)
    for i, (_, pos, m) in enumerate(rt.calls[1:]):
        assert pos == 11 + i
        assert torch.equal(m.long(), torch.cat([mask, torch.ones(2, i + 1, dtype=torch.long)], 1))
    # a second generation resets the cache
    assert torch.equal(h.generate_with_cfg(ids, mask, 4), want[:, :15])


def test_pass_throughs():
    model = _model()
    h = StubHandler(model)
    lm = install_lm(h, runtime=TorchRuntime(model))["lm"]
    assert lm.config is model.config and lm.generation_config is model.generation_config
    assert lm.to("cpu") is lm and lm.eval() is lm
    p = next(lm.parameters())
    assert isinstance(p, torch.Tensor) and p.device == lm.device
    ids, mask = _prompt()
    a = lm.generate(input_ids=ids[:1], max_new_tokens=3, do_sample=False)
    b = model.generate(input_ids=ids[:1], max_new_tokens=3, do_sample=False)
    assert torch.equal(a, b)
    # use_cache=False: a prefill per call, no cache handed out
    o = lm(input_ids=ids, attention_mask=mask, use_cache=False)
    assert o.past_key_values is None and o.logits.shape == (2, 1, CFG["vocab_size"])
    with torch.no_grad():
        ref = model(input_ids=ids, attention_mask=mask).logits[:, -1:]
    assert torch.allclose(o.logits, ref, atol=1e-5)


def test_install_lm_skips():
    model = _model()
    h = StubHandler(model, backend="vllm")
    res = install_lm(h, runtime=TorchRuntime(model))
    assert res["lm"] is None and "pt" in res["skipped"] and h.llm is model
    wide = _model(num_attention_heads=4, num_key_value_heads=1)          # ratio 4: the 4B LM's
    h = StubHandler(wide)
    res = install_lm(h, runtime=TorchRuntime(wide))
    assert res["lm"] is None and "kv_heads" in res["skipped"] and h.llm is wide


def test_cache_contract_value_errors():
    model = _model()
    ids, mask = _prompt()
    lm = HipCausalLM(TorchRuntime(model, max_batch=2, capacity=13), wrapped=model)
    other = HipCausalLM(TorchRuntime(model), wrapped=model)
    past = lm(input_ids=ids, attention_mask=mask).past_key_values
    assert isinstance(past, HipKVCache) and past.get_seq_length() == 11
    tok = ids[:, -1:]
    with pytest.raises(ValueError, match="foreign"):
        lm(input_ids=tok, past_key_values=other(input_ids=ids, attention_mask=mask).past_key_values)
    with pytest.raises(ValueError, match="foreign"):
        lm(input_ids=tok, past_key_values=model(input_ids=ids, use_cache=True).past_key_values)
    with pytest.raises(ValueError, match="new tokens"):
        lm(input_ids=ids[:, -2:], past_key_values=past)
    with pytest.raises(ValueError, match="batch"):
        lm(input_ids=tok[:1], past_key_values=past)
    with pytest.raises(ValueError, match="attention_mask"):
        lm(input_ids=tok, past_key_values=past, attention_mask=mask)            # not grown
    with pytest.raises(ValueError, match="input_ids"):
        lm(attention_mask=mask)
    m = mask
    for i in range(2):
        m = torch.cat([m, torch.ones(2, 1, dtype=torch.long)], 1)
        past = lm(input_ids=tok, past_key_values=past, attention_mask=m).past_key_values
        assert past.get_seq_length() == 12 + i
    with pytest.raises(ValueError, match="full"):
        lm(input_ids=tok, past_key_values=past)
    with pytest.raises(ValueError, match="capacity"):
        lm(input_ids=torch.cat([ids, ids], 1))                                   # 22 > capacity 13
    with pytest.raises(ValueError, match="max_batch"):
        lm(input_ids=torch.cat([ids, ids], 0))
    small = HipCausalLM(TorchRuntime(model, max_batch=2, capacity=13, prefill_tokens=12), wrapped=model)
    with pytest.raises(ValueError, match="prefill_tokens"):
        small(input_ids=ids, attention_mask=mask)                                # 2 x 11 tokens > 12
    fresh = lm(input_ids=ids, attention_mask=mask).past_key_values                # a valid prefill still works
    with pytest.raises(ValueError, match="stale"):
        lm(input_ids=tok, past_key_values=past)
    assert fresh.get_seq_length() == 11


def test_fallback_continues_on_the_original_module():
    model = _model()
    ids, mask = _prompt()
    want = StubHandler(model).generate_with_cfg(ids, mask, 9)
    h = StubHandler(model)
    rt = TorchRuntime(model, fail_at=14)
    install_lm(h, runtime=rt, fallback=True)
    assert torch.equal(h.generate_with_cfg(ids, mask, 9), want)
    assert [c[0] for c in rt.calls] == ["prefill", "decode", "decode", "decode"]   # pos 11, 12, 13, then PyTorch
    # without the fallback the error propagates
    h2 = StubHandler(model)
    install_lm(h2, runtime=TorchRuntime(model, fail_at=14))
    with pytest.raises(RuntimeError, match="injected"):
        h2.generate_with_cfg(ids, mask, 9)


def test_fixture_manifest_conditions():
    with open(os.path.join(GOLDEN, "lm_decode_manifest.json")) as f:
        manifest = json.load(f)
    assert "tiny" in manifest
    for tag, e in manifest.items():
        assert e["clear_share"] >= 0.5, tag
        assert e["ref_bf16_top1_agrees"] is True, tag
        clear = torch.tensor(e["clear"])
        assert clear.shape == (e["steps"] + 1, e["B"])
        assert abs(float(clear.float().mean()) - e["clear_share"]) < 1e-6
        assert os.path.getsize(os.path.join(GOLDEN, f"lm_decode_{tag}.safetensors")) < (1 << 20), tag
