"""install_lm's ``wide_gqa`` switch on the host (no GPU): the stub handler and the torch stand-in
runtime of tests/test_lm_host.py on a 4 / 1-head model (heads / kv_heads = 4, the 4B LM's ratio).
What the default call does with such a model is asserted there (test_install_lm_skips)."""
import json
import os

import torch

from conftest import GOLDEN
from test_lm_host import CFG, StubHandler, TorchRuntime, _model, _prompt

from acehip.integration import install_lm
from acehip.lm import HipCausalLM, HipLogitFilters


class FilterHandler(StubHandler):
    """StubHandler with the two filter methods install_lm(filters=True) rebinds."""

    def _apply_top_k_filter(self, logits, top_k):
        return logits

    def _apply_top_p_filter(self, logits, top_p):
        return logits


def _wide():
    return _model(num_attention_heads=4, num_key_value_heads=1)


def test_wide_gqa_installs_ratio_4_and_drives_the_loop():
    model = _wide()
    ids, mask = _prompt()
    want = StubHandler(model).generate_with_cfg(ids, mask, 6)
    h = StubHandler(model)
    rt = TorchRuntime(model)
    res = install_lm(h, runtime=rt, wide_gqa=True)
    assert "skipped" not in res and isinstance(res["lm"], HipCausalLM) and h.llm is res["lm"]
    assert res["original"] is model and h.get_hf_model_for_scoring() is model
    assert torch.equal(h.generate_with_cfg(ids, mask, 6), want)
    assert [c[0] for c in rt.calls] == ["prefill"] + ["decode"] * 5


def test_wide_gqa_filters_and_slots_pass_through(monkeypatch):
    model = _wide()
    h = FilterHandler(model)
    orig_k, orig_p = h._apply_top_k_filter, h._apply_top_p_filter
    rt = TorchRuntime(model)
    rt.score_slots = 2
    res = install_lm(h, runtime=rt, wide_gqa=True, filters=True, fallback=True)
    lm, f = res["lm"], res["filters"]
    assert lm.score_slots == 2 and len(lm._slot_ids) == 2 and lm.fallback
    assert isinstance(f["hip"], HipLogitFilters) and f["hip"].fallback
    assert f["top_k"] == orig_k and f["top_p"] == orig_p
    assert h._apply_top_k_filter == f["hip"].top_k and h._apply_top_p_filter == f["hip"].top_p
    x = torch.zeros(2, CFG["vocab_size"])
    assert h._apply_top_k_filter(x, 5) is x              # a CPU tensor goes to the original
    # without runtime=, the runtime's keywords reach HipCausalLM.from_reference_model
    seen = {}

    def fake(cls, m, **kw):
        seen.update(kw, model=m)
        return HipCausalLM(TorchRuntime(m), wrapped=m)
    monkeypatch.setattr(HipCausalLM, "from_reference_model", classmethod(fake))
    h2 = StubHandler(model)
    res = install_lm(h2, capacity=128, max_batch=4, wide_gqa=True, score_slots=2)
    assert isinstance(h2.llm, HipCausalLM) and seen["model"] is model
    assert seen["score_slots"] == 2 and seen["capacity"] == 128 and seen["max_batch"] == 4
    assert "wide_gqa" not in seen


def test_other_ratios_stay_skipped():
    for heads, kv in ((8, 1), (3, 1)):
        m = _model(num_attention_heads=heads, num_key_value_heads=kv)
        h = StubHandler(m)
        res = install_lm(h, runtime=TorchRuntime(m), wide_gqa=True)
        assert res["lm"] is None and "kv_heads" in res["skipped"] and h.llm is m
    m = _model()                                         # ratio 2 installs with the switch as without
    assert install_lm(StubHandler(m), runtime=TorchRuntime(m), wide_gqa=True)["lm"] is not None
    m = _wide()                                          # the backend check comes first
    res = install_lm(StubHandler(m, backend="vllm"), runtime=TorchRuntime(m), wide_gqa=True)
    assert res["lm"] is None and "pt" in res["skipped"]


def test_gqa4_fixture_manifest_conditions():
    """The recorder's refusal rule holds for what is committed, and every file is under 1 MiB."""
    with open(os.path.join(GOLDEN, "lm_gqa4_manifest.json")) as f:
        manifest = json.load(f)
    assert sorted(manifest) == ["g4tiny", "w4b"]
    for tag, e in manifest.items():
        assert e["clear_share"] >= 0.5 and e["ref_bf16_top1_agrees"] is True, tag
        clear = torch.tensor(e["clear"])
        assert clear.shape == (e["steps"] + 1, e["B"])
        assert abs(float(clear.float().mean()) - e["clear_share"]) < 1e-6
        assert os.path.getsize(os.path.join(GOLDEN, f"lm_gqa4_{tag}.safetensors")) < (1 << 20), tag
    with open(os.path.join(GOLDEN, "lm_gqa4_score_manifest.json")) as f:
        score = json.load(f)
    e = score["w4b"]
    assert e["clear_share"] >= 0.5 and e["ref_bf16_ranks_agree"] is True and e["fp32_tie_in_top11"] is False
    assert (e["seed"], e["embed_gain"]) == (manifest["w4b"]["seed"], manifest["w4b"]["embed_gain"])
