"""The LM-scoring seam on the host (no GPU): acehip.integration.install_lm + install_lm_score on the
stub handler / tokenizer of tests/lm_score_ref.py and a stub module object, with HipCausalLM's
runtime replaced by a torch fp32 stand-in (``forward_all`` / ``score_rows`` served by the
transformers model built from the fixture's synthetic weights).  The stand-in proves the seam —
tokenisation, slicing, rank → recall, mean, fallback, errors — not the kernel
(tests/test_gpu_lm_score.py does that).  Also: the conditions every recorded fixture must meet."""
import json
import logging
import types

import pytest
import torch
from safetensors import safe_open

from conftest import GOLDEN, load_golden

from acehip.config import DiTConfig
from acehip.integration import install_lm, install_lm_score, recall_from_ranks
from acehip.lm import HipCausalLM
from acehip.weights import synth_text_encoder_weights
from lm_score_ref import StubHandler, StubTokenizer, build_model, ids_to_text
from lm_score_ref import recall_from_ranks as ref_recall_from_ranks

with open(f"{GOLDEN}/lm_score_manifest.json") as _f:
    MANIFEST = json.load(_f)
TAGS = sorted(MANIFEST)


class TorchScoreRuntime:
    """Stand-in for acehip.lm.HipLMRuntime's scoring calls, in fp32 on the CPU.  ``fail``: raise the
    RuntimeError an acehip call would."""

    def __init__(self, model, max_batch=2, capacity=256, prefill_tokens=None, fail=False):
        self.model, self.device = model, torch.device("cpu")
        self.max_batch, self.capacity, self.prefill_tokens, self.fail = max_batch, capacity, prefill_tokens, fail
        self.calls = []

    def embed(self, ids):
        return self.model.model.embed_tokens(ids)

    def forward_all(self, x):
        if self.fail:
            raise RuntimeError("acehip enc_forward failed (-3): injected")
        self.calls.append(("forward_all", tuple(x.shape)))
        with torch.no_grad():
            return self.model.model(inputs_embeds=x).last_hidden_state

    def score_rows(self, h, targets):
        self.calls.append(("score_rows", tuple(h.shape), targets.tolist()))
        with torch.no_grad():
            logits = self.model.lm_head(h).float()
        tl = logits.gather(1, targets[:, None])
        lse = torch.logsumexp(logits, dim=1)
        col = torch.arange(logits.shape[1])[None, :]
        ng = (logits > tl).sum(1).to(torch.int32)
        ne = ((logits == tl) & (col < targets[:, None])).sum(1).to(torch.int32)
        return tl[:, 0] - lse, lse, ng, ne


def _fixture(tag):
    with safe_open(f"{GOLDEN}/lm_score_{tag}.safetensors", "pt") as f:
        meta = f.metadata()
    cfg = DiTConfig(hidden_size=int(meta["hidden_size"]), intermediate_size=int(meta["intermediate_size"]),
                    num_hidden_layers=int(meta["num_hidden_layers"]),
                    num_attention_heads=int(meta["num_attention_heads"]),
                    num_key_value_heads=int(meta["num_key_value_heads"]), head_dim=int(meta["head_dim"]),
                    rms_norm_eps=float(meta["rms_norm_eps"]), rope_theta=float(meta["rope_theta"]))
    W = synth_text_encoder_weights(cfg, int(meta["vocab_size"]), seed=MANIFEST[tag]["seed"], mode="parity")
    W["embed_tokens.weight"] = W["embed_tokens.weight"] * MANIFEST[tag]["embed_gain"]
    return build_model(meta, W), load_golden(f"lm_score_{tag}")


def _stub_module():
    calls = []

    def lp(handler, prompt, target, temperature=1.0):
        calls.append(("lp", prompt, target, temperature))
        return -1.25

    def recall(handler, prompt, target, topk=10):
        calls.append(("recall", prompt, target, topk))
        return 0.75, {1: 0.5}
    return types.SimpleNamespace(_calculate_log_prob=lp, _calculate_topk_recall=recall, calls=calls), lp, recall


@pytest.fixture(scope="module")
def tiny():
    return _fixture("tiny")


def _installed(model, tokenizer=None, fallback=False, **rt_kw):
    handler = StubHandler(model, tokenizer or StubTokenizer())
    rt = TorchScoreRuntime(model, **rt_kw)
    res = install_lm(handler, runtime=rt, fallback=fallback)
    assert isinstance(handler.llm, HipCausalLM) and handler.get_hf_model_for_scoring() is model
    mod, lp, recall = _stub_module()
    out = install_lm_score(handler, mod, fallback=fallback)
    assert out["original"] == {"_calculate_log_prob": lp, "_calculate_topk_recall": recall}
    assert mod._calculate_log_prob is not lp and mod._calculate_topk_recall is not recall
    return handler, rt, mod, res


def _texts(g):
    P = int(g["prompt_len"])
    ids = g["ids"][0].tolist()
    return ids_to_text(ids[:P]), " " + ids_to_text(ids[P:]), P


@pytest.mark.parametrize("tag", TAGS)
def test_seam_matches_the_recorded_reference(tag):
    """The reference's own return values on the fp32 model.  Recall: the same dict, the average
    within 1e-12 (both are sums of the same 48 multiples of 0.1 divided by 48).  Mean log-prob:
    within 1e-5 * max(1, |value|) — both sides are fp32 over V <= 2048, and an fp32 log-sum-exp of
    2048 terms is good to about 1e-6."""
    model, g = _fixture(tag)
    handler, rt, mod, _ = _installed(model)
    prompt, target, P = _texts(g)
    T = g["ids"].shape[1] - P
    avg, per_k = mod._calculate_topk_recall(handler, prompt, target, topk=10)
    want_k = {k + 1: float(v) for k, v in enumerate(g["ref_recall_per_k"].tolist())}
    assert per_k == want_k
    assert abs(avg - float(g["ref_recall_average"])) <= 1e-12
    assert rt.calls[0] == ("forward_all", (1, P + T, model.config.hidden_size))
    assert rt.calls[1] == ("score_rows", (T, model.config.hidden_size), g["ids"][0, P:].tolist())   # lm_score.py:170-171
    got = mod._calculate_log_prob(handler, prompt, target)
    want = float(g["ref_log_prob"])
    assert isinstance(got, float)
    assert abs(got - want) <= 1e-5 * max(1.0, abs(want)), (got, want)
    assert got == mod._calculate_log_prob(handler, prompt, target, 0.7)          # temperature is ignored
    assert handler.contexts == 3 and not mod.calls                              # under _load_model_context
    lp, rank = handler.llm.score(g["ids"], P)
    assert lp.dtype == torch.float32 and rank.dtype == torch.int64
    clear = g["clear"].bool()
    assert torch.equal(rank[clear], g["rank_f32"][clear])


def test_recall_formula_is_the_reference_loop():
    g = torch.Generator().manual_seed(0)
    for topk in (1, 3, 10):
        ranks = torch.randint(1, 15, (40,), generator=g).tolist()
        assert recall_from_ranks(ranks, topk) == ref_recall_from_ranks(ranks, topk)
    assert recall_from_ranks([], 10)[0] == 0.0


def test_empty_and_truncated_target(tiny):
    model, g = tiny
    prompt, target, P = _texts(g)
    handler, rt, mod, _ = _installed(model)
    assert mod._calculate_log_prob(handler, prompt, "") == float("-inf")
    assert mod._calculate_topk_recall(handler, prompt, "") == (0.0, {})
    for limit in (P, P - 5):                              # the target is cut away entirely
        handler, rt, mod, _ = _installed(model, StubTokenizer(model_max_length=limit))
        assert mod._calculate_log_prob(handler, prompt, target) == float("-inf")
        assert mod._calculate_topk_recall(handler, prompt, target, topk=5) == (0.0, {})
        assert not rt.calls and not mod.calls
    # cut in the middle: the targets that are left are scored
    handler, rt, mod, _ = _installed(model, StubTokenizer(model_max_length=P + 7))
    mod._calculate_log_prob(handler, prompt, target)
    assert rt.calls[1][1][0] == 7 and rt.calls[1][2] == g["ids"][0, P:P + 7].tolist()


def test_other_llm_runs_the_original(tiny):
    model, g = tiny
    prompt, target, _ = _texts(g)
    handler = StubHandler(model)                          # install_lm never ran: llm is the transformers module
    mod, lp, recall = _stub_module()
    install_lm_score(handler, mod)
    assert mod._calculate_log_prob(handler, prompt, target, 0.5) == -1.25
    assert mod._calculate_topk_recall(handler, prompt, target, topk=3) == (0.75, {1: 0.5})
    assert mod.calls == [("lp", prompt, target, 0.5), ("recall", prompt, target, 3)]


def test_fallback_policy(tiny, caplog):
    model, g = tiny
    prompt, target, _ = _texts(g)
    handler, rt, mod, _ = _installed(model, fail=True)
    with pytest.raises(RuntimeError, match="injected"):
        mod._calculate_log_prob(handler, prompt, target)
    with pytest.raises(RuntimeError, match="injected"):
        mod._calculate_topk_recall(handler, prompt, target)
    assert not mod.calls
    handler, rt, mod, _ = _installed(model, fallback=True, fail=True)
    with caplog.at_level(logging.WARNING, logger="acehip"):
        assert mod._calculate_log_prob(handler, prompt, target) == -1.25
        assert mod._calculate_topk_recall(handler, prompt, target, topk=4) == (0.75, {1: 0.5})
    assert mod.calls == [("lp", prompt, target, 1.0), ("recall", prompt, target, 4)]
    assert sum("scoring failed" in r.getMessage() for r in caplog.records) == 2
    assert handler.get_hf_model_for_scoring() is model     # what the original function scores on


def test_score_errors_and_state(tiny):
    model, g = tiny
    ids, P = g["ids"], int(g["prompt_len"])
    S = ids.shape[1]
    lm = HipCausalLM(TorchScoreRuntime(model, capacity=S, prefill_tokens=S))
    state = (lm._generation, lm._cache, lm._masked, lm._mask.clone())
    lm.score(ids, P)
    lm.score(ids, 1)
    lm.score(ids, S - 1)
    assert (lm._generation, lm._cache, lm._masked) == state[:3] and torch.equal(lm._mask, state[3])
    for bad in (0, -1, S, S + 3):
        with pytest.raises(ValueError, match="prompt_len"):
            lm.score(ids, bad)
    with pytest.raises(ValueError, match=r"\[1, S\]"):
        lm.score(ids.repeat(2, 1), P)
    with pytest.raises(ValueError, match=r"\[1, S\]"):
        lm.score(ids[0], P)
    with pytest.raises(ValueError, match="capacity"):
        HipCausalLM(TorchScoreRuntime(model, capacity=S - 1)).score(ids, P)
    with pytest.raises(ValueError, match="prefill_tokens"):
        HipCausalLM(TorchScoreRuntime(model, capacity=S, prefill_tokens=S - 1)).score(ids, P)


def test_fixture_manifest_conditions():
    """What tools/record_lm_score.py refuses to write: a clear share under 0.5, a bf16 rank that
    differs from the fp32 rank on a clear position, an fp32 tie with the target in the top 11."""
    assert TAGS == ["tiny", "w06", "w17"]
    for tag in TAGS:
        m, g = MANIFEST[tag], load_golden(f"lm_score_{tag}")
        clear = g["clear"].bool()
        assert m["clear_share"] >= 0.5 and abs(float(clear.float().mean()) - m["clear_share"]) < 1e-6
        assert m["ref_bf16_ranks_agree"] and bool((g["rank_bf16"] == g["rank_f32"])[clear].all())
        assert not m["fp32_tie_in_top11"]
        assert m["ref_bf16_lp_rms"] > 0 and m["ref_bf16_max_abs"] > 0
        rms = float((g["lp_bf16"] - g["lp_f32"]).pow(2).mean().sqrt())
        assert abs(rms - m["ref_bf16_lp_rms"]) <= 1e-9
        assert g["ids"].shape == (1, m["prompt_len"] + m["targets"]) and int(g["prompt_len"]) == m["prompt_len"]
        # ranks on both sides of the top-10 band
        assert int(g["rank_f32"].min()) == 1 and int(g["rank_f32"].max()) > 10
