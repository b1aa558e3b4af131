"""Stubs the LM-scoring recorder (tools/record_lm_score.py) and the scoring tests share: the parts
of ``LLMHandler`` and of its tokenizer that ``acestep/core/scoring/lm_score.py:116-173`` and
``acehip.integration.install_lm_score`` touch, and the model the fixtures were recorded on.

A text is space-separated integers, one token id each; no special tokens exist, so
``add_special_tokens`` changes nothing.  ``truncation=True`` cuts to ``model_max_length`` tokens."""
import contextlib

import torch


def ids_to_text(ids) -> str:
    return " ".join(str(int(i)) for i in ids)


class Encoding(dict):
    """What a tokenizer call returns: ``['input_ids']``, ``['attention_mask']``, ``.to(device)``."""

    def to(self, device):
        return Encoding({k: v.to(device) for k, v in self.items()})


class StubTokenizer:
    def __init__(self, model_max_length: int = 4096):
        self.model_max_length = model_max_length

    def __call__(self, text, return_tensors="pt", add_special_tokens=True, padding=False, truncation=False, **kw):
        assert return_tensors == "pt"
        ids = [int(t) for t in text.split()]
        if truncation:
            ids = ids[:self.model_max_length]
        t = torch.tensor([ids], dtype=torch.long).reshape(1, len(ids))
        return Encoding(input_ids=t, attention_mask=torch.ones_like(t))


class StubHandler:
    """``llm``, ``llm_tokenizer``, ``llm_backend``, ``device``, ``llm_initialized``,
    ``get_hf_model_for_scoring`` and a no-op ``_load_model_context``."""

    def __init__(self, llm, tokenizer=None, device="cpu", backend="pt"):
        self.llm = llm
        self.llm_tokenizer = tokenizer or StubTokenizer()
        self.llm_backend = backend
        self.device = torch.device(device)
        self.llm_initialized = True
        self.contexts = 0

    def get_hf_model_for_scoring(self):
        return self.llm

    @contextlib.contextmanager
    def _load_model_context(self):
        self.contexts += 1
        yield


def recall_from_ranks(ranks, topk=10):
    """The reference's recall formula (lm_score.py:201-232) with "the target is among the first k
    of top-k" read off the target's 1-based rank: the loop structure of the reference, kept here."""
    target_len = len(ranks)
    recall_per_k, position_scores = {}, []
    for k in range(1, topk + 1):
        hits = 0
        for pos in range(target_len):
            if ranks[pos] <= k:
                hits += 1
                if k == topk:
                    position_scores.append(1.0 - (ranks[pos] - 1) / topk)
        recall_per_k[k] = hits / target_len if target_len > 0 else 0.0
    while len(position_scores) < target_len:
        position_scores.append(0.0)
    return (sum(position_scores) / len(position_scores) if position_scores else 0.0), recall_per_k


def ranks_of(logits: torch.Tensor, targets: torch.Tensor) -> torch.Tensor:
    """1-based rank of targets[r] in logits[r], equal values ranked by lower index first."""
    tl = logits.gather(1, targets[:, None])
    col = torch.arange(logits.shape[1])[None, :]
    return 1 + (logits > tl).sum(1) + ((logits == tl) & (col < targets[:, None])).sum(1)


def build_model(meta: dict, weights: dict):
    """The fp32 ``Qwen3ForCausalLM`` of a fixture: ``meta`` is the safetensors metadata (the
    Qwen3Config fields as strings), ``weights`` the regenerated Qwen3Model state dict."""
    from transformers import Qwen3Config, Qwen3ForCausalLM
    ints = ("vocab_size", "hidden_size", "intermediate_size", "num_hidden_layers", "num_attention_heads",
            "num_key_value_heads", "head_dim", "max_position_embeddings")
    cfg = {k: int(meta[k]) for k in ints}
    cfg.update(rms_norm_eps=float(meta["rms_norm_eps"]), rope_theta=float(meta["rope_theta"]), attention_bias=False,
               use_sliding_window=False, tie_word_embeddings=True)
    model = Qwen3ForCausalLM(Qwen3Config(**cfg)).eval()
    missing, unexpected = model.model.load_state_dict(weights, strict=False)
    assert not unexpected and all(k.startswith("rotary_emb") for k in missing), (missing, unexpected)
    model.tie_weights()
    return model
