"""The 5 Hz language model's token loop on the HIP path.

``LLMHandler.llm`` on the reference's ``pt`` backend is a transformers ``Qwen3ForCausalLM``.
Its two custom loops (``_generate_with_cfg_custom`` ``acestep/llm_inference.py:2414-2533`` and
``_generate_with_constrained_decoding`` ``:2321-2412``) touch the model only through
``_forward_pass`` (``:416-438``):

  * first call:   ``model(input_ids=ids[B, S], attention_mask=mask[B, S], use_cache=True)``
  * later calls:  ``model(input_ids=ids[:, -1:], past_key_values=past, attention_mask=mask[B, S+i],
                   use_cache=True)``

and read only ``outputs.logits[:, -1, :]`` and ``outputs.past_key_values``.  :class:`HipCausalLM`
keeps exactly that contract: the first call embeds and prefills (``acehip_enc_prefill``), every
later call runs one decode step over the handle's K/V cache (``acehip_enc_decode``), and both
end in the vocabulary projection (``acehip_lm_head_bf16``).  The batch is ``[cond…, uncond…]``
left-padded to a common length (``:894-910``); RoPE positions are cache indices, padding
included, as transformers computes them when no ``position_ids`` are passed.

The FSM-constrained processor, repetition penalty, temperature and the multinomial stay in
torch, where the reference has them; so do top-k / top-p (``_apply_top_k_filter`` /
``_apply_top_p_filter``, ``:367-385``) unless ``install_lm(..., filters=True)`` rebinds them to
:class:`HipLogitFilters` (``acehip_lm_filter``).  ``generate()`` (no CFG, no
constrained decoding, ``:946``) stays on the wrapped module.

Scoring (``core/scoring/lm_score.py``: a teacher-forced pass over prompt + target, then the
log-probability or the top-k membership of every target token) is :meth:`HipCausalLM.score`:
one ``acehip_enc_forward`` over the sequence (every position's final-norm row; the K/V cache is
not touched) and ``acehip_lm_score_bf16`` over the target rows, which never forms the
``[S, V]`` logits.  :func:`acehip.integration.install_lm_score` rebinds the reference's two
scoring functions to it.  On a runtime with ``score_slots`` the calls that share a prompt reuse
its K/V: a slot is a cache row past the generation's, and a call runs ``acehip_enc_extend`` over
the positions that follow the longest prefix a slot already holds.

:meth:`HipCausalLM.extend` is the multi-token continuation of a running generation
(``acehip_enc_extend``: n new tokens per sequence in one pass); ``__call__`` keeps the
reference's one-token contract.

The prefill of the 0.6B and 1.7B LMs (16 / 8 heads) runs on the flash kernels, which take
heads / kv_heads of 1 or 2.  The 4B LM (32 / 8) is served too: the handle sends the attention of
its prefill and of the scoring forward to ``acehip_attention_extend_bf16`` (every position a new
query at ``pos = 0``), the one kernel besides the decode step's that stacks four query heads on a
KV head.  That kernel writes a query row without any admissible key (the left padding) as zeros;
nothing reads those rows.  :func:`acehip.integration.install_lm` installs a ratio-4 model only
with ``wide_gqa=True``.
"""
from __future__ import annotations

import logging
from typing import Dict, Iterator, Optional

import torch

from . import _ffi
from ._ffi import check, lib, ptr, stream_ptr
from .condition import EncoderStack, _rope_theta
from .config import DiTConfig

log = logging.getLogger("acehip")


class HipLMRuntime:
    """The native side of :class:`HipCausalLM`: a causal ``acehip_enc`` handle with a K/V cache,
    the embedding table and the ``lm_head`` weight."""

    def __init__(self, cfg: DiTConfig, device: int = 0, max_batch: int = 16, capacity: int = 8192,
                 prefill_tokens: Optional[int] = None, score_slots: int = 0):
        self.cfg = cfg
        self.device = torch.device("cuda", device)
        self.max_batch, self.capacity = max_batch, capacity
        # cache rows [max_batch, max_batch + score_slots) belong to HipCausalLM.score's prompt reuse.
        # One cache row is layers · kv_heads · capacity · 128 · 2 (K, V) · 2 bytes: at capacity 8192,
        # 0.94 GB for the 0.6B and 1.7B LMs (28 layers, 8 KV heads) and 1.21 GB for the 4B (36 layers,
        # 8 KV heads)
        self.score_slots = int(score_slots)
        self.cache_epoch = 0
        # prompt tokens of one prefill (B·S): the activation workspace is sized by it
        self.prefill_tokens = prefill_tokens or min(max_batch * capacity, 4 * capacity)
        self.stack = EncoderStack(cfg, cfg.num_hidden_layers, 0, device=device,
                                  max_tokens=max(self.prefill_tokens, max_batch), max_S=capacity, causal=True)
        self.table: Optional[torch.Tensor] = None
        self.w_head: Optional[torch.Tensor] = None

    def load(self, weights: Dict[str, torch.Tensor], lm_head: Optional[torch.Tensor] = None):
        """Qwen3Model state-dict names; ``lm_head`` [V, hidden] or None (tied to embed_tokens)."""
        emb = weights["embed_tokens.weight"]
        self.table = emb.detach().to(self.device, torch.bfloat16).contiguous()
        tied = lm_head is None or lm_head.data_ptr() == emb.data_ptr()
        self.w_head = self.table if tied else lm_head.detach().to(self.device, torch.bfloat16).contiguous()
        self.stack.load({k: v for k, v in weights.items() if k != "embed_tokens.weight"})
        check(lib().acehip_enc_kv_create(self.stack.h, self.max_batch + self.score_slots, self.capacity),
              "enc_kv_create")
        self.reset_score_cache()

    def reset_score_cache(self):
        """Whatever the scoring rows of the cache held is no longer valid: every
        :class:`HipCausalLM` on this runtime empties its slots before its next ``score``."""
        self.cache_epoch += 1

    @property
    def vocab(self) -> int:
        return self.w_head.shape[0]

    def embed(self, ids: torch.Tensor) -> torch.Tensor:
        return torch.nn.functional.embedding(ids.to(self.device), self.table)

    def prefill(self, x: torch.Tensor, kmask: Optional[torch.Tensor]) -> torch.Tensor:
        """x [B, S, D] bf16, kmask uint8 [B, S] contiguous or None → final-norm rows [B, D]."""
        x = x.contiguous()
        B, S, D = x.shape
        out = torch.empty(B, D, device=self.device, dtype=torch.bfloat16)
        check(lib().acehip_enc_prefill(self.stack.h, ptr(x), ptr(kmask), B, S, ptr(out), stream_ptr()), "enc_prefill")
        self._keep = (x, kmask)
        return out

    def decode(self, x: torch.Tensor, kmask: Optional[torch.Tensor], pos: int) -> torch.Tensor:
        """x [B, D] bf16 at cache index pos; kmask uint8 [rows, ld] over cache positions or None."""
        x = x.contiguous()
        B, D = x.shape
        out = torch.empty(B, D, device=self.device, dtype=torch.bfloat16)
        ld = kmask.stride(0) if kmask is not None else 0
        check(lib().acehip_enc_decode(self.stack.h, ptr(x), ptr(kmask), ld, B, pos, ptr(out), stream_ptr()),
              "enc_decode")
        self._keep = (x, kmask)
        return out

    def extend(self, x: torch.Tensor, kmask: Optional[torch.Tensor], row0: int, pos: int) -> torch.Tensor:
        """x [B, n, D] bf16: n tokens per sequence appended at cache positions [pos, pos + n) of
        cache rows row0 .. row0 + B − 1; kmask uint8 [rows, ld] over cache positions (row b for
        sequence b) or None → the final-norm row of every new position [B, n, D]
        (``acehip_enc_extend``)."""
        x = x.contiguous()
        B, n, D = x.shape
        out = torch.empty(B, n, D, device=self.device, dtype=torch.bfloat16)
        ld = kmask.stride(0) if kmask is not None else 0
        with torch.cuda.device(self.device):
            check(lib().acehip_enc_extend(self.stack.h, ptr(x), ptr(kmask), ld, row0, B, pos, n, ptr(out),
                                          stream_ptr()), "enc_extend")
        self._keep = (x, kmask)
        return out

    def lm_head(self, h: torch.Tensor) -> torch.Tensor:
        B, D = h.shape
        V = self.vocab
        y = torch.empty(B, V, device=self.device, dtype=torch.bfloat16)
        check(lib().acehip_lm_head_bf16(ptr(h), D, ptr(self.w_head), ptr(y), V, B, V, D, stream_ptr()), "lm_head")
        return y

    def forward_all(self, x: torch.Tensor) -> torch.Tensor:
        """x [B, S, D] bf16 → the final-norm row of every position [B, S, D] (causal, no padding
        mask).  Runs on the stack's activation workspace only: the K/V cache is not touched."""
        return self.stack.forward(x, None)

    def score_rows(self, h: torch.Tensor, targets: torch.Tensor):
        """h [T, D] bf16 rows (row stride >= D, a multiple of 8), targets [T] →
        (logprob fp32, lse fp32, n_greater int32, n_equal_lower int32), each [T]
        (``acehip_lm_score_bf16``).  The workspace is allocated on first use and kept."""
        if h.dim() != 2 or h.dtype != torch.bfloat16 or h.stride(1) != 1:
            h = h.to(self.device, torch.bfloat16).contiguous()
        T, D = h.shape
        V = self.vocab
        tg = targets.to(device=self.device, dtype=torch.int32).contiguous()
        need = int(lib().acehip_lm_score_ws_bytes(T, V))
        ws = getattr(self, "_score_ws", None)
        if ws is None or ws.numel() < need:
            ws = self._score_ws = torch.empty(need, dtype=torch.uint8, device=self.device)
        lp = torch.empty(T, device=self.device, dtype=torch.float32)
        lse = torch.empty(T, device=self.device, dtype=torch.float32)
        ng = torch.empty(T, device=self.device, dtype=torch.int32)
        ne = torch.empty(T, device=self.device, dtype=torch.int32)
        with torch.cuda.device(self.device):
            check(lib().acehip_lm_score_bf16(ptr(h), h.stride(0), ptr(self.w_head), ptr(tg), T, V, D, ptr(lp),
                                             ptr(lse), ptr(ng), ptr(ne), ptr(ws), ws.numel(), stream_ptr()), "lm_score")
        self._keep_score = (h, tg)
        return lp, lse, ng, ne

    def close(self):
        self.stack.close()


class HipKVCache:
    """What ``outputs.past_key_values`` is: a ticket for the K/V cache inside the handle."""

    def __init__(self, owner: "HipCausalLM", generation: int, batch: int, length: int):
        self._owner, self._generation = owner, generation
        self.batch, self.length = batch, length

    def get_seq_length(self, layer_idx: int = 0) -> int:
        return self.length


class CausalLMOutput:
    def __init__(self, logits: torch.Tensor, past_key_values):
        self.logits = logits
        self.past_key_values = past_key_values


class HipCausalLM:
    """Drop-in for ``LLMHandler.llm`` on the ``pt`` backend (see the module docstring).

    ``runtime`` provides ``device``, ``max_batch``, ``capacity``, ``embed``, ``prefill``,
    ``decode`` and ``lm_head``, for :meth:`score` ``forward_all`` and ``score_rows``, and for
    :meth:`extend` and the prompt-reusing :meth:`score` ``extend`` (and ``score_slots``)
    (:class:`HipLMRuntime`; the host tests inject a stand-in)."""

    def __init__(self, runtime, wrapped=None, fallback: bool = False):
        self.rt = runtime
        self.wrapped = wrapped
        self.fallback = fallback and wrapped is not None
        self.device = runtime.device
        self.max_batch, self.capacity = runtime.max_batch, runtime.capacity
        # key mask over cache positions, and (for the fallback) the tokens fed so far
        self._mask = torch.zeros(self.max_batch, self.capacity, dtype=torch.uint8, device=self.device)
        self._ids = (torch.zeros(self.max_batch, self.capacity, dtype=torch.long, device=self.device)
                     if self.fallback else None)
        self._masked = False
        self._generation = 0
        self._cache: Optional[HipKVCache] = None
        self._delegating = False     # fallback: the rest of this generation runs on the wrapped module
        # prompt-reusing scoring: slot s is cache row max_batch + s; _slot_ids[s] is the CPU id
        # tensor whose K/V that row holds (None: empty), _slot_used[s] the call that last took it
        self.score_slots = int(getattr(runtime, "score_slots", 0) or 0)
        self._slot_ids = [None] * self.score_slots
        self._slot_used = [0] * self.score_slots
        self._slot_tick = 0
        self._slot_epoch = getattr(runtime, "cache_epoch", 0)
        self.score_stats = {"calls": 0, "tokens_computed": 0, "tokens_reused": 0, "last_start": None}

    @classmethod
    def from_reference_model(cls, model, max_batch: int = 16, capacity: int = 8192, fallback: bool = False,
                             device: Optional[int] = None, **kw) -> "HipCausalLM":
        """From a loaded transformers ``Qwen3ForCausalLM``."""
        c = model.config
        cfg = DiTConfig(hidden_size=c.hidden_size, intermediate_size=c.intermediate_size,
                        num_hidden_layers=c.num_hidden_layers, num_attention_heads=c.num_attention_heads,
                        num_key_value_heads=c.num_key_value_heads,
                        head_dim=getattr(c, "head_dim", c.hidden_size // c.num_attention_heads),
                        rms_norm_eps=c.rms_norm_eps, rope_theta=_rope_theta(c))
        if device is None:
            p = next(model.parameters()).device
            device = p.index or 0 if p.type == "cuda" else 0
        rt = HipLMRuntime(cfg, device, max_batch=max_batch, capacity=capacity, **kw)
        # lm_head.weight itself (tied to embed_tokens on the released checkpoints; an untied one works too)
        sd = model.model.state_dict()
        head = model.lm_head.weight
        rt.load(sd, None if head.data_ptr() == sd["embed_tokens.weight"].data_ptr() else head)
        return cls(rt, wrapped=model, fallback=fallback)

    # ------------------------------------------------------------------ the call contract
    def __call__(self, input_ids=None, attention_mask=None, past_key_values=None, use_cache=True, **kw):
        if input_ids is None or input_ids.dim() != 2:
            raise ValueError("HipCausalLM: input_ids [B, S] is required (inputs_embeds is not supported)")
        if self._delegating and past_key_values is not None and not isinstance(past_key_values, HipKVCache):
            return self.wrapped(input_ids=input_ids, attention_mask=attention_mask,
                                past_key_values=past_key_values, use_cache=use_cache, **kw)
        if past_key_values is None:
            self._delegating = False
            self._check_prefill(input_ids, attention_mask)
        else:
            self._check_decode(input_ids, attention_mask, past_key_values)
        try:
            if past_key_values is None:
                return self._prefill(input_ids, attention_mask, use_cache)
            return self._decode(input_ids, attention_mask, past_key_values)
        except RuntimeError as e:
            if not self.fallback:
                raise
            log.warning("acehip LM call failed (%s); this generation continues on PyTorch", e)
            return self._fall_back(input_ids, attention_mask, past_key_values, use_cache, kw)

    forward = __call__

    def _check_prefill(self, ids, mask):
        B, S = ids.shape
        if B > self.max_batch or S > self.capacity or S < 1 or B < 1:
            raise ValueError(f"HipCausalLM: prompt [{B}, {S}] exceeds max_batch {self.max_batch} / "
                             f"capacity {self.capacity}")
        limit = getattr(self.rt, "prefill_tokens", None)
        if limit is not None and B * S > limit:
            raise ValueError(f"HipCausalLM: prompt [{B}, {S}] has {B * S} tokens, more than the runtime's "
                             f"prefill_tokens {limit}")
        if mask is not None and tuple(mask.shape) != (B, S):
            raise ValueError(f"HipCausalLM: attention_mask {tuple(mask.shape)} does not match input_ids [{B}, {S}]")

    def _check_decode(self, ids, mask, past):
        if not isinstance(past, HipKVCache) or past._owner is not self:
            raise ValueError("HipCausalLM: past_key_values is not a cache this model returned (foreign cache)")
        if past is not self._cache or past._generation != self._generation:
            raise ValueError("HipCausalLM: past_key_values is stale (a later prefill reset the cache)")
        B, n = ids.shape
        if n != 1:
            raise ValueError(f"HipCausalLM: with past_key_values, input_ids must be [B, 1] (got {n} new tokens)")
        if B != past.batch:
            raise ValueError(f"HipCausalLM: batch changed from {past.batch} to {B} within one generation")
        if past.length >= self.capacity:
            raise ValueError(f"HipCausalLM: the K/V cache is full (capacity {self.capacity})")
        if mask is not None and tuple(mask.shape) != (B, past.length + 1):
            raise ValueError(f"HipCausalLM: attention_mask {tuple(mask.shape)} must be [{B}, {past.length + 1}]")

    def _prefill(self, ids, mask, use_cache):
        B, S = ids.shape
        self._generation += 1
        self._cache = None
        km = None
        if mask is not None:
            km = (mask != 0).to(device=self.device, dtype=torch.uint8).contiguous()
            self._mask[:B, :S] = km
        else:
            self._mask[:B, :S] = 1
        self._masked = mask is not None
        if self._ids is not None:
            self._ids[:B, :S] = ids.to(self.device)
        h = self.rt.prefill(self.rt.embed(ids), km)
        logits = self.rt.lm_head(h).unsqueeze(1)
        if use_cache:
            self._cache = HipKVCache(self, self._generation, B, S)
        return CausalLMOutput(logits, self._cache)

    def _decode(self, ids, mask, past):
        B, pos = past.batch, past.length
        # column pos of the key mask from the last column of the mask given: a device op
        if mask is not None:
            self._mask[:B, pos] = (mask[:, -1] != 0).to(device=self.device, dtype=torch.uint8)
            self._masked = True
        else:
            self._mask[:B, pos] = 1
        if self._ids is not None:
            self._ids[:B, pos] = ids[:, 0].to(self.device)
        h = self.rt.decode(self.rt.embed(ids[:, 0]), self._mask if self._masked else None, pos)
        logits = self.rt.lm_head(h).unsqueeze(1)
        past.length = pos + 1
        return CausalLMOutput(logits, past)

    def _fall_back(self, ids, mask, past, use_cache, kw, new: int = 1, keep: int = 1):
        """The failing call and the rest of this generation on the wrapped module: it is given
        the whole sequence so far (prompt and every token fed since, the `new` of this call
        included) and builds its own cache; the logits of the last `keep` positions return."""
        self._delegating = True
        if past is not None:
            B, n = past.batch, past.length + new
            ids = self._ids[:B, :n].to(ids.device)
            self._cache = None
        out = self.wrapped(input_ids=ids, attention_mask=mask, use_cache=use_cache, **kw)
        return CausalLMOutput(out.logits[:, -keep:, :], getattr(out, "past_key_values", None))

    # ------------------------------------------------------------------ multi-token continuation
    def extend(self, input_ids, past_key_values, attention_mask=None, logits: str = "last", **kw):
        """``model(input_ids[B, n], past_key_values, attention_mask[B, past + n])``: n >= 1 new tokens
        per sequence appended to a running generation in one pass (``acehip_enc_extend``).  The
        ticket is checked as in ``__call__`` (foreign or stale cache, changed batch), the cache
        must hold ``past.length + n`` positions and a mask, if given, is ``[B, past.length + n]``.
        Returns logits ``[B, 1, V]`` of the last new position, or with ``logits="all"`` ``[B, n, V]``
        of every new position, and the same ticket advanced by n.  ``__call__`` itself keeps
        refusing more than one new token."""
        if logits not in ("last", "all"):
            raise ValueError("HipCausalLM.extend: logits must be 'last' or 'all'")
        if input_ids is None or input_ids.dim() != 2 or input_ids.shape[1] < 1:
            raise ValueError("HipCausalLM.extend: input_ids [B, n >= 1] is required")
        n = input_ids.shape[1]
        keep = n if logits == "all" else 1
        if self._delegating and past_key_values is not None and not isinstance(past_key_values, HipKVCache):
            out = self.wrapped(input_ids=input_ids, attention_mask=attention_mask,
                               past_key_values=past_key_values, use_cache=True, **kw)
            return CausalLMOutput(out.logits[:, -keep:, :], getattr(out, "past_key_values", None))
        self._check_extend(input_ids, attention_mask, past_key_values)
        try:
            return self._extend(input_ids, attention_mask, past_key_values, keep)
        except RuntimeError as e:
            if not self.fallback:
                raise
            log.warning("acehip LM call failed (%s); this generation continues on PyTorch", e)
            return self._fall_back(input_ids, attention_mask, past_key_values, True, kw, new=n, keep=keep)

    def _check_extend(self, ids, mask, past):
        if not isinstance(past, HipKVCache) or past._owner is not self:
            raise ValueError("HipCausalLM: past_key_values is not a cache this model returned (foreign cache)")
        if past is not self._cache or past._generation != self._generation:
            raise ValueError("HipCausalLM: past_key_values is stale (a later prefill reset the cache)")
        B, n = ids.shape
        if B != past.batch:
            raise ValueError(f"HipCausalLM: batch changed from {past.batch} to {B} within one generation")
        if past.length + n > self.capacity:
            raise ValueError(f"HipCausalLM: {past.length} cached + {n} new tokens exceed the K/V cache "
                             f"(capacity {self.capacity})")
        limit = getattr(self.rt, "prefill_tokens", None)
        if limit is not None and B * n > max(limit, self.max_batch):
            raise ValueError(f"HipCausalLM: [{B}, {n}] new tokens exceed the runtime's prefill_tokens {limit}")
        if mask is not None and tuple(mask.shape) != (B, past.length + n):
            raise ValueError(f"HipCausalLM: attention_mask {tuple(mask.shape)} must be [{B}, {past.length + n}]")

    def _extend(self, ids, mask, past, keep):
        B, pos = past.batch, past.length
        n = ids.shape[1]
        if mask is not None:
            self._mask[:B, pos:pos + n] = (mask[:, -n:] != 0).to(device=self.device, dtype=torch.uint8)
            self._masked = True
        else:
            self._mask[:B, pos:pos + n] = 1
        if self._ids is not None:
            self._ids[:B, pos:pos + n] = ids.to(self.device)
        h = self.rt.extend(self.rt.embed(ids), self._mask if self._masked else None, 0, pos)   # [B, n, D]
        rows = h[:, n - keep:].reshape(B * keep, h.shape[-1])
        # lm_head takes at most 16 rows per call
        out = torch.cat([self.rt.lm_head(rows[i:i + 16].contiguous()) for i in range(0, B * keep, 16)], 0)
        past.length = pos + n
        return CausalLMOutput(out.reshape(B, keep, -1), past)

    # ------------------------------------------------------------------ scoring
    def reset_score_cache(self):
        """Empty every scoring slot: the next ``score`` of each starts from position 0."""
        self._slot_ids = [None] * self.score_slots
        self._slot_used = [0] * self.score_slots
        self._slot_epoch = getattr(self.rt, "cache_epoch", 0)

    def _take_slot(self, ids_cpu: torch.Tensor, prompt_len: int):
        """(slot, start) for a sequence: the slot whose cached ids share the longest prefix p with
        it (the least recently used among equals) and start = min(p, prompt_len − 1); without any
        shared prefix the least recently used slot (an empty one first) and start 0.  One
        refinement keeps two alternating prompts that share a template prefix apart: a match that
        does not cover the prompt (p < prompt_len − 1) yields to an empty slot while there is one."""
        def prefix(a):
            m = min(a.numel(), ids_cpu.numel())
            ne = (a[:m] != ids_cpu[:m]).nonzero()
            return int(ne[0]) if ne.numel() else m
        ps = [prefix(a) if a is not None else 0 for a in self._slot_ids]
        lru = sorted(range(self.score_slots), key=lambda s: (self._slot_ids[s] is not None, self._slot_used[s], s))
        best = max(lru, key=lambda s: ps[s])          # max keeps the first of equals: LRU order
        if ps[best] == 0 or (ps[best] < prompt_len - 1 and self._slot_ids[lru[0]] is None):
            return lru[0], 0
        return best, min(ps[best], prompt_len - 1)

    def score(self, input_ids: torch.Tensor, prompt_len: int, reuse: bool = True):
        """Teacher-forced scoring of ``input_ids[0, prompt_len:]`` given what precedes each token
        (``core/scoring/lm_score.py:160-171``): → (logprob fp32 [T], rank int64 [T]), T = S − prompt_len.

        Row j is the target ``ids[prompt_len + j]`` under the distribution predicted at position
        ``prompt_len − 1 + j``; ``rank`` is 1-based, equal logits ranked by lower token id first
        (``1 + n_greater + n_equal_lower``).  The logits are those of a bf16 ``lm_head``
        (fp32 accumulate, rounded to bf16); the log-sum-exp and the log-probabilities are fp32.
        Nothing of a running generation is touched: not its K/V cache rows, the key mask, the
        generation counter or the cache ticket.

        On a runtime with ``score_slots`` and with ``reuse`` the prompt's K/V is kept between
        calls: each slot is a cache row past the generation's and remembers the ids it holds; a
        call continues from the longest prefix a slot shares with it (``acehip_enc_extend`` over
        positions [start, S) only) and leaves the whole sequence in that slot.  A failing call
        leaves its slot empty.  ``score_stats`` counts calls and tokens computed / reused.
        Without slots, or with ``reuse=False``, one ``acehip_enc_forward`` covers the sequence."""
        if input_ids is None or input_ids.dim() != 2 or input_ids.shape[0] != 1:
            raise ValueError("HipCausalLM.score: input_ids [1, S] is required")
        S = input_ids.shape[1]
        prompt_len = int(prompt_len)
        if S > self.capacity:
            raise ValueError(f"HipCausalLM.score: {S} tokens exceed the capacity {self.capacity}")
        limit = getattr(self.rt, "prefill_tokens", None)
        if limit is not None and S > limit:
            raise ValueError(f"HipCausalLM.score: {S} tokens exceed the runtime's prefill_tokens {limit}")
        if not 1 <= prompt_len < S:
            raise ValueError(f"HipCausalLM.score: need 1 <= prompt_len < S (got prompt_len {prompt_len}, S {S})")
        ids = input_ids.to(self.device)
        if not (reuse and self.score_slots > 0):
            h = self.rt.forward_all(self.rt.embed(ids))[0]
            lp, _, ng, ne = self.rt.score_rows(h[prompt_len - 1:S - 1], ids[0, prompt_len:])
            return lp, 1 + ng.to(torch.int64) + ne.to(torch.int64)
        if self._slot_epoch != getattr(self.rt, "cache_epoch", 0):
            self.reset_score_cache()
        ids_cpu = input_ids[0].detach().to("cpu", torch.long)
        slot, start = self._take_slot(ids_cpu, prompt_len)
        self._slot_ids[slot] = None              # empty until the call has succeeded
        self._slot_tick += 1
        self._slot_used[slot] = self._slot_tick
        h = self.rt.extend(self.rt.embed(ids[:, start:]), None, self.max_batch + slot, start)[0]
        lp, _, ng, ne = self.rt.score_rows(h[prompt_len - 1 - start:S - 1 - start], ids[0, prompt_len:])
        self._slot_ids[slot] = ids_cpu
        st = self.score_stats                    # calls that succeeded
        st["calls"] += 1
        st["last_start"] = start
        st["tokens_computed"] += S - start
        st["tokens_reused"] += start
        return lp, 1 + ng.to(torch.int64) + ne.to(torch.int64)

    # ------------------------------------------------------------------ pass-throughs
    @property
    def config(self):
        return self.wrapped.config

    @property
    def generation_config(self):
        return self.wrapped.generation_config

    def generate(self, *a, **k):
        """No CFG and no constrained decoding (llm_inference.py:946): transformers' own loop."""
        return self.wrapped.generate(*a, **k)

    def parameters(self) -> Iterator[torch.Tensor]:
        """One tensor on the handle's device: ``_load_model_context`` (llm_inference.py:3835-3890)
        then sees the model as already there."""
        yield self._mask if getattr(self.rt, "w_head", None) is None else self.rt.w_head

    def to(self, *a, **k) -> "HipCausalLM":
        return self

    def eval(self) -> "HipCausalLM":
        return self

    def close(self):
        close = getattr(self.rt, "close", None)
        if close:
            close()


class HipLogitFilters:
    """``LLMHandler._apply_top_k_filter`` / ``_apply_top_p_filter`` (``acestep/llm_inference.py:367-385``)
    on ``acehip_lm_filter``: the same signatures, the logits filtered in place and the same tensor
    object returned, each method with the other filter off.

    A method calls the original it was built with — never the kernel — when its filter is
    switched off (top_k ``None`` / ``<= 0``; top_p ``None`` or outside (0, 1)) or when ``logits``
    is not a 2-D CUDA tensor of unit inner stride and dtype float32 or bfloat16 (the MLX bridge's
    CPU tensors, ``:3646-3647``).  ``fallback``: an acehip error in a call is logged and that call
    runs on the original.  The workspace is per device, allocated on first use and kept."""

    def __init__(self, orig_top_k, orig_top_p, fallback: bool = False, max_batch: int = 16, vocab: int = 1 << 18):
        self.orig_top_k, self.orig_top_p = orig_top_k, orig_top_p
        self.fallback = fallback
        self.max_batch, self.vocab = max_batch, vocab
        self._ws: Dict[torch.device, torch.Tensor] = {}

    @staticmethod
    def eligible(logits) -> bool:
        return (isinstance(logits, torch.Tensor) and logits.is_cuda and logits.dim() == 2 and logits.numel() > 0
                and logits.stride(1) == 1 and logits.stride(0) >= logits.shape[1]
                and logits.dtype in (torch.float32, torch.bfloat16))

    def _workspace(self, logits: torch.Tensor) -> torch.Tensor:
        B, V = logits.shape
        need = int(lib().acehip_lm_filter_ws_bytes(B, V))
        ws = self._ws.get(logits.device)
        if ws is None or ws.numel() < need:
            need = max(need, int(lib().acehip_lm_filter_ws_bytes(max(B, self.max_batch), max(V, self.vocab))))
            ws = torch.empty(need, dtype=torch.uint8, device=logits.device)
            self._ws[logits.device] = ws
        return ws

    def _run(self, logits: torch.Tensor, top_k: int, top_p: float) -> torch.Tensor:
        B, V = logits.shape
        ws = self._workspace(logits)
        with torch.cuda.device(logits.device):
            check(lib().acehip_lm_filter(ptr(logits), _ffi.dtype_code(logits), logits.stride(0), B, V, top_k, top_p,
                                         ptr(ws), ws.numel(), stream_ptr()), "lm_filter")
        return logits

    def top_k(self, logits, top_k):
        if top_k is None or top_k <= 0 or not self.eligible(logits):
            return self.orig_top_k(logits, top_k)
        if top_k >= logits.shape[1]:          # torch.topk's own error for k > V; k == V removes nothing
            return self.orig_top_k(logits, top_k)
        try:
            return self._run(logits, int(top_k), 0.0)
        except RuntimeError as e:
            if not self.fallback:
                raise
            log.warning("acehip top-k filter failed (%s); this call runs on PyTorch", e)
            return self.orig_top_k(logits, top_k)

    def top_p(self, logits, top_p):
        if top_p is None or not 0.0 < top_p < 1.0 or not self.eligible(logits):
            return self.orig_top_p(logits, top_p)
        try:
            return self._run(logits, 0, float(top_p))
        except RuntimeError as e:
            if not self.fallback:
                raise
            log.warning("acehip top-p filter failed (%s); this call runs on PyTorch", e)
            return self.orig_top_p(logits, top_p)
