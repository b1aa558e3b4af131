"""Plug acehip into a running reference ``AceStepHandler`` (no caller edits).

Seams:
  * init   — ``_initialize_mlx_backends`` (``init_service_setup.py:116-148``) is
             where the reference converts weights for an alternative backend;
             :func:`install` does the same from ``handler.model`` /
             ``handler.vae`` state dicts.
  * DiT    — ``self.model.generate_audio(**generate_kwargs)``
             (``service_generate_execute.py:191,194``): replaced by
             :class:`~acehip.dit.AceStepDiTBackend.generate_audio` with the
             reference's own ``prepare_condition`` for the conditioning.
  * VAE    — ``handler.vae.decode(z).sample`` (``vae_decode_chunks.py:42,95``)
             and ``handler.vae.encode(x).latent_dist.sample()``
             (``vae_encode.py:65``): replaced by :class:`~acehip.vae.OobleckBackend`;
             ``handler.tiled_encode`` (``vae_encode.py:15-82``: 30 s chunks, 2 s
             overlap, per-chunk host offload) becomes ONE untiled encode;
             ``handler.tiled_decode`` (``vae_decode.py:16-85``, called at
             ``generate_music_decode.py:164``) becomes ONE untiled decode of the
             whole batch — the reference's overlap-discard windows (1.6x the useful
             frames at 240 s) are redundant because the decoder's receptive field
             (-8.2/+9.2 frames) is inside the 64-frame overlap (tiled == untiled,
             tests/test_gpu_long.py).

  * cond   — ``prepare_condition`` (``base:1607-1652``, called from
             ``generate_audio`` ``base:1820``): replaced by
             :class:`~acehip.condition.HipPrepareCondition` (text projector, lyric
             and timbre encoders, and for covers the audio tokenizer (pooler + FSQ)
             and detokenizer, all on libacehip).
  * LoRA   — ``add_lora`` / ``remove_lora`` / ``unload_lora`` / ``set_lora_scale`` /
             ``set_use_lora`` / ``set_active_lora_adapter`` (``handler/lora/lifecycle.py:164-420``,
             ``lora/controls.py:12-157``) change the decoder's effective weights;
             :func:`install` wraps them so the merged weights are re-packed into the
             handle afterwards (:func:`refresh_decoder_weights`).
  * lyrics — ``handler.get_lyric_timestamp`` / ``handler.get_lyric_score``
             (``handler/lyric_timestamp.py:15-147``, ``lyric_score.py:15-166``; the LRC
             button and the score of ``ui/gradio/events/results``) call
             ``self.model.decoder(..., output_attentions=True, custom_layers_config,
             enable_early_exit=True)``: replaced by :class:`~acehip.alignment.LyricAlignment`,
             which takes the selected heads' cross-attention maps from the DiT handle
             (``acehip_dit_forward_capture``: the re-packed weights, LoRA included, a stop
             after the highest selected layer) and hands them to the reference's own aligners.
             The capture overwrites the handle's cross K/V cache; ``generate_audio`` re-sets
             it on every request.

  * LM     — ``LLMHandler.llm`` on the ``pt`` backend (the one ROCm users get: nano-vllm needs
             flash-attn and Triton): the 5 Hz planner's token loops call it only through
             ``_forward_pass`` (``llm_inference.py:416-438``).  :func:`install_lm` — a separate
             call on the ``LLMHandler``, :func:`install` does not touch it — replaces it with
             :class:`~acehip.lm.HipCausalLM` (prefill + one-token decode over a K/V cache in the
             handle, vocabulary projection); the logits processors, sampling and ``generate()``
             stay in torch.  With ``filters=True`` the
             handler's ``_apply_top_k_filter`` / ``_apply_top_p_filter`` (``:367-385``) are rebound
             to :class:`~acehip.lm.HipLogitFilters` (``acehip_lm_filter``).

  * score  — ``acestep/core/scoring/lm_score.py``, the auto-score of every generated song:
             :func:`install_lm_score` rebinds its ``_calculate_log_prob`` /
             ``_calculate_topk_recall`` to :meth:`~acehip.lm.HipCausalLM.score` (one forward over
             prompt + target, then ``acehip_lm_score_bf16``: per target token the log-probability
             and the rank, without the ``[S, V]`` logits).

Failure policy: by default an acehip error propagates (the request fails
loudly, ``generate_music.py:181-190`` turns it into an error payload).  The
MLX precedent instead logs and falls back to the PyTorch path
(``service_generate_execute.py:189-191``); pass ``fallback=True`` to get that
behaviour — the fallback is the reference's own GPU path, never a CPU path.
"""
from __future__ import annotations

import logging
from typing import Optional

import torch

from .condition import AudioDetokenizer, AudioTokenizer, ConditionEncoder, HipPrepareCondition, TextEncoder
from .config import VAEConfig
from .alignment import LyricAlignment
from .dit import AceStepDiTBackend
from .vae import OobleckBackend

log = logging.getLogger("acehip")


def vae_from_diffusers(vae, max_seconds: float = 600.0, with_encoder: bool = True,
                       max_batch: int = 8) -> OobleckBackend:
    """Build an OobleckBackend from a loaded diffusers ``AutoencoderOobleck``
    (precedent: ``acestep/models/mlx/vae_convert.py:37-132``)."""
    c = vae.config
    cfg = VAEConfig(encoder_hidden_size=c.encoder_hidden_size,
                    downsampling_ratios=list(c.downsampling_ratios),
                    channel_multiples=list(c.channel_multiples), decoder_channels=c.decoder_channels,
                    decoder_input_channels=c.decoder_input_channels, audio_channels=c.audio_channels)
    dev = next(vae.parameters()).device
    be = OobleckBackend(cfg, dev.index or 0, max_T=int(max_seconds * 48000 / cfg.hop_length) + 1,
                        max_B=max_batch, with_encoder=with_encoder)
    be.load(vae.state_dict())
    return be


def merged_decoder_state_dict(decoder) -> dict:
    """Effective (adapter-merged) decoder weights under the plain HF names.

    Works on a bare ``AceStepDiTModel`` and on a PEFT-wrapped one (``PeftModel``
    / LoRA layers with ``base_layer`` + ``get_delta_weight``, as created by
    ``lifecycle.py:249-258``; LyCORIS LoKr modules expose the same two): every
    adapted Linear becomes ``base.weight + Σ_active get_delta_weight(a)`` unless
    the adapters are disabled or already merged; PEFT's name decorations
    (``base_model.model.``, ``.base_layer``) are stripped."""
    out = {}
    with torch.no_grad():
        for name, mod in decoder.named_modules():
            base = getattr(mod, "base_layer", None)
            if base is None or not hasattr(mod, "get_delta_weight"):
                continue
            w = base.weight.detach().float().clone()
            if not getattr(mod, "disable_adapters", False) and not getattr(mod, "merged", False):
                act = getattr(mod, "active_adapters", None) or []
                for a in ([act] if isinstance(act, str) else act):
                    try:
                        w += mod.get_delta_weight(a).float()
                    except KeyError:      # adapter not present on this layer
                        pass
            out[name + ".weight"] = w
            if getattr(base, "bias", None) is not None:
                out[name + ".bias"] = base.bias.detach()
        for k, v in decoder.state_dict().items():
            if ".base_layer." in k or "lora_" in k or "lokr_" in k or ".hada_" in k:
                continue
            out.setdefault(k, v)
    clean = {}
    for k, v in out.items():
        if k.startswith("base_model.model."):
            k = k[len("base_model.model."):]
        clean[k.replace(".base_layer", "")] = v
    return clean


def refresh_decoder_weights(dit: AceStepDiTBackend, decoder) -> None:
    """Re-pack the decoder's current effective weights into the DiT handle
    (§8f row 3: LoRA add/remove/scale changes)."""
    dit.rt.load(merged_decoder_state_dict(decoder))


_LORA_METHODS = ("add_lora", "load_lora", "add_voice_lora", "remove_lora", "unload_lora", "set_lora_scale",
                 "set_use_lora", "set_active_lora_adapter")


def install(handler, max_seconds: float = 600.0, max_batch: int = 8, fallback: bool = False,
            vae: bool = True, condition: bool = True, text_encoder: bool = True,
            lyric_alignment: bool = True) -> dict:
    """Swap the handler's DiT sampler, VAE, (Qwen3) text encoder and the decoder call of its
    lyric timestamp / score methods for the acehip backends."""
    dit = AceStepDiTBackend.from_reference_model(handler.model, max_seconds=max_seconds,
                                                 max_batch=max_batch)
    if condition:
        ce = ConditionEncoder.from_reference_model(handler.model, max_batch=max_batch)
        tok = det = None
        m = handler.model
        if getattr(m, "tokenizer", None) is not None and getattr(m, "detokenizer", None) is not None:
            dev = ce.device.index or 0
            patches = int(max_seconds * 25) // ce.cfg.pool_window_size + 1
            tok = AudioTokenizer(ce.cfg, dev, max_patches=max_batch * patches)
            tok.load({"tokenizer." + k: v for k, v in m.tokenizer.state_dict().items()})
            det = AudioDetokenizer(ce.cfg, dev, max_patches=max_batch * patches)
            det.load({"detokenizer." + k: v for k, v in m.detokenizer.state_dict().items()})
        hip_prep = HipPrepareCondition(ce, fallback=m.prepare_condition, tokenizer=tok, detokenizer=det)
        # the handler calls prepare_condition itself (service_generate_execute.py:123-142) and then
        # generate_audio calls it again on the same payload (base:1820): the handler's call records
        # its outputs, generate_audio's consumes them — one encoder pass per request
        dit.prepare_condition = hip_prep.consume
        m.prepare_condition = hip_prep.record
        out_prep = hip_prep
    orig_generate = handler.model.generate_audio

    def generate_audio(**kw):
        try:
            return dit.generate_audio(**kw)
        except Exception as e:  # pragma: no cover - exercised only with fallback=True
            if not fallback:
                raise
            log.warning("acehip generate_audio failed (%s); falling back to PyTorch", e)
            return orig_generate(**kw)

    handler.model.generate_audio = generate_audio
    out = {"dit": dit}
    if condition:
        out["prepare_condition"] = out_prep

    if lyric_alignment and (hasattr(handler, "get_lyric_timestamp") or hasattr(handler, "get_lyric_score")):
        out["lyric_alignment"] = LyricAlignment(handler, dit, fallback=fallback).bind()

    # LoRA lifecycle: after any adapter change re-pack the merged decoder weights
    for meth in _LORA_METHODS:
        orig = getattr(handler, meth, None)
        if orig is None:
            continue

        def wrapped(*a, _orig=orig, **k):
            res = _orig(*a, **k)
            refresh_decoder_weights(dit, handler.model.decoder)
            return res
        setattr(handler, meth, wrapped)
    if text_encoder and getattr(handler, "text_encoder", None) is not None:
        # infer_text_embeddings / infer_lyric_embeddings (conditioning_embed.py:71-79)
        te = TextEncoder.from_reference_model(handler.text_encoder, device=dit.rt.device.index or 0,
                                              max_batch=max_batch)
        handler.text_encoder = te
        out["text_encoder"] = te
    if vae and getattr(handler, "vae", None) is not None:
        vb = vae_from_diffusers(handler.vae, max_seconds=max_seconds, max_batch=max_batch)
        orig_decode, orig_encode = handler.vae.decode, handler.vae.encode

        def decode(z, *a, **k):
            try:
                return vb.decode(z)
            except Exception as e:  # pragma: no cover
                if not fallback:
                    raise
                log.warning("acehip vae.decode failed (%s); falling back", e)
                return orig_decode(z, *a, **k)

        def encode(x, *a, **k):
            try:
                return vb.encode(x)
            except Exception as e:  # pragma: no cover
                if not fallback:
                    raise
                log.warning("acehip vae.encode failed (%s); falling back", e)
                return orig_encode(x, *a, **k)

        handler.vae.decode = decode
        handler.vae.encode = encode
        orig_tiled = getattr(handler, "tiled_decode", None)

        def tiled_decode(latents, chunk_size=None, overlap=64, offload_wav_to_cpu=None):
            # vae_decode.py:16-85 contract: [B, 64, T] -> [B, 2, T*hop]; untiled here.
            # None resolves through the handler's policy as the reference does (:53-54)
            if offload_wav_to_cpu is None and hasattr(handler, "_should_offload_wav_to_cpu"):
                offload_wav_to_cpu = bool(handler._should_offload_wav_to_cpu())
            try:
                return vb.tiled_decode(latents, chunk_size, overlap, offload_wav_to_cpu)
            except Exception as e:  # pragma: no cover
                if not fallback or orig_tiled is None:
                    raise
                log.warning("acehip tiled_decode failed (%s); falling back", e)
                return orig_tiled(latents, chunk_size=chunk_size, overlap=overlap,
                                  offload_wav_to_cpu=offload_wav_to_cpu)
        handler.tiled_decode = tiled_decode
        orig_tiled_enc = getattr(handler, "tiled_encode", None)

        def tiled_encode(audio, chunk_size=None, overlap=None, offload_latent_to_cpu=True):
            # vae_encode.py:15-82 contract (batch_prep.py:70, conditioning_embed.py:58):
            # ONE untiled encode instead of the 30 s chunk loop
            try:
                return vb.tiled_encode(audio, chunk_size, overlap, offload_latent_to_cpu)
            except Exception as e:  # pragma: no cover
                if not fallback or orig_tiled_enc is None:
                    raise
                log.warning("acehip tiled_encode failed (%s); falling back", e)
                return orig_tiled_enc(audio, chunk_size=chunk_size, overlap=overlap,
                                      offload_latent_to_cpu=offload_latent_to_cpu)
        handler.tiled_encode = tiled_encode
        out["vae"] = vb
    return out


def install_lm(llm_handler, capacity: int = 8192, max_batch: int = 16, fallback: bool = False, runtime=None,
               filters: bool = False, wide_gqa: bool = False, **kw) -> dict:
    """Put the 5 Hz LM's token loop on libacehip: ``llm_handler.llm`` (a transformers
    ``Qwen3ForCausalLM`` on the ``pt`` backend) becomes a :class:`~acehip.lm.HipCausalLM`.

    Nothing is changed — and the returned dict says why under ``"skipped"`` — when the
    handler's backend is not ``pt`` or the model's heads / kv_heads ratio is not 1 or 2.
    ``wide_gqa=True`` also installs a model of ratio 4 — the 4B LM, 32 / 8 heads — exactly like
    the others (``filters``, ``score_slots``, ``fallback`` and ``runtime`` behave the same): its
    prefill and its scoring forward run their attention on ``acehip_attention_extend_bf16``
    instead of the flash kernels, which take ratios 1 and 2 only.  The switch is off by default,
    so a ratio-4 model is skipped as before; any other ratio is skipped either way.
    ``get_hf_model_for_scoring`` is rebound to return the original module: the
    reference's own scoring functions (``core/scoring/lm_score.py``) call a model for logits at
    every position, which :class:`~acehip.lm.HipCausalLM` does not serve — :func:`install_lm_score`
    puts scoring on the HIP path and keeps this binding for its fallback.  ``fallback=True``: an acehip
    error in a call is logged and that call and the rest of the generation run on the original
    module, the policy of :func:`install`.  ``runtime``: an already built
    :class:`~acehip.lm.HipLMRuntime` (or, in the host tests, a stand-in) instead of one built
    from the model's weights.  Further keywords go to :class:`~acehip.lm.HipLMRuntime`:
    ``install_lm(handler, score_slots=2)`` adds two cache rows in which
    :meth:`~acehip.lm.HipCausalLM.score` keeps a prompt's K/V between the scoring calls that share
    it (two, because the conditional and the unconditional prompt alternate), so that a call
    computes its target's rows only.  A row is layers · kv_heads · capacity · 128 · 2 (K, V) · 2
    bytes: at capacity 8192, 0.94 GB for the 0.6B and 1.7B LMs (28 layers) and 1.21 GB for the 4B
    (36 layers).

    ``filters=True`` (and the LM itself installed): the handler's ``_apply_top_k_filter`` and
    ``_apply_top_p_filter`` (``llm_inference.py:367-385``, called through ``self`` by every loop)
    are rebound on the instance to a :class:`~acehip.lm.HipLogitFilters` (``acehip_lm_filter``:
    no sort, in place, the same tensor returned); the result carries it and the two originals
    under ``"filters"``.  A CPU tensor (the MLX bridge), another dtype or layout, or a
    switched-off filter goes to the original method; ``fallback=True`` covers an acehip error in
    a filter call the same way.  A handler that lacks one of the two methods keeps both as they
    are (logged).  ``_sample_tokens`` (temperature, softmax, multinomial), the CFG combination,
    the FSM processor and the repetition penalty stay as they are.  With ``filters=False``
    nothing about the handler's methods changes."""
    from .lm import HipCausalLM, HipLogitFilters
    backend = getattr(llm_handler, "llm_backend", None)
    if backend != "pt":
        log.info("acehip install_lm: llm_backend is %r, not 'pt'; nothing installed", backend)
        return {"lm": None, "skipped": f"llm_backend is {backend!r}, not 'pt'"}
    orig = llm_handler.llm
    c = orig.config
    ratio = c.num_attention_heads / c.num_key_value_heads
    supported = "1, 2 or 4" if wide_gqa else "1 or 2"
    if ratio not in ((1, 2, 4) if wide_gqa else (1, 2)):
        log.info("acehip install_lm: heads / kv_heads = %s (supported: %s); the LM stays on PyTorch", ratio, supported)
        return {"lm": None, "skipped": f"heads / kv_heads = {ratio:g} (supported: {supported})"}
    if runtime is not None:
        lm = HipCausalLM(runtime, wrapped=orig, fallback=fallback)
    else:
        lm = HipCausalLM.from_reference_model(orig, max_batch=max_batch, capacity=capacity, fallback=fallback, **kw)
    llm_handler.llm = lm
    llm_handler.get_hf_model_for_scoring = lambda: orig
    out = {"lm": lm, "original": orig}
    if filters:
        orig_k = getattr(llm_handler, "_apply_top_k_filter", None)
        orig_p = getattr(llm_handler, "_apply_top_p_filter", None)
        if orig_k is None or orig_p is None:
            log.info("acehip install_lm: the handler has no _apply_top_k_filter / _apply_top_p_filter; "
                     "the logit filters stay as they are")
        else:
            f = HipLogitFilters(orig_k, orig_p, fallback=fallback, max_batch=max_batch)
            llm_handler._apply_top_k_filter = f.top_k
            llm_handler._apply_top_p_filter = f.top_p
            out["filters"] = {"hip": f, "top_k": orig_k, "top_p": orig_p}
    return out


def recall_from_ranks(ranks, topk: int = 10):
    """``_calculate_topk_recall``'s result (``core/scoring/lm_score.py:201-232``) from the 1-based
    rank of every target token: a hit at k iff rank <= k, ``recall_per_k[k] = hits / T``, and the
    average over positions of ``1 - (rank - 1) / topk`` for the hits at k = topk (0 for a miss)."""
    n = len(ranks)
    recall_per_k = {k: sum(1 for r in ranks if r <= k) / n if n > 0 else 0.0 for k in range(1, topk + 1)}
    position_scores = [1.0 - (r - 1) / topk for r in ranks if r <= topk]
    position_scores += [0.0] * (n - len(position_scores))
    return (sum(position_scores) / len(position_scores) if position_scores else 0.0), recall_per_k


def install_lm_score(llm_handler, lm_score_module=None, fallback: bool = False) -> dict:
    """Put the LM's scoring (``acestep/core/scoring/lm_score.py``) on libacehip: the module
    attributes ``_calculate_log_prob`` and ``_calculate_topk_recall`` are rebound, which their
    callers ``calculate_pmi_score_per_condition`` and ``_calculate_metadata_recall`` look up as
    module globals at call time — no caller changes.  ``lm_score_module``: the module object
    (None imports ``acestep.core.scoring.lm_score`` lazily).  Returns the two originals under
    ``"original"``.

    The replacements keep the reference's signatures and return types.  They repeat its
    tokenisation (``:144-158``: the prompt alone for ``prompt_len``, the full text with
    ``truncation=True``; an empty or fully truncated target returns ``-inf``, respectively
    ``(0.0, {})``), run under ``llm_handler._load_model_context()`` and score with
    ``llm_handler.llm.score`` (:meth:`acehip.lm.HipCausalLM.score`: one forward over the sequence
    and the fused vocabulary projection ``acehip_lm_score_bf16``; no ``[S, V]`` logits, no copy of
    them to the host).  When ``llm_handler.llm`` is not a :class:`~acehip.lm.HipCausalLM` (a handler
    on which :func:`install_lm` skipped, or another handler than the one installed on) the
    original function runs.  ``fallback=True``: an acehip ``RuntimeError`` in a call is logged and
    that call runs on the original function — on the original module, which
    ``get_hf_model_for_scoring`` still returns — the policy of :func:`install` and
    :func:`install_lm`.  Prompt reuse needs nothing here: it is decided inside ``score`` by the
    runtime's ``score_slots`` (``install_lm(handler, score_slots=2)``).

    Two deliberate differences from the reference's numbers:

    * the mean log-probability is the fp32 mean of fp32 per-token values (fp32 log-sum-exp over
      the bf16 logits).  The reference's ``log_softmax`` output and its mean are rounded to bf16,
      because its CPU logits are bf16 tensors; ours is the more accurate number;
    * top-k membership is decided by the target's rank ``1 + n_greater + n_equal_lower``: equal
      logits rank by lower token id first (the rule of ``acehip_lm_filter``).  ``torch.topk``'s
      order among equal values is unspecified, and bf16 logits tie often.  The recall values are
      the reference's formula on those ranks (:func:`recall_from_ranks`)."""
    from .lm import HipCausalLM
    if lm_score_module is None:
        import acestep.core.scoring.lm_score as lm_score_module
    orig_lp = lm_score_module._calculate_log_prob
    orig_recall = lm_score_module._calculate_topk_recall

    def _scored(handler, formatted_prompt, target_text):
        """(logprob fp32 [T], rank int64 [T]) on the host, or None for an empty / truncated target."""
        tokenizer = handler.llm_tokenizer
        prompt_len = tokenizer(formatted_prompt, return_tensors="pt", add_special_tokens=True)["input_ids"].shape[1]
        full = tokenizer(formatted_prompt + target_text, return_tensors="pt", padding=False, truncation=True,
                         add_special_tokens=True).to(handler.device)
        input_ids = full["input_ids"]
        if input_ids.shape[1] <= prompt_len:
            return None
        with torch.no_grad():
            with handler._load_model_context():
                lp, rank = handler.llm.score(input_ids, prompt_len)
        return lp.float().cpu(), rank.cpu()

    def _calculate_log_prob(llm_handler, formatted_prompt, target_text, temperature=1.0):
        if not isinstance(getattr(llm_handler, "llm", None), HipCausalLM):
            return orig_lp(llm_handler, formatted_prompt, target_text, temperature)
        try:
            out = _scored(llm_handler, formatted_prompt, target_text)
        except RuntimeError as e:
            if not fallback:
                raise
            log.warning("acehip LM scoring failed (%s); this call runs on PyTorch", e)
            return orig_lp(llm_handler, formatted_prompt, target_text, temperature)
        if out is None:
            return float("-inf")
        return out[0].mean().item()

    def _calculate_topk_recall(llm_handler, formatted_prompt, target_text, topk=10):
        if not isinstance(getattr(llm_handler, "llm", None), HipCausalLM):
            return orig_recall(llm_handler, formatted_prompt, target_text, topk)
        try:
            out = _scored(llm_handler, formatted_prompt, target_text)
        except RuntimeError as e:
            if not fallback:
                raise
            log.warning("acehip LM scoring failed (%s); this call runs on PyTorch", e)
            return orig_recall(llm_handler, formatted_prompt, target_text, topk)
        if out is None:
            return 0.0, {}
        return recall_from_ranks(out[1].tolist(), topk)

    lm_score_module._calculate_log_prob = _calculate_log_prob
    lm_score_module._calculate_topk_recall = _calculate_topk_recall
    return {"original": {"_calculate_log_prob": orig_lp, "_calculate_topk_recall": orig_recall},
            "log_prob": _calculate_log_prob, "topk_recall": _calculate_topk_recall}


def hip_normalize_audio(audio_data: torch.Tensor, target_db: float = -1.0) -> torch.Tensor:
    """``normalize_audio`` (acestep/audio_utils.py:24-62) for device tensors: same
    contract (returns a new tensor; silence returned unchanged) on the fused HIP
    pass.  A caller that normalizes while the audio is still on the GPU (before the
    payload's host copy) can bind it in place of the CPU pass at inference.py:679."""
    if not (isinstance(audio_data, torch.Tensor) and audio_data.is_cuda):
        raise TypeError("hip_normalize_audio: a GPU tensor is required (no CPU path)")
    x = audio_data.detach().float().contiguous().clone().reshape(1, -1)
    if x.shape[1] % 4:
        raise ValueError("hip_normalize_audio: sample count must be a multiple of 4")
    peak = torch.empty(1, device=x.device, dtype=torch.float32)
    from ._ffi import check, lib, ptr, stream_ptr
    target = float(torch.tensor(10 ** (target_db / 20.0), dtype=torch.float32))
    if target_db > 0.0:
        raise ValueError("hip_normalize_audio: target_db must be <= 0 (inference.py:674)")
    # guard off: normalize_audio alone scales a peak above 1 in one multiply
    check(lib().acehip_wav_postprocess(ptr(x), 1, x.shape[1], ptr(peak), 0, target, stream_ptr()), "wav_normalize")
    return x.reshape(audio_data.shape).to(audio_data.dtype)
