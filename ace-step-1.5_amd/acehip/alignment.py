"""Lyric alignment on the HIP path: drop-ins for the handler's ``get_lyric_timestamp``
(``acestep/core/generation/handler/lyric_timestamp.py:15-147``, the LRC button) and
``get_lyric_score`` (``handler/lyric_score.py:15-166``).

Both reference methods run ``self.model.decoder(..., output_attentions=True,
custom_layers_config=..., enable_early_exit=True)`` (lyric_timestamp.py:78-91,
lyric_score.py:93-110): the PyTorch decoder, all 24 layers, eager cross-attention with a
``[B, 16, S, Lenc]`` probability tensor per layer, of which the aligners read 8 heads and the
lyric-token slice of the key axis.  Here that one call becomes
:meth:`acehip.dit.AceStepDiTBackend.cross_attention_maps` (``acehip_dit_forward_capture``):
the handle's re-packed weights, a stop after the highest selected layer, and only the selected
heads' ``[tokens, frames]`` rows written.

What is restated is only what surrounds the decoder call; the handler's own helpers
(``_resolve_custom_layers_config``, ``_move_alignment_inputs_to_runtime``,
``_sample_noise_like``, ``_extract_lyric_segment``, the error payload builders) and the
reference aligners (``MusicStampsAligner``, ``MusicLyricScorer``: consensus, DTW, scoring) are
called, not copied.  The aligners index their input as ``[layer, head]`` through the config
they are given (dit_alignment.py:129-134, dit_score.py:85-87), so they get a compact
``[n_layers_sel, max_heads_per_layer, tokens, frames]`` tensor and a remapped config
``{i: [0..len_i)}`` in the same order; padding slots are never indexed.

``bsz != 1`` goes to the original method: the reference's own stacking is only well-formed
for one song (lyric_timestamp.py:104-105).
"""
from __future__ import annotations

import logging
from typing import Any, Dict, List, Optional, Tuple

import torch

log = logging.getLogger("acehip")


def compact_config(layers_config: Dict[int, List[int]], num_layers: Optional[int] = None,
                   num_heads: Optional[int] = None) -> Tuple[Dict[int, List[int]], Dict[int, List[int]]]:
    """Split ``{layer: [heads]}`` into (kept, remapped).

    ``kept`` has the entries the reference aligners would use, in dict order then list order:
    they skip a pair whose layer or head lies outside the attention tensor
    (dit_alignment.py:132, dit_score.py:87), so with ``num_layers`` / ``num_heads`` given such
    pairs are dropped (and a layer left without heads disappears).  ``remapped`` is
    ``{i: [0..len_i)}`` for the i-th kept layer: the config that indexes :func:`compact_maps`."""
    if not isinstance(layers_config, dict):
        raise TypeError(f"layers_config must be a dict {{layer: [heads]}}, got {type(layers_config).__name__}")
    kept: Dict[int, List[int]] = {}
    for layer, heads in layers_config.items():
        layer = int(layer)
        if layer < 0:
            raise ValueError(f"layers_config: negative layer index {layer}")
        if layer in kept:
            raise ValueError(f"layers_config: layer {layer} listed twice")
        hs = []
        for h in heads:
            h = int(h)
            if h < 0:
                raise ValueError(f"layers_config: negative head index {h} in layer {layer}")
            if (num_layers is None or layer < num_layers) and (num_heads is None or h < num_heads):
                hs.append(h)
        if hs:
            kept[layer] = hs
    remapped = {i: list(range(len(hs))) for i, hs in enumerate(kept.values())}
    return kept, remapped


def compact_maps(maps: torch.Tensor, kept: Dict[int, List[int]]) -> torch.Tensor:
    """maps ``[n, tokens, frames]`` (n over ``kept`` in dict order, then list order) →
    ``[n_layers_sel, max_heads_per_layer, tokens, frames]``; slots past a layer's own head
    count are zero and never indexed by the remapped config."""
    counts = [len(hs) for hs in kept.values()]
    if maps.dim() != 3 or maps.shape[0] != sum(counts) or not counts:
        raise ValueError(f"compact_maps: maps {tuple(maps.shape)} do not match the {sum(counts)} selected heads")
    out = maps.new_zeros(len(counts), max(counts), maps.shape[1], maps.shape[2])
    i = 0
    for li, c in enumerate(counts):
        out[li, :c] = maps[i:i + c]
        i += c
    return out


class LyricAlignment:
    """The two drop-ins, bound onto a handler by :func:`acehip.integration.install`.

    ``stamps_aligner`` / ``scorer``: callables ``tokenizer -> aligner`` (tests inject recording
    ones); None imports the reference classes lazily, as the reference methods do
    (lyric_timestamp.py:113, lyric_score.py:140)."""

    def __init__(self, handler, dit, fallback: bool = False, stamps_aligner=None, scorer=None):
        self.handler = handler
        self.dit = dit
        self.fallback = fallback
        self.stamps_aligner = stamps_aligner
        self.scorer = scorer
        self.orig_timestamp = getattr(handler, "get_lyric_timestamp", None)
        self.orig_score = getattr(handler, "get_lyric_score", None)

    def bind(self):
        """Rebind the methods the handler has (and only those)."""
        if self.orig_timestamp is not None:
            self.handler.get_lyric_timestamp = self.get_lyric_timestamp
        if self.orig_score is not None:
            self.handler.get_lyric_score = self.get_lyric_score
        return self

    # ------------------------------------------------------------ shared --
    def _limits(self):
        cfg = self.dit.rt.cfg
        return cfg.num_hidden_layers, cfg.num_attention_heads

    def _make_stamps_aligner(self):
        if self.stamps_aligner is not None:
            return self.stamps_aligner(self.handler.text_tokenizer)
        from acestep.core.scoring.dit_alignment import MusicStampsAligner
        return MusicStampsAligner(self.handler.text_tokenizer)

    def _make_scorer(self):
        if self.scorer is not None:
            return self.scorer(self.handler.text_tokenizer)
        from acestep.core.scoring.dit_score import MusicLyricScorer
        return MusicLyricScorer(self.handler.text_tokenizer)

    def _key_range(self, lyric_token_ids, vocal_language, Lenc):
        """The lyric-token slice of the key axis, clamped as the reference's slicing clamps it
        (lyric_timestamp.py:107-111)."""
        _, pure_ids, start, end = self.handler._extract_lyric_segment(lyric_token_ids=lyric_token_ids,
                                                                      vocal_language=vocal_language)
        return pure_ids, min(int(start), Lenc), min(int(end), Lenc)

    # --------------------------------------------------------- timestamps --
    @torch.inference_mode()
    def get_lyric_timestamp(self, pred_latent, encoder_hidden_states, encoder_attention_mask, context_latents,
                            lyric_token_ids, total_duration_seconds, vocal_language: str = "en",
                            inference_steps: int = 8, seed: int = 42,
                            custom_layers_config: Optional[Dict[int, List[int]]] = None) -> Dict[str, Any]:
        """``get_lyric_timestamp`` (lyric_timestamp.py:15-147) with the decoder call on acehip."""
        h = self.handler
        args = (pred_latent, encoder_hidden_states, encoder_attention_mask, context_latents, lyric_token_ids,
                total_duration_seconds)
        kw = dict(vocal_language=vocal_language, inference_steps=inference_steps, seed=seed,
                  custom_layers_config=custom_layers_config)
        if h.model is None:
            return h._lyric_timestamp_error("Model not initialized")
        if pred_latent.shape[0] != 1:
            return self.orig_timestamp(*args, **kw)
        try:
            return self._timestamp(*args, **kw)
        except Exception as exc:
            if self.fallback and self.orig_timestamp is not None:
                log.warning("acehip get_lyric_timestamp failed (%s); falling back to PyTorch", exc)
                return self.orig_timestamp(*args, **kw)
            if isinstance(exc, (ValueError, KeyError, RuntimeError, OSError)):      # lyric_timestamp.py:142-144
                log.exception("[get_lyric_timestamp] Failed")
                return h._lyric_timestamp_error(f"Error generating timestamps: {exc}")
            raise

    def _timestamp(self, pred_latent, encoder_hidden_states, encoder_attention_mask, context_latents,
                   lyric_token_ids, total_duration_seconds, vocal_language, inference_steps, seed,
                   custom_layers_config):
        h = self.handler
        config = h._resolve_custom_layers_config(custom_layers_config)
        pred_latent, enc, _mask, ctx = h._move_alignment_inputs_to_runtime(
            pred_latent=pred_latent, encoder_hidden_states=encoder_hidden_states,
            encoder_attention_mask=encoder_attention_mask, context_latents=context_latents)
        if not isinstance(inference_steps, int) or inference_steps <= 0:
            return h._lyric_timestamp_error(
                f"inference_steps must be a positive non-zero integer, got {inference_steps!r}")
        # lyric_timestamp.py:71-74: xt = t_last·noise + (1 − t_last)·pred_latent, t = t_r = t_last
        t_last = 1.0 / inference_steps
        noise = h._sample_noise_like(pred_latent, seed)
        xt = t_last * noise + (1.0 - t_last) * pred_latent
        kept, remapped = compact_config(config, *self._limits())
        if not kept:
            return h._lyric_timestamp_error("No valid attention heads found")      # dit_alignment.py:179-185
        pure_ids, k0, k1 = self._key_range(lyric_token_ids, vocal_language, enc.shape[1])
        if k0 >= k1:
            return h._lyric_timestamp_error("Lyrics indices out of bounds")
        # the encoder mask is not an input: the decoder never masks encoder positions (base:1384-1385)
        maps = self.dit.cross_attention_maps(xt, torch.tensor([t_last]), enc, ctx, kept, k0, k1, stop_early=True)
        matrix = compact_maps(maps[:, 0], kept)
        aligner = self._make_stamps_aligner()
        info = aligner.stamps_align_info(attention_matrix=matrix, lyrics_tokens=pure_ids,
                                         total_duration_seconds=total_duration_seconds, custom_config=remapped,
                                         return_matrices=False, violence_level=2.0, medfilt_width=1)
        if info.get("calc_matrix") is None:
            return h._lyric_timestamp_error(info.get("error", "Failed to process attention matrix"))
        res = aligner.get_timestamps_and_lrc(calc_matrix=info["calc_matrix"], lyrics_tokens=pure_ids,
                                             total_duration_seconds=total_duration_seconds)
        return {"lrc_text": res["lrc_text"], "sentence_timestamps": res["sentence_timestamps"],
                "token_timestamps": res["token_timestamps"], "success": True, "error": None}

    # -------------------------------------------------------------- score --
    @torch.inference_mode()
    def get_lyric_score(self, pred_latent, encoder_hidden_states, encoder_attention_mask, context_latents,
                        lyric_token_ids, vocal_language: str = "en", inference_steps: int = 8, seed: int = 42,
                        custom_layers_config: Optional[Dict[int, List[int]]] = None) -> Dict[str, Any]:
        """``get_lyric_score`` (lyric_score.py:15-166) with the decoder call on acehip."""
        h = self.handler
        args = (pred_latent, encoder_hidden_states, encoder_attention_mask, context_latents, lyric_token_ids)
        kw = dict(vocal_language=vocal_language, inference_steps=inference_steps, seed=seed,
                  custom_layers_config=custom_layers_config)
        if h.model is None:
            return h._lyric_score_error("Model not initialized")
        if pred_latent.shape[0] != 1:
            return self.orig_score(*args, **kw)
        try:
            return self._score(*args, **kw)
        except Exception as exc:
            if self.fallback and self.orig_score is not None:
                log.warning("acehip get_lyric_score failed (%s); falling back to PyTorch", exc)
                return self.orig_score(*args, **kw)
            if isinstance(exc, (ValueError, KeyError, RuntimeError, OSError)):      # lyric_score.py:161-163
                log.exception("[get_lyric_score] Failed")
                return h._lyric_score_error(f"Error generating score: {exc}")
            raise

    def _score(self, pred_latent, encoder_hidden_states, encoder_attention_mask, context_latents, lyric_token_ids,
               vocal_language, inference_steps, seed, custom_layers_config):
        h = self.handler
        config = h._resolve_custom_layers_config(custom_layers_config)
        pred_latent, enc, _mask, ctx = h._move_alignment_inputs_to_runtime(
            pred_latent=pred_latent, encoder_hidden_states=encoder_hidden_states,
            encoder_attention_mask=encoder_attention_mask, context_latents=context_latents)
        bsz = pred_latent.shape[0]
        if not isinstance(inference_steps, int) or inference_steps <= 0:
            raise ValueError(f"inference_steps must be a positive non-zero integer, got {inference_steps!r}")
        # lyric_score.py:70-91: the 2-row batch [noise; xt] at t = [1.0, t_last], condition and
        # context duplicated
        x0 = h._sample_noise_like(pred_latent, seed)
        t_last = 1.0 / inference_steps
        xt_dit = t_last * x0 + (1.0 - t_last) * pred_latent
        xt_in = torch.cat([x0, xt_dit], dim=0)
        t_in = torch.tensor([1.0] * bsz + [t_last] * bsz)
        enc_in = torch.cat([enc, enc], dim=0)
        ctx_in = torch.cat([ctx, ctx], dim=0)
        kept, remapped = compact_config(config, *self._limits())
        pure_ids, k0, k1 = self._key_range(lyric_token_ids, vocal_language, enc.shape[1])
        if k0 >= k1:
            return h._lyric_score_error("Lyrics indices out of bounds")            # lyric_score.py:134-135
        if not kept:                    # no usable head: both evaluations score 0.0 (lyric_score.py:183-184)
            return {"lm_score": 0.0, "dit_score": 0.0, "success": True, "error": None}
        maps = self.dit.cross_attention_maps(xt_in, t_in, enc_in, ctx_in, kept, k0, k1, stop_early=True)
        scorer = self._make_scorer()
        lm = self._single_score(scorer, compact_maps(maps[:, 0], kept), pure_ids, remapped)
        dit = self._single_score(scorer, compact_maps(maps[:, 1], kept), pure_ids, remapped)
        return {"lm_score": lm, "dit_score": dit, "success": True, "error": None}

    @staticmethod
    def _single_score(scorer, matrix, pure_ids, config) -> float:
        """``_calculate_single_lyric_score`` (lyric_score.py:168-190)."""
        info = scorer.lyrics_alignment_info(attention_matrix=matrix, token_ids=pure_ids, custom_config=config,
                                            return_matrices=False, medfilt_width=1)
        if info.get("energy_matrix") is None:
            return 0.0
        res = scorer.calculate_score(energy_matrix=info["energy_matrix"], type_mask=info["type_mask"],
                                     path_coords=info["path_coords"])
        return float(res.get("lyrics_score", res.get("final_score", 0.0)))
