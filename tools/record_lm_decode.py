#!/usr/bin/env python3
"""Golden vectors for the 5 Hz LM's token loop (prefill + one-token decode over a K/V cache).

The reference's ``LLMHandler.llm`` on the ``pt`` backend is a transformers
``Qwen3ForCausalLM`` that its two custom loops drive only through ``_forward_pass``
(``acestep/llm_inference.py:416-438``): one call with the left-padded prompt and its
attention mask, then one call per token with ``input_ids[:, -1:]``, the returned
``past_key_values`` and the mask grown by a column of ones.  This tool runs exactly that
call sequence on the CPU with the seeded synthetic weights of
``acehip.weights.synth_text_encoder_weights`` (parity mode, tied embeddings; the tests
regenerate them), teacher-forced with a fixed random token sequence, once in fp32 and once
with the model cast ``.to(torch.bfloat16)``, and stores the last-position logits of every call.

Per tag it writes tests/golden/lm_decode_{tag}.safetensors and an entry of
tests/golden/lm_decode_manifest.json:
  ref_bf16_rel_l2 / ref_bf16_max_abs   the reference's own bf16 run against its fp32 run;
  clear_share      share of (call, row) pairs whose fp32 top-1 margin exceeds 4 x ref_bf16_max_abs;
  ref_bf16_top1_agrees   whether the bf16 run has the same top-1 on all of those.
A fixture whose share is under 0.5, or on which the bf16 run disagrees, is refused: pick
another seed.

Embedding gain.  The synthetic weights are N(0, 0.02²) everywhere, so with tied embeddings the
logits of the two LM widths are Gaussian over 2048 entries and the fp32 top-1 gap exceeds
4 x the reference's bf16 error on only about a quarter of the pairs at any seed (24 seeds
tried: shares 0.08-0.36).  A trained LM's embedding is far larger than 0.02 against its
layer weights; ``embed_gain`` multiplies ``embed_tokens.weight`` (and so the tied lm_head) of
the synthetic state dict by a constant, which gives the logits real margins while the layers
still decide them (the top-1 is the token just fed on 75 % of w06's calls and 92 % of w17's).
tiny 1 (share 0.79), w06 4 (0.64; 0.24 without), w17 6 (0.90; 0.26 without, 0.46 at 4).
The gain is in the manifest; the tests apply it to the regenerated weights.

usage: python tools/record_lm_decode.py [tag ...]
"""
import json
import os
import sys

import torch
from safetensors.torch import save_file
from transformers import Qwen3Config, Qwen3ForCausalLM

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "ace-step-1.5_amd")]
from acehip.config import DiTConfig  # noqa: E402
from acehip.weights import synth_text_encoder_weights  # noqa: E402

GOLDEN = os.path.join(REPO, "tests", "golden")
B, S, PAD = 2, 70, 9          # prompt [B, S]; row 1 left-padded by PAD
MARGIN = 4.0

_COMMON = dict(head_dim=128, rms_norm_eps=1e-6, rope_theta=1_000_000.0, max_position_embeddings=4096,
               attention_bias=False, use_sliding_window=False, tie_word_embeddings=True)
# tag -> (Qwen3Config fields, weight seed, teacher-forced steps, store the prompt's bf16 hidden state, embed gain)
TAGS = {
    "tiny": (dict(vocab_size=512, hidden_size=256, intermediate_size=512, num_hidden_layers=3,
                  num_attention_heads=2, num_key_value_heads=1), 7, 70, True, 1.0),
    "w06": (dict(vocab_size=2048, hidden_size=1024, intermediate_size=3072, num_hidden_layers=3,
                 num_attention_heads=16, num_key_value_heads=8), 11, 24, True, 4.0),
    # no hidden state here: with it the file would pass the 1 MiB limit of a committed file
    "w17": (dict(vocab_size=2048, hidden_size=2048, intermediate_size=6144, num_hidden_layers=2,
                 num_attention_heads=16, num_key_value_heads=8), 13, 24, False, 6.0),
}


def hf_config(tag: str) -> dict:
    return dict(TAGS[tag][0], **_COMMON)


def dit_cfg(tag: str) -> DiTConfig:
    c = hf_config(tag)
    return DiTConfig(hidden_size=c["hidden_size"], intermediate_size=c["intermediate_size"],
                     num_hidden_layers=c["num_hidden_layers"], num_attention_heads=c["num_attention_heads"],
                     num_key_value_heads=c["num_key_value_heads"], head_dim=c["head_dim"],
                     rms_norm_eps=c["rms_norm_eps"], rope_theta=c["rope_theta"])


def weights(tag: str):
    """The fixture's Qwen3Model state dict (``embed_tokens.weight`` doubles as the tied lm_head)."""
    W = synth_text_encoder_weights(dit_cfg(tag), hf_config(tag)["vocab_size"], seed=TAGS[tag][1], mode="parity")
    W["embed_tokens.weight"] = W["embed_tokens.weight"] * TAGS[tag][4]
    return W


def build_model(tag: str) -> Qwen3ForCausalLM:
    model = Qwen3ForCausalLM(Qwen3Config(**hf_config(tag))).eval()
    missing, unexpected = model.model.load_state_dict(weights(tag), strict=False)
    assert not unexpected and all(k.startswith("rotary_emb") for k in missing), (missing, unexpected)
    model.tie_weights()
    assert model.lm_head.weight.data_ptr() == model.model.embed_tokens.weight.data_ptr()
    return model


def run_loop(model, ids, mask, forced):
    """The call sequence of _forward_pass: logits[:, -1, :] of every call, [N + 1, B, V]."""
    out, past = [], None
    generated, attn = ids.clone(), mask.clone()
    with torch.inference_mode():
        for step in range(forced.shape[1] + 1):
            if past is None:
                o = model(input_ids=generated, attention_mask=attn, use_cache=True)
            else:
                o = model(input_ids=generated[:, -1:], past_key_values=past, attention_mask=attn, use_cache=True)
            out.append(o.logits[:, -1, :].clone())
            past = o.past_key_values
            if step < forced.shape[1]:
                generated = torch.cat([generated, forced[:, step:step + 1]], dim=1)
                attn = torch.cat([attn, torch.ones((B, 1), dtype=attn.dtype)], dim=1)
    return torch.stack(out)


def record(tag: str) -> dict:
    cfg, seed, n_steps, with_hidden, gain = TAGS[tag]
    g = torch.Generator().manual_seed(1000 + seed)
    V = cfg["vocab_size"]
    ids = torch.randint(0, V, (B, S), generator=g)
    mask = torch.ones(B, S, dtype=torch.long)
    mask[1, :PAD] = 0
    forced = torch.randint(0, V, (1, n_steps), generator=g).repeat(B, 1)   # CFG: both rows take the same token
    model = build_model(tag)
    lf = run_loop(model, ids, mask, forced).float()
    mb = model.to(torch.bfloat16)
    lb = run_loop(mb, ids, mask, forced)
    out = {"ids": ids, "mask": mask, "forced": forced, "logits_f32": lf.contiguous(), "logits_bf16": lb.contiguous()}
    if with_hidden:
        with torch.inference_mode():
            out["hidden_last"] = mb.model(input_ids=ids, attention_mask=mask).last_hidden_state.contiguous()
    d = lb.float() - lf
    max_abs = float(d.abs().max())
    top2 = lf.topk(2, dim=-1).values
    clear = (top2[..., 0] - top2[..., 1]) > MARGIN * max_abs                    # [N + 1, B]
    agrees = bool((lb.float().argmax(-1) == lf.argmax(-1))[clear].all())
    entry = {"seed": seed, "embed_gain": gain, "steps": n_steps, "B": B, "S": S, "pad": PAD,
             "ref_bf16_rel_l2": float(d.norm() / lf.norm()),
             "ref_bf16_rel_l2_last_quarter": float(d[-((n_steps + 1) // 4):].norm() / lf[-((n_steps + 1) // 4):].norm()),
             "ref_bf16_max_abs": max_abs, "margin_factor": MARGIN,
             "clear_share": float(clear.float().mean()), "ref_bf16_top1_agrees": agrees,
             "clear": clear.int().tolist()}
    if entry["clear_share"] < 0.5 or not agrees:
        print(tag, {k: v for k, v in entry.items() if k != "clear"})
        raise ValueError(f"{tag}: clear-margin share {entry['clear_share']:.2f}, bf16 top-1 agrees: {agrees} — "
                         "refusing to write this fixture; pick another seed")
    path = os.path.join(GOLDEN, f"lm_decode_{tag}.safetensors")
    save_file(out, path, metadata={k: str(v) for k, v in hf_config(tag).items()})
    assert os.path.getsize(path) < (1 << 20), f"{path} is {os.path.getsize(path)} bytes"
    print(tag, {k: v for k, v in entry.items() if k != "clear"}, os.path.getsize(path), "bytes")
    return entry


def main():
    tags = sys.argv[1:] or list(TAGS)
    mpath = os.path.join(GOLDEN, "lm_decode_manifest.json")
    manifest = json.load(open(mpath)) if os.path.exists(mpath) else {}
    refused = []
    for tag in tags:
        try:
            manifest[tag] = record(tag)
        except ValueError as e:
            print(e)
            refused.append(tag)
    with open(mpath, "w") as f:
        json.dump(manifest, f, indent=1, sort_keys=True)
        f.write("\n")
    if refused:
        raise SystemExit(f"refused: {refused}")


if __name__ == "__main__":
    main()
