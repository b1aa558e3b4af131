#!/usr/bin/env python3
"""Golden vectors for the 5 Hz LM at heads / kv_heads = 4 (the 4B LM: 32 / 8 heads, hidden 2560,
intermediate 9728): the token loop and the scoring path.

The method is tools/record_lm_decode.py's — transformers' ``Qwen3ForCausalLM`` on the CPU on the
seeded synthetic weights of ``acehip.weights.synth_text_encoder_weights``, the ``_forward_pass``
call sequence at B = 2, S = 70 with row 1 left-padded by 9, teacher-forced, one fp32 and one bf16
run, the same refusal rule (clear-margin share >= 0.5 and the bf16 run agreeing on every clear
pair) — and, for the scoring vectors of ``w4b``, tools/record_lm_score.py's (its sequence, its
per-position vectors, its refusal rule, the reference's own two scoring functions).  Those tools'
tag tables drive existing tests, so this one keeps its own:

  g4tiny   hidden 256, intermediate 512, 3 layers, 4 / 1 heads, vocabulary 512, 70 steps;
  w4b      hidden 2560, intermediate 9728, 2 layers, 32 / 8 heads, vocabulary 2048, 24 steps, no
           stored hidden state: the 4B's real widths (divisibility is where the kernels can go
           wrong) with layers and vocabulary shrunk.

Seed and ``embed_gain`` per tag are the first of the values tried that pass the refusal rule on
the CPU (see record_lm_decode.py on why a gain is needed at the LM widths): g4tiny seed 7, gain 1
(share 0.53); w4b seed 17, gain 8 (share 0.76; gain 6, w17's, gave 0.48 and was refused).  Both are
in the manifest, and the tests apply them to the regenerated weights.

Writes tests/golden/lm_gqa4_{tag}.safetensors, tests/golden/lm_gqa4_manifest.json,
tests/golden/lm_gqa4_score_{tag}.safetensors and tests/golden/lm_gqa4_score_manifest.json.

usage: python tools/record_lm_gqa4.py [tag ...]
"""
import json
import os
import sys

import torch
from safetensors.torch import save_file
from transformers import Qwen3Config, Qwen3ForCausalLM

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "ace-step-1.5_amd"), os.path.join(REPO, "tests"),
                os.path.join(REPO, "tools")]
import record_lm_decode as D  # noqa: E402
from acehip.config import DiTConfig  # noqa: E402
from acehip.weights import synth_text_encoder_weights  # noqa: E402

GOLDEN = D.GOLDEN
B, S, PAD, MARGIN = D.B, D.S, D.PAD, D.MARGIN

# tag -> (Qwen3Config fields, weight seed, teacher-forced steps, store the prompt's bf16 hidden state, embed gain)
TAGS = {
    "g4tiny": (dict(vocab_size=512, hidden_size=256, intermediate_size=512, num_hidden_layers=3,
                    num_attention_heads=4, num_key_value_heads=1), 7, 70, True, 1.0),
    "w4b": (dict(vocab_size=2048, hidden_size=2560, intermediate_size=9728, num_hidden_layers=2,
                 num_attention_heads=32, num_key_value_heads=8), 17, 24, False, 8.0),
}
SCORE_TAGS = ("w4b",)
SCORE_IDS_SEED = {"w4b": 77}


def hf_config(tag: str) -> dict:
    return dict(TAGS[tag][0], **D._COMMON)


def dit_cfg(tag: str) -> DiTConfig:
    c = hf_config(tag)
    return DiTConfig(hidden_size=c["hidden_size"], intermediate_size=c["intermediate_size"],
                     num_hidden_layers=c["num_hidden_layers"], num_attention_heads=c["num_attention_heads"],
                     num_key_value_heads=c["num_key_value_heads"], head_dim=c["head_dim"],
                     rms_norm_eps=c["rms_norm_eps"], rope_theta=c["rope_theta"])


def weights(tag: str):
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


def record(tag: str) -> dict:
    """record_lm_decode.record on this tool's tags."""
    cfg, seed, n_steps, with_hidden, gain = TAGS[tag]
    g = torch.Generator().manual_seed(1000 + seed)
    V = cfg["vocab_size"]
    ids = torch.randint(0, V, (B, S), generator=g)
    mask = torch.ones(B, S, dtype=torch.long)
    mask[1, :PAD] = 0
    forced = torch.randint(0, V, (1, n_steps), generator=g).repeat(B, 1)
    model = build_model(tag)
    lf = D.run_loop(model, ids, mask, forced).float()
    mb = model.to(torch.bfloat16)
    lb = D.run_loop(mb, ids, mask, forced)
    out = {"ids": ids, "mask": mask, "forced": forced, "logits_f32": lf.contiguous(), "logits_bf16": lb.contiguous()}
    if with_hidden:
        with torch.inference_mode():
            out["hidden_last"] = mb.model(input_ids=ids, attention_mask=mask).last_hidden_state.contiguous()
    d = lb.float() - lf
    max_abs = float(d.abs().max())
    top2 = lf.topk(2, dim=-1).values
    clear = (top2[..., 0] - top2[..., 1]) > MARGIN * max_abs
    agrees = bool((lb.float().argmax(-1) == lf.argmax(-1))[clear].all())
    q = (n_steps + 1) // 4
    entry = {"seed": seed, "embed_gain": gain, "steps": n_steps, "B": B, "S": S, "pad": PAD,
             "ref_bf16_rel_l2": float(d.norm() / lf.norm()),
             "ref_bf16_rel_l2_last_quarter": float(d[-q:].norm() / lf[-q:].norm()),
             "ref_bf16_max_abs": max_abs, "margin_factor": MARGIN,
             "clear_share": float(clear.float().mean()), "ref_bf16_top1_agrees": agrees,
             "clear": clear.int().tolist()}
    if entry["clear_share"] < 0.5 or not agrees:
        print(tag, {k: v for k, v in entry.items() if k != "clear"})
        raise ValueError(f"{tag}: clear-margin share {entry['clear_share']:.2f}, bf16 top-1 agrees: {agrees} — "
                         "refusing to write this fixture; pick another seed")
    path = os.path.join(GOLDEN, f"lm_gqa4_{tag}.safetensors")
    save_file(out, path, metadata={k: str(v) for k, v in hf_config(tag).items()})
    assert os.path.getsize(path) < (1 << 20), f"{path} is {os.path.getsize(path)} bytes"
    print(tag, {k: v for k, v in entry.items() if k != "clear"}, os.path.getsize(path), "bytes")
    return entry


def record_score(tag: str, ref) -> dict:
    """record_lm_score.record on this tool's tags (that tool reads record_lm_decode's table and
    writes lm_score_*, so its computation is restated on its own helpers)."""
    import record_lm_score as RS
    from lm_score_ref import StubHandler, StubTokenizer, ids_to_text, ranks_of
    seed = SCORE_IDS_SEED[tag]
    V = hf_config(tag)["vocab_size"]
    model = build_model(tag)
    ids = RS._sequence(model, V, seed)
    P = RS.PROMPT
    targets = ids[0, P:]
    lf = RS._rows(model, ids).float()
    handler = StubHandler(model, StubTokenizer())
    prompt, target = ids_to_text(ids[0, :P]), " " + ids_to_text(targets)
    ref_lp = float(ref._calculate_log_prob(handler, prompt, target))
    ref_avg, ref_k = ref._calculate_topk_recall(handler, prompt, target, topk=RS.TOPK)
    lb = RS._rows(model.to(torch.bfloat16), ids).float()

    def lp(logits):
        return torch.log_softmax(logits.double(), dim=-1).gather(1, targets[:, None])[:, 0]
    lp_f, lp_b = lp(lf), lp(lb)
    rank_f, rank_b = ranks_of(lf, targets), ranks_of(lb, targets)
    max_abs = float((lb - lf).abs().max())
    tl = lf.gather(1, targets[:, None])
    other = torch.arange(V)[None, :] != targets[:, None]
    clear = ~(((lf - tl).abs() <= RS.MARGIN * max_abs) & other).any(1)
    agrees = bool((rank_b == rank_f)[clear].all())
    tie = bool((((lf == tl) & other).any(1) & (rank_f <= RS.TOPK + 1)).any())
    entry = {"seed": TAGS[tag][1], "embed_gain": TAGS[tag][4], "ids_seed": seed, "prompt_len": P,
             "targets": RS.TARGETS, "rank_cycle": RS.RANKS, "topk": RS.TOPK, "margin_factor": RS.MARGIN,
             "ref_bf16_lp_rms": float((lp_b - lp_f).pow(2).mean().sqrt()), "ref_bf16_max_abs": max_abs,
             "clear_share": float(clear.float().mean()), "ref_bf16_ranks_agree": agrees, "fp32_tie_in_top11": tie,
             "ref_log_prob": ref_lp, "ref_topk_recall": {"average": float(ref_avg),
                                                         "per_k": {str(k): float(v) for k, v in ref_k.items()}},
             "lp_f32_mean": float(lp_f.mean()), "rank_f32": rank_f.tolist()}
    if entry["clear_share"] < 0.5 or not agrees or tie:
        print(tag, entry)
        raise ValueError(f"{tag}: clear share {entry['clear_share']:.2f}, bf16 ranks agree: {agrees}, fp32 tie in "
                         f"the top 11: {tie} — refusing to write this fixture; pick another seed")
    out = {"ids": ids, "prompt_len": torch.tensor(P), "lp_f32": lp_f, "lp_bf16": lp_b, "rank_f32": rank_f,
           "rank_bf16": rank_b, "clear": clear.to(torch.uint8), "ref_log_prob": torch.tensor(ref_lp, dtype=torch.float64),
           "ref_recall_average": torch.tensor(float(ref_avg), dtype=torch.float64),
           "ref_recall_per_k": torch.tensor([ref_k[k] for k in range(1, RS.TOPK + 1)], dtype=torch.float64)}
    path = os.path.join(GOLDEN, f"lm_gqa4_score_{tag}.safetensors")
    save_file({k: v.contiguous() for k, v in out.items()}, path,
              metadata={k: str(v) for k, v in hf_config(tag).items()})
    assert os.path.getsize(path) < (1 << 20), f"{path} is {os.path.getsize(path)} bytes"
    print("score", tag, {k: v for k, v in entry.items() if k != "rank_f32"}, os.path.getsize(path), "bytes")
    return entry


def _update(path, fn, tags):
    manifest = json.load(open(path)) if os.path.exists(path) else {}
    refused = []
    for tag in tags:
        try:
            manifest[tag] = fn(tag)
        except ValueError as e:
            print(e)
            refused.append(tag)
    with open(path, "w") as f:
        json.dump(manifest, f, indent=1, sort_keys=True)
        f.write("\n")
    return refused


def main():
    tags = sys.argv[1:] or list(TAGS)
    refused = _update(os.path.join(GOLDEN, "lm_gqa4_manifest.json"), record, tags)
    score_tags = [t for t in tags if t in SCORE_TAGS and t not in refused]
    if score_tags:
        import record_lm_score as RS
        ref = RS._load_reference()
        refused += _update(os.path.join(GOLDEN, "lm_gqa4_score_manifest.json"), lambda t: record_score(t, ref),
                           score_tags)
    if refused:
        raise SystemExit(f"refused: {refused}")


if __name__ == "__main__":
    main()
