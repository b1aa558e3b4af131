#!/usr/bin/env python3
"""Golden vectors for the 5 Hz LM's scoring path (this container only; the reference never
travels and this tool is not run on the GPU machine).

The reference scores a finished song with ``acestep/core/scoring/lm_score.py``: a teacher-forced
forward over prompt + target, then per target token its log-probability
(``_calculate_log_prob``, ``:263-289``) or its membership in the top k (``_calculate_topk_recall``,
``:181-232``).  This tool loads that module from the reference tree with a ``loguru`` stub and
runs it, on the CPU, on the stub handler / tokenizer of ``tests/lm_score_ref.py`` and the seeded
synthetic models of ``tools/record_lm_decode.py`` (same weights, same ``embed_gain``; the tests
regenerate them).

Sequence: a random prompt of 70 tokens, then 48 targets chosen autoregressively on the fp32 model
as its j-th ranked next token, j cycling through RANKS — ranks on both sides of the top-10 band,
and targets with margins (a random target sits in the dense middle of the logits).

Per tag it writes tests/golden/lm_score_{tag}.safetensors (ids and per-position vectors only) and
an entry of tests/golden/lm_score_manifest.json:
  lp_f32 / rank_f32, lp_bf16 / rank_bf16   per position, fp64 log-softmax of the fp32 run's and of
                    the bf16 run's (model cast .to(bfloat16)) logits, and the target's 1-based
                    rank (equal values: lower index first);
  ref_log_prob, ref_topk_recall   what the reference's two functions return on the fp32 model;
  ref_bf16_lp_rms   RMS over positions of lp_bf16 - lp_f32;
  ref_bf16_max_abs  largest logit difference of the two runs over the scored rows;
  clear             positions where no other token's fp32 logit lies within
                    MARGIN x ref_bf16_max_abs of the target's; clear_share; ref_bf16_ranks_agree.
A fixture is refused — pick another ids seed — when the clear share is under 0.5, when the bf16
run's rank differs from the fp32 rank on a clear position, or when the fp32 run ties with the
target at a rank <= 11 (torch.topk's order among equal values is unspecified, so the reference's
recall would not be well defined).

usage: python tools/record_lm_score.py [tag ...]
"""
import importlib.util
import json
import os
import sys
import types

import torch
from safetensors.torch import save_file

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "ace-step-1.5_amd"), os.path.join(REPO, "tests"),
                os.path.join(REPO, "tools")]
import record_lm_decode as D  # noqa: E402
from lm_score_ref import StubHandler, StubTokenizer, ids_to_text, ranks_of  # noqa: E402

GOLDEN = os.path.join(REPO, "tests", "golden")
REF_ROOT = "/root/reference"
PROMPT, TARGETS = 70, 48
RANKS = [1, 1, 2, 1, 3, 1, 2, 11, 1, 5]
MARGIN = 4.0
TOPK = 10
IDS_SEED = {"tiny": 77, "w06": 77, "w17": 77}


def _load_reference():
    if "loguru" not in sys.modules:
        m = types.ModuleType("loguru")

        class _L:
            def __getattr__(self, name):
                return lambda *a, **k: None
        m.logger = _L()
        sys.modules["loguru"] = m
    spec = importlib.util.spec_from_file_location(
        "_ref_lm_score", os.path.join(REF_ROOT, "acestep", "core", "scoring", "lm_score.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _sequence(model, V, seed):
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(0, V, (1, PROMPT), generator=g)
    with torch.inference_mode():
        for i in range(TARGETS):
            logits = model(input_ids=ids).logits[0, -1]
            nxt = logits.topk(max(RANKS)).indices[RANKS[i % len(RANKS)] - 1]
            ids = torch.cat([ids, nxt.reshape(1, 1)], dim=1)
    return ids


def _rows(model, ids):
    with torch.inference_mode():
        return model(input_ids=ids).logits[0, PROMPT - 1:-1].clone()


def record(tag: str, ref) -> dict:
    seed = IDS_SEED[tag]
    V = D.hf_config(tag)["vocab_size"]
    model = D.build_model(tag)
    ids = _sequence(model, V, seed)
    targets = ids[0, PROMPT:]
    lf = _rows(model, ids).float()
    handler = StubHandler(model, StubTokenizer())
    prompt, target = ids_to_text(ids[0, :PROMPT]), " " + ids_to_text(targets)
    ref_lp = float(ref._calculate_log_prob(handler, prompt, target))
    ref_avg, ref_k = ref._calculate_topk_recall(handler, prompt, target, topk=TOPK)
    lb = _rows(model.to(torch.bfloat16), ids).float()

    def lp(logits):
        return torch.log_softmax(logits.double(), dim=-1).gather(1, targets[:, None])[:, 0]
    lp_f, lp_b = lp(lf), lp(lb)
    rank_f, rank_b = ranks_of(lf, targets), ranks_of(lb, targets)
    max_abs = float((lb - lf).abs().max())
    tl = lf.gather(1, targets[:, None])
    other = torch.arange(V)[None, :] != targets[:, None]
    clear = ~(((lf - tl).abs() <= MARGIN * max_abs) & other).any(1)
    agrees = bool((rank_b == rank_f)[clear].all())
    tie = bool((((lf == tl) & other).any(1) & (rank_f <= TOPK + 1)).any())
    entry = {"seed": D.TAGS[tag][1], "embed_gain": D.TAGS[tag][4], "ids_seed": seed, "prompt_len": PROMPT,
             "targets": TARGETS, "rank_cycle": RANKS, "topk": TOPK, "margin_factor": MARGIN,
             "ref_bf16_lp_rms": float((lp_b - lp_f).pow(2).mean().sqrt()), "ref_bf16_max_abs": max_abs,
             "clear_share": float(clear.float().mean()), "ref_bf16_ranks_agree": agrees, "fp32_tie_in_top11": tie,
             "ref_log_prob": ref_lp, "ref_topk_recall": {"average": float(ref_avg),
                                                         "per_k": {str(k): float(v) for k, v in ref_k.items()}},
             "lp_f32_mean": float(lp_f.mean()), "rank_f32": rank_f.tolist()}
    if entry["clear_share"] < 0.5 or not agrees or tie:
        print(tag, entry)
        raise ValueError(f"{tag}: clear share {entry['clear_share']:.2f}, bf16 ranks agree: {agrees}, fp32 tie in "
                         f"the top 11: {tie} — refusing to write this fixture; pick another seed")
    out = {"ids": ids, "prompt_len": torch.tensor(PROMPT), "lp_f32": lp_f, "lp_bf16": lp_b, "rank_f32": rank_f,
           "rank_bf16": rank_b, "clear": clear.to(torch.uint8), "ref_log_prob": torch.tensor(ref_lp, dtype=torch.float64),
           "ref_recall_average": torch.tensor(float(ref_avg), dtype=torch.float64),
           "ref_recall_per_k": torch.tensor([ref_k[k] for k in range(1, TOPK + 1)], dtype=torch.float64)}
    path = os.path.join(GOLDEN, f"lm_score_{tag}.safetensors")
    meta = dict(D.hf_config(tag))
    save_file({k: v.contiguous() for k, v in out.items()}, path, metadata={k: str(v) for k, v in meta.items()})
    assert os.path.getsize(path) < (1 << 20), f"{path} is {os.path.getsize(path)} bytes"
    print(tag, {k: v for k, v in entry.items() if k != "rank_f32"}, os.path.getsize(path), "bytes")
    return entry


def main():
    tags = sys.argv[1:] or list(D.TAGS)
    ref = _load_reference()
    mpath = os.path.join(GOLDEN, "lm_score_manifest.json")
    manifest = json.load(open(mpath)) if os.path.exists(mpath) else {}
    refused = []
    for tag in tags:
        try:
            manifest[tag] = record(tag, ref)
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
