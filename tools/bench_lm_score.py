#!/usr/bin/env python3
"""One ``_calculate_log_prob``-equivalent scoring call of the 5 Hz LM (core/scoring/lm_score.py)
on the HIP path against the same call on transformers' bf16 ``Qwen3ForCausalLM``, in one process:
the 0.6B and 1.7B shapes (28 layers, vocabulary 217 204, synthetic weights), a sequence of
S = 1500 tokens (a 240 s song's codes plus caption / lyrics) of which the last T = 64 / 512 are
the scored target.

Per shape and T, medians of interleaved rounds from device events (a 300 MB buffer is written
between rounds, so a round starts with nothing of the model in the caches):
  call_ms          HipCausalLM.score (embedding, acehip_enc_forward over S, acehip_lm_score_bf16
                   over T rows) + the fp32 mean + its copy to the host: what install_lm_score's
                   _calculate_log_prob does after tokenising
  hf_fwd_copy_ms   the reference's path up to where its logits are on the host: model(input_ids,
                   attention_mask) -> [1, S, V] bf16 logits, the T target rows copied to the host
                   (lm_score.py:165-171)
  hf_call_ms       the same plus log_softmax, gather and mean on the host (:281-287), as the
                   reference does them (bf16 CPU tensors)
  ratio            hf_fwd_copy_ms / call_ms — the comparison that favours the reference
and the kernel alone (acehip_lm_score_bf16 on T rows, both passes and both finish steps) against
its two floors: bytes of W per pass over HBM bandwidth (8 TB/s) and 2·T·V·K per pass over the
bf16 MFMA peak (2.5 PF), each times two passes.  W (445 / 890 MB) is larger than the 256 MB
last-level cache, so a pass streams it from HBM.
Writes profiles/lm_score_bench.json.  Condition: call_ms <= hf_fwd_copy_ms at every shape and T.

usage: bench_lm_score.py [--out PATH] [--rounds N] [--iters N] [--models 0.6B,1.7B]
"""
import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "ace-step-1.5_amd")]
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402
from acehip.config import DiTConfig  # noqa: E402
from acehip.lm import HipCausalLM, HipLMRuntime  # noqa: E402
from acehip.weights import synth_text_encoder_weights  # noqa: E402

VOCAB, LAYERS, S = 217204, 28, 1500
TARGETS = (64, 512)
MODELS = {"0.6B": (1024, 3072), "1.7B": (2048, 6144)}
HBM_BPS, MFMA_FLOPS = 8e12, 2.5e15


def timed(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def interleaved(runs, rounds, iters, flush, warm=2):
    for fn in runs.values():
        for _ in range(warm):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in runs}
    for _ in range(rounds):
        for k, fn in runs.items():
            flush.add_(1)
            times[k].append(timed(fn, iters))
    return ({k: round(statistics.median(v), 4) for k, v in times.items()},
            {k: [round(min(v), 4), round(max(v), 4)] for k, v in times.items()})


def hf_model(hidden, inter, dev):
    try:
        from transformers import Qwen3Config, Qwen3ForCausalLM
    except Exception as e:                       # not installed: no baseline, said so in the JSON
        return None, f"transformers does not import: {e}"
    cfg = Qwen3Config(vocab_size=VOCAB, hidden_size=hidden, intermediate_size=inter, num_hidden_layers=LAYERS,
                      num_attention_heads=16, num_key_value_heads=8, head_dim=128, rms_norm_eps=1e-6,
                      rope_theta=1_000_000.0, max_position_embeddings=8192, attention_bias=False,
                      use_sliding_window=False, tie_word_embeddings=True)
    with torch.device(dev):
        model = Qwen3ForCausalLM(cfg).to(torch.bfloat16).eval()
    return model, None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "lm_score_bench.json"))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--models", default="0.6B,1.7B")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_lm_score needs a GPU (no CPU path)"
    dev = torch.device("cuda:0")
    flush = torch.zeros(300 * (1 << 20) // 4, device=dev)
    g = torch.Generator(device=dev).manual_seed(0)
    res = {"device": torch.cuda.get_device_name(0), "rounds": args.rounds, "iters": args.iters, "vocab": VOCAB,
           "layers": LAYERS, "S": S, "hbm_TBps_for_floor": HBM_BPS / 1e12, "mfma_PFLOPs_for_floor": MFMA_FLOPS / 1e15,
           "models": {}}
    ok = True
    for name in args.models.split(","):
        hidden, inter = MODELS[name]
        cfg = DiTConfig(hidden_size=hidden, intermediate_size=inter, num_hidden_layers=LAYERS,
                        num_attention_heads=16, num_key_value_heads=8, head_dim=128, rms_norm_eps=1e-6,
                        rope_theta=1_000_000.0)
        W = synth_text_encoder_weights(cfg, VOCAB, seed=0, mode="bench", device=dev, dtype=torch.bfloat16,
                                       backend="torch")
        rt = HipLMRuntime(cfg, 0, max_batch=2, capacity=S + 64, prefill_tokens=S + 64)
        rt.load(W)
        del W
        lm = HipCausalLM(rt)
        hf, why = hf_model(hidden, inter, dev)
        ids = torch.randint(0, VOCAB, (1, S), device=dev, generator=g)
        mask = torch.ones(1, S, dtype=torch.long, device=dev)
        rows = {}
        for T in TARGETS:
            P = S - T

            def call():
                lp, _ = lm.score(ids, P)
                return lp.float().cpu().mean().item()

            runs = {"call_ms": call}
            if hf is not None:
                def hf_fwd_copy():
                    with torch.no_grad():
                        logits = hf(input_ids=ids, attention_mask=mask).logits
                    return logits[0, P - 1:-1, :].cpu(), ids[0, P:].cpu()

                def hf_call():
                    pred, tg = hf_fwd_copy()
                    lp = F.log_softmax(pred, dim=-1)
                    return lp[torch.arange(tg.shape[0]), tg].mean().item()
                runs["hf_fwd_copy_ms"] = hf_fwd_copy
                runs["hf_call_ms"] = hf_call
            med, spread = interleaved(runs, args.rounds, args.iters, flush)
            row = dict(med, spread_ms=spread)
            if hf is not None:
                row["ratio_hf_fwd_copy_over_ours"] = round(row["hf_fwd_copy_ms"] / row["call_ms"], 2)
                row["ratio_hf_call_over_ours"] = round(row["hf_call_ms"] / row["call_ms"], 2)
                row["not_slower"] = row["call_ms"] <= row["hf_fwd_copy_ms"]
                ok = ok and row["not_slower"]
            # the kernel alone
            h = torch.randn(T, hidden, device=dev, generator=g).bfloat16()
            tg = ids[0, P:]
            med, spread = interleaved({"k": lambda: rt.score_rows(h, tg)}, args.rounds, 10, flush)
            w_bytes = 2 * VOCAB * hidden
            flop = 2 * T * VOCAB * hidden
            kern = {"ms": med["k"], "spread_ms": spread["k"], "passes": 2, "W_bytes_per_pass": w_bytes,
                    "flop_per_pass": flop, "floor_hbm_ms": round(2 * w_bytes / HBM_BPS * 1e3, 4),
                    "floor_mfma_ms": round(2 * flop / MFMA_FLOPS * 1e3, 4)}
            kern["floor_ms"] = max(kern["floor_hbm_ms"], kern["floor_mfma_ms"])
            kern["bound_by"] = "hbm" if kern["floor_hbm_ms"] >= kern["floor_mfma_ms"] else "mfma"
            kern["over_floor"] = round(kern["ms"] / kern["floor_ms"], 2)
            kern["TFLOPs"] = round(2 * flop / kern["ms"] * 1e-9, 1)
            kern["W_GBps"] = round(2 * w_bytes / kern["ms"] * 1e-6, 1)
            row["kernel"] = kern
            rows[f"T{T}"] = row
            print(name, f"T={T}", json.dumps(row), flush=True)
        res["models"][name] = {"hidden": hidden, "intermediate": inter, "calls": rows,
                               "hf_baseline": "timed" if hf is not None else why}
        lm.close()
        del hf, lm, rt
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", args.out)
    assert ok, "a scoring call through HipCausalLM is slower than transformers' at some shape"


if __name__ == "__main__":
    main()
