#!/usr/bin/env python3
"""One decode step of the 5 Hz LM on the HIP path, at the 0.6B and 1.7B shapes (28 layers, 16 / 8
heads) and, with --models 4B, at the 4B's (36 layers, 2560 / 9728, 32 / 8 heads) —
vocabulary 217 204 = Qwen3's 151 936 plus the audio-code tokens, synthetic weights —, B = 2
(CFG: cond + uncond row, the second left-padded), contexts 256 / 1024 / 2304 (the codes
phase of a 240 s song ends near 2304).

Per shape and context, medians of interleaved rounds from device events (a 300 MB buffer is
written between rounds, so a round starts with nothing of the model in the caches):
  step_ms        acehip_enc_decode + acehip_lm_head_bf16 (the runtime call and the vocabulary
                 projection) at cache index context − 1
  call_ms        the same step through HipCausalLM.__call__ (embedding gather, mask column,
                 output objects): what the reference's loop sees
  floor_ms       bytes a step must read — layer weights + lm_head + the K/V rows of the
                 context — at 8 TB/s
  hf_call_ms     transformers' Qwen3ForCausalLM of the same config, bf16, under
                 torch.inference_mode(), the same call pattern (one token, past_key_values, mask), if
                 transformers imports; ratio = hf_call_ms / call_ms
and the two new kernels alone with their GB/s.  lm_head's weight (445 / 890 MB) is larger than
the 256 MB last-level cache by itself, so its figure is an HBM figure.  attn_decode cycles over
28 distinct caches as the layer loop does: 528 MB at context 2304 (from HBM), but 59 MB and
235 MB at 256 and 1024, which fit in the last-level cache (the 300 MB write runs once per
round, not per launch) — those two GB/s figures are not HBM figures.
Writes profiles/lm_decode_bench.json; a run of some models replaces those models' entries of an
existing file and keeps the others.  Condition: call_ms <= hf_call_ms at every shape.

usage: bench_lm_decode.py [--out PATH] [--rounds N] [--iters N] [--models 0.6B,1.7B,4B]
"""
import argparse
import json
import math
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "ace-step-1.5_amd")]
import torch  # noqa: E402
from acehip import _ffi as ff  # noqa: E402
from acehip.config import DiTConfig  # noqa: E402
from acehip.lm import HipCausalLM, HipLMRuntime  # noqa: E402
from acehip.weights import synth_text_encoder_weights  # noqa: E402

VOCAB, B, PAD = 217204, 2, 9
CONTEXTS = (256, 1024, 2304)
# name -> (hidden, intermediate, layers, heads, kv_heads)
MODELS = {"0.6B": (1024, 3072, 28, 16, 8), "1.7B": (2048, 6144, 28, 16, 8), "4B": (2560, 9728, 36, 32, 8)}
HBM_BPS = 8e12


def timed(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def interleaved(runs, rounds, iters, flush):
    for fn in runs.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in runs}
    for _ in range(rounds):
        for k, fn in runs.items():
            flush.add_(1)
            times[k].append(timed(fn, iters))
    return ({k: round(statistics.median(v), 4) for k, v in times.items()},
            {k: [round(min(v), 4), round(max(v), 4)] for k, v in times.items()})


def hf_model(hidden, inter, LAYERS, H, KV, dev):
    try:
        from transformers import Qwen3Config, Qwen3ForCausalLM
    except Exception as e:                       # not installed: no baseline, said so in the JSON
        return None, f"transformers does not import: {e}"
    cfg = Qwen3Config(vocab_size=VOCAB, hidden_size=hidden, intermediate_size=inter, num_hidden_layers=LAYERS,
                      num_attention_heads=H, num_key_value_heads=KV, head_dim=128, rms_norm_eps=1e-6,
                      rope_theta=1_000_000.0, max_position_embeddings=8192, attention_bias=False,
                      use_sliding_window=False, tie_word_embeddings=True)
    with torch.device(dev):
        model = Qwen3ForCausalLM(cfg).to(torch.bfloat16).eval()
    return model, None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "lm_decode_bench.json"))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--models", default="0.6B,1.7B")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_lm_decode needs a GPU (no CPU path)"
    dev = torch.device("cuda:0")
    flush = torch.zeros(300 * (1 << 20) // 4, device=dev)
    cap = max(CONTEXTS) + 64
    g = torch.Generator(device=dev).manual_seed(0)
    res = {"device": torch.cuda.get_device_name(0), "rounds": args.rounds, "iters": args.iters, "vocab": VOCAB,
           "B": B, "left_pad_row1": PAD, "hbm_TBps_for_floor": HBM_BPS / 1e12, "models": {}}
    ok = True
    for name in args.models.split(","):
        hidden, inter, LAYERS, H, KV = MODELS[name]
        cfg = DiTConfig(hidden_size=hidden, intermediate_size=inter, num_hidden_layers=LAYERS,
                        num_attention_heads=H, num_key_value_heads=KV, head_dim=128, rms_norm_eps=1e-6,
                        rope_theta=1_000_000.0)
        W = synth_text_encoder_weights(cfg, VOCAB, seed=0, mode="bench", device=dev, dtype=torch.bfloat16,
                                       backend="torch")
        rt = HipLMRuntime(cfg, 0, max_batch=B, capacity=cap, prefill_tokens=B * cap)
        rt.load(W)
        del W
        lm = HipCausalLM(rt)
        layer_bytes = LAYERS * 2 * (hidden * (H + 2 * KV) * 128 + hidden * H * 128 + 3 * hidden * inter)
        head_bytes = 2 * VOCAB * hidden
        hf, why = hf_model(hidden, inter, LAYERS, H, KV, dev)
        rows = {}
        for ctx in CONTEXTS:
            ids = torch.randint(0, VOCAB, (B, ctx - 1), device=dev, generator=g)
            mask = torch.ones(B, ctx, dtype=torch.long, device=dev)
            mask[1, :PAD] = 0
            past = lm(input_ids=ids, attention_mask=mask[:, :ctx - 1]).past_key_values   # fills the cache
            tok = ids[:, -1:]
            x = rt.embed(tok[:, 0])
            pos = ctx - 1

            def step():
                rt.lm_head(rt.decode(x, lm._mask, pos))

            def call():
                past.length = pos                                 # hold the context: every call is step `pos`
                lm(input_ids=tok, past_key_values=past, attention_mask=mask)

            runs = {"step_ms": step, "call_ms": call}
            if hf is not None:
                with torch.inference_mode():
                    hf_past = hf(input_ids=ids, attention_mask=mask[:, :ctx - 1], use_cache=True).past_key_values
                full = torch.ones(B, ctx + 4096, dtype=torch.long, device=dev)
                full[1, :PAD] = 0

                def hf_call():                                    # its cache grows by one per call
                    with torch.inference_mode():
                        n = hf_past.get_seq_length()
                        hf(input_ids=tok, past_key_values=hf_past, attention_mask=full[:, :n + 1], use_cache=True)
                runs["hf_call_ms"] = hf_call
            med, spread = interleaved(runs, args.rounds, args.iters, flush)
            kv_bytes = LAYERS * B * KV * ctx * 128 * 2 * 2
            row = dict(med, spread_ms=spread, floor_ms=round((layer_bytes + head_bytes + kv_bytes) / HBM_BPS * 1e3, 4),
                       bytes={"layers": layer_bytes, "lm_head": head_bytes, "kv": kv_bytes})
            row["step_over_floor"] = round(row["step_ms"] / row["floor_ms"], 2)
            if hf is not None:
                row["hf_context_end"] = hf_past.get_seq_length()
                row["ratio_hf_over_ours"] = round(row["hf_call_ms"] / row["call_ms"], 2)
                row["not_slower"] = row["call_ms"] <= row["hf_call_ms"]
                ok = ok and row["not_slower"]
                del hf_past
            rows[f"ctx{ctx}"] = row
            print(name, f"ctx={ctx}", json.dumps(row), flush=True)
        # the kernels alone
        kern = {}
        y = torch.empty(B, VOCAB, device=dev, dtype=torch.bfloat16)
        xh = torch.randn(B, hidden, device=dev, generator=g).bfloat16()

        def head():
            ff.check(ff.lib().acehip_lm_head_bf16(ff.ptr(xh), hidden, ff.ptr(rt.w_head), ff.ptr(y), VOCAB, B, VOCAB,
                                                  hidden, ff.stream_ptr()), "lm_head")
        med, _ = interleaved({"lm_head": head}, args.rounds, args.iters, flush)
        kern["lm_head"] = {"us": round(med["lm_head"] * 1e3, 1), "GBps": round(head_bytes / med["lm_head"] * 1e-6, 1)}
        nb = ff.lib().acehip_attention_decode_ws_bytes(B, H)
        ws = torch.empty(nb, device=dev, dtype=torch.uint8)
        q = torch.randn(B, H, 128, device=dev, generator=g).bfloat16()
        o = torch.empty(B, H * 128, device=dev, dtype=torch.bfloat16)
        for ctx in CONTEXTS:
            kc = torch.randn(LAYERS, 2, B, KV, ctx, 128, device=dev, generator=g).bfloat16()
            km = torch.ones(B, ctx, dtype=torch.uint8, device=dev)
            km[1, :PAD] = 0
            state = {"l": 0}

            def attn():
                l = state["l"] = (state["l"] + 1) % LAYERS
                ff.check(ff.lib().acehip_attention_decode_bf16(ff.ptr(q), ff.ptr(kc[l, 0]), ff.ptr(kc[l, 1]), ff.ptr(o),
                                                               B, H, KV, ctx, ctx, ff.ptr(km), ctx,
                                                               1 / math.sqrt(128), ff.ptr(ws), nb, ff.stream_ptr()),
                         "attention_decode")
            med, _ = interleaved({"a": attn}, args.rounds, LAYERS, flush)
            nbytes = 2 * B * KV * ctx * 128 * 2
            kern[f"attn_decode_ctx{ctx}"] = {"us": round(med["a"] * 1e3, 2), "kv_bytes": nbytes,
                                             "GBps": round(nbytes / med["a"] * 1e-6, 1)}
            del kc
        print(name, "kernels", json.dumps(kern), flush=True)
        res["models"][name] = {"rounds": args.rounds, "iters": args.iters, "hidden": hidden, "intermediate": inter,
                               "layers": LAYERS, "heads": H, "kv_heads": KV,
                               "steps": rows, "kernels": kern,
                               "hf_baseline": "timed" if hf is not None else why}
        lm.close()
        del hf, lm, rt
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    if os.path.exists(args.out):                 # the models not run keep their recorded entries
        old = json.load(open(args.out))
        if not set(old.get("models", {})) <= set(res["models"]):     # a partial run: the file's header stays too
            res = dict(old, models=dict(old["models"], **res["models"]))
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", args.out)
    assert ok, "a decode call through HipCausalLM is slower than transformers' at some shape"


if __name__ == "__main__":
    main()
