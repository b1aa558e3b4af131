#!/usr/bin/env python3
"""The LM token loop's top-k / top-p logit filters at the vocabulary of the 5 Hz LM (217 204),
B = 1, 2, 4, fp32 (the CFG loop) and bf16 (the loop without CFG).

Rows: "codes" (the codes phase: only the last 65 268 ids finite, σ = 4) and "text" (all
finite, σ = 4).  Cases: top_p = 0.9 alone, top_k = 50 alone, and both.  Per cell, medians of
interleaved rounds from device events (a 300 MB buffer is written between rounds).  The filters
work in place, so every timed iteration first restores the row from a pristine copy; that copy
is timed alone in the same rounds (copy_ms) and taken off both figures:
  torch_ms        the torch chain of tests/lm_filter_ref.py on the GPU (topk / compare / masked
                  write; sort, softmax, scan, shift, scatter, masked write): what the loop runs today
  hip_ms          acehip_lm_filter through HipLogitFilters
  ratio           torch_ms / hip_ms
  bytes_floor_ms  the passes the kernels make over the rows (top-p: max, one histogram per key
                  digit — 3 for fp32, 2 for bf16 — and the rewrite; top-k: the same without the
                  max pass) at 8 TB/s
  share_*         both times as a share of call_ms (0.6B, context 2304) of profiles/lm_decode_bench.json
Writes profiles/lm_filter_bench.json.  Condition: hip_ms <= torch_ms in every cell.

usage: bench_lm_filter.py [--out PATH] [--rounds N] [--iters N]
"""
import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "ace-step-1.5_amd"), os.path.join(REPO, "tests")]
import torch  # noqa: E402
import lm_filter_ref as R  # noqa: E402
from acehip.lm import HipLogitFilters  # noqa: E402

VOCAB = 217204
BATCHES = (1, 2, 4)
CASES = {"top_p_0.9": (None, 0.9), "top_k_50": (50, None), "top_k_50_top_p_0.9": (50, 0.9)}
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
    return ({k: statistics.median(v) for k, v in times.items()},
            {k: [round(min(v), 4), round(max(v), 4)] for k, v in times.items()})


def passes(dtype, top_k, top_p):
    digits = 3 if dtype == torch.float32 else 2
    return (digits + 1 if top_k else 0) + (digits + 2 if top_p else 0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "lm_filter_bench.json"))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_lm_filter needs a GPU (no CPU path)"
    dev = torch.device("cuda:0")
    flush = torch.zeros(300 * (1 << 20) // 4, device=dev)
    with open(os.path.join(REPO, "profiles", "lm_decode_bench.json")) as f:
        call_ms = json.load(f)["models"]["0.6B"]["steps"]["ctx2304"]["call_ms"]
    hip = HipLogitFilters(R.torch_top_k, R.torch_top_p)
    res = {"device": torch.cuda.get_device_name(0), "rounds": args.rounds, "iters": args.iters, "vocab": VOCAB,
           "hbm_TBps_for_floor": HBM_BPS / 1e12, "call_ms_0.6B_ctx2304": call_ms, "cells": {}}
    ok = True
    for rows_name in ("codes", "text"):
        for dtype, tag in ((torch.float32, "f32"), (torch.bfloat16, "bf16")):
            for B in BATCHES:
                if rows_name == "codes":
                    src = torch.stack([R.codes_phase_row(VOCAB, 4.0, 100 + b, dtype=dtype) for b in range(B)]).to(dev)
                else:
                    src = torch.stack([R.scattered_row(VOCAB, 4.0, 200 + b, 0, dtype) for b in range(B)]).to(dev)
                buf = torch.empty_like(src)
                for case, (k, p) in CASES.items():
                    def restore():
                        buf.copy_(src)

                    def chain():
                        buf.copy_(src)
                        x = R.torch_top_k(buf, k)
                        R.torch_top_p(x, p)

                    def ours():
                        buf.copy_(src)
                        x = hip.top_k(buf, k) if k else buf
                        if p:
                            hip.top_p(x, p)
                    ours()
                    got = buf.clone()
                    chain()
                    same = bool(torch.equal(got.view(torch.int16 if dtype == torch.bfloat16 else torch.int32),
                                            buf.view(torch.int16 if dtype == torch.bfloat16 else torch.int32)))
                    med, spread = interleaved({"copy_ms": restore, "torch_ms": chain, "hip_ms": ours},
                                              args.rounds, args.iters, flush)
                    t, h = med["torch_ms"] - med["copy_ms"], med["hip_ms"] - med["copy_ms"]
                    cell = {"torch_ms": round(t, 4), "hip_ms": round(h, 4), "copy_ms": round(med["copy_ms"], 4),
                            "ratio": round(t / h, 2), "spread_ms_with_copy": spread,
                            "bytes_floor_ms": round(passes(dtype, k, p) * src.numel() * src.element_size() / HBM_BPS * 1e3, 5),
                            "share_of_call_torch": round(t / call_ms, 3), "share_of_call_hip": round(h / call_ms, 3),
                            "kept": [R.kept_count(r) for r in got], "same_bits_as_torch": same,
                            "not_slower": h <= t}
                    ok = ok and cell["not_slower"]
                    name = f"{rows_name}.{tag}.B{B}.{case}"
                    res["cells"][name] = cell
                    print(name, json.dumps(cell), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", args.out)
    assert ok, "acehip_lm_filter is slower than the torch chain in some cell"


if __name__ == "__main__":
    main()
