#!/usr/bin/env python3
"""Lyric-alignment capture at the 240 s shape: T = 6000 (S = 3000), Lenc = 641, the
reference's default selection (acestep/handler.py:129: 7 pairs, layers 2..6), keys
[11, 523), Bc = 1 (get_lyric_timestamp) and Bc = 2 (get_lyric_score).

Reports, per Bc, from device events after warm-up (median of interleaved rounds):
  capture_stop_ms   acehip_dit_forward_capture with stop_after_last (7 of 24 layers)
  forward_ms        plain acehip_dit_forward on the same handle
  map kernel        µs per acehip_attention_probs_bf16 launch at each per-layer head count
                    of the selection, with the bytes it writes and the resulting GB/s
and writes profiles/lyric_attn_bench.json.  The only timing condition: the stop-early
capture is faster than the plain forward of the same Bc.  The reference's PyTorch path is not
timed (the reference is not part of a GPU run of this repository), so no speed-up is quoted.

usage: bench_lyric_attn.py [--out PATH] [--rounds N] [--iters N]
"""
import argparse
import ctypes
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
from acehip.dit import DiTRuntime, config_pairs  # noqa: E402
from acehip.weights import synth_dit_weights  # noqa: E402

T, LENC, K0, K1 = 6000, 641, 11, 523
CONFIG = {2: [6], 3: [10, 11], 4: [3], 5: [8, 9], 6: [8]}


def timed(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "lyric_attn_bench.json"))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_lyric_attn needs a GPU (no CPU path)"
    dev = torch.device("cuda:0")
    cfg = DiTConfig()
    S = (T + 1) // 2
    W = synth_dit_weights(cfg, seed=0, mode="bench", device=dev, dtype=torch.bfloat16, backend="torch")
    rt = DiTRuntime(cfg, 0, max_S=S, max_Bc=2, max_Lenc=LENC)
    rt.load(W)
    del W
    pairs = config_pairs(CONFIG)
    g = torch.Generator(device=dev).manual_seed(0)
    res = {"shape": {"T": T, "S": S, "Lenc": LENC, "k0": K0, "k1": K1, "pairs": len(pairs),
                     "layers_run_stop_early": max(CONFIG) + 1, "layers": cfg.num_hidden_layers},
           "device": torch.cuda.get_device_name(0), "rounds": args.rounds, "iters": args.iters}
    for Bc in (1, 2):
        xt = torch.randn(Bc, T, 64, device=dev, generator=g).bfloat16()
        ctx = torch.randn(Bc, T, 128, device=dev, generator=g).bfloat16()
        enc = torch.randn(Bc, LENC, cfg.hidden_size, device=dev, generator=g).bfloat16()
        t = torch.tensor([1.0, 0.125][:Bc], device=dev)
        rt.set_condition(enc)
        vt = torch.empty(Bc, T, 64, device=dev, dtype=torch.bfloat16)
        runs = {"capture_stop_ms": lambda: rt.forward_capture(xt, ctx, t, pairs, K0, K1, stop_early=True),
                "forward_ms": lambda: rt.forward(xt, ctx, t, out=vt)}
        for fn in runs.values():                     # warm-up: code objects, workspaces
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        times = {k: [] for k in runs}
        for _ in range(args.rounds):                 # interleaved rounds
            for k, fn in runs.items():
                times[k].append(timed(fn, args.iters))
        row = {k: round(statistics.median(v), 4) for k, v in times.items()}
        row["spread_ms"] = {k: [round(min(v), 4), round(max(v), 4)] for k, v in times.items()}
        row["stop_faster_than_forward"] = row["capture_stop_ms"] < row["forward_ms"]
        # the map kernel alone, at each per-layer head count of the selection
        q = torch.randn(Bc, 16, S, 128, device=dev, generator=g).bfloat16()
        k = torch.randn(Bc, 8, LENC, 128, device=dev, generator=g).bfloat16()
        kern = {}
        for n in sorted({len(v) for v in CONFIG.values()}):
            heads = (ctypes.c_int * n)(*range(3, 3 + n))
            out = torch.empty(n, Bc, K1 - K0, S, device=dev)

            def launch():
                ff.check(ff.lib().acehip_attention_probs_bf16(ff.ptr(q), ff.ptr(k), Bc, 16, 8, S, LENC, heads, n, K0,
                                                              K1, 1.0 / math.sqrt(128), ff.ptr(out), ff.stream_ptr()),
                         "attention_probs")
            for _ in range(5):
                launch()
            torch.cuda.synchronize()
            us = statistics.median(timed(launch, 50) * 1e3 for _ in range(args.rounds))
            written = out.numel() * 4
            # 2·128 FLOP per (query, key) score, all Lenc keys in pass 1 + the kept ones again in pass 2
            flop = 2.0 * 128 * n * Bc * S * (LENC + (K1 - K0))
            kern[f"heads_{n}"] = {"us_per_launch": round(us, 2), "bytes_written": written,
                                  "write_GBps": round(written / us * 1e-3, 1), "gflop": round(flop * 1e-9, 3)}
        row["map_kernel"] = kern
        res[f"Bc{Bc}"] = row
        print(f"Bc={Bc}", json.dumps(row), flush=True)
    rt.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", args.out)
    assert all(res[f"Bc{b}"]["stop_faster_than_forward"] for b in (1, 2)), "stop-early capture is not faster"


if __name__ == "__main__":
    main()
