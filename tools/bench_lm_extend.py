#!/usr/bin/env python3
"""Prompt-reusing scoring against the plain scoring call, in one process, by the method of
tools/bench_lm_score.py: the 0.6B and 1.7B shapes (28 layers, vocabulary 217 204, synthetic
weights), S = 1500 tokens of which the last T = 64 / 512 are the scored target; medians of
interleaved rounds from device events, a 300 MB buffer written before every timed arm.

Three arms per shape and T, each a whole ``_calculate_log_prob``-equivalent call (embedding,
layers, acehip_lm_score_bf16 over T rows, the fp32 mean and its copy to the host):
  plain_ms   HipCausalLM.score(reuse=False): acehip_enc_forward over all S positions — the call
             profiles/lm_score_bench.json times as call_ms
  cold_ms    score on an empty slot (start = 0): acehip_enc_extend over all S positions, K/V
             written to the slot's cache row
  warm_ms    score on a slot that holds the sequence (start = prompt_len − 1): acehip_enc_extend
             over T + 1 rows against the cached prompt (primed by an untimed call)
and what they mean for a song's roughly ten calls: warm_faster (the warm arm's slowest round
against the plain arm's fastest), cold − plain, and the number of warm calls after which one
cold call has paid for itself.

The attention kernel alone (acehip_attention_extend_bf16, B = 1, 16 / 8 heads) at (n, keys) =
(64, 1500), (512, 1500), (512, 8192): its plan, its time, and its floors — K and V read once per
KV head plus q and o over HBM bandwidth (8 TB/s), and the causal 4·H·128·Σ(keys of query i) FLOP
over the bf16 MFMA peak (2.5 PF).

With --models 4B the 4B's shape (36 layers, 2560 / 9728, 32 / 8 heads) runs the same arms, and —
for every model whose heads / kv_heads is 4, whose prefill attention the handle sends to
acehip_attention_extend_bf16 — a "prefill" entry: acehip_enc_prefill at B = 2, S = 1500 (row 1
left-padded by 9), that attention launch alone (B = 2, n = S, pos = 0, cap = S, the mask) and the
layer's four GEMMs alone at M = 3000 (QKV head-post, O residual, SwiGLU, down residual), with
attention_share = layers · attention / prefill and attention_over_gemms.

Writes profiles/lm_extend_bench.json; a run of some models replaces those models' entries of an
existing file and keeps the others.

usage: bench_lm_extend.py [--out PATH] [--rounds N] [--iters N] [--models 0.6B,1.7B,4B]
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

VOCAB, S = 217204, 1500
TARGETS = (64, 512)
# name -> (hidden, intermediate, layers, heads, kv_heads)
MODELS = {"0.6B": (1024, 3072, 28, 16, 8), "1.7B": (2048, 6144, 28, 16, 8), "4B": (2560, 9728, 36, 32, 8)}
PREFILL_B, PREFILL_PAD = 2, 9
ATTN_SHAPES = ((64, 1500), (512, 1500), (512, 8192))
H, KV = 16, 8
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
    """runs: name -> (prep or None, fn).  prep runs untimed before the flush of every round."""
    for prep, fn in runs.values():
        for _ in range(warm):
            if prep:
                prep()
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in runs}
    for _ in range(rounds):
        for k, (prep, fn) in runs.items():
            if prep:
                prep()
            flush.add_(1)
            times[k].append(timed(fn, iters))
    return ({k: round(statistics.median(v), 4) for k, v in times.items()},
            {k: [round(min(v), 4), round(max(v), 4)] for k, v in times.items()})


def bench_attention(dev, flush, rounds, gen):
    out = {}
    scale = 1 / math.sqrt(128)
    for n, keys in ATTN_SHAPES:
        pos = keys - n
        q = torch.randn(1, H, n, 128, device=dev, generator=gen).bfloat16()
        k = torch.randn(1, KV, keys, 128, device=dev, generator=gen).bfloat16()
        v = torch.randn(1, KV, keys, 128, device=dev, generator=gen).bfloat16()
        o = torch.empty(n, H * 128, device=dev, dtype=torch.bfloat16)
        nb = ff.lib().acehip_attention_extend_ws_bytes(1, H, n)
        ws = torch.empty(nb, device=dev, dtype=torch.uint8)

        def run():
            ff.check(ff.lib().acehip_attention_extend_bf16(ff.ptr(q), ff.ptr(k), ff.ptr(v), ff.ptr(o), 1, H, KV, n, pos,
                                                           keys, None, 0, scale, ff.ptr(ws), nb, ff.stream_ptr()))
        med, spread = interleaved({"k": (None, run)}, rounds, 20, flush)
        plan = ff.attn_extend_plan(1, H, KV, n, pos)
        nbytes = 2 * KV * keys * 128 * 2 + 2 * H * n * 128 * 2
        flop = 4 * H * 128 * sum(pos + i + 1 for i in range(n))
        row = {"us": round(med["k"] * 1e3, 2), "spread_us": [round(x * 1e3, 2) for x in spread["k"]],
               "plan": {f: plan[f] for f in ("units", "parts", "tiles", "tiles_per_part", "grid")},
               "bytes": nbytes, "flop": flop, "floor_hbm_us": round(nbytes / HBM_BPS * 1e6, 3),
               "floor_mfma_us": round(flop / MFMA_FLOPS * 1e6, 3)}
        row["over_floor"] = round(row["us"] / max(row["floor_hbm_us"], row["floor_mfma_us"]), 1)
        out[f"n{n}_keys{keys}"] = row
        print("attention", n, keys, json.dumps(row), flush=True)
    return out


def bench_prefill(rt, cfg, dev, flush, rounds, iters, gen):
    """acehip_enc_prefill at [PREFILL_B, S] on a heads / kv_heads = 4 runtime, its attention launch
    and one layer's four GEMMs alone."""
    Bp, hidden, inter = PREFILL_B, cfg.hidden_size, cfg.intermediate_size
    Hq, Hkv, L = cfg.num_attention_heads, cfg.num_key_value_heads, cfg.num_hidden_layers
    M, qd, N3 = Bp * S, Hq * 128, (Hq + 2 * Hkv) * 128
    scale = 1 / math.sqrt(128)
    x = rt.embed(torch.randint(0, VOCAB, (Bp, S), device=dev, generator=gen))
    km = torch.ones(Bp, S, dtype=torch.uint8, device=dev)
    km[1, :PREFILL_PAD] = 0

    def rnd(*shape, s=1.0):
        return (torch.randn(*shape, device=dev, generator=gen) * s).bfloat16()
    q, k, v = rnd(Bp, Hq, S, 128), rnd(Bp, Hkv, S, 128), rnd(Bp, Hkv, S, 128)
    ao = torch.empty(M, qd, device=dev, dtype=torch.bfloat16)
    nb = ff.lib().acehip_attention_extend_ws_bytes(Bp, Hq, S)
    ws = torch.empty(nb, device=dev, dtype=torch.uint8)
    xn, hb, res = rnd(M, hidden), rnd(M, inter), rnd(M, hidden)
    wqkv, wo = rnd(N3, hidden, s=0.02), rnd(hidden, qd, s=0.02)
    wgu, wdn = rnd(2 * inter, hidden, s=0.02), rnd(hidden, inter, s=0.02)
    nw = torch.ones(128, device=dev, dtype=torch.bfloat16)
    cs = torch.ones(S, 128, device=dev, dtype=torch.bfloat16)
    hbo = torch.empty(M, inter, device=dev, dtype=torch.bfloat16)
    lib, P, sp = ff.lib(), ff.ptr, ff.stream_ptr

    def prefill():
        rt.prefill(x, km)

    def attn():
        ff.check(lib.acehip_attention_extend_bf16(P(q), P(k), P(v), P(ao), Bp, Hq, Hkv, S, 0, S, P(km), S, scale, P(ws),
                                                  nb, sp()), "attention_extend")

    def gemms():
        ff.check(lib.acehip_gemm_headpost_bf16(P(xn), hidden, P(wqkv), hidden, Bp, S, Hq, Hkv, Hkv, P(nw), P(nw), P(cs),
                                               P(cs), 1e-6, P(q), P(k), P(v), sp()), "qkv")
        ff.check(lib.acehip_gemm_bf16_ex(P(ao), qd, P(wo), qd, P(res), hidden, M, hidden, qd, None, 2, -1, sp()), "o")
        ff.check(lib.acehip_gemm_bf16_ex(P(xn), hidden, P(wgu), hidden, P(hbo), inter, M, 2 * inter, hidden, None, 3, -1,
                                         sp()), "swiglu")
        ff.check(lib.acehip_gemm_bf16_ex(P(hb), inter, P(wdn), inter, P(res), hidden, M, hidden, inter, None, 2, -1,
                                         sp()), "down")
    med, spread = interleaved({"prefill_ms": (None, prefill), "attention_ms": (None, attn), "layer_gemms_ms": (None, gemms)},
                              rounds, iters, flush)
    plan = ff.attn_extend_plan(Bp, Hq, Hkv, S, 0)
    row = dict(med, spread_ms=spread, B=Bp, S=S, left_pad_row1=PREFILL_PAD, layers=L,
               attention_plan={f: plan[f] for f in ("units", "parts", "tiles", "tiles_per_part", "grid")})
    row["attention_share_of_prefill"] = round(L * med["attention_ms"] / med["prefill_ms"], 3)
    row["attention_over_layer_gemms"] = round(med["attention_ms"] / med["layer_gemms_ms"], 2)
    row["prefill_tokens_per_s"] = round(M / med["prefill_ms"] * 1e3)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "lm_extend_bench.json"))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--models", default="0.6B,1.7B")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_lm_extend needs a GPU (no CPU path)"
    dev = torch.device("cuda:0")
    flush = torch.zeros(300 * (1 << 20) // 4, device=dev)
    g = torch.Generator(device=dev).manual_seed(0)
    res = {"device": torch.cuda.get_device_name(0), "rounds": args.rounds, "iters": args.iters, "vocab": VOCAB,
           "S": S, "hbm_TBps_for_floor": HBM_BPS / 1e12, "mfma_PFLOPs_for_floor": MFMA_FLOPS / 1e15,
           "attention": bench_attention(dev, flush, args.rounds, g), "models": {}}
    prior = os.path.join(REPO, "profiles", "lm_score_bench.json")
    prior = json.load(open(prior))["models"] if os.path.exists(prior) else {}
    for name in args.models.split(","):
        hidden, inter, LAYERS, Hm, KVm = MODELS[name]
        cfg = DiTConfig(hidden_size=hidden, intermediate_size=inter, num_hidden_layers=LAYERS,
                        num_attention_heads=Hm, num_key_value_heads=KVm, head_dim=128, rms_norm_eps=1e-6,
                        rope_theta=1_000_000.0)
        W = synth_text_encoder_weights(cfg, VOCAB, seed=0, mode="bench", device=dev, dtype=torch.bfloat16,
                                       backend="torch")
        wide = Hm == 4 * KVm
        rt = HipLMRuntime(cfg, 0, max_batch=2, capacity=S + 64, prefill_tokens=(PREFILL_B if wide else 1) * (S + 64),
                          score_slots=2)
        rt.load(W)
        del W
        lm = HipCausalLM(rt)
        ids = torch.randint(0, VOCAB, (1, S), device=dev, generator=g)
        rows = {}
        for T in TARGETS:
            P = S - T

            def plain():
                lp, _ = lm.score(ids, P, reuse=False)
                return lp.float().cpu().mean().item()

            def cold():
                lm.reset_score_cache()
                lp, _ = lm.score(ids, P)
                assert lm.score_stats["last_start"] == 0
                return lp.float().cpu().mean().item()

            def warm():
                lp, _ = lm.score(ids, P)
                assert lm.score_stats["last_start"] == P - 1
                return lp.float().cpu().mean().item()

            def prime():
                lm.reset_score_cache()
                lm.score(ids, P)
                torch.cuda.synchronize()

            # the arms agree: same targets, same weights, kernels of the same tolerance
            a, b, c = plain(), cold(), warm()
            med, spread = interleaved({"plain_ms": (None, plain), "cold_ms": (None, cold), "warm_ms": (prime, warm)},
                                      args.rounds, args.iters, flush)
            row = dict(med, spread_ms=spread, mean_logprob={"plain": a, "cold": b, "warm": c})
            row["warm_faster_beyond_spread"] = spread["warm_ms"][1] < spread["plain_ms"][0]
            row["plain_over_warm"] = round(row["plain_ms"] / row["warm_ms"], 2)
            row["cold_minus_plain_ms"] = round(row["cold_ms"] - row["plain_ms"], 4)
            gain = row["plain_ms"] - row["warm_ms"]
            row["warm_calls_to_pay_for_one_cold"] = (0 if row["cold_ms"] <= row["plain_ms"] else
                                                     math.ceil((row["cold_ms"] - row["plain_ms"]) / gain) if gain > 0
                                                     else None)
            # a song: one cold call per prompt (two prompts), the other eight warm, against ten plain calls
            row["ten_calls_ms"] = {"plain": round(10 * row["plain_ms"], 2),
                                   "reuse": round(2 * row["cold_ms"] + 8 * row["warm_ms"], 2)}
            was = prior.get(name, {}).get("calls", {}).get(f"T{T}", {}).get("call_ms")
            if was is not None:
                row["lm_score_bench_call_ms"] = was
            rows[f"T{T}"] = row
            print(name, f"T={T}", json.dumps(row), flush=True)
        res["models"][name] = {"rounds": args.rounds, "iters": args.iters, "hidden": hidden, "intermediate": inter,
                               "layers": LAYERS, "heads": Hm, "kv_heads": KVm,
                               "calls": rows}
        if wide:
            res["models"][name]["prefill"] = bench_prefill(rt, cfg, dev, flush, args.rounds, args.iters, g)
            print(name, "prefill", json.dumps(res["models"][name]["prefill"]), flush=True)
        lm.close()
        del lm, rt
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    if os.path.exists(args.out):                 # the models not run keep their recorded entries
        old = json.load(open(args.out))
        if not set(old.get("models", {})) <= set(res["models"]):     # a partial run: the file's header stays too
            res = dict(old, models=dict(old["models"], **res["models"]))
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
