#!/usr/bin/env python3
"""In-process A/B of the fused cross-Q projection + cross-attention launch (cross_q_attn_kernel,
ACEHIP_CROSS_FUSE) on the 240 s song's conditional rows: M = 3000, D = 2048, H = 16, KV = 8,
Lenc = 641, cold weights (rotating copies, ≈ 600 MB), through acehip_cross_attn_bf16:
  arm 0   gemm_w4_kernel<192, 128, head-post, 2> + attn_fwd_kernel<2> (whole units)   two launches
  arm 1   cross_q_attn_kernel                                                          one launch
HIP events around n back-to-back calls, so an arm's figure is the projection plus the attention.
Arms alternate inside every round; the default arms 0,1,0 time the two launches twice per round,
so each round also gives a same-vs-same spread.  The tool prints every arm per round and whether
arm 1 beat the NEARER arm-0 run in every round by more than twice that round's spread.  (Timing
only: tests/test_gpu_cross_fused.py compares the two paths' AO bit for bit; a one-call check of
that at this shape is printed first.)

usage: ab_cross_fuse.py   (ARMS=0,1,0  ROUNDS=5  WARM=2)"""
import ctypes
import math
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "ace-step-1.5_amd")]
import torch  # noqa: E402
from acehip import _ffi as ff  # noqa: E402

dev = torch.device("cuda:0")
arms = os.environ.get("ARMS", "0,1,0").split(",")
rounds = int(os.environ.get("ROUNDS", "5"))
warm = int(os.environ.get("WARM", "2"))   # untimed rounds first: the clock settles over the first few hundred launches
B, S, D, H, KV, Lenc = 1, int(os.environ.get("S", "3000")), 2048, 16, 8, 641
g = torch.Generator(device=dev).manual_seed(0)


def rand(*shape, scale=1.0):
    return (torch.randn(*shape, device=dev, generator=g) * scale).bfloat16()


xn = rand(B * S, D)
Ws = [rand(H * 128, D, scale=0.02) for _ in range(max(2, int(600e6 // (H * 128 * D * 2))))]
qnw, k, v = rand(128), rand(B, KV, Lenc, 128), rand(B, KV, Lenc, 128)
ao = torch.empty(B * S, H * 128, device=dev, dtype=torch.bfloat16)
path = ctypes.c_int(-1)
n = 48


def launch(i, arm):
    ff.check(ff.lib().acehip_cross_attn_bf16(ff.ptr(xn), ff.ptr(Ws[i % len(Ws)]), ff.ptr(qnw), ff.ptr(k), ff.ptr(v),
                                             ff.ptr(ao), B, S, H, KV, Lenc, D, 1e-6, 1.0 / math.sqrt(128.0), arm,
                                             ctypes.byref(path), ff.stream_ptr()))
    assert path.value == arm, f"arm {arm} ran path {path.value}"


outs = []
for arm in (0, 1):
    ao.fill_(float("nan"))
    launch(0, arm)
    torch.cuda.synchronize()
    outs.append(ao.clone())
print(f"AO of the two paths bit-identical: {torch.equal(outs[0].view(torch.int16), outs[1].view(torch.int16))}; "
      f"finite: {bool(torch.isfinite(outs[1].float()).all())}", flush=True)

res = [[] for _ in arms]
for rnd in range(rounds + warm):
    for j, arm in enumerate(arms):
        a = int(arm)
        for i in range(max(2, n // 4)):
            launch(i, a)
        torch.cuda.synchronize()
        if rnd < warm:
            for i in range(n):
                launch(i, a)
            continue
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for i in range(n):
            launch(i, a)
        e1.record()
        torch.cuda.synchronize()
        res[j].append(e0.elapsed_time(e1) / n * 1e3)
wins = []
for rnd in range(rounds):
    t = [res[j][rnd] for j in range(len(arms))]
    base = [t[j] for j, a in enumerate(arms) if a == "0"]
    new = [t[j] for j, a in enumerate(arms) if a == "1"]
    spread = max(base) - min(base) if len(base) > 1 else float("nan")
    win = bool(new) and len(base) > 1 and min(base) - max(new) > 2 * spread
    wins.append(win)
    print(f"round {rnd}: " + "  ".join(f"fuse={a} {t[j]:.2f} us" for j, a in enumerate(arms)) +
          f"   spread {spread:.2f}  gain {min(base) - max(new) if new else float('nan'):.2f}  {'WIN' if win else '-'}",
          flush=True)
for j, a in enumerate(arms):
    print(f"arm {j} fuse={a}: median {sorted(res[j])[len(res[j]) // 2]:.2f} us")
print(f"fused launch ahead of the nearer two-launch arm by > 2 x spread in every round: {all(wins)}")
