#!/usr/bin/env python3
"""In-process A/B of the persistent SwiGLU tile walk (ACEHIP_GEMM_PERSIST) on the 240 s gate/up
shape (M = 6000, N = 12288, K = 2048), cold weights (12 rotating copies, 600 MB), through the
production dispatch.  Arms alternate inside every round; the default arms 0,1,0 time the
one-tile-per-workgroup launch twice per round, so each round also gives a same-vs-same spread.

usage: ab_gemm_persist.py   (ARMS=0,1,0  ROUNDS=5  WARM=2  M=6000)"""
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "ace-step-1.5_amd")]
import torch  # noqa: E402
from acehip import _ffi as ff  # noqa: E402

dev = torch.device("cuda:0")
M, N, K = int(os.environ.get("M", "6000")), 12288, 2048
arms = os.environ.get("ARMS", "0,1,0").split(",")
rounds = int(os.environ.get("ROUNDS", "5"))
warm = int(os.environ.get("WARM", "2"))   # untimed rounds first: the clock settles over the first few hundred launches
g = torch.Generator(device=dev).manual_seed(0)
A = torch.randn(M, K, device=dev, generator=g).bfloat16()
Ws = [(torch.randn(N, K, device=dev, generator=g) * 0.02).bfloat16() for _ in range(12)]
C = torch.empty(M, N // 2, device=dev, dtype=torch.bfloat16)


def launches(n):
    for i in range(n):
        ff.check(ff.lib().acehip_gemm_bf16_ex(ff.ptr(A), K, ff.ptr(Ws[i % 12]), K, ff.ptr(C), N // 2, M, N, K, None,
                                              3, -1, ff.stream_ptr()))


outs = {}
res = [[] for _ in arms]
for rnd in range(rounds + warm):
    for j, arm in enumerate(arms):
        os.environ["ACEHIP_GEMM_PERSIST"] = arm
        ff.reload_knobs()
        launches(12)
        torch.cuda.synchronize()
        if rnd < warm:
            outs.setdefault(arm, C.clone())
            launches(48)
            continue   # warm-up round
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        launches(48)
        e1.record()
        torch.cuda.synchronize()
        res[j].append(e0.elapsed_time(e1) / 48 * 1e3)
same = all(torch.equal(o, outs[arms[0]]) for o in outs.values())
fl = 2.0 * M * N * K
for rnd in range(rounds):
    print(f"round {rnd}: " + "  ".join(f"persist={a} {res[j][rnd]:.2f} us" for j, a in enumerate(arms)), flush=True)
for j, a in enumerate(arms):
    us = sorted(res[j])[len(res[j]) // 2]
    print(f"arm {j} persist={a}: median {us:.2f} us  {fl / us / 1e6:.0f} TF/s")
print(f"outputs bit-identical across arms: {same}")
