#!/usr/bin/env python3
"""In-process A/B of the slot-immediate K loop of the scalar-base ping-pong GEMMs
(ACEHIP_GEMM_SLOTIMM) on the 240 s song's launches, cold weights (rotating copies, ≈ 600 MB per
family), through the production dispatch:
  down      M = 6000, N = 2048, K = 6144, gated residual        gemm_pp_kernel<192, gated>
  o         M = 6000, N = 2048, K = 2048, gated residual        gemm_pp_kernel<192, gated>
  qkv       B = 2, S = 3000, 16 | 8 | 8 heads, K = 2048         gemm_pp_split_kernel<head-post>
  qkv0      B = 1, S = 3000 (layer 0, CFG rows deduplicated)    gemm_pp_kernel<192, head-post>: pointer form at 0,
                                                                scalar base + slot immediates at 1
  swiglu    M = 6000, N = 12288, K = 2048                       gemm_pp_persist_kernel (the walk)
  crosso    M = 3000, N = 2048, K = 2048, residual              the four-wave tile: no ping-pong loop
  vae       (not in the default list) the whole 240 s decode (T = 6000): its GEMM convs, pointer form
crosso runs no ping-pong kernel and the vae's convs keep the pointer form: both arms of those two
time one kernel — they are the controls.
Arms alternate inside every round; the default arms 0,1,0 time knob 0 twice per round, so each round
also gives a same-vs-same spread.  Per round and family the tool prints every arm, and at the end
whether knob 1 (any value other than the first arm's) beat the NEARER knob-0 arm in every round by
more than twice that round's spread.
(Timing only: tests/test_gpu_gemm_slotimm.py compares the two loops' outputs bit for bit; the
in-place residual families accumulate into their output from launch to launch.)

usage: ab_gemm_slotimm.py   (ARMS=0,1,0  ROUNDS=5  WARM=2  LAUNCHES=48  FAMILIES=down,o,qkv,qkv0,swiglu,crosso)"""
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
launches = int(os.environ.get("LAUNCHES", "48"))   # per timed arm
families = os.environ.get("FAMILIES", "down,o,qkv,qkv0,swiglu,crosso").split(",")
g = torch.Generator(device=dev).manual_seed(0)


def rand(*shape, scale=1.0):
    return (torch.randn(*shape, device=dev, generator=g) * scale).bfloat16()


def weights(N, K):
    return [rand(N, K, scale=0.02) for _ in range(max(2, int(600e6 // (N * K * 2))))]


def res_family(M, N, K, gated=True):
    A, Ws = rand(M, K), weights(N, K)
    X, gate = rand(M, N), rand(2, N)

    def launch(i):
        ff.check(ff.lib().acehip_gemm_res_bf16(ff.ptr(A), K, ff.ptr(Ws[i % len(Ws)]), K, ff.ptr(X), N, M, N, K,
                                               ff.ptr(X), N, ff.ptr(gate) if gated else None, N, M // 2, -1,
                                               ff.stream_ptr()))
    return launch, launches


def hp_family(B, S):
    K, nq, nk, nv = 2048, 16, 8, 8
    N = (nq + nk + nv) * 128
    A, Ws = rand(B * S, K), weights(N, K)
    qw, kw, cos, sin = rand(128), rand(128), rand(S, 128), rand(S, 128)
    q, k, v = (torch.empty(B, n, S, 128, device=dev, dtype=torch.bfloat16) for n in (nq, nk, nv))

    def launch(i):
        ff.check(ff.lib().acehip_gemm_headpost_bf16(ff.ptr(A), K, ff.ptr(Ws[i % len(Ws)]), K, B, S, nq, nk, nv,
                                                    ff.ptr(qw), ff.ptr(kw), ff.ptr(cos), ff.ptr(sin), 1e-6, ff.ptr(q),
                                                    ff.ptr(k), ff.ptr(v), ff.stream_ptr()))
    return launch, launches


def swiglu_family(M, N, K):
    A, Ws = rand(M, K), weights(N, K)
    C = torch.empty(M, N // 2, device=dev, dtype=torch.bfloat16)

    def launch(i):
        ff.check(ff.lib().acehip_gemm_bf16_ex(ff.ptr(A), K, ff.ptr(Ws[i % len(Ws)]), K, ff.ptr(C), N // 2, M, N, K, None,
                                              3, -1, ff.stream_ptr()))
    return launch, launches


def vae_family():
    from acehip.config import VAEConfig
    from acehip.vae import OobleckBackend
    from acehip.weights import synth_vae_weights
    vc = VAEConfig()
    vae = OobleckBackend(vc, 0, max_T=6000, with_encoder=False)
    vae.load(synth_vae_weights(vc, seed=0, mode="bench", with_encoder=False, device=dev, dtype=torch.bfloat16,
                               backend="torch"))
    z = rand(1, 64, 6000)
    return (lambda i: vae.decode_tensor(z)), 3


MAKE = {"vae": vae_family, "down": lambda: res_family(6000, 2048, 6144), "o": lambda: res_family(6000, 2048, 2048),
        "qkv": lambda: hp_family(2, 3000), "qkv0": lambda: hp_family(1, 3000),
        "swiglu": lambda: swiglu_family(6000, 12288, 2048), "crosso": lambda: res_family(3000, 2048, 2048, gated=False)}

verdict = {}
for fam in families:
    launch, n = MAKE[fam]()
    res = [[] for _ in arms]
    for rnd in range(rounds + warm):
        for j, arm in enumerate(arms):
            os.environ["ACEHIP_GEMM_SLOTIMM"] = arm
            ff.reload_knobs()
            for i in range(max(2, n // 4)):
                launch(i)
            torch.cuda.synchronize()
            if rnd < warm:
                for i in range(n):
                    launch(i)
                continue
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for i in range(n):
                launch(i)
            e1.record()
            torch.cuda.synchronize()
            res[j].append(e0.elapsed_time(e1) / n * 1e3)
    wins = []
    for rnd in range(rounds):
        t = [res[j][rnd] for j in range(len(arms))]
        base = [t[j] for j, a in enumerate(arms) if a == arms[0]]   # the first arm's value is the baseline
        new = [t[j] for j, a in enumerate(arms) if a != arms[0]]
        spread = max(base) - min(base) if len(base) > 1 else float("nan")
        win = bool(new) and len(base) > 1 and min(base) - max(new) > 2 * spread
        wins.append(win)
        print(f"{fam} round {rnd}: " + "  ".join(f"slotimm={a} {t[j]:.2f} us" for j, a in enumerate(arms)) +
              f"   spread {spread:.2f}  gain {min(base) - max(new) if new else float('nan'):.2f}  {'WIN' if win else '-'}",
              flush=True)
    for j, a in enumerate(arms):
        print(f"{fam} arm {j} slotimm={a}: median {sorted(res[j])[len(res[j]) // 2]:.2f} us")
    verdict[fam] = all(wins)
    del launch
    torch.cuda.empty_cache()
for fam, ok in verdict.items():
    print(f"{fam}: knob 1 ahead of the nearer knob-0 arm by > 2 x spread in every round: {ok}")
