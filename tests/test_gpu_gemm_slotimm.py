"""The slot-immediate K loop of the scalar-base ping-pong GEMMs (ACEHIP_GEMM_SLOTIMM=1: the loop
unrolled by the two ring slots and peeled, every LDS read a hoisted per-lane base + an immediate)
against the loop it replaces (=0, the parent's loop: the reference is not the code under test).
The same reads, DMAs, waits, barriers and MFMAs in the same order (tests/test_gemm_slotimm_host.py
checks the read addresses on the CPU), so the same bits.

Every comparison is torch.equal on int16 views of the whole output allocation — the live result,
the columns between N and the pitch, and guard rows after row M, all pre-filled with NaN.  A and W
are 16-byte-aligned views at a non-zero offset inside NaN-filled allocations with pitch K + 64.

K ∈ {64, 128, 192, 256, 320}, i.e. 1..5 K-tiles, reaches every path of the peeled loop: the steady
state of K-tile pairs runs while more than three K-tiles are left, then one, two or three tail
tiles follow — nk = 1, 2, 3 never enter the steady state, nk = 4 is one pair + a two-tile tail,
nk = 5 one pair + a three-tile tail.  M = 1 (every A row clamps to row 0), 200, 449 (at 192 rows
the last tile has 65 live rows); N = 256, 512.

The walk (gemm_pp_persist_kernel) under ACEHIP_GEMM_CUS, each case asserting its route first:
  (768, 512, 128, 2)    6 main tiles, 3 per workgroup (even), no tail
  (768, 512, 64, 2)     the same with a single K-tile (no B(1) in the early prologue)
  (1990, 512, 192, 7)   14 main + 4 tail tiles of 128 rows on 7 workgroups (uneven): a 128-row tail
                        tile is the last iteration of workgroups 0-3, the last ones ragged
  (1030, 768, 320, 3)   15 main tiles, 5 per workgroup; the last row tile has 6 live rows, so the
                        tile after it enters on the wait that leaves no store in flight
  (1286, 768, 256, 4)   15 main + 3 tail tiles on 4 workgroups (5, 5, 4, 4)

The head-post fused main + tail launch and one-launch grid, the fused store launch and two convs go
through the production dispatch.  The convs run the pointer form, which has no slot-immediate instantiation (gemm_plan.h
pp_tile_slotimm): their cases compare one kernel with itself and are kept so that a later switch of
that family is checked the day it is made.

Absolute check, one shape per epilogue at knob 1, against the fp32 torch product.  Tolerances are
those of tests/test_gpu_dit.py::test_gemm_variants for the epilogues it covers (store: rel-L2 <
5e-3 and atol 0.05 / rtol 0.02; SwiGLU: rel-L2 < 1e-2).  The residual epilogues round twice
(bf16(acc), then bf16(res + ·)) or three times (gated: the product too), each a relative error of
at most 2^-9 on a term no larger than the result's operands, so the store's rel-L2 bound of 5e-3
(2.5 × 2^-9) holds for them as well; a wrong K-tile would move the result by the size of acc
itself (rel-L2 ≈ 0.5 at these scales).
"""
import math
import os
import subprocess
import sys

import pytest
import torch

from conftest import rel_l2, set_knob

pytestmark = pytest.mark.gpu

EPI_STORE, EPI_GATED, EPI_RES, EPI_SWIGLU, EPI_HEADPOST = 0, 1, 2, 3, 4
GUARD = 3      # rows after row M that no launch may touch
OFF = 24       # elements: operands start 48 bytes into their allocations
KS = [64, 128, 192, 256, 320]
KNOB = "ACEHIP_GEMM_SLOTIMM"


def _lib():
    from acehip import _ffi
    return _ffi


def _nan_view(dev, rows, ld, off=0):
    """A [rows][ld] view `off` elements into a NaN-filled allocation (+ the allocation itself)."""
    buf = torch.full((rows * ld + off + 8,), float("nan"), device=dev, dtype=torch.bfloat16)
    return buf, buf[off:off + rows * ld].view(rows, ld)


def _operands(dev, M, N, K):
    g = torch.Generator(device="cpu").manual_seed(M * 7 + N + K)
    _, A = _nan_view(dev, M, K + 64, OFF)
    _, W = _nan_view(dev, N, K + 64, OFF)
    A[:, :K] = torch.randn(M, K, generator=g).to(dev, torch.bfloat16)
    W[:, :K] = (torch.randn(N, K, generator=g) * 0.05).to(dev, torch.bfloat16)
    R = torch.randn(M, N, generator=g).to(dev, torch.bfloat16)
    gate = torch.randn((M + 99) // 100, N, generator=g).to(dev, torch.bfloat16)
    return A, W, R, gate


def _bits(t):
    return t.view(torch.int16)


def _run_ex(ff, dev, A, W, R, M, N, K, epi, variant):
    """acehip_gemm_bf16_ex into a NaN-filled [M + GUARD][ncol + 8] buffer (the in-place residual
    epilogue starts from R in the live part) → (whole allocation, live part)."""
    ncol = N // 2 if epi == EPI_SWIGLU else N
    buf, C = _nan_view(dev, M + GUARD, ncol + 8)
    if epi == EPI_RES:
        C[:M, :N] = R
    ff.check(ff.lib().acehip_gemm_bf16_ex(ff.ptr(A), K + 64, ff.ptr(W), K + 64, ff.ptr(C), ncol + 8, M, N, K, None,
                                          epi, variant, ff.stream_ptr()))
    return buf, C[:M, :ncol]


def _run_gated(ff, dev, A, W, R, gate, M, N, K, variant):
    """acehip_gemm_res_bf16, gated, residual in a buffer of its own with ldr ≠ ldc."""
    buf, C = _nan_view(dev, M + GUARD, N + 16)
    _, Rv = _nan_view(dev, M, N + 8)
    Rv[:, :N] = R
    ff.check(ff.lib().acehip_gemm_res_bf16(ff.ptr(A), K + 64, ff.ptr(W), K + 64, ff.ptr(C), N + 16, M, N, K,
                                           ff.ptr(Rv), N + 8, ff.ptr(gate), N, 100, variant, ff.stream_ptr()))
    return buf, C[:M, :N]


def _assert_same(name, off, on):
    (obuf, olive), (nbuf, nlive) = off, on
    assert torch.isfinite(olive.float()).all(), name
    assert torch.equal(_bits(nbuf), _bits(obuf)), name
    # guard rows and pitch columns: still the fill (the live part is finite, so every NaN left is fill)
    assert int(torch.isnan(obuf.float()).sum()) == obuf.numel() - olive.numel(), name


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("N", [256, 512])
@pytest.mark.parametrize("M", [1, 200, 449])
def test_tile_variants_bit_identical(gpu_device, monkeypatch, M, N, K):
    ff = _lib()
    A, W, R, gate = _operands(gpu_device, M, N, K)
    out = {}
    for knob in (0, 1):
        set_knob(monkeypatch, KNOB, str(knob))
        for v in (7, 8, 9):
            for epi in (EPI_STORE, EPI_RES, EPI_SWIGLU):
                out[knob, v, epi] = _run_ex(ff, gpu_device, A, W, R, M, N, K, epi, v)
            out[knob, v, "gated"] = _run_gated(ff, gpu_device, A, W, R, gate, M, N, K, v)
    torch.cuda.synchronize()
    for (knob, v, epi), res in out.items():
        if knob == 1:
            _assert_same((v, epi), out[0, v, epi], res)


def test_against_fp32(gpu_device, monkeypatch):
    """Knob 1, M = 449, N = 512, K = 320 on the 192-row tile: every epilogue against the fp32 product
    (tolerances: module docstring)."""
    ff = _lib()
    M, N, K, v = 449, 512, 320, 8
    A, W, R, gate = _operands(gpu_device, M, N, K)
    set_knob(monkeypatch, KNOB, "1")
    acc = A[:, :K].float() @ W[:, :K].float().t()
    bf = lambda t: t.bfloat16().float()
    C = _run_ex(ff, gpu_device, A, W, R, M, N, K, EPI_STORE, v)[1].float()
    assert rel_l2(C.cpu(), acc.cpu()) < 5e-3
    assert torch.allclose(C, acc, atol=0.05, rtol=0.02)
    C = _run_ex(ff, gpu_device, A, W, R, M, N, K, EPI_RES, v)[1].float()
    assert rel_l2(C.cpu(), bf(R.float() + bf(acc)).cpu()) < 5e-3
    C = _run_gated(ff, gpu_device, A, W, R, gate, M, N, K, v)[1].float()
    grow = gate.float()[torch.arange(M, device=gpu_device) // 100]
    assert rel_l2(C.cpu(), bf(R.float() + bf(bf(acc) * grow)).cpu()) < 5e-3
    C = _run_ex(ff, gpu_device, A, W, R, M, N, K, EPI_SWIGLU, v)[1].float()
    y = bf(acc).view(M, N // 64, 2, 32)
    g_, u_ = y[:, :, 0, :].reshape(M, N // 2), y[:, :, 1, :].reshape(M, N // 2)
    assert rel_l2(C.cpu(), (bf(torch.nn.functional.silu(g_)) * u_).cpu()) < 1e-2


@pytest.mark.parametrize("K", KS)
def test_split_kernel_store_bit_identical(gpu_device, monkeypatch, K):
    ff = _lib()
    M, N = 1200, 1024
    A, W, R, _ = _operands(gpu_device, M, N, K)
    set_knob(monkeypatch, "ACEHIP_GEMM_CUS", "8")
    out = {}
    for knob in (0, 1):
        set_knob(monkeypatch, KNOB, str(knob))
        plan = ff.gemm_plan(M, N, K, EPI_STORE, lda=K + 64, ldw=K + 64)
        assert (plan["route"], plan["M1"], plan["nmain"], plan["ntail"], plan["saddr"]) == (ff.ROUTE_TAIL1, 1024, 16, 8, 1), plan
        out[knob] = _run_ex(ff, gpu_device, A, W, R, M, N, K, EPI_STORE, -1)
    torch.cuda.synchronize()
    _assert_same("split store", out[0], out[1])


@pytest.mark.parametrize("B,S,K", [(2, 4200, 128), (2, 4200, 320), (1, 4200, 256)])
def test_headpost_bit_identical(gpu_device, monkeypatch, B, S, K):
    """S = 4200, N = 2048 planned on 64 CUs.  B = 2 (M = 8400): 256 main + 16 tail blocks of one
    launch, the second row of tail tiles ragged, the batch boundary inside a main tile.  B = 1: the
    one-launch grid of 192-row tiles (22 × 8, the last row of tiles ragged), which runs the pointer
    form under knob 0 and the scalar base + slot immediates under knob 1."""
    ff = _lib()
    nq, nk, nv = 8, 4, 4
    M, N = B * S, (nq + nk + nv) * 128
    g = torch.Generator(device="cpu").manual_seed(S + K)
    _, A = _nan_view(gpu_device, M, K + 64, OFF)
    A[:, :K] = torch.randn(M, K, generator=g).to(gpu_device, torch.bfloat16)
    W = (torch.randn(N, K, generator=g) * 0.05).to(gpu_device, torch.bfloat16)   # the entry point takes ldw = K
    qw = (1 + 0.1 * torch.randn(128, generator=g)).to(gpu_device, torch.bfloat16)
    kw = (1 + 0.1 * torch.randn(128, generator=g)).to(gpu_device, torch.bfloat16)
    cos = torch.cos(torch.randn(S, 128, generator=g)).to(gpu_device, torch.bfloat16)
    sin = torch.sin(torch.randn(S, 128, generator=g)).to(gpu_device, torch.bfloat16)
    set_knob(monkeypatch, "ACEHIP_GEMM_CUS", "64")
    out = {}
    for knob in (0, 1):
        set_knob(monkeypatch, KNOB, str(knob))
        plan = ff.gemm_plan(M, N, K, EPI_HEADPOST, lda=K + 64, ldw=K)
        if B == 2:
            assert (plan["route"], plan["M1"], plan["nmain"], plan["ntail"], plan["saddr"]) == (ff.ROUTE_TAIL1, 8192, 256, 16, 1), plan
        else:
            assert (plan["route"], plan["v_head"], plan["grid"]) == (ff.ROUTE_TILE, 8, 176), plan
            assert ff.lib().acehip_diag_pp_slotimm(EPI_HEADPOST, 192, K + 64, K) == knob
        qkv = [torch.full((B * n * S + GUARD, 128), float("nan"), device=gpu_device, dtype=torch.bfloat16)
               for n in (nq, nk, nv)]
        ff.check(ff.lib().acehip_gemm_headpost_bf16(ff.ptr(A), K + 64, ff.ptr(W), K, B, S, nq, nk, nv, ff.ptr(qw),
                                                    ff.ptr(kw), ff.ptr(cos), ff.ptr(sin), 1e-6, ff.ptr(qkv[0]),
                                                    ff.ptr(qkv[1]), ff.ptr(qkv[2]), ff.stream_ptr()))
        out[knob] = qkv
    torch.cuda.synchronize()
    for off, on in zip(out[0], out[1]):
        assert torch.isfinite(off[:-GUARD].float()).all()
        assert torch.isnan(off[-GUARD:].float()).all()
        assert torch.equal(_bits(on), _bits(off))


# (kind, Cin, Cout, k, stride, dil, L, raw, res, snake)
CONVS = [
    (0, 1024, 1024, 7, 1, 3, 4200, False, False, True),  # k = 7, dilation 3, 128-row tiles
    (1, 512, 256, 8, 4, 1, 300, True, False, True),      # ConvTranspose: M = 301, N = 4 · 256, one phase per 256 columns
]


@pytest.mark.parametrize("kind,Cin,Cout,k,stride,dil,L,raw,use_res,use_snake", CONVS)
def test_convs_bit_identical(gpu_device, monkeypatch, kind, Cin, Cout, k, stride, dil, L, raw, use_res, use_snake):
    ff = _lib()
    bf = lambda t: t.to(torch.bfloat16)
    g = torch.Generator(device=gpu_device).manual_seed(Cin + Cout + k + dil + L)
    x = bf(torch.randn(L, Cin, device=gpu_device, generator=g))
    wshape = (Cin, Cout, k) if kind == 1 else (Cout, Cin, k)
    w = bf(torch.randn(wshape, device=gpu_device, generator=g) / math.sqrt(Cin * k))
    bias = bf(torch.randn(Cout, device=gpu_device, generator=g) * 0.1)
    L_out = L * stride if kind == 1 else L
    res = bf(torch.randn(L_out, Cout, device=gpu_device, generator=g)) if use_res else None
    alpha = bf(torch.randn(Cout, device=gpu_device, generator=g) * 0.3) if use_snake else None
    beta = bf(torch.randn(Cout, device=gpu_device, generator=g) * 0.3) if use_snake else None
    out = {}
    for knob in (0, 1):
        set_knob(monkeypatch, KNOB, str(knob))
        o = torch.full((L_out + GUARD, Cout), float("nan"), device=gpu_device, dtype=torch.bfloat16) if raw else None
        os_ = torch.full((L_out + GUARD, Cout), float("nan"), device=gpu_device, dtype=torch.bfloat16) if use_snake else None
        ff.check(ff.lib().acehip_vae_conv(kind, ff.ptr(x), L, Cin, ff.ptr(w), ff.ptr(bias), ff.ptr(res), Cout, k, stride,
                                          dil, ff.ptr(o), ff.ptr(alpha), ff.ptr(beta), ff.ptr(os_), ff.stream_ptr()))
        out[knob] = [t for t in (o, os_) if t is not None]
    torch.cuda.synchronize()
    for off, on in zip(out[0], out[1]):
        assert torch.isfinite(off[:L_out].float()).all()
        assert torch.isnan(off[L_out:].float()).all()
        assert torch.equal(_bits(on), _bits(off))


def _walk(M1, nmain, ntail, grid):
    return dict(route=5, M1=M1, nmain=nmain, ntail=ntail, grid=grid, saddr=1)   # ACEHIP_ROUTE_WALK


# (M, N, K, ACEHIP_GEMM_CUS) → the plan
WALKS = {(768, 512, 128, 2): _walk(768, 6, 0, 2), (768, 512, 64, 2): _walk(768, 6, 0, 2),
         (1990, 512, 192, 7): _walk(1792, 14, 4, 7), (1030, 768, 320, 3): _walk(1030, 15, 0, 3),
         (1286, 768, 256, 4): _walk(1280, 15, 3, 4)}


@pytest.mark.parametrize("M,N,K,cus", list(WALKS))
def test_walk_bit_identical(gpu_device, monkeypatch, M, N, K, cus):
    ff = _lib()
    A, W, R, _ = _operands(gpu_device, M, N, K)
    set_knob(monkeypatch, "ACEHIP_GEMM_CUS", str(cus))
    out = {}
    for knob in (0, 1):
        set_knob(monkeypatch, KNOB, str(knob))
        plan, want = ff.gemm_plan(M, N, K, EPI_SWIGLU, lda=K + 64, ldw=K + 64), WALKS[M, N, K, cus]
        assert {k: plan[k] for k in want} == want, plan
        out[knob] = _run_ex(ff, gpu_device, A, W, R, M, N, K, EPI_SWIGLU, -1)
    torch.cuda.synchronize()
    _assert_same("walk", out[0], out[1])
    # and against the one-tile-per-workgroup 256-row grid of the parent's loop
    set_knob(monkeypatch, KNOB, "0")
    ref = _run_ex(ff, gpu_device, A, W, R, M, N, K, EPI_SWIGLU, 7)
    torch.cuda.synchronize()
    assert torch.equal(_bits(ref[1]), _bits(out[1][1]))


_CHILD = r"""
import sys, torch
sys.path[:0] = [sys.argv[1], sys.argv[2]]
from acehip.config import DiTConfig
from acehip.dit import DiTRuntime
from acehip.weights import synth_dit_weights
dev = torch.device("cuda:0")
cfg = DiTConfig.tiny(layers=2, window=8)
W = {k: v.to(dev, torch.bfloat16) for k, v in synth_dit_weights(cfg, seed=5, mode="parity").items()}
g = torch.Generator().manual_seed(12)
rt = DiTRuntime(cfg, 0, max_S=1600, max_Bc=2, max_Lenc=24)
rt.load(W)
T = 3200
rt.set_condition(torch.randn(2, 24, cfg.hidden_size, generator=g).bfloat16().to(dev))
t = torch.tensor([0.5], dtype=torch.float32, device=dev)
outs = []
for graph in (False, True, True):
    xt = torch.randn(1, T, 64, generator=torch.Generator().manual_seed(3)).bfloat16().to(dev)
    ctx = torch.randn(1, T, 128, generator=torch.Generator().manual_seed(4)).bfloat16().to(dev)
    rt.use_graph(graph)
    outs.append(rt.forward(xt, ctx, t).clone().cpu())
    torch.cuda.synchronize()
rt.close()
torch.save(outs, sys.argv[3])
"""


def test_forward_bit_identical(gpu_device, tmp_path):
    """A two-layer forward, S = 1600 and two CFG rows planned on 3 CUs (the M = 3200 projections run
    on ping-pong tiles, the MLP's gate/up GEMM as a many-round walk), eager and graph-replayed
    twice, under knob 0 and knob 1 in a fresh process each: all six outputs byte-equal."""
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    pkg = os.path.join(repo, "ace-step-1.5_amd")
    procs = []
    for knob in ("0", "1"):
        dst = str(tmp_path / f"fwd_{knob}.pt")
        env = dict(os.environ, ACEHIP_GEMM_SLOTIMM=knob, ACEHIP_GEMM_CUS="3")
        procs.append((dst, subprocess.Popen([sys.executable, "-c", _CHILD, repo, pkg, dst], env=env, cwd=str(tmp_path),
                                            stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)))
    res = []
    for dst, p in procs:
        so, se = p.communicate(timeout=100)
        assert p.returncode == 0, (so[-2000:], se[-2000:])
        res.append(torch.load(dst))
    assert torch.isfinite(res[0][0].float()).all()
    for o in res[0][1:] + res[1]:
        assert torch.equal(_bits(o), _bits(res[0][0]))
