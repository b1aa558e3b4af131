"""The scalar-base K loop of the one-tile ping-pong GEMMs (ACEHIP_GEMM_SADDR=1: LDS-DMA sources as
the tile's scalar base + 32-bit lane offsets) against the pointer form it replaces (=0): the same
addresses (tests/test_gemm_saddr_host.py compares them on the CPU), so the same bits.

Every comparison is torch.equal on int16 views of the whole output allocation — the live result,
the columns between N and the pitch, and guard rows after row M, all pre-filled with NaN — so a
store or a source row that moved shows as a changed bit pattern.  A and W are 16-byte-aligned
views at a non-zero offset inside NaN-filled allocations with pitch K + 64.

Tile cases: M = 1 (every A row clamps to row 0), 200 (one ragged tile, or two 128-row tiles, the
second ragged), 449 (at 192 rows the last tile has 65 live rows: piece 1 partly clamped, piece 2
wholly); K = 64 (one K-tile: no B(1), the vmcnt(0) entry), 128 (two), 192 (odd count).

Split kernel (gemm_pp_split_kernel), reached through the production dispatch under ACEHIP_GEMM_CUS;
each case asserts its route before it launches (acehip_diag_gemm_plan; the same rows stand in
tests/test_gemm_plan_host.py):
  store, (1200, 1024, K ≤ 448, cap 8): one launch of 16 main + 8 tail blocks, M1 = 1024.
  head-post, B = 2, S = 600 (M = 1200, N = 1024): a small grid by the DEVICE's CU count, so 128²
      tiles + the standalone head_post kernel under either knob — compared, but it does not reach
      the split kernel.
  head-post, B = 2, S = 4200 (M = 8400, N = 2048, K = 128, cap 64): 256 main + 16 tail blocks
      (the second row of them ragged), M1 = 8192, the batch boundary (row 4200) inside a main tile.

Convs (EPI_CONV through acehip_vae_conv): M = L ≤ a few hundred runs on 64-row tiles
(gemm_conv: t256 · 4 ≤ CUs); k = 7 at C = 1024 with L = 4200 (68 tiles of 256 rows → 128-row
tiles) and L = 8300 (132 → 256-row tiles) reaches the other two heights, each with a ragged last
tile.

The conv epilogue and the one-launch head-post grid did not pass the round-8 timing rule and stay
on the pointer form under either knob value (gemm_plan.h pp_tile_saddr), so their cases here (and the
S = 600 head-post case, which runs 128² tiles) compare one kernel with itself; they are kept so
that a later switch of those families is checked the day it is made.
"""
import math

import pytest
import torch

from conftest import set_knob

from acehip.config import DiTConfig
from acehip.weights import synth_dit_weights

pytestmark = pytest.mark.gpu

EPI_STORE, EPI_RES, EPI_SWIGLU, EPI_HEADPOST = 0, 2, 3, 4
GUARD = 3      # rows after row M that no launch may touch
OFF = 24       # elements: operands start 48 bytes into their allocations


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


@pytest.mark.parametrize("K", [64, 128, 192])
@pytest.mark.parametrize("N", [256, 512])
@pytest.mark.parametrize("M", [1, 200, 449])
def test_tile_variants_bit_identical(gpu_device, monkeypatch, M, N, K):
    ff = _lib()
    A, W, R, gate = _operands(gpu_device, M, N, K)
    out = {}
    for knob in (0, 1):
        set_knob(monkeypatch, "ACEHIP_GEMM_SADDR", str(knob))
        for v in (7, 8, 9):
            for epi in (EPI_STORE, EPI_RES, EPI_SWIGLU):
                out[knob, v, epi] = _run_ex(ff, gpu_device, A, W, R, M, N, K, epi, v)
            out[knob, v, "gated"] = _run_gated(ff, gpu_device, A, W, R, gate, M, N, K, v)
    torch.cuda.synchronize()
    for (knob, v, epi), res in out.items():
        if knob == 1:
            _assert_same((v, epi), out[0, v, epi], res)


@pytest.mark.parametrize("K", [128, 192])
def test_split_kernel_store_bit_identical(gpu_device, monkeypatch, K):
    ff = _lib()
    M, N = 1200, 1024
    A, W, R, _ = _operands(gpu_device, M, N, K)
    set_knob(monkeypatch, "ACEHIP_GEMM_CUS", "8")
    out = {}
    for knob in (0, 1):
        set_knob(monkeypatch, "ACEHIP_GEMM_SADDR", str(knob))
        plan = ff.gemm_plan(M, N, K, EPI_STORE, lda=K + 64, ldw=K + 64)
        assert (plan["route"], plan["M1"], plan["nmain"], plan["ntail"], plan["saddr"]) == (ff.ROUTE_TAIL1, 1024, 16, 8, knob), plan
        out[knob] = _run_ex(ff, gpu_device, A, W, R, M, N, K, EPI_STORE, -1)
    torch.cuda.synchronize()
    _assert_same("split store", out[0], out[1])
    # and against the one-launch 192-row grid (variant 8), knob 0
    set_knob(monkeypatch, "ACEHIP_GEMM_SADDR", "0")
    ref = _run_ex(ff, gpu_device, A, W, R, M, N, K, EPI_STORE, 8)
    torch.cuda.synchronize()
    assert torch.equal(_bits(ref[1]), _bits(out[1][1]))


@pytest.mark.parametrize("B,S,nq,nk,nv,K,cus", [(2, 600, 4, 2, 2, 128, 8), (2, 4200, 8, 4, 4, 128, 64)])
def test_headpost_bit_identical(gpu_device, monkeypatch, B, S, nq, nk, nv, K, cus):
    ff = _lib()
    M, N = B * S, (nq + nk + nv) * 128
    g = torch.Generator(device="cpu").manual_seed(S + K)
    _, A = _nan_view(gpu_device, M, K + 64, OFF)
    A[:, :K] = torch.randn(M, K, generator=g).to(gpu_device, torch.bfloat16)
    W = (torch.randn(N, K, generator=g) * 0.05).to(gpu_device, torch.bfloat16)   # the entry point takes ldw = K
    qw = (1 + 0.1 * torch.randn(128, generator=g)).to(gpu_device, torch.bfloat16)
    kw = (1 + 0.1 * torch.randn(128, generator=g)).to(gpu_device, torch.bfloat16)
    cos = torch.cos(torch.randn(S, 128, generator=g)).to(gpu_device, torch.bfloat16)
    sin = torch.sin(torch.randn(S, 128, generator=g)).to(gpu_device, torch.bfloat16)
    set_knob(monkeypatch, "ACEHIP_GEMM_CUS", str(cus))
    out = {}
    for knob in (0, 1):
        set_knob(monkeypatch, "ACEHIP_GEMM_SADDR", str(knob))
        plan = ff.gemm_plan(M, N, K, EPI_HEADPOST, lda=K + 64, ldw=K)
        if S == 600:
            assert (plan["route"], plan["v_head"]) == (ff.ROUTE_STAGED, 0), plan
        else:
            assert (plan["route"], plan["M1"], plan["nmain"], plan["ntail"], plan["saddr"]) == (ff.ROUTE_TAIL1, 8192, 256, 16, knob), plan
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
    (0, 256, 256, 7, 1, 9, 333, False, False, True),     # k = 7, widest halo, 64-row tiles
    (1, 512, 256, 8, 4, 1, 300, True, False, True),      # ConvTranspose: M = 301, N = 4 · 256
    (0, 512, 512, 1, 1, 1, 333, True, True, True),       # k = 1 with the residual
    (0, 1024, 1024, 7, 1, 3, 4200, False, False, True),  # 128-row tiles
    (0, 1024, 1024, 7, 1, 1, 8300, False, False, True),  # 256-row tiles
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
        set_knob(monkeypatch, "ACEHIP_GEMM_SADDR", str(knob))
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


def test_forward_bit_identical(gpu_device, monkeypatch):
    """A two-layer forward, S = 1600 and two CFG rows planned on 3 CUs (the M = 3200 projections run
    on ping-pong tiles): knob 0 against knob 1, byte-equal."""
    from acehip.dit import DiTRuntime
    set_knob(monkeypatch, "ACEHIP_GEMM_CUS", "3")
    cfg = DiTConfig.tiny(layers=2, window=8)
    W = {k: v.to(gpu_device, torch.bfloat16) for k, v in synth_dit_weights(cfg, seed=5, mode="parity").items()}
    g = torch.Generator().manual_seed(12)
    rt = DiTRuntime(cfg, 0, max_S=1600, max_Bc=2, max_Lenc=24)
    rt.load(W)
    T = 3200
    rt.set_condition(torch.randn(2, 24, cfg.hidden_size, generator=g).bfloat16().to(gpu_device))
    t = torch.tensor([0.5], dtype=torch.float32, device=gpu_device)
    xt = torch.randn(1, T, 64, generator=g).bfloat16().to(gpu_device)
    ctx = torch.randn(1, T, 128, generator=g).bfloat16().to(gpu_device)
    outs = []
    for knob in (0, 1, 0):
        set_knob(monkeypatch, "ACEHIP_GEMM_SADDR", str(knob))
        outs.append(rt.forward(xt.clone(), ctx.clone(), t).clone())
        torch.cuda.synchronize()
    rt.close()
    assert torch.isfinite(outs[0].float()).all()
    assert torch.equal(_bits(outs[0]), _bits(outs[1])) and torch.equal(_bits(outs[0]), _bits(outs[2]))
