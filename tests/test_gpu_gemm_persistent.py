"""The persistent SwiGLU tile walk (gemm_pp_persist_kernel, ACEHIP_GEMM_PERSIST) against the
one-tile-per-workgroup launch it replaces: the same bits, because no element's K order changes.

ACEHIP_GEMM_CUS caps the CU count the tile planner fills, so small shapes plan multi-round grids.
Every launch first asserts its route (acehip_diag_gemm_plan; tests/test_gemm_plan_host.py holds the
same rows on the CPU): with the knob on, the walk the case is there for — or, for the four cases
that plan 192-row or 128×128 tiles, the one grid they take under either knob value; with the knob
off, anything but the walk.

  (768, 512, 128, 2)    6 main tiles, 3 per workgroup, no tail
  (768, 512, 64, 2)     the same walk with a single K-tile: the prologue holds no B(1), so every
                        boundary takes the wait that leaves only the epilogue's stores in flight
  (1990, 512, 192, 7)   tail split: 14 main tiles + 198 tail rows as 4 tiles of 128×256, the last
                        ones ragged; 18 tiles on 7 workgroups: main, main, tail for workgroups 0–3;
                        3 K-tiles (odd)
  (1030, 768, 256, 4)   15 main tiles on 4 workgroups (4, 4, 4, 3), no tail; the last row tile has
                        6 live rows and is followed by another tile in its workgroups' walks
  (1286, 768, 128, 4)   tail split with a 6-row tail (3 tiles of 128×256): 18 tiles on 4
                        workgroups, three of which end on a tail tile
"""
import pytest
import torch

from conftest import rel_l2, set_knob

from acehip.config import DiTConfig
from acehip.weights import synth_dit_weights

pytestmark = pytest.mark.gpu

EPI_SWIGLU = 3



def _walk(M1, nmain, ntail, grid):
    return dict(route=5, M1=M1, nmain=nmain, ntail=ntail, grid=grid)   # ACEHIP_ROUTE_WALK


def _tile(v):
    return dict(route=0, v_head=v)   # ACEHIP_ROUTE_TILE


# (M, N, K, ACEHIP_GEMM_CUS) → the plan with the walk on
WANT = {(768, 512, 128, 2): _walk(768, 6, 0, 2), (700, 512, 192, 4): _tile(8), (520, 768, 64, 2): _tile(8),
        (1030, 512, 256, 3): _tile(8), (300, 512, 128, 8): _tile(0), (768, 512, 64, 2): _walk(768, 6, 0, 2),
        (1990, 512, 192, 7): _walk(1792, 14, 4, 7), (1030, 768, 256, 4): _walk(1030, 15, 0, 4),
        (1286, 768, 128, 4): _walk(1280, 15, 3, 4)}
CASES = list(WANT)


def _lib():
    from acehip import _ffi
    return _ffi


def _inputs(gpu_device, M, N, K):
    g = torch.Generator(device="cpu").manual_seed(M * 3 + N + K)
    A = torch.randn(M, K, generator=g).to(gpu_device, torch.bfloat16)
    # rows packed per 64-row panel as [32 gate ; 32 up]
    W = (torch.randn(N, K, generator=g) * 0.05).to(gpu_device, torch.bfloat16)
    return A, W


def _swiglu(ff, gpu_device, monkeypatch, A, W, persist, cus):
    M, K = A.shape
    N = W.shape[0]
    set_knob(monkeypatch, "ACEHIP_GEMM_CUS", str(cus))
    set_knob(monkeypatch, "ACEHIP_GEMM_PERSIST", "1" if persist else "0")
    plan, want = ff.gemm_plan(M, N, K, EPI_SWIGLU), WANT[M, N, K, cus]
    if persist:
        assert {k: plan[k] for k in want} == want, plan
    else:
        assert plan["route"] != ff.ROUTE_WALK, plan
    C = torch.full((M, N // 2), float("nan"), device=gpu_device, dtype=torch.bfloat16)
    ff.check(ff.lib().acehip_gemm_bf16_ex(ff.ptr(A), K, ff.ptr(W), K, ff.ptr(C), N // 2, M, N, K, None,
                                          EPI_SWIGLU, -1, ff.stream_ptr()))
    torch.cuda.synchronize()
    return C


@pytest.mark.parametrize("M,N,K,cus", CASES)
def test_persistent_walk_bit_identical(gpu_device, monkeypatch, M, N, K, cus):
    ff = _lib()
    A, W = _inputs(gpu_device, M, N, K)
    off = _swiglu(ff, gpu_device, monkeypatch, A, W, False, cus)
    on = _swiglu(ff, gpu_device, monkeypatch, A, W, True, cus)
    assert torch.isfinite(off.float()).all()
    assert torch.equal(on.view(torch.int16), off.view(torch.int16))
    # a second launch over its own output buffer: nothing is kept between launches
    again = _swiglu(ff, gpu_device, monkeypatch, A, W, True, cus)
    assert torch.equal(again.view(torch.int16), off.view(torch.int16))


def test_persistent_walk_vs_fp32(gpu_device, monkeypatch):
    """The cap-2 walk against the fp32 torch product, at the SwiGLU tolerance of
    test_gpu_dit.py::test_gemm_variants (rel-L2 < 1e-2)."""
    ff = _lib()
    M, N, K, cus = CASES[0]
    A, W = _inputs(gpu_device, M, N, K)
    on = _swiglu(ff, gpu_device, monkeypatch, A, W, True, cus)
    y = (A.float() @ W.float().t()).bfloat16().float().view(M, N // 64, 2, 32)
    gate, up = y[:, :, 0, :].reshape(M, N // 2), y[:, :, 1, :].reshape(M, N // 2)
    ref = torch.nn.functional.silu(gate).bfloat16().float() * up
    assert rel_l2(on.float().cpu(), ref.cpu()) < 1e-2


def test_graph_replay_persistent_swiglu(gpu_device, monkeypatch):
    """A two-layer forward captured once with the walk on and replayed twice equals the eager
    result (the kernel keeps no state between launches).  S = 1600, two CFG rows: the MLP's
    gate/up GEMM is M = 3200, N = 2·intermediate, planned on 3 CUs so its grid is many rounds."""
    from acehip.dit import DiTRuntime
    set_knob(monkeypatch, "ACEHIP_GEMM_CUS", "3")
    set_knob(monkeypatch, "ACEHIP_GEMM_PERSIST", "1")
    cfg = DiTConfig.tiny(layers=2, window=8)
    W = {k: v.to(gpu_device, torch.bfloat16) for k, v in synth_dit_weights(cfg, seed=5, mode="parity").items()}
    g = torch.Generator().manual_seed(12)
    rt = DiTRuntime(cfg, 0, max_S=1600, max_Bc=2, max_Lenc=24)
    rt.load(W)
    T = 3200
    enc = torch.randn(2, 24, cfg.hidden_size, generator=g).bfloat16().to(gpu_device)
    rt.set_condition(enc)
    t = torch.tensor([0.5], dtype=torch.float32, device=gpu_device)
    outs = []
    for graph in (False, True, True, True):
        xt = torch.randn(1, T, 64, generator=torch.Generator().manual_seed(3)).bfloat16().to(gpu_device)
        ctx = torch.randn(1, T, 128, generator=torch.Generator().manual_seed(4)).bfloat16().to(gpu_device)
        rt.use_graph(graph)
        outs.append(rt.forward(xt, ctx, t).clone())
        torch.cuda.synchronize()
    rt.close()
    assert torch.isfinite(outs[0].float()).all()
    for o in outs[1:]:
        assert torch.equal(outs[0], o)
