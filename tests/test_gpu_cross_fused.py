"""The fused cross-Q projection + cross-attention launch (cross_q_attn_kernel, ACEHIP_CROSS_FUSE)
against the two launches it replaces, bit for bit.

Kernel level, through acehip_cross_attn_bf16 with the path forced (force = 1: fused wherever the
kernel can run the shape; force = 0: gemm_w4_kernel<192, 128, head-post> + whole units on
attn_fwd_kernel<2>, whatever the CU count).  D = K = 256 (4 K-tiles: deeper than the projection's
3-slot operand ring), H = 4, KV = 2 (N = 512: the head pairs (0, 1) and (2, 3) share a KV head).
  S = 192  exactly one 192-row tile;  S = 200  a second tile with 8 live rows (five of its six waves
  hold only rows past M);  S = 416  three tiles, the last with a 32-row remainder.
  Lenc = 1  a single key;  64  exactly one K/V tile;  65  one tile + one key (the masked tail the
  240 s song's 641 keys also end in);  641  eleven tiles.
Both paths share every query row's instruction sequence (csrc/attn_tile.h) and the bf16 Q values
are the same through HBM or LDS, so the assertion is torch.equal on the bits of AO — no tolerance.

Forward level: the tiny DiT, S = 192 with both CFG rows conditional (two batch-aligned row tiles),
planned on 4 CUs so that the projection takes the four-wave tile and the attention whole units;
ACEHIP_CROSS_FUSE = 0 and 1 run in fresh child processes, the outputs must be byte-equal, and each
child reports the path the forward's rule took and the route gemm() itself plans for that shape.
"""
import math
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

D, H, KV = 256, 4, 2
EPS = 1e-6
SCALE = 1.0 / math.sqrt(128.0)
GUARD = 4   # AO rows after row B·S that no launch may touch


def _ff():
    from acehip import _ffi
    return _ffi


def _bits(t):
    return t.view(torch.int16)


_inputs = {}


def _make(dev, B, S, Lenc):
    """Fixed-seed bf16 inputs of one shape (made once, shared by the tests, never written)."""
    key = (B, S, Lenc)
    if key not in _inputs:
        g = torch.Generator().manual_seed(1000 * B + 10 * S + Lenc)
        xn = torch.randn(B * S, D, generator=g).bfloat16().to(dev)
        wq = (torch.randn(H * 128, D, generator=g) * 0.05).bfloat16().to(dev)
        qnw = (1.0 + 0.1 * torch.randn(128, generator=g)).bfloat16().to(dev)
        k = torch.randn(B, KV, Lenc, 128, generator=g).bfloat16().to(dev)
        v = torch.randn(B, KV, Lenc, 128, generator=g).bfloat16().to(dev)
        _inputs[key] = (xn, wq, qnw, k, v)
    return _inputs[key]


def _run(dev, B, S, Lenc, force):
    """One acehip_cross_attn_bf16 call into a NaN-filled [B·S + GUARD][H·128] buffer → (live AO
    rows, guard rows, path that ran)."""
    import ctypes
    ff = _ff()
    xn, wq, qnw, k, v = _make(dev, B, S, Lenc)
    ao = torch.full((B * S + GUARD, H * 128), float("nan"), device=dev, dtype=torch.bfloat16)
    path = ctypes.c_int(-7)
    ff.check(ff.lib().acehip_cross_attn_bf16(ff.ptr(xn), ff.ptr(wq), ff.ptr(qnw), ff.ptr(k), ff.ptr(v), ff.ptr(ao),
                                             B, S, H, KV, Lenc, D, EPS, SCALE, force, ctypes.byref(path),
                                             ff.stream_ptr()))
    torch.cuda.synchronize()
    return ao[:B * S], ao[B * S:], path.value


_unfused = {}


def _reference(dev, B, S, Lenc):
    """The forced two-launch result of one shape, computed once."""
    key = (B, S, Lenc)
    if key not in _unfused:
        ao, guard, path = _run(dev, B, S, Lenc, 0)
        assert path == 0
        assert torch.isnan(guard.float()).all()
        assert torch.isfinite(ao.float()).all()
        _unfused[key] = ao.clone()
    return _unfused[key]


def _check_fused(dev, B, S, Lenc):
    ref = _reference(dev, B, S, Lenc)
    ao, guard, path = _run(dev, B, S, Lenc, 1)
    assert path == 1, "the fused launch must run this shape"
    assert torch.isnan(guard.float()).all(), "rows past M were stored"
    assert torch.isfinite(ao.float()).all()
    assert torch.equal(_bits(ao), _bits(ref))


@pytest.mark.parametrize("Lenc", [1, 64, 65, 641])
@pytest.mark.parametrize("S", [192, 200, 416])
def test_fused_bit_identical(gpu_device, S, Lenc):
    _check_fused(gpu_device, 1, S, Lenc)


def test_two_launch_path_matches_float_reference(gpu_device):
    """The reference the other tests compare with is itself the cross-attention: against fp32 torch
    on the same bf16 inputs.  Bound: Q, P and O are each rounded to bf16 once (relative 2^-9 per
    element), ≤ 3 · 2^-9 ≈ 0.6 % in the worst case — 2 % asserts a wiring error, not a rounding."""
    B, S, Lenc = 1, 200, 65
    xn, wq, qnw, k, v = (t.float() for t in _make(gpu_device, B, S, Lenc))
    q = (xn @ wq.T).bfloat16().float().view(B, S, H, 128)
    q = (q * torch.rsqrt(q.pow(2).mean(-1, keepdim=True) + EPS)).bfloat16().float() * qnw
    q = q.bfloat16().float().permute(0, 2, 1, 3)                       # [B, H, S, 128]
    kk, vv = k.repeat_interleave(H // KV, 1), v.repeat_interleave(H // KV, 1)
    p = torch.softmax(q @ kk.transpose(-1, -2) * SCALE, -1)
    want = (p @ vv).permute(0, 2, 1, 3).reshape(B * S, H * 128)
    got = _reference(gpu_device, B, S, Lenc).float()
    rel = float((got - want).norm() / want.norm())
    print(f"two-launch cross-attention vs fp32 torch: rel-L2 {rel:.5f}")
    assert rel < 0.02


def test_batch_aligned_tiles(gpu_device):
    """B = 2, S = 192: each row tile is one batch element with its own K/V."""
    _check_fused(gpu_device, 2, 192, 65)


def test_batch_straddling_tile_is_not_fused(gpu_device):
    """B = 2, S = 200: the second row tile would hold rows of both batch elements — two launches,
    even when the fused path is asked for."""
    ao, guard, path = _run(gpu_device, 2, 200, 65, 1)
    assert path == 0
    assert torch.isnan(guard.float()).all()
    assert torch.isfinite(ao.float()).all()


def test_alternating_rounds(gpu_device):
    """fused / two launches × 3 at one shape: no state, LDS image or scratch survives a launch."""
    B, S, Lenc = 1, 416, 641
    ref = _reference(gpu_device, B, S, Lenc)
    for _ in range(3):
        for force in (1, 0):
            ao, guard, path = _run(gpu_device, B, S, Lenc, force)
            assert path == force
            assert torch.isnan(guard.float()).all()
            assert torch.equal(_bits(ao), _bits(ref))


_CHILD = r"""
import ctypes, sys, torch
sys.path[:0] = [sys.argv[1], sys.argv[2]]
from acehip import _ffi as ff
from acehip.config import DiTConfig
from acehip.dit import DiTRuntime
from acehip.weights import synth_dit_weights
dev = torch.device("cuda:0")
cfg = DiTConfig.tiny(layers=2, window=8)
W = {k: v.to(dev, torch.bfloat16) for k, v in synth_dit_weights(cfg, seed=5, mode="parity").items()}
g = torch.Generator().manual_seed(12)
S, Lenc = 192, 70
rt = DiTRuntime(cfg, 0, max_S=S, max_Bc=2, max_Lenc=Lenc)
rt.load(W)
rt.set_condition(torch.randn(2, Lenc, cfg.hidden_size, generator=g).bfloat16().to(dev))
t = torch.tensor([0.5], dtype=torch.float32, device=dev)
xt = torch.randn(1, 2 * S, 64, generator=g).bfloat16().to(dev)
ctx = torch.randn(1, 2 * S, 128, generator=g).bfloat16().to(dev)
out = rt.forward(xt, ctx, t).clone()
torch.cuda.synchronize()
rt.close()
# which path the forward's own rule takes for its cross-attention shape under this environment
Hh, KVh, Dm = cfg.num_attention_heads, cfg.num_key_value_heads, cfg.hidden_size
z = lambda *s: torch.zeros(*s, device=dev, dtype=torch.bfloat16)
path = ctypes.c_int(-7)
ff.check(ff.lib().acehip_cross_attn_bf16(ff.ptr(z(2 * S, Dm)), ff.ptr(z(Hh * 128, Dm)), ff.ptr(z(128)),
                                         ff.ptr(z(2, KVh, Lenc, 128)), ff.ptr(z(2, KVh, Lenc, 128)),
                                         ff.ptr(z(2 * S, Hh * 128)), 2, S, Hh, KVh, Lenc, Dm, 1e-6, 0.088, -1,
                                         ctypes.byref(path), ff.stream_ptr()))
torch.cuda.synchronize()
# gemm()'s own route for the projection under the same environment (acehip_diag_gemm_plan)
plan = ff.gemm_plan(2 * S, Hh * 128, Dm, 4)
# and attention()'s for the cross-attention (acehip_diag_attn_plan)
attn_plan = ff.attn_plan(2, Hh, KVh, S, Lenc)
torch.save({"out": out.cpu(), "path": path.value, "plan": plan, "attn_plan": attn_plan}, sys.argv[3])
"""


def test_forward_knob_bit_equal(gpu_device, tmp_path):
    """The tiny DiT's forward under ACEHIP_CROSS_FUSE = 0 and 1, each in a fresh process.  M = 2 · 192
    rows × N = 256: 2 × 2 four-wave tiles fill the 4 planned CUs (ACEHIP_GEMM_CUS), and the
    attention's 4 GQA-pair units run whole on attn_fwd_kernel<2> (ACEHIP_ATTN_CUS = 4: 24 one-head
    units > 1.5 · 4, so not attn_small_kernel).  The four-wave tile is cross_fuse_planned's choice
    (planned CUs throughout), which the forward follows in both arms; gemm() itself judges a
    half-chip grid by the device's CUs and plans this small grid as 128² tiles + head_post."""
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    pkg = os.path.join(repo, "ace-step-1.5_amd")
    res = []
    for knob in ("0", "1"):
        dst = str(tmp_path / f"fwd_{knob}.pt")
        env = dict(os.environ, ACEHIP_CROSS_FUSE=knob, ACEHIP_GEMM_CUS="4", ACEHIP_ATTN_CUS="4")
        p = subprocess.run([sys.executable, "-c", _CHILD, repo, pkg, dst], env=env, cwd=str(tmp_path),
                           capture_output=True, text=True, timeout=100)
        assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-2000:])
        res.append(torch.load(dst))
    assert res[0]["path"] == 0 and res[1]["path"] == 1, "the knob must switch the forward's cross path"
    for r in res:
        assert (r["plan"]["route"], r["plan"]["v_head"]) == (_ff().ROUTE_STAGED, 0), r["plan"]
        ap = r["attn_plan"]
        assert (ap["kernel"], ap["nrep"], ap["units"], ap["nsplit"], ap["streamk"], ap["grid"]) == \
            (_ff().ATTN_FWD, 2, 4, 1, 0, 4), ap
    assert torch.isfinite(res[0]["out"].float()).all()
    assert torch.equal(_bits(res[0]["out"]), _bits(res[1]["out"]))
