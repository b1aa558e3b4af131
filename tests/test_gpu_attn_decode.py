"""attn_decode (csrc/attn_decode.hip): one query per head over a K/V cache whose row stride
(cap) exceeds the valid length n, with and without a key mask, against fp32 torch on the same
bf16 inputs.  The bar is the attention kernels' (tests/test_gpu_dit.py): rel-L2 < 1e-2.

Cache rows at masked positions and rows [n, cap) hold NaN: they are excluded by selects, so
the output must be finite.  With 64-key parts (every n > 64 here splits) the masks cover a
whole part, and a row with a single admissible key, and rows of different padding."""
import math

import pytest
import torch

from conftest import rel_l2, set_knob

pytestmark = pytest.mark.gpu

CAP = 1024
NS = [1, 63, 64, 65, 129, 1000]
SHAPES = [(2, 2, 1), (2, 16, 8), (1, 32, 8), (3, 4, 4)]     # G = 2, 2, 4, 1
SCALE = 1 / math.sqrt(128)


def _pads(B, n):
    """Left padding per row: different lengths; row 1 keeps a single key (its padding covers every
    64-key part but the last); row 2 pads past the first part."""
    return [n // 3, n - 1, min(n - 1, 70)][:B]


def _case(B, H, KV, n, masked, dev, seed=0):
    g = torch.Generator().manual_seed(seed * 1000 + n * 7 + H)
    q = torch.randn(B, H, 128, generator=g).bfloat16()
    k = torch.randn(B, KV, CAP, 128, generator=g).bfloat16()
    v = torch.randn(B, KV, CAP, 128, generator=g).bfloat16()
    mask = torch.ones(B, CAP, dtype=torch.uint8)
    if masked:
        for b, p in enumerate(_pads(B, n)):
            mask[b, :p] = 0
    valid = mask.bool() & (torch.arange(CAP)[None, :] < n)                # [B, CAP]
    # reference: fp32 over the admissible keys only
    s = torch.einsum("bhd,bhjd->bhj", q.float(), k.float().repeat_interleave(H // KV, 1)) * SCALE
    s = s.masked_fill(~valid[:, None, :], float("-inf"))
    ref = torch.einsum("bhj,bhjd->bhd", s.softmax(-1), v.float().repeat_interleave(H // KV, 1)).reshape(B, H * 128)
    # poison what must never be read into the result
    bad = ~valid[:, None, :, None].expand(B, KV, CAP, 128)
    k = torch.where(bad, torch.tensor(float("nan"), dtype=torch.bfloat16), k)
    v = torch.where(bad, torch.tensor(float("nan"), dtype=torch.bfloat16), v)
    return q.to(dev), k.to(dev), v.to(dev), (mask.to(dev) if masked else None), ref


def _run(ff, q, k, v, mask, B, H, KV, n):
    dev = q.device
    nb = ff.lib().acehip_attention_decode_ws_bytes(B, H)
    ws = torch.full((nb // 4,), float("nan"), device=dev, dtype=torch.float32)
    o = torch.full((B, H * 128), float("nan"), device=dev, dtype=torch.bfloat16)
    ff.check(ff.lib().acehip_attention_decode_bf16(ff.ptr(q), ff.ptr(k), ff.ptr(v), ff.ptr(o), B, H, KV, n, CAP,
                                                   ff.ptr(mask), CAP if mask is not None else 0, SCALE, ff.ptr(ws),
                                                   nb, ff.stream_ptr()), "attention_decode")
    torch.cuda.synchronize()
    return o


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("B,H,KV", SHAPES)
def test_attn_decode_vs_fp32(gpu_device, B, H, KV, masked):
    from acehip import _ffi as ff
    for n in NS:
        q, k, v, mask, ref = _case(B, H, KV, n, masked, gpu_device)
        o = _run(ff, q, k, v, mask, B, H, KV, n).float().cpu()
        assert torch.isfinite(o).all(), (n, "non-finite output")
        err = rel_l2(o, ref)
        assert err < 1e-2, (n, err)


@pytest.mark.parametrize("cus", [0, 4, 24])
def test_attn_decode_repeatable(gpu_device, monkeypatch, cus):
    """Two calls on the same inputs are bit-equal, whatever the split count (the CU-count knob
    changes the number of key ranges); every split count meets the bar."""
    from acehip import _ffi as ff
    if cus:
        set_knob(monkeypatch, "ACEHIP_ATTN_CUS", str(cus))
    B, H, KV = 2, 16, 8
    for n in (129, 1000):
        q, k, v, mask, ref = _case(B, H, KV, n, True, gpu_device, seed=1)
        a = _run(ff, q, k, v, mask, B, H, KV, n)
        b = _run(ff, q, k, v, mask, B, H, KV, n)
        assert torch.equal(a.view(torch.int16), b.view(torch.int16)), (cus, n)
        assert torch.isfinite(a.float()).all()
        assert rel_l2(a.float().cpu(), ref) < 1e-2, (cus, n)


def test_attn_decode_without_workspace_and_bad_arguments(gpu_device):
    """No workspace: one key range per KV head, same bar.  G = 8 and n > cap are refused."""
    from acehip import _ffi as ff
    B, H, KV, n = 2, 16, 8, 129
    q, k, v, mask, ref = _case(B, H, KV, n, True, gpu_device, seed=2)
    o = torch.empty(B, H * 128, device=gpu_device, dtype=torch.bfloat16)
    ff.check(ff.lib().acehip_attention_decode_bf16(ff.ptr(q), ff.ptr(k), ff.ptr(v), ff.ptr(o), B, H, KV, n, CAP,
                                                   ff.ptr(mask), CAP, SCALE, None, 0, ff.stream_ptr()))
    torch.cuda.synchronize()
    assert rel_l2(o.float().cpu(), ref) < 1e-2
    fn = ff.lib().acehip_attention_decode_bf16
    assert fn(ff.ptr(q), ff.ptr(k), ff.ptr(v), ff.ptr(o), B, 16, 2, n, CAP, None, 0, SCALE, None, 0, ff.stream_ptr()) != 0
    assert fn(ff.ptr(q), ff.ptr(k), ff.ptr(v), ff.ptr(o), B, H, KV, CAP + 1, CAP, None, 0, SCALE, None, 0,
              ff.stream_ptr()) != 0
    assert fn(ff.ptr(q), ff.ptr(k), ff.ptr(v), ff.ptr(o), B, H, KV, n, CAP, ff.ptr(mask), n - 1, SCALE, None, 0,
              ff.stream_ptr()) != 0
