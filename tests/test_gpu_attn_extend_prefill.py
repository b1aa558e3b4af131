"""acehip_attention_extend_bf16 as a prefill: pos = 0, cap = n, every position a new query over
the head-post buffers q [B][H][n][128], k / v [B][KV][n][128] — the call the handle makes for a
heads / kv_heads = 4 stack (csrc/encoder.hip, the 4B LM), where tests/test_gpu_attn_extend.py
always leaves the cache's row stride larger than pos + n.

Reference and bar are that file's, restated: fp32 torch on the same bf16 inputs, rel-L2 < 1e-2 per
call, every output finite, and a query without an admissible key exactly zero.

n covers query blocks of 32 (G = 4) with a ragged last block, one, two and five 64-key tiles with a
ragged last tile, and ten query blocks whose waves skip the tiles past their own diagonal.  With
the left-padded mask row 1's first 9 keys are masked and their K / V rows hold NaN; that row's
first min(9, n) queries admit no key.

Each case runs at the default plan and with ACEHIP_ATTN_CUS=4, where every grid has at least as
many units as CUs and runs whole units; the plans seen must include a split and a one-part one."""
import math

import pytest
import torch

from conftest import rel_l2, set_knob

pytestmark = pytest.mark.gpu

SHAPES = [(2, 8, 2), (1, 32, 8)]
NS = [1, 31, 33, 64, 65, 300]
PAD = 9
SCALE = 1 / math.sqrt(128)
GUARD = 3


def _case(B, H, KV, n, masked, dev):
    g = torch.Generator().manual_seed(n * 7 + H * 1009 + B)
    G = H // KV
    q = torch.randn(B, H, n, 128, generator=g).bfloat16()
    k = torch.randn(B, KV, n, 128, generator=g).bfloat16()
    v = torch.randn(B, KV, n, 128, generator=g).bfloat16()
    mask = torch.ones(B, n, dtype=torch.uint8)
    if masked:
        mask[B - 1, :PAD] = 0                                # the last row (row 1 of a pair) is left-padded
    j = torch.arange(n)
    ok = mask.bool()[:, None, :] & (j[None, None, :] <= j[None, :, None])          # [B, n, n]
    s = torch.einsum("bhid,bhjd->bhij", q.float(), k.float().repeat_interleave(G, 1)) * SCALE
    s = s.masked_fill(~ok[:, None], float("-inf"))
    p = torch.nan_to_num(s.softmax(-1), nan=0.0)
    ref = torch.einsum("bhij,bhjd->bihd", p, v.float().repeat_interleave(G, 1)).reshape(B * n, H * 128)
    empty = ~ok.any(-1).reshape(B * n)
    bad = ~mask.bool()[:, None, :, None].expand(B, KV, n, 128)
    nan = torch.tensor(float("nan"), dtype=torch.bfloat16)
    k, v = torch.where(bad, nan, k), torch.where(bad, nan, v)
    return q.to(dev), k.to(dev), v.to(dev), (mask.to(dev) if masked else None), ref, empty


def _run(ff, q, k, v, mask, B, H, KV, n):
    dev = q.device
    nb = ff.lib().acehip_attention_extend_ws_bytes(B, H, n)
    ws = torch.full((nb // 4,), float("nan"), device=dev, dtype=torch.float32)
    o = torch.full((B * n + GUARD, H * 128), float("nan"), device=dev, dtype=torch.bfloat16)
    ff.check(ff.lib().acehip_attention_extend_bf16(ff.ptr(q), ff.ptr(k), ff.ptr(v), ff.ptr(o), B, H, KV, n, 0, n,
                                                   ff.ptr(mask), n if mask is not None else 0, SCALE, ff.ptr(ws),
                                                   nb, ff.stream_ptr()), "attention_extend")
    torch.cuda.synchronize()
    assert torch.isnan(o[B * n:].float()).all(), "rows past B·n were written"
    return o[:B * n]


def _check(o, ref, empty, what):
    o = o.float().cpu()
    assert torch.isfinite(o).all(), (what, "non-finite output")
    if empty.any():
        assert (o[empty] == 0).all(), (what, "a padded query's row is not zero")
    err = rel_l2(o, ref)
    assert err < 1e-2, (what, err)


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("B,H,KV", SHAPES)
def test_prefill_vs_fp32_both_plans(gpu_device, monkeypatch, B, H, KV, masked):
    from acehip import _ffi as ff
    cases = {n: _case(B, H, KV, n, masked, gpu_device) for n in NS}
    outs, parts = {}, {}
    for cus in (0, 4):
        if cus:
            set_knob(monkeypatch, "ACEHIP_ATTN_CUS", str(cus))
        for n in NS:
            q, k, v, mask, ref, empty = cases[n]
            assert bool(empty.any()) == masked and int(empty.sum()) == (min(PAD, n) if masked else 0)
            p = ff.attn_extend_plan(B, H, KV, n, 0)
            parts[cus, n] = p["parts"]
            if cus:
                assert p["units"] >= cus and p["parts"] == 1 and p["grid"] == p["units"], p
            a = _run(ff, q, k, v, mask, B, H, KV, n)
            b = _run(ff, q, k, v, mask, B, H, KV, n)
            assert torch.equal(a.view(torch.int16), b.view(torch.int16)), (cus, n, "not repeatable")
            _check(a, ref, empty, (cus, n))
            outs[cus, n] = a.float().cpu()
    # both kinds of plan were exercised, and they agree within the bar
    assert max(parts[0, n] for n in NS) > 1 and all(parts[4, n] == 1 for n in NS), parts
    for n in NS:
        err = rel_l2(outs[0, n], outs[4, n])
        assert err < 1e-2, (n, parts[0, n], err)
        empty = cases[n][5]
        assert (outs[0, n][empty] == 0).all() and (outs[4, n][empty] == 0).all()
