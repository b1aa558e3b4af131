"""attn_extend (csrc/attn_extend.hip): n new queries per sequence at cache positions
[pos, pos + n), causal over a K/V cache whose row stride (cap) exceeds pos + n, with and without a
key mask, against fp32 torch on the same bf16 inputs.  The bar is the attention kernels'
(tests/test_gpu_attn_decode.py): rel-L2 < 1e-2.

Cache rows at masked positions and rows [pos + n, cap) hold NaN, and the output and the partials
workspace start as NaN: the output must be finite.  pos x n put the diagonal inside, at and across
64-key tile edges, with ragged and multiple query blocks.  In the masked cases every row has its
own left padding, and row 0's ends inside the new tokens, so its first queries admit no key:
those output rows are exactly zero.  A second family of masks scatters zeros over the keys and
always masks the last cache position and one in the middle."""
import math

import pytest
import torch

from conftest import rel_l2, set_knob

pytestmark = pytest.mark.gpu

CAP = 384
SHAPES = [(2, 2, 1), (1, 16, 8), (1, 8, 2), (3, 4, 4)]     # G = 2, 2, 4, 1
POS = [0, 1, 63, 64, 130]
NEW = [1, 31, 64, 129, 200]
SCALE = 1 / math.sqrt(128)
GUARD = 3                                                  # sentinel rows of o past B·n


def _pads(B, pos, n):
    """Left padding per row: row 0's ends inside the new tokens (its first queries admit no key),
    the others differ."""
    return [min(max(pos + n // 2, 1), pos + n - 1), (pos + n) // 3, min(pos + n - 1, 70)][:B]


def _case(B, H, KV, n, pos, masked, dev, seed=0):
    g = torch.Generator().manual_seed(seed * 100003 + pos * 1009 + n * 7 + H)
    G = H // KV
    q = torch.randn(B, H, n, 128, generator=g).bfloat16()
    k = torch.randn(B, KV, CAP, 128, generator=g).bfloat16()
    v = torch.randn(B, KV, CAP, 128, generator=g).bfloat16()
    mask = torch.ones(B, CAP, dtype=torch.uint8)
    if masked == "scatter":
        # zeros anywhere, among them the last cache position pos + n − 1 (the row the kernel's
        # staging repeats past the valid range) and one in the middle
        mask[:, :pos + n] = (torch.rand(B, pos + n, generator=g) >= 0.3).to(torch.uint8)
        mask[:, pos + n - 1] = 0
        mask[:, (pos + n) // 2] = 0
    elif masked:
        for b, p in enumerate(_pads(B, pos, n)):
            mask[b, :p] = 0
    j = torch.arange(CAP)
    live = mask.bool() & (j[None, :] < pos + n)                                     # [B, CAP]
    ok = live[:, None, :] & (j[None, None, :] <= pos + torch.arange(n)[None, :, None])   # [B, n, CAP]
    s = torch.einsum("bhid,bhjd->bhij", q.float(), k.float().repeat_interleave(G, 1)) * SCALE
    s = s.masked_fill(~ok[:, None], float("-inf"))
    p = torch.nan_to_num(s.softmax(-1), nan=0.0)             # a query with no admissible key: zeros
    ref = torch.einsum("bhij,bhjd->bihd", p, v.float().repeat_interleave(G, 1)).reshape(B * n, H * 128)
    empty = ~ok.any(-1).reshape(B * n)                       # rows that must be exactly zero
    bad = ~live[:, None, :, None].expand(B, KV, CAP, 128)
    nan = torch.tensor(float("nan"), dtype=torch.bfloat16)
    k, v = torch.where(bad, nan, k), torch.where(bad, nan, v)
    return q.to(dev), k.to(dev), v.to(dev), (mask.to(dev) if masked else None), ref, empty


def _run(ff, q, k, v, mask, B, H, KV, n, pos, with_ws=True):
    dev = q.device
    nb = ff.lib().acehip_attention_extend_ws_bytes(B, H, n) if with_ws else 0
    ws = torch.full((nb // 4,), float("nan"), device=dev, dtype=torch.float32) if with_ws else None
    o = torch.full((B * n + GUARD, H * 128), float("nan"), device=dev, dtype=torch.bfloat16)
    ff.check(ff.lib().acehip_attention_extend_bf16(ff.ptr(q), ff.ptr(k), ff.ptr(v), ff.ptr(o), B, H, KV, n, pos, CAP,
                                                   ff.ptr(mask), CAP if mask is not None else 0, SCALE, ff.ptr(ws),
                                                   nb, ff.stream_ptr()), "attention_extend")
    torch.cuda.synchronize()
    assert torch.isnan(o[B * n:].float()).all(), "rows past B·n were written"
    return o[:B * n]


def _check(o, ref, empty, what):
    o = o.float().cpu()
    assert torch.isfinite(o).all(), (what, "non-finite output")
    if empty.any():
        assert (o[empty] == 0).all(), (what, "a query without an admissible key is not zero")
    err = rel_l2(o, ref)
    assert err < 1e-2, (what, err)


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("B,H,KV", SHAPES)
def test_attn_extend_vs_fp32(gpu_device, B, H, KV, masked):
    from acehip import _ffi as ff
    seen_empty = False
    for pos in POS:
        for n in NEW:
            q, k, v, mask, ref, empty = _case(B, H, KV, n, pos, masked, gpu_device)
            seen_empty |= bool(empty.any())
            _check(_run(ff, q, k, v, mask, B, H, KV, n, pos), ref, empty, (pos, n))
    assert seen_empty == masked


@pytest.mark.parametrize("B,H,KV", SHAPES)
def test_attn_extend_scattered_mask(gpu_device, B, H, KV):
    """Masked keys inside otherwise admitted tiles and at the last cache position, all holding
    NaN: every element's mask bit and the V rows of the ragged last tile are on the line.  The
    last query then never admits its own key, and a query all of whose keys are masked is zero."""
    from acehip import _ffi as ff
    seen_empty = False
    for pos in POS:
        for n in NEW:
            q, k, v, mask, ref, empty = _case(B, H, KV, n, pos, "scatter", gpu_device, seed=3)
            assert not mask[:, pos + n - 1].any() and bool(torch.isnan(v[:, :, pos + n - 1].float()).all())
            seen_empty |= bool(empty.any())
            _check(_run(ff, q, k, v, mask, B, H, KV, n, pos), ref, empty, (pos, n))
            if (pos, n) in ((130, 200), (63, 31)):
                _check(_run(ff, q, k, v, mask, B, H, KV, n, pos, with_ws=False), ref, empty, (pos, n, "no ws"))
    assert seen_empty


REPEAT = [(130, 200), (200, 31), (1, 129)]


@pytest.mark.parametrize("cus", [0, 4, 24])
def test_attn_extend_repeatable(gpu_device, monkeypatch, cus):
    """Two calls on the same inputs are bit-equal at every split count (the CU-count knob changes
    the number of key ranges), and every split count meets the bar."""
    from acehip import _ffi as ff
    if cus:
        set_knob(monkeypatch, "ACEHIP_ATTN_CUS", str(cus))
    B, H, KV = 1, 16, 8
    for pos, n in REPEAT:
        q, k, v, mask, ref, empty = _case(B, H, KV, n, pos, True, gpu_device, seed=1)
        a = _run(ff, q, k, v, mask, B, H, KV, n, pos)
        b = _run(ff, q, k, v, mask, B, H, KV, n, pos)
        assert torch.equal(a.view(torch.int16), b.view(torch.int16)), (cus, pos, n)
        _check(a, ref, empty, (cus, pos, n))


def test_attn_extend_tested_plans_split_and_whole(gpu_device, monkeypatch):
    """The shapes of the repeatability test run both ways: a split plan and a one-part plan."""
    from acehip import _ffi as ff
    parts = set()
    for cus in (0, 4, 24):
        if cus:
            set_knob(monkeypatch, "ACEHIP_ATTN_CUS", str(cus))
        for pos, n in REPEAT:
            p = ff.attn_extend_plan(1, 16, 8, n, pos)
            assert (p["parts"] - 1) * p["tiles_per_part"] < p["tiles"] <= p["parts"] * p["tiles_per_part"]
            parts.add(p["parts"])
    assert 1 in parts and max(parts) > 1, parts


def test_attn_extend_without_workspace_and_bad_arguments(gpu_device):
    """No workspace: one key range per unit, same bar.  Refused calls leave the output untouched."""
    from acehip import _ffi as ff
    B, H, KV, pos, n = 1, 16, 8, 130, 200
    q, k, v, mask, ref, empty = _case(B, H, KV, n, pos, True, gpu_device, seed=2)
    _check(_run(ff, q, k, v, mask, B, H, KV, n, pos, with_ws=False), ref, empty, "no workspace")

    fn = ff.lib().acehip_attention_extend_bf16
    nb = ff.lib().acehip_attention_extend_ws_bytes(B, H, n)
    ws = torch.empty(nb, device=gpu_device, dtype=torch.uint8)
    o = torch.full((B * n, H * 128), float("nan"), device=gpu_device, dtype=torch.bfloat16)
    P, sp = ff.ptr, ff.stream_ptr()
    need = ff.attn_extend_plan(B, H, KV, n, pos)["ws_need"]
    assert need > 16, "the short-workspace case needs a split plan"
    bad = [
        ("G = 8", (P(q), P(k), P(v), P(o), B, 16, 2, n, pos, CAP, None, 0, SCALE, P(ws), nb, sp)),
        ("pos + n > cap", (P(q), P(k), P(v), P(o), B, H, KV, n, CAP - n + 1, CAP, None, 0, SCALE, P(ws), nb, sp)),
        ("mask_ld < pos + n", (P(q), P(k), P(v), P(o), B, H, KV, n, pos, CAP, P(mask), pos + n - 1, SCALE, P(ws), nb, sp)),
        ("short workspace", (P(q), P(k), P(v), P(o), B, H, KV, n, pos, CAP, None, 0, SCALE, P(ws), need - 16, sp)),
        ("null q", (None, P(k), P(v), P(o), B, H, KV, n, pos, CAP, None, 0, SCALE, P(ws), nb, sp)),
        ("null k", (P(q), None, P(v), P(o), B, H, KV, n, pos, CAP, None, 0, SCALE, P(ws), nb, sp)),
        ("null v", (P(q), P(k), None, P(o), B, H, KV, n, pos, CAP, None, 0, SCALE, P(ws), nb, sp)),
        ("n = 0", (P(q), P(k), P(v), P(o), B, H, KV, 0, pos, CAP, None, 0, SCALE, P(ws), nb, sp)),
        ("pos < 0", (P(q), P(k), P(v), P(o), B, H, KV, n, -1, CAP, None, 0, SCALE, P(ws), nb, sp)),
    ]
    for what, args in bad:
        assert fn(*args) == -1, what
    assert fn(P(q), P(k), P(v), None, B, H, KV, n, pos, CAP, None, 0, SCALE, P(ws), nb, sp) == -1, "null o"
    torch.cuda.synchronize()
    assert torch.isnan(o.float()).all(), "a refused call wrote the output"
