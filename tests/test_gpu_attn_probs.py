"""``acehip_attention_probs_bf16`` (attn_probs.hip) — the selected-head softmax rows behind the
lyric-alignment capture — against fp32 torch ``softmax(scale · q·kᵀ)`` over all keys on the
same bf16 q / k, transposed to [key, query] and cut to [k0, k1).

Bar: every element within 2⁻⁸ relative + 1e-7 absolute: one bf16 rounding of the stored value
(half an ulp of an 8-bit significand: at most 2⁻⁸/(1 + 2⁻⁸) of the value) plus the exp error;
both sides see identical inputs.  Memory right after ``out`` (a canary) must stay untouched.
"""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

REL, ABS = 2.0 ** -8, 1e-7
CANARY = -77.25

# (B, H, KV, Sq, Sk, heads, k0, k1, q_gain)
SHAPES = [
    pytest.param((1, 2, 1, 1, 13, [1], 0, 13, 1.0), id="one_query_subtile_keys"),
    pytest.param((2, 16, 8, 125, 77, [3, 10, 15], 5, 61, 1.0), id="gqa_ragged_two_rows"),
    pytest.param((1, 16, 8, 300, 200, [0, 7], 31, 97, 1.0), id="q_blocks_tail_unaligned_range"),
    pytest.param((1, 16, 8, 160, 700, [9], 0, 700, 1.0), id="long_key_loop"),
    pytest.param((1, 4, 2, 64, 64, [2], 63, 64, 1.0), id="one_key_at_tile_edge"),
    pytest.param((1, 4, 2, 70, 90, [3, 0], 0, 90, 40.0), id="logits_pm40"),
]


def _inputs(B, H, KV, Sq, Sk, gain, dev):
    g = torch.Generator().manual_seed(B * 1000 + Sq * 7 + Sk)
    q = torch.randn(B, H, Sq, 128, generator=g)
    k = torch.randn(B, KV, Sk, 128, generator=g)      # different per kv head and batch row
    scale = 128 ** -0.5
    if gain != 1.0:
        # scale q so that the largest |logit| is `gain`: exercises the max subtraction
        logits = torch.einsum("bhsd,bhjd->bhsj", q, k.repeat_interleave(H // KV, dim=1)) * scale
        q = q * (gain / logits.abs().max())
    return q.bfloat16().to(dev), k.bfloat16().to(dev), scale


def _reference(q, k, H, KV, heads, k0, k1, scale):
    kk = k.float().repeat_interleave(H // KV, dim=1)                         # head h reads kv head h // (H/KV)
    logits = torch.einsum("bhsd,bhjd->bhsj", q.float(), kk) * scale
    p = torch.softmax(logits, dim=-1)                                        # fp32, over ALL keys
    return logits, p[:, heads].permute(1, 0, 3, 2)[:, :, k0:k1, :].contiguous()   # [n, B, k1-k0, Sq]


def _run(q, k, B, H, KV, Sq, Sk, heads, k0, k1, scale):
    from acehip import _ffi
    n = len(heads)
    numel = n * B * (k1 - k0) * Sq
    buf = torch.full((numel + 256,), CANARY, device=q.device, dtype=torch.float32)
    hs = (ctypes.c_int * n)(*heads)
    rc = _ffi.lib().acehip_attention_probs_bf16(_ffi.ptr(q), _ffi.ptr(k), B, H, KV, Sq, Sk, hs, n, k0, k1,
                                                float(scale), _ffi.ptr(buf), _ffi.stream_ptr())
    _ffi.check(rc, "attention_probs")
    torch.cuda.synchronize()
    return buf[:numel].view(n, B, k1 - k0, Sq), buf[numel:]


@pytest.mark.parametrize("shape", SHAPES)
def test_attention_probs_vs_torch_softmax(gpu_device, shape):
    B, H, KV, Sq, Sk, heads, k0, k1, gain = shape
    q, k, scale = _inputs(B, H, KV, Sq, Sk, gain, gpu_device)
    logits, ref = _reference(q, k, H, KV, heads, k0, k1, scale)
    if gain != 1.0:
        assert 39.0 < float(logits.abs().max()) < 41.0 and float(logits.min()) < -30.0 < 30.0 < float(logits.max())
    out, tail = _run(q, k, B, H, KV, Sq, Sk, heads, k0, k1, scale)
    assert torch.all(tail == CANARY), "memory past out was written"
    err = (out - ref).abs()
    bound = REL * ref.abs() + ABS
    worst = float((err / bound).max())
    print(f"{shape}: max err/bound = {worst:.4f}, max abs err = {float(err.max()):.3e}")
    assert torch.isfinite(out).all()
    assert worst <= 1.0, (shape, worst)
    # the stored values are bf16-representable (rounded before the fp32 store)
    assert torch.equal(out, out.bfloat16().float())
    if k0 == 0 and k1 == Sk:      # whole rows: they sum to 1 up to the bf16 rounding of each term
        assert float((out.sum(dim=2) - 1.0).abs().max()) < 2.0 ** -7


def test_attention_probs_bad_arguments(gpu_device):
    from acehip import _ffi
    lib = _ffi.lib()
    B, H, KV, Sq, Sk = 1, 4, 2, 8, 40
    q, k, scale = _inputs(B, H, KV, Sq, Sk, 1.0, gpu_device)
    out = torch.full((4 * B * Sk * Sq,), CANARY, device=gpu_device)

    def call(heads, k0, k1, qq=q, n=None, kv=KV):
        hs = (ctypes.c_int * max(len(heads), 1))(*heads)
        return lib.acehip_attention_probs_bf16(_ffi.ptr(qq), _ffi.ptr(k), B, H, kv, Sq, Sk, hs,
                                               len(heads) if n is None else n, k0, k1, scale, _ffi.ptr(out),
                                               _ffi.stream_ptr())
    assert call([0], 0, Sk) == 0
    for bad in (lambda: call([4], 0, Sk), lambda: call([-1], 0, Sk),        # head out of range
                lambda: call([0], -1, 5), lambda: call([0], 5, 5), lambda: call([0], 7, 3),
                lambda: call([0], 0, Sk + 1),                                # key range
                lambda: call([0], 0, Sk, n=0), lambda: call([0], 0, Sk, n=65),
                lambda: call([0], 0, Sk, kv=3),                              # H % KV
                lambda: call([0], 0, Sk, qq=None)):
        assert bad() == -1
        assert lib.acehip_last_error()
    torch.cuda.synchronize()
    assert torch.all(out[Sk * Sq:] == CANARY)        # the refused calls wrote nothing
