"""acehip_lm_head_bf16 (csrc/attn_decode.hip): y = bf16(x · Wᵀ) for M <= 16 rows and a
vocabulary-sized N that is no multiple of 4 or of the block's column count, against
bf16(x.float() @ W.float().T).  The bar is the GEMM tests': rel-L2 < 5e-3; the last row and
the last column are checked on their own, and the columns past N of a wider output stay
untouched."""
import pytest
import torch

from conftest import rel_l2

pytestmark = pytest.mark.gpu

NMAX = 70001


@pytest.fixture(scope="module")
def weights(gpu_device):
    g = torch.Generator().manual_seed(3)
    return {K: (torch.randn(NMAX, K, generator=g) * 0.05).bfloat16().to(gpu_device) for K in (256, 1024, 2048)}


@pytest.mark.parametrize("N", [512, NMAX])
@pytest.mark.parametrize("K", [256, 1024, 2048])
@pytest.mark.parametrize("M", [1, 2, 4, 16])    # 4: the M = 3..4 kernel variant
def test_lm_head_vs_fp32(gpu_device, weights, M, K, N):
    from acehip import _ffi as ff
    W = weights[K][:N]
    g = torch.Generator().manual_seed(M * 100 + K + N)
    x = torch.randn(M, K, generator=g).bfloat16().to(gpu_device)
    ldy = N + 5
    y = torch.full((M, ldy), 7.0, device=gpu_device, dtype=torch.bfloat16)
    ff.check(ff.lib().acehip_lm_head_bf16(ff.ptr(x), K, ff.ptr(W), ff.ptr(y), ldy, M, N, K, ff.stream_ptr()), "lm_head")
    torch.cuda.synchronize()
    ref = (x.float() @ W.float().T).bfloat16().float().cpu()
    out = y[:, :N].float().cpu()
    assert torch.isfinite(out).all()
    assert rel_l2(out, ref) < 5e-3, rel_l2(out, ref)
    assert rel_l2(out[M - 1], ref[M - 1]) < 5e-3          # last row
    assert rel_l2(out[:, N - 1], ref[:, N - 1]) < 5e-3    # last column (N % 4 != 0 at 70 001)
    assert bool((y[:, N:] == 7.0).all())                  # nothing written past N


def test_lm_head_arguments(gpu_device, weights):
    from acehip import _ffi as ff
    W = weights[256]
    x = torch.zeros(17, 256, device=gpu_device, dtype=torch.bfloat16)
    y = torch.zeros(17, 512, device=gpu_device, dtype=torch.bfloat16)
    fn = ff.lib().acehip_lm_head_bf16
    assert fn(ff.ptr(x), 256, ff.ptr(W), ff.ptr(y), 512, 17, 512, 256, ff.stream_ptr()) != 0     # M > 16
    assert fn(ff.ptr(x), 256, ff.ptr(W), ff.ptr(y), 256, 2, 512, 256, ff.stream_ptr()) != 0      # ldy < N
    assert fn(ff.ptr(x), 256, ff.ptr(W), ff.ptr(y), 512, 2, 512, 252, ff.stream_ptr()) != 0      # K % 8
