"""The GEMM-side kernels of the LM token loop at the 4B LM's widths (hidden 2560, intermediate
9728, QKV width 6144 = (32 + 8 + 8) · 128), kernel by kernel: the 4B is the first user of K = 2560
(40 K-tiles) and K = 9728 (152), of N = 19 456 for the small-M SwiGLU, of rmsnorm at D = 2560 with
deferred split-K partials and of head-post at 32 + 8 + 8 heads.

M = 2 is a decode pair, 16 the lm_head limit, 140 a short prompt with a ragged 128-row tile.
References are fp64 on the same bf16 inputs; the bars are those of the existing direct tests,
restated:
  * store (tests/test_gpu_dit.py test_gemm_splitk_small_m): rel-L2 < 5e-3;
  * SwiGLU (the same test): rel-L2 < 1e-2 against silu(bf16(gate))·bf16(up) of the fp64 product;
  * residual (tests/test_gpu_gemm_residual.py, acehip_gemm_res_bf16 in place): against
    rbf(res + rbf(acc)), share of not-bit-equal elements < 1e-3 overall and < 0.05 per row, each
    such element within 2^-6 · (|o| + |out|);
  * residual + norm pair (the same file): X under the residual bars, the norm output against the
    oracle norm of the kernel's own X with a mismatch share < 1e-3 and rel-L2 < 2e-3, deferred == 1;
  * head-post (tests/test_gpu_fused.py): against the oracle head-post of the same GEMM's plain
    store, rel-L2 < 2e-3, mismatch share < 1e-3 (+ 5e-3 for q and k), v bit-exact;
  * lm_head (tests/test_gpu_lm_head.py): rel-L2 < 5e-3, nothing written past N;
  * lm_score (tests/test_gpu_lm_score.py): integer-valued inputs, counts exact, lse and logprob
    within (L + 8) · 2^-24 + |lse| · 2^-23, L = 40 + ceil(ceil(V / 128) / 64).

The plan's diagnostic entry must put the M = 2 store and residual shapes on the split-K route, with
a ragged last split among them (on 256 CUs: K = 2560 as 14 + 14 + 12 K-tiles, K = 4096 as 6 × 10 +
4, K = 9728 as 6 × 22 + 20).

Measured on an MI355X: store rel-L2 1.65e-3 … 1.67e-3, SwiGLU 1.64e-3 … 1.66e-3; residual shares not
bit-equal overall 0 … 1.95e-4 (K = 9728, M = 2), worst row 3.9e-4 (one element of 2560), none past the
element bound; the pair's X the same and its norm output equal to the oracle's; head-post equal to
the oracle of its own plain store; lm_score lse / logprob error 1.4e-6 / 1.3e-6 (bound 6.4e-6)."""
import ctypes
import functools
import math

import pytest
import torch

from conftest import rel_l2

from oracle import dit_oracle

pytestmark = pytest.mark.gpu

EPI_STORE, EPI_RES, EPI_SWIGLU = 0, 2, 3
MS = (2, 16, 140)
# (epilogue, N, K)
SHAPES = [(EPI_STORE, 6144, 2560), (EPI_RES, 2560, 4096), (EPI_SWIGLU, 19456, 2560), (EPI_RES, 2560, 9728)]
BAR_OVERALL, BAR_ROW, BAR_ELEM = 1e-3, 0.05, 2.0 ** -6
GUARD, SENTINEL, EPS = 16, 24576.0, 1e-6


def _ff():
    from acehip import _ffi
    return _ffi


def rbf(x):
    return x.to(torch.float32).to(torch.bfloat16).to(torch.float64)


def _bits(t):
    return t.contiguous().view(torch.int16)


@functools.lru_cache(maxsize=None)
def _weight(N, K):
    """W ~ 0.02 · N(0, 1) as bf16 on the GPU, one per (N, K), never modified."""
    g = torch.Generator(device="cuda").manual_seed(N * 1009 + K)
    return (torch.randn(N, K, device="cuda", generator=g) * 0.02).bfloat16()


@functools.lru_cache(maxsize=None)
def _rows(M, N, K):
    """A ~ N(0, 1) [M, K], res ~ N(0, 1) [M, N] as bf16 on the GPU, and acc = A·Wᵀ in fp64."""
    g = torch.Generator(device="cuda").manual_seed(M * 1000003 + N * 1009 + K)
    A = torch.randn(M, K, device="cuda", generator=g).bfloat16()
    res = torch.randn(M, N, device="cuda", generator=g).bfloat16()
    return A, res, A.double() @ _weight(N, K).double().t()


def accept(got, o, out, what):
    """got bf16 [M, N] against the specification's o (fp64) and out (bf16)."""
    ne = _bits(got) != _bits(out)
    diff = (got.double() - out.double()).abs()
    far = int((ne & ~(diff <= BAR_ELEM * (o.abs() + out.double().abs()))).sum())      # ~(≤): a NaN counts
    share = ne.double().mean(dim=1)
    overall, worst = float(share.mean()), float(share.max())
    print(f"{what}: not bit-equal overall {overall:.2e}, worst row {worst:.2e}, past the element bound {far}")
    assert overall < BAR_OVERALL, (what, "overall share not bit-equal", overall)
    assert worst < BAR_ROW, (what, "worst row share not bit-equal", worst)
    assert far == 0, (what, "elements past 2^-6·(|o| + |out|)", far)


def _sentinel_intact(t):
    return bool((t == SENTINEL).all())


@pytest.mark.parametrize("M", MS)
@pytest.mark.parametrize("epi,N,K", SHAPES)
def test_gemm_at_4b_widths_vs_fp64(gpu_device, epi, N, K, M):
    ff = _ff()
    A, res, acc = _rows(M, N, K)
    W = _weight(N, K)
    what = (epi, M, N, K)
    if epi == EPI_RES:
        C = torch.full((M + GUARD, N), SENTINEL, dtype=torch.bfloat16, device=gpu_device)
        C[:M] = res
        ff.check(ff.lib().acehip_gemm_res_bf16(ff.ptr(A), K, ff.ptr(W), K, ff.ptr(C), N, M, N, K, ff.ptr(C), N, None,
                                               0, M, -1, ff.stream_ptr()), "gemm_res")
        torch.cuda.synchronize()
        assert _sentinel_intact(C[M:]), "rows past M were written"
        o = rbf(acc)
        accept(C[:M], o, (res.double() + o).to(torch.float32).to(torch.bfloat16), what)
        return
    ncol = N // 2 if epi == EPI_SWIGLU else N
    C = torch.full((M + GUARD, ncol), SENTINEL, dtype=torch.bfloat16, device=gpu_device)
    ff.check(ff.lib().acehip_gemm_bf16_ex(ff.ptr(A), K, ff.ptr(W), K, ff.ptr(C), ncol, M, N, K, None, epi, -1,
                                          ff.stream_ptr()), "gemm")
    torch.cuda.synchronize()
    assert _sentinel_intact(C[M:]), "rows past M were written"
    got = C[:M].float()
    assert torch.isfinite(got).all()
    if epi == EPI_SWIGLU:
        y = rbf(acc).float().view(M, N // 64, 2, 32)
        gate, up = y[:, :, 0, :].reshape(M, ncol), y[:, :, 1, :].reshape(M, ncol)
        want, tol = torch.nn.functional.silu(gate).bfloat16().double() * up.double(), 1e-2
    else:
        want, tol = acc, 5e-3
    err = rel_l2(got.cpu(), want.cpu())
    err_last = rel_l2(got[M - 1].cpu(), want[M - 1].cpu())
    print(f"{what}: rel-L2 {err:.2e}, last row {err_last:.2e}, bar {tol:.0e}")
    assert err < tol and err_last < tol, (what, err, err_last)


def test_decode_pair_plans_split_k_with_a_ragged_last_split(gpu_device):
    """The M = 2 store and residual shapes run as split-K (the SwiGLU takes whole-K small-M tiles),
    the residual ones deferred when the caller allows it, and a last split is shorter than the
    others at least once."""
    ff = _ff()
    ragged = []
    for epi, N, K in SHAPES:
        p = ff.gemm_plan(2, N, K, epi)
        if epi == EPI_SWIGLU:
            assert p["route"] == ff.ROUTE_TILE and p["splits"] == 0, p
            continue
        assert p["route"] == ff.ROUTE_SPLITK and p["splits"] > 1, (N, K, p)
        tiles = K // 64
        assert (p["splits"] - 1) * p["kper"] < tiles <= p["splits"] * p["kper"], (N, K, p)
        if tiles % p["kper"]:
            ragged.append((N, K, p["splits"], p["kper"], tiles % p["kper"]))
        if epi == EPI_RES:
            assert ff.gemm_plan(2, N, K, epi, defer_ok=True)["deferred"] == 1
    print("ragged last splits (N, K, splits, kper, last):", ragged)
    assert ragged


@pytest.mark.parametrize("K", [4096, 9728])
def test_deferred_residual_and_norm_at_d2560(gpu_device, K):
    """The production pair of a decode step: the O / down GEMM leaves its split-K partials and
    rmsnorm applies the residual epilogue (D = 2560: ten 256-column groups per row)."""
    ff = _ff()
    M, D = 2, 2560
    A, res, acc = _rows(M, D, K)
    W = _weight(D, K)
    g = torch.Generator().manual_seed(K)
    w = (1 + 0.1 * torch.randn(D, generator=g)).bfloat16()
    wd = w.to(gpu_device)
    X = res.clone()
    out = torch.full((M + GUARD, D), SENTINEL, dtype=torch.bfloat16, device=gpu_device)
    deferred = ctypes.c_int(-1)
    ff.check(ff.lib().acehip_gemm_res_norm_bf16(
        ff.ptr(A), K, ff.ptr(W), K, ff.ptr(X), M, D, K, None, 0, M, 1, ff.ptr(wd), None, None, 0,
        ff.ptr(out), M, EPS, None, M, ctypes.byref(deferred), ff.stream_ptr()), "gemm_res_norm")
    torch.cuda.synchronize()
    assert deferred.value == 1, "the pair did not defer: no split-K at this shape"
    assert _sentinel_intact(out[M:]), "norm rows past M were written"
    o = rbf(acc)
    accept(X, o, (res.double() + o).to(torch.float32).to(torch.bfloat16), ("X", K))
    Xc, oc = X.cpu(), out[:M].cpu()
    ref = dit_oracle.rms_norm(Xc, w, EPS)
    share = (oc != ref).float().mean().item()
    print(f"K{K}: norm output mismatch share {share:.2e}, rel-L2 {rel_l2(oc.float(), ref.float()):.2e}")
    assert share < 1e-3, ("norm output vs oracle", share)
    assert rel_l2(oc.float(), ref.float()) < 2e-3


def _headpost_ref(C, B, S, nq, nk, nv, qw, kw, cos, sin, eps):
    x = C.view(B, S, nq + nk + nv, 128)
    q = x[:, :, :nq].transpose(1, 2)
    k = x[:, :, nq:nq + nk].transpose(1, 2)
    v = x[:, :, nq + nk:].transpose(1, 2)
    q, k = dit_oracle.rms_norm(q, qw, eps), dit_oracle.rms_norm(k, kw, eps)
    c, s_ = cos[None, None], sin[None, None]
    q = q * c + dit_oracle._rotate_half(q) * s_
    k = k * c + dit_oracle._rotate_half(k) * s_
    return q.contiguous(), k.contiguous(), v.contiguous()


@pytest.mark.parametrize("B,S", [(2, 1), (2, 70)])
def test_headpost_at_32_8_8_heads(gpu_device, B, S):
    """The QKV projection with q / k norm, RoPE and the head-major scatter at 32 + 8 + 8 heads,
    K = 2560: M = 2 (a decode pair) and M = 140; both plan as split-K partials + head_post."""
    ff = _ff()
    nq, nk, nv, K = 32, 8, 8, 2560
    N, M = (nq + nk + nv) * 128, B * S
    assert ff.gemm_plan(M, N, K, 4)["route"] == ff.ROUTE_SPLITK
    A = _rows(M, N, K)[0]
    W = _weight(N, K)
    g = torch.Generator().manual_seed(S)
    qw = (1 + 0.1 * torch.randn(128, generator=g)).bfloat16()
    kw = (1 + 0.1 * torch.randn(128, generator=g)).bfloat16()
    cos, sin = dit_oracle.rope_tables(S, 128, 1e6, torch.bfloat16)
    cos, sin = cos[0].contiguous(), sin[0].contiguous()
    qwd, kwd, cosd, sind = (t.to(gpu_device) for t in (qw, kw, cos, sin))
    q, k, v = (torch.full((B, n, S, 128), float("nan"), dtype=torch.bfloat16, device=gpu_device) for n in (nq, nk, nv))
    ff.check(ff.lib().acehip_gemm_headpost_bf16(ff.ptr(A), K, ff.ptr(W), K, B, S, nq, nk, nv, ff.ptr(qwd), ff.ptr(kwd),
                                                ff.ptr(cosd), ff.ptr(sind), EPS, ff.ptr(q), ff.ptr(k), ff.ptr(v),
                                                ff.stream_ptr()), "gemm_headpost")
    C = torch.empty(M, N, dtype=torch.bfloat16, device=gpu_device)
    ff.check(ff.lib().acehip_gemm_bf16_ex(ff.ptr(A), K, ff.ptr(W), K, ff.ptr(C), N, M, N, K, None, EPI_STORE, -1,
                                          ff.stream_ptr()), "gemm")
    torch.cuda.synchronize()
    rq, rk, rv = _headpost_ref(C.cpu(), B, S, nq, nk, nv, qw, kw, cos, sin, EPS)
    for name, got, ref in (("q", q, rq), ("k", k, rk), ("v", v, rv)):
        got = got.cpu()
        assert torch.isfinite(got.float()).all(), name
        err, share = rel_l2(got.float(), ref.float()), (got != ref).float().mean().item()
        print(f"M{M} {name}: rel-L2 {err:.2e}, mismatch share {share:.2e}")
        assert err < 2e-3, (name, err)
        assert share < 1e-3 + (0 if name == "v" else 5e-3), (name, share)
    assert torch.equal(v.cpu(), rv)


def test_lm_head_at_k2560_ragged_vocab(gpu_device):
    ff = _ff()
    M, K, N = 2, 2560, 2051
    g = torch.Generator().manual_seed(N)
    W = (torch.randn(N, K, generator=g) * 0.05).bfloat16().to(gpu_device)
    x = torch.randn(M, K, generator=g).bfloat16().to(gpu_device)
    ldy = N + 5
    y = torch.full((M, ldy), 7.0, device=gpu_device, dtype=torch.bfloat16)
    ff.check(ff.lib().acehip_lm_head_bf16(ff.ptr(x), K, ff.ptr(W), ff.ptr(y), ldy, M, N, K, ff.stream_ptr()), "lm_head")
    torch.cuda.synchronize()
    ref = rbf(x.double() @ W.double().T).cpu()
    out = y[:, :N].double().cpu()
    assert torch.isfinite(out).all()
    assert rel_l2(out, ref) < 5e-3, rel_l2(out, ref)
    assert rel_l2(out[M - 1], ref[M - 1]) < 5e-3
    assert rel_l2(out[:, N - 1], ref[:, N - 1]) < 5e-3
    assert bool((y[:, N:] == 7.0).all())


def test_lm_score_at_k2560_exact(gpu_device):
    """x and W hold {-1, 0, 1}, at most 256 non-zeros per W row: every logit is an integer of
    magnitude <= 256, exact in fp32 and in bf16, so the counts equal torch's integer computation."""
    ff = _ff()
    T, K, V = 5, 2560, 2051
    g = torch.Generator(device=gpu_device).manual_seed(100 + K)
    nz = torch.rand(V, K, device=gpu_device, generator=g) < 128.0 / K
    W = (nz * (torch.randint(0, 2, (V, K), device=gpu_device, generator=g) * 2 - 1)).to(torch.bfloat16)
    assert int((W != 0).sum(1).max()) <= 256
    targets = torch.tensor([0, V - 1, 2048 + 1, 205, 1111])
    for c in (0, V - 1, 205):                            # ties on both sides of a target's index
        for d in (-1, 1, -129, 129):
            if 0 <= c + d < V and c + d not in targets.tolist():
                W[c + d] = W[c]
    x = torch.randint(-1, 2, (T, K), generator=torch.Generator().manual_seed(7)).to(torch.bfloat16).to(gpu_device)
    tg = targets.to(device=gpu_device, dtype=torch.int32)
    SENT_F, SENT_I, PAD = 1234.5, 777, 5
    lp = torch.full((T + PAD,), SENT_F, device=gpu_device)
    lse = torch.full((T + PAD,), SENT_F, device=gpu_device)
    ng = torch.full((T + PAD,), SENT_I, device=gpu_device, dtype=torch.int32)
    ne = torch.full((T + PAD,), SENT_I, device=gpu_device, dtype=torch.int32)
    need = int(ff.lib().acehip_lm_score_ws_bytes(T, V))
    ws = torch.full((need + 256,), 0x5A, device=gpu_device, dtype=torch.uint8)
    ff.check(ff.lib().acehip_lm_score_bf16(ff.ptr(x), K, ff.ptr(W), ff.ptr(tg), T, V, K, ff.ptr(lp), ff.ptr(lse),
                                           ff.ptr(ng), ff.ptr(ne), ff.ptr(ws), need, ff.stream_ptr()), "lm_score")
    torch.cuda.synchronize()
    logits = x.float() @ W.float().T
    assert float(logits.abs().max()) <= 256
    tgl = targets.to(gpu_device)
    tl = logits.gather(1, tgl[:, None])
    col = torch.arange(V, device=gpu_device)[None, :]
    want_ng, want_ne = (logits > tl).sum(1), ((logits == tl) & (col < tgl[:, None])).sum(1)
    assert torch.equal(ng[:T].long(), want_ng), (ng[:T].tolist(), want_ng.tolist())
    assert torch.equal(ne[:T].long(), want_ne), (ne[:T].tolist(), want_ne.tolist())
    assert int(want_ne.max()) > 0                        # the planted ties are there
    ref = torch.logsumexp(logits.double(), dim=1)
    bound = (40 + math.ceil(math.ceil(V / 128) / 64) + 8) * 2.0 ** -24 + ref.abs() * 2.0 ** -23
    e_lse = (lse[:T].double() - ref).abs()
    e_lp = (lp[:T].double() - (tl[:, 0].double() - ref)).abs()
    print(f"lse err max {float(e_lse.max()):.3e}, logprob err max {float(e_lp.max()):.3e}, bound min {float(bound.min()):.3e}")
    assert bool((e_lse <= bound).all()) and bool((e_lp <= bound).all())
    assert bool((lp[T:] == SENT_F).all()) and bool((lse[T:] == SENT_F).all())
    assert bool((ng[T:] == SENT_I).all()) and bool((ne[T:] == SENT_I).all()) and bool((ws[need:] == 0x5A).all())
