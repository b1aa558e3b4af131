"""The GEMM residual epilogues (EPI_RES, EPI_GATED_RES) and the norm that absorbs them, kernel by
kernel, against an fp64 reference that applies every bf16 rounding of the specification:

    acc = A·Wᵀ                       (fp64; the kernels accumulate in fp32: the only freedom)
    o   = rbf(acc)
    o   = rbf(o · gate[row // rows_per_batch])          (gated form only)
    out = rbf(res + o)

rbf is a round trip through bf16 (by way of fp32, as the kernels round: sums and products of two
bf16 values are exact in fp32 and in fp64, so past `acc` the reference and a correct kernel agree
bit for bit).  Acceptance of a result against this reference (conditions, not measurements):

    overall share of elements not bit-equal to the reference      < 1e-3
    share of not-bit-equal elements per row, maximum over rows    < 0.05
    each not-bit-equal element   |got − ref| ≤ 2⁻⁶·(|o| + |out|), o and out from the reference

The third bound: one flipped bf16 rounding of acc moves o by at most one ulp (≤ 2⁻⁷ relative),
the re-rounded gate product by at most one more, the final sum by one ulp of out.

fp32 accumulation on the CPU (torch fp32 matmul, a 4-chunk split sum) against this reference:
(300, 512, 192) overall ≤ 1.3e-5, worst row ≤ 2.0e-3; (300, 512, 128) 0 / 0; (200, 2048, 2048)
≤ 3.5e-5 / ≤ 4.9e-4; (125, 768, 1024) ≤ 1.1e-5 / ≤ 1.4e-3.  The mutants (test_acceptance_
rejects_mutants) land at 8–31 % overall, or 98 % of a row for a batch index off by one.
The shares each family measured on an MI355X stand in the docstring of its test.
"""
import contextlib
import ctypes
import functools

import pytest
import torch

from conftest import rel_l2, set_knob

from oracle import dit_oracle

gpu = pytest.mark.gpu

BAR_OVERALL, BAR_ROW, BAR_ELEM = 1e-3, 0.05, 2.0 ** -6
GATE_SLOTS, GATE_SLOT = 6, 2        # gate rows are a strided slice of a [batch][6][N] table, as in the DiT
GUARD = 16                          # rows past M that must keep the sentinel
PAD = 64                            # pad columns of the out-of-place layout (ldc = ldr = N + 64)
SENTINEL = 24576.0                  # exactly a bf16 value; no result of these inputs comes near it
EPS = 1e-6


# ------------------------------------------------------------------ reference ---
def rbf(x):
    return x.to(torch.float32).to(torch.bfloat16).to(torch.float64)


def _randn(seed, *shape, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).bfloat16()


@functools.lru_cache(maxsize=None)
def _base(M, N, K):
    """A ~ N(0,1), W ~ 0.05·N(0,1), res ~ N(0,1) as bf16, and acc = A·Wᵀ in fp64.  Shared and
    never modified: every launch works on copies."""
    seed = M * 1000003 + N * 1009 + K
    A, W, res = _randn(seed, M, K), _randn(seed + 1, N, K, scale=0.05), _randn(seed + 2, M, N)
    return A, W, res, A.double() @ W.double().t()


@functools.lru_cache(maxsize=None)
def _gate_table(M, N, rpb):
    """gate ~ 0.5·N(0,1), a distinct row per batch: exactly ceil(M / rpb) rows (loads are clamped
    to row M − 1), GATE_SLOTS·N apart."""
    nb = (M + rpb - 1) // rpb
    return _randn(M * 7919 + N * 31 + rpb, nb, GATE_SLOTS, N, scale=0.5)


def _epilogue_ref(acc, res, gate_rows, round_acc=True, round_prod=True):
    """(o, out) of the specification; gate_rows [M][N] (the gate row of each output row) or None.
    round_acc / round_prod = False drop one rounding: the mutants of the CPU test."""
    o = rbf(acc) if round_acc else acc
    if gate_rows is not None:
        o = o * gate_rows.double()
        if round_prod:
            o = rbf(o)
    return o, (res.double() + o).to(torch.float32).to(torch.bfloat16)


def _gate_rows(M, N, rpb, shift=0):
    tab = _gate_table(M, N, rpb)
    b = ((torch.arange(M) + shift) // rpb).clamp_max(tab.shape[0] - 1)
    return tab[b, GATE_SLOT]


@functools.lru_cache(maxsize=None)
def _ref(M, N, K, rpb, gated):
    _, _, res, acc = _base(M, N, K)
    return _epilogue_ref(acc, res, _gate_rows(M, N, rpb) if gated else None)


def _bits(t):
    return t.contiguous().view(torch.int16)


def judge(got, ref):
    """(overall share, worst row share, elements past the per-element bound) of got [M][N] bf16
    against ref = (o fp64, out bf16)."""
    o, out = ref
    ne = _bits(got) != _bits(out)
    diff = (got.double() - out.double()).abs()
    lim = BAR_ELEM * (o.abs() + out.double().abs())
    far = int((ne & ~(diff <= lim)).sum())          # ~(≤) so that a NaN counts
    share = ne.double().mean(dim=1)
    return float(share.mean()), float(share.max()), far


def accept(got, ref, what=""):
    overall, worst, far = judge(got, ref)
    assert overall < BAR_OVERALL, (what, "overall share not bit-equal", overall)
    assert worst < BAR_ROW, (what, "worst row share not bit-equal", worst)
    assert far == 0, (what, "elements past 2^-6·(|o| + |out|)", far)
    return overall, worst


# ------------------------------------------------------------- CPU: sharpness ---
def test_acceptance_rejects_mutants():
    """The acceptance passes fp32 accumulation and rejects each subtle error it exists to catch,
    at (300, 512, 192), rows_per_batch 77: a dropped bf16(acc), a dropped rounding of the gate
    product (both fail the overall bar), and a batch index off by one row (about 1 % overall,
    98 % of the rows before a batch boundary: the per-row bar)."""
    M, N, K, rpb = 300, 512, 192, 77
    A, W, res, acc = _base(M, N, K)
    gr = _gate_rows(M, N, rpb)
    acc32 = (A.float() @ W.float().t()).double()
    chunks = sum((A[:, k:k + 48].float() @ W[:, k:k + 48].float().t() for k in range(0, K, 48)),
                 torch.zeros(M, N)).double()
    for g in (None, gr):
        ref = _epilogue_ref(acc, res, g)
        assert judge(ref[1], ref) == (0.0, 0.0, 0)
        for a32 in (acc32, chunks):
            overall, worst = accept(_epilogue_ref(a32, res, g)[1], ref, "fp32 accumulation")
            assert overall <= 1e-4 and worst <= 1e-2
        # dropped bf16(acc)
        overall, _, _ = judge(_epilogue_ref(acc, res, g, round_acc=False)[1], ref)
        assert overall > 50 * BAR_OVERALL
        with pytest.raises(AssertionError):
            accept(_epilogue_ref(acc, res, g, round_acc=False)[1], ref)
    ref = _epilogue_ref(acc, res, gr)
    # dropped rounding of the product
    mut = _epilogue_ref(acc, res, gr, round_prod=False)[1]
    assert judge(mut, ref)[0] > 50 * BAR_OVERALL
    with pytest.raises(AssertionError):
        accept(mut, ref)
    # batch index off by one row: rows 76, 153, 230 read the next batch's gate
    mut = _epilogue_ref(acc, res, _gate_rows(M, N, rpb, shift=1))[1]
    overall, worst, _ = judge(mut, ref)
    assert overall < 0.02 and worst > 10 * BAR_ROW
    with pytest.raises(AssertionError, match="worst row|overall"):
        accept(mut, ref)
    ne_rows = (_bits(mut) != _bits(ref[1])).any(dim=1).nonzero().flatten().tolist()
    assert ne_rows == [76, 153, 230]
    # a NaN is never accepted
    bad = ref[1].clone()
    bad[7, 9] = float("nan")
    assert judge(bad, ref)[2] == 1


# ------------------------------------------------------------------ GPU side ---
def _ff():
    from acehip import _ffi
    return _ffi


@contextlib.contextmanager
def knobs(monkeypatch, **kn):
    """ACEHIP_* switches for a block of launches (None: leave the default)."""
    kn = {k: v for k, v in kn.items() if v is not None}
    for k, v in kn.items():
        set_knob(monkeypatch, k, v)
    try:
        yield
    finally:
        for k in kn:
            monkeypatch.delenv(k, raising=False)
        _ff().reload_knobs()


def _sentinel_intact(t):
    return bool((_bits(t) == _bits(torch.tensor([SENTINEL], dtype=torch.bfloat16))[0]).all())


# C / residual layouts as (pad columns of C, pad columns of the residual buffer): in place (C == res,
# ldc = ldr = N), out of place with one pitch (ldc = ldr = N + 64), out of place with two pitches
# (ldc = N + 64, ldr = N + 128: a kernel that indexed the residual with ldc, or C with ldr, shows)
IN_PLACE, SAME_PITCH, OWN_PITCH = None, (PAD, PAD), (PAD, 2 * PAD)
RES_LAYOUTS = (IN_PLACE, SAME_PITCH, OWN_PITCH)


def run_gemm_res(dev, M, N, K, rpb, gated, variant, layout):
    """One acehip_gemm_res_bf16 launch on fresh copies of the shared inputs → the live [M][N]
    region on the CPU, after checking that guard rows and pad columns kept their sentinel."""
    ff = _ff()
    A, W, res, _ = _base(M, N, K)
    Ad, Wd = A.to(dev), W.to(dev)
    gd = _gate_table(M, N, rpb).to(dev) if gated else None
    ldc, ldr = (N, N) if layout is IN_PLACE else (N + layout[0], N + layout[1])
    C = torch.full((M + GUARD, ldc), SENTINEL, dtype=torch.bfloat16, device=dev)
    if layout is IN_PLACE:
        C[:M] = res.to(dev)
        R = C
    else:   # the residual in its own buffer; its pad columns hold NaN (never to be read)
        R = torch.full((M, ldr), float("nan"), dtype=torch.bfloat16, device=dev)
        R[:, :N] = res.to(dev)
    ff.check(ff.lib().acehip_gemm_res_bf16(
        ff.ptr(Ad), K, ff.ptr(Wd), K, ff.ptr(C), ldc, M, N, K, ff.ptr(R), ldr,
        ff.ptr(gd[:, GATE_SLOT]) if gated else None, GATE_SLOTS * N, rpb, variant, ff.stream_ptr()), "gemm_res")
    torch.cuda.synchronize()
    Cc = C.cpu()
    assert _sentinel_intact(Cc[M:]), "rows past M were written"
    assert _sentinel_intact(Cc[:M, N:]), "pad columns were written"
    if layout is not IN_PLACE:
        assert torch.equal(_bits(R[:, :N].cpu()), _bits(res)), "the separate residual was written"
    return Cc[:M, :N].contiguous()


def check_layouts(dev, M, N, K, rpb, gated, variant, what):
    """Every layout against the reference, and all bit-identical to the in-place result."""
    ref = _ref(M, N, K, rpb, gated)
    outs = [run_gemm_res(dev, M, N, K, rpb, gated, variant, layout) for layout in RES_LAYOUTS]
    for o, layout in zip(outs, RES_LAYOUTS):
        accept(o, ref, (what, layout))
        assert torch.equal(_bits(o), _bits(outs[0])), (what, layout, "!= in place")
    return outs[0]


# (M, N, K, rows_per_batch): odd K-tile count + ragged M + batch boundaries inside 16-row groups +
# a partial last batch; more than two row tiles of every variant; a single K tile with N % 256 != 0;
# one row
TILE_SHAPES = [(300, 512, 192, 77), (517, 768, 128, 130), (200, 384, 64, 67), (1, 256, 128, 1)]
TILE_CASES = [(v, s) for v in (0, 7, 8, 9, 13, 16, 17) for s in TILE_SHAPES if not (v in (7, 8, 9) and s[1] % 256)]


@gpu
@pytest.mark.parametrize("variant,shape", TILE_CASES, ids=lambda p: "x".join(map(str, p)) if isinstance(p, tuple) else f"v{p}")
def test_tile_variants_residual_epilogues(gpu_device, variant, shape):
    """Family 1: every tile variant (gemm_kernel 128×128 / 128×64 ± helper waves, gemm_pp_kernel
    256 / 192 / 128 rows, gemm_w4_kernel) with both residual epilogues through epilogue_tile's
    chunked load-before-store path, in place (C == res) and out of place with ldr = ldc = N + 64 and
    with ldr = N + 128 != ldc = N + 64 (guard rows and pad columns keep their sentinel, the
    residual's pad columns hold NaN), the three layouts bit-identical.  The ping-pong
    variants need N % 256 == 0 and are not generated for N = 384.
    MI355X, the same for every variant (all sum the K tiles in order): (300, 512, 192) overall
    6.5e-6, worst row 2.0e-3 (one element of 512); (517, 768, 128) 5.0e-6 / 1.3e-3; (200, 384, 64) and
    (1, 256, 128) 0 / 0."""
    for gated in (False, True):
        check_layouts(gpu_device, *shape, gated, variant, (variant, shape, gated))


@gpu
@pytest.mark.parametrize("shape", TILE_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_four_wave_tile_without_helpers_residual_epilogues(gpu_device, monkeypatch, shape):
    """Family 1, the A/B arm of variant 13: gemm_w4_kernel without its LDS-DMA helper waves
    (ACEHIP_GEMM_HELPERS=0), bit-identical to the arm with them.
    MI355X: the shares of the arm with helpers (test_tile_variants_residual_epilogues)."""
    for gated in (False, True):
        with knobs(monkeypatch, ACEHIP_GEMM_HELPERS="0"):
            off = check_layouts(gpu_device, *shape, gated, 13, (shape, gated))
        on = run_gemm_res(gpu_device, *shape, gated, 13, IN_PLACE)
        assert torch.equal(_bits(on), _bits(off))


@gpu
@pytest.mark.parametrize("M,N,rpb,cus,want", [(300, 512, 77, None, 0), (300, 512, 77, 6, 9),
                                              (1100, 512, 333, 8, 8), (2400, 256, 700, 4, 7)])
def test_production_dispatch_without_splitk(gpu_device, monkeypatch, M, N, rpb, cus, want):
    """Family 2: variant −1 at K = 128 (2 K-tiles < 8, so gemm() takes no split-K) must run one
    whole grid of the tile its plan names (asserted through acehip_diag_gemm_plan; the rows stand in
    tests/test_gemm_plan_host.py): right against the reference, and bit-identical to that explicit
    variant.  The last two shapes are grids the planner splits for a store epilogue (asserted too),
    with a batch boundary on either side of M1: a tail launched for a residual epilogue would read
    the wrong gate batch and residual rows.
    MI355X: overall ≤ 6.5e-6, worst row ≤ 3.9e-3 (one element of a 256-column row at (2400, 256))."""
    K = 128
    ff = _ff()
    for gated in (False, True):
        with knobs(monkeypatch, ACEHIP_GEMM_CUS=cus):
            plan = ff.gemm_plan(M, N, K, 1 if gated else 2)
            assert (plan["route"], plan["v_head"]) == (ff.ROUTE_TILE, want), plan
            if want in (7, 8):
                assert ff.gemm_plan(M, N, K, 0)["route"] in (ff.ROUTE_TAIL1, ff.ROUTE_TAIL2)
            prod = check_layouts(gpu_device, M, N, K, rpb, gated, -1, (M, N, cus, gated))
            explicit = run_gemm_res(gpu_device, M, N, K, rpb, gated, want, IN_PLACE)
        assert torch.equal(_bits(prod), _bits(explicit)), f"production dispatch is not variant {want}"


SPLITK_SHAPES = [(M, N, K) for M in (125, 250) for N in (256, 2048) for K in (512, 1088)]
RPB = 50


@gpu
@pytest.mark.parametrize("M,N,K", SPLITK_SHAPES)
def test_splitk_epilogue_kernel(gpu_device, monkeypatch, M, N, K):
    """Family 3: variant −1 where the grid cannot fill half the chip and K has ≥ 8 tiles: fp32
    partials by gemm_kernel<EPI_PARTIAL> (128×64 tiles by default and with ACEHIP_SPLITK_BN=64,
    128×128 with =128), then splitk_epilogue_kernel's plain and gated branches, in place and out
    of place with ldr = ldc = N + 64 and with ldr = N + 128 != ldc = N + 64.  That the shape really
    splits on this device is asserted first, on the plan (2 splits of 4 K-tiles at K = 512; 4 splits
    of 5, 5, 5 and 2 at K = 1088, 17 K-tiles; the tile width the knob asks for) and through the
    entry point that reports it: the same GEMM with defer gives deferred == 1.
    Both tile widths sum the same splits in order, so the three settings are bit-identical.
    MI355X: overall ≤ 2.7e-5; worst row ≤ 3.9e-3 at N = 256 (one element), ≤ 9.8e-4 at N = 2048."""
    for bn in (None, "64", "128"):
        with knobs(monkeypatch, ACEHIP_SPLITK_BN=bn):
            plan = _ff().gemm_plan(M, N, K, 2)
            assert (plan["route"], plan["splits"], plan["kper"], plan["bn"]) == \
                (_ff().ROUTE_SPLITK, *((2, 4) if K == 512 else (4, 5)), int(bn or 64)), plan
            assert run_gemm_res_norm(gpu_device, M, N, K, False, False, "rows")[2] == 1, ("no split-K here", bn)
    for gated in (False, True):
        outs = []
        for bn in (None, "64", "128"):
            with knobs(monkeypatch, ACEHIP_SPLITK_BN=bn):
                outs.append(check_layouts(gpu_device, M, N, K, RPB, gated, -1, (M, N, K, gated, bn)))
        assert torch.equal(_bits(outs[0]), _bits(outs[1])) and torch.equal(_bits(outs[0]), _bits(outs[2]))


# -------------------------------------------- the deferred epilogue in the norm ---
NULL_ROWS = 50


@functools.lru_cache(maxsize=None)
def _norm_inputs(M, D):
    """Null rows appended to the residual stream, their constant v, the norm weight and the
    modulation table (rows 6·D apart, ceil((M + NULL_ROWS) / RPB) batches)."""
    seed = M * 104729 + D
    nb = (M + NULL_ROWS + RPB - 1) // RPB
    return (_randn(seed, NULL_ROWS, D), _randn(seed + 1, D),
            (1 + 0.1 * torch.randn(D, generator=torch.Generator().manual_seed(seed + 2))).bfloat16(),
            _randn(seed + 3, nb, 6, D, scale=0.3))


# M_norm == M | + null rows with v from row M, deferral allowed | not allowed | v from row M + GAP:
# rows [M, M + GAP) get neither the epilogue nor v and must come through unchanged
LAYOUTS = ("rows", "rows+null", "null-only", "rows+gap+null")
GAP = 10


def run_gemm_res_norm(dev, M, D, K, gated, mod, layout):
    """One acehip_gemm_res_norm_bf16 launch on fresh copies → (X, out, deferred) on the CPU."""
    ff = _ff()
    A, W, res, _ = _base(M, D, K)
    null, v, w, tab = _norm_inputs(M, D)
    with_v = layout != "rows"
    Mn = M + NULL_ROWS if with_v else M
    X = (torch.cat([res, null]) if with_v else res).to(dev)
    Ad, Wd, wd, td = A.to(dev), W.to(dev), w.to(dev), tab.to(dev)
    gd = _gate_table(M, D, RPB).to(dev) if gated else None
    vd = v.to(dev) if with_v else None
    out = torch.full((Mn + GUARD, D), SENTINEL, dtype=torch.bfloat16, device=dev)
    deferred = ctypes.c_int(-1)
    frm = M + GAP if layout == "rows+gap+null" else M
    ff.check(ff.lib().acehip_gemm_res_norm_bf16(
        ff.ptr(Ad), K, ff.ptr(Wd), K, ff.ptr(X), M, D, K,
        ff.ptr(gd[:, GATE_SLOT]) if gated else None, GATE_SLOTS * D, RPB, 0 if layout == "null-only" else 1,
        ff.ptr(wd), ff.ptr(td[:, 0]) if mod else None, ff.ptr(td[:, 1]) if mod else None, 6 * D,
        ff.ptr(out), Mn, EPS, ff.ptr(vd), frm, ctypes.byref(deferred), ff.stream_ptr()), "gemm_res_norm")
    torch.cuda.synchronize()
    oc = out.cpu()
    assert _sentinel_intact(oc[Mn:]), "norm rows past M_norm were written"
    return X.cpu(), oc[:Mn].contiguous(), deferred.value


def check_norm_result(M, D, K, gated, mod, layout, X, out):
    """X rows < M against the epilogue reference, rows [M, from) unchanged, null rows ==
    rbf(x + v) exactly, out against the oracle norm of the kernel's own X."""
    null, v, w, tab = _norm_inputs(M, D)
    accept(X[:M], _ref(M, D, K, RPB, gated), (M, D, K, gated, mod, layout))
    frm = M + GAP if layout == "rows+gap+null" else M
    if layout != "rows":
        assert torch.equal(_bits(X[M:frm]), _bits(null[:frm - M]))
        want = (null[frm - M:].double() + v.double()).to(torch.float32).to(torch.bfloat16)
        assert torch.equal(_bits(X[frm:]), _bits(want)), "null rows != rbf(x + v)"
    ref = dit_oracle.rms_norm(X, w, EPS)
    if mod:
        b = torch.arange(X.shape[0]) // RPB
        ref = ref * (1 + tab[b, 1]) + tab[b, 0]
    share = (out != ref).float().mean().item()
    assert share < 1e-3, ("norm output vs oracle", share)
    assert rel_l2(out.float(), ref.float()) < 2e-3


@gpu
@pytest.mark.parametrize("K", [512, 1088])
@pytest.mark.parametrize("M", [125, 250])
@pytest.mark.parametrize("D", [768, 1024, 2048])
def test_deferred_epilogue_in_norm(gpu_device, monkeypatch, D, M, K):
    """Family 4: the production pair gemm(…, defer) → rmsnorm_mod.  By default the split-K GEMM
    leaves its partials and the norm applies the epilogue through RowAdd::part — in
    rmsnorm_mod_kernel<4, 3, 1> at D = 768, rmsnorm_split_kernel with 2 waves per row at 1024 and 4
    at 2048 — and, in the same pass, the null-row constant through RowAdd::v / from (the CFG
    cross-O case; one layout starts v ten rows later, so that rows in between take neither branch
    and must stay as they were).  With ACEHIP_SPLITK_FUSE=0, or when the caller allows no deferral,
    splitk_epilogue_kernel runs the epilogue and the one-row-per-wave norm kernel adds v.  X and
    out must be bit-identical either way: the deferred form is the split-K epilogue's arithmetic.
    MI355X: X rows < M overall ≤ 6.3e-5 (D 768, M 125, K 1088), worst row ≤ 1.3e-3 (one element of
    768); the norm output against the oracle norm of the kernel's X: share ≤ 1.6e-5."""
    for gated in (False, True):
        for mod in (False, True):
            for layout in LAYOUTS:
                X1, out1, d1 = run_gemm_res_norm(gpu_device, M, D, K, gated, mod, layout)
                with knobs(monkeypatch, ACEHIP_SPLITK_FUSE="0"):
                    X0, out0, d0 = run_gemm_res_norm(gpu_device, M, D, K, gated, mod, layout)
                assert d1 == (0 if layout == "null-only" else 1) and d0 == 0, (layout, d1, d0)
                assert torch.equal(_bits(X1), _bits(X0)), ("X: deferred != split-K epilogue kernel", gated, mod, layout)
                assert torch.equal(_bits(out1), _bits(out0)), ("out: deferred != undeferred", gated, mod, layout)
                check_norm_result(M, D, K, gated, mod, layout, X1, out1)


@gpu
def test_null_row_add_without_splitk(gpu_device, monkeypatch):
    """Family 4, no split-K: K = 128 has 2 K-tiles, so the GEMM runs its epilogue in its own tile
    (variant 0) under either setting and RowAdd::v / from runs alone, on the default
    one-row-per-wave rmsnorm_mod_kernel.
    MI355X: X rows < M overall 7.8e-6, worst row 9.8e-4; norm output share 0."""
    M, D, K = 125, 1024, 128
    for gated in (False, True):
        for mod in (False, True):
            X1, out1, d1 = run_gemm_res_norm(gpu_device, M, D, K, gated, mod, "rows+null")
            with knobs(monkeypatch, ACEHIP_SPLITK_FUSE="0"):
                X0, out0, d0 = run_gemm_res_norm(gpu_device, M, D, K, gated, mod, "rows+null")
            assert d1 == 0 and d0 == 0
            assert torch.equal(_bits(X1), _bits(X0)) and torch.equal(_bits(out1), _bits(out0))
            check_norm_result(M, D, K, gated, mod, "rows+null", X1, out1)


# --------------------------------------------------------------- repeatability ---
@gpu
@pytest.mark.parametrize("M,N,K", SPLITK_SHAPES)
def test_splitk_repeatable(gpu_device, M, N, K):
    """Family 5: the split-K workspace is reused from call to call.  Three rounds of the plain and
    the gated GEMM, in place and out of place (ldr != ldc), alternating, each on fresh copies of the inputs:
    every round gives the same bits (gemm_kernel<EPI_PARTIAL> + splitk_epilogue_kernel)."""
    rounds = [[run_gemm_res(gpu_device, M, N, K, RPB, gated, -1, layout)
               for gated in (False, True) for layout in (IN_PLACE, OWN_PITCH)] for _ in range(3)]
    for r in rounds[1:]:
        for a, b in zip(rounds[0], r):
            assert torch.equal(_bits(a), _bits(b))


@gpu
@pytest.mark.parametrize("K", [512, 1088])
@pytest.mark.parametrize("M", [125, 250])
@pytest.mark.parametrize("D", [768, 1024, 2048])
def test_deferred_epilogue_in_norm_repeatable(gpu_device, D, M, K):
    """Family 5 for the pair: three rounds of the plain and the gated GEMM with the modulated norm
    in each of the four layouts (deferred into rmsnorm_mod_kernel / rmsnorm_split_kernel, and
    splitk_epilogue_kernel for the layout without deferral), alternating over the same workspace,
    each on fresh inputs: the same X and out."""
    cfgs = [(gated, True, layout) for gated in (False, True) for layout in LAYOUTS]
    rounds = [[run_gemm_res_norm(gpu_device, M, D, K, *c) for c in cfgs] for _ in range(3)]
    for r in rounds[1:]:
        for (Xa, oa, da), (Xb, ob, db), c in zip(rounds[0], r, cfgs):
            assert da == db == (0 if c[2] == "null-only" else 1)
            assert torch.equal(_bits(Xa), _bits(Xb)) and torch.equal(_bits(oa), _bits(ob))
