"""acehip_lm_filter on the GPU: the LM's top-k / top-p logit filters against the fixture recorded
from the reference's own methods, against the torch chain and the fp64 contract of
lm_filter_ref.py at the sizes the fixture does not cover, and through install_lm's binding."""
import ctypes
import json
import os

import pytest
import torch

from conftest import GOLDEN, load_golden

import lm_filter_ref as R

pytestmark = pytest.mark.gpu

V_LM = 217204
NEG = float("-inf")


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def _call(buf, V, top_k, top_p, ws=None, ws_bytes=None, B=None, ld=None, dtype=None, logits_ptr=None):
    from acehip import _ffi
    lib = _ffi.lib()
    B = buf.shape[0] if B is None else B
    ld = buf.stride(0) if ld is None else ld
    if ws is None:
        ws = torch.empty(int(lib.acehip_lm_filter_ws_bytes(max(B, 1), max(V, 1))), dtype=torch.uint8, device=buf.device)
    rc = lib.acehip_lm_filter(_ffi.ptr(buf) if logits_ptr is None else logits_ptr,
                              _ffi.dtype_code(buf) if dtype is None else dtype, ld, B, V, top_k, top_p,
                              _ffi.ptr(ws), ws.numel() if ws_bytes is None else ws_bytes, _ffi.stream_ptr())
    return rc


def hip_filter(x, top_k=0, top_p=0.0, pad=5):
    """x [B, V] (CPU or GPU) → filtered copy on the CPU; run with ld = V + pad and sentinel columns,
    which must come back unchanged."""
    B, V = x.shape
    buf = torch.full((B, V + pad), 123.0, dtype=x.dtype, device="cuda")
    buf[:, :V] = x.cuda()
    assert _call(buf, V, top_k, top_p) == 0
    torch.cuda.synchronize()
    out = buf.cpu()
    assert bool((out[:, V:] == 123.0).all()), "columns [V, ld) were written"
    return out[:, :V].contiguous()


def check_top_p(x, y, top_p, tag=""):
    """The contract's properties on every row of y = top_p(x) (CPU tensors); returns the kept counts."""
    ns = []
    for i in range(x.shape[0]):
        xi, yi = x[i], y[i]
        live = torch.isfinite(xi.float())
        kept = torch.isfinite(yi.float())
        want = torch.where(kept, xi, torch.full_like(xi, NEG))
        if not bool(live.any()):
            assert torch.equal(_bits(yi), _bits(xi)), (tag, i, "a row with no finite entry was touched")
            ns.append(0)
            continue
        assert torch.equal(_bits(yi), _bits(want)), (tag, i, "an entry is neither untouched nor -inf")
        assert bool((kept & ~live).sum() == 0)
        n = int(kept.sum())
        assert n >= 1, (tag, i)
        removed = live & ~kept
        xf = xi.float()
        vmin = xf[kept].min()
        if bool(removed.any()):
            assert float(vmin) >= float(xf[removed].max()), (tag, i, "not a top-n set")
        ties = kept[xf == vmin]                                    # in index order
        nk = int(ties.sum())
        assert bool(ties[:nk].all()), (tag, i, "kept ties are not the lowest indices")
        lo, hi = R.band64(xi, top_p)
        print(f"{tag} row {i}: n = {n}, fp64 band [{lo}, {hi}]")
        assert lo <= n <= hi, (tag, i, n, lo, hi)
        ns.append(n)
    return ns


# ------------------------------------------------------------------ fixture replay
@pytest.fixture(scope="module")
def fixture():
    with open(os.path.join(GOLDEN, "lm_filter_manifest.json")) as f:
        return json.load(f), load_golden("lm_filter")


@pytest.mark.parametrize("tag", ["f32", "bf16"])
def test_fixture_replay(gpu_device, fixture, tag):
    manifest, t = fixture
    x = t[f"{tag}.input"]
    for case in manifest["cases"]:
        got = hip_filter(x, top_k=case["top_k"] or 0, top_p=case["top_p"] or 0.0)
        want = t[f"{tag}.{case['name']}"]
        assert torch.equal(_bits(got), _bits(want)), (tag, case["name"],
                                                      [R.kept_count(r) for r in got], [R.kept_count(r) for r in want])


# ------------------------------------------------------------------ shapes
def _rows(B, V, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, V, generator=g) * 3.0
    if V > 8:                                                   # a masked stretch and a masked scatter
        x[0, : V // 3] = NEG
        x[-1][torch.randperm(V, generator=g)[: V // 2]] = NEG
    return x.to(dtype)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("B", [1, 3, 16])
@pytest.mark.parametrize("V", [1, 2, 63, 64, 65, 1024, 4099, V_LM])
def test_shapes(gpu_device, V, B, dtype):
    x = _rows(B, V, dtype, seed=V + B)
    for k in sorted({1, 2, V - 1, V, V + 1}):
        if k < 1:
            continue
        got = hip_filter(x, top_k=k)
        want = R.torch_top_k(x.clone(), k) if k <= V else x
        assert torch.equal(_bits(got), _bits(want)), (V, B, dtype, k)
    check_top_p(x, hip_filter(x, top_p=0.9), 0.9, f"V={V} B={B} {dtype}")


def _special_rows(V, dtype):
    g = torch.Generator().manual_seed(V)
    out = {}
    base = torch.randn(V, generator=g) * 2.0
    dup = base.clone()
    dup[torch.randperm(V, generator=g)[: min(V, 40)]] = 1.25              # duplicated values (threshold ties)
    out["duplicates"] = dup
    lsb = torch.full((V,), 1.0).view(torch.int32) + torch.randint(0, 2, (V,), generator=g, dtype=torch.int32)
    out["lowest_mantissa_bit"] = lsb.view(torch.float32)
    z = base.clone()
    z[0::7] = -0.0
    z[1::7] = 0.0
    z[2::7] = 1e-40
    z[3::7] = -1e-40
    z[4::7] = 1.4e-45
    out["zeros_denormals"] = z
    out["one_bin"] = 1.0 + torch.rand(V, generator=g) * 2.0 ** -10 * 0.999
    out["constant"] = torch.full((V,), 0.5)
    out["all_neg_inf"] = torch.full((V,), NEG)
    one = torch.full((V,), NEG)
    one[V // 2] = -3.0
    out["one_finite"] = one
    dom = base.clone().clamp(max=4.0)
    dom[V // 3] = 40.0
    out["dominant_top"] = dom
    return {k: v.to(dtype) for k, v in out.items()}


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("V", [65, 4099, V_LM])
def test_special_rows_top_k(gpu_device, V, dtype):
    rows = _special_rows(V, dtype)
    names = list(rows)
    x = torch.stack([rows[n] for n in names])
    # top-k: exact, ties at the threshold all kept (k lands inside the duplicated / equal values)
    dup_rank = int((rows["duplicates"].float() > 1.25).sum())
    for k in sorted({1, 2, dup_rank + 1, dup_rank + 2, V // 2, V - 1}):
        if not 1 <= k < V:
            continue
        got = hip_filter(x, top_k=k)
        want = R.torch_top_k(x.clone(), k)
        for i, n in enumerate(names):
            assert torch.equal(_bits(got[i]), _bits(want[i])), (V, dtype, k, n, R.kept_count(got[i]), R.kept_count(want[i]))
    i_dup = names.index("duplicates")
    got = hip_filter(x, top_k=dup_rank + 1)
    assert R.kept_count(got[i_dup]) == dup_rank + int((rows["duplicates"].float() == 1.25).sum())


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("p", [0.9, 0.5])
@pytest.mark.parametrize("V", [65, 4099, V_LM])
def test_special_rows_top_p(gpu_device, V, p, dtype):
    rows = _special_rows(V, dtype)
    names = list(rows)
    x = torch.stack([rows[n] for n in names])
    got = hip_filter(x, top_p=p)
    ns = dict(zip(names, check_top_p(x, got, p, f"V={V} {dtype} p={p}")))
    assert ns["all_neg_inf"] == 0 and ns["one_finite"] == 1 and ns["dominant_top"] == 1
    chain = R.torch_top_p(x.clone(), p)
    for i, n in enumerate(names):
        if n != "all_neg_inf" and R.gapped(x[i], p):
            assert torch.equal(_bits(got[i]), _bits(chain[i])), (V, dtype, p, n)


# ------------------------------------------------------------------ top-p against fp64 at the LM's size
def _lm_rows(dtype):
    rows = {}
    for seed in (0, 1):
        rows[f"flat_s{seed}"] = R.scattered_row(V_LM, 1.0, seed, 150000, dtype)
        rows[f"peaked_s{seed}"] = R.scattered_row(V_LM, 8.0, seed, 150000, dtype)
    rows["codes_flat"] = R.codes_phase_row(V_LM, 1.0, 2, dtype=dtype)
    rows["codes_s4"] = R.codes_phase_row(V_LM, 4.0, 3, dtype=dtype)
    return rows


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("top_p", [0.5, 0.9])
def test_top_p_against_fp64(gpu_device, top_p, dtype):
    rows = _lm_rows(dtype)
    names = list(rows)
    x = torch.stack([rows[n] for n in names])
    got = hip_filter(x, top_p=top_p)
    check_top_p(x, got, top_p, f"hip {dtype} p={top_p}")
    # the torch chain itself (on the GPU, what the loop runs today) meets the same bound
    chain = R.torch_top_p(x.cuda(), top_p).cpu()
    for i, n in enumerate(names):
        lo, hi = R.band64(x[i], top_p)
        nc = R.kept_count(chain[i])
        print(f"torch chain {n} {dtype} p={top_p}: n = {nc}, fp64 band [{lo}, {hi}]")
        assert lo <= nc <= hi, (n, nc, lo, hi)
    for i, n in enumerate(names):
        if n.startswith("peaked"):
            assert R.gapped(x[i], top_p), n                       # σ = 8, seeds 0 and 1: gapped at 0.5 and 0.9
        if R.gapped(x[i], top_p):
            assert torch.equal(_bits(got[i]), _bits(chain[i])), (n, dtype, top_p)


# ------------------------------------------------------------------ composition, determinism
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_composition_equals_two_calls(gpu_device, dtype):
    for V, B in ((4099, 3), (V_LM, 2)):
        x = torch.stack([R.scattered_row(V, 4.0, 10 + b, (V // 2) * (b % 2), dtype) for b in range(B)])
        both = hip_filter(x, top_k=50, top_p=0.9)
        seq = hip_filter(hip_filter(x, top_k=50), top_p=0.9)
        assert torch.equal(_bits(both), _bits(seq))
        assert all(1 <= R.kept_count(r) <= 50 + 8 for r in both)
        if dtype == torch.float32:
            assert torch.equal(_bits(both), _bits(R.torch_top_p(R.torch_top_k(x.clone(), 50), 0.9)))


def test_deterministic(gpu_device):
    flat = R.scattered_row(V_LM, 1.0, 0, 150000)
    x = torch.stack([flat.roll(b) for b in range(16)])
    a = hip_filter(x, top_p=0.9)
    b = hip_filter(x, top_p=0.9)
    assert torch.equal(_bits(a), _bits(b))
    # the same row at every batch position: the same kept count
    assert len({R.kept_count(r) for r in a}) == 1
    xb = torch.full((16, V_LM), 0.5, dtype=torch.bfloat16)              # one tie group: the index-ordered path
    a, b = hip_filter(xb, top_p=0.9), hip_filter(xb, top_p=0.9)
    assert torch.equal(_bits(a), _bits(b))
    k = hip_filter(x, top_k=50)
    assert torch.equal(_bits(k), _bits(hip_filter(x, top_k=50)))


# ------------------------------------------------------------------ arguments
def test_argument_errors(gpu_device):
    from acehip import _ffi
    lib = _ffi.lib()
    V, B = 300, 2
    x = torch.randn(B, V + 5, device="cuda")
    keep = x.clone()
    ws = torch.empty(int(lib.acehip_lm_filter_ws_bytes(B, V)), dtype=torch.uint8, device="cuda")
    assert ws.numel() > 0
    bad = [dict(logits_ptr=ctypes.c_void_p(None)), dict(B=0), dict(ld=V - 1), dict(dtype=2), dict(dtype=-1),
           dict(ws_bytes=ws.numel() - 1), dict(ws_bytes=0)]
    for kw in bad:
        rc = _call(x, V, 5, 0.9, ws=ws, **kw)
        assert rc == -1 and lib.acehip_last_error(), kw
    assert _call(x, 0, 5, 0.9, ws=ws) == -1
    rc = lib.acehip_lm_filter(_ffi.ptr(x), 0, V + 5, B, V, 5, 0.9, None, ws.numel(), _ffi.stream_ptr())
    assert rc == -1
    torch.cuda.synchronize()
    assert torch.equal(x, keep)
    # both filters off: a valid call that launches nothing
    for k, p in ((0, 0.0), (-3, 1.0), (V, 1.5), (V + 7, -0.5)):
        assert _call(x, V, k, p, ws=ws) == 0
    torch.cuda.synchronize()
    assert torch.equal(x, keep)


# ------------------------------------------------------------------ through the binding
def test_through_install_lm(gpu_device):
    from acehip.integration import install_lm
    from test_lm_filter_host import FilterHandler
    from test_lm_host import TorchRuntime, _model
    model = _model()
    h = FilterHandler(model)
    res = install_lm(h, runtime=TorchRuntime(model), filters=True)
    assert "filters" in res
    x = torch.stack([R.scattered_row(V_LM, 4.0, 20 + b, 150000 * (b % 2)) for b in range(2)])
    want = R.torch_top_p(R.torch_top_k(x.clone(), 50), 0.9)
    y = x.cuda()
    got = h._apply_top_p_filter(h._apply_top_k_filter(y, 50), 0.9)
    assert got is y and h.seen == []                              # same object, the originals never ran
    assert torch.equal(_bits(got.cpu()), _bits(want))
    draws = []
    for logits in (got, want.cuda()):
        torch.manual_seed(1234)
        draws.append(torch.multinomial(torch.softmax(logits.float() / 0.85, dim=-1), num_samples=1).squeeze(1))
    assert torch.equal(draws[0], draws[1])
    # bf16 rows run on the kernel too
    yb = x.to(torch.bfloat16).cuda()
    gb = h._apply_top_k_filter(yb, 50)
    assert gb is yb and h.seen == []
    assert torch.equal(_bits(gb.cpu()), _bits(R.torch_top_k(x.to(torch.bfloat16), 50)))
    # a row-strided view (unit inner stride) is filtered in place; a transposed one goes to the original
    wide = torch.full((2, V_LM + 3), 7.0, device="cuda")
    wide[:, :V_LM] = x.cuda()
    view = wide[:, :V_LM]
    assert h._apply_top_k_filter(view, 50) is view and h.seen == []
    assert torch.equal(view.cpu(), R.torch_top_k(x.clone(), 50)) and bool((wide[:, V_LM:] == 7.0).all())
    xt = torch.randn(97, 2, device="cuda").t()                   # [2, 97], inner stride 2
    ref = R.torch_top_k(xt.clone(), 5)
    out = h._apply_top_k_filter(xt, 5)
    assert out is xt and h.seen == [("top_k", 5)] and torch.equal(out, ref)
    for bad in (torch.randn(2, 97, device="cuda", dtype=torch.float16), torch.randn(2, 97, device="cuda").double()):
        h.seen.clear()
        h._apply_top_p_filter(bad, 0.9)
        assert h.seen == [("top_p", 0.9)]
