"""The LM's top-k / top-p filters on the host (no GPU): the fixture recorded from the reference's
own methods (tools/record_lm_filter.py) against the two statements in lm_filter_ref.py, and the
``filters`` switch of acehip.integration.install_lm on a stub handler."""
import json
import os

import pytest
import torch

from conftest import GOLDEN, load_golden

import lm_filter_ref as R
from acehip.integration import install_lm
from acehip.lm import HipLogitFilters
from test_lm_host import StubHandler, TorchRuntime, _model


@pytest.fixture(scope="module")
def fixture():
    with open(os.path.join(GOLDEN, "lm_filter_manifest.json")) as f:
        manifest = json.load(f)
    return manifest, load_golden("lm_filter")


def test_fixture_shape_and_size(fixture):
    manifest, t = fixture
    assert os.path.getsize(os.path.join(GOLDEN, "lm_filter.safetensors")) < 1000000
    assert manifest["V"] == 4099 and manifest["delta"] == R.DELTA == 1e-4
    assert {c["top_k"] for c in manifest["cases"]} == {None, 1, 50, 4098}
    assert {c["top_p"] for c in manifest["cases"]} == {None, 0.9, 0.5, 0.05}
    for tag, dt in (("f32", torch.float32), ("bf16", torch.bfloat16)):
        x = t[f"{tag}.input"]
        assert x.dtype == dt and x.shape == (len(manifest["rows"]), 4099)
        finite = torch.isfinite(x.float()).sum(1).tolist()
        assert finite == manifest["dtypes"][tag]["finite"]
        assert 1 in finite and 4099 - 3000 in finite          # the single-entry row, the pre-masked row


def test_fp32_chain_reproduces_the_fixture(fixture):
    manifest, t = fixture
    for tag in manifest["dtypes"]:
        x = t[f"{tag}.input"]
        for case in manifest["cases"]:
            want = t[f"{tag}.{case['name']}"]
            y = x.clone()
            got = R.torch_top_k(y, case["top_k"]) if case["top_k"] is not None else R.torch_top_p(y, case["top_p"])
            assert got is y
            # bit for bit: kept entries keep their bits, removed ones are −inf
            assert torch.equal(got.view(torch.int16 if got.dtype == torch.bfloat16 else torch.int32),
                               want.view(torch.int16 if want.dtype == torch.bfloat16 else torch.int32)), (tag, case)
            kept = torch.isfinite(want.float())
            assert torch.equal(want[kept], x[kept]) and bool(torch.isneginf(want[~kept].float()).all())


def test_fp64_mask_agrees_on_gapped_rows(fixture):
    manifest, t = fixture
    for tag in manifest["dtypes"]:
        x = t[f"{tag}.input"]
        for case in manifest["cases"]:
            if case["top_p"] is None:
                continue
            want = t[f"{tag}.{case['name']}"]
            for i in range(x.shape[0]):
                assert R.gapped(x[i], case["top_p"]), (tag, case, i)
                assert torch.equal(torch.isfinite(want[i].float()), R.mask64(x[i], case["top_p"])), (tag, case, i)
                assert R.n64(x[i], case["top_p"]) == manifest["dtypes"][tag]["kept"][case["name"]][i]


def test_fp64_helpers_on_small_rows():
    row = torch.tensor([0.0, 2.0, 2.0, float("-inf"), 1.0])
    # p ≈ [.0537, .3969, .3969, 0, .1460]; ranks: 1, 2, 4, 0, 3
    assert R.n64(row, 0.3) == 1 and R.n64(row, 0.5) == 2 and R.n64(row, 0.9) == 3 and R.n64(row, 0.95) == 4
    assert R.mask64(row, 0.3).tolist() == [False, True, False, False, False]     # equal values: lower index first
    assert R.mask64(row, 0.9).tolist() == [False, True, True, False, True]
    assert not R.gapped(row, 0.3) and R.gapped(row, 0.5) and R.gapped(row, 0.9)
    dead = torch.full((4,), float("-inf"))
    assert R.n64(dead, 0.9) == 0 and R.mask64(dead, 0.9) is None
    assert torch.equal(R.torch_top_p(dead[None].clone(), 0.9)[0], dead)            # the chain removes nothing there


class FilterHandler(StubHandler):
    """StubHandler plus the two filter methods, as LLMHandler has them; calls are recorded."""

    def __init__(self, model, backend="pt"):
        super().__init__(model, backend)
        self.seen = []

    def _apply_top_k_filter(self, logits, top_k):
        self.seen.append(("top_k", top_k))
        return R.torch_top_k(logits, top_k)

    def _apply_top_p_filter(self, logits, top_p):
        self.seen.append(("top_p", top_p))
        return R.torch_top_p(logits, top_p)


def test_install_lm_filters_switch():
    model = _model()
    h = FilterHandler(model)
    orig_k, orig_p = h._apply_top_k_filter, h._apply_top_p_filter
    res = install_lm(h, runtime=TorchRuntime(model), filters=True)
    f = res["filters"]["hip"]
    assert isinstance(f, HipLogitFilters)
    assert res["filters"]["top_k"] == orig_k and res["filters"]["top_p"] == orig_p
    assert h._apply_top_k_filter == f.top_k and h._apply_top_p_filter == f.top_p
    assert "_apply_top_p_filter" in vars(h) and "_apply_top_k_filter" in vars(h)      # bound on the instance
    # a CPU tensor goes to the original and returns its result
    g = torch.Generator().manual_seed(1)
    x = torch.randn(2, 97, generator=g) * 4
    want = R.torch_top_p(R.torch_top_k(x.clone(), 5), 0.9)
    y = x.clone()
    got = h._apply_top_p_filter(h._apply_top_k_filter(y, 5), 0.9)
    assert got is y and torch.equal(got, want)
    assert h.seen == [("top_k", 5), ("top_p", 0.9)]
    # a disabled filter returns the input untouched
    for off in (None, 0, 1.0):
        y = x.clone()
        assert h._apply_top_p_filter(y, off) is y and torch.equal(y, x)
    for off in (None, 0):
        y = x.clone()
        assert h._apply_top_k_filter(y, off) is y and torch.equal(y, x)


def test_install_lm_filters_off_by_default():
    model = _model()
    h = FilterHandler(model)
    res = install_lm(h, runtime=TorchRuntime(model))
    assert "filters" not in res
    assert "_apply_top_p_filter" not in vars(h) and "_apply_top_k_filter" not in vars(h)
    assert h._apply_top_p_filter.__func__ is FilterHandler._apply_top_p_filter
    res = install_lm(FilterHandler(model), runtime=TorchRuntime(model), filters=False)
    assert "filters" not in res


def test_install_lm_filters_skipped_installs_bind_nothing():
    model = _model()
    h = FilterHandler(model, backend="vllm")
    res = install_lm(h, runtime=TorchRuntime(model), filters=True)
    assert res["lm"] is None and "filters" not in res
    assert "_apply_top_p_filter" not in vars(h) and "_apply_top_k_filter" not in vars(h)
    # a handler without the methods: the LM is installed, the filters are not
    h = StubHandler(model)
    res = install_lm(h, runtime=TorchRuntime(model), filters=True)
    assert res["lm"] is not None and "filters" not in res and not hasattr(h, "_apply_top_p_filter")


def test_filter_errors_follow_the_fallback_policy(monkeypatch):
    """An acehip error inside a filter call: raised by default, logged and served by the original
    with fallback=True (the eligibility test is bypassed: there is no GPU here)."""
    x = torch.randn(2, 97, generator=torch.Generator().manual_seed(2)) * 4

    def boom(self, logits, top_k, top_p):
        raise RuntimeError("acehip lm_filter failed (-3): injected")
    monkeypatch.setattr(HipLogitFilters, "_run", boom)
    monkeypatch.setattr(HipLogitFilters, "eligible", staticmethod(lambda t: True))
    strict = HipLogitFilters(R.torch_top_k, R.torch_top_p)
    with pytest.raises(RuntimeError, match="injected"):
        strict.top_p(x.clone(), 0.9)
    soft = HipLogitFilters(R.torch_top_k, R.torch_top_p, fallback=True)
    y = x.clone()
    assert soft.top_p(y, 0.9) is y and torch.equal(y, R.torch_top_p(x.clone(), 0.9))
    y = x.clone()
    assert soft.top_k(y, 5) is y and torch.equal(y, R.torch_top_k(x.clone(), 5))
