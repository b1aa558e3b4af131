"""The key-range split of attention_extend, read on the CPU (no GPU call).

csrc/attn_plan.h attn_extend_plan gives every call its launch: units of 128 stacked rows (the
H/KV heads of a KV head x 128/(H/KV) queries), the 64-key tiles of the pos + n cached keys, and
`parts` key ranges of `tiles_per_part` tiles per unit.  acehip_diag_attn_extend_plan returns it.
The CU count is set through ACEHIP_ATTN_CUS, so nothing here depends on the machine."""
import itertools

import pytest

from conftest import set_knob

from acehip import _ffi

SHAPES = [(1, 16, 8), (2, 2, 1), (1, 8, 2), (3, 4, 4), (16, 16, 8)]
NEW = [1, 31, 64, 129, 200, 512]
POS = [0, 1, 63, 64, 130, 1436, 7680]
SLAB = 128 * 132 * 4          # bytes of one part's partials: 128 rows x (m, l, pad, o[128]) fp32


@pytest.mark.parametrize("cus", [4, 24, 256, 304])
def test_extend_plan_covers_every_tile(monkeypatch, cus):
    set_knob(monkeypatch, "ACEHIP_ATTN_CUS", str(cus))
    for (B, H, KV), n, pos in itertools.product(SHAPES, NEW, POS):
        G = H // KV
        bound = _ffi.lib().acehip_attention_extend_ws_bytes(B, H, n)
        for have_ws in (True, False):
            p = _ffi.attn_extend_plan(B, H, KV, n, pos, have_ws=have_ws)
            what = (cus, B, H, KV, n, pos, have_ws, p)
            assert p["unit_rows"] == 128 and p["unit_queries"] == 128 // G, what
            assert p["qblocks"] == -(-n // p["unit_queries"]) and p["units"] == B * KV * p["qblocks"], what
            assert p["tiles"] == -(-(pos + n) // 64), what
            # every key tile of the longest unit (so of every unit) lies in a part, and no part is empty
            assert p["parts"] >= 1 and p["tiles_per_part"] >= 1, what
            assert p["parts"] * p["tiles_per_part"] >= p["tiles"], what
            assert (p["parts"] - 1) * p["tiles_per_part"] < p["tiles"], what
            assert p["grid"] == p["units"] * p["parts"] and p["block"] == 256, what
            assert p["uses_ws"] == int(p["parts"] > 1), what
            if not have_ws:
                assert p["parts"] == 1 and p["ws_need"] == 0, what
            else:
                # the split stops at one round of the planned CUs, which bounds the partials,
                # and keeps two tiles per part
                assert p["parts"] == 1 or (p["grid"] <= cus and p["tiles_per_part"] >= 2), what
                assert p["ws_need"] == (p["grid"] * SLAB if p["parts"] > 1 else 0), what
                assert p["ws_need"] <= bound, what
        assert bound <= cus * SLAB, (cus, B, H, n, bound)


def test_extend_plan_scoring_shape_splits(monkeypatch):
    """A 64-token target after a 1436-token prompt, B = 1: 8 units on 256 CUs, two tiles per part."""
    set_knob(monkeypatch, "ACEHIP_ATTN_CUS", "256")
    p = _ffi.attn_extend_plan(1, 16, 8, 64, 1436)
    assert p["units"] == 8 and p["tiles"] == 24, p
    assert p["parts"] == 12 and p["tiles_per_part"] == 2 and p["grid"] == 96 and p["uses_ws"] == 1, p
    # 512 new tokens over 8192 keys: 64 units, 4 ranges of 32 tiles: one round of the 256 CUs
    p = _ffi.attn_extend_plan(1, 16, 8, 512, 7680)
    assert (p["units"], p["tiles"], p["parts"], p["tiles_per_part"]) == (64, 128, 4, 32), p


def test_extend_plan_full_grid_does_not_split(monkeypatch):
    """At least `cus` units: one part per unit, no workspace use."""
    set_knob(monkeypatch, "ACEHIP_ATTN_CUS", "24")
    for B, H, KV, n in [(1, 16, 8, 200), (3, 4, 4, 1024), (16, 16, 8, 1), (3, 16, 8, 1)]:
        p = _ffi.attn_extend_plan(B, H, KV, n, 1000)
        assert p["units"] >= 24 and p["parts"] == 1 and p["uses_ws"] == 0 and p["ws_need"] == 0, p
    set_knob(monkeypatch, "ACEHIP_ATTN_CUS", "256")
    p = _ffi.attn_extend_plan(4, 16, 8, 512, 1000)            # 256 units on 256 CUs
    assert p["units"] == 256 and p["parts"] == 1, p
    p = _ffi.attn_extend_plan(2, 16, 8, 512, 1000)            # 128 units: two parts fill the round
    assert p["units"] == 128 and p["parts"] == 2 and p["grid"] == 256, p


def test_extend_plan_refuses_bad_shapes():
    with pytest.raises(RuntimeError):
        _ffi.attn_extend_plan(1, 16, 2, 8, 0)                 # G = 8
    with pytest.raises(RuntimeError):
        _ffi.attn_extend_plan(1, 16, 8, 0, 0)                 # n < 1
    with pytest.raises(RuntimeError):
        _ffi.attn_extend_plan(1, 16, 8, 4, -1)                # pos < 0
