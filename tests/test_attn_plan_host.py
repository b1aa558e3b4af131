"""The route of the attention dispatch, read on the CPU (no GPU call).

attention() plans every launch with csrc/attn_plan.h before it launches; acehip_diag_attn_plan
returns that plan for a shape under the ACEHIP_ATTN_* switches of the environment.  Every row below
was derived by hand from the dispatch rules as they stood before the planner was separated from the
launch, so a planner edit that reroutes one of these shapes fails here, before any kernel runs.
device_cus is always 256, so the table does not depend on the machine; ACEHIP_ATTN_CUS ("cus")
replaces the CU count the rules plan for.  Units are 128 query rows of a GQA pair (pw, fwd<2>), of
one head (fwd<1>), or 32 query rows of one head (small); a KV tile is 64 keys.
"""
import pytest

from conftest import set_knob

from acehip import _ffi
from acehip._ffi import ATTN_FWD, ATTN_PW, ATTN_SMALL


def small(units, parts, **kw):
    return dict(kernel=ATTN_SMALL, nrep=1, units=units, parts=parts, grid=units * parts, block=256, full=0, nsplit=0,
                uses_ws=int(parts > 1), **kw)


def _units(kernel, nrep, units, full, nsplit, **kw):
    want = dict(kernel=kernel, nrep=nrep, units=units, full=full, nsplit=nsplit, grid=full + (units - full) * nsplit,
                block=512 if (kernel, nrep) == (ATTN_FWD, 2) else 256, uses_ws=int(nsplit > 1), streamk=0, persist=0,
                parts=0)
    want.update(kw)
    return want


def fwd(nrep, units, **kw):
    """attn_fwd_kernel<nrep>, whole units"""
    return _units(ATTN_FWD, nrep, units, units, 1, **kw)


def fwd_split(units, full, nsplit, **kw):
    """attn_fwd_kernel<2>: units [0, full) whole, the rest as nsplit KV-range parts (full 0: the short split)"""
    return _units(ATTN_FWD, 2, units, full, nsplit, **kw)


def streamk(units, tiles, grid):
    return _units(ATTN_FWD, 2, units, units, 1, streamk=1, sk_nt=tiles, sk_total=units * tiles, unit_tiles=tiles,
                  grid=grid, uses_ws=1)


def pw(units, **kw):
    return _units(ATTN_PW, 2, units, units, 1, **kw)


def pw_split(units, full, nsplit, **kw):
    return _units(ATTN_PW, 2, units, full, nsplit, **kw)


def pw_walk(units, grid, **kw):
    return _units(ATTN_PW, 2, units, units, 1, persist=1, grid=grid, **kw)


TAIL = (2, 4, 2, 700, 1600, -1)     # 24 units of 25 tiles
SHORT = (1, 4, 2, 257, 641, -1)     # 6 units of 11 tiles

# (switches, ACEHIP_ATTN_CUS or None, (B, H, KV, Sq, Sk, window), masked, expected fields)
# --- every (shape, cus, switches) tuple a GPU attention test launches
GPU_TEST_ROWS = [
    # tests/test_gpu_dit.py test_attention_tail_split: tail 8 / 6 / 4 of 24 units -> 2, 3, 4 parts each
    *[({"ACEHIP_ATTN_PW": 7}, cus, TAIL, 0, pw_split(24, cus, n, unit_tiles=25))
      for cus, n in ((16, 2), (18, 3), (20, 4))],
    *[({"ACEHIP_ATTN_PW": 0, "ACEHIP_ATTN_STREAMK": 0}, cus, TAIL, 0, fwd_split(24, cus, n, unit_tiles=25))
      for cus, n in ((16, 2), (18, 3), (20, 4))],
    *[({"ACEHIP_ATTN_PW": 0}, cus, TAIL, 0, streamk(24, 25, cus)) for cus in (16, 18, 20)],   # stream-K overrides the split
    # test_attention_small, ACEHIP_ATTN_SMALL = 1 and 2
    ({}, None, (1, 16, 8, 125, 641, -1), 0, small(64, 3, unit_tiles=11)),
    ({}, None, (1, 16, 8, 125, 125, -1), 0, small(64, 1)),
    ({}, None, (2, 16, 8, 125, 641, -1), 0, small(128, 2)),
    ({}, None, (1, 16, 8, 1, 641, -1), 0, small(16, 3)),
    ({}, None, (1, 2, 1, 33, 65, -1), 0, small(4, 1)),
    ({}, None, (3, 4, 2, 77, 1000, -1), 0, small(36, 4)),
    ({}, None, (1, 16, 16, 200, 2000, -1), 0, small(112, 2)),
    ({}, 100, (1, 16, 8, 125, 641, -1), 0, small(64, 1)),
    ({}, 64, (1, 4, 2, 31, 3000, -1), 0, small(4, 12)),
    ({}, None, (1, 2, 1, 40, 1, -1), 0, small(4, 1)),
    *[({"ACEHIP_ATTN_SMALL": 2}, cus, shape, 0, small(units, 1))
      for cus, shape, units in ((None, (1, 16, 8, 125, 641, -1), 64), (None, (1, 16, 8, 125, 125, -1), 64),
                                (None, (2, 16, 8, 125, 641, -1), 128), (None, (1, 16, 8, 1, 641, -1), 16),
                                (None, (1, 2, 1, 33, 65, -1), 4), (None, (3, 4, 2, 77, 1000, -1), 36),
                                (None, (1, 16, 16, 200, 2000, -1), 112), (100, (1, 16, 8, 125, 641, -1), 64),
                                (64, (1, 4, 2, 31, 3000, -1), 4), (None, (1, 2, 1, 40, 1, -1), 4))],
    # test_attention_band_persistent (ACEHIP_ATTN_PW = 2), ACEHIP_ATTN_PERSIST = 1 and 0: only grids of
    # more units than CUs walk
    ({"ACEHIP_ATTN_PW": 2}, 16, (2, 4, 2, 1000, 1000, 128), 0, pw_walk(32, 16, unit_tiles=7)),
    ({"ACEHIP_ATTN_PW": 2}, 37, (2, 4, 2, 1000, 1000, 128), 0, pw(32, unit_tiles=7)),
    ({"ACEHIP_ATTN_PW": 2}, 100, (1, 16, 8, 777, 777, 64), 0, pw(56, unit_tiles=5)),
    ({"ACEHIP_ATTN_PW": 2}, 7, (1, 2, 1, 450, 450, 200), 0, pw(4, unit_tiles=9)),
    ({"ACEHIP_ATTN_PW": 2}, None, (2, 16, 8, 3000, 3000, 128), 0, pw_walk(384, 256, unit_tiles=7)),
    ({"ACEHIP_ATTN_PW": 2}, None, (4, 16, 8, 3000, 3000, 128), 0, pw_walk(768, 256, unit_tiles=7)),
    *[({"ACEHIP_ATTN_PW": 2, "ACEHIP_ATTN_PERSIST": 0}, cus, shape, 0, pw(units))
      for cus, shape, units in ((16, (2, 4, 2, 1000, 1000, 128), 32), (37, (2, 4, 2, 1000, 1000, 128), 32),
                                (100, (1, 16, 8, 777, 777, 64), 56), (7, (1, 2, 1, 450, 450, 200), 4),
                                (None, (2, 16, 8, 3000, 3000, 128), 384), (None, (4, 16, 8, 3000, 3000, 128), 768))],
    # test_attention: rows whose route is the same under ACEHIP_ATTN_PW = 0 and 7 ...
    *[({"ACEHIP_ATTN_PW": p}, None, shape, 0, want) for p in (0, 7) for shape, want in (
        ((2, 4, 2, 300, 300, -1), small(80, 2)),
        ((2, 4, 2, 257, 641, -1), small(72, 3)),
        ((1, 2, 1, 50, 20, -1), small(4, 1)),
        ((1, 16, 8, 125, 641, -1), small(64, 3)),
        ((1, 16, 8, 125, 125, 128), small(64, 1, window=-1)),           # a band wider than the sequence: full
        ((2, 16, 8, 128, 128, -2), small(128, 1, causal=1)),
        ((1, 16, 8, 77, 77, -2), small(48, 1, causal=1)),
        ((3, 4, 2, 300, 300, -2), small(120, 2, causal=1)),
        ((1, 2, 2, 257, 257, -2), small(18, 2, causal=1)))],
    # ... and the rows that ACEHIP_ATTN_PW moves between attn_fwd_kernel and attn_pw_kernel
    ({"ACEHIP_ATTN_PW": 0}, None, (2, 4, 2, 300, 300, 8), 0, fwd(2, 12, unit_tiles=3, window=8)),
    ({"ACEHIP_ATTN_PW": 7}, None, (2, 4, 2, 300, 300, 8), 0, pw(12, unit_tiles=3)),
    ({"ACEHIP_ATTN_PW": 0}, None, (1, 16, 8, 1000, 1000, 128), 0, fwd(2, 64, unit_tiles=7)),
    ({"ACEHIP_ATTN_PW": 7}, None, (1, 16, 8, 1000, 1000, 128), 0, pw(64, unit_tiles=7)),
    ({"ACEHIP_ATTN_PW": 0}, None, (1, 2, 1, 3000, 3000, 128), 0, fwd(2, 24)),
    ({"ACEHIP_ATTN_PW": 7}, None, (1, 2, 1, 3000, 3000, 128), 0, pw(24)),
    ({"ACEHIP_ATTN_PW": 0}, None, (2, 16, 8, 3000, 3000, -1), 0, streamk(384, 47, 256)),
    ({"ACEHIP_ATTN_PW": 7}, None, (2, 16, 8, 3000, 3000, -1), 0, pw_split(384, 256, 2)),
    ({"ACEHIP_ATTN_PW": 0}, None, (2, 16, 8, 3000, 3000, 128), 0, fwd(1, 768, unit_tiles=7)),
    ({"ACEHIP_ATTN_PW": 7}, None, (2, 16, 8, 3000, 3000, 128), 0, pw_walk(384, 256)),
    ({"ACEHIP_ATTN_PW": 0}, None, (2, 16, 8, 3000, 641, -1), 0, fwd(1, 768, unit_tiles=11)),
    ({"ACEHIP_ATTN_PW": 7}, None, (2, 16, 8, 3000, 641, -1), 0, pw(384, unit_tiles=11)),
    # test_attention_short_split
    ({}, None, (1, 16, 8, 1000, 641, -1), 0, fwd_split(64, 0, 4, unit_tiles=11)),
    ({"ACEHIP_ATTN_SMALL": 0, "ACEHIP_ATTN_PW": 0}, None, SHORT, 0, fwd_split(6, 0, 4, unit_tiles=11)),
    ({"ACEHIP_ATTN_SMALL": 0, "ACEHIP_ATTN_PW": 0}, 16, SHORT, 0, fwd_split(6, 0, 2)),
    ({"ACEHIP_ATTN_SMALL": 0, "ACEHIP_ATTN_PW": 7}, None, SHORT, 0, pw_split(6, 0, 4, unit_tiles=11)),
    ({"ACEHIP_ATTN_SMALL": 0, "ACEHIP_ATTN_PW": 7}, 16, SHORT, 0, pw_split(6, 0, 2)),
    # test_attention_streamk (ACEHIP_ATTN_PW = 2, ACEHIP_ATTN_STREAMK = 1); 384 units on 384 CUs are one whole round
    ({}, 16, (2, 4, 2, 700, 1600, -1), 0, streamk(24, 25, 16)),
    ({}, 20, (2, 4, 2, 700, 3100, -1), 0, streamk(24, 49, 20)),
    ({}, None, (2, 16, 8, 3000, 3000, -1), 0, streamk(384, 47, 256)),
    ({}, None, (2, 16, 8, 7500, 7500, -1), 0, streamk(944, 118, 256)),
    ({}, 7, (1, 4, 2, 1000, 1700, -1), 0, streamk(16, 27, 7)),
    ({}, 3, (1, 2, 1, 450, 1600, -1), 0, streamk(4, 25, 3)),
    ({}, 512, (2, 16, 8, 7500, 7500, -1), 0, streamk(944, 118, 512)),
    ({}, 384, (2, 16, 8, 3000, 3000, -1), 0, fwd(2, 384, unit_tiles=47)),
    # test_graph_replay_single_streamk_layer: the tiny DiT's full layer at S = 1600, two rows
    ({}, 7, (2, 2, 1, 1600, 1600, -1), 0, streamk(26, 25, 7)),
    # tests/test_gpu_cross_fused.py test_forward_knob_bit_equal: the tiny DiT's cross-attention, whole units
    ({}, 4, (2, 2, 1, 192, 70, -1), 0, fwd(2, 4, unit_tiles=2)),
    # tests/test_gpu_condenc.py test_masked_attention_small, ACEHIP_ATTN_SMALL_MASK = 1 and 0
    ({}, None, (2, 16, 8, 300, 300, -1), 1, small(320, 1)),
    ({}, None, (2, 2, 1, 1000, 1000, -1), 1, small(128, 2)),
    ({}, None, (2, 4, 2, 77, 77, -1), 1, small(24, 1)),
    ({}, None, (2, 16, 16, 250, 250, -1), 1, small(256, 1)),
    ({"ACEHIP_ATTN_SMALL_MASK": 0}, None, (2, 16, 8, 300, 300, -1), 1, fwd_split(48, 0, 2, unit_tiles=5)),
    ({"ACEHIP_ATTN_SMALL_MASK": 0}, None, (2, 2, 1, 1000, 1000, -1), 1, fwd_split(16, 0, 6, unit_tiles=16)),
    ({"ACEHIP_ATTN_SMALL_MASK": 0}, None, (2, 4, 2, 77, 77, -1), 1, fwd(2, 4, unit_tiles=2)),
    ({"ACEHIP_ATTN_SMALL_MASK": 0}, None, (2, 16, 16, 250, 250, -1), 1, fwd(1, 64, unit_tiles=4)),
    # test_causal_attention_small, ACEHIP_ATTN_SMALL_CAUSAL = 0 (= 1: test_attention's causal rows above,
    # and (2, 16, 8, 77) below)
    ({}, None, (2, 16, 8, 77, 77, -2), 0, small(96, 1, causal=1)),
    ({"ACEHIP_ATTN_SMALL_CAUSAL": 0}, None, (1, 16, 8, 128, 128, -2), 0, fwd(2, 8, causal=1, window=-2)),
    ({"ACEHIP_ATTN_SMALL_CAUSAL": 0}, None, (2, 16, 8, 77, 77, -2), 0, fwd(2, 16, causal=1)),
    ({"ACEHIP_ATTN_SMALL_CAUSAL": 0}, None, (3, 4, 2, 300, 300, -2), 0, fwd(2, 18, causal=1, unit_tiles=5)),
    ({"ACEHIP_ATTN_SMALL_CAUSAL": 0}, None, (1, 2, 2, 257, 257, -2), 0, fwd(1, 6, causal=1)),
]

# --- production shapes on 256 CUs, default switches: S = 12.5 patches per second, 641 encoder tokens,
# 16 heads on 8 KV heads, window 128; one or two conditional rows
PRODUCTION_ROWS = [
    ({}, None, (2, 16, 8, 3000, 3000, -1), 0, streamk(384, 47, 256)),                 # 240 s full
    ({}, None, (2, 16, 8, 3000, 3000, 128), 0, pw_walk(384, 256, unit_tiles=7)),      # 240 s band
    ({}, None, (1, 16, 8, 3000, 641, -1), 0, fwd(2, 192, unit_tiles=11)),             # 240 s cross, one row: the fused-cross case
    ({}, None, (2, 16, 8, 3000, 641, -1), 0, fwd(1, 768, unit_tiles=11)),             # 240 s cross, two rows
    ({}, None, (1, 16, 8, 3000, 3000, -1), 0, fwd(2, 192, unit_tiles=47)),            # 240 s full, one row
    ({}, None, (1, 16, 8, 3000, 3000, 128), 0, pw(192, unit_tiles=7)),                # 240 s band, one row
    ({}, None, (1, 16, 8, 125, 641, -1), 0, small(64, 3)),                            # turbo 10 s cross
    ({}, None, (1, 16, 8, 125, 125, -1), 0, small(64, 1)),                            # turbo 10 s full
    ({}, None, (1, 16, 8, 125, 125, 128), 0, small(64, 1, window=-1)),                # turbo 10 s band
    ({}, None, (1, 16, 8, 1250, 641, -1), 0, fwd_split(80, 0, 3, unit_tiles=11)),     # 100 s cross, one row: short split
    ({}, None, (2, 16, 8, 1250, 641, -1), 0, fwd(2, 160, unit_tiles=11)),             # 100 s cross, two rows
]

# --- one row per switch's other arm (ACEHIP_ATTN_PW and ACEHIP_ATTN_CUS: the rows above)
OFF_ARM_ROWS = [
    ({"ACEHIP_ATTN_PW": 0}, None, (2, 16, 8, 3000, 3000, 128), 0, fwd(1, 768)),
    ({"ACEHIP_ATTN_PERSIST": 0}, None, (2, 16, 8, 3000, 3000, 128), 0, pw(384)),
    ({"ACEHIP_ATTN_STREAMK": 0}, None, (2, 16, 8, 3000, 3000, -1), 0, fwd_split(384, 256, 2, unit_tiles=47)),
    ({"ACEHIP_ATTN_SMALL": 0}, None, (1, 16, 8, 125, 641, -1), 0, fwd_split(8, 0, 4, unit_tiles=11)),
    ({"ACEHIP_ATTN_SMALL": 2}, None, (1, 16, 8, 125, 641, -1), 0, small(64, 1)),
    ({"ACEHIP_ATTN_SMALL_MASK": 0}, None, (2, 16, 8, 300, 300, -1), 1, fwd_split(48, 0, 2)),
    ({"ACEHIP_ATTN_SMALL_CAUSAL": 0}, None, (1, 16, 8, 128, 128, -2), 0, fwd(2, 8, causal=1)),
]

# --- without the split workspace: whole units, no parts
NO_WS_ROWS = [
    ((2, 16, 8, 3000, 3000, -1), fwd(2, 384)),
    ((1, 16, 8, 1250, 641, -1), fwd(2, 80)),
    ((1, 16, 8, 125, 641, -1), small(64, 1)),
]


def _plan(monkeypatch, knobs, cus, shape, masked, **kw):
    for name, value in knobs.items():
        set_knob(monkeypatch, name, value)
    if cus is not None:
        set_knob(monkeypatch, "ACEHIP_ATTN_CUS", cus)
    return _ffi.attn_plan(*shape, masked=bool(masked), device_cus=256, **kw)


def _assert_plan(got, want, what):
    assert {k: got[k] for k in want} == want, (what, got)


@pytest.mark.parametrize("knobs,cus,shape,masked,want", GPU_TEST_ROWS + PRODUCTION_ROWS + OFF_ARM_ROWS)
def test_routes(monkeypatch, knobs, cus, shape, masked, want):
    _assert_plan(_plan(monkeypatch, knobs, cus, shape, masked), want, (knobs, cus, shape, masked))


@pytest.mark.parametrize("shape,want", NO_WS_ROWS)
def test_without_workspace(monkeypatch, shape, want):
    _assert_plan(_plan(monkeypatch, {}, None, shape, 0, have_ws=False), want, shape)


def test_unused_fields_are_zero(monkeypatch):
    got = _plan(monkeypatch, {}, None, (1, 16, 8, 3000, 641, -1), 0)
    assert got == dict(kernel=ATTN_FWD, nrep=2, window=-1, units=192, unit_tiles=11, full=192, nsplit=1, parts=0,
                       grid=192, block=512, persist=0, streamk=0, sk_nt=0, sk_total=0, causal=0, uses_ws=0)
    got = _plan(monkeypatch, {}, None, (1, 16, 8, 125, 641, -1), 0)
    assert got == dict(kernel=ATTN_SMALL, nrep=1, window=-1, units=64, unit_tiles=11, full=0, nsplit=0, parts=3,
                       grid=192, block=256, persist=0, streamk=0, sk_nt=0, sk_total=0, causal=0, uses_ws=1)


def test_shapes_the_dispatch_refuses():
    # empty batches / sequences, heads that are no multiple of the KV heads, and — off
    # attn_small_kernel — more than two heads per KV head
    for shape in [(0, 16, 8, 125, 125, -1), (1, 16, 8, 0, 125, -1), (1, 16, 8, 125, 0, -1), (1, 16, 0, 125, 125, -1),
                  (1, 16, 3, 125, 125, -1), (2, 4, 1, 3000, 3000, -1), (1, 8, 2, 3000, 3000, 128)]:
        with pytest.raises(RuntimeError, match="diag_attn_plan"):
            _ffi.attn_plan(*shape, device_cus=256)
