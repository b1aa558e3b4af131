"""The route of the production GEMM dispatch, read on the CPU (no GPU call).

gemm() plans every launch with csrc/gemm_plan.h before it launches; acehip_diag_gemm_plan returns
that plan for a shape under the ACEHIP_* switches of the environment.  Every row below was derived
by hand from the dispatch rules as they stood before the planner was separated from the launches
(the rows of the first group are the arithmetic the GPU tests used to walk in their docstrings), so
a planner edit that reroutes one of these shapes fails here, before any kernel runs.  device_cus is
always 256, so the table does not depend on the machine; ACEHIP_GEMM_CUS ("cap") lowers the CU
count that the tile planner fills.
"""
import pytest

from conftest import set_knob

from acehip import _ffi
from acehip._ffi import ROUTE_SPLITK, ROUTE_STAGED, ROUTE_TAIL1, ROUTE_TAIL2, ROUTE_TILE, ROUTE_WALK

STORE, GATED, RES, SWIGLU, HEADPOST = range(5)


def tile(v, **kw):
    return dict(route=ROUTE_TILE, v_head=v, **kw)


def walk(M1, nmain, ntail, grid):
    return dict(route=ROUTE_WALK, M1=M1, nmain=nmain, ntail=ntail, grid=grid, saddr=1)


def tail1(M1, nmain, ntail, **kw):
    return dict(route=ROUTE_TAIL1, v_head=7, v_tail=9, M1=M1, nmain=nmain, ntail=ntail, grid=nmain + ntail, **kw)


def tail2(M1, v_head, v_tail, **kw):
    return dict(route=ROUTE_TAIL2, M1=M1, v_head=v_head, v_tail=v_tail, **kw)


def splitk(splits, kper, bn=64, **kw):
    return dict(route=ROUTE_SPLITK, splits=splits, kper=kper, bn=bn, **kw)


# (M, N, K, epilogue, cap or None, expected fields)
# --- the (shape, cap) pairs the GPU tests launch: K <= 448, default switches
GPU_TEST_ROWS = [
    # tests/test_gpu_gemm_persistent.py
    (768, 512, 128, SWIGLU, 2, walk(768, 6, 0, 2)),
    (768, 512, 64, SWIGLU, 2, walk(768, 6, 0, 2)),
    (1990, 512, 192, SWIGLU, 7, walk(1792, 14, 4, 7)),
    (1030, 768, 256, SWIGLU, 4, walk(1030, 15, 0, 4)),
    (1286, 768, 128, SWIGLU, 4, walk(1280, 15, 3, 4)),
    (700, 512, 192, SWIGLU, 4, tile(8)),
    (520, 768, 64, SWIGLU, 2, tile(8)),
    (1030, 512, 256, SWIGLU, 3, tile(8)),
    (300, 512, 128, SWIGLU, 8, tile(0)),
    # tests/test_gpu_gemm_saddr.py
    (1200, 1024, 64, STORE, 8, tail1(1024, 16, 8, saddr=1)),
    (1200, 1024, 256, STORE, 8, tail1(1024, 16, 8, saddr=1)),
    (1200, 1024, 448, STORE, 8, tail1(1024, 16, 8, saddr=1)),
    (1200, 1024, 128, HEADPOST, 8, dict(route=ROUTE_STAGED, v_head=0, grid=80)),
    (1200, 1024, 128, HEADPOST, None, dict(route=ROUTE_STAGED, v_head=0, grid=80)),
    (8400, 2048, 128, HEADPOST, 64, tail1(8192, 256, 16)),
    # tests/test_gpu_gemm_residual.py
    (300, 512, 128, RES, None, tile(0)),
    (300, 512, 128, GATED, 6, tile(9)),
    (1100, 512, 128, RES, 8, tile(8)),
    (2400, 256, 128, GATED, 4, tile(7)),
    (1100, 512, 128, STORE, 8, tail2(768, 8, 9, nmain=8, ntail=6)),
    (2400, 256, 128, STORE, 4, tail1(2048, 8, 3)),
] + [(M, N, 512, epi, None, splitk(2, 4, deferred=0)) for M in (125, 250) for N in (256, 2048) for epi in (RES, GATED)] \
  + [(M, N, 1088, epi, None, splitk(4, 5, deferred=0)) for M in (125, 250) for N in (256, 2048) for epi in (RES, GATED)]

# --- the 240 s song (S = 3000 patches, two CFG rows) on 256 CUs, D = 2048
SONG_240S_ROWS = [
    (6000, 4096, 2048, HEADPOST, None, tail1(4096, 256, 240, saddr=1)),           # QKV
    (3000, 4096, 2048, HEADPOST, None, tile(8, saddr=0, grid=256)),                # layer 0's deduplicated QKV
    (6000, 2048, 2048, GATED, None, tile(8, saddr=1, grid=256)),                   # O
    (6000, 2048, 6144, GATED, None, tile(8, saddr=1, grid=256)),                   # down
    (6000, 12288, 2048, SWIGLU, None, walk(5376, 1008, 240, 256)),                 # gate / up
    (3000, 2048, 2048, HEADPOST, None, tile(13, helpers=1, grid=256)),             # cross-Q
    (3000, 2048, 2048, GATED, None, tile(13, helpers=1, grid=256)),                # cross-O
]

# --- short songs (turbo 10 s: M = 125; 20 s with CFG: M = 500)
SHORT_ROWS = [
    (125, 12288, 2048, SWIGLU, None, tile(17, helpers=1)),
    (125, 2048, 2048, GATED, None, splitk(8, 4, stages=3)),
    (125, 4096, 2048, HEADPOST, None, splitk(4, 8, stages=3)),
    (500, 12288, 2048, SWIGLU, None, tile(9, grid=192)),
    (500, 4096, 2048, HEADPOST, None, dict(route=ROUTE_STAGED, v_head=0)),
    (500, 2048, 2048, GATED, None, splitk(2, 16, stages=3)),
]


def _plan(monkeypatch, M, N, K, epi, cap, knobs=None, **kw):
    for name, value in (knobs or {}).items():
        set_knob(monkeypatch, name, value)
    if cap is not None:
        set_knob(monkeypatch, "ACEHIP_GEMM_CUS", cap)
    return _ffi.gemm_plan(M, N, K, epi, device_cus=256, **kw)


def _assert_plan(got, want, what):
    assert {k: got[k] for k in want} == want, (what, got)


@pytest.mark.parametrize("M,N,K,epi,cap,want", GPU_TEST_ROWS + SONG_240S_ROWS + SHORT_ROWS)
def test_default_switches(monkeypatch, M, N, K, epi, cap, want):
    _assert_plan(_plan(monkeypatch, M, N, K, epi, cap), want, (M, N, K, epi, cap))


# one row per A/B switch's other arm: (switches, M, N, K, epilogue, cap, keyword arguments, expected)
OFF_ARM_ROWS = [
    # 14 main tiles are no multiple of 8: without the walk the split takes two launches
    ({"ACEHIP_GEMM_PERSIST": 0}, 1990, 512, 192, SWIGLU, 7, {}, tail2(1792, 7, 9, nmain=14, ntail=4, saddr=1)),
    ({"ACEHIP_GEMM_PERSIST": 0}, 6000, 12288, 2048, SWIGLU, None, {}, tail1(5376, 1008, 240, saddr=1)),
    ({"ACEHIP_GEMM_PERSIST": 0}, 768, 512, 128, SWIGLU, 2, {}, tile(7, grid=6, saddr=1)),
    ({"ACEHIP_GEMM_TAILSPLIT": 0}, 1200, 1024, 128, STORE, 8, {}, tile(7, grid=20, saddr=1)),
    ({"ACEHIP_GEMM_TAILSPLIT": 0}, 6000, 12288, 2048, SWIGLU, None, {}, walk(6000, 1152, 0, 256)),
    ({"ACEHIP_GEMM_HPTAIL": 0}, 6000, 4096, 2048, HEADPOST, None, {}, tile(8, grid=512, saddr=0)),
    ({"ACEHIP_GEMM_HELPERS": 0}, 3000, 2048, 2048, GATED, None, {}, tile(13, helpers=0)),
    ({"ACEHIP_GEMM_SADDR": 0}, 1200, 1024, 128, STORE, 8, {}, tail1(1024, 16, 8, saddr=0)),
    ({"ACEHIP_GEMM_SADDR": 0}, 6000, 2048, 2048, GATED, None, {}, tile(8, saddr=0)),
    ({"ACEHIP_SMALLM_WHOLEK": 1}, 125, 12288, 2048, SWIGLU, None, {}, tile(16, helpers=0)),
    ({"ACEHIP_SMALLM_WHOLEK": 0}, 125, 12288, 2048, SWIGLU, None, {}, splitk(2, 16, stages=3, grid=192)),
    ({"ACEHIP_SPLITK_BN": 128}, 125, 2048, 512, RES, None, {}, splitk(2, 4, bn=128, stages=3, grid=16)),
    ({"ACEHIP_SPLITK_BN": 128}, 125, 8192, 512, RES, None, {}, splitk(2, 4, bn=128, stages=2, grid=64)),
    ({}, 125, 2048, 512, RES, None, {"defer_ok": True}, splitk(2, 4, deferred=1, grid=32)),
    ({"ACEHIP_SPLITK_FUSE": 0}, 125, 2048, 512, RES, None, {"defer_ok": True}, splitk(2, 4, deferred=0)),
    # no workspace: no split-K, and no staging buffer for the small head-post grid
    ({}, 125, 2048, 2048, GATED, None, {"ws_bytes": 0}, tile(0, grid=16)),
    ({}, 500, 4096, 2048, HEADPOST, None, {"ws_bytes": 0}, tile(8, grid=48, saddr=0)),
    # a pitch whose 32-bit lane offsets would wrap keeps the pointer form, and the walk with it
    ({}, 6000, 2048, 2048, GATED, None, {"lda": 1 << 25}, tile(8, saddr=0)),
    ({}, 768, 512, 128, SWIGLU, 2, {"lda": 1 << 25}, tile(7, saddr=0)),
]


@pytest.mark.parametrize("knobs,M,N,K,epi,cap,kw,want", OFF_ARM_ROWS)
def test_other_arms(monkeypatch, knobs, M, N, K, epi, cap, kw, want):
    _assert_plan(_plan(monkeypatch, M, N, K, epi, cap, knobs, **kw), want, (knobs, M, N, K, epi, cap, kw))


def test_unused_fields_are_zero(monkeypatch):
    got = _plan(monkeypatch, 300, 512, 128, RES, None)
    assert got == dict(route=ROUTE_TILE, v_head=0, v_tail=0, M1=0, nmain=0, ntail=0, grid=12, splits=0, kper=0, bn=0,
                       stages=0, deferred=0, saddr=0, helpers=0)


def test_shapes_the_dispatch_refuses():
    for M, N, K, epi in [(0, 512, 128, STORE), (8, 200, 128, STORE), (8, 512, 96, STORE), (8, 384, 128, HEADPOST),
                         (8, 512, 128, 5)]:
        with pytest.raises(RuntimeError, match="diag_gemm_plan"):
            _ffi.gemm_plan(M, N, K, epi, device_cus=256)
