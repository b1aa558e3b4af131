"""The slot-immediate K loop of the ping-pong GEMM tiles (ACEHIP_GEMM_SLOTIMM), checked on the CPU
(no GPU call).

The loop (gemm.hip pp_main SLOTIMM) issues every LDS read as one of eight per-lane base registers —
operand A / W × k-step × ring slot, formed once before the loop — plus an instruction immediate of
2048 bytes per 16-row sub-tile.  The integer arithmetic is csrc/pp_addr.h's (pp_rd_base,
pp_rd_imm), and acehip_diag_pp_lds_check walks it for BM ∈ {64, 128, 192, 256} × wave × lane ×
slot × k-step × operand × sub-tile in 32-bit arithmetic against the slot's swizzled address
lds + slot·BUF + swz(row, chunk), so a wrong base, an immediate past the 16-bit field or a read
outside the tile's LDS array shows as a count here before any kernel runs.

The routing predicate (gemm_plan.h pp_tile_slotimm): the scalar-base launches and the one-launch
head-post grid take the loop, the conv epilogue and leading dimensions that do not fit the 32-bit
lane offsets keep the pointer form; the plan itself — route, tiles, grid, saddr — does not depend on the
knob, so knob 0 launches exactly what the plan launched before.
"""
import ctypes

import pytest

from conftest import set_knob

STORE, GATED, RES, SWIGLU, HEADPOST, CONV = 0, 1, 2, 3, 4, 6


def _lds_check(lds):
    from acehip import _ffi
    reads, imm, end = ctypes.c_int64(), ctypes.c_int(), ctypes.c_int64()
    bad = _ffi.lib().acehip_diag_pp_lds_check(lds, ctypes.byref(reads), ctypes.byref(imm), ctypes.byref(end))
    return bad, reads.value, imm.value, end.value


# the kernel's LDS array sits at 0 (its only __shared__ object); the arithmetic is checked at other
# bases too, the last one with the ring ending exactly at the top of the 32-bit address space
@pytest.mark.parametrize("lds", [0, 16, 4096, 2 ** 32 - 2 * (256 + 256) * 128])
def test_reads_equal_swizzled_addresses_and_stay_inside(lds):
    bad, reads, imm, end = _lds_check(lds)
    assert bad == 0
    # per BM: 8 waves × 64 lanes × 2 slots × 2 k-steps × (BM / 32 A + 4 W sub-tiles)
    assert reads == sum(8 * 64 * 2 * 2 * (BM // 32 + 4) for BM in (64, 128, 192, 256))
    # the largest immediate: A sub-tile 7 of a 256-row tile — inside the 16-bit offset field
    assert imm == 7 * 2048 < 65536
    # the highest read ends exactly at the end of the 256-row tile's ring (slot 1, last W row's chunks)
    assert end == 2 * (256 + 256) * 128


def test_slot_one_needs_its_own_base():
    """Why eight bases and not four: slot 1 is one tile buffer on — 57 344 bytes at 192 rows, 65 536
    at 256 — and that plus a sub-tile immediate does not fit the 16-bit field."""
    for BM in (192, 256):
        assert (BM + 256) * 128 + (BM // 32 - 1) * 2048 >= 65536


@pytest.mark.parametrize("knob", [0, 1])
def test_predicate(monkeypatch, knob):
    from acehip import _ffi
    set_knob(monkeypatch, "ACEHIP_GEMM_SLOTIMM", str(knob))
    f = _ffi.lib().acehip_diag_pp_slotimm
    for BM in (128, 192, 256):
        for epi in (STORE, GATED, RES, SWIGLU, HEADPOST):
            assert f(epi, BM, 2048, 2048) == knob       # scalar-base launches, the one-launch head-post grid
            assert f(epi, BM, 1 << 25, 2048) == 0       # 32-bit lane offsets would wrap: pointer form
    for BM in (64, 128, 256):
        assert f(CONV, BM, 1024, 7168) == 0             # the conv epilogue: no slot-immediate instantiation
    # the boundary of pp_saddr_fits (tests/test_gemm_saddr_host.py test_guard_is_tight)
    lda_ok = (2 ** 32 - 113) // 510 // 8 * 8
    assert f(GATED, 256, lda_ok, 128) == knob and f(GATED, 256, lda_ok + 8, 128) == 0
    # a scalar-base loop: never without ACEHIP_GEMM_SADDR
    set_knob(monkeypatch, "ACEHIP_GEMM_SADDR", "0")
    assert f(GATED, 192, 2048, 2048) == 0 and f(HEADPOST, 192, 2048, 2048) == 0


# (M, N, K, epi, ACEHIP_GEMM_CUS, lda): the 240 s song's ping-pong GEMMs, the unit-test shapes of
# tests/test_gpu_gemm_slotimm.py and a leading dimension that does not fit the scalar-base form
PLAN_ROWS = [(6000, 2048, 2048, GATED, None, None), (6000, 2048, 6144, GATED, None, None),
             (6000, 4096, 2048, HEADPOST, None, None), (3000, 4096, 2048, HEADPOST, None, None),
             (6000, 12288, 2048, SWIGLU, None, None), (1200, 1024, 320, STORE, 8, 384),
             (768, 512, 128, SWIGLU, 2, None), (6000, 2048, 2048, GATED, None, 1 << 25)]


@pytest.mark.parametrize("M,N,K,epi,cus,lda", PLAN_ROWS)
def test_plan_does_not_depend_on_the_knob(monkeypatch, M, N, K, epi, cus, lda):
    from acehip import _ffi
    if cus:
        set_knob(monkeypatch, "ACEHIP_GEMM_CUS", str(cus))
    plans = []
    for knob in (0, 1):
        set_knob(monkeypatch, "ACEHIP_GEMM_SLOTIMM", str(knob))
        plans.append(_ffi.gemm_plan(M, N, K, epi, lda=lda, ldw=None, device_cus=256))
    assert plans[0] == plans[1]
