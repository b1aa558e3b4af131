"""The two source-address forms of the ping-pong GEMM tiles, compared on the CPU (no GPU call).

A ping-pong tile (gemm.hip, variants 7 / 8 / 9 and the implicit-GEMM convs) fetches its operands
by LDS-DMA either from a 64-bit pointer per piece and lane (PPSrcPtr) or from the tile's scalar
base plus a 32-bit lane offset (PPSrcOff, ACEHIP_GEMM_SADDR).  Both sets take their integer
arithmetic from csrc/pp_addr.h, and acehip_diag_pp_src_check walks a whole grid with it: every row
and column tile, wave, lane, piece and K-tile, the scalar form's lane offset in 32-bit wrap-around
arithmetic as the hardware adds it.  So a wrong or wrapping offset shows here as a mismatch count,
before any kernel runs.

Bounds: without a conv shift the pieces stay inside their operand — A offsets in
[0, M·lda·2), W offsets in [0, N·ldw·2).  A conv reads input rows m + a0 + tap·dil: down to a0 rows
before the activation and (taps − 1)·dil + a0 rows past it, the zero halo rows the caller provides
(conv.hip: 3·dil rows each side for k = 7, one row each side for a ConvTranspose).  The conv
epilogue currently launches the pointer form only (gemm_plan.h pp_tile_saddr); its shapes are checked
all the same, so the scalar form is known to be address-equal for them before anyone switches it on.
"""
import ctypes

import pytest

# the shapes tests/test_gpu_gemm_saddr.py runs (pitch = K + 64), on each tile height they reach
TILE_CASES = [(M, N, K, K + 64, K + 64, BM) for M in (1, 200, 449) for N in (256, 512) for K in (64, 128, 192)
              for BM in (256, 192, 128)]
# the tail-split cases: a 1024-row main grid of 256-row tiles + a 176-row tail of 128-row tiles
SPLIT_CASES = [(1024, 1024, 256, 256, 256, 256), (176, 1024, 256, 256, 256, 128),
               (1200, 1024, 256, 256, 256, 192)]
# the 240 s song's DiT GEMMs (S = 3000 patches, two CFG rows: M = 6000; layer 0 runs its QKV once
# for both rows: M = 3000): QKV head-post, O, down, SwiGLU gate/up
DIT_CASES = [(6000, 4096, 2048, 2048, 2048, 192), (6000, 4096, 2048, 2048, 2048, 256), (952, 4096, 2048, 2048, 2048, 128),
             (3000, 4096, 2048, 2048, 2048, 192), (6000, 2048, 2048, 2048, 2048, 192),
             (6000, 2048, 6144, 6144, 6144, 192), (6000, 12288, 2048, 2048, 2048, 256),
             (6000, 12288, 2048, 2048, 2048, 128)]

# (M, N, K, cin, dil, a0, BM): the convs of a 240 s decode (6000 latent frames; activations of
# 60 000 × 1024, 360 000 × 512, 1 440 000 × 256 and 5 760 000 × 128) that run as implicit GEMMs —
# k = 7 (dilations 1, 3, 9) and k = 1 at C ≥ 256, the five ConvTranspose blocks (M = L_in + 1,
# N = stride · Cout) — and the small-tile unit-test shapes of tests/test_gpu_gemm_saddr.py
VAE_CONVS = []
for L, C in ((60000, 1024), (360000, 512), (1440000, 256)):
    VAE_CONVS += [(L, C, 7 * C, C, d, -3 * d, 256) for d in (1, 3, 9)]
    VAE_CONVS.append((L, C, C, C, 1, 0, 256))
for L, Cin, Cout, s in ((6000, 2048, 1024, 10), (60000, 1024, 512, 6), (360000, 512, 256, 4),
                        (1440000, 256, 128, 4), (5760000, 128, 128, 2)):
    VAE_CONVS.append((L + 1, s * Cout, 2 * Cin, Cin, 1, -1, 256))
VAE_CONVS += [(333, 256, 7 * 256, 256, 9, -27, 128), (333, 256, 7 * 256, 256, 9, -27, 64),
              (301, 1024, 2 * 512, 512, 1, -1, 128), (301, 1024, 2 * 512, 512, 1, -1, 64),
              (333, 256, 256, 256, 1, 0, 128), (333, 256, 256, 256, 1, 0, 64)]


def _check(M, N, K, lda, ldw, BM, cin=0, dil=1, a0=0):
    from acehip import _ffi
    fits, lo, hi_a, hi_b = ctypes.c_int(-1), ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64()
    bad = _ffi.lib().acehip_diag_pp_src_check(M, N, K, lda, ldw, BM, cin, dil, a0, ctypes.byref(fits),
                                              ctypes.byref(lo), ctypes.byref(hi_a), ctypes.byref(hi_b))
    return bad, fits.value, lo.value, hi_a.value, hi_b.value


@pytest.mark.parametrize("M,N,K,lda,ldw,BM", TILE_CASES + SPLIT_CASES + DIT_CASES)
def test_gemm_addresses_equal_and_inside(M, N, K, lda, ldw, BM):
    bad, fits, lo, hi_a, hi_b = _check(M, N, K, lda, ldw, BM)
    assert bad == 0 and fits == 1
    assert 0 <= lo and hi_a < M * lda * 2
    # the last piece ends exactly at the end of the operand's last row of K
    assert hi_a == (M - 1) * lda * 2 + K * 2 - 1
    assert hi_b == (N - 1) * ldw * 2 + K * 2 - 1 < N * ldw * 2


@pytest.mark.parametrize("M,N,K,cin,dil,a0,BM", VAE_CONVS)
def test_conv_addresses_equal_and_inside_halo(M, N, K, cin, dil, a0, BM):
    taps = K // cin
    bad, fits, lo, hi_a, hi_b = _check(M, N, K, cin, K, BM, cin, dil, a0)
    assert bad == 0 and fits == 1
    # first tap of row 0 … last tap of row M − 1: inside the halo rows, never beyond
    assert lo == a0 * cin * 2
    assert hi_a == (M - 1 + a0 + (taps - 1) * dil) * cin * 2 + cin * 2 - 1
    assert -a0 <= 32 and a0 + (taps - 1) * dil <= 3 * dil   # conv.h kActPadRows / the rows conv.hip clears
    assert hi_b == N * K * 2 - 1


def test_guard_is_tight():
    """pp_saddr_fits at its boundary: the largest leading dimension whose row-255 offset still fits
    32 bits compares equal; the next multiple of 8 wraps (mismatches) and the guard refuses it, while
    a 64-row tile, whose last row is 63, still takes it."""
    lda_ok = (2 ** 32 - 113) // 510 // 8 * 8
    bad, fits, *_ = _check(300, 256, 64, lda_ok, 128, 256)
    assert (bad, fits) == (0, 1)
    bad, fits, *_ = _check(300, 256, 64, lda_ok + 8, 128, 256)
    assert bad > 0 and fits == 0
    bad, fits, *_ = _check(300, 256, 64, lda_ok + 8, 128, 64)
    assert (bad, fits) == (0, 1)
    # W: row 63 and the 64-row step between pieces
    ldw_ok = (2 ** 32 - 1) // 128 // 8 * 8
    bad, fits, *_ = _check(8, 256, 64, 64, ldw_ok, 128)
    assert (bad, fits) == (0, 1)
    bad, fits, *_ = _check(8, 256, 64, 64, ldw_ok + 8, 128)
    assert bad > 0 and fits == 0


def test_bad_arguments_are_refused():
    assert _check(8, 200, 64, 64, 64, 128)[0] == -1
    assert _check(8, 256, 64, 64, 64, 100)[0] == -1
    assert _check(8, 256, 96, 96, 96, 128)[0] == -1
