// gemm_plan.h — which launch gemm() gives a shape, as plain integer functions of the shape, the
// CU counts and the A/B switches: no HIP, no knobs(), no device query, so the route is a value
// that host code reads, tabulates and tests (acehip_diag_gemm_plan) before anything launches.
// gemm.hip launches from the plan (gemm_launch); nothing else holds a routing rule.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>

#include "../../include/acehip.h"
#include "pp_addr.h"

namespace acehip {

enum GemmEpi {
    EPI_STORE = 0,       // C = bf16(acc + bias)
    EPI_GATED_RES = 1,   // C = bf16(res + bf16(bf16(acc) * gate[b][n]))   (AdaLN-Zero gated residual)
    EPI_RES = 2,         // C = bf16(res + bf16(acc))                       (plain residual)
    EPI_SWIGLU = 3,      // packed [gate|up] blocks of 32 rows → C[M, N/2] = bf16(silu(g)·u)
    EPI_HEADPOST = 4,    // bf16(acc) staged in LDS, then per-128-column head: q/k RMSNorm (+RoPE) and
                         // scatter to head-major [B][heads][S][128] (GemmArgs::hp); C unused
};
constexpr int EPI_PARTIAL = 5;   // internal: fp32 partials of split blockIdx.y → ws
constexpr int EPI_CONV = 6;      // the VAE's implicit-GEMM convs (gemm_conv)
constexpr int GEMM_BK = 64;      // K-tile of every GEMM kernel

struct PlanIn {
    int M, N, K, epi;
    int64_t lda, ldw;
    size_t ws_bytes;   // split-K workspace (0: none)
    bool defer_ok;     // the caller takes a deferred residual epilogue: in place, ldr = ldc = N
};
// The CU count each decision reads (kept as measured; the two differ only under ACEHIP_GEMM_CUS):
//   dev_cus   split-K (admission and split count), the half-chip four-wave test (half_chip_w4:
//             the head-post arm and gemm_pick_variant's variant 13), the head-post "small grid"
//             test and its tail-split cost comparison, the conv tile height (conv_tile_rows)
//   plan_cus  gemm_pick_variant's 0 / 9 / 7 / 8 model, the tail split (rounds, M1, whether the
//             tail fits one round), the persistent walk (multi-round test, grid), and
//             cross_fuse_plan throughout
struct PlanEnv {
    int dev_cus, plan_cus;   // the device's; min(that, ACEHIP_GEMM_CUS) (plan_env in gemm.hip)
    int gemm_tailsplit, gemm_helpers, splitk_fuse, splitk_bn, smallm_wholek, gemm_hp_tail, gemm_persist, gemm_saddr;
};
using GemmPlan = acehip_gemm_plan;   // include/acehip.h: the route and the numbers its launch needs

inline int64_t tile_count(int64_t M, int N, int BM, int BN) { return ((M + BM - 1) / BM) * (N / BN); }
inline int variant_bm(int v) { return v == 7 ? 256 : v == 8 || v == 13 ? 192 : 128; }
inline int variant_bn(int v) { return v == 7 || v == 8 || v == 9 ? 256 : v == 16 || v == 17 ? 64 : 128; }

// Whether a one-tile ping-pong launch of BM-row tiles takes the scalar-base K loop
// (gemm_pp_body SADDR): ACEHIP_GEMM_SADDR, and leading dimensions whose 32-bit lane offsets
// cannot wrap — anything else keeps the pointer form, so no call that works there fails here.
// The store / residual / SwiGLU epilogues and the fused main + tail launch (head-post included)
// take it; the conv epilogue and the one-launch head-post grid (layer 0's deduplicated QKV) stay
// on the pointer form — in the round-8 A/B they were ahead with it, but not by twice the
// same-vs-same spread in every round, so this switch alone leaves them there (the
// head-post grid takes the scalar base together with the slot-immediate loop: pp_tile_slotimm).
inline bool pp_tile_saddr(int gemm_saddr, int epi, int BM, int64_t lda, int64_t ldw) {
    return gemm_saddr && epi != EPI_HEADPOST && epi != EPI_CONV && pp_saddr_fits(BM, lda, ldw);
}

// Whether a ping-pong launch of BM-row tiles runs the slot-immediate K loop (pp_main SLOTIMM, a
// scalar-base loop): ACEHIP_GEMM_SLOTIMM, on every launch that takes the scalar-base form — the
// one-tile kernels of pp_tile_saddr, the fused main + tail launch (BM = 256, where the plan says
// saddr) and the persistent walk (scalar-base under either ACEHIP_GEMM_SADDR: gemm_saddr = 1) —
// and on the one-launch head-post grid (layer 0's deduplicated QKV), which takes the scalar base
// only together with the slot immediates: that pair passed the round-11 A/B against the pointer
// form, the scalar base alone had not in round 8.  The conv epilogue did not pass it
// either way and has no such instantiation: the knob does nothing there.  With the knob 0 every
// launch is the one pp_tile_saddr picks.
inline bool pp_tile_slotimm(int gemm_slotimm, int gemm_saddr, int epi, int BM, int64_t lda, int64_t ldw) {
    return gemm_slotimm && gemm_saddr && epi != EPI_CONV && pp_saddr_fits(BM, lda, ldw);
}

// Half-chip grids (M ≈ 3000: the conditional rows' cross-Q / cross-O): the four-wave
// 192×128 tile with a 3-deep ring fills the chip in one round (16 × 16 tiles at
// N = 2048) where the 128² tile runs 0.75 of a 2-blocks-per-CU round: 34–35 → 31 µs,
// hot or cold weights (tools/bench_gemm.py, r02).
inline bool half_chip_w4(int64_t M, int N, int cus) {
    if (N % 128) return false;
    const int64_t t = tile_count(M, N, 192, 128);
    return t <= cus && t * 4 >= (int64_t)cus * 3;
}

// Tile choice from a one-block-per-CU cost model fitted on MI355X
// (tools/bench_gemm.py): time ∝ ⌈tiles / CUs⌉ × per-tile time, with a 256×256
// ping-pong tile costing 1.093× a 192×256 one (it does 1.33× the work).  The
// model reproduces the measured v7/v8 ratios on all four DiT shapes to 2 %.
// Grids that fill at most half the chip fall back to 128×128 (2 blocks/CU): at
// M = 3000, N = 2048 (the cross-O GEMM of the conditional rows) 37 µs vs 46 µs.
constexpr double kCost256 = 1.093;
inline int64_t rounds_up(int64_t tiles, int cus) { return (tiles + cus - 1) / cus; }
inline int gemm_pick_variant(int64_t M, int N, const PlanEnv &e) {
    if (half_chip_w4(M, N, e.dev_cus) && (N % 256 || tile_count(M, N, 192, 256) <= e.dev_cus / 2)) return 13;
    if (N % 256) return 0;
    const int cus = e.plan_cus;
    const int64_t t7 = tile_count(M, N, 256, 256), t8 = tile_count(M, N, 192, 256);
    if (t8 <= cus / 2) return 0;
    // one partial round of 192-row tiles (M ≈ 500: the 20 s song's CFG batch, the lyric
    // encoder's SwiGLU): 128-row tiles still fit one round and finish sooner
    if (t8 <= cus && tile_count(M, N, 128, 256) <= cus) return 9;
    return (double)rounds_up(t7, cus) * kCost256 < (double)rounds_up(t8, cus) ? 7 : 8;
}

// Split-K is for grids that cannot fill half the chip even with 128×128 tiles and have K to
// split (short songs / turbo: M = Bc·S of a few hundred rows)
inline bool splitk_small(int64_t M, int N, int K, int cus) {
    return tile_count(M, N, 128, 128) * 2 <= cus && K / GEMM_BK >= 8;
}

// gemm_plan's tile route: variant v in one grid
inline GemmPlan plan_tile(const PlanIn &in, const PlanEnv &e, int v) {
    GemmPlan p{};
    p.route = ACEHIP_ROUTE_TILE; p.v_head = v; p.grid = (int)tile_count(in.M, in.N, variant_bm(v), variant_bn(v));
    p.saddr = v >= 7 && v <= 9 && pp_tile_saddr(e.gemm_saddr, in.epi, variant_bm(v), in.lda, in.ldw);
    // variant 13: + 2 LDS-DMA helper waves (M ≈ 3000 shapes: 1 round; ACEHIP_GEMM_HELPERS=0: without, A/B)
    p.helpers = v == 17 || (v == 13 && e.gemm_helpers);
    return p;
}

// SwiGLU grids of 256² tiles (with their tail) as one persistent walk (ACEHIP_GEMM_PERSIST=0:
// one tile per workgroup); the walk's K loop is the scalar-base one
inline bool walk_ok(const PlanIn &in, const PlanEnv &e) {
    return in.epi == EPI_SWIGLU && e.gemm_persist && pp_saddr_fits(256, in.lda, in.ldw);
}

// Tail split for ping-pong grids whose last round is a small fraction of the chip
// (SwiGLU gate/up at 240 s: 24 × 48 = 1152 tiles of 256² on 256 CUs = 4.5 rounds, the
// last half-round costing a whole tile time): rows [0, M1) keep the big tile with
// M1 chosen so their grid is whole rounds (less at most one row of tiles), and the
// remaining rows run as one round of 128×256 two-phase ping-pong tiles where they fit one
// round (variant 9), else of 128×128 tiles (2 blocks/CU, variant 0).  Row-local epilogues
// only: store, SwiGLU and head-post (whose tail needs the 128×256 tile: the 128×128 one has
// no head-post epilogue); the gated residual indexes its batch by row.
// ACEHIP_GEMM_TAILSPLIT=0 disables it.  False (p untouched) when not applicable; v = 7 or 8.
inline bool plan_tail_split(GemmPlan &p, const PlanIn &in, const PlanEnv &e, int v) {
    if (in.epi != EPI_SWIGLU && in.epi != EPI_STORE && in.epi != EPI_HEADPOST) return false;
    if (!e.gemm_tailsplit) return false;
    const int BMv = variant_bm(v), cus = e.plan_cus;
    const int64_t nN = in.N / 256, tiles = tile_count(in.M, in.N, BMv, 256);
    const int64_t full = tiles / cus, rem = tiles - full * cus;
    if (full < 1 || rem == 0 || rem * 5 > (int64_t)cus * 3) return false;   // last round > 60 % full
    const int64_t rows = full * cus / nN, M1 = rows * BMv;   // whole rows of tiles in the full rounds
    if (M1 <= 0 || M1 >= in.M) return false;
    if (tile_count(in.M - M1, in.N, 128, 128) > 2 * (int64_t)cus) return false;
    // the tail as one round of 128×256 two-phase ping-pong tiles
    const int64_t t9 = tile_count(in.M - M1, in.N, 128, 256);
    const bool pp128 = t9 <= cus;
    if (in.epi == EPI_HEADPOST && !pp128) return false;   // the 128×128 tail tile has no head-post epilogue
    p = GemmPlan{};
    p.route = ACEHIP_ROUTE_TAIL2; p.v_head = v; p.v_tail = pp128 ? 9 : 0; p.M1 = (int)M1;
    p.grid = p.nmain = (int)(rows * nN); p.ntail = (int)(pp128 ? t9 : tile_count(in.M - M1, in.N, 128, 128));
    p.saddr = pp_tile_saddr(e.gemm_saddr, in.epi, BMv, in.lda, in.ldw);
    if (pp128 && v == 7) {
        // both grids in one launch.  SwiGLU: one persistent walk over both, on one workgroup per
        // planned CU (at most one tail tile each: t9 ≤ cus ≤ grid).  Else, where the main grid's
        // block count is a multiple of 8 — so the tail blocks' XCD is their own index mod 8, as
        // in a launch of their own — blocks [0, nmain) main, the rest tail; head and tail share
        // lda / ldw and 256 rows bound both tiles' offsets
        if (walk_ok(in, e)) {
            p.route = ACEHIP_ROUTE_WALK; p.grid = std::min(cus, p.nmain + p.ntail); p.saddr = 1;
        } else if (p.nmain % 8 == 0) {
            p.route = ACEHIP_ROUTE_TAIL1; p.grid = p.nmain + p.ntail; p.saddr = e.gemm_saddr && pp_saddr_fits(256, in.lda, in.ldw);
        }
    }
    return true;
}

// The route of gemm(): in.M > 0, N % 128 == 0 (head-post: % 256), K % 64 == 0, K > 0
inline GemmPlan gemm_plan(const PlanIn &in, const PlanEnv &e) {
    const int M = in.M, N = in.N, nk = in.K / GEMM_BK;
    GemmPlan p{};
    // SwiGLU of one 128-row chunk (turbo / short songs, M ≤ 128): whole-K 128×64 tiles with the
    // SwiGLU epilogue fused (variant 16: no fp32 partials, no second launch) — M = 125, cold
    // weights: 26.1 → 19.0 µs (tools/bench_small_m.py).  ACEHIP_SMALLM_WHOLEK=0: split-K (A/B);
    // 2: variant 17, 16 + two LDS-DMA helper waves
    if (in.epi == EPI_SWIGLU && M <= 128 && N % 64 == 0 && e.smallm_wholek) return plan_tile(in, e, e.smallm_wholek == 2 ? 17 : 16);
    // Split-K: the K range is split so the grid reaches ~1 block per CU (at least 4 K-tiles per
    // split), every split stores fp32 partials, and the epilogue is either folded into the
    // consumer (head_post for the head-post case; the next rmsnorm_mod for residual epilogues,
    // gemm(…, defer)) or run by splitk_epilogue_kernel.
    if (in.ws_bytes && splitk_small(M, N, in.K, e.dev_cus)) {
        // tile width: 64-column tiles double the grid at a given split count (half the splits
        // and partial bytes for ~1 block per CU).  Round 3 kept 128 where N and K < 4096 (O at M = 125
        // measured 18.7 → 25.3 µs on 64); round 4 measured every shape faster on 64 (O 16.0 → 14.7, QKV
        // 15.4 → 14.8, `profiles/r04h2_small_m.log`) and the songs too (turbo 10 s DiT 25.6 → 24.6 ms,
        // base 10 s 96.9 → 93.9, `profiles/r04h3_ab_turbo.log`): 64 everywhere.  ACEHIP_SPLITK_BN =
        // 128 | 64 forces one (A/B)
        const int bn = e.splitk_bn && e.splitk_bn != 64 ? 128 : 64;
        const int64_t tb = tile_count(M, N, 128, bn);   // grid tiles of the split kernel
        const int splits = (int)std::min<int64_t>(std::min<int64_t>(16, nk / 4), (e.dev_cus + tb - 1) / tb);
        const size_t need = (size_t)splits * M * N * 4 + (size_t)M * N * 2;   // partials + head-post staging
        if (splits >= 2 && need <= in.ws_bytes) {
            p.route = ACEHIP_ROUTE_SPLITK; p.bn = bn; p.grid = (int)tb;
            p.kper = (nk + splits - 1) / splits; p.splits = (nk + p.kper - 1) / p.kper;
            // Ring depth (tools/ab_splitk.py, M = 125): 3 stages for N ≤ 4096 (down / QKV / O:
            // 20.1 → 19.0, 18.3 → 17.4, 15.1 → 14.9 µs), 2 for the wide SwiGLU (26.2 vs 28.3 µs).
            // (helper waves measured no gain here: 2 MFMA waves / SIMD already cover the DMA issue)
            p.stages = bn == 64 || N <= 4096 ? 3 : 2;
            p.deferred = in.defer_ok && e.splitk_fuse && (in.epi == EPI_GATED_RES || in.epi == EPI_RES);
            return p;
        }
    }
    if (in.epi == EPI_HEADPOST) {
        // a 192×256 grid that fills at most half the chip (cross-Q of the conditional rows,
        // M = 3000) runs as 192×128 tiles — one head each — with the same fused epilogue; a
        // small grid outside the four-wave tile's geometry goes through the staging buffer +
        // the standalone head_post kernel on 128×128 tiles
        const int cus = e.dev_cus;
        const int64_t t7 = tile_count(M, N, 256, 256), t8 = tile_count(M, N, 192, 256);
        const bool small = t8 * 2 <= cus;
        if (small && half_chip_w4(M, N, cus)) return plan_tile(in, e, 13);
        if (small && in.ws_bytes && (size_t)M * N * 2 <= in.ws_bytes) {
            p = plan_tile(in, e, 0);
            p.route = ACEHIP_ROUTE_STAGED;
            return p;
        }
        // whole rounds of 256-row tiles + one round of 128-row tiles where that costs less than
        // the 192-row rounds (cost model of gemm_pick_variant, a 128×256 tile ≈ 0.6 of a 192×256
        // one): QKV at 240 s, 32 × 16 = 2 rounds of 192 → 1 round of 256 + 1 of 128
        if (e.gemm_hp_tail && t7 >= cus && (double)(t7 / cus) * kCost256 + 0.6 < (double)rounds_up(t8, cus) &&
            plan_tail_split(p, in, e, 7))
            return p;
        return plan_tile(in, e, 8);
    }
    const int v = gemm_pick_variant(M, N, e);
    if ((v == 7 || v == 8) && plan_tail_split(p, in, e, v)) return p;
    // a multi-round SwiGLU grid of 256² tiles without a tail split: the same persistent walk
    const int64_t t7 = tile_count(M, N, 256, 256);
    if (v == 7 && walk_ok(in, e) && t7 > e.plan_cus && t7 < (1ll << 30)) {
        p.route = ACEHIP_ROUTE_WALK; p.v_head = 7; p.M1 = M; p.nmain = (int)t7; p.grid = e.plan_cus; p.saddr = 1;
        return p;
    }
    return plan_tile(in, e, v);
}

// cross_fuse_planned (gemm.hip): the cross-Q head-post GEMM on the half-chip four-wave tile with
// its helper waves.  Not gemm_plan's route to variant 13: the CU count is the planned one
// throughout (tests fill a 4-CU "chip" with a 2 × 2 grid), and the split-K term is the coarser
// one — a workspace and splitk_small, without the split count or the workspace size.
inline bool cross_fuse_plan(int64_t M, int N, int K, bool have_ws, const PlanEnv &e) {
    if (!e.gemm_helpers || N % 256) return false;
    if (have_ws && splitk_small(M, N, K, e.plan_cus)) return false;   // split-K
    return half_chip_w4(M, N, e.plan_cus);
}

// gemm_conv's tile height.  Short activations (a 10 s decode's C = 1024 / 512 blocks: 40 / 118
// tiles of 256 rows on 256 CUs): 128-row tiles double the grid, 64-row tiles (80 KB of LDS, 118
// VGPRs: two blocks per CU) quadruple it.  10 s decode 2.13 → 1.96 (128) → 1.91 ms (64 below a
// quarter of the chip), bit-identical (profiles/r05az_ab_vae_small_tiles.log)
inline int conv_tile_rows(int64_t M, int N, int dev_cus) {
    const int64_t t256 = tile_count(M, N, 256, 256);
    return t256 * 4 <= dev_cus ? 64 : t256 * 2 <= dev_cus ? 128 : 256;
}

}  // namespace acehip
