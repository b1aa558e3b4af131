// attn_plan.h — which launch attention() gives a shape, as plain integer functions of the shape,
// the planned CU count and the A/B switches: no HIP, no knobs(), no device query, so the route is
// a value that host code reads, tabulates and tests (acehip_diag_attn_plan) before anything
// launches.  attention.hip launches from the plan (attn_launch) and attention_whole_units reads
// it; nothing else holds a routing rule.  attn_decode_plan is the key-range split of
// attention_decode (attn_decode.hip).
#pragma once
#include <algorithm>
#include <cstdint>

#include "../../include/acehip.h"

namespace acehip {

constexpr int ATTN_QB = 128;      // queries per workgroup of attn_fwd_kernel / attn_pw_kernel
constexpr int ATTN_KT = 64;       // keys per K/V tile
// window: < 0 full, >= 0 band |i−j| <= window, ATTN_CAUSAL keys j <= i (Qwen3 text encoder)
constexpr int ATTN_CAUSAL = -2;

struct AttnPlanIn {
    int B, H, KV, Sq, Sk, window;
    bool masked;    // a key-padding mask is given
    bool have_ws;   // the caller passes the split workspace (attention_ws_bytes())
};
// cus: the CU count every rule below plans for — the device's, or ACEHIP_ATTN_CUS, which replaces
// it (tests use it to exercise 3- and 4-way splits, walks and stream-K on small shapes); the
// other six are the attention switches as Knobs holds them (attn_env in attention.hip)
struct AttnEnv {
    int cus;
    int attn_pw, attn_persist, attn_small, attn_small_mask, attn_small_causal, attn_streamk;
};
using AttnPlan = acehip_attn_plan;   // include/acehip.h: the kernel and the numbers its launch needs

// ticket / slab slots of the split workspace: [tickets: slots ints][slabs: slots · 8 waves ·
// 66·64 floats] (≤ cus split parts in flight; stream-K uses 2 slabs per workgroup)
inline int attn_ws_slots(int cus) { return std::max(1024, cus); }

// short-sequence KV split (a grid of a few units, e.g. the 10 s song's cross-attention: 8
// units): KV tiles per part.  Turbo 10 s cross
// (11 tiles, 8 units; tools/gpu_r03z.sh, one process): 1 tile per part 28.5 µs, 2: 22.7, 3: 20.3
// (DiT song 27.7 / 27.1 / 26.8 ms) — fewer, longer parts pay fewer hand-offs; 4 and 6 tiles
// (after the slab hand-off, tools/gpu_r03m2.sh): 19.6 / 21.9 vs 19.7 µs, song 25.7 / 26.1 vs 25.6
// ms; 3 kept
constexpr int SHORT_TPP = 3;
// shortest KV loop (tiles) whose tail units are split on attn_pw_kernel: 24 keeps the 240 s band
// layers (7 tiles) on the persistent walk (tried 7, the tail split: band 48.8 → 57.0 µs, DiT song
// 490.9 → 493.8 ms, profiles/r06za_band_tailsplit_ab.log)
constexpr int PW_SPLIT_MIN = 24;
// shortest KV loop (tiles) that attn_fwd_kernel splits — tail split and stream-K — and keeps
// on the GQA-pair workgroup (split_heads below):
// only long KV loops pay for the partial write + merge (measured: full attention
// at S = 3000, 47 tiles, −27 %; band (≈7 tiles) and cross (11 tiles) lose)
constexpr int FWD_SPLIT_MIN = 24;

// The two KV splits of attn_pw_kernel and attn_fwd_kernel<2> (units of one GQA pair, p.units and
// p.unit_tiles set, a workspace given; split_min: PW_SPLIT_MIN / FWD_SPLIT_MIN).  Units
// [0, full) run whole; each later unit runs as nsplit KV-range parts.
inline void plan_kv_split(AttnPlan &p, int cus, int split_min) {
    // one workgroup per CU: a partial last round of whole units is replaced by
    // tail units split over ⌊CUs / tail⌋ KV ranges (1.5 rounds instead of 2 at
    // 384 units on 256 CUs)
    const int tail = p.units % cus;
    if (p.unit_tiles >= split_min && p.units > cus && tail > 0 && tail <= cus / 2) {
        p.full = p.units - tail;
        p.nsplit = std::min(4, cus / tail);
    } else if (p.window < 0 && p.units * 2 <= cus && p.unit_tiles >= 4) {
        // short sequences (a few query blocks): every unit split over KV ranges so the
        // grid reaches the CUs (cross-attention of a 10 s song: 8 units → 40 parts)
        p.full = 0;
        p.nsplit = std::min(std::min(cus / p.units, (p.unit_tiles + SHORT_TPP - 1) / SHORT_TPP), 16);
    }
    p.uses_ws = p.nsplit > 1;
}

// The route of attention(): B, Sq, Sk, KV > 0, H % KV == 0.  kernel 0 (every field 0): refused —
// off attn_small_kernel, heads/kv_heads must be 1 or 2.
inline AttnPlan attn_plan(const AttnPlanIn &in, const AttnEnv &e) {
    const int B = in.B, H = in.H, KV = in.KV, Sq = in.Sq, Sk = in.Sk, cus = e.cus;
    const bool masked = in.masked;
    AttnPlan p{};
    // a band wider than the sequence (|i − j| ≤ max(Sq, Sk) − 1 ≤ window: every pair admitted)
    // is full attention — the 10 s songs' sliding layers (S = 125, window 128) then run the full
    // kernel without per-tile band classification and masks
    const int window = in.window >= 0 && !masked && std::max(Sq, Sk) - 1 <= in.window ? -1 : in.window;
    p.window = window;
    p.causal = window == ATTN_CAUSAL;
    const int grp = H / KV, nq = (Sq + ATTN_QB - 1) / ATTN_QB, ntall = (Sk + ATTN_KT - 1) / ATTN_KT;
    p.unit_tiles = window >= 0 && !masked ? (ATTN_QB + 2 * window) / ATTN_KT + 1 : ntall;

    // attn_small_kernel where its grid is at most 1.5 rounds of one-head × 32-row units (measured,
    // tools/bench_attn.py, one process, profiles/r05an_attn_small_vs_fwd.log: B = 2 full / cross at
    // S = 125 8.6 / 13.5 vs 15.6 / 26.7 µs, S = 375 (384 units) 21.6 / 29.1 vs 24.6 / 30.6; at
    // S = 750 (768 units) 45.1 / 43.0 vs 34.8 / 34.0 — attn_fwd_kernel's 128-row GQA-pair units
    // read K / V once per pair and tile, and win once the grid fills the chip).  Full attention,
    // with a key-padding mask under ACEHIP_ATTN_SMALL_MASK, unmasked causal under
    // ACEHIP_ATTN_SMALL_CAUSAL
    const int64_t small_units = (int64_t)((Sq + 31) / 32) * H * B;
    if (e.attn_small && window < 0 && small_units <= cus + cus / 2 && (!masked || e.attn_small_mask) &&
        (!p.causal || (!masked && e.attn_small_causal))) {
        p.kernel = ACEHIP_ATTN_SMALL;
        p.nrep = 1;
        p.units = (int)small_units;
        // KV parts per unit: about one tile per wave while the grid stays within one round
        // (ACEHIP_ATTN_SMALL=2: no parts)
        p.parts = 1;
        if (in.have_ws && e.attn_small == 1 && small_units <= attn_ws_slots(cus))
            p.parts = (int)std::max<int64_t>(1, std::min<int64_t>({(int64_t)(ntall + 3) / 4, cus / small_units, 16}));
        p.uses_ws = p.parts > 1;
        p.grid = p.units * p.parts;
        p.block = 256;
        return p;
    }

    // 64-row-per-wave kernel for the DiT's unmasked GQA-pair layers: ACEHIP_ATTN_PW = bit mask of
    // the layer kinds that use it (1 full, 2 band, 4 cross = window < 0 with Sk != Sq).  r02 A/B
    // (tools/bench_attn.py, one process, three boxes): band 46.4-48.4 vs 47.6-48.8 µs (kept),
    // full 166-189 vs 161-179 and B = 1 cross 30.5-31.8 vs 29.6-30.6 (stay on attn_fwd_kernel)
    const int kind_bit = window >= 0 ? 2 : (Sk == Sq ? 1 : 4);
    const int pair_units = nq * KV * B;
    if (grp == 2 && !masked && !p.causal && (e.attn_pw & kind_bit)) {
        p.kernel = ACEHIP_ATTN_PW;
        p.nrep = 2;
        p.units = p.full = pair_units;
        p.nsplit = 1;
        if (in.have_ws) plan_kv_split(p, cus, PW_SPLIT_MIN);
        p.grid = p.full + (p.units - p.full) * p.nsplit;
        // band layers with more units than CUs: one persistent workgroup per CU walking units
        // blockIdx.x + k·grid as one KV-tile stream (every unit then has ≥ 2 tiles: window ≥ KT,
        // Sq = Sk > 2·KT).  ACEHIP_ATTN_PERSIST=0 restores one workgroup per unit (A/B)
        if (e.attn_persist && p.nsplit == 1 && window >= ATTN_KT && Sq == Sk && Sq > 2 * ATTN_KT && p.units > cus) {
            p.persist = 1;
            p.grid = cus;
        }
        p.block = 256;
        return p;
    }

    // heads per workgroup: the GQA pair shares one 8-wave workgroup (K/V staged once per
    // tile for both heads), or each head gets its own 4-wave workgroup, two per CU, whose
    // SIMD partners run out of phase. Measured (r02, one box): band −3 %, cross −9 %,
    // full (47 tiles: the doubled K/V staging dominates) +7 %, cross with fewer pair units
    // than CUs (B = 1) +11 %, short split-KV cross slower.
    const bool short_split = window < 0 && pair_units * 2 <= cus && p.unit_tiles >= 4;   // plan_kv_split's
    const bool split_heads = grp == 2 && !p.causal && p.unit_tiles < FWD_SPLIT_MIN && !short_split && pair_units > cus;
    const int nrep = split_heads ? 1 : grp;
    if (nrep != 1 && nrep != 2) return AttnPlan{};
    p.kernel = ACEHIP_ATTN_FWD;
    p.nrep = nrep;
    p.units = p.full = pair_units * (grp / nrep);
    p.nsplit = 1;
    p.grid = p.units;
    p.block = nrep == 2 ? 512 : 256;
    // stream-K (ACEHIP_ATTN_STREAMK): unmasked full layers whose units do not divide into whole
    // rounds run as ONE round of `cus` workgroups over the units' concatenated KV tiles, instead
    // of a whole round + tail-split parts (a second round's fixed cost).  240 s full attention
    // (384 units × 47 tiles on 256 CUs) 186.1 → 175.8 µs in one process; the one-round cross grid
    // (192 units × 11 tiles) loses, 34.8 → 45.8 (its pieces' restart + merge ≥ the 2.75 tiles
    // saved), so only grids of more units than CUs and long loops take it
    // (two slab slots per workgroup: 2·cus ≤ the workspace's 1024 slots)
    if (e.attn_streamk && in.have_ws && nrep == 2 && window < 0 && !masked && p.units > cus && p.units % cus != 0 &&
        p.unit_tiles >= FWD_SPLIT_MIN && 2 * (int64_t)cus <= attn_ws_slots(cus)) {
        p.streamk = p.uses_ws = 1;
        p.sk_nt = p.unit_tiles;
        p.sk_total = p.units * p.unit_tiles;
        p.grid = cus;
    } else if (in.have_ws && nrep == 2 && !p.causal) {
        // causal (text encoder): whole units only — a KV-range part past the diagonal
        // would hold no valid key
        plan_kv_split(p, cus, FWD_SPLIT_MIN);
        p.grid = p.full + (p.units - p.full) * p.nsplit;
    }
    return p;
}

// attention_decode's key ranges (grid (parts, KV, B)): `parts` ranges of `per` whole 64-key steps,
// about two workgroups per CU (four per CU measured slower
// at 2304 keys, B·KV = 16: 26.1 vs 22.2 µs — more partials to write and fold)
constexpr int DECODE_KEYS_PER_STEP = 64;    // 4 waves × 16 keys
constexpr int DECODE_MAX_PARTS = 64;
struct AttnDecodePlan { int parts, per; };
inline AttnDecodePlan attn_decode_plan(int B, int KV, int n, bool have_ws, int cus) {
    const int steps = (n + DECODE_KEYS_PER_STEP - 1) / DECODE_KEYS_PER_STEP;
    int parts = std::min({steps, std::max(1, 2 * cus / (B * KV)), DECODE_MAX_PARTS});
    if (!have_ws) parts = 1;
    const int per = (steps + parts - 1) / parts;
    return {(steps + per - 1) / per, per};
}

// attention_extend (attn_extend.hip): n new queries per sequence at cache positions [pos, pos + n),
// causal over the pos + n cached keys.  A unit is one workgroup's 128 stacked rows: the G = H / KV
// query heads of one KV head × 128 / G consecutive queries, so a K/V tile is staged once per group;
// units = B · KV · ⌈n / (128 / G)⌉, query block fastest.  Every unit's 64-key tiles [0, its last
// diagonal] are cut into the same `parts` ranges of `tiles_per_part` tiles (the last unit holds all
// `tiles` of them; an earlier unit's ranges past its diagonal hold no key and weigh 0 in the fold).
// A grid of at least `cus` units is not split; a smaller one stops splitting where units × parts
// would pass ONE round of the planned CUs (the kernel holds one workgroup per CU) and keeps at
// least two tiles per part.  Measured at B = 1, 16 / 8 heads, one process (the CU knob moving the
// plan): 64 new queries over 1500 keys 26.3 µs as 24 parts of one tile, 19.1 as 12 parts of two;
// 512 over 1500 keys 47.1 µs as 8 parts (512 workgroups, two rounds), 32.6 as 4 parts (one round),
// 44.9 unsplit; 512 over 8192 keys 90.7 / 76.1 / 214.  The rule also bounds the partials
// (attn_extend_ws_bound): cus slabs of 128 rows × 132 floats, 17.3 MB at 256 CUs, whatever the shape.
constexpr int EXTEND_ROWS = 128;            // stacked rows per unit: 4 waves × 32
constexpr int EXTEND_MAX_PARTS = 64;
constexpr int EXTEND_PART_STRIDE = 132;     // floats per (row, part): m, l, 2 pad, o[128] (16-B aligned)
using AttnExtendPlan = acehip_attn_extend_plan;
inline AttnExtendPlan attn_extend_plan(int B, int H, int KV, int n, int pos, bool have_ws, int cus) {
    AttnExtendPlan p{};
    const int G = H / KV;
    p.unit_queries = EXTEND_ROWS / G;
    p.unit_rows = EXTEND_ROWS;
    p.qblocks = (n + p.unit_queries - 1) / p.unit_queries;
    p.units = B * KV * p.qblocks;
    p.tiles = (pos + n + ATTN_KT - 1) / ATTN_KT;
    int parts = (int)std::min<int64_t>({(int64_t)(p.tiles + 1) / 2, std::max<int64_t>(1, (int64_t)cus / p.units),
                                        (int64_t)EXTEND_MAX_PARTS});
    if (!have_ws || p.units >= cus) parts = 1;      // a grid that fills the CUs runs whole units
    p.tiles_per_part = (p.tiles + parts - 1) / parts;
    p.parts = (p.tiles + p.tiles_per_part - 1) / p.tiles_per_part;
    p.grid = p.units * p.parts;
    p.block = 256;
    p.uses_ws = p.parts > 1;
    return p;
}
// bytes of partials a plan writes (0: one part, straight to o)
inline size_t attn_extend_plan_ws_bytes(const AttnExtendPlan &p) {
    return p.parts > 1 ? (size_t)p.grid * EXTEND_ROWS * EXTEND_PART_STRIDE * sizeof(float) : 0;
}
// the most any plan of (B, H, n) writes on `cus` CUs, over every pos and every G in {1, 2, 4}:
// a split grid stays within cus workgroups
inline size_t attn_extend_ws_bound(int B, int H, int n, int cus) {
    int64_t units = 0;
    for (int G = 1; G <= 4; G *= 2)
        if (H % G == 0)
            units = std::max<int64_t>(units, (int64_t)B * (H / G) * ((n + EXTEND_ROWS / G - 1) / (EXTEND_ROWS / G)));
    const int64_t slabs = std::min<int64_t>((int64_t)cus, units * EXTEND_MAX_PARTS);
    return (size_t)std::max<int64_t>(slabs, 1) * EXTEND_ROWS * EXTEND_PART_STRIDE * sizeof(float);
}

}  // namespace acehip
