// attn_extend.hip — causal attention of n new queries per sequence over a K/V cache (head_dim
// 128, GQA): the multi-token continuation between the prefill (positions [0, S), flash kernels)
// and the one-token decode step (attn_decode.hip).
//
// q [B][H][n][128] (head-post's layout at S_dst_q = n); k / v [B][KV][cap][128], rows
// [0, pos + n) valid with the new tokens' rows already written; o [B·n][H·128] token-major;
// kmask [B][mask_ld] over cache positions (1 = attend) or null.  Query i attends keys
// j <= pos + i with kmask[b][j] != 0.
//
// Structure: attn_fwd_kernel<1>'s — 4 waves × 32 rows, 64-key K/V tiles in a 2-deep LDS ring
// filled by LDS-DMA (swizzle on the source address), the next tile in flight during the current
// tile's MFMAs, one raw barrier per tile, and the per-wave tile body of attn_tile.h — with three
// differences.  (1) The 128 rows of a workgroup are the G = H/KV query heads of one KV head
// stacked, G × 128/G queries, so a K/V tile is staged once per group (a wave's 32 rows belong to
// one head).  (2) K/V rows are `cap` apart and the causal diagonal sits at pos + i: a unit visits
// tiles up to its last row's diagonal only, a wave skips tiles past its own last diagonal, and
// tiles wholly before its first diagonal with no masked key take the tile body's interior path
// (no per-element selects).  (3) Exclusion follows attn_decode: an excluded score is −inf, so
// its probability is exp2(−inf) = 0 exactly, and before the tile body reads a V tile that holds a
// masked key, that key's V row is overwritten with zeros in LDS — whatever a masked cache row
// holds (NaN included) meets neither l nor O.  Rows at [pos + n, cap) are never fetched: the
// staging clamps to cache row pos + n − 1, and with a mask those copies are zeroed like masked
// rows (that row may be masked itself).  The running max
// starts at attn_tile.h's finite sentinel, from which the first admitted key's rescale factor is
// exp2(−huge) = 0; a row that admitted no key ends with l = 0 and is written as zeros, or as
// the partial (−inf, 0, 0).
//
// Key-range split (attn_plan.h attn_extend_plan): with parts > 1 every part writes fp32
// (m, l, o[128]) per stacked row to the workspace and attn_extend_fold_kernel folds them in part
// order with attn_decode's fold — no atomics, no tickets, so the same input gives the same bits
// on every call.
#include <cmath>

#include "attn_tile.h"
#include "kernels.h"
#include "../../include/acehip.h"

namespace acehip {
namespace {

constexpr int PSTRIDE = EXTEND_PART_STRIDE;

// One wave per SIMD: the tile body's live set (Q 32, O 64, two K fragment sets 64, Sᵀ 32, two Vᵀ
// read sets 32, P 16 VGPRs + addresses) is 347 registers here; held to 256 (two workgroups per
// CU) every instance spilled 52-344 B per lane to scratch, so the kernel takes the one-wave
// budget (219 VGPRs + 128 AGPRs, no scratch) and one workgroup per CU.
template <int G>
__global__ __launch_bounds__(256, 1) void attn_extend_kernel(const bf16_t *__restrict__ q, const bf16_t *__restrict__ k,
                                                             const bf16_t *__restrict__ v, bf16_t *__restrict__ o,
                                                             int H, int KV, int n, int pos, int cap,
                                                             const uint8_t *__restrict__ kmask, int mask_ld, float sl2,
                                                             int qblocks, int parts, int tpp, float *__restrict__ ws) {
    constexpr int QU = EXTEND_ROWS / G;            // queries per unit
    constexpr int TILE = KT * 256;                 // one K or V tile: 64 rows × 256 B
    constexpr int NBUF = 2;
    // [K slot 0, 1 | V slot 0, 1] (attn_fwd_kernel's ring), 64 KB
    __shared__ __attribute__((aligned(16))) char lds[NBUF * 2 * TILE];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);   // scalar: the head, q0 and tile classes are too
    const int r = lane & 31, hh = lane >> 5;
    const int u = blockIdx.x / parts, part = blockIdx.x % parts;
    const int qb = u % qblocks, kvh = (u / qblocks) % KV, b = u / (qblocks * KV);
    const int hq = kvh * G + (wave * 32) / QU;     // the wave's head
    const int q0 = qb * QU + (wave * 32) % QU;     // its first query
    const int qi = q0 + r;
    const int nk = pos + n;                        // valid cache rows

    const bf16_t *qp = q + (((int64_t)b * H + hq) * n + min(qi, n - 1)) * 128;
    bf16x8 qf[8];
#pragma unroll
    for (int s = 0; s < 8; ++s) qf[s] = *(const bf16x8 *)(qp + 16 * s + 8 * hh);
    // a wait the compiler sees, so that it does not re-wait vmcnt(0) for qf in every tile
    // (attn_fwd_kernel)
    __builtin_amdgcn_s_waitcnt(waitcnt_enc(0, 15));

    const bf16_t *kp = k + ((int64_t)b * KV + kvh) * (int64_t)cap * 128;
    const bf16_t *vp = v + ((int64_t)b * KV + kvh) * (int64_t)cap * 128;
    const uint8_t *km = kmask ? kmask + (int64_t)b * mask_ld : nullptr;
    // the unit's tiles end at its last query's diagonal; this part's range of them
    const int kv_hi = min(nk, pos + min(n, (qb + 1) * QU));
    const int nt_u = (kv_hi + KT - 1) / KT;
    const int t_first = min(nt_u, part * tpp);
    const int ntiles = min(nt_u, t_first + tpp) - t_first;

    // one K/V tile = 32 wave-instructions of 1 KiB, 8 per wave (attn_fwd_kernel's stage_tile);
    // rows past the valid range are clamped to the last valid row
    auto stage_tile = [&](int kv0, int buf) {
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int c = wave * 8 + i;
            const int isv = c >> 4, row = (c & 15) * 4 + (lane >> 4), pc = lane & 15;
            const int ch = pc ^ (((row & 3) << 2) | ((row >> 2) & 3));
            const int key = min(kv0 + row, nk - 1);
            glds16((isv ? vp : kp) + (int64_t)key * 128 + ch * 8, lds + (isv * NBUF + buf) * TILE + (c & 15) * 1024);
        }
    };
    // the lane's key of a tile (kv0 + lane) is admitted by the mask and inside the valid range
    auto key_ok = [&](int kv0) {
        const int kj = kv0 + lane;
        return kj < nk && (!km || km[min(kj, nk - 1)] != 0);
    };

    float m = NEG, l = 0.f;
    f32x16 oacc[4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 16; ++j) oacc[i][j] = 0.f;

    const uint32_t lds_base = lds_addr(lds);
    uint32_t koff[8], voff[4][2];
    attn_lane_offsets(lds_base, lds_base + NBUF * TILE, lane, koff, voff);

    auto tile_barrier = [&] {
        wait_vm_lgkm0<0>();
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
    };

    bool ok_next = ntiles > 0 ? key_ok(t_first * KT) : false;
    auto tile = [&](int it, auto SLOTC) {
        constexpr int SLOT = decltype(SLOTC)::value;
        constexpr int KB = SLOT * TILE, VB = SLOT * TILE;
        const int kv0 = (t_first + it) * KT;
        // bit j: key kv0 + j is valid and unmasked (the same value in every wave)
        const uint64_t okm = __ballot(ok_next);
        if (it + 1 < ntiles) {
            ok_next = key_ok(kv0 + KT);
            stage_tile(kv0 + KT, (SLOT + 1) % NBUF);
        }
        // V rows of masked keys → zeros (workgroup-uniform branch: every wave sees the same okm).
        // With a mask the image rows past the valid range go too: they are copies of cache row
        // nk − 1, which may itself be masked and hold anything.  Without a mask that row is valid,
        // its copies meet P = 0, and no tile pays the pass
        const uint64_t zero = km ? ~okm : 0ull;
        if (zero) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int idx = tid + 256 * i;     // 16-B chunk of the V image: row idx / 16
                if ((zero >> (idx >> 4)) & 1)
                    *(uint4 *)(lds + (NBUF + SLOT) * TILE + idx * 16) = make_uint4(0, 0, 0, 0);
            }
            wait_lgkm0();
            __builtin_amdgcn_s_barrier();
            asm volatile("" ::: "memory");
        }
        if (kv0 > pos + q0 + 31) {                 // wholly past this wave's last diagonal
            tile_barrier();
            return;
        }
        const bool interior = okm == ~0ull && kv0 + KT - 1 <= pos + q0;
        // the lane's keys are kv0 + 4hh + c, c = 32t + (j & 3) + 8(j >> 2) a constant per element:
        // mask bits and diagonal distance relative to key kv0 + 4hh
        const uint64_t okl = okm >> (4 * hh);
        const int rel = pos + qi - kv0 - 4 * hh;
        attn_wave_tile<KB, VB>(qf, koff, voff, oacc, m, l, sl2, interior, [&](int t, int j, float sc) {
            const int c = 32 * t + (j & 3) + 8 * (j >> 2);
            const bool ok = ((okl >> c) & 1) && c <= rel;
            return ok ? sc : -INFINITY;
        });
        tile_barrier();
    };
    if (ntiles > 0) stage_tile(t_first * KT, 0);
    tile_barrier();
    int it = 0;
    for (; it + 1 < ntiles; it += 2) {
        tile(it, IC<0>{});
        tile(it + 1, IC<1>{});
    }
    if (it < ntiles) tile(it, IC<0>{});

    if (qi >= n) return;                           // both lanes of a row pair agree
    if (parts == 1) {
        // l = 0: no admissible key; 1 / inf = 0 turns the (zero) accumulators into zeros
        attn_wave_store_o(oacc, l > 0.f ? l : INFINITY, o + ((int64_t)b * n + qi) * ((int64_t)H * 128) + hq * 128, hh);
        return;
    }
    // partial of stacked row 32·wave + r: lane (r, hh) holds o[32dt + 8gg + 4hh .. +3] in
    // oacc[dt][4gg .. 4gg + 3]
    float *w = ws + (((int64_t)u * parts + part) * EXTEND_ROWS + wave * 32 + r) * PSTRIDE;
    if (hh == 0) {
        w[0] = l > 0.f ? m : -INFINITY;
        w[1] = l;
    }
#pragma unroll
    for (int dt = 0; dt < 4; ++dt)
#pragma unroll
        for (int gg = 0; gg < 4; ++gg)
            *(f32x4 *)(w + 4 + 32 * dt + 8 * gg + 4 * hh) =
                f32x4{oacc[dt][4 * gg], oacc[dt][4 * gg + 1], oacc[dt][4 * gg + 2], oacc[dt][4 * gg + 3]};
}

// o[b·n + i][h·128 + d] = fold of the parts of (b, h, i) in part order; 128 threads = the 128 dims
__global__ __launch_bounds__(128) void attn_extend_fold_kernel(const float *__restrict__ ws, int H, int KV, int n,
                                                               int qblocks, int parts, bf16_t *__restrict__ o) {
    const int d = threadIdx.x;
    const int G = H / KV, QU = EXTEND_ROWS / G;
    const int i = blockIdx.x % n, h = (blockIdx.x / n) % H, b = blockIdx.x / (n * H);
    const int u = (b * KV + h / G) * qblocks + i / QU, row = (h % G) * QU + i % QU;
    const float *w = ws + ((int64_t)u * parts * EXTEND_ROWS + row) * PSTRIDE;
    const int64_t ps = (int64_t)EXTEND_ROWS * PSTRIDE;
    float mt = -INFINITY;
    for (int p = 0; p < parts; ++p) mt = fmaxf(mt, w[p * ps]);
    float l = 0.f, acc = 0.f;
    for (int p = 0; p < parts; ++p) {
        const float *wp = w + p * ps;
        const float a = wp[0] == -INFINITY ? 0.f : __builtin_amdgcn_exp2f(wp[0] - mt);
        l += wp[1] * a;
        acc += wp[4 + d] * a;
    }
    o[((int64_t)b * n + i) * ((int64_t)H * 128) + h * 128 + d] = f2bf(l > 0.f ? acc / l : 0.f);
}

}  // namespace

size_t attention_extend_ws_bytes(int B, int H, int n) {
    return attn_extend_ws_bound(std::max(B, 1), std::max(H, 1), std::max(n, 1), attn_env().cus);
}

int attention_extend(const bf16_t *q, const bf16_t *k, const bf16_t *v, bf16_t *o, int B, int H, int KV, int n, int pos,
                     int cap, const uint8_t *kmask, int mask_ld, float scale, void *ws, size_t ws_bytes,
                     hipStream_t s) {
    if (!q || !k || !v || !o) return fail(-1, "attention_extend: null argument");
    if (B <= 0 || H <= 0 || KV <= 0 || H % KV) return fail(-1, "attention_extend: B/H/KV out of range");
    const int G = H / KV;
    if (G != 1 && G != 2 && G != 4) return fail(-1, "attention_extend: heads/kv_heads must be 1, 2 or 4");
    if (n <= 0 || pos < 0 || (int64_t)pos + n > cap) return fail(-1, "attention_extend: need n >= 1, pos >= 0, pos + n <= cap");
    if (kmask && mask_ld < pos + n) return fail(-1, "attention_extend: mask_ld < pos + n");
    if ((int64_t)B * KV * ((n + EXTEND_ROWS / G - 1) / (EXTEND_ROWS / G)) > (1 << 24) || (int64_t)B * n * H > INT32_MAX)
        return fail(-1, "attention_extend: grid out of range");
    const AttnExtendPlan p = attn_extend_plan(B, H, KV, n, pos, ws != nullptr, attn_env().cus);
    if (ws_bytes < attn_extend_plan_ws_bytes(p)) return fail(-1, "attention_extend: workspace smaller than the plan needs");
    const float sl2 = scale * 1.4426950408889634f;
    float *wsf = p.uses_ws ? (float *)ws : nullptr;
#define EXT_LAUNCH(GG)                                                                                              \
    attn_extend_kernel<GG><<<(unsigned)p.grid, p.block, 0, s>>>(q, k, v, o, H, KV, n, pos, cap, kmask, mask_ld, sl2, \
                                                                 p.qblocks, p.parts, p.tiles_per_part, wsf)
    if (G == 1) EXT_LAUNCH(1);
    else if (G == 2) EXT_LAUNCH(2);
    else EXT_LAUNCH(4);
#undef EXT_LAUNCH
    HIP_TRY(hipGetLastError());
    if (p.parts > 1) {
        attn_extend_fold_kernel<<<(unsigned)(B * n * H), 128, 0, s>>>(wsf, H, KV, n, p.qblocks, p.parts, o);
        HIP_TRY(hipGetLastError());
    }
    return 0;
}

}  // namespace acehip

extern "C" {

size_t acehip_attention_extend_ws_bytes(int B, int H, int n) { return acehip::attention_extend_ws_bytes(B, H, n); }

int acehip_attention_extend_bf16(const void *q, const void *k, const void *v, void *o, int B, int H, int KV, int n,
                                 int pos, int cap, const uint8_t *kmask, int mask_ld, float scale, void *ws,
                                 size_t ws_bytes, void *stream) {
    return acehip::attention_extend((const bf16_t *)q, (const bf16_t *)k, (const bf16_t *)v, (bf16_t *)o, B, H, KV, n,
                                    pos, cap, kmask, mask_ld, scale, ws, ws_bytes, (hipStream_t)stream);
}

int acehip_diag_attn_extend_plan(int B, int H, int KV, int n, int pos, int have_ws, int device_cus,
                                 acehip_attn_extend_plan *out, size_t *ws_need) {
    using namespace acehip;
    if (!out || B <= 0 || H <= 0 || KV <= 0 || H % KV || n <= 0 || pos < 0 || device_cus < 0)
        return fail(ACEHIP_E_ARG, "diag_attn_extend_plan: a shape attention_extend refuses, or a null plan");
    const int G = H / KV;
    if (G != 1 && G != 2 && G != 4) return fail(ACEHIP_E_ARG, "diag_attn_extend_plan: heads/kv_heads must be 1, 2 or 4");
    *out = attn_extend_plan(B, H, KV, n, pos, have_ws != 0, attn_env(device_cus).cus);
    if (ws_need) *ws_need = attn_extend_plan_ws_bytes(*out);
    return 0;
}

}  // extern "C"
