// attn_tile.h — the per-wave tile body of the flash-attention forward (head_dim 128): one wave,
// 32 query rows, one 64-key K/V tile held in LDS.  Shared by attn_fwd_kernel (attention.hip) and
// the fused cross-Q projection + cross-attention kernel (gemm.hip), so that a query row's
// arithmetic is one instruction sequence wherever its Q fragments come from.
//
// LDS tile image: a K or V tile is 64 rows of 256 B, 16-B chunks XOR-swizzled (kvoff) so that
// the K row reads (ds_read_b128) and the V transposed reads (ds_read_b64_tr_b16) are
// bank-conflict free.  v_mfma_f32_32x32x16_bf16 computes the swapped score tile Sᵀ = K·Qᵀ, so
// each lane owns one query row; Sᵀ's accumulator registers, converted to bf16, are directly the
// B operand of Oᵀ += Vᵀ·Pᵀ.  Online softmax in the exp2 domain with a lazy rescale.
#pragma once
#include "kernels.h"

namespace acehip {

constexpr float ATT_TAU = 8.0f;   // lazy-rescale threshold (0: rescale on every new max)
constexpr int KT = ATTN_KT;       // keys per tile
constexpr int KV_TILE = KT * 256; // one K or V tile image: 64 rows × 256 B
// Sentinels are powers of two so that NEG·sl2 is exact: the exp2 argument
// fmaf(NEG, sl2, −m) of a row whose max IS the sentinel is then exactly 0
// (an all-masked row weighs its keys uniformly, and a row's all-masked first
// tiles add finite garbage that the first real tile's rescale zeroes).  With a
// non-power-of-two sentinel the fma's unrounded product differs from the
// rounded max by up to half an ulp of 1e29 — exp2 of that is 0 or inf.
constexpr float NEG = -0x1p100f;
constexpr float PAST = -0x1p126f;   // masked mode: keys past Sk (never weighted, even in an all-masked row)

// ds_read_b64_tr_b16 by inline asm (see attn_wave_tile's P·V for why not the builtin)
__device__ __forceinline__ s16x4 ds_read_tr16(const char *lds_ptr) {
    s16x4 r;
    const uint32_t a = lds_addr(lds_ptr);
    asm volatile("ds_read_b64_tr_b16 %0, %1" : "=v"(r) : "v"(a));
    return r;
}

__device__ __forceinline__ bf16x8 ds_read_b128(const char *lds_ptr) {
    bf16x8 r;
    const uint32_t a = lds_addr(lds_ptr);
    asm volatile("ds_read_b128 %0, %1" : "=v"(r) : "v"(a));
    return r;
}
// LDS reads at (per-lane offset VGPR + compile-time immediate): the per-lane parts
// (swizzled chunk offsets) are 8 VGPRs for K and 8 for V; the ring slot and the row
// block are the instruction's 16-bit offset field (the tile loop is unrolled by the
// two ring slots so both are constants) — no address VALU per read, and no hoisted
// VGPR address per (slot, fragment), which had cost ~50 VGPRs and spills.
template <int OFF>
__device__ __forceinline__ bf16x8 ds_read_b128_imm(uint32_t lane_off) {
    static_assert(OFF >= 0 && OFF < 65536, "ds offset field");
    bf16x8 r;
    asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(r) : "v"(lane_off), "n"(OFF));
    return r;
}
template <int OFF>
__device__ __forceinline__ s16x4 ds_read_tr16_imm(uint32_t lane_off) {
    static_assert(OFF >= 0 && OFF < 65536, "ds offset field");
    s16x4 r;
    asm volatile("ds_read_b64_tr_b16 %0, %1 offset:%2" : "=v"(r) : "v"(lane_off), "n"(OFF));
    return r;
}
// s_waitcnt lgkmcnt(0) that the listed fragments depend on (nothing using them can be
// scheduled above it)
__device__ __forceinline__ void lgkm_wait8(bf16x8 (&f)[8]) {
    asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(f[0]), "+v"(f[1]), "+v"(f[2]), "+v"(f[3]), "+v"(f[4]), "+v"(f[5]),
                 "+v"(f[6]), "+v"(f[7]));
}

__device__ __forceinline__ int kvoff(int row, int ch) {
    return row * 256 + ((ch ^ (((row & 3) << 2) | ((row >> 2) & 3))) << 4);
}

// Per-lane swizzled LDS byte addresses of the fragment reads, relative to the K region (kbase)
// and the V region (vbase) of the ring — the ring slot and the row block are added as immediates:
// K fragment (row r [+32], logical chunk 2s+hh) — the swizzle depends on row & 15 only;
// Vᵀ fragment (d-block dt, row 4(g>>1)+qq [+8]) — rows +16s, +32t are uniform offsets
__device__ __forceinline__ void attn_lane_offsets(uint32_t kbase, uint32_t vbase, int lane, uint32_t (&koff)[8],
                                                  uint32_t (&voff)[4][2]) {
    const int r = lane & 31, hh = lane >> 5;
    const int g = lane >> 4, gi = lane & 15, qq = gi >> 2, pp = gi & 3;
#pragma unroll
    for (int s = 0; s < 8; ++s) koff[s] = kbase + kvoff(r, 2 * s + hh);
#pragma unroll
    for (int dt = 0; dt < 4; ++dt)
#pragma unroll
        for (int h8 = 0; h8 < 2; ++h8)
            voff[dt][h8] = vbase + kvoff(4 * (g >> 1) + qq + 8 * h8, 4 * dt + 2 * (g & 1) + (pp >> 1)) + 8 * (pp & 1);
}

// One K/V tile of one wave: Sᵀ = K·Qᵀ, the online softmax step on (m, l), Oᵀ += Vᵀ·Pᵀ.
//   KB / VB   byte offset of the tile's K / V image from koff's / voff's region base (compile-time:
//             the callers unroll their tile loop by the ring slots)
//   qf        Q fragments (B operand of Sᵀ): lane (r, hh) holds Q[row r][16s + 8hh .. +8]
//   interior  every key of the tile is admitted for every row of the wave (no mask pass);
//             otherwise mask(t, j, score) returns the score or the sentinel for the lane's key
//             32t + (j & 3) + 8(j >> 2) + 4hh of the tile
template <int KB, int VB, typename Mask>
__device__ __forceinline__ void attn_wave_tile(const bf16x8 (&qf)[8], const uint32_t (&koff)[8],
                                               const uint32_t (&voff)[4][2], f32x16 (&oacc)[4], float &m, float &l,
                                               float sl2, bool interior, Mask mask) {
    // Oᵀ[d][q] += Vᵀ·Pᵀ; Vᵀ fragments by transposed LDS reads.  The reads are issued by
    // inline asm: hipcc's waitcnt pass treats its own ds_read_tr builtin as an LDS read
    // that may alias the in-flight LDS-DMA refills and waits vmcnt(0) before it (every
    // tile, draining the ring); the asm reads are waited explicitly (lgkmcnt(0) bound to
    // their results, so no MFMA can move above the wait)
    // key rows +32t +16s are immediates
    auto pv_reads = [&](int dt, s16x4 (&rd)[2][2][2]) {
        rd[0][0][0] = ds_read_tr16_imm<VB>(voff[dt][0]);
        rd[0][0][1] = ds_read_tr16_imm<VB>(voff[dt][1]);
        rd[0][1][0] = ds_read_tr16_imm<VB + 16 * 256>(voff[dt][0]);
        rd[0][1][1] = ds_read_tr16_imm<VB + 16 * 256>(voff[dt][1]);
        rd[1][0][0] = ds_read_tr16_imm<VB + 32 * 256>(voff[dt][0]);
        rd[1][0][1] = ds_read_tr16_imm<VB + 32 * 256>(voff[dt][1]);
        rd[1][1][0] = ds_read_tr16_imm<VB + 48 * 256>(voff[dt][0]);
        rd[1][1][1] = ds_read_tr16_imm<VB + 48 * 256>(voff[dt][1]);
    };
    auto pv_wait = [](s16x4 (&rd)[2][2][2]) {
        asm volatile("s_waitcnt lgkmcnt(0)"
                     : "+v"(rd[0][0][0]), "+v"(rd[0][0][1]), "+v"(rd[0][1][0]), "+v"(rd[0][1][1]),
                       "+v"(rd[1][0][0]), "+v"(rd[1][0][1]), "+v"(rd[1][1][0]), "+v"(rd[1][1][1]));
    };
    auto pv_mfma = [&](int dt, const s16x4 (&rd)[2][2][2], const bf16x8 (&pf)[2][2]) {
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                // whole-vector reinterpretation (per-element bit_cast<__bf16> insertion
                // is miscompiled by ROCm 7.2 hipcc: it keeps only the first dword)
                const s16x8 cat = __builtin_shufflevector(rd[t][s][0], rd[t][s][1], 0, 1, 2, 3, 4, 5, 6, 7);
                const bf16x8 vf = __builtin_bit_cast(bf16x8, cat);
                oacc[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vf, pf[t][s], oacc[dt], 0, 0, 0);
            }
    };
    // P·V: the reads of d-block dt+1 are in flight during the MFMAs of dt
    auto pv = [&](const bf16x8 (&pf)[2][2]) {
        s16x4 ra[2][2][2], rb[2][2][2];
        pv_reads(0, ra);
        pv_wait(ra);
        pv_reads(1, rb);
        pv_mfma(0, ra, pf);
        pv_wait(rb);
        pv_reads(2, ra);
        pv_mfma(1, rb, pf);
        pv_wait(ra);
        pv_reads(3, rb);
        pv_mfma(2, ra, pf);
        pv_wait(rb);
        pv_mfma(3, rb, pf);
    };

    // Sᵀ tiles: keys 32t..32t+31 × this wave's 32 queries
    // K fragments by asm reads (see pv()); the reads of key half t=1 are in flight
    // during the MFMAs of t=0
    f32x16 st[2];
    {
        bf16x8 k0[8], k1[8];
#pragma unroll
        for (int s = 0; s < 8; ++s) k0[s] = ds_read_b128_imm<KB>(koff[s]);
        lgkm_wait8(k0);
#pragma unroll
        for (int s = 0; s < 8; ++s) k1[s] = ds_read_b128_imm<KB + 32 * 256>(koff[s]);
#pragma unroll
        for (int j = 0; j < 16; ++j) { st[0][j] = 0.f; st[1][j] = 0.f; }
#pragma unroll
        for (int s = 0; s < 8; ++s) st[0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(k0[s], qf[s], st[0], 0, 0, 0);
        lgkm_wait8(k1);
#pragma unroll
        for (int s = 0; s < 8; ++s) st[1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(k1[s], qf[s], st[1], 0, 0, 0);
    }
    // running max on raw scores (scale folded into the exp2 FMA below);
    // interior tiles of full / cross attention need no mask
    float mx = NEG;
    if (interior) {
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int j = 0; j < 16; ++j) mx = fmaxf(mx, st[t][j]);
    } else {
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int j = 0; j < 16; ++j) {
                const float sv = mask(t, j, st[t][j]);
                st[t][j] = sv;
                mx = fmaxf(mx, sv);
            }
    }
    mx = fmaxf(mx, __shfl_xor(mx, 32, 64)) * sl2;
    // lazy rescale: the running reference max moves only when a score exceeds it by more
    // than ATT_TAU (log2 units), so P = 2^(s − m) ≤ 2^TAU and after the first tiles the
    // O/l rescale (64 VALU per lane) is skipped almost always; O/l is the same softmax
    const float mn = mx > m + ATT_TAU ? mx : m;
    const float alpha = __builtin_amdgcn_exp2f(m - mn);   // raw v_exp_f32 (no denormal range fix-up)
    m = mn;
    float rs = 0.f;
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const float p = __builtin_amdgcn_exp2f(fmaf(st[t][j], sl2, -mn));
            st[t][j] = p;
            rs += p;
        }
    rs += __shfl_xor(rs, 32, 64);
    l = l * alpha + rs;
    if (__any(alpha != 1.0f)) {                  // skip the O rescale when no row's max grew
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 16; ++j) oacc[i][j] *= alpha;
    }

    // P (bf16) as the B operand: tile t, k-step s ← registers 8s..8s+7
    bf16x8 pf[2][2];
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int s = 0; s < 2; ++s)
#pragma unroll
            for (int j = 0; j < 8; ++j) pf[t][s][j] = (__bf16)st[t][8 * s + j];
    pv(pf);
}

// O row of one lane's query → op[0 .. 127] (bf16), normalised by 1 / l.  Both lanes of a row pair
// (lane, lane ^ 32) must call it: lane (r, hh) holds columns 32dt + 8gg + 4hh .. +3 of its row; the
// two half-waves swap one 4-column group per pair (gg, gg+1) so each lane stores 8 contiguous
// columns as one 16-B store (the store tail is issue-bound: MI355X_MICROARCH "attention epilogue
// store tail")
__device__ __forceinline__ void attn_wave_store_o(const f32x16 (&oacc)[4], float l, bf16_t *op, int hh) {
    const float inv = 1.0f / l;
#pragma unroll
    for (int dt = 0; dt < 4; ++dt)
#pragma unroll
        for (int gp = 0; gp < 2; ++gp) {
            float v[8];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float a0 = oacc[dt][8 * gp + j] * inv, a1 = oacc[dt][8 * gp + 4 + j] * inv;
                const float got = __shfl_xor(hh ? a0 : a1, 32, 64);
                v[j] = hh ? got : a0;
                v[4 + j] = hh ? a1 : got;
            }
            *(uint4 *)(op + 32 * dt + 16 * gp + 8 * hh) = pack8(v);
        }
}

}  // namespace acehip
