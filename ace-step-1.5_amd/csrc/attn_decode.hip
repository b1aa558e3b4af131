// attn_decode.hip — single-token attention over a K/V cache (head_dim 128, GQA) and the
// vocabulary projection of the 5 Hz LM's token loop.
//
// attn_decode: one query per head, q [B][H][128], against cached K / V [B][KV][cap][128] of
// which the first n rows are valid; an optional key mask [B][mask_ld] (1 = attend) removes
// the left padding of a batched prompt.  o [B][H·128] token-major (the O projection's A
// operand).  The work is a byte stream — every K and V row is read once, straight from global
// memory into VGPRs in 16-B loads (no LDS ring), and shared by the G = H/KV query heads of its
// KV head; the dot products are VALU FMAs in fp32 — but at the LM's sizes the kernel is
// latency-bound, not bandwidth-bound: 21.8 µs at 2304 keys, B·KV = 16, against a 2.4 µs HBM
// floor (0.87 TB/s), with about one 4-wave workgroup per CU and eight loads in flight per lane.
//
// Work split: grid (parts, KV, B), 4 waves per workgroup.  A wave reads 16 keys per step:
// lane (rr = lane >> 4, c = lane & 15) holds elements 8c..8c+7 of keys 4u + rr (u = 0..3), so
// one wave-wide load is four whole 256-B rows; all eight loads (K and V) of a step are issued
// before the first FMA.  A score is the 16-lane sum of the lane partials (four xor shuffles);
// every 16-lane group keeps its own online softmax (m, l, o[8]) per head, folded across the
// four groups, then the four waves (LDS), at the end.  A masked or out-of-range key is
// excluded by selects on its score, its probability and its V row — whatever the cache holds
// there (NaN included) never reaches an accumulator.  State starts at (m, l) = (−inf, 0) and
// every rescale factor of a −inf state is a select to 0, so a part without a single
// admissible key yields (−inf, 0, 0) and no NaN.
//
// With more than one part each workgroup writes fp32 (m, l, o[128]) per head to the
// workspace and attn_decode_fold_kernel folds them in part order: the result does not depend
// on scheduling and is bit-identical from call to call.
//
// lm_head: y[m][n] = bf16(Σ_k x[m][k]·W[n][k]), M ≤ 16 and N ≈ 2·10⁵: a pure weight stream.
// One wave owns R consecutive rows of W and issues their loads of a 512-column chunk
// together (R·16 B per lane in flight); x stays in L1/L2.
#include <cmath>

#include "kernels.h"
#include "../../include/acehip.h"

namespace acehip {
namespace {

constexpr float LOG2E_D = 1.4426950408889634f;
constexpr int PART_STRIDE = 132;     // floats per (head, part): m, l, 2 pad, o[128] (16-B aligned)
constexpr int KEYS_PER_STEP = DECODE_KEYS_PER_STEP;   // 4 waves × 16 keys (attn_plan.h)
constexpr int MAX_PARTS = DECODE_MAX_PARTS;

__device__ __forceinline__ float ex2(float x) { return __builtin_amdgcn_exp2f(x); }

// (m, l, o) ← fold((m, l, o), (m2, l2, o2)); a −inf side weighs 0
template <int N>
__device__ __forceinline__ void fold_state(float &m, float &l, float (&o)[N], float m2, float l2, const float (&o2)[N]) {
    const float mt = fmaxf(m, m2);
    const float a1 = m == -INFINITY ? 0.f : ex2(m - mt);
    const float a2 = m2 == -INFINITY ? 0.f : ex2(m2 - mt);
    l = l * a1 + l2 * a2;
#pragma unroll
    for (int j = 0; j < N; ++j) o[j] = o[j] * a1 + o2[j] * a2;
    m = mt;
}

template <int G>
__global__ __launch_bounds__(256) void attn_decode_kernel(const bf16_t *__restrict__ q, const bf16_t *__restrict__ k,
                                                          const bf16_t *__restrict__ v,
                                                          const uint8_t *__restrict__ kmask, int mask_ld, int n,
                                                          int cap, int H, int KV, float sl2, int kper, int parts,
                                                          float *__restrict__ ws, bf16_t *__restrict__ o) {
    __shared__ float sm[4][G][16][10];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int rr = lane >> 4, c = lane & 15;
    const int part = blockIdx.x, kvh = blockIdx.y, b = blockIdx.z;
    const int k0 = part * kper, k1 = min(n, k0 + kper);
    const bf16_t *Kb = k + ((int64_t)b * KV + kvh) * (int64_t)cap * 128 + 8 * c;
    const bf16_t *Vb = v + ((int64_t)b * KV + kvh) * (int64_t)cap * 128 + 8 * c;
    const uint8_t *km = kmask ? kmask + (int64_t)b * mask_ld : nullptr;

    float qf[G][8];
#pragma unroll
    for (int g = 0; g < G; ++g) {
        unpack8(*(const uint4 *)(q + ((int64_t)b * H + kvh * G + g) * 128 + 8 * c), qf[g]);
#pragma unroll
        for (int j = 0; j < 8; ++j) qf[g][j] *= sl2;     // scores in the exp2 domain
    }
    float m[G], l[G], acc[G][8];
#pragma unroll
    for (int g = 0; g < G; ++g) {
        m[g] = -INFINITY;
        l[g] = 0.f;
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[g][j] = 0.f;
    }

    for (int kb = k0 + wave * 16; kb < k1; kb += KEYS_PER_STEP) {
        uint4 kq[4], vq[4];
        bool ok[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int key = kb + 4 * u + rr;
            const int kc = min(key, n - 1);              // rows past the range: a real row, dropped below
            ok[u] = key < k1 && (!km || km[kc] != 0);
            kq[u] = *(const uint4 *)(Kb + (int64_t)kc * 128);
            vq[u] = *(const uint4 *)(Vb + (int64_t)kc * 128);
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            float kf[8], vf[8];
            unpack8(kq[u], kf);
            unpack8(ok[u] ? vq[u] : make_uint4(0, 0, 0, 0), vf);
#pragma unroll
            for (int g = 0; g < G; ++g) {
                float s = 0.f;
#pragma unroll
                for (int j = 0; j < 8; ++j) s = fmaf(qf[g][j], kf[j], s);
                s += __shfl_xor(s, 1, 64);
                s += __shfl_xor(s, 2, 64);
                s += __shfl_xor(s, 4, 64);
                s += __shfl_xor(s, 8, 64);
                s = ok[u] ? s : -INFINITY;
                const float mn = fmaxf(m[g], s);
                const float alpha = m[g] == -INFINITY ? 0.f : ex2(m[g] - mn);
                const float p = ok[u] ? ex2(s - mn) : 0.f;
                l[g] = l[g] * alpha + p;
#pragma unroll
                for (int j = 0; j < 8; ++j) acc[g][j] = fmaf(p, vf[j], acc[g][j] * alpha);
                m[g] = mn;
            }
        }
    }

    // the wave's four 16-lane groups
#pragma unroll
    for (int g = 0; g < G; ++g) {
#pragma unroll
        for (int off = 16; off <= 32; off <<= 1) {
            const float m2 = __shfl_xor(m[g], off, 64), l2 = __shfl_xor(l[g], off, 64);
            float o2[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) o2[j] = __shfl_xor(acc[g][j], off, 64);
            fold_state(m[g], l[g], acc[g], m2, l2, o2);
        }
        if (rr == 0) {
            sm[wave][g][c][0] = m[g];
            sm[wave][g][c][1] = l[g];
#pragma unroll
            for (int j = 0; j < 8; ++j) sm[wave][g][c][2 + j] = acc[g][j];
        }
    }
    __syncthreads();
    if (tid >= G * 16) return;
    // the four waves, in wave order
    const int g = tid >> 4, cc = tid & 15;
    float mm = sm[0][g][cc][0], ll = sm[0][g][cc][1], oo[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) oo[j] = sm[0][g][cc][2 + j];
    for (int w = 1; w < 4; ++w) {
        float o2[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) o2[j] = sm[w][g][cc][2 + j];
        fold_state(mm, ll, oo, sm[w][g][cc][0], sm[w][g][cc][1], o2);
    }
    const int h = kvh * G + g;
    if (parts == 1) {
        const float inv = ll > 0.f ? 1.0f / ll : 0.f;     // no admissible key at all: zeros
#pragma unroll
        for (int j = 0; j < 8; ++j) oo[j] *= inv;
        *(uint4 *)(o + ((int64_t)b * H + h) * 128 + 8 * cc) = pack8(oo);
    } else {
        float *w = ws + (((int64_t)b * H + h) * parts + part) * PART_STRIDE;
        if (cc == 0) {
            w[0] = mm;
            w[1] = ll;
        }
        *(f32x4 *)(w + 4 + 8 * cc) = f32x4{oo[0], oo[1], oo[2], oo[3]};
        *(f32x4 *)(w + 8 + 8 * cc) = f32x4{oo[4], oo[5], oo[6], oo[7]};
    }
}

// o[b][h·128 + d] = fold of the parts of (b, h) in part order; 128 threads = the 128 dims
__global__ __launch_bounds__(128) void attn_decode_fold_kernel(const float *__restrict__ ws, int parts,
                                                               bf16_t *__restrict__ o) {
    const int d = threadIdx.x;
    const int64_t bh = blockIdx.x;
    const float *w = ws + bh * parts * PART_STRIDE;
    float mt = -INFINITY;
    for (int p = 0; p < parts; ++p) mt = fmaxf(mt, w[(int64_t)p * PART_STRIDE]);
    float l = 0.f, acc = 0.f;
    for (int p = 0; p < parts; ++p) {
        const float *wp = w + (int64_t)p * PART_STRIDE;
        const float a = wp[0] == -INFINITY ? 0.f : ex2(wp[0] - mt);
        l += wp[1] * a;
        acc += wp[4 + d] * a;
    }
    o[bh * 128 + d] = f2bf(l > 0.f ? acc / l : 0.f);
}

// ------------------------------------------------------------------ lm_head ---
template <int MB, int R>
__global__ __launch_bounds__(256) void lm_head_kernel(const bf16_t *__restrict__ x, int64_t ldx,
                                                      const bf16_t *__restrict__ W, bf16_t *__restrict__ y,
                                                      int64_t ldy, int M, int N, int K) {
    const int lane = threadIdx.x & 63;
    const int n0 = (blockIdx.x * 4 + (threadIdx.x >> 6)) * R;
    if (n0 >= N) return;
    float acc[R][MB];
#pragma unroll
    for (int r = 0; r < R; ++r)
#pragma unroll
        for (int m = 0; m < MB; ++m) acc[r][m] = 0.f;
    const bf16_t *wr[R];
#pragma unroll
    for (int r = 0; r < R; ++r) wr[r] = W + (int64_t)min(n0 + r, N - 1) * K;   // rows past N: the last row, not stored
#pragma unroll 2
    for (int kk = lane * 8; kk < K; kk += 512) {
        uint4 wq[R];
#pragma unroll
        for (int r = 0; r < R; ++r) wq[r] = __builtin_bit_cast(uint4, __builtin_nontemporal_load((const u32x4 *)(wr[r] + kk)));   // streamed once
        float xv[MB][8];
#pragma unroll
        for (int m = 0; m < MB; ++m) unpack8(*(const uint4 *)(x + (int64_t)min(m, M - 1) * ldx + kk), xv[m]);
#pragma unroll
        for (int r = 0; r < R; ++r) {
            float wv[8];
            unpack8(wq[r], wv);
#pragma unroll
            for (int m = 0; m < MB; ++m)
#pragma unroll
                for (int j = 0; j < 8; ++j) acc[r][m] = fmaf(wv[j], xv[m][j], acc[r][m]);
        }
    }
#pragma unroll
    for (int r = 0; r < R; ++r)
#pragma unroll
        for (int m = 0; m < MB; ++m) {
            const float s = wave_sum(acc[r][m]);
            if (lane == r * MB + m && m < M && n0 + r < N) y[(int64_t)m * ldy + n0 + r] = f2bf(s);
        }
}

}  // namespace

size_t attention_decode_ws_bytes(int B, int H) {
    return (size_t)std::max(B, 1) * std::max(H, 1) * MAX_PARTS * PART_STRIDE * sizeof(float);
}

int attention_decode(const bf16_t *q, const bf16_t *k, const bf16_t *v, bf16_t *o, int B, int H, int KV, int n,
                     int cap, const uint8_t *kmask, int mask_ld, float scale, void *ws, size_t ws_bytes,
                     hipStream_t s) {
    if (!q || !k || !v || !o) return fail(-1, "attention_decode: null argument");
    if (B <= 0 || B > 65535 || H <= 0 || KV <= 0 || KV > 65535 || H % KV)
        return fail(-1, "attention_decode: B/H/KV out of range");
    const int G = H / KV;
    if (G != 1 && G != 2 && G != 4) return fail(-1, "attention_decode: heads/kv_heads must be 1, 2 or 4");
    if (n <= 0 || n > cap) return fail(-1, "attention_decode: need 0 < n <= cap");
    if (kmask && mask_ld < n) return fail(-1, "attention_decode: mask_ld < n");
    const bool have_ws = ws && ws_bytes >= attention_decode_ws_bytes(B, H);
    const auto [parts, per] = attn_decode_plan(B, KV, n, have_ws, attn_env().cus);   // key ranges (attn_plan.h)
    const dim3 grid((unsigned)parts, (unsigned)KV, (unsigned)B);
    const float sl2 = scale * LOG2E_D;
    const int kper = per * KEYS_PER_STEP;
    if (G == 1)
        attn_decode_kernel<1><<<grid, 256, 0, s>>>(q, k, v, kmask, mask_ld, n, cap, H, KV, sl2, kper, parts, (float *)ws, o);
    else if (G == 2)
        attn_decode_kernel<2><<<grid, 256, 0, s>>>(q, k, v, kmask, mask_ld, n, cap, H, KV, sl2, kper, parts, (float *)ws, o);
    else
        attn_decode_kernel<4><<<grid, 256, 0, s>>>(q, k, v, kmask, mask_ld, n, cap, H, KV, sl2, kper, parts, (float *)ws, o);
    HIP_TRY(hipGetLastError());
    if (parts > 1) {
        attn_decode_fold_kernel<<<(unsigned)(B * H), 128, 0, s>>>((const float *)ws, parts, o);
        HIP_TRY(hipGetLastError());
    }
    return 0;
}

int lm_head(const bf16_t *x, int64_t ldx, const bf16_t *W, bf16_t *y, int64_t ldy, int M, int N, int K, hipStream_t s) {
    if (!x || !W || !y) return fail(-1, "lm_head: null argument");
    if (M <= 0 || M > 16 || N <= 0 || K <= 0 || K % 8 || ldx % 8 || ldx < K || ldy < N)
        return fail(-1, "lm_head: need 0 < M <= 16, K % 8 == 0, ldx % 8 == 0, ldx >= K, ldy >= N");
    if (M <= 2) {
        lm_head_kernel<2, 4><<<(unsigned)((N + 15) / 16), 256, 0, s>>>(x, ldx, W, y, ldy, M, N, K);
    } else if (M <= 4) {
        lm_head_kernel<4, 4><<<(unsigned)((N + 15) / 16), 256, 0, s>>>(x, ldx, W, y, ldy, M, N, K);
    } else {
        lm_head_kernel<16, 2><<<(unsigned)((N + 7) / 8), 256, 0, s>>>(x, ldx, W, y, ldy, M, N, K);
    }
    HIP_TRY(hipGetLastError());
    return 0;
}

}  // namespace acehip

extern "C" {

size_t acehip_attention_decode_ws_bytes(int B, int H) { return acehip::attention_decode_ws_bytes(B, H); }

int acehip_attention_decode_bf16(const void *q, const void *k, const void *v, void *o, int B, int H, int KV, int n,
                                 int cap, const uint8_t *kmask, int mask_ld, float scale, void *ws, size_t ws_bytes,
                                 void *stream) {
    return acehip::attention_decode((const bf16_t *)q, (const bf16_t *)k, (const bf16_t *)v, (bf16_t *)o, B, H, KV, n,
                                    cap, kmask, mask_ld, scale, ws, ws_bytes, (hipStream_t)stream);
}

int acehip_lm_head_bf16(const void *x, int ldx, const void *W, void *y, int ldy, int M, int N, int K, void *stream) {
    return acehip::lm_head((const bf16_t *)x, ldx, (const bf16_t *)W, (bf16_t *)y, ldy, M, N, K, (hipStream_t)stream);
}

}  // extern "C"
