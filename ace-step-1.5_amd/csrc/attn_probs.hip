// attn_probs.hip — normalised cross-attention probabilities of selected heads.
//
// The flash kernels of attention.hip never form a normalised softmax row; the lyric
// aligners (reference handler/lyric_timestamp.py:78-111, lyric_score.py:93-138) need a
// few heads' rows, a key range of them, transposed to [key][query].  This kernel writes
// exactly that and nothing else:
//
//   out[slot][b][j − k0][s] = softmax_j(scale · q[b, head, s, :] · k[b, head / (H/KV), j, :])
//
// for j in [k0, k1), the softmax over ALL Sk keys (the decoder never masks encoder
// positions, base:1384-1385), each value rounded to bf16 (the reference's eager softmax is
// fp32 followed by .to(query.dtype)) and stored as fp32.
//
// One wave per (32 queries, selected head, batch row).  v_mfma_f32_32x32x16_bf16 computes
// the swapped tile Sᵀ = K·Qᵀ (A = 32 keys, B = 32 queries): in the result layout a lane owns
// query column lane & 31 and 16 key rows (reg & 3) + 8·(reg >> 2) + 4·(lane >> 5), so the
// row max / sum are per-lane register reductions plus one exchange with lane ^ 32, and one
// result register of the 32 lanes of a half is one key's 32 consecutive frames: a 128-B
// store.  Two passes over the key tiles: pass 1 the max and sum, pass 2 recomputes K·Qᵀ for
// the tiles that meet [k0, k1) and stores exp(s − m) / l (no Sk/32 accumulator tiles held).
// Both operands are read straight from global memory in their MFMA fragment layout (lane
// (r, h) holds row r, elements 16·step + 8h .. +7): 16-B loads, no LDS.  Rows past Sq / Sk
// are read from the clamped last row and masked (keys) or not stored (queries).
#include <cmath>

#include "kernels.h"

namespace acehip {

namespace {

constexpr float LOG2E = 1.4426950408889634f;

// scores of key tile kt against this wave's 32 queries, in the D layout described above
__device__ __forceinline__ f32x16 probs_tile(const bf16_t *K, int kt, int Sk, int r, const bf16x8 (&qf)[8]) {
    const bf16_t *Kr = K + (int64_t)min(kt * 32 + r, Sk - 1) * 128;
    bf16x8 kf[8];
#pragma unroll
    for (int s = 0; s < 8; ++s) kf[s] = *(const bf16x8 *)(Kr + 16 * s);
    f32x16 st;
#pragma unroll
    for (int j = 0; j < 16; ++j) st[j] = 0.f;
#pragma unroll
    for (int s = 0; s < 8; ++s) st = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf[s], qf[s], st, 0, 0, 0);
    return st;
}

__global__ __launch_bounds__(64) void attn_probs_kernel(const bf16_t *q, const bf16_t *k, int B, int H, int KV, int Sq,
                                                        int Sk, AttnProbsSel sel, int k0, int k1, float scale,
                                                        float *out) {
    const int lane = threadIdx.x, r = lane & 31, hf = lane >> 5;
    const int i = blockIdx.y, b = blockIdx.z;
    const int head = sel.head[i], kvh = head / (H / KV);
    const int qi = blockIdx.x * 32 + r;
    const bf16_t *Q = q + ((int64_t)(b * H + head) * Sq + min(qi, Sq - 1)) * 128 + 8 * hf;
    const bf16_t *K = k + (int64_t)(b * KV + kvh) * Sk * 128 + 8 * hf;
    bf16x8 qf[8];
#pragma unroll
    for (int s = 0; s < 8; ++s) qf[s] = *(const bf16x8 *)(Q + 16 * s);
    const float sl2 = scale * LOG2E;   // exponents in base 2: p = 2^(s·scale·log2 e − m)

    // pass 1: this lane's running max and sum over its 16 rows of every key tile
    float m = -INFINITY, l = 0.f;
    const int nt = (Sk + 31) / 32;
    for (int kt = 0; kt < nt; ++kt) {
        const f32x16 st = probs_tile(K, kt, Sk, r, qf);
        float t[16], tm = -INFINITY;
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const int key = kt * 32 + (j & 3) + 8 * (j >> 2) + 4 * hf;
            t[j] = key < Sk ? st[j] * sl2 : -INFINITY;
            tm = fmaxf(tm, t[j]);
        }
        const float mn = fmaxf(m, tm);
        if (mn > -INFINITY) {     // a lane half whose rows are all past Sk so far keeps (−inf, 0)
            float acc = 0.f;
#pragma unroll
            for (int j = 0; j < 16; ++j) acc += exp2f(t[j] - mn);
            l = l * exp2f(m - mn) + acc;
            m = mn;
        }
    }
    // the other 16 rows of every tile live in lane ^ 32 (key 0 is a row of half 0, so mt is finite)
    const float mo = __shfl_xor(m, 32, 64), lo = __shfl_xor(l, 32, 64);
    const float mt = fmaxf(m, mo);
    const float la = m > -INFINITY ? l * exp2f(m - mt) : 0.f;
    const float lb = mo > -INFINITY ? lo * exp2f(mo - mt) : 0.f;
    const float inv = 1.0f / (la + lb);

    // pass 2: the tiles that meet [k0, k1)
    const int64_t nk = k1 - k0;
    float *o = out + ((int64_t)sel.slot[i] * B + b) * nk * Sq;
    for (int kt = k0 / 32; kt <= (k1 - 1) / 32; ++kt) {
        const f32x16 st = probs_tile(K, kt, Sk, r, qf);
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const int key = kt * 32 + (j & 3) + 8 * (j >> 2) + 4 * hf;
            if (key >= k0 && key < k1 && qi < Sq) o[(int64_t)(key - k0) * Sq + qi] = rbf(exp2f(st[j] * sl2 - mt) * inv);
        }
    }
}

}  // namespace

int attention_probs_check(int B, int H, int KV, int Sq, int Sk, const AttnProbsSel &sel, int k0, int k1) {
    if (B <= 0 || B > 65535 || H <= 0 || KV <= 0 || H % KV || Sq <= 0 || Sk <= 0)
        return fail(-1, "attention_probs: B/H/KV/Sq/Sk out of range");
    if (sel.n < 1 || sel.n > 64) return fail(-1, "attention_probs: n must be in [1, 64]");
    for (int i = 0; i < sel.n; ++i) {
        if (sel.head[i] < 0 || sel.head[i] >= H) return fail(-1, "attention_probs: head index out of range");
        if (sel.slot[i] < 0) return fail(-1, "attention_probs: output slot out of range");
    }
    if (k0 < 0 || k0 >= k1 || k1 > Sk) return fail(-1, "attention_probs: key range must satisfy 0 <= k0 < k1 <= Sk");
    return 0;
}

int attention_probs(const bf16_t *q, const bf16_t *k, int B, int H, int KV, int Sq, int Sk, const AttnProbsSel &sel,
                    int k0, int k1, float scale, float *out, hipStream_t s) {
    if (!q || !k || !out) return fail(-1, "attention_probs: null argument");
    if (int rc = attention_probs_check(B, H, KV, Sq, Sk, sel, k0, k1)) return rc;
    const dim3 grid((unsigned)((Sq + 31) / 32), (unsigned)sel.n, (unsigned)B);
    attn_probs_kernel<<<grid, 64, 0, s>>>(q, k, B, H, KV, Sq, Sk, sel, k0, k1, scale, out);
    HIP_TRY(hipGetLastError());
    return 0;
}

}  // namespace acehip
