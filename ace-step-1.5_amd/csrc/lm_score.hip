// lm_score.hip — teacher-forced scoring head of the 5 Hz LM (core/scoring/lm_score.py:
// _calculate_log_prob / _calculate_topk_recall): per target row the log-probability and the rank
// of the target token, from the vocabulary projection fused with its reductions.  No [T, V]
// matrix is ever written.
//
// With logit[r][n] = bf16(Σ_k x[r][k]·W[n][k]) (fp32 MFMA accumulate, rounded as a bf16 lm_head
// rounds its output):
//   lse[r] = log Σ_n exp(logit[r][n]),  logprob[r] = logit[r][target[r]] − lse[r],
//   n_greater[r] = #{n : logit[r][n] > logit[r][target[r]]},
//   n_equal_lower[r] = #{n < target[r] : logit[r][n] == logit[r][target[r]]}.
//
// Tile kernel (lms_tile_kernel): 128 rows × 128 vocabulary columns × 64 k, 4 waves (2 × 2, 64×64
// wave tiles = 2×2 v_mfma_f32_32x32x16_bf16), both operands by LDS-DMA into a 2-stage ring of
// 128-B rows, XOR-swizzled on the source address (common.h swz), vmcnt(0) and one barrier per
// K-tile (conv_gemm_kernel's loop).  The MFMA computes the swapped tile Lᵀ = W·xᵀ, so a lane owns
// ONE row of x (lane & 31) and 16 vocabulary columns per accumulator: a row's reductions are
// register loops plus one exchange with lane ^ 32 and one LDS exchange between the two waves
// that share the row.  A workgroup owns one column tile (blockIdx.x) and walks the row tiles of
// its group (blockIdx.y, up to 8 row tiles = 1024 rows), so W leaves HBM once per group of row
// tiles; a later row tile finds the W tile in L2 / Infinity Cache.  Ragged edges: loads of rows
// >= T and of columns >= V are clamped to the last valid one, such columns are −inf in pass A,
// uncounted in pass B, and such rows write nothing.
//
// The same tile code runs twice (template PASS):
//   pass A  per (row, column tile): m = max of the tile's 128 logits, s = Σ exp(logit − m); the
//           lane that holds column target[r] writes that logit to tl[r].  lms_finish_kernel<0>
//           (one wave per row) folds the tiles: M = max m, lse = M + log Σ_t s_t·exp(m_t − M).
//   pass B  recomputes the tiles — identical instructions on identical operands, so every
//           logit has the bits it had in pass A — and counts > and ==-with-lower-index against
//           tl[r]; per (row, column tile) one packed int32 partial.  lms_finish_kernel<1> sums.
// Nothing is accumulated by atomics: every partial has one writer and every fold a fixed order, so
// the same input gives the same bits on every call.
//
// L, the longest chain of additions that feeds one lse (an add onto the initial 0 counted):
// 32 in a lane (32 values of one row in a tile, sequential) + 1 (lane ^ 32) + 1 (the two waves of
// a row) — these 34 in fp32 — + ceil(tiles / 64) (a finish lane folds tiles lane, lane + 64, …
// sequentially) + 6 (butterfly over the 64 lanes) — these in fp64 —
// = 40 + ceil(ceil(V / 128) / 64): 67 at V = 217204, 1064 at the largest V (2^23) — L <= 2048.
// Besides the chain an lse carries one fp32 exp per term and the rounding of the result to fp32.
//
// Workspace: two fp32 / int32 planes [tiles][T] (m then the packed counts; s) and tl[T]:
// (2·ceil(V/128) + 1)·T·4 bytes — O(T·V/BN).
#include <algorithm>

#include "kernels.h"
#include "../../include/acehip.h"

namespace acehip {
namespace {

constexpr int BM = 128, BN = 128, BK = 64;
constexpr int STAGE = (BM + BN) * 128;      // bytes of one K-tile: [x rows | W rows], 128-B rows
constexpr int GROUP = 8;                    // row tiles one workgroup walks
constexpr int MAX_T = 8192, MAX_V = 1 << 23;

struct ScoreArgs {
    const bf16_t *x; int64_t ldx;
    const bf16_t *W;
    const int32_t *targets;
    int T, V, K;
    float *pm;          // [tiles][T]  pass A: tile max; pass B: packed counts (int32 image)
    float *ps;          // [tiles][T]  pass A: tile sum of exponentials
    float *tl;          // [T]         the target's logit (NaN for a target outside [0, V))
    float *logprob, *lse;
    int32_t *n_greater, *n_equal_lower;
};

// vocabulary column of accumulator register `reg` in lane half h (32×32 C/D map: the row index)
__device__ __forceinline__ int crow(int reg, int h) { return (reg & 3) + 8 * (reg >> 2) + 4 * h; }

template <int PASS>
__global__ __launch_bounds__(256, 2) void lms_tile_kernel(ScoreArgs a) {
    __shared__ __attribute__((aligned(16))) char lds[2 * STAGE];
    __shared__ float xm[2][BM];       // per wave column (wn): a row's max, then its sum / counts
    __shared__ float xs[2][BM];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    const int lr = lane & 31, h = lane >> 5;
    const int tile = blockIdx.x;
    const int n0 = tile * BN;
    const int tilesM = (a.T + BM - 1) / BM;
    const int tm0 = blockIdx.y * GROUP, tm1 = min(tm0 + GROUP, tilesM);
    const int K = a.K, nk = K / BK;

    // staging: 32 pieces of 1 KiB (8 rows) per stage, 8 per wave; piece q covers rows 8q..8q+7;
    // the W rows of this workgroup do not change over the row tiles
    const bf16_t *wsrc[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int r = (wave + 4 * i) * 8 + (lane >> 3);
        const int c = (lane & 7) ^ ((r >> 1) & 7);
        wsrc[i] = a.W + (int64_t)min(n0 + r, a.V - 1) * K + c * 8;
    }

    for (int tm = tm0; tm < tm1; ++tm) {
        const int m0 = tm * BM;
        const bf16_t *xsrc[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int r = (wave + 4 * i) * 8 + (lane >> 3);
            const int c = (lane & 7) ^ ((r >> 1) & 7);
            xsrc[i] = a.x + (int64_t)min(m0 + r, a.T - 1) * a.ldx + c * 8;
        }
        auto stage = [&](int buf, int k0) {
            char *b = lds + buf * STAGE;
#pragma unroll
            for (int i = 0; i < 4; ++i) glds16(xsrc[i] + k0, b + (wave + 4 * i) * 1024);
#pragma unroll
            for (int i = 0; i < 4; ++i) glds16(wsrc[i] + k0, b + BM * 128 + (wave + 4 * i) * 1024);
        };

        f32x16 acc[2][2];     // [i: row block of 32][j: column block of 32]
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;

        __syncthreads();      // the previous row tile's LDS reads are over
        stage(0, 0);
        for (int kt = 0; kt < nk; ++kt) {
            wait_vm_lgkm0<0>();
            __builtin_amdgcn_s_barrier();
            asm volatile("" ::: "memory");
            if (kt + 1 < nk) stage((kt + 1) & 1, (kt + 1) * BK);
            const char *b = lds + (kt & 1) * STAGE;
#pragma unroll
            for (int ks = 0; ks < 4; ++ks) {
                bf16x8 xf[2], wf[2];
#pragma unroll
                for (int i = 0; i < 2; ++i) {
                    xf[i] = *(const bf16x8 *)(b + swz(wm * 64 + i * 32 + lr, ks * 2 + h));
                    wf[i] = *(const bf16x8 *)(b + swz(BM + wn * 64 + i * 32 + lr, ks * 2 + h));
                }
#pragma unroll
                for (int i = 0; i < 2; ++i)
#pragma unroll
                    for (int j = 0; j < 2; ++j)
                        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wf[j], xf[i], acc[i][j], 0, 0, 0);
            }
        }

        // epilogue: lane (lr, h) holds, for row block i, row m0 + wm·64 + i·32 + lr and the
        // columns n0 + wn·64 + j·32 + crow(e, h)
        int tgt[2];
        float tv[2];
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int row = m0 + wm * 64 + i * 32 + lr;
            const int t = row < a.T ? a.targets[row] : -1;
            tgt[i] = (t >= 0 && t < a.V) ? t : -1;
            tv[i] = (PASS == 1 && row < a.T) ? a.tl[row] : 0.f;
        }
        const int nbase = n0 + wn * 64;
        if constexpr (PASS == 0) {
            float mx[2];
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const int row = m0 + wm * 64 + i * 32 + lr;
                float m = -INFINITY;
#pragma unroll
                for (int j = 0; j < 2; ++j)
#pragma unroll
                    for (int e = 0; e < 16; ++e) {
                        const int n = nbase + j * 32 + crow(e, h);
                        const float v = n < a.V ? rbf(acc[i][j][e]) : -INFINITY;
                        acc[i][j][e] = v;
                        m = fmaxf(m, v);
                        if (n == tgt[i]) a.tl[row] = v;      // tgt >= 0 implies row < T and n < V
                    }
                m = fmaxf(m, __shfl_xor(m, 32, 64));
                if (h == 0) xm[wn][wm * 64 + i * 32 + lr] = m;
            }
            __syncthreads();
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const int rl = wm * 64 + i * 32 + lr;
                mx[i] = fmaxf(xm[0][rl], xm[1][rl]);       // finite: a tile has a column < V
                float s = 0.f;
#pragma unroll
                for (int j = 0; j < 2; ++j)
#pragma unroll
                    for (int e = 0; e < 16; ++e) s += expf(acc[i][j][e] - mx[i]);
                s += __shfl_xor(s, 32, 64);
                if (h == 0) xs[wn][rl] = s;
            }
            __syncthreads();
            if (wn == 0 && h == 0) {
#pragma unroll
                for (int i = 0; i < 2; ++i) {
                    const int rl = wm * 64 + i * 32 + lr, row = m0 + rl;
                    if (row < a.T) {
                        a.pm[(int64_t)tile * a.T + row] = mx[i];
                        a.ps[(int64_t)tile * a.T + row] = xs[0][rl] + xs[1][rl];
                    }
                }
            }
        } else {
            int *xc = (int *)&xm[0][0];
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                int gt = 0, eq = 0;
#pragma unroll
                for (int j = 0; j < 2; ++j)
#pragma unroll
                    for (int e = 0; e < 16; ++e) {
                        const int n = nbase + j * 32 + crow(e, h);
                        const float v = rbf(acc[i][j][e]);
                        gt += (n < a.V && v > tv[i]) ? 1 : 0;
                        eq += (n < tgt[i] && v == tv[i]) ? 1 : 0;     // n < tgt < V
                    }
                int c = gt | (eq << 16);                              // each <= 128 per tile
                c += __shfl_xor(c, 32, 64);
                if (h == 0) xc[wn * BM + wm * 64 + i * 32 + lr] = c;
            }
            __syncthreads();
            if (wn == 0 && h == 0) {
#pragma unroll
                for (int i = 0; i < 2; ++i) {
                    const int rl = wm * 64 + i * 32 + lr, row = m0 + rl;
                    if (row < a.T) ((int *)a.pm)[(int64_t)tile * a.T + row] = xc[rl] + xc[BM + rl];
                }
            }
        }
    }
}

// one wave per row: fold the row's tiles, lane-strided in tile order, then a butterfly
template <int PASS>
__global__ __launch_bounds__(256) void lms_finish_kernel(ScoreArgs a, int tiles) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= a.T) return;
    const int t = a.targets[row];
    const bool valid = t >= 0 && t < a.V;
    if constexpr (PASS == 0) {
        float M = -INFINITY;
        for (int i = lane; i < tiles; i += 64) M = fmaxf(M, a.pm[(int64_t)i * a.T + row]);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) M = fmaxf(M, __shfl_xor(M, o, 64));
        // the fold itself in fp64 (a few thousand terms per row): what an lse carries is then the
        // fp32 sum inside a tile and one rounding of the result; logprob is rounded once, too
        double s = 0.0;
        for (int i = lane; i < tiles; i += 64)
            s += (double)a.ps[(int64_t)i * a.T + row] * exp((double)(a.pm[(int64_t)i * a.T + row] - M));
        s = wave_sum_d(s);
        const double l = (double)M + log(s);
        if (lane == 0) {
            a.lse[row] = (float)l;
            a.logprob[row] = valid ? (float)((double)a.tl[row] - l) : __builtin_nanf("");
            if (!valid) a.tl[row] = __builtin_nanf("");     // pass B then counts nothing on this row
        }
    } else {
        int gt = 0, eq = 0;
        for (int i = lane; i < tiles; i += 64) {
            const int c = ((const int *)a.pm)[(int64_t)i * a.T + row];
            gt += c & 0xffff;
            eq += c >> 16;
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            gt += __shfl_xor(gt, o, 64);
            eq += __shfl_xor(eq, o, 64);
        }
        if (lane == 0) {
            a.n_greater[row] = valid ? gt : -1;
            a.n_equal_lower[row] = valid ? eq : -1;
        }
    }
}

}  // namespace

size_t lm_score_ws_bytes(int T, int V) {
    const size_t tiles = ((size_t)std::max(V, 1) + BN - 1) / BN;
    return (2 * tiles + 1) * (size_t)std::max(T, 1) * sizeof(float);
}

int lm_score(const bf16_t *x, int64_t ldx, const bf16_t *W, const int32_t *targets, int T, int V, int K, float *logprob,
             float *lse, int32_t *n_greater, int32_t *n_equal_lower, void *ws, size_t ws_bytes, hipStream_t s) {
    if (!x || !W || !targets || !logprob || !lse || !n_greater || !n_equal_lower || !ws)
        return fail(-1, "lm_score: null argument");
    if (T < 1 || T > MAX_T) return fail(-1, "lm_score: need 1 <= T <= 8192");
    if (V < 1 || V > MAX_V) return fail(-1, "lm_score: need 1 <= V <= 2^23");
    if (K < BK || K % BK) return fail(-1, "lm_score: need K % 64 == 0");
    if (ldx < K || ldx % 8) return fail(-1, "lm_score: need ldx >= K and ldx % 8 == 0");
    if (ws_bytes < lm_score_ws_bytes(T, V)) return fail(-1, "lm_score: workspace smaller than acehip_lm_score_ws_bytes");
    if ((uintptr_t)x % 16 || (uintptr_t)W % 16 || (uintptr_t)ws % 4)
        return fail(-1, "lm_score: x and W must be 16-byte aligned, the workspace 4-byte aligned");
    const int tiles = (V + BN - 1) / BN, tilesM = (T + BM - 1) / BM;
    ScoreArgs a;
    a.x = x; a.ldx = ldx; a.W = W; a.targets = targets;
    a.T = T; a.V = V; a.K = K;
    a.pm = (float *)ws;
    a.ps = a.pm + (size_t)tiles * T;
    a.tl = a.ps + (size_t)tiles * T;
    a.logprob = logprob; a.lse = lse; a.n_greater = n_greater; a.n_equal_lower = n_equal_lower;
    const dim3 grid((unsigned)tiles, (unsigned)((tilesM + GROUP - 1) / GROUP));
    const unsigned fin = (unsigned)((T + 3) / 4);
    lms_tile_kernel<0><<<grid, 256, 0, s>>>(a);
    lms_finish_kernel<0><<<fin, 256, 0, s>>>(a, tiles);
    lms_tile_kernel<1><<<grid, 256, 0, s>>>(a);
    lms_finish_kernel<1><<<fin, 256, 0, s>>>(a, tiles);
    HIP_TRY(hipGetLastError());
    return 0;
}

}  // namespace acehip

extern "C" {

size_t acehip_lm_score_ws_bytes(int T, int V) { return acehip::lm_score_ws_bytes(T, V); }

int acehip_lm_score_bf16(const void *x, int ldx, const void *W, const int32_t *targets, int T, int V, int K,
                         float *logprob, float *lse, int32_t *n_greater, int32_t *n_equal_lower, void *ws,
                         size_t ws_bytes, void *stream) {
    return acehip::lm_score((const bf16_t *)x, ldx, (const bf16_t *)W, targets, T, V, K, logprob, lse, n_greater,
                            n_equal_lower, ws, ws_bytes, (hipStream_t)stream);
}

}  // extern "C"
