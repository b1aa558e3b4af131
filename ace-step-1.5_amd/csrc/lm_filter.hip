// lm_filter.hip — top-k / top-p logit filters of the 5 Hz LM's token loop
// (LLMHandler._apply_top_k_filter / _apply_top_p_filter, acestep/llm_inference.py:367-385),
// in place on [B][ld] rows of V fp32 or bf16 values, without a sort.
//
// Both filters are one selection.  An entry's key is the order-preserving 32-bit integer image
// of its value (−0 folded onto +0; a bf16 value's key is its 16-bit image, low 16 bits zero).
// Entries whose key is not above −inf's are "dead": never counted, never written.  Every live
// entry carries a weight q: 1 for top-k, round(exp(x − max)·2⁴⁰) — an integer — for top-p.  With
// A(v) = Σ q over live entries of key > v, the cut is the SMALLEST present key v* with
// A(v*) <= T, where T = k − 1 (top-k) or floor(top_p · Σ q) (top-p):
//   * entries above v* are kept, entries below are overwritten with −inf;
//   * top-k keeps every entry equal to v* (all ties, as `logits < kth` does);
//   * top-p keeps, of the c entries equal to v*, the n = min(c, (T − A(v*)) / q(v*) + 1) of
//     lowest index: the entry of tie rank j has A(v*) + j·q(v*) of mass ranked before it and
//     is kept iff that is <= T — "rank i >= 1 kept iff the mass of ranks < i is <= top_p".
// All sums are integer sums, so they do not depend on the order the atomics arrive in: the same
// input gives the same bits on every call.  The fixed-point weights differ from exact
// arithmetic by one exp rounding (~1e-7 relative) and 2⁻⁴¹ per entry; Σ q < 2⁶⁴ for V < 2²³.
//
// v* is found by a radix descent over the key, digits of 11 + 11 + 10 bits (a bf16 key is done
// after the first two).  Per level one kernel, grid (parts, B): a workgroup histograms its
// contiguous segment of the row in LDS — per bin a count and a weight sum, only entries that
// match the digits already fixed — and flushes its non-empty bins to the row's global histogram
// with integer atomics.  The next kernel starts by resolving that level: every workgroup scans
// the 2048 bins from the top (identical inputs, identical result — no hand-off between
// workgroups), part 0 records the state for the kernels after it.  Top-p runs a max pass first;
// the last kernel resolves the last level and rewrites the row.  A partial tie group (n < c)
// takes a second write path: the last level also leaves every part's own counts, a workgroup
// sums those of the parts before it, then each wave walks a quarter of the segment in index
// order, ranking ties by ballot.  The histograms are zeroed by a memset on the
// caller's stream.  Rows are read with scalar element loads (ld is arbitrary, so rows are not
// 16-B aligned); after the first pass they come from L2 / Infinity Cache.
//
// top_k and top_p in one call: the top-k pipeline, then the top-p pipeline over what survived
// (the removed entries are −inf, hence dead: the softmax is over the survivors) — two calls.
#include <algorithm>

#include "kernels.h"
#include "../../include/acehip.h"

namespace acehip {
namespace {

typedef unsigned long long u64;

constexpr int THREADS = 256;
constexpr int NBINS = 2048;
constexpr int MAX_PARTS = 64;
constexpr int MIN_SEG = 4096;                    // entries per workgroup below which a row is not split further
constexpr uint32_t KEY_NEGINF = 0x007fffffu;     // key of −inf: live keys are above it
constexpr float MASS_ONE = 1099511627776.0f;     // 2⁴⁰: the weight of the row's largest entry

// what a level's resolve leaves for the kernels after it
struct State {
    uint32_t prefix;    // the digits fixed so far, in place (lower bits zero)
    uint32_t done;      // 1: nothing to remove (no live entry, or top-k's k-th entry is a dead one)
    uint32_t maxkey;    // top-p: the key of the row maximum
    uint32_t count;     // entries in the selected bin (after the last level: c, the entries equal to v*)
    u64 above;          // A: weight of the entries above the selected bin
    u64 T;
    u64 binq;           // weight of the selected bin
};

struct RowWs {
    uint32_t count[3][NBINS];
    u64 mass[3][NBINS];
    uint32_t pmax[MAX_PARTS];
    State st[4];        // st[d]: what the level-d histogram kernel starts from
};

__device__ __forceinline__ uint32_t key_of(uint32_t bits) {
    bits = bits == 0x80000000u ? 0u : bits;
    return (bits & 0x80000000u) ? ~bits : (bits | 0x80000000u);
}
// a bf16 entry's key is its 16-bit image in the high half (the low half zero for either sign)
template <bool BF>
__device__ __forceinline__ float value_of(uint32_t key) {
    const uint32_t bits = (key & 0x80000000u) ? (key & 0x7fffffffu) : ~key;
    return __builtin_bit_cast(float, BF ? bits & 0xffff0000u : bits);
}
template <bool BF>
__device__ __forceinline__ uint32_t load_key(const void *row, int i) {
    if (BF) return key_of((uint32_t)((const bf16_t *)row)[i] << 16) & 0xffff0000u;
    return key_of(((const uint32_t *)row)[i]);
}
template <bool BF>
__device__ __forceinline__ u64 mass_of(uint32_t key, float maxv) {
    // float → integer conversions saturate and send NaN to 0: out-of-contract rows stay defined
    return (u64)(expf(value_of<BF>(key) - maxv) * MASS_ONE + 0.5f);
}
// f(i, key) for every entry i of [i0, i1), a workgroup's threads striding it together; eight
// loads are issued before the first is used (one load per trip is a latency chain)
template <bool BF, typename F>
__device__ __forceinline__ void for_keys(const void *row, int i0, int i1, F &&f) {
    for (int base = i0 + (int)threadIdx.x; base < i1; base += THREADS * 8) {
        uint32_t k[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int i = base + u * THREADS;
            k[u] = i < i1 ? load_key<BF>(row, i) : 0u;
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int i = base + u * THREADS;
            if (i < i1) f(i, k[u]);
        }
    }
}
__device__ __forceinline__ int level_shift(int d) { return d == 0 ? 21 : d == 1 ? 10 : 0; }
__device__ __forceinline__ int level_digit(uint32_t key, int d) {
    return d == 0 ? (int)(key >> 21) : d == 1 ? (int)((key >> 10) & 0x7ff) : (int)(key & 0x3ff);
}

// Resolve level d of a row from its global histogram: the lowest non-empty bin whose weight
// above, st.above + Σ q(higher bins), is <= T.  Called by all THREADS threads of a workgroup;
// every thread returns the same state.  Thread t owns bins 2047 − 8t … 2040 − 8t, top first.
template <bool TOPP>
__device__ State resolve_level(const RowWs *w, int d, State st, float top_p) {
    __shared__ u64 part[THREADS];
    __shared__ u64 wsum[THREADS / 64];
    __shared__ uint32_t csum[THREADS / 64];
    __shared__ int best;
    __shared__ State out;
    const int tid = threadIdx.x;
    uint32_t c[8];
    u64 q[8];
    u64 tq = 0;
    uint32_t tc = 0;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int b = NBINS - 1 - (8 * tid + j);
        c[j] = w->count[d][b];
        q[j] = TOPP ? w->mass[d][b] : (u64)c[j];
        tq += q[j];
        tc += c[j];
    }
    __syncthreads();     // the shared arrays may still be read from an earlier resolve
    part[tid] = tq;
    if (tid == 0) best = -1;
    __syncthreads();
    if (tid < THREADS / 64) {
        u64 s = 0;
        for (int j = 0; j < 64; ++j) s += part[64 * tid + j];
        wsum[tid] = s;
    }
    // the row's live count, level 0 only (does any entry take part at all)
    uint32_t wc = tc;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) wc += __shfl_xor(wc, o, 64);
    if ((tid & 63) == 0) csum[tid >> 6] = wc;
    __syncthreads();
    u64 total = 0, before = 0;
    uint32_t live = 0;
#pragma unroll
    for (int j = 0; j < THREADS / 64; ++j) {
        total += wsum[j];
        live += csum[j];
        before += j < (tid >> 6) ? wsum[j] : 0;
    }
    for (int j = 64 * (tid >> 6); j < tid; ++j) before += part[j];
    if (d == 0) {
        if (TOPP) st.T = (u64)((double)total * (double)top_p);
        // no live entry; or fewer live entries than k: the k-th largest is a dead one, t = −inf
        if (live == 0 || (!TOPP && (u64)live <= st.T)) {
            st.done = 1;
            return st;
        }
    }
    u64 a = st.above + before;
    int mine = -1;
    u64 mine_a = 0, mine_q = 0;
    uint32_t mine_c = 0;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        if (c[j] != 0 && a <= st.T) {
            mine = 8 * tid + j;          // position from the top: the largest position is the lowest bin
            mine_a = a;
            mine_q = q[j];
            mine_c = c[j];
        }
        a += q[j];
    }
    if (mine >= 0) atomicMax(&best, mine);
    __syncthreads();
    if (best < 0) {      // unreachable with a live entry (the top bin has nothing above it); stay defined
        st.done = 1;
        return st;
    }
    if (mine == best) {
        State o = st;
        o.prefix = st.prefix | ((uint32_t)(NBINS - 1 - mine) << level_shift(d));
        o.above = mine_a;
        o.binq = mine_q;
        o.count = mine_c;
        out = o;
    }
    __syncthreads();
    return out;
}

__device__ __forceinline__ void seg_range(int V, int seg, int &i0, int &i1) {
    i0 = (int)min((int64_t)blockIdx.x * seg, (int64_t)V);
    i1 = (int)min((int64_t)i0 + seg, (int64_t)V);
}

// top-p: the key of the maximum of each part of each row
template <bool BF>
__global__ __launch_bounds__(THREADS) void lmf_max_kernel(const void *__restrict__ logits, int64_t ld, int V, int seg,
                                                          RowWs *__restrict__ ws) {
    __shared__ uint32_t smax;
    const char *row = (const char *)logits + (int64_t)blockIdx.y * ld * (BF ? 2 : 4);
    int i0, i1;
    seg_range(V, seg, i0, i1);
    if (threadIdx.x == 0) smax = 0;
    __syncthreads();
    uint32_t m = 0;
    for_keys<BF>(row, i0, i1, [&](int, uint32_t key) { m = max(m, key); });
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = max(m, (uint32_t)__shfl_xor(m, o, 64));
    if ((threadIdx.x & 63) == 0) atomicMax(&smax, m);
    __syncthreads();
    if (threadIdx.x == 0) ws[blockIdx.y].pmax[blockIdx.x] = smax;
}

// level d: resolve level d − 1 (d >= 1), then histogram the entries that match the prefix
template <bool BF, bool TOPP>
__global__ __launch_bounds__(THREADS) void lmf_hist_kernel(const void *__restrict__ logits, int64_t ld, int V, int seg,
                                                           int parts, int d, int top_k, float top_p,
                                                           RowWs *__restrict__ ws, uint32_t *__restrict__ pc) {
    __shared__ uint32_t hc[NBINS];
    __shared__ u64 hm[TOPP ? NBINS : 1];
    RowWs *w = ws + blockIdx.y;
    const char *row = (const char *)logits + (int64_t)blockIdx.y * ld * (BF ? 2 : 4);
    State st;
    if (d == 0) {
        st.prefix = 0;
        st.done = 0;
        st.count = 0;
        st.above = 0;
        st.binq = 0;
        st.T = TOPP ? 0 : (u64)(top_k - 1);
        uint32_t m = 0;
        if (TOPP)
            for (int p = 0; p < parts; ++p) m = max(m, w->pmax[p]);
        st.maxkey = m;
    } else {
        st = w->st[d - 1];
        if (!st.done) st = resolve_level<TOPP>(w, d - 1, st, top_p);
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) w->st[d] = st;
    if (st.done) return;
    for (int b = threadIdx.x; b < NBINS; b += THREADS) {
        hc[b] = 0;
        if (TOPP) hm[b] = 0;
    }
    __syncthreads();
    int i0, i1;
    seg_range(V, seg, i0, i1);
    const float maxv = value_of<BF>(st.maxkey);
    const int psh = d == 0 ? 31 : level_shift(d - 1);
    const uint32_t pfx = st.prefix >> psh;
    for_keys<BF>(row, i0, i1, [&](int, uint32_t key) {
        if (key <= KEY_NEGINF || (d != 0 && (key >> psh) != pfx)) return;
        const int b = level_digit(key, d);
        atomicAdd(&hc[b], 1u);
        if (TOPP) atomicAdd(&hm[b], mass_of<BF>(key, maxv));
    });
    __syncthreads();
    // top-p, last level: this part's own counts too (all bins: nothing to zero beforehand) — the
    // tie ranks of the rewrite start from the parts before it
    if (pc) pc += ((int64_t)blockIdx.y * MAX_PARTS + blockIdx.x) * NBINS;
    for (int b = threadIdx.x; b < NBINS; b += THREADS) {
        const uint32_t c = hc[b];
        if (pc) pc[b] = c;
        if (c == 0) continue;
        atomicAdd(&w->count[d][b], c);
        if (TOPP) atomicAdd(&w->mass[d][b], hm[b]);
    }
}

// resolve the last level, then overwrite what is below the cut
template <bool BF, bool TOPP>
__global__ __launch_bounds__(THREADS) void lmf_write_kernel(void *__restrict__ logits, int64_t ld, int V, int seg,
                                                            int levels, float top_p, RowWs *__restrict__ ws,
                                                            const uint32_t *__restrict__ pc) {
    __shared__ uint32_t wtot[2][THREADS / 64];
    RowWs *w = ws + blockIdx.y;
    char *row = (char *)logits + (int64_t)blockIdx.y * ld * (BF ? 2 : 4);
    State st = w->st[levels - 1];
    if (st.done) return;
    st = resolve_level<TOPP>(w, levels - 1, st, top_p);
    if (st.done) return;
    const uint32_t vstar = st.prefix, c = st.count;
    uint32_t keep = c;
    if (TOPP) {
        const u64 q1 = st.binq / c;      // every entry of the bin has the same key, hence the same weight
        if (q1 != 0) keep = (uint32_t)min((u64)c, (st.T - st.above) / q1 + 1);
    }
    int i0, i1;
    seg_range(V, seg, i0, i1);
    if (!TOPP || keep >= c) {
        for_keys<BF>(row, i0, i1, [&](int i, uint32_t key) {
            if (key > KEY_NEGINF && key < vstar) {
                if (BF) ((bf16_t *)row)[i] = 0xff80;
                else ((uint32_t *)row)[i] = 0xff800000u;
            }
        });
        return;
    }
    // partial tie group: ranks in index order.  The ties of the parts before this one come from
    // their last-level counts; wave w then owns the w-th quarter of the segment and walks it in
    // 64-entry steps, a tie's rank being the running count plus the lower lanes of the ballot
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t *pcr = pc + (int64_t)blockIdx.y * MAX_PARTS * NBINS + level_digit(vstar, levels - 1);
    uint32_t n = 0;
    for (int p = threadIdx.x; p < (int)blockIdx.x; p += THREADS) n += pcr[(int64_t)p * NBINS];
    const int quarter = ((i1 - i0 + 255) / 256) * 64;
    const int w0 = min(i0 + wave * quarter, i1), w1 = min(w0 + quarter, i1);
    uint32_t mine = 0;
    for (int c0 = w0 + lane; c0 < w1; c0 += 256) {
        uint32_t k[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) k[u] = c0 + 64 * u < w1 ? load_key<BF>(row, c0 + 64 * u) : 0u;      // 0: dead
#pragma unroll
        for (int u = 0; u < 4; ++u) mine += k[u] == vstar;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        n += __shfl_xor(n, o, 64);
        mine += __shfl_xor(mine, o, 64);
    }
    if (lane == 0) {
        wtot[0][wave] = n;
        wtot[1][wave] = mine;
    }
    __syncthreads();
    uint32_t base = 0;
#pragma unroll
    for (int j = 0; j < THREADS / 64; ++j) base += wtot[0][j] + (j < wave ? wtot[1][j] : 0);
    for (int c0 = w0; c0 < w1; c0 += 256) {
        uint32_t k[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) k[u] = c0 + 64 * u + lane < w1 ? load_key<BF>(row, c0 + 64 * u + lane) : 0u;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int i = c0 + 64 * u + lane;
            const bool tie = k[u] == vstar;
            const u64 bal = __ballot(tie);
            const uint32_t rank = base + (uint32_t)__popcll(bal & ((1ull << lane) - 1ull));
            base += (uint32_t)__popcll(bal);
            if (k[u] > KEY_NEGINF && (k[u] < vstar || (tie && rank >= keep))) {
                if (BF) ((bf16_t *)row)[i] = 0xff80;
                else ((uint32_t *)row)[i] = 0xff800000u;
            }
        }
    }
}

template <bool BF, bool TOPP>
int run_filter(void *logits, int64_t ld, int B, int V, int top_k, float top_p, RowWs *ws, hipStream_t s) {
    uint32_t *pc = TOPP ? (uint32_t *)(ws + B) : nullptr;     // [B][MAX_PARTS][NBINS], after the rows' RowWs
    const int parts = std::min(MAX_PARTS, (V + MIN_SEG - 1) / MIN_SEG);
    const int seg = (V + parts - 1) / parts;
    const int levels = BF ? 2 : 3;
    const dim3 grid((unsigned)parts, (unsigned)B);
    HIP_TRY(hipMemsetAsync(ws, 0, sizeof(RowWs) * (size_t)B, s));
    if (TOPP) lmf_max_kernel<BF><<<grid, THREADS, 0, s>>>(logits, ld, V, seg, ws);
    for (int d = 0; d < levels; ++d)
        lmf_hist_kernel<BF, TOPP><<<grid, THREADS, 0, s>>>(logits, ld, V, seg, parts, d, top_k, top_p, ws,
                                                           d == levels - 1 ? pc : nullptr);
    lmf_write_kernel<BF, TOPP><<<grid, THREADS, 0, s>>>(logits, ld, V, seg, levels, top_p, ws, pc);
    HIP_TRY(hipGetLastError());
    return 0;
}

}  // namespace

size_t lm_filter_ws_bytes(int B, int V) {
    (void)V;
    return (sizeof(RowWs) + sizeof(uint32_t) * MAX_PARTS * NBINS) * (size_t)std::max(B, 1);
}

int lm_filter(void *logits, int dtype, int ld, int B, int V, int top_k, float top_p, void *ws, size_t ws_bytes,
              hipStream_t s) {
    if (!logits || !ws) return fail(-1, "lm_filter: null argument");
    if (B < 1 || B > 65535 || V < 1 || V > (1 << 23))
        return fail(-1, "lm_filter: need 1 <= B <= 65535 and 1 <= V <= 2^23");
    if (ld < V) return fail(-1, "lm_filter: ld < V");
    if (dtype != ACEHIP_F32 && dtype != ACEHIP_BF16) return fail(-1, "lm_filter: dtype must be ACEHIP_F32 or ACEHIP_BF16");
    if (ws_bytes < lm_filter_ws_bytes(B, V)) return fail(-1, "lm_filter: workspace smaller than acehip_lm_filter_ws_bytes");
    if ((uintptr_t)ws % 8) return fail(-1, "lm_filter: workspace must be 8-byte aligned");
    const bool bf = dtype == ACEHIP_BF16;
    RowWs *w = (RowWs *)ws;
    if (top_k > 0 && top_k < V) {
        const int rc = bf ? run_filter<true, false>(logits, ld, B, V, top_k, 0.f, w, s)
                          : run_filter<false, false>(logits, ld, B, V, top_k, 0.f, w, s);
        if (rc) return rc;
    }
    if (top_p > 0.f && top_p < 1.f) {
        const int rc = bf ? run_filter<true, true>(logits, ld, B, V, 0, top_p, w, s)
                          : run_filter<false, true>(logits, ld, B, V, 0, top_p, w, s);
        if (rc) return rc;
    }
    return 0;
}

}  // namespace acehip

extern "C" {

size_t acehip_lm_filter_ws_bytes(int B, int V) { return acehip::lm_filter_ws_bytes(B, V); }

int acehip_lm_filter(void *logits, int dtype, int ld, int B, int V, int top_k, float top_p, void *ws, size_t ws_bytes,
                     void *stream) {
    return acehip::lm_filter(logits, dtype, ld, B, V, top_k, top_p, ws, ws_bytes, (hipStream_t)stream);
}

}  // extern "C"
