// gemm.hip — bf16 MFMA GEMM for the DiT projections: C[M,N] = A[M,K]·W[N,K]^T.
//
// Every dense contraction of the DiT (QKV, O, cross Q/O, SwiGLU gate/up and
// down, proj_in, proj_out, condition_embedder, cross K/V) goes through here
// with a fused epilogue (bias / AdaLN-Zero gated residual / plain residual /
// SwiGLU) so the reference's separate elementwise kernels never touch HBM
// (reference base:499-533).
//
// Structure (templated on tile BM×BN, waves WM×WN, LDS ring depth STAGES):
//   * both operands are K-contiguous ([rows][K]); each K-tile of 64 is staged
//     global→LDS by global_load_lds_dwordx4 into an STAGES-deep ring, the
//     [A tile; W tile] image lane-linear with the XOR swizzle applied on the
//     SOURCE address (chunk' = chunk ^ ((row>>1)&7)) so the ds_read_b128
//     fragment reads are bank-conflict free;
//   * STAGES−1 K-tiles are kept in flight ACROSS the barrier: a counted
//     s_waitcnt vmcnt(N) (never 0 in the steady state) + a raw s_barrier —
//     __syncthreads() would drain the LDS-DMA queue every tile (the ~900 TF
//     ceiling of the 2-barrier structure, cdna_hip_programming.md §5);
//   * v_mfma_f32_16x16x32_bf16 computes the transposed tile (W as the A
//     operand) so each lane owns 4 consecutive output columns of one row
//     (8-byte epilogue stores; the SwiGLU pairs gate/up in registers);
//   * block ids are remapped XCD-aware, then grouped along M so co-resident
//     blocks share the weight panel in L2;
//   * the production tiles are the ping-pong kernels (gemm_pp_kernel, 256×256
//     and 192×256, two wave groups one barrier apart so MFMA and LDS traffic
//     overlap on every SIMD), picked per shape by gemm_pick_variant.
#include <hip/hip_ext.h>

#include <type_traits>

#include "attn_tile.h"
#include "kernels.h"
#include "headpost.h"
#include "pp_addr.h"

namespace acehip {
namespace {

constexpr int BK = 64;
constexpr int GROUP_M = 8;

// GEMM_STAMPS (diagnostic builds only, tools/gemm_stamps.py): per workgroup and wave group,
// shader-clock stamps at kernel entry, after the prologue, after the main loop and after the
// epilogue, plus the real-time clock and the XCC id — where a tile's time goes
#ifdef GEMM_STAMPS
constexpr int STAMP_WG = 16384;
__device__ unsigned long long g_gemm_stamps[STAMP_WG * 2 * 8];
__device__ __forceinline__ void stamp(int slot, int i, unsigned long long v) {
    if (slot < STAMP_WG * 2) {
        asm volatile("" : "+v"(v));
        g_gemm_stamps[slot * 8 + i] = v;
    }
}
// (the ping-pong bodies stamp by tile: slot = the tile's index in the launch's grid, which is
// blockIdx.x except in the persistent kernel, whose workgroups stamp every tile they walk)
#define GSTAMP_AT(slot, i)                                                                       \
    do {                                                                                         \
        if ((threadIdx.x & 255) == 0 && threadIdx.x < 512) stamp((slot) * 2 + (threadIdx.x >> 8), i, __builtin_amdgcn_s_memtime()); \
    } while (0)
#define GSTAMP_REAL_AT(slot, i)                                                                  \
    do {                                                                                         \
        if ((threadIdx.x & 255) == 0 && threadIdx.x < 512) stamp((slot) * 2 + (threadIdx.x >> 8), i, __builtin_amdgcn_s_memrealtime()); \
    } while (0)
#else
#define GSTAMP_AT(slot, i) do {} while (0)
#define GSTAMP_REAL_AT(slot, i) do {} while (0)
#endif
#define GSTAMP(i) GSTAMP_AT(blockIdx.x, i)
#define GSTAMP_REAL(i) GSTAMP_REAL_AT(blockIdx.x, i)

// launch-attached timing events (gemm_ext_events): a hipEventRecord around a launch is its own
// barrier packet — ≈ 5.6 µs of idle GPU before and after the timed kernel on this stack
// (turbo timeline, tools/timeline.py) — while hipExtLaunchKernel stamps the dispatch itself
struct ExtEvents {
    hipEvent_t start = nullptr, stop = nullptr;
};
thread_local ExtEvents g_ext_ev;
template <typename... KArgs, typename... Args>
inline void klaunch(void (*kern)(KArgs...), dim3 grid, dim3 block, hipStream_t s, Args... args) {
    if (g_ext_ev.stop) {
        hipEvent_t st = g_ext_ev.start;
        g_ext_ev.start = nullptr;
        hipExtLaunchKernelGGL(kern, grid, block, 0, s, st, g_ext_ev.stop, 0, args...);
    } else {
        kern<<<grid, block, 0, s>>>(args...);
    }
}

// own LDS-DMAs retired down to N outstanding + own LDS reads retired, then a
// raw barrier (no implicit vmcnt(0)) and a compiler fence so no LDS access
// moves across it
template <int N>
__device__ __forceinline__ void ring_barrier() {
    wait_vm_lgkm0<N>();
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
}

// Epilogue of one wave's SM×SN grid of 16×16 sub-tiles: lane (fr, fc) holds row
// row0 + 16i + fr, columns col0 + 16j + 4fc .. +3 (the transposed MFMA tile).
// Adjacent sub-tiles j, j+1 are paired and the lane pair (fc, fc ^ 1) swaps four
// accumulators (lane ^ 16), so every lane owns 8 CONTIGUOUS columns of one
// sub-tile: one 16-B load / store per operand instead of two 8-B ones (the
// epilogue is store-issue-bound, MI355X_MICROARCH "attention epilogue store
// tail").  SwiGLU: the wave's columns are whole 64-column panels [32 gate | 32 up].
template <int SM, int SN, int EPI, int CHMAX = 12>
__device__ __forceinline__ void epilogue_tile(const GemmArgs &a, const f32x4 (&acc)[SM][SN], int row0, int col0,
                                              int fr, int fc) {
    static_assert(SN % 2 == 0, "sub-tiles are paired");
    const bool odd = fc & 1;
    const int cpos = (fc >> 1) * 8;          // this lane's 8-column group inside its sub-tile
#pragma unroll
    for (int i = 0; i < SM; ++i) {
        const int m = row0 + i * 16 + fr;
        const bool live = m < a.M;           // rows past M still join the lane exchange
        if constexpr (EPI == EPI_SWIGLU) {
#pragma unroll
            for (int pnl = 0; pnl < SN / 4; ++pnl) {
                // silu(gate)·up in the MFMA layout first, then one exchange of the products
                f32x4 p0, p1;
                float o[8];
                // bf16(gate) and bf16(up) of both sub-tiles, pairwise rounded, then silu
                float g8[8], u8[8];
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    g8[r] = acc[i][4 * pnl][r];
                    g8[4 + r] = acc[i][4 * pnl + 1][r];
                    u8[r] = acc[i][4 * pnl + 2][r];
                    u8[4 + r] = acc[i][4 * pnl + 3][r];
                }
                rbf_n<8>(g8);
                rbf_n<8>(u8);
#pragma unroll
                for (int r = 0; r < 8; ++r) g8[r] = silu_f(g8[r]);
                rbf_n<8>(g8);
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    p0[r] = g8[r] * u8[r];
                    p1[r] = g8[4 + r] * u8[4 + r];
                }
                pair8(p0, p1, odd, o);
                const int nout = ((col0 + pnl * 64) >> 1) + (odd ? 16 : 0) + cpos;
                if (live) *(uint4 *)(a.C + (int64_t)m * a.ldc + nout) = pack8(o);
            }
        }
    }
    if constexpr (EPI == EPI_CONV) {
        // vmcnt counts loads and stores together, so a load issued after a store is waited with
        // that store: every per-column operand (bias, Snake a / 1/b) is loaded once, before the
        // first store, and each row group's residual before the previous row group's stores.
        // The chunked form of the other epilogues (below) loaded the Snake parameters after each
        // store — one store latency in front of every 16-B parameter load: k = 1 C = 256 tile
        // epilogue 64.6 k → 41.0 k cycles, k = 7 C = 256 → 10.7 k (profiles/r05aq_conv_stamps_
        // before.log, r05ar_conv_stamps_after.log); 240 s decode 34.87 → 32.84 ms, bit-identical
        // (r05ar_ab_vae.log).  What is left of the k = 1 epilogue is its 256 KB of stores per
        // tile (raw x' and its Snake): staging the residual tile in LDS first measured ±0
        // (r05as_ab_env_vae_reslds.log)
        constexpr int NP = SN / 2;
        uint4 bz[NP];
        float sav[NP][8], sbv[NP][8];
        int colv[NP], phv[NP];
#pragma unroll
        for (int jp = 0; jp < NP; ++jp) {
            const int n = col0 + (2 * jp + (odd ? 1 : 0)) * 16 + cpos;
            phv[jp] = n / a.conv_cout;
            colv[jp] = n - phv[jp] * a.conv_cout;
            bz[jp] = a.bias ? *(const uint4 *)(a.bias + colv[jp]) : make_uint4(0, 0, 0, 0);
            if (a.Cs) {
                const float4 a0 = *(const float4 *)(a.sa + colv[jp]), a1 = *(const float4 *)(a.sa + colv[jp] + 4);
                const float4 b0 = *(const float4 *)(a.sib + colv[jp]), b1 = *(const float4 *)(a.sib + colv[jp] + 4);
                sav[jp][0] = a0.x; sav[jp][1] = a0.y; sav[jp][2] = a0.z; sav[jp][3] = a0.w;
                sav[jp][4] = a1.x; sav[jp][5] = a1.y; sav[jp][6] = a1.z; sav[jp][7] = a1.w;
                sbv[jp][0] = b0.x; sbv[jp][1] = b0.y; sbv[jp][2] = b0.z; sbv[jp][3] = b0.w;
                sbv[jp][4] = b1.x; sbv[jp][5] = b1.y; sbv[jp][6] = b1.z; sbv[jp][7] = b1.w;
            }
        }
        // residual (k = 1 convs of the C ≥ 256 residual units; one phase, so the output row is
        // m; res may be C): row group i + 1's loads issued before row group i's stores
        uint4 gv[2][NP];
        auto load_res = [&](int i, uint4 (&g)[NP]) {
            const int m = min(row0 + i * 16 + fr, a.M - 1);
#pragma unroll
            for (int jp = 0; jp < NP; ++jp)
                g[jp] = *(const uint4 *)(a.res + (int64_t)m * a.ldr + col0 + (2 * jp + (odd ? 1 : 0)) * 16 + cpos);
        };
        if (a.res) load_res(0, gv[0]);
#pragma unroll
        for (int i = 0; i < SM; ++i) {
            if (a.res && i + 1 < SM) load_res(i + 1, gv[(i + 1) & 1]);
            const int m = row0 + i * 16 + fr;
            const bool live = m < a.M;           // rows past M still join the lane exchange
#pragma unroll
            for (int jp = 0; jp < NP; ++jp) {
                float o[8];
                pair8(acc[i][2 * jp], acc[i][2 * jp + 1], odd, o);
                if (a.bias) {
                    float bb[8];
                    unpack8(bz[jp], bb);
                    add_n<8>(o, bb);
                }
                // the conv output rounded to bf16 (raw), then its Snake (conv.hip)
                rbf_n<8>(o);
                if (a.res) {                     // x' = bf16(x + bf16(acc + b))
                    float rr[8];
                    unpack8(gv[i & 1][jp], rr);
                    add_n<8>(o, rr);
                    rbf_n<8>(o);
                }
                const int64_t orow = (int64_t)m * a.conv_ostride + a.conv_ooff + phv[jp];
                const bool ok = live && orow >= 0 && orow < a.conv_lout;
                if (a.C && ok) *(uint4 *)(a.C + orow * a.ldc + colv[jp]) = pack8(o);
                if (a.Cs) {
                    float sn[8];
                    snake_n<8>(o, sav[jp], sbv[jp], sn);
                    if (ok) *(uint4 *)(a.Cs + orow * a.ldc + colv[jp]) = pack8(sn);
                }
            }
        }
    } else if constexpr (EPI != EPI_SWIGLU) {
        // operand loads (residual, gate, bias) of a chunk of CH row groups are all issued
        // before its first store: the stores may alias them (in-place residual: C == res),
        // so the compiler would otherwise wait for every load right after issuing it —
        // one full memory latency per 16-B store, exposed at one wave per SIMD
        constexpr int NP = SN / 2, CH = (CHMAX / NP) < 1 ? 1 : (CHMAX / NP);
#pragma unroll
        for (int c0 = 0; c0 < SM; c0 += CH) {
            uint4 rv[CH][NP], gv[CH][NP];
#pragma unroll
            for (int ii = 0; ii < CH; ++ii) {
                if (c0 + ii >= SM) break;
                const int m = min(row0 + (c0 + ii) * 16 + fr, a.M - 1);
                const int bb_ = (EPI == EPI_GATED_RES) ? m / a.rows_per_batch : 0;
#pragma unroll
                for (int jp = 0; jp < NP; ++jp) {
                    const int n = col0 + (2 * jp + (odd ? 1 : 0)) * 16 + cpos;
                    if constexpr (EPI == EPI_STORE) {
                        if (a.bias) rv[ii][jp] = *(const uint4 *)(a.bias + n);
                    } else {
                        rv[ii][jp] = *(const uint4 *)(a.res + (int64_t)m * a.ldr + n);
                        if constexpr (EPI == EPI_GATED_RES)
                            gv[ii][jp] = *(const uint4 *)(a.gate + (int64_t)bb_ * a.gate_bstride + n);
                    }
                }
            }
#pragma unroll
            for (int ii = 0; ii < CH; ++ii) {
                if (c0 + ii >= SM) break;
                const int i = c0 + ii;
                const int m = row0 + i * 16 + fr;
                const bool live = m < a.M;       // rows past M still join the lane exchange
#pragma unroll
                for (int jp = 0; jp < NP; ++jp) {
                    float o[8];
                    pair8(acc[i][2 * jp], acc[i][2 * jp + 1], odd, o);
                    const int n = col0 + (2 * jp + (odd ? 1 : 0)) * 16 + cpos;
                    if constexpr (EPI == EPI_STORE) {
                        if (a.bias) {
                            float bb[8];
                            unpack8(rv[ii][jp], bb);
#pragma unroll
                            for (int r = 0; r < 8; ++r) o[r] += bb[r];
                        }
                    } else {
                        float rr[8];
                        unpack8(rv[ii][jp], rr);
                        // same roundings as rr + bf16(bf16(o)·g) / rr + bf16(o), pairwise
                        rbf_n<8>(o);
                        if constexpr (EPI == EPI_GATED_RES) {
                            float gg[8];
                            unpack8(gv[ii][jp], gg);
#pragma unroll
                            for (int r = 0; r < 8; ++r) o[r] *= gg[r];
                            rbf_n<8>(o);
                        }
#pragma unroll
                        for (int r = 0; r < 8; ++r) o[r] = rr[r] + o[r];
                    }
                    if (live) *(uint4 *)(a.C + (int64_t)m * a.ldc + n) = pack8(o);
                }
            }
        }
    }
}

// NH > 0: NH helper waves issue every LDS-DMA piece (q ≡ h mod NH) with the same counted
// waits and barriers, so the NW MFMA waves (one per SIMD at NW = 4) carry no DMA in their stream
template <int BM, int BN, int WM, int WN, int STAGES, int EPI, int NH = 0>
__global__ __launch_bounds__(WM *WN * 64 + 64 * NH, 1) void gemm_kernel(GemmArgs a) {
    constexpr int NW = WM * WN;
    constexpr int TM = BM / WM, TN = BN / WN;          // wave tile
    constexpr int SM = TM / 16, SN = TN / 16;          // 16×16 sub-tiles per wave
    constexpr int ROWS = BM + BN;                      // rows of one stage image (128 B each)
    constexpr int STAGE = ROWS * 128;
    constexpr int NINS = ROWS / 8;                     // glds instructions per stage
    constexpr int PER_WAVE = NINS / NW;
    static_assert(NINS % NW == 0, "staging must split evenly over waves");
    static_assert(EPI != EPI_SWIGLU || TN % 64 == 0, "SwiGLU pairs 32+32 columns per 64-column panel");
    __shared__ __attribute__((aligned(16))) char lds[STAGES * STAGE];
    // split-K (EPI_PARTIAL): split blockIdx.y covers K-tiles [y·kper, min(nk, (y+1)·kper))
    const int ktile0 = EPI == EPI_PARTIAL ? (int)blockIdx.y * a.kper : 0;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave / WN, wn = wave % WN;
    const int tilesM = (a.M + BM - 1) / BM, tilesN = a.N / BN;
    const int nwg = tilesM * tilesN;
    const int wg = xcd_remap(blockIdx.x, nwg);
    const int per_group = GROUP_M * tilesN;
    const int gid = wg / per_group, first_m = gid * GROUP_M;
    const int gsz = min(tilesM - first_m, GROUP_M);
    const int tm = first_m + (wg % per_group) % gsz;
    const int tn = (wg % per_group) / gsz;
    const int m0 = tm * BM, n0 = tn * BN;
    const int nk = EPI == EPI_PARTIAL ? min(a.kper, a.K / BK - ktile0) : a.K / BK;

    if constexpr (NH > 0) {
        if (__builtin_amdgcn_readfirstlane(wave) >= NW) {
            constexpr int PPH = NINS / NH;
            static_assert(NINS % NH == 0 && (STAGES - 1) * PPH < 64, "helper pieces / vmcnt field");
            const int h = wave - NW;
            const bf16_t *hs[PPH];
#pragma unroll
            for (int i = 0; i < PPH; ++i) {
                const int q = h + NH * i, r = q * 8 + (lane >> 3);
                const int c = (lane & 7) ^ ((r >> 1) & 7);
                if (r < BM) hs[i] = a.A + (int64_t)min(m0 + r, a.M - 1) * a.lda + c * 8 + ktile0 * BK;
                else hs[i] = a.W + (int64_t)(n0 + r - BM) * a.ldw + c * 8 + ktile0 * BK;
            }
            auto hst = [&](int buf, int k0) {
#pragma unroll
                for (int i = 0; i < PPH; ++i) glds16(hs[i] + k0, lds + buf * STAGE + (h + NH * i) * 1024);
            };
#pragma unroll
            for (int s2 = 0; s2 < STAGES - 1; ++s2)
                if (s2 < nk) hst(s2, s2 * BK);
            for (int kt = 0; kt < nk; ++kt) {
                if (kt + STAGES - 2 < nk) ring_barrier<(STAGES - 2) * PPH>();
                else ring_barrier<0>();
                if (kt + STAGES - 1 < nk) hst((kt + STAGES - 1) % STAGES, (kt + STAGES - 1) * BK);
            }
            wait_vm<0>();
            return;
        }
    }

    // staging sources: wave issues image rows [8q, 8q+8) for q = wave + NW·i
    const bf16_t *src[PER_WAVE];
#pragma unroll
    for (int i = 0; i < PER_WAVE; ++i) {
        const int q = wave + NW * i;
        const int r = q * 8 + (lane >> 3);
        const int c = (lane & 7) ^ ((r >> 1) & 7);
        if (r < BM) src[i] = a.A + (int64_t)min(m0 + r, a.M - 1) * a.lda + c * 8 + ktile0 * BK;
        else src[i] = a.W + (int64_t)(n0 + r - BM) * a.ldw + c * 8 + ktile0 * BK;
    }
    auto stage = [&](int buf, int k0) {
        char *b = lds + buf * STAGE;
#pragma unroll
        for (int i = 0; i < PER_WAVE; ++i) glds16(src[i] + k0, b + (wave + NW * i) * 1024);
    };

    f32x4 acc[SM][SN];
#pragma unroll
    for (int i = 0; i < SM; ++i)
#pragma unroll
        for (int j = 0; j < SN; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

    if constexpr (NH == 0) {
#pragma unroll
        for (int s = 0; s < STAGES - 1; ++s)
            if (s < nk) stage(s, s * BK);
    }
    const int fr = lane & 15, fc = lane >> 4;
    for (int kt = 0; kt < nk; ++kt) {
        // tile kt landed (its own wave's DMAs), leaving STAGES-2 newer tiles in flight
        // every wave's DMA for tile kt landed; tile kt-1 fully read (WAR for the refill below)
        if constexpr (NH > 0) {
            ring_barrier<0>();   // own reads retired (no DMA of its own); the helpers waited
        } else {
            if (kt + STAGES - 2 < nk) ring_barrier<(STAGES - 2) * PER_WAVE>();
            else ring_barrier<0>();
            if (kt + STAGES - 1 < nk) stage((kt + STAGES - 1) % STAGES, (kt + STAGES - 1) * BK);
        }
        const char *b = lds + (kt % STAGES) * STAGE;
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            bf16x8 xf[SM], wf[SN];
#pragma unroll
            for (int i = 0; i < SM; ++i) xf[i] = *(const bf16x8 *)(b + swz(wm * TM + i * 16 + fr, ks * 4 + fc));
#pragma unroll
            for (int j = 0; j < SN; ++j) wf[j] = *(const bf16x8 *)(b + swz(BM + wn * TN + j * 16 + fr, ks * 4 + fc));
#pragma unroll
            for (int i = 0; i < SM; ++i)
#pragma unroll
                for (int j = 0; j < SN; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[j], xf[i], acc[i][j], 0, 0, 0);
        }
    }

    if constexpr (EPI == EPI_PARTIAL) {
        // fp32 partial sums of this split: lane's 4 consecutive columns → one 16-B store
        float *ws = (float *)a.ws + (size_t)blockIdx.y * a.M * a.N;
#pragma unroll
        for (int i = 0; i < SM; ++i) {
            const int m = m0 + wm * TM + i * 16 + fr;
            if (m >= a.M) continue;
#pragma unroll
            for (int j = 0; j < SN; ++j)
                *(f32x4 *)(ws + (int64_t)m * a.N + n0 + wn * TN + j * 16 + fc * 4) = acc[i][j];
        }
        return;
    } else {
        epilogue_tile<SM, SN, EPI>(a, acc, m0 + wm * TM, n0 + wn * TN, fr, fc);
    }
}

// Split-K reduction + the GEMM's epilogue (same rounding as epilogue_tile): the
// splits are summed in order (deterministic); one thread per 4 output columns.
// SwiGLU: packed columns p·64 + [0, 32) gate, p·64 + [32, 64) up → output p·32 + i.
__global__ __launch_bounds__(256) void splitk_epilogue_kernel(GemmArgs a, int splits, bf16_t *out, int64_t ldo) {
    const int nout = a.epi == EPI_SWIGLU ? a.N / 2 : a.N;
    const int64_t e = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * 4;
    if (e >= (int64_t)a.M * nout) return;
    const int m = (int)(e / nout), q = (int)(e % nout);
    const float *ws = (const float *)a.ws;
    const size_t plane = (size_t)a.M * a.N;
    auto sum4 = [&](int col) {
        f32x4 t = *(const f32x4 *)(ws + (int64_t)m * a.N + col);
        for (int sp = 1; sp < splits; ++sp) t += *(const f32x4 *)(ws + sp * plane + (int64_t)m * a.N + col);
        return t;
    };
    float o[4];
    if (a.epi == EPI_SWIGLU) {
        const int pnl = q / 32, i = q % 32;
        const f32x4 g = sum4(pnl * 64 + i), u = sum4(pnl * 64 + 32 + i);
#pragma unroll
        for (int r = 0; r < 4; ++r) o[r] = rbf(silu_f(rbf(g[r]))) * rbf(u[r]);
    } else {
        const f32x4 acc = sum4(q);
        if (a.epi == EPI_STORE || a.epi == EPI_HEADPOST) {
            float bb[4] = {0.f, 0.f, 0.f, 0.f};
            if (a.bias && a.epi == EPI_STORE) unpack4(*(const uint2 *)(a.bias + q), bb);
#pragma unroll
            for (int r = 0; r < 4; ++r) o[r] = acc[r] + bb[r];
        } else {
            float rr[4];
            unpack4(*(const uint2 *)(a.res + (int64_t)m * a.ldr + q), rr);
            if (a.epi == EPI_GATED_RES) {
                float gg[4];
                unpack4(*(const uint2 *)(a.gate + (int64_t)(m / a.rows_per_batch) * a.gate_bstride + q), gg);
#pragma unroll
                for (int r = 0; r < 4; ++r) o[r] = rr[r] + rbf(rbf(acc[r]) * gg[r]);
            } else {
#pragma unroll
                for (int r = 0; r < 4; ++r) o[r] = rr[r] + rbf(acc[r]);
            }
        }
    }
    *(uint2 *)(out + (int64_t)m * ldo + q) = pack4(o);
}

// Head-post epilogue of a BM×256 QKV tile (two 128-column heads): bf16(acc) → LDS tile
// [BM][PITCH] (the operand ring is dead; store_acc(st, PITCH) writes the wave's
// accumulators), then one 16-lane group per (row, head): RMSNorm + RoPE + head-major
// store.  A lane's units: a fixed head (hh = sub & 1) and rows r = wave·2 + (sub >> 1)
// + 2·NW·it, so (batch, position) advance incrementally (no integer division per unit)
// and every cos/sin row is loaded BEFORE the first store (a load's vmcnt would
// otherwise also wait for the older stores).  When both heads of every tile are of one
// kind (q / k / v boundaries at even heads: the DiT's 16 | 8 | 8) the kind is a scalar, so
// the norm / RoPE choice is a scalar branch; otherwise (tiny test layouts) per lane.
//
// HPT = 1: a BM×128 tile holds one head; the four 16-lane groups of a wave take four rows.
template <int MODE, int ITER, int RPI, int PITCH>
__device__ __forceinline__ void headpost_rows(const GemmArgs &a, const bf16_t *st, int m0, int r0, int hh, int li,
                                              int d, int b0, int s0, bf16_t *base, int64_t bstride, bool norm,
                                              const float (&w)[8], const uint4 (&cv)[ITER], const uint4 (&sv)[ITER]) {
    // MODE: 0 v heads (scatter), 1 q/k without RoPE, 2 q/k with RoPE, 3 per-lane `norm`
    const HeadPostArgs &h = a.hp;
    int bq = b0, sq = s0;
#pragma unroll
    for (int it = 0; it < ITER; ++it) {
        const int r = r0 + RPI * it;
        float x[8], cs[8] = {}, sn[8] = {};
        unpack8(*(const uint4 *)(st + r * PITCH + hh * 128 + d), x);
        if constexpr (MODE >= 2) {
            unpack8(cv[it], cs);
            unpack8(sv[it], sn);
        }
        if constexpr (MODE == 1) head_norm_rope_t<true, false>(x, li, w, cs, sn, h.eps);
        else if constexpr (MODE == 2) head_norm_rope_t<true, true>(x, li, w, cs, sn, h.eps);
        else if constexpr (MODE == 3) head_norm_rope(x, li, norm, w, h.cos != nullptr, cs, sn, h.eps);
        if (m0 + r < a.M) *(uint4 *)(base + (int64_t)bq * bstride + sq * 128) = pack8(x);
        sq += RPI;
        while (sq >= h.S) { sq -= h.S; ++bq; }
    }
}

template <int BM, int NW, int LDS_BYTES, int HPT, typename StoreAcc>
__device__ __forceinline__ void headpost_epilogue(const GemmArgs &a, char *lds, int m0, int n0, int wave, int lane,
                                                  StoreAcc store_acc) {
    static_assert(HPT == 1 || HPT == 2, "one or two heads per tile");
    constexpr int PITCH = 128 * HPT + 8;   // 16-B aligned rows, 2-way conflicts on the 8-B writes
    constexpr int RPW = 4 / HPT;           // rows per wave per iteration
    constexpr int RPI = RPW * NW;          // rows per iteration
    constexpr int ITER = BM / RPI;
    static_assert(BM % RPI == 0, "rows must split evenly over the iterations");
    static_assert(BM * PITCH * 2 <= LDS_BYTES, "head-post staging tile must fit the operand ring");
    const HeadPostArgs &h = a.hp;
    const int sub = lane >> 4, li = lane & 15, d = li * 8, hh = HPT == 2 ? sub & 1 : 0;
    const int head = (n0 >> 7) + hh;
    const int nqk = h.nq + h.nk;
    const bool norm = head < nqk;
    const bool rope = h.cos != nullptr;
    const int r0 = wave * RPW + (HPT == 2 ? sub >> 1 : sub);
    const int mf = min(m0 + r0, a.M - 1) + h.m_off;
    const int b0 = mf / h.S, s0 = mf - b0 * h.S;
    uint4 cv[ITER], sv[ITER];
    if (rope) {
        int sq = s0;
#pragma unroll
        for (int it = 0; it < ITER; ++it) {
            const int sc = min(sq, h.S - 1);
            cv[it] = *(const uint4 *)(h.cos + (int64_t)sc * 128 + d);
            sv[it] = *(const uint4 *)(h.sin + (int64_t)sc * 128 + d);
            sq += RPI;
            while (sq >= h.S) sq -= h.S;
        }
    }
    // destination of this lane's head at (b = 0, s = 0) + its 8 columns, and the batch stride
    bf16_t *base;
    int64_t bstride;
    const int64_t hs = (int64_t)h.S_dst * 128;
    if (head < h.nq) {
        const int64_t hq = h.S_dst_q ? (int64_t)h.S_dst_q * 128 : hs;
        base = h.q + head * hq;
        bstride = h.nq * hq;
    } else if (head < nqk) {
        base = h.k + (head - h.nq) * hs;
        bstride = h.nk * hs;
    } else {
        base = h.v + (head - nqk) * hs;
        bstride = h.nv * hs;
    }
    base += d;
    float w[8] = {};
    if (norm) unpack8(*(const uint4 *)((head < h.nq ? h.qw : h.kw) + d), w);
    bf16_t *st = (bf16_t *)lds;
    __syncthreads();
    store_acc(st, PITCH);
    __syncthreads();
    const bool uniform = HPT == 1 || (h.nq % 2 == 0 && nqk % 2 == 0);
    if (uniform) {
        if ((n0 >> 7) >= nqk)
            headpost_rows<0, ITER, RPI, PITCH>(a, st, m0, r0, hh, li, d, b0, s0, base, bstride, norm, w, cv, sv);
        else if (!rope)
            headpost_rows<1, ITER, RPI, PITCH>(a, st, m0, r0, hh, li, d, b0, s0, base, bstride, norm, w, cv, sv);
        else
            headpost_rows<2, ITER, RPI, PITCH>(a, st, m0, r0, hh, li, d, b0, s0, base, bstride, norm, w, cv, sv);
    } else {
        headpost_rows<3, ITER, RPI, PITCH>(a, st, m0, r0, hh, li, d, b0, s0, base, bstride, norm, w, cv, sv);
    }
}

// the attention half's arguments of the fused cross-Q projection + cross-attention kernel
struct XAttnArgs {
    const bf16_t *k, *v;   // [B][KV][Sk][128]
    bf16_t *o;             // token-major [B·S][o_ld], head h at column h·128
    int KV, Sk;
    float sl2;             // scale · log2(e)
    int64_t o_ld;
};

// Epilogue of the fused cross-Q projection + cross-attention tile (w4_body XATT): BM = 192 rows
// × one q head, six waves.  The operand ring is dead after the K loop; LDS becomes
//   [0, QIMG)               the bf16 Q tile [192][PITCH] — the head-post staging tile, transformed
//                           in place (q RMSNorm, no RoPE: headpost_rows' MODE 1 arithmetic)
//   [QIMG, QIMG + 4 tiles)  the attention's K/V ring, K slots 0, 1 then V slots 0, 1 (attn_tile.h)
// Wave w owns rows [32w, 32w + 32) from the transform on: it normalises them, reads them back as
// its Q fragments and runs attn_fwd_kernel's per-wave tile body over KV tiles 0 … ⌈Sk / 64⌉ − 1,
// so nothing but the two block barriers around store_acc orders the waves before the tile loop.
// The transform's LDS accesses are inline asm (explicit lgkmcnt waits): the first K/V tile's
// LDS-DMA is already in flight, and the compiler would drain it (vmcnt(0)) before any LDS access
// of its own.  Per KV tile: one barrier, every wave — rows past M included — reaches it.
// The tile lies inside one batch element (the dispatch guarantees it), rows ≥ M are not stored.
template <int BM, int LDS_BYTES, typename StoreAcc>
__device__ __forceinline__ void xattn_epilogue(const GemmArgs &a, const XAttnArgs &xa, char *lds, int m0, int n0,
                                               int wave, int lane, bool mfma_wave, StoreAcc store_acc) {
    constexpr int PITCH = 136;                       // 16-B aligned rows (headpost_epilogue's pitch)
    constexpr int QIMG = BM * PITCH * 2;             // bytes of the Q tile
    constexpr int NBUF = 2;
    static_assert(BM == 6 * 32, "six waves × 32 query rows");
    static_assert(QIMG % 1024 == 0 && QIMG + 2 * NBUF * KV_TILE <= LDS_BYTES, "Q tile + K/V ring must fit the operand ring");
    const HeadPostArgs &h = a.hp;
    const int wv = __builtin_amdgcn_readfirstlane(wave);
    const int r = lane & 31, hh = lane >> 5;
    const int sub = lane >> 4, li = lane & 15, d = li * 8;
    const int head = n0 >> 7, kvh = head / (h.nq / xa.KV), b = m0 / h.S;
    const int Sk = xa.Sk;
    const float sl2 = xa.sl2;
    const bf16_t *kp = xa.k + ((int64_t)b * xa.KV + kvh) * (int64_t)Sk * 128;
    const bf16_t *vp = xa.v + ((int64_t)b * xa.KV + kvh) * (int64_t)Sk * 128;
    const int ntiles = (Sk + KT - 1) / KT;
    float w[8];
    unpack8(*(const uint4 *)(h.qw + d), w);
    char *const ring = lds + QIMG;

    __syncthreads();                                 // every wave is past the operand ring
    if (mfma_wave) store_acc((bf16_t *)lds, PITCH);
    __syncthreads();
    asm volatile("" ::: "memory");

    // LDS-DMA staging of one K/V tile, attn_fwd_kernel's image (32 one-KiB pieces; waves 0 and 1
    // issue six, the others five): piece c covers image rows 4c..4c+3 of K (c < 16) or V, lane L
    // fetches the logical chunk that kvoff() places in the 16-B slot (row 4c + L/16, chunk L%16).
    // Rows past Sk are clamped to a real row: those keys are masked (K) or meet P = 0 (V).
    auto stage_piece = [&](int kv0, int buf, int c) {
        const int isv = c >> 4, row = (c & 15) * 4 + (lane >> 4), pc = lane & 15;
        const int ch = pc ^ (((row & 3) << 2) | ((row >> 2) & 3));
        const int key = min(kv0 + row, Sk - 1);
        glds16((isv ? vp : kp) + (int64_t)key * 128 + ch * 8, ring + (isv * NBUF + buf) * KV_TILE + (c & 15) * 1024);
    };
    auto stage_tile = [&](int kv0, int buf) {
#pragma unroll
        for (int i = 0; i < 5; ++i) stage_piece(kv0, buf, wv + 6 * i);   // pieces 0 .. 29
        if (wv < 2) stage_piece(kv0, buf, 30 + wv);
    };
    stage_tile(0, 0);

    // q RMSNorm of the wave's 32 rows, four rows (one per 16-lane group) per step, in place
    {
        const float none[8] = {};
        bf16x8 raw[8];
#pragma unroll
        for (int it = 0; it < 8; ++it) raw[it] = ds_read_b128(lds + ((wv * 32 + it * 4 + sub) * PITCH + d) * 2);
        lgkm_wait8(raw);
#pragma unroll
        for (int it = 0; it < 8; ++it) {
            float x[8];
            unpack8(__builtin_bit_cast(uint4, raw[it]), x);
            head_norm_rope_t<true, false>(x, li, w, none, none, h.eps);
            const uint4 pk = pack8(x);
            const u32x4 out = {pk.x, pk.y, pk.z, pk.w};
            const uint32_t dst = lds_addr(lds + ((wv * 32 + it * 4 + sub) * PITCH + d) * 2);
            asm volatile("ds_write_b128 %0, %1" ::"v"(dst), "v"(out) : "memory");
        }
    }
    // Q fragments (B operand of Sᵀ = K·Qᵀ): lane (r, hh) holds Q[32w + r][16s + 8hh .. +8]; the
    // reads follow the wave's own writes in its LDS queue
    bf16x8 qf[8];
#pragma unroll
    for (int s = 0; s < 8; ++s) qf[s] = ds_read_b128(lds + ((wv * 32 + r) * PITCH + 16 * s + 8 * hh) * 2);
    lgkm_wait8(qf);

    float m = NEG, l = 0.f;
    f32x16 oacc[4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 16; ++j) oacc[i][j] = 0.f;
    const uint32_t ring_base = lds_addr(ring);
    uint32_t koff[8], voff[4][2];
    attn_lane_offsets(ring_base, ring_base + NBUF * KV_TILE, lane, koff, voff);

    // end-of-tile wait (counted: the one tile in flight) + the tile's one barrier, as in
    // attn_fwd_kernel: own DMAs of the next tile landed, own LDS reads retired
    auto tile_barrier = [&] {
        wait_vm_lgkm0<0>();
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
    };
    auto tile = [&](int it, auto SLOTC) {
        constexpr int SLOT = decltype(SLOTC)::value;
        constexpr int KB = SLOT * KV_TILE, VB = SLOT * KV_TILE;
        const int kv0 = it * KT;
        // refill: tile it+1 into the slot of tile it−1, read by nobody now
        if (it + 1 < ntiles) stage_tile(kv0 + KT, (SLOT + 1) % NBUF);
        attn_wave_tile<KB, VB>(qf, koff, voff, oacc, m, l, sl2, kv0 + KT <= Sk, [&](int t, int j, float sc) {
            const int kj = kv0 + 32 * t + (j & 3) + 8 * (j >> 2) + 4 * hh;
            return kj < Sk ? sc : NEG;
        });
        tile_barrier();
    };
    tile_barrier();
    int it = 0;
    for (; it + 1 < ntiles; it += 2) {
        tile(it, IC<0>{});
        tile(it + 1, IC<1>{});
    }
    if (it < ntiles) tile(it, IC<0>{});

    const int row = m0 + wv * 32 + r;                // token b·S + s: AO is token-major
    if (row < a.M)                                   // both lanes of a row pair (lane, lane ^ 32) agree
        attn_wave_store_o(oacc, l, xa.o + (int64_t)row * xa.o_ld + head * 128, hh);
}

// ---------------------------------------------------------------------------
// Ping-pong variant: BM×256 tile, 8 waves as 2 groups (wr = 0/1, A rows
// [wr·BM/2, +BM/2)) × 4 (64 columns each).  The groups run one barrier apart,
// so on every SIMD one wave issues MFMAs while the other issues LDS reads and
// LDS-DMA (s_setprio(1) on the MFMA side).  Per K-tile, two phases of
// [ds_read · (stage) · barrier · MFMA over both 32-deep k-steps · barrier]:
//   phase 0  read the four B sub-tiles + A-half 0     stage A(kt+1) → other buffer
//   phase 1  read A-half 1                             stage B(kt+2) → this buffer's B slots,
//                                                       then vmcnt(#B glds): A(kt+1) landed
// (24 / 32 MFMAs per interval at 192 / 256 rows; reads retire before each barrier).
// WAR: A(kt+1) overwrites tile kt−1's A, last read by group 1's phase 1 of kt−1, retired
// before this phase's opening barrier; B(kt+2) overwrites tile kt's B, last read by group 1's
// phase 0, retired before the barrier that opens phase 1.  RAW: each wave's vmcnt precedes
// the barrier that opens the first read of the tile.  Two LDS tile buffers.
// Round 4 replaced a four-phase schedule (12 / 16 MFMAs per interval, 8
// barriers per K-tile; stamps: the 192-row loop 62 % MFMA-busy, now 80 %): DESIGN.md.
// The body of one ping-pong tile; `bid` = the block's index in this GEMM's grid (the fused
// main + tail launch below runs two GEMMs' grids in one) and `lds` = the kernel's 2·BUF bytes
template <int BM>
constexpr int pp_lds_bytes() { return 2 * (BM + 256) * 128; }
//
// The body is three pieces — pp_tile_origin + a source-address set (where tile `bid` lies and
// where its operands come from), pp_main (accumulators, prologue, K loop) and pp_epilogue —
// which the one-tile-per-workgroup kernels call once in that order and the persistent kernel
// (gemm_pp_persist_kernel) calls per tile, with the next tile's prologue issued in between.
template <int BM>
__device__ __forceinline__ void pp_tile_origin(const GemmArgs &a, int bid, int slot, int &m0, int &n0) {
    constexpr int BN = 256;
    const int tilesM = (a.M + BM - 1) / BM, tilesN = a.N / BN;
    const int nwg = tilesM * tilesN;
    const int wg = xcd_remap(bid, nwg);
    const int per_group = GROUP_M * tilesN;
    const int gid = wg / per_group, first_m = gid * GROUP_M;
    const int gsz = min(tilesM - first_m, GROUP_M);
    const int tm = first_m + (wg % per_group) % gsz;
    const int tn = (wg % per_group) / gsz;
    m0 = tm * BM;
    n0 = tn * BN;
#ifdef GEMM_STAMPS
    {
        unsigned xcc;
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
        if ((threadIdx.x & 255) == 0) {
            stamp(slot * 2 + (threadIdx.x >> 8), 6, ((unsigned long long)wg << 32) | xcc);
            stamp(slot * 2 + (threadIdx.x >> 8), 7, blockIdx.x);   // the workgroup that ran the tile
        }
    }
#endif
}

// Source addresses of a wave's LDS-DMA pieces, one 64-bit pointer per piece and lane (the tile
// a one-tile workgroup keeps for its whole life).  The integer arithmetic of both sets is
// pp_addr.h's, which host code can call (acehip_diag_pp_src_check)
template <int BM>
struct PPSrcPtr {
    static constexpr int NA = BM / 64, NB = 4;               // glds per wave for A / B of one K-tile
    static constexpr bool SCALAR = false;
    const bf16_t *pa[NA], *pb[NB];
    __device__ __forceinline__ void set(const GemmArgs &a, int m0, int n0, int wave, int lane) {
#pragma unroll
        for (int i = 0; i < NA; ++i) pa[i] = a.A + pp_ptr_a(a.M, a.lda, m0, wave, lane, i);
#pragma unroll
        for (int i = 0; i < NB; ++i) pb[i] = a.W + pp_ptr_b(BM, a.ldw, n0, wave, lane, i);
    }
    // piece i of the K-tile at element offset k0 → the wave's 1 KiB LDS slot
    __device__ __forceinline__ void dmaA(int i, int k0, char *dst) const { glds16(pa[i] + k0, dst); }
    __device__ __forceinline__ void dmaB(int i, int k0, char *dst) const { glds16(pb[i] + k0, dst); }
};

// The same addresses as a wave-uniform tile base (scalar registers: the tile origin is the
// same for every lane) + 32-bit per-lane byte offsets.  A tile walk derives the next tile's set
// from scalars after the K loop instead of holding a second set of 64-bit pointers across it.
// The offsets do not depend on the tile — the swizzle chunk (lane & 7) ^ ((r >> 1) & 7) is the
// same for rows 64 apart — but for the A rows clamped to M − 1, a no-op except on the last row tile.
template <int BM>
struct PPSrcOff {
    static constexpr int NA = BM / 64, NB = 4;
    static constexpr bool SCALAR = true;   // the LDS slot address is scalar too: `wave` must be wave-uniform
    static_assert(BM % 16 == 0, "A and W image rows share the swizzle chunk");
    const char *ba, *bb;
    uint32_t oa[NA], ob, bstep;
    __device__ __forceinline__ void set(const GemmArgs &a, int m0, int n0, int wave, int lane) {
        ba = (const char *)(a.A + (int64_t)m0 * a.lda);
        bb = (const char *)(a.W + (int64_t)n0 * a.ldw);
        bstep = pp_off_bstep(a.ldw);
        ob = pp_off_b(a.ldw, wave, lane);
#pragma unroll
        for (int i = 0; i < NA; ++i) oa[i] = pp_off_a(a.M, a.lda, m0, wave, lane, i);
    }
    __device__ __forceinline__ void dmaA(int i, int k0, char *dst) const {
        glds16_s(ba + (int64_t)k0 * 2, oa[i], lds_addr(dst));
    }
    __device__ __forceinline__ void dmaB(int i, int k0, char *dst) const {
        glds16_s(bb + (uint64_t)i * bstep + (int64_t)k0 * 2, ob, lds_addr(dst));
    }
};

template <int BM, int EPI, typename Src>
__device__ __forceinline__ void pp_stageA(const GemmArgs &a, char *lds, const Src &src, int wave, int buf, int k0) {
    constexpr int BUF = (BM + 256) * 128;
    char *b = lds + buf * BUF;
    int ko = k0;
    if constexpr (EPI == EPI_CONV) {
        // implicit-GEMM conv: K-tile k0 = tap·cin + c0 reads the input rows shifted by
        // conv_a0 + tap·dil (zero halo rows around the activation)
        ko = pp_conv_ko(k0, a.conv_cin, a.conv_dil, a.conv_a0);
    }
#pragma unroll
    for (int i = 0; i < Src::NA; ++i) src.dmaA(i, ko, b + (wave + 8 * i) * 1024);
}
template <int BM, typename Src>
__device__ __forceinline__ void pp_stageB(char *lds, const Src &src, int wave, int buf, int k0) {
    constexpr int BUF = (BM + 256) * 128;
    char *b = lds + buf * BUF + BM * 128;
#pragma unroll
    for (int i = 0; i < Src::NB; ++i) src.dmaB(i, k0, b + (wave + 8 * i) * 1024);
}
__device__ __forceinline__ void pp_bar() {
    __builtin_amdgcn_sched_barrier(0);
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_sched_barrier(0);
}
// the prologue's LDS-DMAs: tile 0 complete, B(1) in flight
template <int BM, int EPI, typename Src>
__device__ __forceinline__ void pp_prologue_issue(const GemmArgs &a, char *lds, const Src &src, int wave) {
    pp_stageB<BM>(lds, src, wave, 0, 0);
    pp_stageA<BM, EPI>(a, lds, src, wave, 0, 0);
    if (a.K > BK) pp_stageB<BM>(lds, src, wave, 1, BK);
}

// Stores of one wave in the SwiGLU epilogue of a full 256-row tile (one 16-B store per 16-row
// group): what a persistent workgroup has in flight BEHIND the next tile's prologue DMAs
constexpr int PP_SWIGLU_STORES = 256 / 2 / 16;

// Accumulators, prologue and K loop of one tile.  `pend` (PERSIST only): −1 the prologue is
// issued here, as in a one-tile workgroup; otherwise it was issued before the previous tile's
// epilogue — 1: followed by exactly PP_SWIGLU_STORES stores per wave (vmcnt counts loads and
// stores together, in order, so the counted wait leaves them and B(1) in flight), 0: by an
// unknown number of stores (a ragged tile skips some), all waited for.
//
// SLOTIMM (ACEHIP_GEMM_SLOTIMM, scalar-base form only): the K loop is unrolled by the two ring
// slots and peeled, so the read phase — which has to fit under the other wave group's MFMA
// interval — holds no address arithmetic and no data-independent branch.  Every ds_read_b128 is
// one of eight per-lane bases (operand × k-step × slot, formed before the loop; pp_addr.h
// pp_rd_base) + the immediate 2048·sub-tile, the DMA destinations are the wave's scalar slot + a
// constant, and A(kt+1) / B(kt+2) are staged unconditionally in the steady state of K-tile
// pairs, which runs while more than three K-tiles are left; the last one to three run as
// slot-constant bodies that keep the two stage predicates (fully constant tail bodies in an
// if / else chain made the compiler copy the accumulators at the joins: scratch).  The same
// reads, DMAs, waits, barriers and MFMAs in the same order as the loop below it, so the same
// bits.  The asm reads are invisible to the compiler's lgkmcnt bookkeeping: the asm waits
// before each barrier retire them.
template <int BM, int EPI, bool PERSIST, bool SLOTIMM, typename Src>
__device__ __forceinline__ void pp_main(const GemmArgs &a, char *lds, const Src &src, f32x4 (&acc)[BM / 32][4],
                                        int slot, int pend) {
    constexpr int BN = 256, TM = BM / 2, SM = TM / 16, SMH = SM / 2;
    constexpr int ROWS = BM + BN, BUF = ROWS * 128;
    constexpr int NB = BN / 64;
    static_assert(SM % 2 == 0, "A half must be whole 16-row sub-tiles");
    const int tid = threadIdx.x, lane = tid & 63;
    int wave = tid >> 6;
    if constexpr (Src::SCALAR) wave = __builtin_amdgcn_readfirstlane(wave);   // scalar LDS slot addresses (glds16_s)
    const int wr = wave >> 2, wc = wave & 3;
    auto stageA = [&](int buf, int k0) { pp_stageA<BM, EPI>(a, lds, src, wave, buf, k0); };
    auto stageB = [&](int buf, int k0) { pp_stageB<BM>(lds, src, wave, buf, k0); };
    auto bar = [] { pp_bar(); };

#pragma unroll
    for (int i = 0; i < SM; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

    const int fr = lane & 15, fc = lane >> 4;
    const int arow = wr * TM, brow = BM + wc * 64;

    const int nk = a.K / BK;
    if constexpr (!PERSIST) {
        // prologue: tile 0 complete, B(1) in flight
        stageB(0, 0);
        stageA(0, 0);
        if (nk > 1) {
            stageB(1, BK);
            wait_vm<NB>();
        } else {
            wait_vm<0>();
        }
    } else {
        if (pend < 0) pp_prologue_issue<BM, EPI>(a, lds, src, wave);
        __builtin_amdgcn_sched_barrier(0);
        if (pend > 0) {
            if (nk > 1) wait_vm<NB + PP_SWIGLU_STORES>();
            else wait_vm<PP_SWIGLU_STORES>();
        } else {
            if (nk > 1) wait_vm<NB>();
            else wait_vm<0>();
        }
    }
    bar();
    if (wr == 1) bar();   // group 1 runs one barrier behind
    GSTAMP_AT(slot, 1);

    {
    bf16x8 xa[SMH][2], bf[4][2];
    auto readA = [&](const char *b, int h) {
#pragma unroll
        for (int i = 0; i < SMH; ++i)
#pragma unroll
            for (int ks = 0; ks < 2; ++ks)
                xa[i][ks] = *(const bf16x8 *)(b + swz(arow + (h * SMH + i) * 16 + fr, ks * 4 + fc));
    };
    auto mma = [&](int h) {
        __builtin_amdgcn_sched_barrier(0);
        __builtin_amdgcn_s_setprio(1);
#pragma unroll
        for (int ks = 0; ks < 2; ++ks)
#pragma unroll
            for (int i = 0; i < SMH; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    acc[h * SMH + i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bf[j][ks], xa[i][ks], acc[h * SMH + i][j], 0, 0, 0);
        __builtin_amdgcn_s_setprio(0);
    };
    if constexpr (SLOTIMM) {
        static_assert(Src::SCALAR, "the slot-immediate loop issues the scalar-base DMAs");
        uint32_t ra[2][2], rb[2][2];   // [slot][ks]
#pragma unroll
        for (int s = 0; s < 2; ++s)
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
                ra[s][ks] = pp_rd_base(lds_addr(lds), BM, arow, lane, ks, s);
                rb[s][ks] = pp_rd_base(lds_addr(lds), BM, brow, lane, ks, s);
                asm volatile("" : "+v"(ra[s][ks]), "+v"(rb[s][ks]));   // held, not rematerialised in the loop
            }
        // K-tile kt in ring slot S; sa / sb: A(kt+1) / B(kt+2) exist (compile-time true in the
        // steady state, the parent's data-independent branches in the tail)
        auto tile = [&](auto S_, auto STEADY_, int kt) {
            constexpr int S = decltype(S_)::value;
            constexpr bool STEADY = decltype(STEADY_)::value != 0;
            sfor<0, 4>([&](auto j) {
#pragma unroll
                for (int ks = 0; ks < 2; ++ks) bf[j][ks] = ds_read_b128_imm<pp_rd_imm(decltype(j)::value)>(rb[S][ks]);
            });
            sfor<0, SMH>([&](auto i) {
#pragma unroll
                for (int ks = 0; ks < 2; ++ks) xa[i][ks] = ds_read_b128_imm<pp_rd_imm(decltype(i)::value)>(ra[S][ks]);
            });
            if (STEADY || kt + 1 < nk) stageA(S ^ 1, (kt + 1) * BK);
            wait_lgkm0();
            bar();
            mma(0);
            bar();
            sfor<0, SMH>([&](auto i) {
#pragma unroll
                for (int ks = 0; ks < 2; ++ks) xa[i][ks] = ds_read_b128_imm<pp_rd_imm(SMH + decltype(i)::value)>(ra[S][ks]);
            });
            if (STEADY || kt + 2 < nk) {
                stageB(S, (kt + 2) * BK);
                wait_vm_lgkm0<NB>();
            } else {
                wait_vm_lgkm0<0>();
            }
            bar();
            mma(1);
            bar();
        };
        constexpr IC<0> s0{}, tail{};
        constexpr IC<1> s1{}, steady{};
        int kt = 0;
#pragma nounroll
        for (; kt + 3 < nk; kt += 2) {
            tile(s0, steady, kt);
            tile(s1, steady, kt + 1);
        }
        // one to three K-tiles are left (nk ≤ 3: all of them); kt is even
        tile(s0, tail, kt);
        if (kt + 1 < nk) tile(s1, tail, kt + 1);
        if (kt + 2 < nk) tile(s0, tail, kt + 2);
    } else {
        for (int kt = 0; kt < nk; ++kt) {
            const char *b = lds + (kt & 1) * BUF;
            // phase 0: B (all four sub-tiles, both k-steps) + A-half 0; A(kt+1) → other buffer
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int ks = 0; ks < 2; ++ks) bf[j][ks] = *(const bf16x8 *)(b + swz(brow + j * 16 + fr, ks * 4 + fc));
            readA(b, 0);
            if (kt + 1 < nk) stageA((kt + 1) & 1, (kt + 1) * BK);
            wait_lgkm0();
            bar();
            mma(0);
            bar();
            // phase 1: A-half 1; B(kt+2) → this buffer's B slots (tile kt's B: last read by the
            // other group in its phase 0, retired before the barrier above), then A(kt+1) landed
            readA(b, 1);
            if (kt + 2 < nk) {
                stageB(kt & 1, (kt + 2) * BK);
                wait_vm_lgkm0<NB>();
            } else {
                wait_vm_lgkm0<0>();
            }
            bar();
            mma(1);
            bar();
        }
    }
    }
    if (wr == 0) bar();   // balance the barrier count: every wave's LDS reads have retired
    GSTAMP_AT(slot, 2);
}

template <int BM, int EPI>
__device__ __forceinline__ void pp_epilogue(const GemmArgs &a, char *lds, const f32x4 (&acc)[BM / 32][4], int m0, int n0) {
    constexpr int TM = BM / 2, SM = TM / 16, BUF = (BM + 256) * 128;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wr = wave >> 2, wc = wave & 3;
    const int fr = lane & 15, fc = lane >> 4;
    const int arow = wr * TM;
    if constexpr (EPI == EPI_HEADPOST && BM == 256) {
        // the 256-row staging tile (135 KB at the padded pitch) exceeds the operand ring: the two
        // wave groups' 128-row halves go through it one after the other (headpost_epilogue's
        // opening barrier keeps half 1's staging behind half 0's row pass)
#pragma unroll
        for (int hf = 0; hf < 2; ++hf)
            headpost_epilogue<128, 8, 2 * BUF, 2>(a, lds, m0 + hf * 128, n0, wave, lane, [&](bf16_t *st, int pitch) {
                if (wr != hf) return;
#pragma unroll
                for (int i = 0; i < SM; ++i)
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        float o[4] = {acc[i][j][0], acc[i][j][1], acc[i][j][2], acc[i][j][3]};
                        *(uint2 *)(st + (i * 16 + fr) * pitch + wc * 64 + j * 16 + fc * 4) = pack4(o);
                    }
            });
        return;
    } else if constexpr (EPI == EPI_HEADPOST) {
        headpost_epilogue<BM, 8, 2 * BUF, 2>(a, lds, m0, n0, wave, lane, [&](bf16_t *st, int pitch) {
#pragma unroll
            for (int i = 0; i < SM; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    float o[4] = {acc[i][j][0], acc[i][j][1], acc[i][j][2], acc[i][j][3]};
                    *(uint2 *)(st + (arow + i * 16 + fr) * pitch + wc * 64 + j * 16 + fc * 4) = pack4(o);
                }
        });
        return;
    }

    epilogue_tile<SM, 4, EPI>(a, acc, m0 + arow, n0 + wc * 64, fr, fc);
}

// SADDR (ACEHIP_GEMM_SADDR, chosen at launch): the K loop issues its LDS-DMAs from the tile's
// scalar base + 32-bit lane offsets (PPSrcOff) — per piece an s_add_u32 / s_addc_u32 / s_mov m0 —
// instead of a 64-bit pointer per piece and lane (PPSrcPtr: per piece and K-tile a
// v_lshl_add_u64, a v_readfirstlane → m0 chain and a v_add_u32, in the read phase that has to
// fit under the other wave group's MFMA interval).  The same addresses (pp_addr.h), so the same
// bits; the host takes this form only where the 32-bit offsets cannot wrap (pp_saddr_fits).
template <int BM, int EPI, bool SADDR, bool SLOTIMM = false>
__device__ __forceinline__ void gemm_pp_body(const GemmArgs &a, char *lds, int bid) {
    GSTAMP(0);
    GSTAMP_REAL(4);
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = SADDR ? __builtin_amdgcn_readfirstlane(tid >> 6) : tid >> 6;
    int m0, n0;
    pp_tile_origin<BM>(a, bid, blockIdx.x, m0, n0);
    std::conditional_t<SADDR, PPSrcOff<BM>, PPSrcPtr<BM>> src;
    src.set(a, m0, n0, wave, lane);
    f32x4 acc[BM / 32][4];
    pp_main<BM, EPI, false, SLOTIMM>(a, lds, src, acc, blockIdx.x, -1);
    pp_epilogue<BM, EPI>(a, lds, acc, m0, n0);
    if constexpr (EPI == EPI_HEADPOST) return;
#ifdef GEMM_STAMPS
    wait_vm<0>();
#endif
    GSTAMP(3);
    GSTAMP_REAL(5);
}

// Persistent tile walk (SwiGLU gate/up, whose epilogue writes straight from registers and leaves
// the operand ring alone): one workgroup per CU, workgroup w takes tiles w, w + G, w + 2G, … of
// the launch's tile list — the main grid's 256² tiles, then the tail-split tail's 128×256 ones
// (gemm_plan.h plan_tail_split), i.e. the order in which the hardware hands the fused main + tail grid's
// blocks to the CUs, so xcd_remap + GROUP_M keep their per-XCD panel sharing.  At a tile
// boundary the ring is idle (every wave's LDS reads retired before the K loop's closing
// barrier), so the NEXT tile's whole prologue — B(0), A(0), B(1) — is issued before this tile's
// epilogue and lands under it; the next K loop is entered on a counted vmcnt that leaves B(1) and
// the epilogue's stores in flight (pp_main).  A one-tile workgroup instead ends, the next is
// dispatched onto an empty ring, and its prologue waits a full memory latency before the
// first MFMA.  The next tile's addresses are derived from scalars after the K loop (PPSrcOff).
// No workgroup waits for another and nothing is kept between launches.
// The host guarantees ntot − nmain ≤ gridDim.x: a tail tile is its workgroup's last (a tail tile
// followed by another would still be correct — its prologue is simply not issued early).
template <int EPI, bool SLOTIMM>
__global__ __launch_bounds__(512, 1) void gemm_pp_persist_kernel(GemmArgs a, GemmArgs t, int nmain, int ntot) {
    static_assert(EPI == EPI_SWIGLU, "the early prologue needs an epilogue that leaves LDS alone and a known store count");
    __shared__ __attribute__((aligned(16))) char lds[pp_lds_bytes<256>()];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int G = gridDim.x;
    int i = blockIdx.x;
    int pend = -1;   // ≥ 0: tile i's prologue is already in flight (pp_main)
    int m0 = 0, n0 = 0;
    GSTAMP_AT(i, 0);
    GSTAMP_REAL_AT(i, 4);
    PPSrcOff<256> src;
    PPSrcOff<128> tsrc;
    if (i < nmain) {
        pp_tile_origin<256>(a, i, i, m0, n0);
        src.set(a, m0, n0, wave, lane);
    }
    for (; i < nmain; i += G) {
        f32x4 acc[8][4];
        pp_main<256, EPI, true, SLOTIMM>(a, lds, src, acc, i, pend);
        const int cm0 = m0, cn0 = n0, nx = i + G;
        pend = cm0 + 256 <= a.M ? 1 : 0;   // a ragged tile's waves skip stores
        if (nx < ntot) {
            GSTAMP_AT(nx, 0);
            GSTAMP_REAL_AT(nx, 4);
        }
        if (nx < nmain) {
            pp_tile_origin<256>(a, nx, nx, m0, n0);
            src.set(a, m0, n0, wave, lane);
            pp_prologue_issue<256, EPI>(a, lds, src, wave);
        } else if (nx < ntot) {
            pp_tile_origin<128>(t, nx - nmain, nx, m0, n0);
            tsrc.set(t, m0, n0, wave, lane);
            pp_prologue_issue<128, EPI>(t, lds, tsrc, wave);
        }
        __builtin_amdgcn_sched_barrier(0);
        pp_epilogue<256, EPI>(a, lds, acc, cm0, cn0);
        __builtin_amdgcn_sched_barrier(0);
        GSTAMP_AT(i, 3);
        GSTAMP_REAL_AT(i, 5);
    }
    for (; i < ntot; i += G) {
        if (pend < 0) {
            pp_tile_origin<128>(t, i - nmain, i, m0, n0);
            tsrc.set(t, m0, n0, wave, lane);
        }
        f32x4 acc[4][4];
        pp_main<128, EPI, true, SLOTIMM>(t, lds, tsrc, acc, i, pend);
        pend = -1;
        pp_epilogue<128, EPI>(t, lds, acc, m0, n0);
#ifdef GEMM_STAMPS
        wait_vm<0>();
#endif
        GSTAMP_AT(i, 3);
        GSTAMP_REAL_AT(i, 5);
        if (i + G < ntot) {
            GSTAMP_AT(i + G, 0);
            GSTAMP_REAL_AT(i + G, 4);
        }
    }
}

template <int BM, int EPI, bool SADDR, bool SLOTIMM = false>
__global__ __launch_bounds__(512, 1) void gemm_pp_kernel(GemmArgs a) {
    __shared__ __attribute__((aligned(16))) char lds[pp_lds_bytes<BM>()];
    gemm_pp_body<BM, EPI, SADDR, SLOTIMM>(a, lds, blockIdx.x);
}

// The tail-split GEMM (gemm_plan.h plan_tail_split: whole rounds of 256-row tiles + the remaining rows as
// one round of 128-row tiles) in ONE launch: blocks [0, nmain) run the main grid, the rest the
// tail grid, so the tail's blocks start on CUs as the main grid's last round drains instead of
// behind a kernel boundary
template <int EPI, bool SADDR, bool SLOTIMM = false>
__global__ __launch_bounds__(512, 1) void gemm_pp_split_kernel(GemmArgs a, GemmArgs t, int nmain) {
    __shared__ __attribute__((aligned(16))) char lds[pp_lds_bytes<256>()];
    if ((int)blockIdx.x < nmain) gemm_pp_body<256, EPI, SADDR, SLOTIMM>(a, lds, blockIdx.x);
    else gemm_pp_body<128, EPI, SADDR, SLOTIMM>(t, lds, blockIdx.x - nmain);
}

// ---------------------------------------------------------------------------
// Four-wave variant: BM×BN tile, one wave per SIMD (2×2 waves, wave tile
// (BM/2)×(BN/2): at the production 192×128, the half-chip M ≈ 3000 shapes, 24
// accumulators of 16×16 in AGPRs), register double-buffered fragments.  Per K-tile kt (two 32-deep k-steps), ONE barrier in the middle:
//   half A   MFMAs of k-step 0 (fragments F0)  ∥ ds_reads of k-step 1 → F1
//   ──────   own LDS-DMA of tile kt+1 retired (vmcnt(0): nothing newer is in
//            flight yet) + own reads retired, barrier: tile kt+1 is visible and
//            every wave has finished reading tile kt
//   half B   LDS-DMA of tile kt+2 into tile kt's buffer, MFMAs of k-step 1 (F1)
//            ∥ ds_reads of tile kt+1's k-step 0 → F0
// so the MFMA pipe never waits for a fragment read, the DMA of a tile has one whole
// K-tile (≈96 MFMAs) of lead, and two LDS buffers suffice.
// NH > 0: NH extra helper waves issue every LDS-DMA piece (pieces q ≡ h mod NH), so the four
// MFMA waves carry no DMA in their instruction stream (one wave per SIMD pays ≈ 60-185 cycles
// per piece there); a helper waits for tile kt+1 before barrier kt and refills tile kt's buffer
// after it, the same ordering as the MFMA waves' own refills
//
// XATT (the fused cross-attention kernel below; BM = 192, BN = 128, NH = 2, head-post epilogue): the
// tile is the cross-Q projection of 192 rows × one head.  After the K loop the bf16 Q rows stay
// in LDS and all six waves — the helper waves included, 32 rows each — run the cross-attention
// of those rows over the layer's cached K/V (attn_tile.h, attn_fwd_kernel's per-wave body) and
// write AO (xattn_epilogue above).

// ring depth: 3 tile buffers when they fit (a refill's DMA then has two K-tiles of lead,
// enough for HBM-cold weights), else 2 (one K-tile of lead)
template <int BM, int BN>
constexpr int w4_stages() { return 3 * (BM + BN) * 128 <= 160 * 1024 ? 3 : 2; }
template <int BM, int BN>
constexpr int w4_lds_bytes() { return w4_stages<BM, BN>() * (BM + BN) * 128; }

template <int BM, int BN, int EPI, int NH, bool XATT>
__device__ __forceinline__ void w4_body(const GemmArgs &a, char *lds, const XAttnArgs &xa) {
    constexpr int TM = BM / 2, TN = BN / 2, SM = TM / 16, SN = TN / 16;
    constexpr int ROWS = BM + BN, STAGE = ROWS * 128;
    constexpr int NS = w4_stages<BM, BN>();
    constexpr int PW = ROWS / 32;                              // glds per wave per K-tile
    static_assert(ROWS % 32 == 0, "staging must split evenly over 4 waves");
    static_assert(!XATT || (BM == 192 && BN == 128 && NH == 2 && EPI == EPI_HEADPOST), "fused cross-attention tile");

    GSTAMP(0);
    GSTAMP_REAL(4);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    const int tilesM = (a.M + BM - 1) / BM, tilesN = a.N / BN;
    const int nwg = tilesM * tilesN;
    const int wg = xcd_remap(blockIdx.x, nwg);
    const int per_group = GROUP_M * tilesN;
    const int gid = wg / per_group, first_m = gid * GROUP_M;
    const int gsz = min(tilesM - first_m, GROUP_M);
    const int tm = first_m + (wg % per_group) % gsz;
    const int tn = (wg % per_group) / gsz;
    const int m0 = tm * BM, n0 = tn * BN;
    const int nk = a.K / BK;

    bool mfma_wave = true;   // false: a helper wave of the fused kernel, past its DMA loop
    if constexpr (NH > 0) {
        if (__builtin_amdgcn_readfirstlane(wave) >= 4) {
            constexpr int PPH = 4 * PW / NH;                        // pieces per helper per K-tile
            static_assert((4 * PW) % NH == 0 && (NS - 1) * PPH < 64, "helper pieces / vmcnt field");
            const int h = wave - 4;
            const bf16_t *hs[PPH];
#pragma unroll
            for (int i = 0; i < PPH; ++i) {
                const int q = h + NH * i, r = q * 8 + (lane >> 3);
                const int c = (lane & 7) ^ ((r >> 1) & 7);
                if (r < BM) hs[i] = a.A + (int64_t)min(m0 + r, a.M - 1) * a.lda + c * 8;
                else hs[i] = a.W + (int64_t)(n0 + r - BM) * a.ldw + c * 8;
            }
            auto fill = [&](int buf, int k0) {
#pragma unroll
                for (int i = 0; i < PPH; ++i) glds16(hs[i] + k0, lds + buf * STAGE + (h + NH * i) * 1024);
            };
            for (int t = 0; t < NS; ++t) fill(t, min(t, nk - 1) * BK);
            wait_vm<(NS - 1) * PPH>();
            __builtin_amdgcn_s_barrier();
            for (int kt = 0; kt < nk; ++kt) {
                wait_vm<(NS - 2) * PPH>();   // tile kt+1 landed
                __builtin_amdgcn_s_barrier();
                asm volatile("" ::: "memory");
                fill(kt % NS, min(kt + NS, nk - 1) * BK);
            }
            wait_vm<0>();
            if constexpr (XATT) {
                mfma_wave = false;                 // joins the fused epilogue below
            } else {
                if constexpr (EPI == EPI_HEADPOST) {   // the head-post epilogue's two block barriers
                    __syncthreads();
                    __syncthreads();
                }
                return;
            }
        }
    }

    const int fr = lane & 15, fc = lane >> 4;
    f32x4 acc[SM][SN];
    if (mfma_wave) {
    // staging: wave issues image rows [8q, 8q+8) for q = wave + 4i (swizzle on the source)
    const bf16_t *src[PW];
#pragma unroll
    for (int i = 0; i < PW; ++i) {
        const int r = (wave + 4 * i) * 8 + (lane >> 3);
        const int c = (lane & 7) ^ ((r >> 1) & 7);
        if (r < BM) src[i] = a.A + (int64_t)min(m0 + r, a.M - 1) * a.lda + c * 8;
        else src[i] = a.W + (int64_t)(n0 + r - BM) * a.ldw + c * 8;
    }
    auto stage1 = [&](int buf, int k0, int i) { glds16(src[i] + k0, lds + buf * STAGE + (wave + 4 * i) * 1024); };
#pragma unroll
    for (int i = 0; i < SM; ++i)
#pragma unroll
        for (int j = 0; j < SN; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

    const int xrow = wm * TM + fr, wrow = BM + wn * TN + fr;
    bf16x8 x0[SM], w0[SN], x1[SM], w1[SN];
    auto rd = [&](const char *b, int ks, bf16x8 (&xf)[SM], bf16x8 (&wf)[SN]) {
#pragma unroll
        for (int j = 0; j < SN; ++j) wf[j] = *(const bf16x8 *)(b + swz(wrow + j * 16, ks * 4 + fc));
#pragma unroll
        for (int i = 0; i < SM; ++i) xf[i] = *(const bf16x8 *)(b + swz(xrow + i * 16, ks * 4 + fc));
    };
    // MFMA by inline asm with the accumulator tied in place in AGPRs ("+a"): with the
    // builtin, the register allocator of ROCm 7.2 splits dst from srcC at this register
    // pressure (192 accumulators + 112 fragment registers) and rotates the whole
    // accumulator set through v_accvgpr_mov copies every K-tile
    // hook(n) runs after the n-th MFMA (the LDS-DMA pieces of a refill are spread over
    // the MFMA stream this way: volatile asm and the DMA builtin keep their order)
    auto mm = [&](const bf16x8 (&xf)[SM], const bf16x8 (&wf)[SN], auto hook) {
#pragma unroll
        for (int i = 0; i < SM; ++i)
#pragma unroll
            for (int j = 0; j < SN; ++j) {
                // (XATT: in arch VGPRs — the attention half needs nearly all 256 registers of the
                // wave as arch VGPRs, and the AGPR / VGPR boundary is one per kernel)
                if constexpr (XATT)
                    asm volatile("v_mfma_f32_16x16x32_bf16 %0, %1, %2, %0" : "+v"(acc[i][j]) : "v"(wf[j]), "v"(xf[i]));
                else
                    asm volatile("v_mfma_f32_16x16x32_bf16 %0, %1, %2, %0" : "+a"(acc[i][j]) : "v"(wf[j]), "v"(xf[i]));
                hook(i * SN + j);
            }
    };
    auto none = [](int) {};
    // the wait is the builtin (vmcnt((NS−2)·PW) expcnt(7) lgkmcnt(0): tile kt+1 landed,
    // the NS−2 newer refills still in flight), so the compiler's own waitcnt pass knows
    // every read before it has retired and adds none after it
    constexpr int VM = (NS - 2) * PW;
    static_assert(VM < 64, "vmcnt field");
    constexpr int WAIT_ENC = waitcnt_enc(VM, 0);
    auto bar = [] {
        __builtin_amdgcn_s_waitcnt(WAIT_ENC);
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
    };
    // (F0 was read during the previous half B: retire it with a compiler-visible
    // lgkmcnt(0) — vmcnt(63) expcnt(7) — before the next reads are issued, or the
    // compiler waits lgkmcnt(0) for it behind them)
    //
    // ONE straight-line loop body for every K-tile, the last ones included: the refill
    // source is clamped to the last tile (a duplicate load into a buffer nobody reads
    // again) and the last iteration's "next" reads hit a stale buffer (unused).  A
    // second copy of the MFMA code (a peeled tail) makes the register allocator move the
    // accumulators between copies with VALU instructions that the asm MFMAs — opaque
    // to the hazard recognizer — would read without the required wait states.
    // prologue: tiles 0..NS−1 (clamped: duplicates past the last tile keep the count
    // uniform), tile 0 landed
    if constexpr (NH == 0) {
#pragma unroll
        for (int t = 0; t < NS; ++t)
#pragma unroll
            for (int i = 0; i < PW; ++i) stage1(t, min(t, nk - 1) * BK, i);
        wait_vm<(NS - 1) * PW>();
    }
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    GSTAMP(1);
    rd(lds, 0, x0, w0);
    // refill pieces: one after every EVERY-th MFMA of half B, from MFMA FIRST on
    constexpr int EVERY = SM * SN / PW, FIRST = 1;
    static_assert(FIRST + EVERY * (PW - 1) < SM * SN, "refill pieces must fit in half B");
    for (int kt = 0; kt < nk; ++kt) {
        const int cur = kt % NS, nxt = (kt + 1) % NS;
        __builtin_amdgcn_s_waitcnt(waitcnt_enc(63, 0));
        rd(lds + cur * STAGE, 1, x1, w1);
        mm(x0, w0, none);
        bar();
        // refill of this tile's buffer (every wave is past its reads) with tile kt+NS
        const int kr = min(kt + NS, nk - 1) * BK;
        rd(lds + nxt * STAGE, 0, x0, w0);
        if constexpr (NH == 0) {
            mm(x1, w1, [&](int n) {
                if (n >= FIRST && (n - FIRST) % EVERY == 0 && (n - FIRST) / EVERY < PW) stage1(cur, kr, (n - FIRST) / EVERY);
            });
        } else {
            (void)kr;
            mm(x1, w1, none);
        }
    }
    wait_vm<0>();
    // the asm MFMAs are opaque to the hazard recognizer: let the last ones retire
    // before their accumulators are read
    GSTAMP(2);
    asm volatile("s_nop 15\n\ts_nop 15\n\ts_nop 15\n\ts_nop 15" ::: "memory");
    }   // mfma_wave
    // the wave's accumulators as bf16 into the LDS tile st[BM][pitch] (head-post staging)
    auto store_acc = [&](bf16_t *st, int pitch) {
#pragma unroll
        for (int i = 0; i < SM; ++i)
#pragma unroll
            for (int j = 0; j < SN; ++j) {
                float o[4] = {acc[i][j][0], acc[i][j][1], acc[i][j][2], acc[i][j][3]};
                *(uint2 *)(st + (wm * TM + i * 16 + fr) * pitch + wn * TN + j * 16 + fc * 4) = pack4(o);
            }
    };
    (void)store_acc;
    if constexpr (XATT) {
        xattn_epilogue<BM, NS * STAGE>(a, xa, lds, m0, n0, wave, lane, mfma_wave, store_acc);
    } else if constexpr (EPI == EPI_HEADPOST) {
        headpost_epilogue<BM, 4, NS * STAGE, BN / 128>(a, lds, m0, n0, wave, lane, store_acc);
    } else {
        epilogue_tile<SM, SN, EPI>(a, acc, m0 + wm * TM, n0 + wn * TN, fr, fc);
    }
#ifdef GEMM_STAMPS
    wait_vm<0>();
#endif
    GSTAMP(3);
    GSTAMP_REAL(5);
}

template <int BM, int BN, int EPI, int NH = 0>
__global__ __launch_bounds__(256 + 64 * NH, 1) void gemm_w4_kernel(GemmArgs a) {
    __shared__ __attribute__((aligned(16))) char lds[w4_lds_bytes<BM, BN>()];
    w4_body<BM, BN, EPI, NH, false>(a, lds, XAttnArgs{});
}

// The fused cross-Q projection + cross-attention of the DiT's conditional rows: gemm_w4_kernel<192,
// 128, head-post, 2 helpers>'s tile (one 192-row tile × one head per workgroup), whose Q rows go to
// LDS and whose six waves then attend over the cached K/V of that head's KV head (w4_body XATT)
__global__ __launch_bounds__(384, 1) void cross_q_attn_kernel(GemmArgs a, XAttnArgs xa) {
    __shared__ __attribute__((aligned(16))) char lds[w4_lds_bytes<192, 128>()];
    w4_body<192, 128, EPI_HEADPOST, 2, true>(a, lds, xa);
}

template <int BM, int BN = 256, int NH = 0>
int launch_w4(const GemmArgs &a, hipStream_t s) {
    if (a.N % BN) return fail(-1, "gemm: N not a multiple of the 4-wave tile");
    const int tiles = ((a.M + BM - 1) / BM) * (a.N / BN);
    constexpr int NT = 256 + 64 * NH;
    switch (a.epi) {
        case EPI_STORE: gemm_w4_kernel<BM, BN, EPI_STORE, NH><<<tiles, NT, 0, s>>>(a); break;
        case EPI_GATED_RES: gemm_w4_kernel<BM, BN, EPI_GATED_RES, NH><<<tiles, NT, 0, s>>>(a); break;
        case EPI_RES: gemm_w4_kernel<BM, BN, EPI_RES, NH><<<tiles, NT, 0, s>>>(a); break;
        case EPI_SWIGLU: klaunch(gemm_w4_kernel<BM, BN, EPI_SWIGLU, NH>, dim3(tiles), dim3(NT), s, a); break;
        case EPI_HEADPOST:
            if constexpr (BM == 192 && (BN == 256 || BN == 128)) {
                gemm_w4_kernel<BM, BN, EPI_HEADPOST, NH><<<tiles, NT, 0, s>>>(a);
                break;
            }
            return fail(-1, "gemm: the head-post epilogue needs the 192-row tile");
        default: return fail(-1, "gemm: bad epilogue for the 4-wave variant");
    }
    HIP_TRY(hipGetLastError());
    return 0;
}

template <int BM, bool SADDR, bool SLOTIMM = false>
int launch_pp_as(const GemmArgs &a, hipStream_t s) {
    if (a.N % 256) return fail(-1, "gemm: N not a multiple of 256");
    const int tiles = ((a.M + BM - 1) / BM) * (a.N / 256);
    switch (a.epi) {
        case EPI_STORE: gemm_pp_kernel<BM, EPI_STORE, SADDR, SLOTIMM><<<tiles, 512, 0, s>>>(a); break;
        case EPI_GATED_RES: gemm_pp_kernel<BM, EPI_GATED_RES, SADDR, SLOTIMM><<<tiles, 512, 0, s>>>(a); break;
        case EPI_RES: gemm_pp_kernel<BM, EPI_RES, SADDR, SLOTIMM><<<tiles, 512, 0, s>>>(a); break;
        case EPI_SWIGLU: klaunch(gemm_pp_kernel<BM, EPI_SWIGLU, SADDR, SLOTIMM>, dim3(tiles), dim3(512), s, a); break;
        case EPI_CONV:
            if constexpr (BM == 256 || BM == 128) {
                gemm_pp_kernel<BM, EPI_CONV, false><<<tiles, 512, 0, s>>>(a);
                break;
            }
            return fail(-1, "gemm: the conv epilogue runs on the 256- or 128-row ping-pong tile");
        case EPI_HEADPOST:
            if constexpr (BM == 256 || BM == 192 || BM == 128) {
                gemm_pp_kernel<BM, EPI_HEADPOST, SLOTIMM, SLOTIMM><<<tiles, 512, 0, s>>>(a);   // scalar base only with slot immediates
                break;
            }
            return fail(-1, "gemm: head-post epilogue needs the 256-, 192- or 128-row ping-pong tile");
        default: return fail(-1, "gemm: bad epilogue");
    }
    HIP_TRY(hipGetLastError());
    return 0;
}
template <int BM>
int launch_pp(const GemmArgs &a, hipStream_t s) {
    const Knobs &k = knobs();
    if (pp_tile_slotimm(k.gemm_slotimm, k.gemm_saddr, a.epi, BM, a.lda, a.ldw)) return launch_pp_as<BM, true, true>(a, s);
    return pp_tile_saddr(k.gemm_saddr, a.epi, BM, a.lda, a.ldw) ? launch_pp_as<BM, true>(a, s) : launch_pp_as<BM, false>(a, s);
}

template <int BM, int BN, int WM, int WN, int STAGES, int NH = 0>
int launch(const GemmArgs &a, hipStream_t s) {
    if (a.N % BN) return fail(-1, "gemm: N not a multiple of the tile");
    const int tiles = ((a.M + BM - 1) / BM) * (a.N / BN);
    constexpr int NT = WM * WN * 64 + 64 * NH;
    switch (a.epi) {
        case EPI_STORE: gemm_kernel<BM, BN, WM, WN, STAGES, EPI_STORE, NH><<<tiles, NT, 0, s>>>(a); break;
        case EPI_GATED_RES: gemm_kernel<BM, BN, WM, WN, STAGES, EPI_GATED_RES, NH><<<tiles, NT, 0, s>>>(a); break;
        case EPI_RES: gemm_kernel<BM, BN, WM, WN, STAGES, EPI_RES, NH><<<tiles, NT, 0, s>>>(a); break;
        case EPI_SWIGLU: klaunch(gemm_kernel<BM, BN, WM, WN, STAGES, EPI_SWIGLU, NH>, dim3(tiles), dim3(NT), s, a); break;
        default: return fail(-1, "gemm: bad epilogue for this variant");
    }
    HIP_TRY(hipGetLastError());
    return 0;
}

}  // namespace

int gemm_variant(const GemmArgs &a, int variant, hipStream_t s) {
    switch (variant) {
        case 0: return launch<128, 128, 2, 2, 2>(a, s);   // 4 waves, 2-stage (2 blocks/CU): half-chip grids, tails
        // two-phase ping-pong tiles: 256x256 (128 KiB), 192x256 (112 KiB), 128x256 (96 KiB)
        case 7: return launch_pp<256>(a, s);
        case 8: return launch_pp<192>(a, s);
        case 9: return launch_pp<128>(a, s);
        // 4 MFMA waves, 96x64 wave tiles, + 2 LDS-DMA helper waves (M≈3000 shapes: 1 round;
        // ACEHIP_GEMM_HELPERS=0: without, A/B)
        case 13: return knobs().gemm_helpers ? launch_w4<192, 128, 2>(a, s) : launch_w4<192, 128>(a, s);
        case 16: return launch<128, 64, 4, 1, 4>(a, s);   // 4 waves × 32 rows × 64 columns, 4-stage: M ≤ 128 SwiGLU
        case 17: return launch<128, 64, 4, 1, 4, 2>(a, s);  // 16 + two LDS-DMA helper waves (M ≤ 128 SwiGLU)
        default: return fail(-1, "gemm: bad variant (0, 7, 8, 9, 13, 16, 17)");
    }
}

#ifdef GEMM_STAMPS
}  // namespace acehip
extern "C" int acehip_diag_gemm_stamps(void *host, int n_wg) {
    n_wg = std::min(n_wg, acehip::STAMP_WG);
    HIP_TRY(hipMemcpyFromSymbol(host, HIP_SYMBOL(acehip::g_gemm_stamps), (size_t)n_wg * 2 * 8 * 8));
    return 0;
}
extern "C" int acehip_diag_gemm_stamps_clear(void) {
    void *p = nullptr;
    HIP_TRY(hipGetSymbolAddress(&p, HIP_SYMBOL(acehip::g_gemm_stamps)));
    HIP_TRY(hipMemset(p, 0, sizeof(acehip::g_gemm_stamps)));
    return 0;
}
namespace acehip {
#endif

bool gemm_ext_events(hipEvent_t start, hipEvent_t stop) {
    const bool consumed = g_ext_ev.stop && !g_ext_ev.start;
    g_ext_ev.start = start;
    g_ext_ev.stop = stop;
    return consumed;
}

// what gemm_plan reads besides the shape: the device's CU count, the count the tile planner
// fills (fewer under ACEHIP_GEMM_CUS, so tests reach multi-round grids at small shapes; PlanEnv
// says which decision reads which) and the planner's A/B switches
static PlanEnv plan_env(int dev_cus = 0) {
    const Knobs &k = knobs();
    const int n = dev_cus > 0 ? dev_cus : device_cus();
    return {n, k.gemm_cus > 0 && k.gemm_cus < n ? k.gemm_cus : n, k.gemm_tailsplit, k.gemm_helpers, k.splitk_fuse,
            k.splitk_bn, k.smallm_wholek, k.gemm_hp_tail, k.gemm_persist, k.gemm_saddr};
}

// sum the fp32 split partials in order + the GEMM's epilogue (head-post: staged bf16
// projection + the standalone head_post kernel, or head_post reading the partials itself)
static int splitk_finish(const GemmArgs &a, const GemmArgs &p, int splits, hipStream_t s) {
    if (a.epi == EPI_HEADPOST && knobs().splitk_fuse) {
        // head_post reads the partials itself (one launch, no bf16 staging round trip)
        HeadPostArgs h = a.hp;
        h.part = (const float *)a.ws;
        h.splits = splits;
        h.plane = (int64_t)a.M * a.N;
        h.ld_src = a.N;
        return head_post(h, s);
    }
    bf16_t *out = a.C;
    int64_t ldo = a.ldc;
    if (a.epi == EPI_HEADPOST) {   // bf16 projection staged after the partials
        out = (bf16_t *)((char *)a.ws + (size_t)splits * a.M * a.N * 4);
        ldo = a.N;
    }
    const int nout = a.epi == EPI_SWIGLU ? a.N / 2 : a.N;
    const int64_t thr = (int64_t)a.M * nout / 4;
    splitk_epilogue_kernel<<<(unsigned)((thr + 255) / 256), 256, 0, s>>>(p, splits, out, ldo);
    HIP_TRY(hipGetLastError());
    if (a.epi == EPI_HEADPOST) {
        HeadPostArgs h = a.hp;
        h.src = out;
        h.ld_src = a.N;
        return head_post(h, s);
    }
    return 0;
}

// The launches of a plan (gemm_plan.h), in order.  Tail splits and the walk with a tail run rows
// [0, M1) as hd and rows [M1, M) as tl.
static int gemm_launch(const GemmArgs &a, const GemmPlan &p, hipStream_t s, RowAdd *defer) {
    using Kern1 = void (*)(GemmArgs);
    using Kern2 = void (*)(GemmArgs, GemmArgs, int);
    GemmArgs hd = a, tl = a;
    if (p.ntail) {
        hd.M = p.M1;
        tl.M = a.M - p.M1;
        tl.A = a.A + (int64_t)p.M1 * a.lda;
        if (a.epi == EPI_HEADPOST) tl.hp.m_off += p.M1;   // C unused: rows scatter by (b, s)
        else tl.C = a.C + (int64_t)p.M1 * a.ldc;
    }
    switch (p.route) {
        case ACEHIP_ROUTE_TILE: return gemm_variant(a, p.v_head, s);
        case ACEHIP_ROUTE_TAIL2:
            if (int rc = gemm_variant(hd, p.v_head, s)) return rc;
            return gemm_variant(tl, p.v_tail, s);
        case ACEHIP_ROUTE_STAGED: {   // the projection as bf16 [M][N] in the workspace, then head_post
            GemmArgs st = a;
            st.epi = EPI_STORE;
            st.bias = nullptr;
            st.C = (bf16_t *)a.ws;
            st.ldc = a.N;
            if (int rc = gemm_variant(st, p.v_head, s)) return rc;
            HeadPostArgs hh = a.hp;
            hh.src = st.C;
            hh.ld_src = a.N;
            return head_post(hh, s);
        }
        case ACEHIP_ROUTE_WALK:   // gemm_pp_persist_kernel: at most one tail tile per workgroup
            if (p.ntail > p.grid) return fail(-1, "gemm: persistent walk with more tail tiles than workgroups");
            if (pp_tile_slotimm(knobs().gemm_slotimm, 1, a.epi, 256, a.lda, a.ldw))   // the walk is scalar-base under either ACEHIP_GEMM_SADDR
                klaunch(gemm_pp_persist_kernel<EPI_SWIGLU, true>, dim3(p.grid), dim3(512), s, hd, tl, p.nmain, p.nmain + p.ntail);
            else
                klaunch(gemm_pp_persist_kernel<EPI_SWIGLU, false>, dim3(p.grid), dim3(512), s, hd, tl, p.nmain, p.nmain + p.ntail);
            break;
        case ACEHIP_ROUTE_SPLITK: {   // fp32 partials of p.splits K ranges, then their sum + the epilogue
            GemmArgs q = a;
            q.kper = p.kper;
            const Kern1 k = p.bn == 64      ? (Kern1)gemm_kernel<128, 64, 4, 1, 3, EPI_PARTIAL>
                            : p.stages == 3 ? (Kern1)gemm_kernel<128, 128, 2, 2, 3, EPI_PARTIAL>
                                            : (Kern1)gemm_kernel<128, 128, 2, 2, 2, EPI_PARTIAL>;
            k<<<dim3(p.grid, p.splits), 256, 0, s>>>(q);
            HIP_TRY(hipGetLastError());
            if (!p.deferred) return splitk_finish(a, q, p.splits, s);
            // the residual epilogue is left to the consumer norm (in place: C == res)
            defer->xw = a.C;
            defer->part = (const float *)a.ws;
            defer->splits = p.splits;
            defer->prows = a.M;
            defer->plane = (int64_t)a.M * a.N;
            defer->gate = a.epi == EPI_GATED_RES ? a.gate : nullptr;
            defer->gate_bstride = a.gate_bstride;
            defer->gate_rpb = a.epi == EPI_GATED_RES ? a.rows_per_batch : 1;
            return 0;
        }
        case ACEHIP_ROUTE_TAIL1: {   // gemm_pp_split_kernel by source-address form and epilogue
            static const Kern2 split[3][3] = {
                {gemm_pp_split_kernel<EPI_SWIGLU, true, true>, gemm_pp_split_kernel<EPI_HEADPOST, true, true>, gemm_pp_split_kernel<EPI_STORE, true, true>},
                {gemm_pp_split_kernel<EPI_SWIGLU, true>, gemm_pp_split_kernel<EPI_HEADPOST, true>, gemm_pp_split_kernel<EPI_STORE, true>},
                {gemm_pp_split_kernel<EPI_SWIGLU, false>, gemm_pp_split_kernel<EPI_HEADPOST, false>, gemm_pp_split_kernel<EPI_STORE, false>}};
            const int form = !p.saddr ? 2 : pp_tile_slotimm(knobs().gemm_slotimm, 1, a.epi, 256, a.lda, a.ldw) ? 0 : 1;
            const Kern2 k = split[form][a.epi == EPI_SWIGLU ? 0 : a.epi == EPI_HEADPOST ? 1 : 2];
            if (a.epi == EPI_SWIGLU) klaunch(k, dim3(p.grid), dim3(512), s, hd, tl, p.nmain);
            else k<<<p.grid, 512, 0, s>>>(hd, tl, p.nmain);
            break;
        }
        default: return fail(-1, "gemm: bad route");
    }
    HIP_TRY(hipGetLastError());
    return 0;
}

// the conv epilogue on 64-row ping-pong tiles
static int launch_conv64(const GemmArgs &a, hipStream_t s) {
    const int tiles = ((a.M + 63) / 64) * (a.N / 256);
    gemm_pp_kernel<64, EPI_CONV, false><<<tiles, 512, 0, s>>>(a);
    HIP_TRY(hipGetLastError());
    return 0;
}

int gemm_conv(const GemmArgs &a, hipStream_t s) {
    if (a.epi != EPI_CONV || (!a.C && !a.Cs) || (a.Cs && (!a.sa || !a.sib)) || a.conv_cin <= 0 || a.conv_dil < 1 ||
        a.conv_ostride < 1 || a.conv_cout <= 0 || a.conv_cout % 8 || a.N % a.conv_cout || a.conv_lout <= 0 || a.M <= 0)
        return fail(-1, "gemm_conv: EPI_CONV with an output, snake parameters and conv geometry required");
    if (a.N % 256 || a.conv_cin % BK || a.K % a.conv_cin || a.lda != a.conv_cin || a.ldw != a.K || a.ldc != a.conv_cout)
        return fail(-1, "gemm_conv: N % 256, cin % 64, K = taps·cin and dense layouts required");
    if (a.res && (a.N != a.conv_cout || a.ldr != a.N || a.conv_ostride != 1 || a.conv_ooff != 0 || a.conv_lout != a.M))
        return fail(-1, "gemm_conv: a residual needs one phase with output row = m");
    if ((int64_t)((a.M + 255) / 256) * (a.N / 256) >= (1ll << 31)) return fail(-1, "gemm_conv: grid too large");
    switch (conv_tile_rows(a.M, a.N, device_cus())) {
        case 64: return launch_conv64(a, s);
        case 128: return launch_pp<128>(a, s);
        default: return launch_pp<256>(a, s);
    }
}

// what every path (split-K included) needs of a GEMM's shape and epilogue arguments
static int gemm_check(const GemmArgs &a) {
    if (a.N % 128 || a.K % BK || a.K <= 0)
        return fail(-1, "gemm: N%128 / K%64 violated (M=" + std::to_string(a.M) + " N=" +
                            std::to_string(a.N) + " K=" + std::to_string(a.K) + ")");
    if ((a.lda | a.ldw | a.ldc) % 8) return fail(-1, "gemm: leading dims must be multiples of 8");
    if (a.epi == EPI_GATED_RES && (!a.gate || a.rows_per_batch <= 0)) return fail(-1, "gemm: gate");
    if ((a.epi == EPI_GATED_RES || a.epi == EPI_RES) && !a.res) return fail(-1, "gemm: res");
    if (a.epi == EPI_HEADPOST) {
        const HeadPostArgs &h = a.hp;
        if (a.N % 256 || h.S <= 0 || (int64_t)h.B * h.S != a.M || (h.nq + h.nk + h.nv) * 128 != a.N ||
            h.S_dst < h.S || (h.S_dst_q && h.S_dst_q < h.S) || (h.nq && !h.qw) || (h.nk && !h.kw) || (h.cos == nullptr) != (h.sin == nullptr))
            return fail(-1, "gemm: head-post arguments inconsistent with the GEMM shape");
    }
    return 0;
}

int gemm(const GemmArgs &a, hipStream_t s, RowAdd *defer) {
    if (defer) defer->part = nullptr;
    if (a.M <= 0) return 0;
    if (int rc = gemm_check(a)) return rc;
    // a deferred epilogue needs the in-place residual form the consumer norm applies
    const bool defer_ok = defer && a.res == a.C && a.ldr == a.ldc && a.ldc == a.N;
    const PlanIn in{a.M, a.N, a.K, a.epi, a.lda, a.ldw, a.ws ? a.ws_bytes : 0, defer_ok};
    return gemm_launch(a, gemm_plan(in, plan_env()), s, defer);
}

// ---------------------------------------------------------------------------
// Fused cross-Q projection + cross-attention (cross_q_attn_kernel).  cq is the cross-Q head-post
// GEMM as forward_body builds it (q heads only, no RoPE; cq.hp.q is not written).
// cross_fuse_shape: what the kernel itself needs — one q head per 128 columns, two q heads per KV
// head, and every 192-row tile inside one batch element.
bool cross_fuse_shape(const GemmArgs &cq, int KV, int Sk) {
    const HeadPostArgs &h = cq.hp;
    return cq.epi == EPI_HEADPOST && cq.M > 0 && cq.K > 0 && cq.K % BK == 0 && cq.N == h.nq * 128 && h.nk == 0 &&
           h.nv == 0 && !h.cos && !h.sin && h.qw && h.m_off == 0 && h.S > 0 && (int64_t)h.B * h.S == cq.M &&
           KV > 0 && h.nq == 2 * KV && Sk > 0 && (h.B == 1 || h.S % 192 == 0) && (cq.lda | cq.ldw) % 8 == 0;
}
// cross_fuse_planned: cq belongs on the half-chip four-wave tile with its helper waves (variant
// 13: one round of 192 × 128 tiles on at least three quarters of the planned CUs, and not the
// small-M split-K path) — gemm_plan.h cross_fuse_plan, which says how it differs from gemm()'s route
bool cross_fuse_planned(const GemmArgs &cq) { return cross_fuse_plan(cq.M, cq.N, cq.K, cq.ws != nullptr, plan_env()); }
int cross_q_attention(const GemmArgs &cq, const bf16_t *k, const bf16_t *v, bf16_t *o, int KV, int Sk, float scale,
                      int64_t o_ld, hipStream_t s) {
    if (!cross_fuse_shape(cq, KV, Sk)) return fail(-1, "cross_q_attention: shape outside the fused kernel's");
    if (!k || !v || !o || o_ld % 8 || o_ld < cq.N) return fail(-1, "cross_q_attention: K / V / O");
    XAttnArgs xa{k, v, o, KV, Sk, scale * 1.4426950408889634f, o_ld};
    const int tiles = ((cq.M + 191) / 192) * (cq.N / 128);
    cross_q_attn_kernel<<<tiles, 384, 0, s>>>(cq, xa);
    HIP_TRY(hipGetLastError());
    return 0;
}

}  // namespace acehip

// Host-only window on the dispatch (tests; no kernel launch): the plan gemm() would launch from
extern "C" int acehip_diag_gemm_plan(int M, int N, int K, int64_t lda, int64_t ldw, int epi, size_t ws_bytes,
                                     int defer_ok, int device_cus, acehip_gemm_plan *out) {
    using namespace acehip;
    if (!out || M <= 0 || N <= 0 || N % 128 || K <= 0 || K % BK || epi < EPI_STORE || epi > EPI_HEADPOST ||
        (epi == EPI_HEADPOST && N % 256) || lda < K || ldw < K || (lda | ldw) % 8 || device_cus < 0)
        return fail(ACEHIP_E_ARG, "diag_gemm_plan: a shape gemm() refuses, or a null plan");
    *out = gemm_plan(PlanIn{M, N, K, epi, lda, ldw, ws_bytes, defer_ok != 0}, plan_env(device_cus));
    return 0;
}

// Host-only check of the two source-address forms (tests; no GPU call): for every row tile, column
// tile, wave, lane, piece and K-tile of a BM × 256 ping-pong grid, the byte address relative to A / W
// formed as the pointer form does (64-bit per lane) and as the scalar-base form does (64-bit tile
// base + K offset, plus the lane's offset in 32-bit wrap-around arithmetic, zero-extended — what
// global_load_lds with an SGPR base adds).  An A address depends on the row tile only and a W
// address on the column tile only, so the two are walked separately.
extern "C" int64_t acehip_diag_pp_src_check(int M, int N, int K, int64_t lda, int64_t ldw, int BM, int conv_cin,
                                            int conv_dil, int conv_a0, int *fits, int64_t *min_a, int64_t *max_a,
                                            int64_t *max_b) {
    using namespace acehip;
    if (M <= 0 || N <= 0 || N % 256 || K <= 0 || K % BK || lda <= 0 || ldw <= 0 ||
        (BM != 64 && BM != 128 && BM != 192 && BM != 256) ||
        (conv_cin && (conv_cin < 0 || conv_cin % BK || K % conv_cin || conv_dil < 1))) {
        fail(-1, "diag_pp_src_check: M, N % 256, K % 64, BM in {64, 128, 192, 256}, conv_cin % 64");
        return -1;
    }
    int64_t bad = 0, lo = INT64_MAX, hi_a = INT64_MIN, hi_b = INT64_MIN;
    const int nk = K / BK, NA = BM / 64;
    for (int m0 = 0; m0 < M; m0 += BM)
        for (int wave = 0; wave < 8; ++wave)
            for (int lane = 0; lane < 64; ++lane)
                for (int i = 0; i < NA; ++i) {
                    const int64_t p = pp_ptr_a(M, lda, m0, wave, lane, i) * 2, base = (int64_t)m0 * lda * 2;
                    const uint32_t off = pp_off_a(M, lda, m0, wave, lane, i);
                    for (int kt = 0; kt < nk; ++kt) {
                        const int ko = conv_cin ? pp_conv_ko(kt * BK, conv_cin, conv_dil, conv_a0) : kt * BK;
                        const int64_t ap = p + (int64_t)ko * 2, as = base + (int64_t)ko * 2 + (int64_t)(uint64_t)off;
                        bad += ap != as;
                        lo = std::min(lo, ap);
                        hi_a = std::max(hi_a, ap + 15);
                    }
                }
    const uint32_t bstep = pp_off_bstep(ldw);
    for (int n0 = 0; n0 < N; n0 += 256)
        for (int wave = 0; wave < 8; ++wave)
            for (int lane = 0; lane < 64; ++lane)
                for (int i = 0; i < 4; ++i) {
                    const int64_t p = pp_ptr_b(BM, ldw, n0, wave, lane, i) * 2;
                    const int64_t base = (int64_t)n0 * ldw * 2 + (int64_t)((uint64_t)i * bstep);
                    const uint32_t off = pp_off_b(ldw, wave, lane);
                    for (int kt = 0; kt < nk; ++kt) {
                        const int64_t bp = p + (int64_t)kt * BK * 2, bs = base + (int64_t)kt * BK * 2 + (int64_t)(uint64_t)off;
                        bad += bp != bs;
                        hi_b = std::max(hi_b, bp + 15);
                    }
                }
    if (fits) *fits = pp_saddr_fits(BM, lda, ldw) ? 1 : 0;
    if (min_a) *min_a = lo;
    if (max_a) *max_a = hi_a;
    if (max_b) *max_b = hi_b;
    return bad;
}

// acehip_diag_pp_lds_check (include/acehip.h): every LDS read of the slot-immediate K loop as
// the kernel forms it — pp_rd_base + pp_rd_imm, in 32-bit arithmetic — against the ring slot's
// swizzled address
extern "C" int64_t acehip_diag_pp_lds_check(uint32_t lds, int64_t *reads, int *max_imm, int64_t *max_end) {
    using namespace acehip;
    int64_t bad = 0, n = 0, end = 0;
    int imm_hi = 0;
    for (int BM : {64, 128, 192, 256}) {
        const int SM = BM / 32;   // 16-row A sub-tiles per wave
        for (int wave = 0; wave < 8; ++wave)
            for (int lane = 0; lane < 64; ++lane)
                for (int slot = 0; slot < 2; ++slot)
                    for (int ks = 0; ks < 2; ++ks)
                        for (int op = 0; op < 2; ++op) {   // 0: A, 1: W
                            const int first = op ? pp_rd_brow(BM, wave) : pp_rd_arow(BM, wave);
                            const uint32_t base = pp_rd_base(lds, BM, first, lane, ks, slot);
                            for (int sub = 0; sub < (op ? 4 : SM); ++sub) {
                                const int imm = pp_rd_imm(sub), row = first + sub * 16 + (lane & 15);
                                const uint32_t got = base + (uint32_t)imm;
                                const uint32_t want = lds + (uint32_t)(slot * pp_buf_bytes(BM)) + pp_swz(row, ks * 4 + (lane >> 4));
                                const int64_t rel = (int64_t)got - (int64_t)lds;   // inside the kernel's LDS array
                                bad += got != want || imm < 0 || imm >= 65536 || rel < 0 || rel + 16 > 2 * (int64_t)pp_buf_bytes(BM) ||
                                       row >= (op ? BM + 256 : BM);
                                imm_hi = std::max(imm_hi, imm);
                                end = std::max(end, rel + 16);
                                ++n;
                            }
                        }
    }
    if (reads) *reads = n;
    if (max_imm) *max_imm = imm_hi;
    if (max_end) *max_end = end;
    return bad;
}

// acehip_diag_pp_slotimm (include/acehip.h)
extern "C" int acehip_diag_pp_slotimm(int epi, int BM, int64_t lda, int64_t ldw) {
    const acehip::Knobs &k = acehip::knobs();
    return acehip::pp_tile_slotimm(k.gemm_slotimm, k.gemm_saddr, epi, BM, lda, ldw) ? 1 : 0;
}
