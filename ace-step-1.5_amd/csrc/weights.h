// weights.h — host-only weight loading the model handles (dit.hip, dit_f32.hip, encoder.hip,
// vae.hip) share: the table of state-dict names a handle accepts, the two ways a caller's tensor
// is fetched (to the host as float, to the device as bf16), the DiT's patch-conv repacks and the
// gate/up packing.  Runs at load time only; no kernel, plan or launch argument lives here.
#pragma once
#include <algorithm>
#include <map>
#include <string>
#include <vector>

#include "kernels.h"
#include "../../include/acehip.h"

namespace acehip {

// `elems` bf16 elements of device memory, freed with the handle (its `allocs`); null on failure
inline bf16_t *dev_alloc(std::vector<void *> &allocs, size_t elems) {
    void *p = nullptr;
    if (hipMalloc(&p, std::max<size_t>(elems, 1) * 2) != hipSuccess) return nullptr;
    allocs.push_back(p);
    return (bf16_t *)p;
}

// device memory of one call, freed when it returns
struct DevTemp {
    void *p = nullptr;
    DevTemp() = default;
    DevTemp(const DevTemp &) = delete;
    DevTemp &operator=(const DevTemp &) = delete;
    ~DevTemp() {
        if (p) (void)hipFree(p);
    }
};

// a handle's device staging buffer for fp32 → bf16 casts; p == null: the handle keeps none
struct Staging {
    void *p = nullptr;
    size_t bytes = 0;
};

// ---- source fetches: ptr holds n contiguous elements of dtype (ACEHIP_F32 / ACEHIP_BF16), on
// the device or the host
inline int fetch_host_f32(const void *ptr, int dtype, int64_t n, int on_device, std::vector<float> &out) {
    const hipMemcpyKind kind = on_device ? hipMemcpyDeviceToHost : hipMemcpyHostToHost;
    out.resize(n);
    if (dtype == ACEHIP_F32) {
        HIP_TRY(hipMemcpy(out.data(), ptr, n * 4, kind));
    } else {
        std::vector<bf16_t> b(n);
        HIP_TRY(hipMemcpy(b.data(), ptr, n * 2, kind));
        for (int64_t i = 0; i < n; ++i) out[i] = bf2f(b[i]);
    }
    return 0;
}

// to n contiguous bf16 at dst (device).  fp32 input is cast by cast_f32_bf16 (RNE, the rounding
// of torch's .to(bfloat16)) in chunks through `staging`; without one, through a temporary that
// is freed before returning.
inline int fetch_dev_bf16(const void *ptr, int dtype, int64_t n, int on_device, bf16_t *dst, Staging staging) {
    const hipMemcpyKind kind = on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
    if (dtype == ACEHIP_BF16) {
        HIP_TRY(hipMemcpy(dst, ptr, n * 2, kind));
        return 0;
    }
    DevTemp own;
    if (!staging.p) {
        staging.bytes = (size_t)std::min<int64_t>(std::max<int64_t>(n, 1), (int64_t)16 << 20) * 4;
        if (hipMalloc(&own.p, staging.bytes) != hipSuccess) {
            own.p = nullptr;
            return fail(ACEHIP_E_OOM, "weight load: staging allocation failed");
        }
        staging.p = own.p;
    }
    const float *fsrc = (const float *)ptr;
    float *fstage = (float *)staging.p;
    const int64_t chunk = (int64_t)(staging.bytes / 4);
    for (int64_t off = 0; off < n; off += chunk) {
        const int64_t c = std::min(chunk, n - off);
        HIP_TRY(hipMemcpy(fstage, fsrc + off, c * 4, kind));
        if (int rc = cast_f32_bf16(fstage, dst + off, c, 0)) return rc;
        HIP_TRY(hipDeviceSynchronize());
    }
    return 0;
}

// gate_proj / up_proj [F][K] (contiguous bf16 at src) into the SwiGLU epilogue's layout at dst
// [2F][K]: 64-row panels of 32 gate rows, then the 32 up rows of the same outputs
inline int pack_gate_up(bf16_t *dst, const bf16_t *src, int64_t F, int64_t K, bool is_up, hipMemcpyKind kind) {
    HIP_TRY(hipMemcpy2D(dst + (is_up ? 32 * K : 0), 64 * K * 2, src, 32 * K * 2, 32 * K * 2, F / 32, kind));
    return 0;
}

// ---- the DiT's patch convs as GEMM operands (index maps only; the destination rounds)
// proj_in Conv1d [D][192][2] → [D][k·192 + c]: the patch GEMM reads [T][192] rows pairwise
inline void repack_proj_in(const float *src, int64_t D, float *dst) {
    for (int64_t o = 0; o < D; ++o)
        for (int c = 0; c < 192; ++c)
            for (int k = 0; k < 2; ++k) dst[o * 384 + k * 192 + c] = src[(o * 192 + c) * 2 + k];
}
// proj_out ConvTranspose1d [D][64][2] → [k·64 + o][D]: the GEMM output [S][128] is the
// de-patchified [2S][64] sequence in place
inline void repack_proj_out_w(const float *src, int64_t D, float *dst) {
    for (int64_t c = 0; c < D; ++c)
        for (int o = 0; o < 64; ++o)
            for (int k = 0; k < 2; ++k) dst[(k * 64 + o) * D + c] = src[(c * 64 + o) * 2 + k];
}
// proj_out bias [64] → [k·64 + o]
inline void repack_proj_out_b(const float *src, float *dst) {
    for (int k = 0; k < 2; ++k)
        for (int o = 0; o < 64; ++o) dst[k * 64 + o] = src[o];
}

// ---- the table of weights a handle accepts
enum class Pack { COPY, GU_GATE, GU_UP, PROJ_IN, PROJ_OUT_W, PROJ_OUT_B };

struct WeightSlot {
    void *dst = nullptr;          // device; bf16_t or float by f32
    bool f32 = false;             // the destination's precision
    std::vector<int64_t> shape;   // of the reference tensor
    Pack kind = Pack::COPY;
    bool set = false;
};

inline std::string shape_text(const std::vector<int64_t> &s) {
    std::string e = "[";
    for (auto v : s) e += std::to_string(v) + ",";
    return e + "]";
}

struct WeightTable {
    std::map<std::string, WeightSlot> slots;

    void add(const std::string &name, bf16_t *dst, std::vector<int64_t> shape, Pack kind = Pack::COPY) {
        slots[name] = WeightSlot{dst, false, std::move(shape), kind, false};
    }
    void add(const std::string &name, float *dst, std::vector<int64_t> shape, Pack kind = Pack::COPY) {
        slots[name] = WeightSlot{dst, true, std::move(shape), kind, false};
    }
    // the slot of `name` if the caller's shape is the reference's; who: "dit_set_weight" / "enc_set_weight"
    int find_checked(const std::string &name, int ndim, const int64_t *shape, const char *who, WeightSlot *&out) {
        auto it = slots.find(name);
        if (it == slots.end()) return fail(ACEHIP_E_NAME, std::string(who) + ": unknown weight " + name);
        const std::vector<int64_t> sh(shape, shape + std::max(ndim, 0));
        if (sh != it->second.shape)
            return fail(ACEHIP_E_ARG, std::string(who) + ": shape mismatch for " + name + " got " + shape_text(sh) +
                                          " want " + shape_text(it->second.shape));
        out = &it->second;
        return 0;
    }
    // 0 when every slot is set; who: "dit_finalize" / "enc_finalize"
    int missing(const char *who) const {
        std::string m;
        for (auto &kv : slots)
            if (!kv.second.set) m += kv.first + " ";
        return m.empty() ? 0 : fail(ACEHIP_E_STATE, std::string(who) + ": missing weights: " + m.substr(0, 400));
    }
};

// Store the caller's tensor (the slot's reference shape, contiguous) in the slot's layout and
// precision.  bf16 destinations: plain weights and gate/up stay on the device (fetch_dev_bf16),
// the small patch-conv repacks go through the host; fp32 destinations (the DiT parity mode,
// where load time is no concern) always go through the host.  who / name: for the error texts.
inline int load_weight(WeightSlot &s, const char *who, const std::string &name, const void *ptr, int dtype,
                       int on_device, Staging staging) {
    if (dtype != ACEHIP_F32 && dtype != ACEHIP_BF16)
        return fail(ACEHIP_E_ARG, std::string(who) + ": unsupported dtype code for " + name);
    int64_t n = 1;
    for (auto v : s.shape) n *= v;
    const bool gate_up = s.kind == Pack::GU_GATE || s.kind == Pack::GU_UP;
    if (s.f32 || (!gate_up && s.kind != Pack::COPY)) {
        if (gate_up) return fail(ACEHIP_E_ARG, std::string(who) + ": gate/up panels have no fp32 form (" + name + ")");
        std::vector<float> v, r;
        if (int rc = fetch_host_f32(ptr, dtype, n, on_device, v)) return rc;
        if (s.kind == Pack::PROJ_IN) { r.resize(n); repack_proj_in(v.data(), s.shape[0], r.data()); }
        else if (s.kind == Pack::PROJ_OUT_W) { r.resize(n); repack_proj_out_w(v.data(), s.shape[0], r.data()); }
        else if (s.kind == Pack::PROJ_OUT_B) { r.resize(128); repack_proj_out_b(v.data(), r.data()); }
        else r.swap(v);
        if (s.f32) {
            HIP_TRY(hipMemcpy(s.dst, r.data(), r.size() * 4, hipMemcpyHostToDevice));
        } else {
            std::vector<bf16_t> b(r.size());
            for (size_t i = 0; i < r.size(); ++i) b[i] = f2bf(r[i]);
            HIP_TRY(hipMemcpy(s.dst, b.data(), b.size() * 2, hipMemcpyHostToDevice));
        }
    } else if (s.kind == Pack::COPY) {
        if (int rc = fetch_dev_bf16(ptr, dtype, n, on_device, (bf16_t *)s.dst, staging)) return rc;
    } else {
        // gate / up: bf16 input is packed straight from where it lies; fp32 input is cast whole,
        // the fp32 copy at the front of the staging buffer and its bf16 cast behind it
        const bf16_t *src = (const bf16_t *)ptr;
        hipMemcpyKind kind = on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
        DevTemp own;
        if (dtype == ACEHIP_F32) {
            if (staging.p) {
                if ((size_t)n * 6 > staging.bytes)
                    return fail(ACEHIP_E_ARG, "fp32 weight too large for staging; pass bf16");
            } else {
                if (hipMalloc(&own.p, (size_t)n * 6) != hipSuccess) {
                    own.p = nullptr;
                    return fail(ACEHIP_E_OOM, "weight load: staging allocation failed");
                }
                staging.p = own.p;
            }
            bf16_t *b16 = (bf16_t *)staging.p + n * 2;
            if (int rc = fetch_dev_bf16(ptr, dtype, n, on_device, b16, Staging{staging.p, (size_t)n * 4})) return rc;
            src = b16;
            kind = hipMemcpyDeviceToDevice;
        }
        if (int rc = pack_gate_up((bf16_t *)s.dst, src, s.shape[0], s.shape[1], s.kind == Pack::GU_UP, kind)) return rc;
    }
    s.set = true;
    return 0;
}

}  // namespace acehip
