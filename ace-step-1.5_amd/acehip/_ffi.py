"""ctypes binding of libacehip.so (C ABI declared in include/acehip.h).

The library is built in-tree (``make -C ace-step-1.5_amd`` or
``__graft_entry__.build()``) and loaded from this directory.  There is no
fallback: if the shared object is missing or fails to load, every entry point
raises — the product path never silently degrades to a CPU/eager path.
"""
from __future__ import annotations

import ctypes
import os
from ctypes import POINTER, c_char_p, c_float, c_int, c_int64, c_uint8, c_void_p

LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "libacehip.so")

ACEHIP_F32 = 0
ACEHIP_BF16 = 1
# include/acehip.h ACEHIP_VERSION this binding's signatures were written against
ABI_VERSION = 400

# every symbol include/acehip.h declares (checked by tests/test_abi.py)
EXPORTS = [
    "acehip_get_version", "acehip_last_error", "acehip_reload_knobs", "acehip_build_hash",
    "acehip_dit_create", "acehip_dit_set_weight", "acehip_dit_finalize",
    "acehip_dit_set_condition", "acehip_dit_set_uniform_rows", "acehip_dit_forward", "acehip_dit_destroy",
    "acehip_dit_set_graph", "acehip_dit_set_timesteps", "acehip_dit_forward_step",
    "acehip_dit_profile", "acehip_dit_profile_read", "acehip_dit_profile_kinds",
    "acehip_sampler_apg_euler", "acehip_sampler_adg_euler", "acehip_sampler_axpy",
    "acehip_vae_create", "acehip_vae_set_weight", "acehip_vae_finalize", "acehip_vae_decode",
    "acehip_vae_decode_blocks",
    "acehip_vae_encode", "acehip_vae_destroy", "acehip_vae_conv", "acehip_vae_resunit",
    "acehip_wav_peak_normalize", "acehip_wav_postprocess", "acehip_wav_postprocess_pcm16",
    "acehip_gemm_bf16", "acehip_gemm_bf16_ex", "acehip_gemm_res_bf16", "acehip_gemm_res_norm_bf16",
    "acehip_attention_bf16",
    "acehip_rmsnorm_bf16", "acehip_gemm_headpost_bf16", "acehip_attention_masked_bf16", "acehip_cross_attn_bf16",
    "acehip_enc_create", "acehip_enc_set_weight", "acehip_enc_finalize", "acehip_enc_embed",
    "acehip_enc_forward", "acehip_enc_destroy", "acehip_fsq_quantize", "acehip_fsq_codes_from_indices",
    "acehip_attention_probs_bf16", "acehip_dit_forward_capture",
    "acehip_enc_kv_create", "acehip_enc_prefill", "acehip_enc_decode",
    "acehip_attention_decode_ws_bytes", "acehip_attention_decode_bf16", "acehip_lm_head_bf16",
    "acehip_lm_filter_ws_bytes", "acehip_lm_filter", "acehip_lm_score_ws_bytes", "acehip_lm_score_bf16",
    "acehip_diag_pp_src_check", "acehip_diag_gemm_plan", "acehip_diag_attn_plan",
    "acehip_diag_pp_lds_check", "acehip_diag_pp_slotimm",
    "acehip_attention_extend_ws_bytes", "acehip_attention_extend_bf16", "acehip_diag_attn_extend_plan",
    "acehip_enc_extend",
]


class DiTCfg(ctypes.Structure):
    _fields_ = [("hidden", c_int), ("intermediate", c_int), ("heads", c_int), ("kv_heads", c_int),
                ("head_dim", c_int), ("layers", c_int), ("window", c_int), ("patch", c_int),
                ("in_channels", c_int), ("out_channels", c_int), ("eps", c_float),
                ("rope_theta", c_float), ("max_S", c_int), ("max_Bc", c_int), ("max_Lenc", c_int),
                ("sliding", POINTER(c_uint8)), ("fp32", c_int)]


class EncCfg(ctypes.Structure):
    _fields_ = [("hidden", c_int), ("intermediate", c_int), ("heads", c_int), ("kv_heads", c_int),
                ("head_dim", c_int), ("layers", c_int), ("window", c_int), ("in_dim", c_int),
                ("embed_bias", c_int), ("out_dim", c_int), ("eps", c_float), ("rope_theta", c_float),
                ("max_tokens", c_int), ("max_S", c_int), ("sliding", POINTER(c_uint8))]


class VAECfg(ctypes.Structure):
    _fields_ = [("encoder_hidden", c_int), ("decoder_channels", c_int), ("latent_channels", c_int),
                ("audio_channels", c_int), ("n_blocks", c_int), ("ratios", c_int * 8),
                ("multiples", c_int * 8), ("max_T", c_int), ("max_B", c_int),
                ("with_encoder", c_int)]


class AttnCapture(ctypes.Structure):
    """acehip_attn_capture (include/acehip.h)."""
    _fields_ = [("n", c_int), ("layer", POINTER(c_int)), ("head", POINTER(c_int)), ("k0", c_int), ("k1", c_int),
                ("out", POINTER(c_float)), ("stop_after_last", c_int)]


# acehip_gemm_plan.route (include/acehip.h ACEHIP_ROUTE_*)
ROUTE_TILE, ROUTE_SPLITK, ROUTE_STAGED, ROUTE_TAIL2, ROUTE_TAIL1, ROUTE_WALK = range(6)


class GemmPlan(ctypes.Structure):
    """acehip_gemm_plan (include/acehip.h)."""
    _fields_ = [(n, c_int) for n in ("route", "v_head", "v_tail", "M1", "nmain", "ntail", "grid", "splits", "kper",
                                     "bn", "stages", "deferred", "saddr", "helpers")]


# acehip_attn_plan.kernel (include/acehip.h ACEHIP_ATTN_*)
ATTN_SMALL, ATTN_PW, ATTN_FWD = 1, 2, 3


class AttnPlan(ctypes.Structure):
    """acehip_attn_plan (include/acehip.h)."""
    _fields_ = [(n, c_int) for n in ("kernel", "nrep", "window", "units", "unit_tiles", "full", "nsplit", "parts",
                                     "grid", "block", "persist", "streamk", "sk_nt", "sk_total", "causal", "uses_ws")]


class AttnExtendPlan(ctypes.Structure):
    """acehip_attn_extend_plan (include/acehip.h)."""
    _fields_ = [(n, c_int) for n in ("unit_rows", "unit_queries", "qblocks", "units", "tiles", "parts",
                                     "tiles_per_part", "grid", "block", "uses_ws")]


_LIB = None


def _declare(lib):
    P = c_void_p
    sig = {
        "acehip_get_version": (c_int, []),
        "acehip_last_error": (c_char_p, []),
        "acehip_build_hash": (c_char_p, []),
        "acehip_reload_knobs": (c_int, []),
        "acehip_dit_create": (c_int, [c_int, POINTER(DiTCfg), POINTER(c_void_p)]),
        "acehip_dit_set_weight": (c_int, [P, c_char_p, P, c_int, c_int, POINTER(c_int64), c_int]),
        "acehip_dit_finalize": (c_int, [P]),
        "acehip_dit_set_condition": (c_int, [P, P, c_int, c_int, P]),
        "acehip_dit_set_uniform_rows": (c_int, [P, c_int, P]),
        "acehip_dit_forward": (c_int, [P, P, P, c_int, P, P, c_int, c_int, c_int, c_int, P, P]),
        "acehip_dit_forward_capture": (c_int, [P, P, P, c_int, P, P, c_int, c_int, c_int, c_int, P,
                                               POINTER(AttnCapture), P]),
        "acehip_dit_destroy": (c_int, [P]),
        "acehip_dit_set_graph": (c_int, [P, c_int]),
        "acehip_dit_set_timesteps": (c_int, [P, P, P, c_int, P]),
        "acehip_dit_forward_step": (c_int, [P, P, P, c_int, c_int, c_int, c_int, c_int, P, P]),
        "acehip_dit_profile": (c_int, [P, c_int]),
        "acehip_dit_profile_kinds": (c_int, [P, ctypes.c_uint]),
        "acehip_dit_profile_read": (c_int, [P, c_int, POINTER(c_int), POINTER(c_float)]),
        "acehip_sampler_apg_euler": (c_int, [P, P, P, c_int, c_int, c_int, c_float, c_float, c_int,
                                             c_int, c_int, c_int, P]),
        "acehip_sampler_adg_euler": (c_int, [P, P, c_int, c_int, c_int, c_float, c_float, c_float, c_int, c_int, P]),
        "acehip_sampler_axpy": (c_int, [P, P, c_int64, c_float, c_int, P]),
        "acehip_vae_create": (c_int, [c_int, POINTER(VAECfg), POINTER(c_void_p)]),
        "acehip_vae_set_weight": (c_int, [P, c_char_p, P, c_int, c_int, POINTER(c_int64), c_int]),
        "acehip_vae_finalize": (c_int, [P]),
        "acehip_vae_decode": (c_int, [P, P, c_int, c_int, P, P]),
        "acehip_vae_decode_blocks": (c_int, [P, P, c_int, c_int, P, P]),
        "acehip_vae_encode": (c_int, [P, P, c_int, c_int, P, P, P]),
        "acehip_vae_destroy": (c_int, [P]),
        "acehip_vae_conv": (c_int, [c_int, P, c_int64, c_int, P, P, P, c_int, c_int, c_int, c_int, P, P, P, P, P]),
        "acehip_vae_resunit": (c_int, [P, P, c_int64, c_int, c_int, P, P, P, P, P, P, P, P, P, P, P]),
        "acehip_wav_peak_normalize": (c_int, [P, c_int, c_int64, P, P]),
        "acehip_wav_postprocess": (c_int, [P, c_int, c_int64, P, c_int, c_float, P]),
        "acehip_wav_postprocess_pcm16": (c_int, [P, c_int, c_int, c_int64, P, c_int, c_float, P, P]),
        "acehip_gemm_bf16": (c_int, [P, c_int, P, c_int, P, c_int, c_int, c_int, c_int, P, P]),
        "acehip_gemm_bf16_ex": (c_int, [P, c_int, P, c_int, P, c_int, c_int, c_int, c_int, P, c_int,
                                        c_int, P]),
        "acehip_gemm_res_bf16": (c_int, [P, c_int, P, c_int, P, c_int, c_int, c_int, c_int, P, c_int, P, c_int64,
                                         c_int, c_int, P]),
        "acehip_diag_pp_src_check": (c_int64, [c_int, c_int, c_int, c_int64, c_int64, c_int, c_int, c_int, c_int,
                                               POINTER(c_int), POINTER(c_int64), POINTER(c_int64),
                                               POINTER(c_int64)]),
        "acehip_diag_pp_lds_check": (c_int64, [ctypes.c_uint32, POINTER(c_int64), POINTER(c_int), POINTER(c_int64)]),
        "acehip_diag_pp_slotimm": (c_int, [c_int, c_int, c_int64, c_int64]),
        "acehip_diag_gemm_plan": (c_int, [c_int, c_int, c_int, c_int64, c_int64, c_int, ctypes.c_size_t, c_int, c_int,
                                          POINTER(GemmPlan)]),
        "acehip_diag_attn_plan": (c_int, [c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int,
                                          POINTER(AttnPlan)]),
        "acehip_gemm_res_norm_bf16": (c_int, [P, c_int, P, c_int, P, c_int, c_int, c_int, P, c_int64, c_int, c_int,
                                              P, P, P, c_int64, P, c_int, c_float, P, c_int, POINTER(c_int), P]),
        "acehip_attention_bf16": (c_int, [P, P, P, P, c_int, c_int, c_int, c_int, c_int, c_int,
                                          c_float, P]),
        "acehip_attention_masked_bf16": (c_int, [P, P, P, P, c_int, c_int, c_int, c_int, c_int, c_int,
                                                 c_float, P, P]),
        "acehip_attention_probs_bf16": (c_int, [P, P, c_int, c_int, c_int, c_int, c_int, POINTER(c_int), c_int,
                                                c_int, c_int, c_float, P, P]),
        "acehip_enc_create": (c_int, [c_int, POINTER(EncCfg), POINTER(c_void_p)]),
        "acehip_enc_set_weight": (c_int, [P, c_char_p, P, c_int, c_int, POINTER(c_int64), c_int]),
        "acehip_enc_finalize": (c_int, [P]),
        "acehip_enc_embed": (c_int, [P, P, c_int, P, P]),
        "acehip_enc_forward": (c_int, [P, P, P, c_int, c_int, P, P]),
        "acehip_enc_destroy": (c_int, [P]),
        "acehip_enc_kv_create": (c_int, [P, c_int, c_int]),
        "acehip_enc_prefill": (c_int, [P, P, P, c_int, c_int, P, P]),
        "acehip_enc_decode": (c_int, [P, P, P, c_int, c_int, c_int, P, P]),
        "acehip_attention_decode_ws_bytes": (ctypes.c_size_t, [c_int, c_int]),
        "acehip_attention_decode_bf16": (c_int, [P, P, P, P, c_int, c_int, c_int, c_int, c_int, P, c_int, c_float,
                                                 P, ctypes.c_size_t, P]),
        "acehip_enc_extend": (c_int, [P, P, P, c_int, c_int, c_int, c_int, c_int, P, P]),
        "acehip_attention_extend_ws_bytes": (ctypes.c_size_t, [c_int, c_int, c_int]),
        "acehip_attention_extend_bf16": (c_int, [P, P, P, P, c_int, c_int, c_int, c_int, c_int, c_int, P, c_int,
                                                 c_float, P, ctypes.c_size_t, P]),
        "acehip_diag_attn_extend_plan": (c_int, [c_int, c_int, c_int, c_int, c_int, c_int, c_int,
                                                 POINTER(AttnExtendPlan), POINTER(ctypes.c_size_t)]),
        "acehip_lm_head_bf16": (c_int, [P, c_int, P, P, c_int, c_int, c_int, c_int, P]),
        "acehip_lm_filter_ws_bytes": (ctypes.c_size_t, [c_int, c_int]),
        "acehip_lm_filter": (c_int, [P, c_int, c_int, c_int, c_int, c_int, c_float, P, ctypes.c_size_t, P]),
        "acehip_lm_score_ws_bytes": (ctypes.c_size_t, [c_int, c_int]),
        "acehip_lm_score_bf16": (c_int, [P, c_int, P, P, c_int, c_int, c_int, P, P, P, P, P, ctypes.c_size_t, P]),
        "acehip_fsq_quantize": (c_int, [P, c_int, c_int, POINTER(c_int), c_int, P, c_int, P, P]),
        "acehip_fsq_codes_from_indices": (c_int, [P, c_int, POINTER(c_int), c_int, P, c_int, P]),
        "acehip_rmsnorm_bf16": (c_int, [P, P, P, P, c_int64, c_int, P, c_int, c_int, c_float, c_int, P]),
        "acehip_gemm_headpost_bf16": (c_int, [P, c_int, P, c_int, c_int, c_int, c_int, c_int, c_int,
                                              P, P, P, P, c_float, P, P, P, P]),
        "acehip_cross_attn_bf16": (c_int, [P, P, P, P, P, P, c_int, c_int, c_int, c_int, c_int, c_int, c_float,
                                           c_float, c_int, POINTER(c_int), P]),
    }
    for name, (res, args) in sig.items():
        if not hasattr(lib, name):
            continue  # reported by missing_exports()
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args


def lib():
    """Load libacehip.so (raises if it is missing — no fallback path exists)."""
    global _LIB
    if _LIB is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(f"acehip: {LIB_PATH} not built; run `make -C ace-step-1.5_amd` "
                               "or __graft_entry__.build()")
        handle = ctypes.CDLL(LIB_PATH)
        _declare(handle)
        v = handle.acehip_get_version()
        if v != ABI_VERSION:
            raise RuntimeError(f"acehip: {LIB_PATH} has ABI version {v}, this binding expects "
                               f"{ABI_VERSION} (include/acehip.h); rebuild the library")
        built, tree = build_hash(handle), source_hash()
        if tree is not None and built != tree:
            raise RuntimeError(f"acehip: {LIB_PATH} has build hash {built}, the default build of the native "
                               f"sources beside it is {tree}: {_mismatch_cause(built)}; rebuild the library "
                               "(make -C ace-step-1.5_amd, no EXTRA)")
        _LIB = handle
    return _LIB


def build_hash(handle=None) -> str:
    """The build hash compiled into the library (acehip_build_hash): sources + compile flags."""
    h = handle if handle is not None else lib()
    if not hasattr(h, "acehip_build_hash"):
        return "none"
    h.acehip_build_hash.restype = c_char_p
    return h.acehip_build_hash().decode()


def _native_hash_module():
    """csrc/native_hash.py of the tree this package sits in (None if the sources are absent)."""
    script = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "csrc", "native_hash.py")
    if not os.path.exists(script):
        return None
    import importlib.util
    spec = importlib.util.spec_from_file_location("_acehip_native_hash", script)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def source_hash():
    """The build hash of the DEFAULT build (gfx950, no extra flags) of the tree this package sits in
    (None if the sources are absent, e.g. an installed wheel: then only the ABI version is checked)."""
    mod = _native_hash_module()
    return mod.native_hash() if mod is not None else None


def _mismatch_cause(built: str) -> str:
    """Why the library's hash is not the default build's: the flags the last `make` recorded
    (build/flags.stamp) if they explain it, else the sources."""
    mod = _native_hash_module()
    stamp = os.path.join(os.path.dirname(os.path.dirname(LIB_PATH)), "build", "flags.stamp")
    try:
        flags = dict(ln.split("=", 1) for ln in open(stamp).read().splitlines() if "=" in ln)
        arch, extra = flags["ARCH"], flags["EXTRA"]
    except (OSError, KeyError):
        arch = extra = None
    if arch is not None and mod.flags_text(arch, extra) != mod.flags_text() and mod.native_hash(arch=arch, extra=extra) == built:
        return f"it was built with non-default compile flags (ARCH={arch} EXTRA={extra!r})"
    return "it was built from other native sources or with non-default compile flags (ARCH / EXTRA)"


def missing_exports():
    l = lib()
    return [n for n in EXPORTS if not hasattr(l, n)]


def gemm_plan(M, N, K, epi, lda=None, ldw=None, ws_bytes=48 << 20, defer_ok=False, device_cus=0) -> dict:
    """The route the production GEMM dispatch takes for a shape under the current ACEHIP_* switches
    (acehip_diag_gemm_plan; host only), as a dict of acehip_gemm_plan's fields.  device_cus 0: the
    current device's; ws_bytes defaults to the runtimes' split-K workspace."""
    out = GemmPlan()
    check(lib().acehip_diag_gemm_plan(M, N, K, K if lda is None else lda, K if ldw is None else ldw, epi, ws_bytes,
                                      int(defer_ok), device_cus, ctypes.byref(out)), "diag_gemm_plan")
    return {n: getattr(out, n) for n, _ in GemmPlan._fields_}


def attn_plan(B, H, KV, Sq, Sk, window=-1, masked=False, have_ws=True, device_cus=0) -> dict:
    """The launch the attention dispatch gives a shape under the current ACEHIP_ATTN_* switches
    (acehip_diag_attn_plan; host only), as a dict of acehip_attn_plan's fields.  device_cus 0: the
    current device's; have_ws: the split workspace, which the standalone entries and the runtimes pass."""
    out = AttnPlan()
    check(lib().acehip_diag_attn_plan(B, H, KV, Sq, Sk, window, int(masked), int(have_ws), device_cus,
                                      ctypes.byref(out)), "diag_attn_plan")
    return {n: getattr(out, n) for n, _ in AttnPlan._fields_}


def attn_extend_plan(B, H, KV, n, pos, have_ws=True, device_cus=0) -> dict:
    """The launch acehip_attention_extend_bf16 gives a shape (acehip_diag_attn_extend_plan; host only), as a
    dict of acehip_attn_extend_plan's fields plus ws_need, the bytes of partials that plan writes."""
    out, need = AttnExtendPlan(), ctypes.c_size_t(0)
    check(lib().acehip_diag_attn_extend_plan(B, H, KV, n, pos, int(have_ws), device_cus, ctypes.byref(out),
                                             ctypes.byref(need)), "diag_attn_extend_plan")
    d = {n_: getattr(out, n_) for n_, _ in AttnExtendPlan._fields_}
    d["ws_need"] = need.value
    return d


def reload_knobs():
    """Re-read the ACEHIP_* A/B switches after changing the environment (tests / A/B tools)."""
    check(lib().acehip_reload_knobs(), "reload_knobs")


def check(rc: int, what: str = ""):
    if rc != 0:
        msg = lib().acehip_last_error()
        raise RuntimeError(f"acehip {what} failed ({rc}): {msg.decode() if msg else ''}")


def stream_ptr(stream=None):
    """HIP stream handle of a torch stream (current stream by default)."""
    import torch
    s = stream if stream is not None else torch.cuda.current_stream()
    return c_void_p(s.cuda_stream)


def dtype_code(t) -> int:
    """ACEHIP_F32 / ACEHIP_BF16 of a tensor (anything else is refused)."""
    import torch
    if t.dtype == torch.float32:
        return ACEHIP_F32
    if t.dtype == torch.bfloat16:
        return ACEHIP_BF16
    raise TypeError(f"acehip: unsupported dtype {t.dtype}")


def ptr(t):
    return c_void_p(t.data_ptr()) if t is not None else None


def shape_arg(shape):
    return (c_int64 * len(shape))(*shape)
