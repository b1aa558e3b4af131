"""CPU-only checks of the lyric-alignment layer: config remapping and ordering, argument
validation, and the new C-ABI names (declared in include/acehip.h, exported by the library,
listed in ``_ffi.EXPORTS`` with argtypes).  No GPU work is issued."""
import ctypes
import json
import os
import re

import pytest
import torch

from conftest import GOLDEN, REPO

NEW_SYMBOLS = ("acehip_attention_probs_bf16", "acehip_dit_forward_capture")


def test_compact_config_order_and_remap():
    from acehip.alignment import compact_config
    from acehip.dit import config_pairs
    cfg = {5: [8, 9], 2: [6], 3: [10, 11, 1]}                    # dict order is not sorted, lists ragged
    kept, remapped = compact_config(cfg)
    assert kept == cfg and list(kept) == [5, 2, 3]
    assert remapped == {0: [0, 1], 1: [0], 2: [0, 1, 2]} and list(remapped) == [0, 1, 2]
    assert config_pairs(kept) == [(5, 8), (5, 9), (2, 6), (3, 10), (3, 11), (3, 1)]
    # the reference's default selection (acestep/handler.py:129): 7 pairs over layers 2..6
    default = {2: [6], 3: [10, 11], 4: [3], 5: [8, 9], 6: [8]}
    kept, remapped = compact_config(default, 24, 16)
    assert kept == default and len(config_pairs(kept)) == 7 and max(len(v) for v in remapped.values()) == 2
    # pairs outside the model are skipped as the aligners skip them; an emptied layer disappears
    kept, remapped = compact_config({30: [1], 4: [3, 16], 1: [0]}, 24, 16)
    assert kept == {4: [3], 1: [0]} and remapped == {0: [0], 1: [0]}
    assert compact_config({}, 24, 16) == ({}, {})
    assert compact_config({"3": ["2"]})[0] == {3: [2]}           # JSON-style keys


def test_compact_maps_padding_slots():
    from acehip.alignment import compact_config, compact_maps
    cfg = {5: [8, 9], 2: [6], 3: [10, 11, 1]}
    kept, remapped = compact_config(cfg)
    maps = torch.arange(1, 7, dtype=torch.float32).reshape(6, 1, 1).expand(6, 4, 5).contiguous()
    m = compact_maps(maps, kept)
    assert tuple(m.shape) == (3, 3, 4, 5) and m.dtype == torch.float32
    # what an aligner reads through the remapped config is the flat order; padding is zero
    read = [float(m[l, h, 0, 0]) for l, hs in remapped.items() for h in hs]
    assert read == [1.0, 2.0, 3.0, 4.0, 5.0, 6.0]
    assert not m[0, 2].any() and not m[1, 1:].any()
    with pytest.raises(ValueError):
        compact_maps(maps[:5], kept)
    with pytest.raises(ValueError):
        compact_maps(maps[0], kept)


def test_config_validation():
    from acehip.alignment import compact_config
    from acehip.dit import config_pairs
    with pytest.raises(TypeError):
        compact_config([(1, 2)])
    with pytest.raises(ValueError):
        compact_config({-1: [0]})
    with pytest.raises(ValueError):
        compact_config({1: [-2]})
    with pytest.raises(ValueError):
        compact_config({1: [0], "1": [2]})
    with pytest.raises(ValueError):
        config_pairs({})
    with pytest.raises(ValueError):
        config_pairs({3: []})


def test_new_abi_names_declared_exported_listed():
    from acehip import _ffi
    hdr = open(os.path.join(REPO, "include", "acehip.h")).read()
    lib = _ffi.lib()
    for name in NEW_SYMBOLS:
        assert re.search(r"\bint\s+" + name + r"\s*\(", hdr), name + " not declared"
        assert name in _ffi.EXPORTS
        fn = getattr(lib, name)
        assert fn.restype is ctypes.c_int and fn.argtypes, name + " has no argtypes"
    assert "typedef struct acehip_attn_capture" in hdr
    assert [f[0] for f in _ffi.AttnCapture._fields_] == ["n", "layer", "head", "k0", "k1", "out", "stop_after_last"]
    assert len(lib.acehip_dit_forward_capture.argtypes) == 13 and len(lib.acehip_attention_probs_bf16.argtypes) == 14
    assert lib.acehip_get_version() == 400


def test_abi_null_arguments_refused_without_gpu():
    from acehip import _ffi
    lib = _ffi.lib()
    assert lib.acehip_dit_forward_capture(None, None, None, 1, None, None, 0, 1, 10, _ffi.ACEHIP_BF16, None, None,
                                          None) == -1
    assert b"null" in lib.acehip_last_error()
    heads = (ctypes.c_int * 1)(0)
    assert lib.acehip_attention_probs_bf16(None, None, 1, 2, 1, 4, 4, heads, 1, 0, 4, 1.0, None, None) == -1
    assert b"null" in lib.acehip_last_error()


def test_install_signature_and_fixture_manifest():
    import inspect
    from acehip.integration import install
    p = inspect.signature(install).parameters
    assert p["lyric_alignment"].default is True
    with open(os.path.join(GOLDEN, "lyric_attn_manifest.json")) as f:
        meta = json.load(f)
    assert (meta["B"], meta["T"], meta["Lenc"], meta["k0"], meta["k1"]) == (2, 250, 77, 5, 61)
    assert meta["layers_config"] == {"1": [3, 10], "2": [0], "3": [15, 8]} and meta["t"] == [1.0, 0.125]
    for tag, fx in meta["fixtures"].items():
        # far from the uniform 1/Lenc map: a kernel writing a constant cannot pass the GPU test
        assert fx["contrast_rel_l2_vs_uniform"] >= meta["min_contrast"] >= 0.25
        assert os.path.getsize(os.path.join(GOLDEN, f"lyric_attn_{tag}.safetensors")) < (1 << 20)
