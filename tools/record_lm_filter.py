#!/usr/bin/env python3
"""Record the reference's own top-k / top-p logit filters (this container only; the reference
never travels and this tool is not run on the GPU machine).

Loads ``acestep.llm_inference`` from the reference tree with a ``loguru`` stub and calls
``LLMHandler._apply_top_k_filter(None, x, k)`` / ``_apply_top_p_filter(None, x, p)``
(``acestep/llm_inference.py:367-385``; neither touches ``self``) on CPU rows of V = 4099, fp32
and bf16.  Writes ``tests/golden/lm_filter.safetensors`` — per dtype the input rows and, per
case, the reference's filtered rows — and ``tests/golden/lm_filter_manifest.json`` listing the
cases and the seed of every row.

Rows (one per line of ROWS): randn·σ with σ = 4 and σ = 8, a σ = 4 row with 3000 entries
pre-masked to −inf, and a row with a single finite entry.  Cases: top_k 1, 50, 4098 and
top_p 0.9, 0.5, 0.05.  A row's seed is admitted only if the row is *gapped*
(tests/lm_filter_ref.py) at all three top_p values in its dtype: no fp64 prefix mass within
DELTA of top_p, and the last kept value above the first removed one — asserted again on what is
written, so the fixture never depends on the reference's order among equal values.
"""
from __future__ import annotations

import importlib.util
import json
import os
import sys
import types

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tests"))
import lm_filter_ref as R  # noqa: E402

GOLDEN = os.path.join(REPO, "tests", "golden")
OUT = os.path.join(GOLDEN, "lm_filter.safetensors")
MANIFEST = os.path.join(GOLDEN, "lm_filter_manifest.json")
REF_ROOT = "/root/reference"
V = 4099
TOP_K = (1, 50, 4098)
TOP_P = (0.9, 0.5, 0.05)
ROWS = (("sigma4", 4.0, 0), ("sigma8", 8.0, 0), ("sigma4_masked3000", 4.0, 3000), ("single_finite", 4.0, V - 1))
DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16}


def _load_handler():
    if "loguru" not in sys.modules:
        m = types.ModuleType("loguru")

        class _L:
            def __getattr__(self, name):
                return lambda *a, **k: None
        m.logger = _L()
        sys.modules["loguru"] = m
    if REF_ROOT not in sys.path:
        sys.path.insert(0, REF_ROOT)
    spec = importlib.util.spec_from_file_location("_ref_llm_inference",
                                                  os.path.join(REF_ROOT, "acestep", "llm_inference.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.LLMHandler


def _admit(sigma, masked, dtype):
    for seed in range(100000):
        row = R.scattered_row(V, sigma, seed, masked, dtype)
        if all(R.gapped(row, p) for p in TOP_P):
            return seed, row
    raise RuntimeError("no gapped row found")


def main():
    H = _load_handler()
    tensors, manifest = {}, {"reference": "acestep/llm_inference.py:367-385", "generator": "tools/record_lm_filter.py",
                             "V": V, "delta": R.DELTA, "rows": [r[0] for r in ROWS], "dtypes": {}, "cases": []}
    for k in TOP_K:
        manifest["cases"].append({"name": f"top_k_{k}", "top_k": k, "top_p": None})
    for p in TOP_P:
        manifest["cases"].append({"name": f"top_p_{p}", "top_k": None, "top_p": p})
    for tag, dt in DTYPES.items():
        seeds, rows = [], []
        for name, sigma, masked in ROWS:
            seed, row = _admit(sigma, masked, dt)
            seeds.append(seed)
            rows.append(row)
        x = torch.stack(rows)
        tensors[f"{tag}.input"] = x
        manifest["dtypes"][tag] = {"seeds": seeds, "finite": [R.kept_count(r) for r in rows], "kept": {}}
        for case in manifest["cases"]:
            y = x.clone()
            if case["top_k"] is not None:
                got = H._apply_top_k_filter(None, y, case["top_k"])
            else:
                got = H._apply_top_p_filter(None, y, case["top_p"])
                for i, r in enumerate(rows):
                    assert R.gapped(r, case["top_p"]), (tag, case, i)
                    assert torch.equal(torch.isfinite(got[i].float()), R.mask64(r, case["top_p"])), (tag, case, i)
            assert got is y and got.dtype == dt
            tensors[f"{tag}.{case['name']}"] = got
            manifest["dtypes"][tag]["kept"][case["name"]] = [R.kept_count(r) for r in got]
    from safetensors.torch import save_file
    os.makedirs(GOLDEN, exist_ok=True)
    save_file({k: v.contiguous() for k, v in tensors.items()}, OUT)
    assert os.path.getsize(OUT) < 1000000, os.path.getsize(OUT)
    with open(MANIFEST, "w") as f:
        json.dump(manifest, f, indent=1)
    print("wrote", OUT, os.path.getsize(OUT), "bytes;", MANIFEST)


if __name__ == "__main__":
    main()
