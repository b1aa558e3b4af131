"""CPU-only checks: the C-ABI library loads and exports every symbol
include/acehip.h declares; argument errors surface as RuntimeError (no GPU
work is issued); host logic (schedules, song sharding) matches the reference;
the multi-rank path is covered by test_multirank.py."""
import ctypes
import os
import re

import pytest
import torch

from conftest import REPO


def test_header_symbols_exported():
    from acehip import _ffi
    hdr = open(os.path.join(REPO, "include", "acehip.h")).read()
    declared = set(re.findall(r"\b(acehip_[a-z0-9_]+)\s*\(", hdr))
    assert declared, "no declarations parsed"
    lib = _ffi.lib()
    missing = [s for s in sorted(declared) if not hasattr(lib, s)]
    assert not missing, missing
    assert set(_ffi.EXPORTS) == declared
    assert lib.acehip_get_version() == 400 == _ffi.ABI_VERSION


def test_library_built_from_this_tree(monkeypatch):
    """acehip_build_hash() = the native-source hash of the sources beside the library, and the
    binding refuses a library built from other sources (verdict r05 hygiene item)."""
    from acehip import _ffi
    lib = _ffi.lib()
    assert _ffi.build_hash(lib) == _ffi.source_hash()
    assert re.fullmatch(r"[0-9a-f]{16}", _ffi.build_hash(lib))
    monkeypatch.setattr(_ffi, "_LIB", None)
    monkeypatch.setattr(_ffi, "source_hash", lambda: "0" * 16)
    with pytest.raises(RuntimeError, match="native sources"):
        _ffi.lib()
    monkeypatch.undo()
    assert _ffi.lib() is lib


def _makefile_hash(tmp_path, *make_args):
    """The hash the Makefile would compile in: the -DACEHIP_BUILD_HASH of a dry run (nothing is
    built; the flags stamp goes to tmp_path, not into the tree)."""
    import subprocess
    pkg = os.path.join(REPO, "ace-step-1.5_amd")
    env = {k: v for k, v in os.environ.items() if k not in ("ARCH", "EXTRA", "MAKEFLAGS", "MFLAGS")}
    out = subprocess.run(["make", "-C", pkg, "-n", "-B", "build/buildhash.o", f"STAMP={tmp_path}/flags.stamp",
                          *make_args], check=True, capture_output=True, text=True, env=env).stdout
    hashes = re.findall(r"-DACEHIP_BUILD_HASH='\"([^\"]*)\"'", out)
    assert len(hashes) == 1, out
    return hashes[0]


def test_build_hash_covers_compile_flags(tmp_path):
    """The build hash covers the flags `make` received as well as the sources: a non-empty EXTRA
    (or another ARCH) gives another hash, which _ffi.lib() therefore refuses, and what the Makefile
    compiles in is native_hash() of the same flags (for the default build: _ffi.source_hash())."""
    from acehip import _ffi
    nh = _ffi._native_hash_module()
    default = _ffi.source_hash()
    assert default == nh.native_hash() == nh.native_hash(arch=nh.DEFAULT_ARCH, extra="")
    stamps = nh.native_hash(extra="-DGEMM_STAMPS")
    others = {stamps, nh.native_hash(extra="-DRU8_STAMPS"), nh.native_hash(extra="-O1"),
              nh.native_hash(arch="gfx942"), nh.native_hash(arch="gfx942", extra="-DGEMM_STAMPS")}
    assert len(others) == 5 and default not in others
    assert nh.native_hash(extra="  -DGEMM_STAMPS ") == stamps          # as make passes it on, unquoted
    for h in others | {default}:
        assert re.fullmatch(r"[0-9a-f]{16}", h)
    assert _makefile_hash(tmp_path) == default
    assert _makefile_hash(tmp_path, f"ARCH={nh.DEFAULT_ARCH}", "EXTRA=") == default
    assert _makefile_hash(tmp_path, "EXTRA=-DGEMM_STAMPS") == stamps


def test_flags_stamp_rewritten_only_on_change(tmp_path):
    """Every object depends on the flags stamp, so it must change when, and only when, the flags do."""
    from acehip import _ffi
    nh = _ffi._native_hash_module()
    stamp = tmp_path / "b" / "flags.stamp"
    nh.write_stamp(str(stamp), nh.flags_text())
    os.utime(stamp, ns=(1, 1))
    nh.write_stamp(str(stamp), nh.flags_text(nh.DEFAULT_ARCH, " "))
    assert stamp.stat().st_mtime_ns == 1
    nh.write_stamp(str(stamp), nh.flags_text(extra="-DGEMM_STAMPS"))
    assert stamp.stat().st_mtime_ns != 1 and stamp.read_text() == "ARCH=gfx950\nEXTRA=-DGEMM_STAMPS\n"


def test_error_paths_without_gpu():
    from acehip import _ffi
    lib = _ffi.lib()
    h = ctypes.c_void_p()
    rc = lib.acehip_dit_create(0, None, ctypes.byref(h))
    assert rc == -1 and b"null" in lib.acehip_last_error()
    cfg = _ffi.DiTCfg(hidden=2048, intermediate=6144, heads=16, kv_heads=8, head_dim=64, layers=24,
                      window=128, patch=2, in_channels=192, out_channels=64, eps=1e-6,
                      rope_theta=1e6, max_S=16, max_Bc=2, max_Lenc=16)
    rc = lib.acehip_dit_create(0, ctypes.byref(cfg), ctypes.byref(h))
    assert rc == -1 and b"head_dim" in lib.acehip_last_error()
    with pytest.raises(RuntimeError, match="head_dim"):
        _ffi.check(rc, "dit_create")
    assert lib.acehip_dit_forward(None, None, None, 1, None, None, 0, 2, 10, _ffi.ACEHIP_BF16, None, None) == -1
    assert lib.acehip_vae_decode(None, None, 1, 1, None, None) == -1


def test_product_has_no_oracle_import():
    """The product package must never import the CPU oracle (no CPU fallback)."""
    pkg = os.path.join(REPO, "ace-step-1.5_amd", "acehip")
    for f in os.listdir(pkg):
        if f.endswith(".py"):
            src = open(os.path.join(pkg, f)).read()
            assert "oracle" not in re.sub(r'""".*?"""', "", src, flags=re.S).replace("#", "\n#"), f


def test_turbo_schedule_host_logic():
    from acehip.dit import turbo_schedule
    from oracle.sampler_oracle import turbo_schedule_list
    for sh in (1.0, 2.0, 3.0, 2.6, 0.4):
        assert turbo_schedule(sh) == turbo_schedule_list(sh)
    ts = torch.tensor([0.97, 0.76, 0.5, 0.26, 0.0])
    assert turbo_schedule(3.0, ts) == turbo_schedule_list(3.0, ts)


def test_base_schedule_matches_oracle_cpu():
    from acehip.dit import base_schedule
    from oracle.sampler_oracle import base_schedule as ob
    for n, sh in ((27, 3.0), (60, 3.0), (8, 1.0)):
        assert torch.equal(base_schedule(n, sh, "cpu", torch.bfloat16), ob(n, sh, torch.bfloat16))


def test_song_assignment_partitions():
    from acehip.distributed import song_assignment
    for world in (1, 2, 4, 8):
        got = sorted(sum((song_assignment(16, r, world) for r in range(world)), []))
        assert got == list(range(16))


def test_lora_merge_state_dict():
    """§8f row 3: the LoRA re-pack hook merges PEFT-style adapted Linears
    (base_layer + get_delta_weight over the active adapters) into plain HF names."""
    import torch
    from acehip.integration import merged_decoder_state_dict

    class LoraLinear(torch.nn.Module):
        def __init__(self, base, r=2, scale=0.5):
            super().__init__()
            self.base_layer = base
            self.lora_A = torch.nn.ModuleDict({"v": torch.nn.Linear(base.in_features, r, bias=False)})
            self.lora_B = torch.nn.ModuleDict({"v": torch.nn.Linear(r, base.out_features, bias=False)})
            self.scaling = {"v": scale}
            self.active_adapters = ["v"]
            self.merged = False
            self.disable_adapters = False

        def get_delta_weight(self, a):
            return (self.lora_B[a].weight @ self.lora_A[a].weight) * self.scaling[a]

    class Attn(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.q_proj = LoraLinear(torch.nn.Linear(8, 8, bias=False))
            self.q_norm = torch.nn.LayerNorm(8)

    class Wrapped(torch.nn.Module):       # PeftModel naming: base_model.model.<decoder keys>
        def __init__(self):
            super().__init__()
            self.base_model = torch.nn.Module()
            self.base_model.model = torch.nn.Module()
            self.base_model.model.layers = torch.nn.ModuleList([torch.nn.Module()])
            self.base_model.model.layers[0].self_attn = Attn()

    m = Wrapped()
    sd = merged_decoder_state_dict(m)
    q = m.base_model.model.layers[0].self_attn.q_proj
    want = q.base_layer.weight + q.get_delta_weight("v")
    assert torch.allclose(sd["layers.0.self_attn.q_proj.weight"], want)
    assert "layers.0.self_attn.q_norm.weight" in sd
    assert not any("lora" in k or "base_layer" in k for k in sd)
    q.disable_adapters = True
    assert torch.equal(merged_decoder_state_dict(m)["layers.0.self_attn.q_proj.weight"], q.base_layer.weight)


def test_pw_kernel_agprs_stay_asm_owned(tmp_path):
    """attn_pw_kernel owns a[0:255] by number from inline asm (O, Q and the K fragments live
    there across the tile loop), so hipcc must never place a value of its own in an AGPR: a
    VGPR spill into AGPRs (the compiler's first choice once arch VGPRs run out) would be
    overwritten by the asm and corrupt addresses or results (seen once in round 3 as an
    illegal address).  Compile the kernel to gfx950 assembly and require that every
    v_accvgpr_read / v_accvgpr_write of the kernel body comes from an inline-asm block."""
    import shutil
    import subprocess
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    src = os.path.join(REPO, "ace-step-1.5_amd", "csrc", "attention.hip")
    out = tmp_path / "attention.s"
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "-S", src, "-o",
                    str(out)], check=True, capture_output=True)
    # the kernel body up to its .Lfunc_end label (early returns put several s_endpgm in one body)
    bodies, body, in_asm, compiler_agpr = {}, None, False, []
    for line in out.read_text().splitlines():
        mk = re.match(r"^(_ZN6acehip12_GLOBAL__N_114attn_pw_kernel\S*):", line)
        if mk:
            body = bodies.setdefault(mk.group(1), [])
            continue
        if body is None:
            continue
        if line.startswith(".Lfunc_end"):
            body = None
            continue
        body.append(line)
        if ";;#ASMSTART" in line:
            in_asm = True
        elif ";;#ASMEND" in line:
            in_asm = False
        elif not in_asm and re.search(r"v_accvgpr_(read|write)", line):
            compiler_agpr.append(line.strip())
    assert len(bodies) >= 1, f"attn_pw_kernel not found in the assembly: {list(bodies)}"
    assert not compiler_agpr, f"hipcc uses AGPRs in attn_pw_kernel: {compiler_agpr[:4]}"
    for name, b in bodies.items():
        assert not any("scratch_" in ln for ln in b), f"{name} spills to scratch"
