#!/usr/bin/env python3
"""Build hash of libacehip.so: the native sources (csrc/*.hip, csrc/*.h, include/*.h), the Makefile
that compiles them and the flags `make` received (ARCH, EXTRA).  The Makefile compiles it into the
library (acehip_build_hash) and acehip._ffi refuses a library whose hash differs from that of the
DEFAULT build of the tree it is loaded from, so the binary on the GPU box is provably built from
these sources and without extra flags (a diagnostic build such as EXTRA=-DGEMM_STAMPS is refused).

usage: native_hash.py [--arch=A] [--extra="FLAGS"] [--stamp=FILE] | --default-arch
--stamp FILE also records the flags in FILE, rewritten only when they change: every object depends
on it, so a change of flags rebuilds them all."""
import argparse
import glob
import hashlib
import os
import sys

PKG = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))   # ace-step-1.5_amd/
ROOT = os.path.dirname(PKG)
# the default build (the Makefile takes its ARCH default from here; its EXTRA default is empty)
DEFAULT_ARCH = "gfx950"
DEFAULT_EXTRA = ""


def flags_text(arch: str = DEFAULT_ARCH, extra: str = DEFAULT_EXTRA) -> str:
    """The flags as hashed and as written to the stamp file (whitespace in EXTRA normalised)."""
    return f"ARCH={arch.strip()}\nEXTRA={' '.join(extra.split())}\n"


def native_hash(pkg: str = PKG, arch: str = DEFAULT_ARCH, extra: str = DEFAULT_EXTRA) -> str:
    root = os.path.dirname(pkg)
    files = sorted(glob.glob(os.path.join(pkg, "csrc", "*.hip")) + glob.glob(os.path.join(pkg, "csrc", "*.h")) +
                   glob.glob(os.path.join(root, "include", "*.h")) + glob.glob(os.path.join(pkg, "Makefile")))
    h = hashlib.sha256()
    for f in files:
        rel = os.path.relpath(f, root).replace(os.sep, "/")
        rel = rel.split("/", 1)[1] if rel.startswith(os.path.basename(pkg) + "/") else rel
        h.update(rel.encode())
        with open(f, "rb") as fh:
            h.update(fh.read())
    h.update(b"\0flags\0" + flags_text(arch, extra).encode())
    return h.hexdigest()[:16]


def write_stamp(path: str, text: str) -> None:
    try:
        with open(path) as fh:
            if fh.read() == text:
                return
    except OSError:
        pass
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as fh:
        fh.write(text)


if __name__ == "__main__":
    p = argparse.ArgumentParser()
    p.add_argument("--arch", default=DEFAULT_ARCH)
    p.add_argument("--extra", default=DEFAULT_EXTRA)
    p.add_argument("--stamp")
    p.add_argument("--default-arch", action="store_true")
    a = p.parse_args()
    if a.default_arch:
        sys.stdout.write(DEFAULT_ARCH)
    else:
        if a.stamp:
            write_stamp(a.stamp, flags_text(a.arch, a.extra))
        sys.stdout.write(native_hash(arch=a.arch, extra=a.extra))
