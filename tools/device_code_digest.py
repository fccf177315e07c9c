#!/usr/bin/env python3
"""Digest of the device code of csrc translation units, to show that a host-only change left
the kernels byte for byte as they were.

    tools/device_code_digest.py [--tree DIR] [--define NAME ...] [--out FILE.json]
                                [--union FILE.txt] [unit.hip ...]

Each unit (default: every unit of _build.py's SOURCES in DIR, default this checkout) is
compiled with _build.py's flags into a temporary directory; the object's .hip_fatbin section is
dumped (llvm-objcopy) and hashed, the gfx950 code object is unbundled from it
(clang-offload-bundler), and every function symbol and every kernel descriptor (<kernel>.kd) of
that ELF is listed with its size and the sha256 of its bytes. The tool only hashes: it reads no
instruction. Compare two trees with --out and `diff`, or read the section hashes. Two trees
whose unit lists differ (code moved between units) compare with --union: one sorted line
"name kind size sha256" per symbol over all units, without the unit, and a summary line that
counts the names found in more than one unit.

Two things make digests of two checkouts comparable. The compile adds -cuid=<unit name>: hipcc
otherwise derives the unit's id, a symbol name in the code object, from the source's path, so
the same source in two directories gives two sections. And a descriptor's hash leaves out its
kernel_code_entry_byte_offset (bytes 16-23), which is where the kernel lies in .text and not
code: templates are emitted in the order the host code first uses them, so moving host code
moves kernels. The section hash then differs while every symbol's does not.
"""
import argparse
import collections
from concurrent.futures import ThreadPoolExecutor
import hashlib
import json
import os
import struct
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"


def llvm_tool(name):
    for d in (os.environ.get("ROCM_PATH", "/opt/rocm") + "/llvm/bin", "/opt/rocm/llvm/bin"):
        if os.path.exists(os.path.join(d, name)):
            return os.path.join(d, name)
    return name


def build_flags(tree):
    sys.path.insert(0, tree)
    from deep_quantized_recommendation_model_dqrm_amd import _build

    return _build.hipcc(), list(_build.HIPCC_FLAGS), list(_build.SOURCES)


def elf_symbols(blob):
    """[(name, kind, size, sha256)] of an ELF64 little-endian code object: kind 'func' for
    STT_FUNC symbols, 'kd' for kernel descriptors."""
    assert blob[:4] == b"\x7fELF" and blob[4] == 2 and blob[5] == 1, "not an ELF64 LE object"
    shoff, = struct.unpack_from("<Q", blob, 0x28)
    shentsize, shnum, _ = struct.unpack_from("<HHH", blob, 0x3A)
    secs = [struct.unpack_from("<IIQQQQIIQQ", blob, shoff + i * shentsize) for i in range(shnum)]
    out = []
    for sh in secs:
        if sh[1] != 2:  # SHT_SYMTAB
            continue
        stroff = secs[sh[6]][4]
        for off in range(sh[4], sh[4] + sh[5], sh[9]):
            st_name, st_info, _, st_shndx, st_value, st_size = struct.unpack_from("<IBBHQQ", blob, off)
            name = blob[stroff + st_name: blob.index(b"\0", stroff + st_name)].decode()
            kind = "func" if (st_info & 15) == 2 else "kd" if name.endswith(".kd") else None
            if kind is None or st_shndx == 0 or st_shndx >= len(secs) or st_size == 0:
                continue
            sec = secs[st_shndx]
            start = sec[4] + (st_value - sec[3])
            data = blob[start:start + st_size]
            if kind == "kd":  # without kernel_code_entry_byte_offset
                data = data[:16] + bytes(8) + data[24:]
            out.append((name, kind, st_size, hashlib.sha256(data).hexdigest()))
    return sorted(out)


def digest_unit(src, tree, defines, tmp):
    hipcc, flags, _ = build_flags(tree)
    base = os.path.join(tmp, os.path.splitext(os.path.basename(src))[0])
    obj, fat, co = base + ".o", base + ".hip_fatbin", base + ".gfx950.co"
    cmd = [hipcc, *flags, "-cuid=" + os.path.basename(base), *["-D" + d for d in defines], "-I", os.path.join(tree, "include"), "-c", src, "-o", obj]
    subprocess.run(cmd, check=True, stderr=subprocess.DEVNULL)
    has_device = subprocess.run([llvm_tool("llvm-objcopy"), "--dump-section", ".hip_fatbin=" + fat, obj],
                                stderr=subprocess.DEVNULL).returncode == 0
    if not has_device:  # a unit without device code has no such section
        return {"unit": os.path.basename(src), "defines": defines, "section_bytes": 0, "section_sha256": None,
                "kernels": 0, "symbols": []}
    subprocess.run([llvm_tool("clang-offload-bundler"), "--unbundle", "--type=o", "--targets=" + TARGET,
                    "--input=" + fat, "--output=" + co], check=True)
    with open(fat, "rb") as f:
        section = f.read()
    with open(co, "rb") as f:
        syms = elf_symbols(f.read())
    return {"unit": os.path.basename(src), "defines": defines, "section_bytes": len(section),
            "section_sha256": hashlib.sha256(section).hexdigest(),
            "kernels": sum(1 for s in syms if s[1] == "kd"),
            "symbols": [{"name": n, "kind": k, "size": z, "sha256": h} for n, k, z, h in syms]}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--tree", default=os.path.dirname(HERE), help="checkout to digest (default: this one)")
    ap.add_argument("--define", action="append", default=[], help="extra -D (e.g. DQRM_DIAG_CLOCK)")
    ap.add_argument("--out", help="write the full digest (every symbol) as JSON")
    ap.add_argument("--union", help="write one 'name kind size sha256' line per symbol over all units")
    ap.add_argument("units", nargs="*")
    a = ap.parse_args()
    tree = os.path.abspath(a.tree)
    units = [os.path.abspath(u) for u in a.units] or build_flags(tree)[2]
    with tempfile.TemporaryDirectory() as tmp, ThreadPoolExecutor(min(8, os.cpu_count() or 1)) as pool:
        res = list(pool.map(lambda u: digest_unit(u, tree, a.define, tmp), units))
    for r in res:
        allsyms = hashlib.sha256(json.dumps(r["symbols"], sort_keys=True).encode()).hexdigest()
        print(f"{r['unit']}: .hip_fatbin {r['section_bytes']} bytes sha256 {r['section_sha256']}; "
              f"{r['kernels']} kernels, {len(r['symbols'])} symbols, digest of all (name, size, sha256) {allsyms}")
    union = sorted((s["name"], s["kind"], s["size"], s["sha256"]) for r in res for s in r["symbols"])
    seen = collections.Counter(u[0] for u in union)
    dup = sorted(n for n, c in seen.items() if c > 1)
    usum = hashlib.sha256(json.dumps(union).encode()).hexdigest()
    print(f"union of {len(res)} units: {sum(r['kernels'] for r in res)} kernels, {len(union)} symbols, "
          f"{len(dup)} names in more than one unit, digest of all (name, kind, size, sha256) {usum}")
    for n in dup:
        print(f"  in more than one unit: {n}")
    if a.union:
        with open(a.union, "w") as f:
            f.writelines(f"{n} {k} {z} {h}\n" for n, k, z, h in union)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
