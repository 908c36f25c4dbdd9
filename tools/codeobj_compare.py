#!/usr/bin/env python3
"""Are the gfx950 kernels of two builds of the library the same device code?  Unbundles the code objects of both (llvm-objdump --offloading,
as tests/test_abi.py does) and compares, per kernel symbol, the metadata note (VGPR / SGPR / AGPR counts, LDS and private segment sizes,
spill counts, ...) and the disassembled instruction stream (mnemonics, operands, encodings; addresses and address comments stripped).
Needs no GPU.  Prints one JSON line: the kernel count and every difference; exit status 1 when there is one.
Usage: python tools/codeobj_compare.py OLD/libadafocus_hip.so NEW/libadafocus_hip.so"""
import glob
import hashlib
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile

LLVM = "/opt/rocm/lib/llvm/bin/"


def kernels(lib_path):
    """{kernel symbol: (metadata note text, sha256 of its instruction stream)} over every gfx950 code object of the library."""
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        shutil.copy(lib_path, os.path.join(tmp, "lib.so"))
        subprocess.run([LLVM + "llvm-objdump", "--offloading", "lib.so"], cwd=tmp, check=True, capture_output=True)
        cos = sorted(glob.glob(os.path.join(tmp, "lib.so.*gfx950*")))
        assert cos, os.listdir(tmp)
        for co in cos:
            notes = subprocess.run([LLVM + "llvm-readelf", "--notes", co], check=True, capture_output=True, text=True).stdout
            meta = {}
            for k in re.split(r"\n\s+- (?=\.agpr_count:)", notes)[1:]:
                k = re.split(r"\n\s*amdhsa\.", k)[0]
                meta[re.search(r"\.name:\s+(\S+)", k).group(1)] = "\n".join(sorted(ln.strip() for ln in k.splitlines()))
            dis = subprocess.run([LLVM + "llvm-objdump", "-d", co], check=True, capture_output=True, text=True).stdout
            cur, h = None, None
            for line in dis.splitlines():
                m = re.match(r"^[0-9a-f]+ <(\S+)>:", line)
                if m:
                    cur, h = m.group(1), hashlib.sha256()
                    if cur in meta:
                        out[cur] = (meta[cur], h)
                elif cur in meta and line.strip() not in ("", "..."):      # ("...": zero padding up to the next symbol's alignment)
                    # "\ts_load_dwordx2 s[0:1], ...   // 000000001900: C0060002 00000000"  ->  text + encoding, no address
                    ins, _, enc = line.partition("//")
                    h.update((ins.strip() + " | " + enc.split(":", 1)[-1].split("<")[0].strip() + "\n").encode())
            assert set(meta) <= set(out), sorted(set(meta) - set(out))[:3]
    return {k: (m, h.hexdigest()) for k, (m, h) in out.items()}


def main():
    old, new = kernels(sys.argv[1]), kernels(sys.argv[2])
    diff = {"only_old": sorted(set(old) - set(new)), "only_new": sorted(set(new) - set(old)),
            "metadata": sorted(k for k in old if k in new and old[k][0] != new[k][0]),
            "instructions": sorted(k for k in old if k in new and old[k][1] != new[k][1])}
    print(json.dumps(dict(kernels_old=len(old), kernels_new=len(new), **diff)))
    return 1 if any(diff.values()) else 0


if __name__ == "__main__":
    sys.exit(main())
