#!/usr/bin/env python3
"""tools/kres.py [extra hipcc flags] -- registers, scratch, LDS and occupancy of every kernel of libptrs_hip (hipcc's kernel-resource-usage remarks).
tools/kres.py --lib [PATH] -- the same from the kernel metadata of a built library (no occupancy remark there).

`occ` is the compiler's figure (waves per SIMD by registers and by LDS counted to the byte); `wgs_lds` beside it is the workgroups per CU
by LDS alone when every workgroup's LDS is rounded up to the allocation granule, as the hardware hands it out (the granule measured by
tools/lds_residency.hip, profiles/lds_residency.json; 8 = the wave slots, LDS does not bind).  A workgroup of these kernels is one wave
per SIMD, so the two compare directly."""
import json
import os
import re
import shutil
import struct
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LDS_PER_CU = 163840


def granule():
    try:
        return int(json.load(open(os.path.join(ROOT, "profiles", "lds_residency.json")))["granule"])
    except (OSError, ValueError, KeyError):
        return 1280  # LLVM's figure for parts with 160 KB of LDS


def wgs_by_lds(lds, g):
    return min(8, LDS_PER_CU // (-(-lds // g) * g)) if lds else 8


def demangle(names):
    out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.splitlines()
    return [re.sub(r"\(.*", "", n.replace("(anonymous namespace)::", "").replace("void ", "")) for n in out]


def library_kernels(path, hipcc="/opt/rocm/bin/hipcc"):
    """{demangled kernel name: {v, a, s, scr, lds}} from the AMDGPU metadata note of the gfx950 code object bundled into a built library."""
    blob = open(path, "rb").read()
    i = blob.find(b"__CLANG_OFFLOAD_BUNDLE__")
    if i < 0:
        raise RuntimeError("%s: no offload bundle" % path)
    n, p, co = struct.unpack_from("<Q", blob, i + 24)[0], i + 32, None
    for _ in range(n):
        off, size, ln = struct.unpack_from("<QQQ", blob, p)
        tid = blob[p + 24:p + 24 + ln].decode()
        p += 24 + ln
        if "gfx950" in tid:
            co = blob[i + off:i + off + size]
    if co is None:
        raise RuntimeError("%s: no gfx950 code object" % path)
    readelf = next((r for r in (os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(hipcc))), "llvm", "bin", "llvm-readelf"), "/opt/rocm/llvm/bin/llvm-readelf",
                                shutil.which("llvm-readelf") or "") if r and os.path.exists(r)), None)
    if readelf is None:
        raise RuntimeError("llvm-readelf not found")
    with tempfile.NamedTemporaryFile(suffix=".co") as f:
        f.write(co); f.flush()
        notes = subprocess.run([readelf, "--notes", f.name], capture_output=True, text=True, check=True).stdout
    keys = ((".vgpr_count", "v"), (".agpr_count", "a"), (".sgpr_count", "s"), (".private_segment_fixed_size", "scr"), (".group_segment_fixed_size", "lds"))
    recs = []
    for rec in re.split(r"\n  - ", notes.split("amdhsa.kernels:", 1)[1].split("\namdhsa.", 1)[0])[1:]:
        m = re.search(r"^\s*\.name:\s+(\S+)", rec, re.M)
        if m:
            recs.append((m.group(1), {short: int(re.search(r"^\s*" + re.escape(k) + r":\s+(\d+)", rec, re.M).group(1)) for k, short in keys}))
    return dict(zip(demangle([r[0] for r in recs]), [r[1] for r in recs]))


def remark_kernels(text):
    cur, d = None, {}
    for l in text.splitlines():
        m = re.search(r"Function Name: (\S+)", l)
        if m:
            cur = m.group(1); d[cur] = {}
        for k, short in (("VGPRs:", "v"), ("AGPRs:", "a"), ("TotalSGPRs:", "s"), ("ScratchSize [bytes/lane]:", "scr"), ("Occupancy [waves/SIMD]:", "occ"), ("LDS Size [bytes/block]:", "lds"), ("VGPRs Spill:", "vspill"), ("SGPRs Spill:", "sspill")):
            m = re.search(r"remark:\s+" + re.escape(k) + r" (\d+)", l)
            if m and cur:
                d[cur][short] = int(m.group(1))
    return dict(zip(demangle(list(d)), d.values()))


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    import importlib
    b = importlib.import_module("pathtracer-rs_amd.build")
    g = granule()
    if "--lib" in sys.argv:
        k = sys.argv.index("--lib")
        kernels = library_kernels(sys.argv[k + 1] if len(sys.argv) > k + 1 else b.LIB, b.HIPCC)
    elif "--from" in sys.argv:
        kernels = remark_kernels(open(sys.argv.pop(sys.argv.index("--from") + 1)).read())
    else:
        cmd = [b.HIPCC] + b.FLAGS + sys.argv[1:] + ["-Rpass-analysis=kernel-resource-usage", "-o", "/tmp/kres.so", os.path.join(b.CSRC, "ptrs_hip.hip")]
        kernels = remark_kernels(subprocess.run(cmd, capture_output=True, text=True).stderr)
    for n in sorted(kernels):
        items = []
        for key, val in kernels[n].items():
            items.append((key, val))
            if key == "occ":
                items.append(("wgs_lds", wgs_by_lds(kernels[n].get("lds", 0), g)))
        if "occ" not in kernels[n]:
            items.append(("wgs_lds", wgs_by_lds(kernels[n].get("lds", 0), g)))
        print("%-64s %s" % (n[:64], " ".join("%s=%d" % kv for kv in items)))
