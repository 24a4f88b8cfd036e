#!/usr/bin/env python3
"""tools/codeobj_same.py PARENT.so NEW.so -- is the gfx950 code object of NEW the one of PARENT, kernel by kernel?

A refactor of the device code must leave the code object alone.  Byte identity of .text is reported, but is stricter than "the same
code": hoisting a block into a function can flip the sense of a compare-and-branch pair or renumber a few registers.  The criterion:
  * the same function symbols in the same order (by address), each of the same size;
  * the same kernel descriptor (the 64 bytes of NAME.kd: registers, scratch, LDS, ...), field names from tools/kres.py's metadata;
  * the same mnemonic histogram per function, where the two senses of a scalar compare (s_cmp_eq_* / s_cmp_lg_*) and of the branch on
    its result (s_cbranch_scc0 / s_cbranch_scc1) count as one.
One line per kernel that differs, and how; exit status 0 only when the criterion holds for every kernel."""
import collections
import hashlib
import os
import re
import shutil
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kres  # noqa: E402

LLVM = next((d for d in (os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")))), "llvm", "bin"), "/opt/rocm/llvm/bin",
                         os.path.dirname(shutil.which("llvm-objdump") or "")) if d and os.path.exists(os.path.join(d, "llvm-objdump"))), "")  # (beside hipcc, like tools/kres.py)
SAME_SENSE = ((re.compile(r"^s_cmp_(eq|lg)_"), "s_cmp_eq|lg_"), (re.compile(r"^s_cbranch_scc[01]$"), "s_cbranch_scc0|1"))


def tool(name, *args):
    return subprocess.run([os.path.join(LLVM, name)] + list(args), capture_output=True, text=True, check=True).stdout


class CodeObject:
    def __init__(self, lib, tmp, tag):
        fat, self.path = os.path.join(tmp, tag + ".fat"), os.path.join(tmp, tag + ".co")
        tool("llvm-objcopy", "--dump-section", ".hip_fatbin=" + fat, lib)
        tool("clang-offload-bundler", "--unbundle", "--type=o", "--input=" + fat, "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--output=" + self.path)
        self.sections = {}  # name -> (address, bytes)
        for m in re.finditer(r"^\s*\[\s*\d+\]\s+(\.\S+)\s+PROGBITS\s+([0-9a-f]+)\s+[0-9a-f]+\s+([0-9a-f]+)", tool("llvm-readelf", "-SW", self.path), re.M):
            if m.group(1) in (".text", ".rodata"):
                out = os.path.join(tmp, tag + m.group(1))
                tool("llvm-objcopy", "--dump-section", m.group(1) + "=" + out, self.path)
                self.sections[m.group(1)] = (int(m.group(2), 16), open(out, "rb").read())
        self.funcs, self.kd = [], {}  # [(address, size, name)] by address; kernel name -> descriptor bytes
        for m in re.finditer(r"^\s*\d+:\s+([0-9a-f]+)\s+(\d+)\s+(FUNC|OBJECT)\s+\S+\s+\S+\s+\d+\s+(\S+)$", tool("llvm-readelf", "-sW", "--dyn-syms", self.path), re.M):
            addr, size, name = int(m.group(1), 16), int(m.group(2)), m.group(4)
            if m.group(3) == "FUNC":
                self.funcs.append((addr, size, name))
            elif name.endswith(".kd"):
                base, data = self.sections[".rodata"]
                kd = data[addr - base:addr - base + size]
                self.kd[name[:-3]] = kd[:16] + kd[24:]  # (without kernel_code_entry_byte_offset: where the code lies is the symbol table's matter)
        self.funcs = sorted(set(self.funcs))
        self.text_sha = hashlib.sha256(self.sections[".text"][1]).hexdigest()
        self.meta = kres.library_kernels(lib)

    def histograms(self):
        """function name -> Counter of mnemonics (llvm-objdump's disassembly, `<name>:` labels)"""
        hist, cur = {}, None
        for line in tool("llvm-objdump", "-d", "--no-show-raw-insn", self.path).splitlines():
            m = re.match(r"^[0-9a-f]+ <(\S+)>:$", line)
            if m:
                cur = hist.setdefault(m.group(1), collections.Counter())
            elif cur is not None and line.startswith("\t") and line.strip() != "...":  # ("...": the disassembler's mark for a run of zero padding)
                op = line.split()[0]
                for rx, cls in SAME_SENSE:
                    if rx.match(op):
                        op = cls
                cur[op] += 1
        return hist


def main():
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    with tempfile.TemporaryDirectory() as tmp:
        a, b = CodeObject(sys.argv[1], tmp, "parent"), CodeObject(sys.argv[2], tmp, "new")
        bad = 0
        names_a, names_b = [f[2] for f in a.funcs], [f[2] for f in b.funcs]
        short = dict(zip(names_a + names_b, kres.demangle(names_a + names_b)))
        if names_a != names_b:
            bad += 1
            for n in [n for n in names_a if n not in set(names_b)]:
                print("%-72s only in the parent" % short[n][:72])
            for n in [n for n in names_b if n not in set(names_a)]:
                print("%-72s only in the new object" % short[n][:72])
            common = set(names_a) & set(names_b)
            if [n for n in names_a if n in common] != [n for n in names_b if n in common]:
                first = next(i for i, (x, y) in enumerate(zip(names_a, names_b)) if x != y)
                print("symbol order differs from position %d: %s / %s" % (first, short[names_a[first]][:60], short[names_b[first]][:60]))
        ha, hb = a.histograms(), b.histograms()
        size_a, size_b = {f[2]: f[1] for f in a.funcs}, {f[2]: f[1] for f in b.funcs}
        for n in names_a:
            if n not in size_b:
                continue
            how = []
            if size_a[n] != size_b[n]:
                how.append("size %d -> %d" % (size_a[n], size_b[n]))
            if a.kd.get(n) != b.kd.get(n):
                ma, mb = a.meta.get(short[n], {}), b.meta.get(short[n], {})
                how.append("descriptor (" + (", ".join("%s %s -> %s" % (k, ma.get(k), mb.get(k)) for k in sorted(set(ma) | set(mb)) if ma.get(k) != mb.get(k)) or "other bits") + ")")
            if ha.get(n) != hb.get(n):
                d = {op: hb[n][op] - ha[n][op] for op in set(ha[n]) | set(hb[n]) if ha[n][op] != hb[n][op]}
                how.append("mnemonics " + " ".join("%s%+d" % kv for kv in sorted(d.items())))
            if how:
                bad += 1
                print("%-72s %s" % (short[n][:72], "; ".join(how)))
        print("%d functions, %d kernel descriptors; .text %s (sha256 %s / %s); %s" % (
            len(names_b), len(b.kd), "byte-identical" if a.text_sha == b.text_sha else "differs in bytes", a.text_sha[:16], b.text_sha[:16],
            "the criterion holds" if not bad else "%d difference(s)" % bad))
        sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
