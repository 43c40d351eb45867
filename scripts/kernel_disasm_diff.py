"""Per-kernel comparison of the gfx950 instructions of two builds of one translation unit (no GPU needed):
    python scripts/kernel_disasm_diff.py <parent object file> <branch object file> [<pattern>=<replacement>]
The optional third argument is a regular-expression substitution applied to the parent's demangled kernel names before the kernels
are paired (for a branch that renames kernels, e.g. by dropping a template parameter).  Unbundles both code objects, disassembles them and compares kernel by kernel.  Two things differ between builds whose kernels are the
same and are left out of the comparison: the alignment padding after a kernel's last instruction, and the literal of the s_add_u32 that
follows an s_getpc_b64 (a pc-relative distance to another symbol of the code object, which moves when any other kernel changes size)."""
import difflib
import os
import re
import subprocess
import sys
import tempfile

LLVM = "/opt/rocm/lib/llvm/bin"


def kernels(obj):
    with tempfile.TemporaryDirectory() as d:
        fat, co = os.path.join(d, "fat.bin"), os.path.join(d, "k.co")
        subprocess.check_call([LLVM + "/llvm-objcopy", "--dump-section", ".hip_fatbin=" + fat, obj])
        subprocess.check_call([LLVM + "/clang-offload-bundler", "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--input=" + fat,
                               "--output=" + co, "--unbundle"])
        dis = subprocess.run([LLVM + "/llvm-objdump", "-d", "--no-show-raw-insn", "--no-leading-addr", co], capture_output=True, text=True,
                             check=True).stdout
    out, cur, after_getpc = {}, None, False
    for line in (ln.strip() for ln in dis.splitlines()):
        m = re.match(r"^[0-9a-f]* ?<(\S+)>:$", line)
        if m:
            cur = out.setdefault(m.group(1), [])
        elif cur is not None and line and line != "...":
            line = re.sub(r"\s*//.*", "", line)
            if after_getpc and line.startswith("s_add_u32"):
                line = re.sub(r"0x[0-9a-f]+$|-?\d+$", "<pc-relative>", line)
            after_getpc = line.startswith("s_getpc_b64")
            cur.append(line)
    return out


def demangled(ks, rename=None):
    names = subprocess.run(["c++filt"], input="\n".join(ks), capture_output=True, text=True).stdout.splitlines()
    return {re.sub(rename[0], rename[1], dn) if rename else dn: ks[n] for n, dn in zip(ks, names)}


def main():
    a = demangled(kernels(sys.argv[1]), sys.argv[3].split("=", 1) if len(sys.argv) > 3 else None)
    b = demangled(kernels(sys.argv[2]))
    for n in sorted(set(a) | set(b)):
        dn = re.sub(r"\(.*", "", n).replace("dmb::", "").replace("void ", "")
        if n not in a or n not in b:
            print("%-9s %6s   %6s   %s" % ("only in", "parent" if n in a else "", "branch" if n in b else "", dn))
            continue
        print("%-9s %6d / %6d instructions  %s" % ("identical" if a[n] == b[n] else "DIFFERENT", len(a[n]), len(b[n]), dn))
        if a[n] != b[n]:
            print("\n".join("    " + ln for ln in list(difflib.unified_diff(a[n], b[n], lineterm="", n=1))[:40]))


if __name__ == "__main__":
    main()
