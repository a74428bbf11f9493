"""Per-kernel instruction diff of the gfx950 code objects bundled in two host objects of the same translation unit:
    python tools/kernel_disdiff.py OLD.o NEW.o [NAME-PART [LINES]]
The way to check that a change left the existing kernels alone: compile the translation unit of the parent commit and
of the working tree with the Makefile's flags, then compare.  The device code is taken out of each object's .hip_fatbin section
(llvm-objcopy, clang-offload-bundler), disassembled (llvm-objdump -d) and split at the kernel symbols; addresses and branch-target
labels are dropped, names are demangled (c++filt).  Template arguments that the NEW side added with a default -- `false`, and an
empty parameter pack, at the end of beam_xl_scan's and beam_xl_finish's lists; an empty pack prints as nothing -- are dropped from
its names, so a kernel whose instantiation got a longer name is compared with the kernel it was.
Prints DIFFERS / GONE / NEW lines and the count of identical kernels; with NAME-PART, a unified diff of the kernels whose name
contains it.  Exit status 1 when a kernel both objects have differs or one is gone."""
import difflib
import os
import re
import subprocess
import sys
import tempfile

LLVM = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin")
TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"


def kernels(obj):
    d = tempfile.mkdtemp()
    fb, co = os.path.join(d, "fat.bin"), os.path.join(d, "dev.co")
    subprocess.check_call([f"{LLVM}/llvm-objcopy", "-O", "binary", "--only-section=.hip_fatbin", obj, fb])
    subprocess.check_call([f"{LLVM}/clang-offload-bundler", "--unbundle", "--type=o", f"--input={fb}", f"--targets={TARGET}", f"--output={co}"])
    txt = subprocess.check_output([f"{LLVM}/llvm-objdump", "-d", "--no-show-raw-insn", co], text=True)
    out, name = {}, None
    for line in txt.splitlines():
        m = re.match(r"^[0-9a-f]+ <(.+)>:$", line)
        if m:
            name = m.group(1)
            out[name] = []
            continue
        if name is None or not line.strip():
            continue
        ins = line.split("//")[0].strip()          # the address comment
        ins = re.sub(r"<[^>]+>", "<L>", ins)        # branch-target labels carry addresses
        out[name].append(re.sub(r"^[0-9a-f]+:\s*", "", ins))
    return out


def canon(names, strip):
    dm = subprocess.check_output(["c++filt"], input="\n".join(names), text=True).splitlines()
    out = {}
    for n, d in zip(names, dm):
        if strip:
            d = re.sub(r"^(void w2l::beam_xl_scan<[^>]*?, (?:true|false)), false>\(", r"\1>(", d)
            d = re.sub(r"^(void w2l::beam_xl_finish<(?:true|false)), false>\(", r"\1>(", d)
        out[n] = d
    return out


if __name__ == "__main__":
    a, b = kernels(sys.argv[1]), kernels(sys.argv[2])
    ca, cb = canon(list(a), False), canon(list(b), True)
    a = {ca[k]: v for k, v in a.items()}
    b = {cb[k]: v for k, v in b.items()}
    same = diff = gone = 0
    for k in sorted(a):
        if k not in b:
            gone += 1
            print("GONE   ", k)
        elif a[k] == b[k]:
            same += 1
        else:
            diff += 1
            print("DIFFERS", k, len(a[k]), len(b[k]))
    new = [k for k in sorted(b) if k not in a]
    for k in new:
        print("NEW    ", k, len(b[k]))
    print(f"{same} kernels identical, {diff} differ, {gone} gone, {len(new)} new")
    if len(sys.argv) > 3:
        for k in sorted(a):
            if sys.argv[3] in k and k in b:
                print(k)
                for line in list(difflib.unified_diff(a[k], b[k], lineterm="", n=1))[:int(sys.argv[4]) if len(sys.argv) > 4 else 60]:
                    print(line)
    sys.exit(1 if diff or gone else 0)
