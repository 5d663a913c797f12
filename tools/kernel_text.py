#!/usr/bin/env python
"""
The text of every gfx950 kernel in object files or in the library, one file per kernel symbol: mnemonics and operands only
(no addresses, no encodings; a branch's target as an offset from the kernel's start), so that two trees built with the same
flags can be compared kernel by kernel:

    python tools/kernel_text.py OUT_DIR magphase_amd/_obj/magphase_comp.hip.std.o [more objects or libmagphase_hip.so]
    diff -r OUT_DIR_OF_THE_PARENT OUT_DIR

Steps, as by hand: llvm-objcopy dumps the .hip_fatbin section (in a linked library: one offload bundle per translation
unit, back to back), clang-offload-bundler unbundles the hipv4-amdgcn-amd-amdhsa--gfx950 entry of each, llvm-objdump
disassembles it.  A kernel is a function with a kernel descriptor (symbol NAME.kd).  Needs no GPU.
"""
import os
import re
import shutil
import subprocess
import sys
import tempfile

TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"
MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"


def llvm_tool(name):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    rocm = os.path.dirname(os.path.dirname(os.path.realpath(hipcc)))
    for d in (os.path.join(rocm, "lib", "llvm", "bin"), os.path.join(rocm, "llvm", "bin")):
        if os.path.isfile(os.path.join(d, name)):
            return os.path.join(d, name)
    return shutil.which(name) or sys.exit("kernel_text: %s not found" % name)


def code_objects(path, tmp):
    """The gfx950 code objects of `path`, as files under tmp."""
    fat = os.path.join(tmp, "fatbin")
    subprocess.check_call([llvm_tool("llvm-objcopy"), "-O", "binary", "--only-section=.hip_fatbin", path, fat])
    data = open(fat, "rb").read()
    starts = [m.start() for m in re.finditer(re.escape(MAGIC), data)]
    if not starts:
        sys.exit("kernel_text: no offload bundle in %s" % path)
    for i, (a, b) in enumerate(zip(starts, starts[1:] + [len(data)])):
        bundle, co = os.path.join(tmp, "bundle%d" % i), os.path.join(tmp, "co%d" % i)
        open(bundle, "wb").write(data[a:b])
        subprocess.check_call([llvm_tool("clang-offload-bundler"), "--unbundle", "--type=o", "--input=" + bundle,
                               "--targets=" + TARGET, "--output=" + co])
        yield co


def kernels(co):
    """{symbol: text} of the kernels of one code object."""
    objdump = llvm_tool("llvm-objdump")
    syms = subprocess.run([objdump, "-t", co], check=True, capture_output=True, text=True).stdout
    names = {ln.split()[-1][:-3] for ln in syms.splitlines() if ln.endswith(".kd")}
    size = {ln.split()[-1]: int(ln.split()[-3], 16) for ln in syms.splitlines() if " F .text" in ln}
    out, cur, end = {}, None, 0
    for ln in subprocess.run([objdump, "-d", co], check=True, capture_output=True, text=True).stdout.splitlines():
        m = re.match(r"([0-9a-f]+) <(.+)>:$", ln)
        if m:
            cur = out.setdefault(m.group(2), []) if m.group(2) in names else None
            end = int(m.group(1), 16) + size.get(m.group(2), 0)   # what follows is padding up to the next function
        elif cur is not None and "//" in ln:
            ins, _, note = ln.partition("//")                     # "<instruction>  // <address>: <encoding> [<kernel+0x14c>]"
            if int(note.split(":")[0], 16) >= end:
                continue
            tgt = re.search(r"<.+\+(0x[0-9a-f]+)>\s*$", note)     # a branch's target
            cur.append(" ".join(ins.split()) + ("   -> +" + tgt.group(1) if tgt else ""))
    return {k: "\n".join(v) + "\n" for k, v in out.items()}


def main(out_dir, inputs):
    found = {}
    for path in inputs:
        with tempfile.TemporaryDirectory() as tmp:
            for co in code_objects(path, tmp):
                for name, text in kernels(co).items():
                    if found.setdefault(name, text) != text:   # (a template kernel of a header may be in two units)
                        sys.exit("kernel_text: two different kernels named %s" % name)
    os.makedirs(out_dir, exist_ok=True)
    for name, text in found.items():
        open(os.path.join(out_dir, name + ".txt"), "w").write(text)
    print("%d kernels -> %s" % (len(found), out_dir))


if __name__ == "__main__":
    if len(sys.argv) < 3:
        sys.exit(__doc__)
    main(sys.argv[1], sys.argv[2:])
