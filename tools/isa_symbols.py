"""Per-symbol gfx950 ISA of a HIP object, to check that a change leaves the machine code of kernels as it was.

    python tools/isa_symbols.py OBJ_BEFORE OBJ_AFTER      # prints the symbols whose instructions differ (none: exit status 0)
    python tools/isa_symbols.py OBJ                        # one line per symbol: instruction count and a hash

OBJ is what `hipcc --offload-arch=gfx950 <the FLAGS of messyerraytracer_amd/build.py> --cuda-device-only -c kernels.hip -o OBJ`
writes (an offload bundle; a bare code object works too).  The gfx950 code object is unbundled with clang-offload-bundler and
disassembled with `llvm-objdump -d --no-show-raw-insn`; per symbol, the instructions are compared with addresses, symbolised branch
targets and objdump's `...` for alignment padding taken out.  Labels of inline assembly count as part of their kernel.  Only symbols
present in both objects are compared; the ones only in the second are listed as new."""
import hashlib
import os
import re
import subprocess
import sys
import tempfile

LLVM = "/opt/rocm/llvm/bin"


def disassemble(obj: str) -> str:
    with tempfile.TemporaryDirectory() as d:
        co = os.path.join(d, "k.co")
        r = subprocess.run([os.path.join(LLVM, "clang-offload-bundler"), "--unbundle", "--type=o", "--input=" + obj,
                            "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--output=" + co], capture_output=True, text=True)
        if r.returncode != 0:
            co = obj  # not a bundle: a code object already
        return subprocess.run([os.path.join(LLVM, "llvm-objdump"), "-d", "--no-show-raw-insn", co],
                              capture_output=True, text=True, check=True).stdout


def symbols(obj: str) -> dict:
    out, cur = {}, None
    for line in disassemble(obj).splitlines():
        m = re.match(r"^[0-9a-f]+ <(.*)>:$", line)
        if m:
            if m.group(1).startswith("L_") and cur is not None:
                out[cur].append("label " + re.sub(r"_\d+$", "", m.group(1)))
            else:
                cur = m.group(1)
                out[cur] = []
            continue
        text = line.split("//")[0].strip()
        if cur is None or not text or text == "...":
            continue
        out[cur].append(re.sub(r"<[^>]*>", "", text))
    return out


def main() -> int:
    if len(sys.argv) == 2:
        for name, ins in sorted(symbols(sys.argv[1]).items()):
            print(f"{len(ins):6d} {hashlib.sha1(chr(10).join(ins).encode()).hexdigest()[:16]} {name}")
        return 0
    a, b = symbols(sys.argv[1]), symbols(sys.argv[2])
    common = [k for k in a if k in b]
    changed = [k for k in common if a[k] != b[k]]
    for k in changed:
        print("changed", k)
    for k in a:
        if k not in b:
            print("missing", k)
    print(f"{len(common)} symbols in both, {len(changed)} changed, {sum(k not in b for k in a)} missing, {sum(k not in a for k in b)} new")
    return 1 if changed or any(k not in b for k in a) else 0


if __name__ == "__main__":
    sys.exit(main())
