"""Per-symbol gfx950 ISA of HIP objects, to check that a change leaves the machine code of kernels as it was.

    python tools/isa_symbols.py --before OBJ... --after OBJ...   # prints the symbols whose instructions differ (none: exit status 0)
    python tools/isa_symbols.py OBJ_BEFORE OBJ_AFTER             # the same for one object on each side
    python tools/isa_symbols.py OBJ                               # one line per symbol: instruction count and a hash

OBJ is what `hipcc --offload-arch=gfx950 <the FLAGS of messyerraytracer_amd/build.py> --cuda-device-only -c UNIT.hip -o OBJ`
writes (an offload bundle; a bare code object works too).  The gfx950 code object is unbundled with clang-offload-bundler and
disassembled with `llvm-objdump -d --no-show-raw-insn`; per symbol, the instructions are compared with addresses, symbolised branch
targets and objdump's `...` for alignment padding taken out.  Labels of inline assembly count as part of their kernel.  A run of
`s_nop 0` at the end of a symbol is dropped as well: it is the padding that ends a code section, and it belongs to whichever kernel
happens to be last in its object, not to that kernel.  The objects of one side are taken together, as the units of one library; a
symbol present in two of them is an error.  Only symbols present on both sides are compared; the ones only in the second are listed
as new."""
import argparse
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
    for ins in out.values():
        while ins and ins[-1] == "s_nop 0":
            ins.pop()
    return out


def side(objs) -> dict:
    """The symbols of a set of objects; SystemExit if two of them define the same one."""
    out, where = {}, {}
    for obj in objs:
        for name, ins in symbols(obj).items():
            if name in out:
                raise SystemExit(f"error: {name} is in {where[name]} and in {obj}")
            out[name], where[name] = ins, obj
    return out


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("objs", nargs="*")
    ap.add_argument("--before", nargs="+", default=[])
    ap.add_argument("--after", nargs="+", default=[])
    args = ap.parse_args()
    if len(args.objs) == 1 and not args.before and not args.after:
        for name, ins in sorted(symbols(args.objs[0]).items()):
            print(f"{len(ins):6d} {hashlib.sha1(chr(10).join(ins).encode()).hexdigest()[:16]} {name}")
        return 0
    before, after = (args.objs[:1], args.objs[1:]) if len(args.objs) == 2 and not args.before and not args.after else (args.before, args.after)
    if not before or not after or (args.objs and (args.before or args.after)):
        ap.error("give OBJ, OBJ_BEFORE OBJ_AFTER, or --before OBJ... --after OBJ...")
    a, b = side(before), side(after)
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
