#!/bin/bash
# A/B builds of libmrt_hip.so with extra -D flags:  tools/build_variant.sh <name> [-DFLAG ...]  ->  tools/_bin/libmrt_<name>.so
# (run a tool against it with MRT_LIB_PATH=tools/_bin/libmrt_<name>.so).  The sources and flags are build.py's; the variant keeps its
# own objects in tools/_bin/obj_<name>.
set -e
name=$1; shift
root=$(cd "$(dirname "$0")/.." && pwd)
cd "$root"
python3 -c 'import sys; from messyerraytracer_amd import build; n = sys.argv[1]
print("built", build.build_lib(lib="tools/_bin/libmrt_%s.so" % n, obj_dir="tools/_bin/obj_%s" % n, defines=sys.argv[2:]))' "$name" "$@"
