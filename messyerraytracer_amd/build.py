"""Builds libmrt_hip.so (the C-ABI library: HIP kernels for gfx950 + host-side
scene preparation) and the C++ test drivers in-tree with hipcc.  hipcc cross-compiles without a GPU."""
import concurrent.futures
import glob
import os
import shutil
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
LIB = os.path.join(HERE, "libmrt_hip.so")
OBJ = os.path.join(HERE, "_obj")  # object files, their dependency files and the define set of the last build (git-ignored)

# The library's translation units.  The kernels are three of them: kernels.hip = the walks, shade_kernels.hip = the
# passes over hit records, prep_kernels.hip = what prepares a scene or a cast; an edit to one is compiled apart from the others.
SOURCES = ["kernels.hip", "shade_kernels.hip", "prep_kernels.hip", "api.hip", "cast.hip", "schedule.hip", "launch_policy.cpp", "group.hip",
           "device_build.hip", "refit.hip", "tlas_device.hip", "surface.hip", "texture.hip", "lighting.hip", "path.hip", "panorama.hip", "channels.hip", "accum.hip", "denoise.hip", "svgf.hip", "emitters.hip",
           "host/shade_data.cpp", "host/texture_data.cpp", "host/light_data.cpp", "host/path_data.cpp", "host/panorama_data.cpp", "host/channel_data.cpp", "host/accum_data.cpp", "host/denoise_data.cpp", "host/svgf_data.cpp", "host/gbuffer_data.cpp", "host/source_cast_data.cpp", "host/emitter_data.cpp", "host/scene_prep.cpp", "host/bvh_builder.cpp", "host/two_level_prep.cpp"]
# -Xarch_host -mfma: explicit fmaf() calls of the host code (the 8-wide collapse verifies every quantised
# box with the kernel's own fma) become one instruction instead of a libm call; nothing is contracted
# implicitly (-ffp-contract=off), so every result is unchanged.
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-Wall",
         "-Wno-unused-result", "-Xarch_host", "-mfma"]

# The C++ test drivers: name -> (sources under csrc, flags, whether it links the library).  MIRROR: the host mirrors over the C-ABI;
# POLICY: launch_policy.cpp alone; CPU: headers or host/*.cpp compiled for the CPU alone.  The last two need no device and no library.
# A new driver is one row here (and a second one by _twin if it is to run under the sanitizers too): build_<name> below, build() of
# __graft_entry__.py and .gitignore follow from it.
MIRROR = ["-O2", "-std=c++17", "-ffp-contract=off", "-Wall"]
POLICY = ["-O2", "-std=c++17", "-Wall"]
CPU = ["-x", "c++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall"]
LANE = ["-x", "c++", "-O2", "-std=c++17", "-Wall"]
SANITIZE = ["-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]


def _twin(row):
    """The row of a driver's sanitized twin, <name>_san: the same sources under AddressSanitizer and UndefinedBehaviorSanitizer."""
    srcs, flags, links = row
    return srcs, [f for f in flags if f != "-O2"] + SANITIZE, links


DRIVERS = {
    "host_mirror_test": (["host/host_mirror_test.cpp"], MIRROR, True),  # GPURayCaster / RayDispatcher
    "host_cpu_test": (["host/host_cpu_test.cpp"], MIRROR, True),        # RayTracerServer over the router's CPU backend
    "host_tlas_test": (["host/host_tlas_test.cpp"], MIRROR, True),      # the router with a TLAS set, CPU and device backend
    "launch_policy_test": (["host/launch_policy_test.cpp", "launch_policy.cpp"], POLICY, False),
    "record_policy_test": (["host/record_policy_test.cpp", "launch_policy.cpp"], POLICY, False),  # the six record-driven families: <exe> [family]
    "instance_math_test": (["host/instance_math_test.cpp"], CPU, False),  # instance_math.h, shared by the host path and the device TLAS build
    "build_rules_test": (["host/build_rules_test.cpp"], CPU, False),  # build_rules.h, shared by the host and the device scene builders
    "walk_steps_test": (["host/walk_steps_test.cpp"], CPU, False),  # walk_steps.h (the token expansion, the host walkers) against oracle/mrt_oracle.c
    "shade_data_test": (["host/shade_data_test.cpp", "host/shade_data.cpp"], CPU, False),
    "light_data_test": (["host/light_data_test.cpp", "host/light_data.cpp"], CPU, False),
    "path_data_test": (["host/path_data_test.cpp", "host/path_data.cpp"], CPU, False),
    "texture_data_test": (["host/texture_data_test.cpp", "host/texture_data.cpp"], CPU, False),
    "panorama_data_test": (["host/panorama_data_test.cpp", "host/panorama_data.cpp"], CPU, False),  # panorama.h, shared with the kernels
    "channel_data_test": (["host/channel_data_test.cpp", "host/channel_data.cpp"], CPU, False),  # channels.h, shared with the kernels
    "accum_data_test": (["host/accum_data_test.cpp", "host/accum_data.cpp"], CPU, False),  # accum.h, shared with the kernels
    "denoise_data_test": (["host/denoise_data_test.cpp", "host/denoise_data.cpp"], CPU, False),  # denoise.h, shared with the kernels
    "svgf_data_test": (["host/svgf_data_test.cpp", "host/svgf_data.cpp"], CPU, False),  # svgf.h, shared with the kernels
    "gbuffer_data_test": (["host/gbuffer_data_test.cpp", "host/gbuffer_data.cpp"], CPU, False),  # gbuffer.h, shared with the kernels
    "source_cast_data_test": (["host/source_cast_data_test.cpp", "host/source_cast_data.cpp"], CPU, False),  # source_cast.h
    "emitter_data_test": (["host/emitter_data_test.cpp", "host/emitter_data.cpp", "host/path_data.cpp"], CPU, False),  # emitters.h
    "emitter_policy_test": (["host/emitter_policy_test.cpp", "launch_policy.cpp"], POLICY, False),  # the emitter-shadow entries against the selected-shadow entries
    "lane_map_test": (["host/lane_map_test.cpp"], LANE, False),  # lane_map.h
    "lane_map_fast_test": (["host/lane_map_fast_test.cpp"], LANE, False),  # lane_map.h: the short map of whole-tile pairs
}
for _name in ("build_rules_test", "walk_steps_test", "accum_data_test", "denoise_data_test", "svgf_data_test", "gbuffer_data_test", "source_cast_data_test", "emitter_data_test",
              "lane_map_test", "lane_map_fast_test"):
    DRIVERS[_name + "_san"] = _twin(DRIVERS[_name])


def _hipcc() -> str:
    for c in (shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if c and os.path.exists(c):
            return c
    raise RuntimeError("hipcc not found: libmrt_hip.so cannot be built")


def _run(cmd, what: str) -> str:
    r = subprocess.run(cmd, capture_output=True, text=True, cwd=CSRC)
    if r.returncode != 0:
        raise RuntimeError(what + " failed:\n" + " ".join(cmd) + "\n" + r.stdout + r.stderr)
    return r.stderr


def _stale(target: str, deps) -> bool:
    """deps None: not known (no dependency file yet)."""
    if deps is None or not os.path.exists(target):
        return True
    t = os.path.getmtime(target)
    return any(not os.path.exists(d) or os.path.getmtime(d) > t for d in list(deps) + [os.path.abspath(__file__)])


def _deps(dfile: str):
    """The files a compiler's -MD output names (relative ones are relative to csrc); None without one."""
    if not os.path.exists(dfile):
        return None
    with open(dfile) as f:
        words = f.read().replace("\\\n", " ").split()
    return [os.path.join(CSRC, w) for w in words if not w.endswith(":")]


def define_set(env) -> list:
    """The -D flags that decide what is built.  MRT_WITH_QUAD=1 also compiles the four-wide packet walk (packet_quad_kernel.h: an
    experiment kept for the record, slower than the default on every measured config; the packet tests hold it to the oracle only
    in such a build and skip its cases in any other, where tests/test_define_sets_cpu.py holds it to compiling: from 7a50a6c
    until that test came it did not);
    MRT_EXTRA_DEFINES: A/B builds of the tools (e.g. -DMRT_ASM_KPF=0)."""
    return sorted((["-DMRT_WITH_QUAD"] if env.get("MRT_WITH_QUAD") == "1" else []) + env.get("MRT_EXTRA_DEFINES", "").split())


def defines_changed(stamp, defines) -> bool:
    """stamp = the text written beside the objects by the build that made them (None: there is none)."""
    return stamp is None or stamp.split() != sorted(defines)


def pool_size(n_sources: int, env, limit: int = 16) -> int:
    """Compiles side by side: never sized by the machine's CPU count (a shared machine shows all of them to everyone)."""
    jobs = min(n_sources, limit)
    if env.get("MAX_JOBS", "").isdigit() and int(env["MAX_JOBS"]) > 0:
        jobs = min(jobs, int(env["MAX_JOBS"]))
    return max(jobs, 1)


def build_lib(force: bool = False, verbose: bool = False, lib: str = None, obj_dir: str = None, defines=None) -> str:
    """One object per translation unit with the dependencies the compiler reports, then one link.  Nothing is done while the library is
    newer than everything its objects were made from (the objects themselves are intermediates: a tree that brings its library needs
    none); else an object is compiled when it is missing or older than a file it depends on.  defines: instead of define_set's."""
    lib, obj_dir = os.path.abspath(lib or LIB), os.path.abspath(obj_dir or OBJ)
    defines = define_set(os.environ) if defines is None else sorted(defines)
    stamp = os.path.join(obj_dir, "defines.txt")
    objs = [os.path.join(obj_dir, s.replace("/", "_") + ".o") for s in SOURCES]
    old = open(stamp).read() if os.path.exists(stamp) else None
    force = force or defines_changed(old, defines)
    all_deps = [_deps(o + ".d") for o in objs]
    if not force and not _stale(lib, None if None in all_deps else [d for ds in all_deps for d in ds]):
        return lib
    os.makedirs(obj_dir, exist_ok=True)
    if force and old is not None:
        os.remove(stamp)  # (until every object is of the new set)
    jobs = [(s, o) for s, o, ds in zip(SOURCES, objs, all_deps) if force or _stale(o, ds)]

    def compile_one(job):
        src, obj = job
        log = _run([_hipcc()] + FLAGS + defines + ["-MD", "-MF", obj + ".d", "-c", os.path.join(CSRC, src), "-o", obj], "hipcc")
        with open(obj + ".d") as f:  # the tree's own files relative to csrc: a tree that moves with its library is not stale for that
            text = f.read().replace(CSRC + os.sep, "")
        with open(obj + ".d", "w") as f:
            f.write(text)
        return log

    with concurrent.futures.ThreadPoolExecutor(max_workers=pool_size(len(SOURCES), os.environ)) as pool:
        logs = list(pool.map(compile_one, jobs))
    with open(stamp, "w") as f:
        f.write(" ".join(defines) + "\n")
    if jobs or _stale(lib, objs):
        logs.append(_run([_hipcc(), "--offload-arch=gfx950", "-shared", "-fPIC"] + objs + ["-o", lib, "-pthread"], "hipcc link"))
    if verbose:
        print("".join(logs))
    return lib


def build_driver(name: str, force: bool = False) -> str:
    """One row of DRIVERS, rebuilt when a source, any header of csrc or (if it links it) the library is newer."""
    srcs, flags, links = DRIVERS[name]
    srcs, exe = [os.path.join(CSRC, s) for s in srcs], os.path.join(HERE, name)
    headers = [h for pat in ("*.h", "*.inc", "host/*.h", "host/*.hpp", "../../include/*.h", "../../oracle/mrt_oracle.[ch]") for h in glob.glob(os.path.join(CSRC, pat))]
    if force or _stale(exe, srcs + headers + ([LIB] if links else [])):
        _run([_hipcc()] + flags + srcs + ["-o", exe] + (["-L" + HERE, "-lmrt_hip", "-Wl,-rpath," + HERE, "-pthread"] if links else []), name + " build")
    return exe


STREAM_GATE = os.path.join(HERE, "libmrt_stream_gate.so")
STREAM_GATE_SRC = os.path.join(HERE, "test_support", "stream_gate.cpp")  # (in the package: build() needs nothing of tests/)


def build_stream_gate(force: bool = False) -> str:
    """The tests' own caller of the HIP runtime (test_support/stream_gate.cpp: a stream, a timed gate and copies on it; no
    kernel), linked against the runtime the library links.  The package never loads it."""
    if force or _stale(STREAM_GATE, [STREAM_GATE_SRC]):
        _run([_hipcc(), "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", STREAM_GATE_SRC, "-o", STREAM_GATE, "-pthread"], "stream gate build")
    return STREAM_GATE


def build_drivers(force: bool = False) -> list:
    """Every driver but the sanitized twins (a test that runs one builds it)."""
    return [build_driver(name, force) for name in DRIVERS if not name.endswith("_san")]


def _driver(name: str):
    """build_<name>(force=False), and sanitize=False exactly where DRIVERS has the row's twin."""
    if name + "_san" in DRIVERS:
        def build(force: bool = False, sanitize: bool = False) -> str:
            return build_driver(name + "_san" if sanitize else name, force)
        build.__doc__ = "C++ test driver " + name + " (DRIVERS); sanitize = its twin under AddressSanitizer and UndefinedBehaviorSanitizer."
    else:
        def build(force: bool = False) -> str:
            return build_driver(name, force)
        build.__doc__ = "C++ test driver " + name + " (DRIVERS)."
    return build


for _name in DRIVERS:
    if not _name.endswith("_san"):
        globals()["build_" + _name] = _driver(_name)
# callables whose name is not their row's
build_host_test = build_host_mirror_test  # noqa: F821
build_policy_test = build_launch_policy_test  # noqa: F821
# (one driver for every family now: run it with the family's name)
build_shadow_policy_test = build_reflection_policy_test = build_hemisphere_policy_test = build_bounce_policy_test = build_record_policy_test  # noqa: F821
build_gbuffer_policy_test = build_record_policy_test  # noqa: F821


if __name__ == "__main__":
    print(build_lib(force=True, verbose=True))
    print("\n".join(build_drivers(force=True)))
