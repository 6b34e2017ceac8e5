"""Builds libmrt_hip.so (the C-ABI library: HIP kernels for gfx950 + host-side
scene preparation) in-tree with hipcc.  hipcc cross-compiles without a GPU."""
import concurrent.futures
import os
import shutil
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
LIB = os.path.join(HERE, "libmrt_hip.so")
OBJ = os.path.join(HERE, "_obj")  # object files of the last build (git-ignored; not needed at run time)
HOST_TEST = os.path.join(HERE, "host_mirror_test")
HOST_CPU_TEST = os.path.join(HERE, "host_cpu_test")
HOST_TLAS_TEST = os.path.join(HERE, "host_tlas_test")
POLICY_TEST = os.path.join(HERE, "launch_policy_test")
SHADOW_POLICY_TEST = os.path.join(HERE, "shadow_policy_test")
REFLECTION_POLICY_TEST = os.path.join(HERE, "reflection_policy_test")
HEMISPHERE_POLICY_TEST = os.path.join(HERE, "hemisphere_policy_test")
BOUNCE_POLICY_TEST = os.path.join(HERE, "bounce_policy_test")
INSTANCE_MATH_TEST = os.path.join(HERE, "instance_math_test")
SHADE_DATA_TEST = os.path.join(HERE, "shade_data_test")
LANE_MAP_TEST = os.path.join(HERE, "lane_map_test")
LIGHT_DATA_TEST = os.path.join(HERE, "light_data_test")
PATH_DATA_TEST = os.path.join(HERE, "path_data_test")
TEXTURE_DATA_TEST = os.path.join(HERE, "texture_data_test")

SOURCES = ["kernels.hip", "api.hip", "cast.hip", "schedule.hip", "launch_policy.cpp", "group.hip", "device_build.hip", "refit.hip",
           "tlas_device.hip", "surface.hip", "texture.hip", "lighting.hip", "path.hip", "host/shade_data.cpp", "host/texture_data.cpp", "host/light_data.cpp", "host/path_data.cpp", "host/scene_prep.cpp", "host/bvh_builder.cpp", "host/two_level_prep.cpp"]
HEADERS = ["mrt_internal.h", "instance_math.h", "lane_map.h", "mrt_context.h", "launch_policy.h", "packet_kernel.h", "packet_asm_kernel.h", "packet_rows_kernel.h", "packet_quad_kernel.h", "two_level_kernel.h", "lane_persistent_kernel.h", "source_common.h", "shadow_kernel.h", "reflection_kernel.h", "hemisphere_kernel.h", "bounce_kernel.h", "surface_kernel.h", "surface_tex_kernel.h", "shade_data.h", "texture.h", "light_kernel.h", "lighting.h", "path_kernel.h", "path_frame_kernel.h", "path.h", "lane_walk.inc", "two_level_walk.inc", "persistent_walk.inc", "../../include/mrt_hip.h", "host/gpu_ray_caster.hpp", "host/ray_dispatcher.hpp",
           "host/host_types.hpp", "host/cpu_backend.hpp", "host/ray_tracer_server.hpp", "host/record_policy_test.h"]
# -Xarch_host -mfma: explicit fmaf() calls of the host code (the 8-wide collapse verifies every quantised
# box with the kernel's own fma) become one instruction instead of a libm call; nothing is contracted
# implicitly (-ffp-contract=off), so every result is unchanged.
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-Wall",
         "-Wno-unused-result", "-Xarch_host", "-mfma"]


def _hipcc() -> str:
    for c in (shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if c and os.path.exists(c):
            return c
    raise RuntimeError("hipcc not found: libmrt_hip.so cannot be built")


def _stale(target: str, deps) -> bool:
    if not os.path.exists(target):
        return True
    t = os.path.getmtime(target)
    return any(os.path.exists(d) and os.path.getmtime(d) > t for d in deps)


def build_lib(force: bool = False, verbose: bool = False) -> str:
    """MRT_WITH_QUAD=1 in the environment also compiles the four-wide packet walk (packet_quad_kernel.h: an experiment kept
    for the record, held to the oracle by the packet tests, slower than the default on every measured config)."""
    srcs = [os.path.join(CSRC, s) for s in SOURCES]
    deps = srcs + [os.path.join(CSRC, h) for h in HEADERS] + [os.path.abspath(__file__)]
    if force or _stale(LIB, deps):
        extra = ["-DMRT_WITH_QUAD"] if os.environ.get("MRT_WITH_QUAD") == "1" else []
        extra += os.environ.get("MRT_EXTRA_DEFINES", "").split()  # A/B builds of the tools (e.g. -DMRT_ASM_KPF=0)
        # one object per translation unit, compiled side by side (kernels.hip alone is over a minute), then one link
        os.makedirs(OBJ, exist_ok=True)
        objs = [os.path.join(OBJ, s.replace("/", "_") + ".o") for s in SOURCES]

        def compile_one(job):
            src, obj = job
            cmd = [_hipcc()] + FLAGS + extra + ["-c", src, "-o", obj]
            r = subprocess.run(cmd, capture_output=True, text=True, cwd=CSRC)
            if r.returncode != 0:
                raise RuntimeError("hipcc failed:\n" + " ".join(cmd) + "\n" + r.stdout + r.stderr)
            return r.stderr

        with concurrent.futures.ThreadPoolExecutor(max_workers=min(len(srcs), os.cpu_count() or 1)) as pool:
            logs = list(pool.map(compile_one, zip(srcs, objs)))
        cmd = [_hipcc(), "--offload-arch=gfx950", "-shared", "-fPIC"] + objs + ["-o", LIB, "-pthread"]
        r = subprocess.run(cmd, capture_output=True, text=True, cwd=CSRC)
        if r.returncode != 0:
            raise RuntimeError("hipcc link failed:\n" + " ".join(cmd) + "\n" + r.stdout + r.stderr)
        if verbose:
            print("".join(logs) + r.stderr)
    return LIB


def build_host_test(force: bool = False) -> str:
    """C++ test driver for the GPURayCaster / RayDispatcher mirrors (links the C-ABI)."""
    src = os.path.join(CSRC, "host", "host_mirror_test.cpp")
    deps = [src, LIB] + [os.path.join(CSRC, h) for h in HEADERS]
    if force or _stale(HOST_TEST, deps):
        cmd = [_hipcc(), "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", src, "-o", HOST_TEST,
               "-L" + HERE, "-lmrt_hip", "-Wl,-rpath," + HERE, "-pthread"]
        r = subprocess.run(cmd, capture_output=True, text=True, cwd=CSRC)
        if r.returncode != 0:
            raise RuntimeError("host test build failed:\n" + r.stdout + r.stderr)
    return HOST_TEST


def build_host_cpu_test(force: bool = False) -> str:
    """C++ test driver for the RayTracerServer mirror over the router's CPU backend (links the C-ABI for the host-side builder)."""
    src = os.path.join(CSRC, "host", "host_cpu_test.cpp")
    deps = [src, LIB] + [os.path.join(CSRC, h) for h in HEADERS]
    if force or _stale(HOST_CPU_TEST, deps):
        cmd = [_hipcc(), "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", src, "-o", HOST_CPU_TEST,
               "-L" + HERE, "-lmrt_hip", "-Wl,-rpath," + HERE, "-pthread"]
        r = subprocess.run(cmd, capture_output=True, text=True, cwd=CSRC)
        if r.returncode != 0:
            raise RuntimeError("host cpu test build failed:\n" + r.stdout + r.stderr)
    return HOST_CPU_TEST


def build_host_tlas_test(force: bool = False) -> str:
    """C++ test driver for the router with a TLAS set (two-level scenes on the CPU and the device backend)."""
    src = os.path.join(CSRC, "host", "host_tlas_test.cpp")
    deps = [src, LIB] + [os.path.join(CSRC, h) for h in HEADERS]
    if force or _stale(HOST_TLAS_TEST, deps):
        cmd = [_hipcc(), "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", src, "-o", HOST_TLAS_TEST,
               "-L" + HERE, "-lmrt_hip", "-Wl,-rpath," + HERE, "-pthread"]
        r = subprocess.run(cmd, capture_output=True, text=True, cwd=CSRC)
        if r.returncode != 0:
            raise RuntimeError("host tlas test build failed:\n" + r.stdout + r.stderr)
    return HOST_TLAS_TEST


def build_policy_test(force: bool = False) -> str:
    """C++ test driver for the cast launch policy (launch_policy.cpp alone: host code, no device, no library)."""
    srcs = [os.path.join(CSRC, "host", "launch_policy_test.cpp"), os.path.join(CSRC, "launch_policy.cpp")]
    deps = srcs + [os.path.join(CSRC, h) for h in HEADERS]
    if force or _stale(POLICY_TEST, deps):
        cmd = [_hipcc(), "-O2", "-std=c++17", "-Wall"] + srcs + ["-o", POLICY_TEST]
        r = subprocess.run(cmd, capture_output=True, text=True, cwd=CSRC)
        if r.returncode != 0:
            raise RuntimeError("launch policy test build failed:\n" + r.stdout + r.stderr)
    return POLICY_TEST


def build_shadow_policy_test(force: bool = False) -> str:
    """C++ test driver for the plans of shadow casts (launch_policy.cpp alone: host code, no device, no library)."""
    srcs = [os.path.join(CSRC, "host", "shadow_policy_test.cpp"), os.path.join(CSRC, "launch_policy.cpp")]
    deps = srcs + [os.path.join(CSRC, h) for h in HEADERS]
    if force or _stale(SHADOW_POLICY_TEST, deps):
        cmd = [_hipcc(), "-O2", "-std=c++17", "-Wall"] + srcs + ["-o", SHADOW_POLICY_TEST]
        r = subprocess.run(cmd, capture_output=True, text=True, cwd=CSRC)
        if r.returncode != 0:
            raise RuntimeError("shadow policy test build failed:\n" + r.stdout + r.stderr)
    return SHADOW_POLICY_TEST


def build_reflection_policy_test(force: bool = False) -> str:
    """C++ test driver for the plans of reflection casts (launch_policy.cpp alone: host code, no device, no library)."""
    srcs = [os.path.join(CSRC, "host", "reflection_policy_test.cpp"), os.path.join(CSRC, "launch_policy.cpp")]
    deps = srcs + [os.path.join(CSRC, h) for h in HEADERS]
    if force or _stale(REFLECTION_POLICY_TEST, deps):
        cmd = [_hipcc(), "-O2", "-std=c++17", "-Wall"] + srcs + ["-o", REFLECTION_POLICY_TEST]
        r = subprocess.run(cmd, capture_output=True, text=True, cwd=CSRC)
        if r.returncode != 0:
            raise RuntimeError("reflection policy test build failed:\n" + r.stdout + r.stderr)
    return REFLECTION_POLICY_TEST


def build_hemisphere_policy_test(force: bool = False) -> str:
    """C++ test driver for the plans of hemisphere casts (launch_policy.cpp alone: host code, no device, no library)."""
    srcs = [os.path.join(CSRC, "host", "hemisphere_policy_test.cpp"), os.path.join(CSRC, "launch_policy.cpp")]
    deps = srcs + [os.path.join(CSRC, h) for h in HEADERS]
    if force or _stale(HEMISPHERE_POLICY_TEST, deps):
        cmd = [_hipcc(), "-O2", "-std=c++17", "-Wall"] + srcs + ["-o", HEMISPHERE_POLICY_TEST]
        r = subprocess.run(cmd, capture_output=True, text=True, cwd=CSRC)
        if r.returncode != 0:
            raise RuntimeError("hemisphere policy test build failed:\n" + r.stdout + r.stderr)
    return HEMISPHERE_POLICY_TEST


def build_bounce_policy_test(force: bool = False) -> str:
    """C++ test driver for the plans of bounce casts (launch_policy.cpp alone: host code, no device, no library)."""
    srcs = [os.path.join(CSRC, "host", "bounce_policy_test.cpp"), os.path.join(CSRC, "launch_policy.cpp")]
    deps = srcs + [os.path.join(CSRC, h) for h in HEADERS]
    if force or _stale(BOUNCE_POLICY_TEST, deps):
        cmd = [_hipcc(), "-O2", "-std=c++17", "-Wall"] + srcs + ["-o", BOUNCE_POLICY_TEST]
        r = subprocess.run(cmd, capture_output=True, text=True, cwd=CSRC)
        if r.returncode != 0:
            raise RuntimeError("bounce policy test build failed:\n" + r.stdout + r.stderr)
    return BOUNCE_POLICY_TEST


def build_instance_math_test(force: bool = False) -> str:
    """C++ test driver for the per-instance arithmetic shared by the host path and the device top-level build (instance_math.h
    compiled for the CPU alone: no device, no library)."""
    src = os.path.join(CSRC, "host", "instance_math_test.cpp")
    deps = [src, os.path.join(CSRC, "instance_math.h")]
    if force or _stale(INSTANCE_MATH_TEST, deps):
        cmd = [_hipcc(), "-x", "c++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", src, "-o", INSTANCE_MATH_TEST]
        r = subprocess.run(cmd, capture_output=True, text=True, cwd=CSRC)
        if r.returncode != 0:
            raise RuntimeError("instance math test build failed:\n" + r.stdout + r.stderr)
    return INSTANCE_MATH_TEST


def build_shade_data_test(force: bool = False) -> str:
    """C++ test driver for the checks and the row packing of shade data (host/shade_data.cpp alone: host code, no device, no
    library)."""
    srcs = [os.path.join(CSRC, "host", "shade_data_test.cpp"), os.path.join(CSRC, "host", "shade_data.cpp")]
    deps = srcs + [os.path.join(CSRC, "shade_data.h"), os.path.join(CSRC, "../../include/mrt_hip.h")]
    if force or _stale(SHADE_DATA_TEST, deps):
        cmd = [_hipcc(), "-x", "c++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall"] + srcs + ["-o", SHADE_DATA_TEST]
        r = subprocess.run(cmd, capture_output=True, text=True, cwd=CSRC)
        if r.returncode != 0:
            raise RuntimeError("shade data test build failed:\n" + r.stdout + r.stderr)
    return SHADE_DATA_TEST


def build_light_data_test(force: bool = False) -> str:
    """C++ test driver for the checks of a light list and an environment, the kernel's copy of both and pow01 (host/light_data.cpp and
    lighting.h alone: host code, no device, no library)."""
    srcs = [os.path.join(CSRC, "host", "light_data_test.cpp"), os.path.join(CSRC, "host", "light_data.cpp")]
    deps = srcs + [os.path.join(CSRC, "lighting.h"), os.path.join(CSRC, "../../include/mrt_hip.h")]
    if force or _stale(LIGHT_DATA_TEST, deps):
        cmd = [_hipcc(), "-x", "c++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall"] + srcs + ["-o", LIGHT_DATA_TEST]
        r = subprocess.run(cmd, capture_output=True, text=True, cwd=CSRC)
        if r.returncode != 0:
            raise RuntimeError("light data test build failed:\n" + r.stdout + r.stderr)
    return LIGHT_DATA_TEST


def build_path_data_test(force: bool = False) -> str:
    """C++ test driver for the refusals of the path state calls, the generator's jump, the kernel's copy of a descriptor, the tone
    mappers and the gamma (host/path_data.cpp, path.h and lighting.h alone: host code, no device, no library)."""
    srcs = [os.path.join(CSRC, "host", "path_data_test.cpp"), os.path.join(CSRC, "host", "path_data.cpp")]
    deps = srcs + [os.path.join(CSRC, "path.h"), os.path.join(CSRC, "lighting.h"), os.path.join(CSRC, "../../include/mrt_hip.h")]
    if force or _stale(PATH_DATA_TEST, deps):
        cmd = [_hipcc(), "-x", "c++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall"] + srcs + ["-o", PATH_DATA_TEST]
        r = subprocess.run(cmd, capture_output=True, text=True, cwd=CSRC)
        if r.returncode != 0:
            raise RuntimeError("path data test build failed:\n" + r.stdout + r.stderr)
    return PATH_DATA_TEST


def build_texture_data_test(force: bool = False) -> str:
    """C++ test driver for the refusals of a texture set and the layout of its texel pool (host/texture_data.cpp and texture.h alone:
    host code, no device, no library)."""
    srcs = [os.path.join(CSRC, "host", "texture_data_test.cpp"), os.path.join(CSRC, "host", "texture_data.cpp")]
    deps = srcs + [os.path.join(CSRC, "texture.h"), os.path.join(CSRC, "../../include/mrt_hip.h")]
    if force or _stale(TEXTURE_DATA_TEST, deps):
        cmd = [_hipcc(), "-x", "c++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall"] + srcs + ["-o", TEXTURE_DATA_TEST]
        r = subprocess.run(cmd, capture_output=True, text=True, cwd=CSRC)
        if r.returncode != 0:
            raise RuntimeError("texture data test build failed:\n" + r.stdout + r.stderr)
    return TEXTURE_DATA_TEST


def build_lane_map_test(force: bool = False, sanitize: bool = False) -> str:
    """C++ test driver for the lane map (lane_map.h compiled for the CPU alone: no device, no library); sanitize = a second binary
    under AddressSanitizer and UndefinedBehaviorSanitizer."""
    src = os.path.join(CSRC, "host", "lane_map_test.cpp")
    exe = LANE_MAP_TEST + ("_san" if sanitize else "")
    deps = [src, os.path.join(CSRC, "lane_map.h")]
    if force or _stale(exe, deps):
        flags = ["-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"] if sanitize else ["-O2"]
        cmd = [_hipcc(), "-x", "c++", "-std=c++17", "-Wall"] + flags + [src, "-o", exe]
        r = subprocess.run(cmd, capture_output=True, text=True, cwd=CSRC)
        if r.returncode != 0:
            raise RuntimeError("lane map test build failed:\n" + r.stdout + r.stderr)
    return exe


if __name__ == "__main__":
    print(build_lib(force=True, verbose=True))
    print(build_host_test(force=True))
    print(build_host_cpu_test(force=True))
    print(build_host_tlas_test(force=True))
    print(build_policy_test(force=True))
    print(build_shadow_policy_test(force=True))
    print(build_reflection_policy_test(force=True))
    print(build_hemisphere_policy_test(force=True))
    print(build_bounce_policy_test(force=True))
    print(build_instance_math_test(force=True))
    print(build_shade_data_test(force=True))
    print(build_light_data_test(force=True))
    print(build_path_data_test(force=True))
    print(build_texture_data_test(force=True))
    print(build_lane_map_test(force=True))
