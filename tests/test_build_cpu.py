"""build.py's own rules, checked without compiling anything: what is built from what, when a define set means a rebuild, how
many compiles run side by side, and the names the rest of the suite calls."""
import glob
import inspect
import os

from messyerraytracer_amd import build


def test_every_source_file_is_built_exactly_once():
    """Every .hip / .cpp under csrc is a unit of the library, or a source of exactly one host-driver row that is not a unit
    (a unit may be compiled into drivers as well: launch_policy.cpp, host/*_data.cpp)."""
    on_disk = {os.path.relpath(p, build.CSRC) for pat in ("*.hip", "*.cpp", "host/*.hip", "host/*.cpp")
               for p in glob.glob(os.path.join(build.CSRC, pat))}
    assert len(build.SOURCES) == len(set(build.SOURCES))
    assert set(build.SOURCES) <= on_disk
    main_of = {}
    for name, (srcs, flags, links) in build.DRIVERS.items():
        assert set(srcs) <= on_disk, name
        for s in srcs:
            if s not in build.SOURCES:
                main_of.setdefault(s, []).append(name.removesuffix("_san"))  # (the sanitized twin is the same row's source)
    assert all(len(set(v)) == 1 for v in main_of.values()), main_of
    assert on_disk == set(build.SOURCES) | set(main_of)
    for unit in ("kernels.hip", "shade_kernels.hip", "prep_kernels.hip"):
        assert unit in build.SOURCES


def test_define_set_decides_the_build():
    assert build.define_set({}) == []
    assert build.define_set({"MRT_WITH_QUAD": "1"}) == ["-DMRT_WITH_QUAD"]
    assert build.define_set({"MRT_WITH_QUAD": "0"}) == []
    env = {"MRT_WITH_QUAD": "1", "MRT_EXTRA_DEFINES": "-DMRT_ROWS_WG_LARGE=128 -DMRT_ASM_KPF=0"}
    d = build.define_set(env)
    assert d == sorted(d) and set(d) == {"-DMRT_WITH_QUAD", "-DMRT_ROWS_WG_LARGE=128", "-DMRT_ASM_KPF=0"}
    assert build.define_set(dict(env)) == d  # a pure function of its argument
    stamp = " ".join(d) + "\n"
    assert not build.defines_changed(stamp, d)
    assert not build.defines_changed(stamp, list(reversed(d)))  # the order the flags were given in is not a difference
    assert build.defines_changed(None, d) and build.defines_changed(None, [])  # no stamp: rebuild
    assert build.defines_changed(stamp, []) and build.defines_changed("\n", d)
    assert build.defines_changed(stamp, d[:-1]) and build.defines_changed(stamp, d + ["-DX"])
    assert not build.defines_changed("\n", [])


def test_compile_pool_is_not_sized_by_the_cpu_count(monkeypatch):
    monkeypatch.setattr(os, "cpu_count", lambda: 256)
    n = len(build.SOURCES)
    assert build.pool_size(n, {}) == min(n, 16) <= 16
    assert build.pool_size(100, {}) == 16
    assert build.pool_size(100, {"MAX_JOBS": "64"}) == 16
    assert build.pool_size(100, {"MAX_JOBS": "4"}) == 4
    assert build.pool_size(3, {"MAX_JOBS": "4"}) == 3
    assert build.pool_size(100, {"MAX_JOBS": "0"}) == 16 and build.pool_size(100, {"MAX_JOBS": "x"}) == 16
    assert "cpu_count" not in inspect.getsource(build)


def test_stream_gate_is_the_tests_alone():
    """messyerraytracer_amd/test_support/stream_gate.cpp holds no kernel and lies outside tests/ (build() must not need that
    directory); nothing of the package but build.py (which compiles it) names it, nor bench.py."""
    with open(build.STREAM_GATE_SRC) as f:
        src = f.read()
    assert "__global__" not in src and "hipLaunchKernelGGL" not in src and "<<<" not in src
    assert os.path.dirname(build.STREAM_GATE) == build.HERE
    assert os.path.dirname(build.STREAM_GATE_SRC) == os.path.join(build.HERE, "test_support")
    root = os.path.dirname(build.HERE)
    for path in glob.glob(os.path.join(build.HERE, "*.py")) + [os.path.join(root, "bench.py")]:
        if os.path.basename(path) != "build.py":
            with open(path) as f:
                assert "stream_gate" not in f.read(), path


def test_public_build_names():
    rows = ["build_" + name for name in build.DRIVERS if not name.endswith("_san")]
    assert set(rows) >= {"build_record_policy_test", "build_source_cast_data_test", "build_gbuffer_data_test", "build_lane_map_fast_test"}
    for name in ["build_lib", "build_drivers", "build_host_test", "build_host_cpu_test", "build_host_tlas_test", "build_policy_test",
                 "build_shadow_policy_test", "build_reflection_policy_test", "build_hemisphere_policy_test", "build_bounce_policy_test", "build_gbuffer_policy_test",
                 "build_instance_math_test", "build_build_rules_test", "build_shade_data_test", "build_light_data_test", "build_path_data_test",
                 "build_texture_data_test", "build_lane_map_test", "build_stream_gate"] + rows:
        f = getattr(build, name)
        params = inspect.signature(f).parameters
        assert "force" in params and params["force"].default is False, name
    assert inspect.signature(build.build_lane_map_test).parameters["sanitize"].default is False
    assert inspect.signature(build.build_build_rules_test).parameters["sanitize"].default is False
    for name in rows:  # sanitize exactly where the row has a sanitized twin
        params = inspect.signature(getattr(build, name)).parameters
        assert ("sanitize" in params) == (name[len("build_"):] + "_san" in build.DRIVERS), name
        assert "sanitize" not in params or params["sanitize"].default is False, name
    lib = inspect.signature(build.build_lib).parameters
    assert [lib[k].default for k in ("verbose", "lib", "obj_dir", "defines")] == [False, None, None, None]
    assert build.LIB == os.path.join(build.HERE, "libmrt_hip.so")
