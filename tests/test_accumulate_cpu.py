"""Progressive frames without a device: the library exports the four entry points, the struct size and layout agree and the device call
rejects a null context; the host rules (csrc/host/accum_data_test.cpp, also under AddressSanitizer and UndefinedBehaviorSanitizer as a
program of its own) on hand-written frame scripts and, through a file written here, on everything tests/golden/accumulate_reference.npz
holds; the numpy restatement (messyerraytracer_amd/accumulate.py, what the GPU tests hold the kernel to byte for byte) against the same
recording -- the reference's own text of ray_renderer.cpp:444-469, :480-504, :804-835 and :850-857.  Only fp32 + - * / and
integer arithmetic enter, so every tuple is compared bit for bit: no tolerance, no tuple left out.  Where the recording holds a NaN the
restatement must hold one too (compared as NaN, not by payload): N_NAN_TUPLES below counts the running-mean columns that hold one, and no
other tuple's recording does."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

from messyerraytracer_amd import accumulate as A
from messyerraytracer_amd import build as mbuild
from messyerraytracer_amd import capi
from messyerraytracer_amd import channels as Ch

F = np.float32
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "accumulate_reference.npz")
N_NAN_TUPLES = 37   # columns of the running means in which a NaN appears: given one, or made by inf - inf

_FIXTURE = []


def fixture():
    if not _FIXTURE:
        g = np.load(GOLDEN)
        _FIXTURE.append({k: g[k] for k in g.files})
    return _FIXTURE[0]


def bits(a):
    return np.ascontiguousarray(a, dtype=F).view(np.uint32)


def test_exports_sizes_and_layouts():
    L = capi.load()
    for s in ("mrt_halton_jitter", "mrt_accum_begin_frame", "mrt_accum_end_frame", "mrt_accumulate"):
        assert hasattr(L, s) and s in capi.SYMBOLS
    assert capi.STRUCT_ACCUM_STATE == 26
    assert L.mrt_struct_size(capi.STRUCT_ACCUM_STATE) == C.sizeof(capi.AccumState) == 96
    assert L.mrt_struct_size(25) == 0 and L.mrt_struct_size(27) == 0
    assert [getattr(capi.AccumState, n).offset for n, _ in capi.AccumState._fields_] == [0, 4, 8, 12, 16, 24, 36, 72, 76, 80, 84, 88, 92]
    assert (capi.ACCUM_SRC_RGBA, capi.ACCUM_SRC_LIT, capi.ACCUM_SRC_PATH_STATE) == (0, 1, 2) == (A.SRC_RGBA, A.SRC_LIT, A.SRC_PATH_STATE)
    assert L.mrt_version() == 1
    # the struct before it is as it was
    assert L.mrt_struct_size(capi.STRUCT_CHANNEL_OUT) == C.sizeof(capi.ChannelOut)


def test_null_context_is_invalid():
    """(With a context, every bad argument is refused before any device work: test_accumulate_gpu.py.)"""
    L = capi.load()
    assert L.mrt_accumulate(None, 0, 16, 4, 0, 0, 4096, 8192, 0) == capi.ERR_INVALID
    assert L.mrt_accumulate(None, 0, None, 0, 0, 0, None, None, 0) == capi.ERR_INVALID
    assert L.mrt_halton_jitter(0, None) == capi.ERR_INVALID
    assert L.mrt_accum_begin_frame(None, None, None) == capi.ERR_INVALID and L.mrt_accum_end_frame(None, 0) == capi.ERR_INVALID
    with pytest.raises(capi.MrtError):
        capi.halton_jitter(0x7FFFFFFF)


def _driver_file(path):
    """The recording as the driver reads it: counts and arrays, little-endian"""
    g = fixture()
    with open(path, "wb") as f:
        for count, arrays in (((g["h_idx"].size,), ("h_idx", "h_out")), ((g["m_out"].size,), ("m_in", "m_out")), ((g["q_in"].shape[0],), ("q_in", "q_out")),
                              (g["a_src"].shape, ("a_src", "a_acc", "a_bytes"))):
            f.write(struct.pack("<%dI" % len(count), *count))
            for k in arrays:
                f.write(np.ascontiguousarray(g[k]).tobytes())


@pytest.mark.parametrize("sanitize", [False, True])
def test_accum_data_driver(tmp_path, sanitize):
    """A program of its own, with and without the sanitizers; never loaded into this process."""
    exe = mbuild.build_accum_data_test(sanitize=sanitize)
    path = str(tmp_path / "accumulate_reference.bin")
    _driver_file(path)
    g = fixture()
    for args in ([], [path]):
        r = subprocess.run([exe] + args, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stdout + r.stderr
        assert "FAIL" not in r.stdout and " checks hold " in r.stdout, r.stdout
        assert "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, r.stderr
    assert "recorded: %d halton pairs, %d motion decisions, %d frames, %d x %d means" % (
        g["h_idx"].size, g["m_out"].size, g["q_in"].shape[0], g["a_src"].shape[0], g["a_src"].shape[1]) in r.stdout


def test_fixture_covers_what_it_must():
    g = fixture()
    assert set(g) == {"h_idx", "h_out", "m_in", "m_out", "q_in", "q_out", "a_src", "a_acc", "a_bytes"}
    assert os.path.getsize(GOLDEN) < 256 * 1024
    # Halton: 0 .. 4096 and a few up to 2^31 - 2
    idx = g["h_idx"]
    assert np.array_equal(idx[:4097], np.arange(4097)) and idx.max() == 2 ** 31 - 2 and (idx[4097:] > 4096).all() and idx.size >= 4097 + 8
    assert not np.isnan(g["h_out"]).any() and (g["h_out"] > 0).all() and (g["h_out"] <= 1).all()
    # motion: both outcomes at, one ulp under and one ulp over both thresholds
    m, out = g["m_in"], g["m_out"]
    assert set(np.unique(out)) == {0, 7}
    with np.errstate(invalid="ignore"):
        d_o, d_b = m[:, 12:15] - m[:, 0:3], m[:, 15:24] - m[:, 3:12]
        for eps, d, other in ((A.POS_EPS, d_o, d_b), (A.ROT_EPS, d_b, d_o)):
            alone = (other == 0).all(axis=1) & ((d != 0).sum(axis=1) == 1)
            a = np.abs(d).max(axis=1)
            for x, reset in ((eps, False), (np.nextafter(eps, F(0)), False), (np.nextafter(eps, F(1)), True)):
                k = alone & (a == x)
                assert k.sum() >= 2 and ((out[k] == 0) == reset).all(), (eps, x)
    both = (np.abs(d_o).max(axis=1) > 0.5) & (np.abs(d_b).max(axis=1) > 0.1)
    assert both.any() and (out[both] == 0).all()                                          # a rotation hidden by a move
    nan_pose = np.isnan(m).any(axis=1)
    assert nan_pose.sum() >= 12 and (out[nan_pose] == 7).sum() >= 6 and (out[nan_pose] == 0).sum() >= 1   # (another column may still decide)
    nan_origin, still = np.isnan(m[:, 12:15]).any(axis=1) | np.isnan(m[:, 0:3]).any(axis=1), (d_b == 0).all(axis=1)
    assert (nan_origin & still).sum() >= 6 and (out[nan_origin & still] == 7).all()       # a NaN origin alone resets nothing
    assert (out[nan_origin & ~still] == 0).any()                                           # ... and the rotation is still looked at
    # scripted frames: AA off and on, max_samples 0, 1, 3 and a negative one, frames shown raw, resolution changes
    q, o = g["q_in"], g["q_out"]
    assert np.unique(q[:, 0]).size >= 10 and (q[:, 1] == 0).any() and (q[:, 1] == 1).any()
    assert {0, 1, 3} <= set(q[:, 2].view(np.int32).tolist()) and (q[:, 2].view(np.int32) < 0).any()
    assert (o[:, 3] == 0).sum() >= 20 and (o[:, 3] == 1).sum() >= 60 and o[:, 0].max() >= 39 and np.unique(q[:, 3]).size >= 3
    passed = (q[:, 1] == 1) & (o[:, 3] == 0)                                              # max_samples reached: raw and un-jittered
    assert passed.sum() >= 10 and (o[passed, 1] == F(0.5).view(np.uint32)).all() and (o[passed, 2] == F(0.5).view(np.uint32)).all()
    # running means: 64 samples of a few hundred values of every kind
    src, acc = g["a_src"], g["a_acc"]
    assert src.shape == acc.shape == g["a_bytes"].shape == (64, 256)
    fin = np.isfinite(src)
    assert ((src >= 0) & (src <= 1)).sum() >= 8000 and (fin & (src > 1)).sum() >= 1000 and (src < 0).sum() >= 1000
    assert (bits(src) == 0x80000000).sum() >= 64 and (bits(src) == 0).sum() >= 64
    sub = fin & (src != 0) & (np.abs(src) < np.finfo(F).tiny)
    assert sub.sum() >= 500 and (fin & (acc != 0) & (np.abs(acc) < np.finfo(F).tiny)).sum() >= 300
    big = np.finfo(F).max
    assert ((src[:-1] == big) & (src[1:] == -big)).any() and np.isinf(acc[:, 216:220]).any() and np.isnan(acc[:, 216:220]).any()
    assert (src == np.inf).sum() >= 6 and (src == -np.inf).sum() >= 6 and np.isnan(src).sum() >= 12
    assert np.isnan(src[0]).sum() >= 2 and (bits(src[0]) == 0x80000000).sum() >= 2 and np.isinf(src[0]).sum() >= 2   # what the first copy must keep
    # the NaNs are where they must be: in N_NAN_TUPLES columns of the means, and in no other array
    assert np.isnan(acc).any(axis=0).sum() == N_NAN_TUPLES
    assert not (np.isnan(acc).any(axis=0) & np.isfinite(src).all(axis=0) & (np.abs(src) < 1e30).all(axis=0)).any()


def test_halton_equals_the_reference_bit_for_bit():
    g = fixture()
    got = np.array([A.halton_jitter(int(i)) for i in g["h_idx"]], dtype=F)
    np.testing.assert_array_equal(bits(got), bits(g["h_out"]))
    lib = np.array([capi.halton_jitter(int(i)) for i in g["h_idx"][::7]], dtype=F)
    np.testing.assert_array_equal(bits(lib), bits(g["h_out"][::7]))
    with pytest.raises(ValueError):
        A.halton_jitter(0x7FFFFFFF)


def test_motion_decisions_equal_the_reference():
    g = fixture()
    for k, (row, want) in enumerate(zip(g["m_in"], g["m_out"])):
        st = A.new_state(True, 256)
        st["prev_origin"], st["prev_basis"], st["count"] = row[0:3].copy(), row[3:12].reshape(3, 3).copy(), 7
        A.begin_frame(st, row[12:15], row[15:24].reshape(3, 3))
        assert st["count"] == want == st["sample_index"], k


def _replay(begin, end, fresh, read):
    g = fixture()
    seq, st, out = None, None, []
    for w in g["q_in"]:
        if w[0] != seq:
            seq, st = w[0], fresh()
        pose = w[4:16].view(F)
        st = begin(st, int(w[1]), int(w[2:3].view(np.int32)[0]), pose[0:3], pose[3:12].reshape(3, 3))
        first = read(st)[:3]
        st = end(st, int(w[3]))
        out.append(first + read(st)[3:])
    return np.array(out, dtype=np.uint32)


def test_frame_scripts_equal_the_reference_restated_and_in_the_library():
    g = fixture()

    def begin_np(st, aa, mx, o, b):
        st["aa_enabled"], st["max_samples"] = bool(aa), mx
        return A.begin_frame(st, o, b)

    def read_np(st):
        return [st["sample_index"], int(F(st["jitter"][0]).view(np.uint32)), int(F(st["jitter"][1]).view(np.uint32)), st["accumulate"], st["n_prior"], st["count"]]

    np.testing.assert_array_equal(_replay(begin_np, A.end_frame, A.new_state, read_np), g["q_out"])

    def begin_lib(st, aa, mx, o, b):
        st.aa_enabled, st.max_samples = aa, mx
        return capi.accum_begin_frame(st, o, b)

    def read_lib(st):
        return [st.sample_index, int(F(st.jitter_x).view(np.uint32)), int(F(st.jitter_y).view(np.uint32)), st.accumulate, st.n_prior, st.count]

    np.testing.assert_array_equal(_replay(begin_lib, capi.accum_end_frame, lambda: capi.accum_state(False, 0), read_lib), g["q_out"])


def test_running_means_and_bytes_equal_the_reference_bit_for_bit():
    g = fixture()
    src, want, want8 = g["a_src"], g["a_acc"], g["a_bytes"]
    acc = None
    got = np.zeros_like(want)
    for k in range(src.shape[0]):
        acc = A.accumulate(acc, src[k], k)
        got[k] = acc
    nan = np.isnan(want)
    assert np.isnan(got[nan]).all()                                                        # NaN in both
    assert nan.any(axis=0).sum() == N_NAN_TUPLES
    np.testing.assert_array_equal(bits(got)[~nan], bits(want)[~nan])
    np.testing.assert_array_equal(bits(got[0]), bits(src[0]))                              # the first sample is copied, payload and sign kept
    np.testing.assert_array_equal(Ch.to_rgba8(want), want8)
    np.testing.assert_array_equal(Ch.to_rgba8(got), want8)
    # the frame form on pixels: the same numbers
    a4, b4 = A.accumulate_frame(want[4].reshape(-1, 4), A.SRC_RGBA, src[5].reshape(-1, 4), 5)
    keep = ~np.isnan(want[5])
    np.testing.assert_array_equal(bits(a4).reshape(-1)[keep], bits(want[5])[keep])
    np.testing.assert_array_equal(b4.reshape(-1), want8[5])


def test_fused_samples_are_the_finishing_passes():
    from messyerraytracer_amd import path as P
    rng = np.random.default_rng(9)
    lit = np.zeros((512, 4), F)
    lit[:, :3], lit[:, 3] = rng.uniform(0, 4, (512, 3)), rng.integers(0, 2, 512)
    state = P.init_state(512)
    state["radiance"] = lit[:, :3]
    acc = rng.uniform(0, 1, (512, 4)).astype(F)
    for mode in range(5):
        for kind, src, fin in ((A.SRC_LIT, lit, Ch.finish_color(lit, mode)), (A.SRC_PATH_STATE, state, P.path_finish(state, mode))):
            for n in (0, 3):
                got, got8 = A.accumulate_frame(acc, kind, src, n, mode)
                want, want8 = A.accumulate_frame(acc, A.SRC_RGBA, fin, n)
                np.testing.assert_array_equal(bits(got), bits(want))
                np.testing.assert_array_equal(got8, want8)
