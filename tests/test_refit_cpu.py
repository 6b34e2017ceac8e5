"""Refit without a device: the library exports mrt_refit_scene / mrt_refit_instanced_scene, both refuse a null context before any
device work, and synth.deform -- the animation frames the refit tests and tools/bench_refit.py share -- is deterministic."""
import numpy as np

from messyerraytracer_amd import capi, synth


def test_exports():
    L = capi.load()
    for s in ("mrt_refit_scene", "mrt_refit_instanced_scene"):
        assert hasattr(L, s) and s in capi.SYMBOLS


def test_null_context_is_invalid():
    L = capi.load()
    tris = capi.make_triangles(synth.soup(4, 1.0, 1))
    assert L.mrt_refit_scene(None, tris.ctypes.data_as(capi.C.c_void_p), 4, 0) == capi.ERR_INVALID
    assert L.mrt_refit_scene(None, None, 0, 0) == capi.ERR_INVALID
    local, inst = synth.room()
    assert L.mrt_refit_instanced_scene(None, local.ctypes.data_as(capi.C.c_void_p), local.shape[0],
                                       inst.ctypes.data_as(capi.C.c_void_p), inst.shape[0], 0) == capi.ERR_INVALID


def test_deformation_is_deterministic_and_smooth():
    v = synth.soup(500, 0.5, 3)
    a = synth.deform(v, 0.05, 0.7, seed=4)
    assert a.dtype == np.float32 and a.shape == v.shape
    assert a.tobytes() == synth.deform(v, 0.05, 0.7, seed=4).tobytes()
    assert a.tobytes() != synth.deform(v, 0.05, 0.8, seed=4).tobytes()     # the phase moves the frame
    assert a.tobytes() != synth.deform(v, 0.05, 0.7, seed=5).tobytes()     # the seed picks the field
    assert synth.deform(v, 0.0, 0.7, seed=4).tobytes() == v.tobytes()
    step = np.abs(a - v).max()
    assert 0.0 < step <= 0.05 * 1.0001
    # one field: a vertex two triangles share moves alike in both (a closed mesh stays closed)
    local, _ = synth.room()
    d = synth.deform(local, 0.1, 1.0, seed=1)
    p, q = local.reshape(-1, 3), d.reshape(-1, 3)
    _, first, inverse = np.unique(p, axis=0, return_index=True, return_inverse=True)
    assert np.array_equal(q, q[first][inverse.reshape(-1)])
