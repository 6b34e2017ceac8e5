"""Two-level refit without a device: the library exports mrt_refit_two_level_scene, the bindings list it, and a null context or a
null argument is refused before any device work."""
from messyerraytracer_amd import capi, synth


def test_export():
    L = capi.load()
    assert hasattr(L, "mrt_refit_two_level_scene") and "mrt_refit_two_level_scene" in capi.SYMBOLS
    assert hasattr(capi.Context, "refit_two_level_scene")


def test_null_arguments_are_invalid():
    L = capi.load()
    local, inst = synth.room()
    v, i = local.ctypes.data_as(capi.C.c_void_p), inst.ctypes.data_as(capi.C.c_void_p)
    n_mesh, n_inst = local.shape[0], inst.shape[0]
    assert L.mrt_refit_two_level_scene(None, v, n_mesh, i, n_inst, 0) == capi.ERR_INVALID
    assert L.mrt_refit_two_level_scene(None, None, n_mesh, i, n_inst, 0) == capi.ERR_INVALID
    assert L.mrt_refit_two_level_scene(None, v, n_mesh, None, n_inst, 0) == capi.ERR_INVALID
    assert L.mrt_refit_two_level_scene(None, None, 0, None, 0, 0) == capi.ERR_INVALID
