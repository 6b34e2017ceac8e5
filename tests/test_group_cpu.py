"""mrt_group_* (several devices from one process): the host-side span logic and the error behaviour without a device."""
import ctypes as C

import pytest

from conftest import gpu_present
from messyerraytracer_amd import capi, sharded
from oracle import digests
import numpy as np


@pytest.mark.parametrize("rows", [1, 7, 8, 100, 8192, 8191])
@pytest.mark.parametrize("n", [1, 2, 3, 8])
def test_row_blocks_tile_the_grid_and_match_the_torch_path(built, rows, n):
    blocks = [capi.group_row_block(r, n, rows) for r in range(n)]
    assert blocks[0][0] == 0 and blocks[-1][1] == rows
    for (a0, a1), (b0, b1) in zip(blocks, blocks[1:]):
        assert a1 == b0 and a0 <= a1
    assert blocks == [sharded.row_block(r, n, rows) for r in range(n)]   # the same split as the one-process-per-GPU path


def test_group_without_a_device_fails_loudly(built):
    L = capi.load()
    h = C.c_void_p()
    assert L.mrt_group_create(0, None, None, C.byref(h)) == capi.ERR_INVALID
    assert L.mrt_group_create(1, None, None, None) == capi.ERR_INVALID
    assert L.mrt_group_size(None) == 0 and L.mrt_group_context(None, 0) is None
    assert L.mrt_group_cast_grid(None, None, 0, 0, None, 0, 0, 0) == capi.ERR_INVALID
    L.mrt_group_destroy(None)
    if not gpu_present():
        assert L.mrt_group_create(2, None, None, C.byref(h)) == capi.ERR_NO_DEVICE   # never a CPU fallback
        with pytest.raises(capi.MrtError):
            capi.Group([0])


def test_digests_are_additive_over_row_blocks():
    """The digest a rank computes over its block (global ray indices) adds up to the digest of the whole grid."""
    rng = np.random.default_rng(5)
    n = 10000
    prim = rng.integers(-1, 1 << 20, n).astype(np.int32)
    t = rng.random(n).astype(np.float32)
    whole = digests.digest_columns(prim, t)
    acc = dict(rays=0, hit_count=0, prim_xor=0, prim_hash=0, t_hash=0, sum_t=0.0)
    for a, b in ((0, 1234), (1234, 7000), (7000, n)):
        acc = digests.combine(acc, digests.digest_columns(prim[a:b], t[a:b], a))
    assert digests.same(acc, whole)
    swapped = prim.copy(); swapped[[3, 4]] = swapped[[4, 3]]
    if swapped[3] != swapped[4]:
        assert not digests.same(digests.digest_columns(swapped, t), whole)   # position-dependent: a permutation is seen


def test_committed_full_digests_are_consistent():
    import json, os
    from conftest import GOLDEN
    full = json.load(open(os.path.join(GOLDEN, "full_digests.json")))
    assert set(full) >= {"C2", "C3", "C4", "C5"}
    for name in ("C2", "C3", "C5"):
        acc = dict(rays=0, hit_count=0, prim_xor=0, prim_hash=0, t_hash=0, sum_t=0.0)
        for b in full[name]["row_blocks"]:
            acc = digests.combine(acc, b)
        assert digests.same(acc, full[name]), name
    # C2's digest again from the oracle (a few seconds): the file is what make_full_digests.py computes
    from messyerraytracer_amd import synth
    from oracle import pyoracle as po
    cfg = synth.CONFIGS["C2"]
    w, h = cfg["grid"]
    hits = po.OracleScene(synth.scene_vertices(cfg)).trace(po.grid_rays(cfg["origin"], cfg["forward"], w, h, cfg["fov"]))
    assert digests.same(digests.digest_records(hits), full["C2"])
