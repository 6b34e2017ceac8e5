"""The oracle's two-level walk on mirrored, non-uniformly scaled and sheared instances (tests/affine_scene.py), pinned against a
float64 brute force over the flattened world triangles: with a general basis the mesh-space direction has a different length per
axis while t stays world-parameterised, and normalize(basis . n_mesh) -- the reference's record normal, scene_tlas.h:245 -- is no
longer the flattened triangle's normal.  This file makes the oracle the specification the device is then held to bit for bit
(tests/test_affine_instances_gpu.py).  No device.

Bounds: prim_id differences at most max(2, n // 10000) per cast, each explained in float64 (parity.explain_mismatch); on common hits
|dt| <= TWO_LEVEL_T_REL_OUTLIER max(t, 1) for all and <= 1e-5 max(t, 1) for all but TWO_LEVEL_OUTLIER_FRACTION; the record normal
within 1e-6 (absolute, per component) of float64 normalize(B n_mesh) -- float32 carries 6e-8 per operation through a cross product,
a normalisation, a 3x3 product and a second normalisation.

Measured (40 instances, 11 875 flattened triangles; grids 96x72 and 61x37, 4 000 incoherent rays; masks 0xFFFFFFFF, 0x1, 0x4):
prim_id differences 0 in every cast; |dt| / max(t, 1) at most 4.0e-6 (none above 1e-5); normal error at most 2.7e-7; hits of the
96x72 grid by class 680 / 790 / 379 / 564 / 703; singular values 0.381 .. 1.810; of the (instance, 8x8 tile) pairs of that grid 503
have mesh-space directions of one octant and 62 of several (2x2-pixel pieces: 5 856 and 125).  Dot product of the flat walk's normal
with the two-level normal of the same triangle, 96x72 grid: rigid 0.9999999 .. 1, mirror -1 .. -0.9999999, nonuniform 0.464 .. 0.9979,
shear 0.663 .. 0.9984, mirror_nonuni -0.9977 .. -0.461."""
import numpy as np
import pytest

import affine_scene as A
import layout_check as lc
import parity
from messyerraytracer_amd import capi
from oracle import pyoracle as po

RAY_SETS = ("grid", "clipped", "incoherent")


class Results:
    """every cast of the file, computed once: per (ray set, mask) the rays, the brute force, the two-level and the flat oracle walk"""

    def __init__(self):
        self.sc = A.scene()
        self.two = po.OracleTwoLevelScene(self.sc.local, self.sc.inst)
        self.flat = po.OracleScene(self.sc.world, self.sc.ids, self.sc.layers)
        self.rays = {"grid": self.sc.grid_rays(*A.GRID), "clipped": self.sc.grid_rays(*A.CLIPPED), "incoherent": self.sc.incoherent_rays(4000)}
        self._cast = {}

    def cast(self, name, mask):
        if (name, mask) not in self._cast:
            rays = self.rays[name]
            self._cast[name, mask] = (rays, self.sc.brute(rays, mask), self.two.trace(rays, query_mask=mask),
                                      self.flat.trace(rays, query_mask=mask))
        return self._cast[name, mask]


@pytest.fixture(scope="module")
def res():
    return Results()


def test_the_scene_is_what_it_says(res):
    sc = res.sc
    sv = sc.singular_values()
    print(f"singular values {sv.min():.4g} .. {sv.max():.4g}")
    assert A.SV_RANGE[0] <= sv.min() and sv.max() <= A.SV_RANGE[1]
    assert np.array_equal(np.bincount(sc.cls), np.full(len(A.CLASSES), A.N_INSTANCES // len(A.CLASSES)))
    det = np.linalg.det(sc.basis64())
    mirrored = np.isin(sc.cls, [A.CLASSES.index("mirror"), A.CLASSES.index("mirror_nonuni")])
    assert ((det < 0) == mirrored).all()
    rigid = sv[sc.cls == A.CLASSES.index("rigid")]
    assert np.abs(rigid - 1.0).max() < 1e-6
    for name in A.DISTORTED:                      # no distorted basis is a rotation times one scale
        s = sv[sc.cls == A.CLASSES.index(name)]
        assert (s.max(axis=1) / s.min(axis=1) > 1.2).all(), name
    assert set(np.unique(sc.inst["layers"])) == {1, 2, 4}
    assert len({(c, m) for c, m in zip(sc.cls, sc.mesh)}) == 25, "every mesh under every class"
    rigid_set = sc.rigid_instances()
    assert np.abs(np.linalg.svd(rigid_set["basis"].astype(np.float64).reshape(-1, 3, 3), compute_uv=False) - 1.0).max() < 1e-6
    # the packet walk's octant choice has both kinds of work: whole 8x8 tiles, and the 2x2-pixel pieces small grids are cast in
    for tile in (8, 2):
        uniform, mixed = sc.tile_octants(*A.GRID, tile=tile)
        print(f"{tile}x{tile} tiles: {uniform} (instance, tile) pairs of one octant, {mixed} of several")
        assert uniform > 0 and mixed > 0


@pytest.mark.parametrize("name", RAY_SETS)
def test_oracle_two_level_walk_against_float64_brute_force(res, name):
    sc = res.sc
    for mask in A.MASKS:
        rays, ref, got, _ = res.cast(name, mask)
        n = rays.shape[0]
        assert int((got["prim_id"] >= 0).sum()) > 100
        diff = np.nonzero(got["prim_id"] != ref["prim_id"])[0]
        same = got["prim_id"] == ref["prim_id"]
        hit = same & (got["prim_id"] >= 0)
        ta, tr = got["t"][hit].astype(np.float64), ref["t"][hit]
        rel = np.abs(ta - tr) / np.maximum(tr, 1.0)
        print(f"{name} mask={mask:#x}: {diff.size} prim_id differences of {n}; {int(hit.sum())} common hits, |dt| / max(t, 1) at most "
              f"{rel.max():.3g}, {int((rel > 1e-5).sum())} above 1e-5")
        assert diff.size <= max(2, n // 10000)
        for i in diff:
            assert parity.explain_mismatch(sc.tris, rays[i], int(got["prim_id"][i]), int(ref["prim_id"][i])), f"{name} mask={mask:#x} ray {i}"
        assert (rel <= parity.TWO_LEVEL_T_REL_OUTLIER).all()
        assert (rel > 1e-5).sum() <= parity.TWO_LEVEL_OUTLIER_FRACTION * hit.sum()
        miss = same & ~hit
        assert miss.any() and np.array_equal(got["t"][miss], rays["t_max"][miss])           # misses carry t_max
        assert np.array_equal(got["hit_layers"][hit], sc.layers[got["prim_id"][hit]])
        assert (got["hit_layers"][hit] & np.uint32(mask)).all()
        occluded = res.two.trace(rays, query_mask=mask, any_hit=True)
        assert np.array_equal(occluded["prim_id"] >= 0, got["prim_id"] >= 0)                # any-hit: "a closest hit exists"
    # the intervals that end or begin inside the scene decide something
    if name == "incoherent":
        rays, ref, got, _ = res.cast(name, 0xFFFFFFFF)
        full = rays.copy()
        full["t_min"], full["t_max"] = np.float32(0.001), np.float32(3.0e38)
        assert (res.two.trace(full)["prim_id"] != got["prim_id"]).sum() > 20


def test_every_class_is_hit(res):
    _, _, got, _ = res.cast("grid", 0xFFFFFFFF)
    hits = np.bincount(res.sc.class_of_prim(got["prim_id"][got["prim_id"] >= 0]), minlength=len(A.CLASSES))
    print("hits of the 96x72 grid by class:", dict(zip(A.CLASSES, hits.tolist())))
    assert (hits >= 100).all()


def test_the_normal_is_the_references(res):
    """hits["normal"] is normalize(B n_mesh), n_mesh the normalised cross product of the mesh-space edges -- in every class"""
    worst = 0.0
    for name in RAY_SETS:
        for mask in A.MASKS:
            _, _, got, _ = res.cast(name, mask)
            hit = got["prim_id"] >= 0
            err = np.abs(got["normal"][hit].astype(np.float64) - res.sc.mesh_normal64(got["prim_id"][hit])).max(axis=1)
            cl = res.sc.class_of_prim(got["prim_id"][hit])
            assert all((cl == c).any() for c in range(len(A.CLASSES)))
            worst = max(worst, float(err.max()))
            assert err.max() <= 1e-6, f"{name} mask={mask:#x}"
    print(f"record normal against float64 normalize(B n_mesh): at most {worst:.3g}")


def test_the_normal_against_the_flattened_triangles_normal(res):
    """Recorded, not judged: under a mirror the two conventions are opposite, under non-uniform scale or shear the record normal is
    not perpendicular to the world triangle -- but on its side: (B n) . (B^-T n) = |n|^2 > 0."""
    _, _, got, flat = res.cast("grid", 0xFFFFFFFF)
    for name, (lo, hi) in A.normal_relation(res.sc, got, flat).items():
        print(f"{name}: dot {lo:.7g} .. {hi:.7g}")


def test_host_preparation_is_a_valid_layout(built, res):
    prepared = capi.two_level_prepare_host(res.sc.local, res.sc.inst)
    assert prepared["n_instances"] == A.N_INSTANCES and prepared["n_tris"] == res.sc.local.shape[0]
    findings = lc.check_two_level(prepared, res.sc.local, res.sc.inst, leaf_boxes="host")
    assert not findings, lc.summary(findings)


@pytest.mark.parametrize("which", ["one_row", "whole_basis"])
def test_singular_instances_are_still_refused(built, res, which):
    bad = res.sc.inst.copy()
    k = int(np.flatnonzero(res.sc.cls == A.CLASSES.index("shear"))[1])
    if which == "one_row":
        bad["basis"][k, 3:6] = 0.0
    else:
        bad["basis"][k] = 0.0
    with pytest.raises(ValueError):
        po.OracleTwoLevelScene(res.sc.local, bad)
    with pytest.raises(capi.MrtError) as e:
        capi.two_level_prepare_host(res.sc.local, bad)
    assert e.value.status == capi.ERR_INVALID
