"""Known answers that pin tests/ray_mesh_reference.py: the fp64 oracle and the
fp32 emulation of csrc/ray_tri_pair.h must both give them.  No GPU, no library."""
import numpy as np
import pytest

from tests import ray_mesh_reference as RR

UNIT = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], np.float32)
TRI = np.array([[0, 1, 2]], np.int32)


def _both(v, f, o, d, **kw):
    """``(t, face)`` of the oracle and of the emulation, asserted to agree on the mask and
    the face; returns the oracle's and the emulation's t."""
    o, d = np.atleast_2d(np.asarray(o, np.float32)), np.atleast_2d(np.asarray(d, np.float32))
    t64, f64 = RR.ray_mesh_ref(v, f, o, d, **kw)
    t32, f32, bary = RR.ray_mesh_emul(v, f, o, d, **kw)
    assert np.array_equal(f64, f32.astype(np.int64)), (f64, f32)
    assert np.array_equal(np.isinf(t64), np.isinf(t32))
    return t64, t32, f32, bary


def test_axis_ray_on_the_unit_triangle_is_exact():
    t64, t32, face, bary = _both(UNIT, TRI, [0.25, 0.25, 2.0], [0, 0, -1])
    assert t64[0] == 2.0 and t32[0] == np.float32(2.0) and face[0] == 0
    assert np.array_equal(bary[0], np.float32([0.5, 0.25, 0.25]))
    # from below: the other side of the triangle counts too
    t64, t32, face, _ = _both(UNIT, TRI, [0.25, 0.25, -3.0], [0, 0, 1])
    assert t64[0] == 3.0 and t32[0] == np.float32(3.0) and face[0] == 0


def test_shared_edge_of_two_coplanar_triangles_hits_the_lower_index():
    v = np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0]], np.float32)
    for f in ([[0, 1, 2], [0, 2, 3]], [[0, 2, 3], [0, 1, 2]], [[0, 1, 2], [2, 0, 3]]):
        f = np.array(f, np.int32)
        t64, t32, face, _ = _both(v, f, [0.5, 0.5, 1.0], [0, 0, -1])
        assert t64[0] == 1.0 and t32[0] == np.float32(1.0) and face[0] == 0
    # and a corner shared by both
    t64, t32, face, _ = _both(v, np.array([[0, 1, 2], [0, 2, 3]], np.int32), [0, 0, 1.0],
                              [0, 0, -1])
    assert t32[0] == np.float32(1.0) and face[0] == 0


@pytest.mark.parametrize("o,d,v", [
    ([0.25, 0.25, 1.0], [1, 0, 0], UNIT),                                  # parallel, above
    ([0.25, 0.25, 0.0], [1, 1, 0], UNIT),                                  # in the plane
    ([0.25, 0.25, 1.0], [0, 0, 1], UNIT),                                  # behind the origin
    ([0.25, 0.25, 1.0], [0, 0, 0], UNIT),                                  # d = 0
    ([0.5, 0.0, 1.0], [0, 0, -1], np.array([[0, 0, 0], [1, 0, 0], [0.5, 0, 0]], np.float32)),
    ([0.0, 0.0, 1.0], [0, 0, -1], np.zeros((3, 3), np.float32)),           # a point triangle
    ([2.0, 2.0, 1.0], [0, 0, -1], UNIT)])                                  # beside it
def test_misses(o, d, v):
    t64, t32, face, bary = _both(v, TRI, o, d)
    assert np.isinf(t64[0]) and np.isinf(t32[0]) and t32[0] > 0 and face[0] == -1
    assert np.array_equal(bary[0], np.zeros(3, np.float32))


def test_non_finite_rays_miss_in_the_emulation():
    o = np.array([[np.inf, 0.25, 1], [0.25, np.nan, 1], [0.25, 0.25, 1], [0.25, 0.25, 1]],
                 np.float32)
    d = np.array([[0, 0, -1], [0, 0, -1], [0, 0, -np.inf], [np.nan, 0, -1]], np.float32)
    t32, face, _ = RR.ray_mesh_emul(UNIT, TRI, o, d)
    assert np.all(np.isinf(t32)) and np.all(face == -1)


def test_t_range_is_inclusive():
    o, d = [0.25, 0.25, 2.0], [0, 0, -1]
    for kw, hit in (({"t_min": 2.0}, True), ({"t_max": 2.0}, True),
                    ({"t_min": 2.0, "t_max": 2.0}, True), ({"t_min": 2.0000002}, False),
                    ({"t_max": 1.9999999}, False)):
        t64, t32, face, _ = _both(UNIT, TRI, o, d, **kw)
        assert (face[0] == 0) == hit and (t32[0] == np.float32(2.0)) == hit
    # the bound picks the second of two stacked triangles
    v = np.concatenate([UNIT, UNIT + np.float32([0, 0, -1])])
    f = np.array([[0, 1, 2], [3, 4, 5]], np.int32)
    t64, t32, face, _ = _both(v, f, o, d, t_min=2.5)
    assert t32[0] == np.float32(3.0) and face[0] == 1


def test_doubling_the_direction_halves_t():
    rng = np.random.default_rng(0)
    o, d = RR.random_rays(200, seed=1)
    o *= np.float32(0.3)
    v = (rng.uniform(-1, 1, (3, 3)) * [1, 1, 0.1]).astype(np.float32)
    t1, f1, b1 = RR.ray_mesh_emul(v, TRI, o, d)
    t2, f2, b2 = RR.ray_mesh_emul(v, TRI, o, d * np.float32(2))
    assert (f1 >= 0).sum() >= 20
    # a power of two scales Sz exactly and leaves Sx, Sy alone: t halves bit for bit
    assert np.array_equal(f1, f2) and np.array_equal(t2, t1 * np.float32(0.5))
    assert np.array_equal(b1, b2)
    r1, _ = RR.ray_mesh_ref(v, TRI, o, d)
    r2, _ = RR.ray_mesh_ref(v, TRI, o, d.astype(np.float64) * 2)
    ok = np.isfinite(r1)
    assert np.array_equal(np.isfinite(r2), ok) and np.allclose(r2[ok], r1[ok] / 2, rtol=1e-14)


def test_ray_segment_distance_known_answers():
    d = RR.ray_segment_distance
    assert d([0, 0, 0], [1, 0, 0], [2, 3, 0], [2, 3, 5]) == pytest.approx(3.0)     # skew
    assert d([0, 0, 0], [1, 0, 0], [-2, 0, 1], [-2, 0, 4]) == pytest.approx(5 ** 0.5)  # behind
    assert d([0, 0, 0], [1, 0, 0], [1, 1, 0], [3, 1, 0]) == pytest.approx(1.0)     # parallel
    assert d([0, 0, 0], [0, 0, 2], [1, 1, 1], [-1, -1, 1]) == pytest.approx(0.0)   # crossing
    assert d([0, 0, 0], [0, 0, 1], [1, 0, 5], [1, 0, 5]) == pytest.approx(1.0)     # a point


def test_emulation_tracks_the_oracle_on_random_rays():
    """The accuracy statement the GPU parity bound rests on: on 2000 random rays at an
    icosphere the emulation's t is within the bound without its factor 8 times 2."""
    from tests import mesh_sdf_reference as M
    v, f = M.icosphere(2)
    o, d = RR.random_rays(2000, seed=5)
    t64, f64 = RR.ray_mesh_ref(v, f, o, d)
    t32, f32, _ = RR.ray_mesh_emul(v, f, o, d)
    both = np.isfinite(t64) & np.isfinite(t32)
    assert both.sum() > 500 and (np.isfinite(t64) != np.isfinite(t32)).sum() <= 2
    n = RR.face_normals(v, f)[f64[both]]
    ratio = np.abs(t32[both] - t64[both]) / RR.t_bound(o[both], d[both], t64[both], n)
    assert ratio.max() <= 2 / 8, ratio.max()
