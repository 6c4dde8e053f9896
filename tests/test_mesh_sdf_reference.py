"""Known answers that pin tests/mesh_sdf_reference.py, the fp64 reference of ``mesh_sdf``
(DESIGN.md §16): a closed-form box, the seven Voronoi regions of one triangle, winding numbers
of closed and open meshes, and zero-area faces."""
import numpy as np
import pytest

from tests import mesh_sdf_reference as M


@pytest.fixture(scope="module")
def pts():
    return np.random.default_rng(0).uniform(-1, 1, (2000, 3)).astype(np.float32)


def test_unit_cube_is_the_box_sdf(pts):
    v, f = M.cube_mesh()
    assert f.shape == (12, 3)
    sdf, closest, w, d = M.mesh_sdf_ref(v, f, pts)
    assert np.abs(sdf - M.box_sdf(pts)).max() <= 1e-15
    assert ((closest >= 0) & (closest < 12)).all()
    assert np.array_equal(d, np.abs(sdf))


# triangle a = (0,0,0), b = (2,0,0), c = (0,2,0): point, region, distance by hand
REGIONS = [
    ((0.5, 0.5, 0.75), "face", 0.75),
    ((-1.0, -1.0, 0.0), "A", 2 ** 0.5),
    ((3.0, -0.5, 0.0), "B", 1.25 ** 0.5),
    ((-0.5, 3.0, 0.0), "C", 1.25 ** 0.5),
    ((1.0, -2.0, 0.0), "AB", 2.0),
    ((-2.0, 1.0, 0.0), "AC", 2.0),
    ((2.0, 2.0, 1.0), "BC", 3 ** 0.5),       # foot (1, 1, 0): sqrt(1 + 1 + 1)
]


@pytest.mark.parametrize("p,region,want", REGIONS, ids=[r[1] for r in REGIONS])
def test_seven_voronoi_regions(p, region, want):
    v = np.array([[0, 0, 0], [2, 0, 0], [0, 2, 0]], np.float64)
    f = np.array([[0, 1, 2]])
    _, closest, _, d = M.mesh_sdf_ref(v, f, np.array([p]))
    assert closest[0] == 0
    assert abs(d[0] - want) <= 1e-15
    # the same answer with the corners rotated: the region names move, the distance does not
    for r in (1, 2):
        _, _, _, dr = M.mesh_sdf_ref(v, np.roll(f, r, axis=1), np.array([p]))
        assert abs(dr[0] - want) <= 1e-15


def test_ties_go_to_the_smaller_index():
    v, f = M.cube_mesh()
    # the two triangles of the +z quad share their diagonal: a point above it is equally far
    _, closest, _, _ = M.mesh_sdf_ref(v, f, np.array([[0.0, 0.0, 1.0]]))
    assert closest[0] == 2
    _, closest, _, _ = M.mesh_sdf_ref(v, np.concatenate([f, f]), np.array([[0.3, 0.1, 0.9]]))
    assert closest[0] < 12


@pytest.mark.parametrize("mesh", ["cube", "icosphere"])
def test_watertight_winding_is_one_or_zero(pts, mesh):
    v, f = M.cube_mesh() if mesh == "cube" else M.icosphere()
    assert len(f) == (12 if mesh == "cube" else 320)
    sdf, _, w, d = M.mesh_sdf_ref(v, f, pts)
    inside = sdf < 0
    assert inside.any() and (~inside).any()
    assert np.abs(w[inside] - 1).max() <= 1e-12 and np.abs(w[~inside]).max() <= 1e-12
    if mesh == "cube":
        assert np.array_equal(inside, M.box_sdf(pts) < 0)
    else:                                      # inscribed in the radius-0.8 sphere
        r = np.linalg.norm(pts.astype(np.float64), axis=1)
        assert not inside[r > 0.8].any() and inside[r < 0.75].all()


def test_open_hemisphere_winding_is_fractional(pts):
    v, f = M.hemisphere()
    assert len(f) == 152
    _, _, w, _ = M.mesh_sdf_ref(v, f, pts)
    assert -0.3 < w.min() < -0.2 and 0.8 < w.max() < 0.9
    assert ((w > 0.05) & (w < 0.95)).mean() > 0.3
    assert (np.abs(w - 0.5) < 0.05).mean() < 0.05


def test_degenerate_faces_change_nothing_and_stay_finite(pts):
    v0, f0 = M.cube_mesh()
    v, f = M.cube_with_degenerates()
    assert len(f) == 15
    sdf0, _, w0, _ = M.mesh_sdf_ref(v0, f0, pts)
    sdf, _, w, d = M.mesh_sdf_ref(v, f, pts)
    assert np.isfinite(sdf).all() and np.isfinite(w).all()
    assert np.abs(w - w0).max() <= 1e-12
    assert (d <= np.abs(sdf0)).all()           # more geometry: never farther
    # a zero-area face is its segment or point: the collinear triple spans x in [0.5, 0.875]
    a, b = np.array([0.5, 0.875, 0.875]), np.array([0.875, 0.875, 0.875])
    q = pts.astype(np.float64)
    t = np.clip((q - a) @ (b - a) / ((b - a) @ (b - a)), 0, 1)
    seg = np.linalg.norm(q - (a + t[:, None] * (b - a)), axis=1)
    assert np.abs(d - np.minimum(np.abs(sdf0), seg)).max() <= 1e-14
    # on the segment, between two corners of the collinear face
    on = np.array([[0.8125, 0.875, 0.875], [0.625, 0.875, 0.875]])
    sdf, _, w, d = M.mesh_sdf_ref(v, f, on)
    assert np.array_equal(d, [0.0, 0.0]) and np.abs(w).max() <= 1e-12
    only = M.mesh_sdf_ref(v, f[12:], on)
    assert np.array_equal(only[2], [0.0, 0.0]) and np.array_equal(only[3], [0.0, 0.0])


def test_empty_mesh_and_no_points():
    sdf, closest, w, d = M.mesh_sdf_ref(np.zeros((0, 3)), np.zeros((0, 3), int), np.zeros((3, 3)))
    assert np.isposinf(sdf).all() and (closest == -1).all() and (w == 0).all()
    v, f = M.cube_mesh()
    assert all(len(x) == 0 for x in M.mesh_sdf_ref(v, f, np.zeros((0, 3))))
