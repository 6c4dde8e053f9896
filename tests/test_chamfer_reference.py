"""Known answers for tests/chamfer_reference.py, the fp64 reference of the Chamfer kernels."""
import numpy as np

from tests import chamfer_reference as C


def test_a_cloud_against_itself():
    rng = np.random.default_rng(0)
    a = rng.uniform(-1, 1, (500, 3))
    d2, idx = C.nearest(a, a)
    assert np.array_equal(d2, np.zeros(500)) and np.array_equal(idx, np.arange(500))
    assert C.directed(a, a) == 0.0
    assert np.array_equal(C.chamfer_matrix(a[None]), np.zeros((1, 1)))


def test_two_single_points():
    a, b = np.array([[0.25, -0.5, 1.0]]), np.array([[-0.75, 0.5, 0.5]])
    want = 1.0 + 1.0 + 0.25
    d2, idx = C.nearest(a, b)
    assert d2[0] == want and idx[0] == 0
    assert C.directed(a, b) == want and C.directed(b, a) == want
    assert C.chamfer_matrix(a[None], b[None])[0, 0] == 2 * want


def test_translated_unit_lattice():
    g = np.arange(-3, 4, dtype=np.float64)
    lat = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    t = np.array([0.25, -0.125, 0.375])           # |t| < 1/2: every point's nearest is its own
    d2, idx = C.nearest(lat + t, lat)
    assert np.array_equal(idx, np.arange(len(lat)))
    assert np.array_equal(d2, np.full(len(lat), float(t @ t)))
    assert C.directed(lat + t, lat) == float(t @ t) == C.directed(lat, lat + t)
    assert C.chamfer_matrix((lat + t)[None], lat[None])[0, 0] == 2 * float(t @ t)


def test_tie_goes_to_the_smaller_index():
    c = np.array([[1.0, 0, 0], [-1.0, 0, 0], [0, 1.0, 0], [1.0, 0, 0], [0, 0, 0.5]])
    q = np.array([[0.0, 0, 0], [1.0, 0, 0], [0, 0.5, 0.25]])
    d2, idx = C.nearest(q, c)
    # the origin: 0.25 to the last point alone; (1,0,0): points 0 and 3 tie at 0;
    # (0, .5, .25): points 2 and 4 tie at 0.3125
    assert idx.tolist() == [4, 0, 2] and d2.tolist() == [0.25, 0.0, 0.3125]
    d2, idx = C.nearest(np.zeros((1, 3)), c[:4])
    assert idx[0] == 0 and d2[0] == 1.0            # four points at distance 1
    old = C.CHUNK
    try:
        C.CHUNK = 4                                 # the chunking changes nothing
        d2b, idxb = C.nearest(q, c)
    finally:
        C.CHUNK = old
    assert idxb.tolist() == [4, 0, 2] and d2b.tolist() == [0.25, 0.0, 0.3125]


def test_directed_is_not_symmetric_and_matrix_shapes():
    a = np.array([[[0.0, 0, 0], [1.0, 0, 0]], [[0.0, 0, 0], [0.0, 0, 0]]])   # [2, 2, 3]
    b = np.array([[[0.0, 0, 0]]])                                           # [1, 1, 3]
    d_ab, d_ba = C.directed_matrix(a, b), C.directed_matrix(b, a)
    assert d_ab.tolist() == [[0.5], [0.0]] and d_ba.tolist() == [[0.0, 0.0]]
    assert C.chamfer_matrix(a, b).tolist() == [[0.5], [0.0]]
    within = C.chamfer_matrix(a)
    assert within.tolist() == [[0.0, 0.5], [0.5, 0.0]]
