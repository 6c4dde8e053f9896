"""Nearest points, Chamfer matrices and the generation metrics on the MI355X,
against the fp64 reference tests/chamfer_reference.py.

Sizes come from the exported constants: Ta = tile_a() points of the first cloud per workgroup
tile, Cb = chunk_b() points of the second cloud per split unit.  u = 2^-24.

Bounds.  A pair is three exact-input subtractions (relative error u each, 2u after squaring)
and three more roundings of non-negative terms: |d - d_exact| <= 5u d_exact + O(u^2); the tests
hold 6u.  A matrix entry adds its minima in fp64 and rounds once to fp32: 2^-23 against the fp64
mean of the same minima, 8u against the full reference.

Measured on the MI355X (this file, printed before each assertion):
  test_accuracy_on_random_clouds      max |d2 - ref| / ref 2.97 u; the returned index always the
                                      reference's minimum
  test_matrix_against_points          0.54 u against the fp64 mean of nearest_points, 1.40 u
                                      against the fp64 reference
"""
import math

import numpy as np
import pytest
import torch

from tests import chamfer_reference as C

pytestmark = pytest.mark.gpu
U = 2.0 ** -24


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import ldm_sdf
    ldm_sdf.load_library()
    return torch.device("cuda", 0)


def _consts():
    from ldm_sdf import metrics
    return metrics.tile_a(), metrics.chunk_b()


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32).numpy()


# ------------------------------------------------------------------ 1. exactness on a lattice
_LATTICE = {}


def _lattice():
    """Queries and a cloud on the lattice k / 64, |k| <= 64 (every difference, square and sum
    exact in fp32), at the largest sizes of the test, with ties planted: duplicated cloud points
    (at a distance and at 0) whose smaller index has to win.  The reference is computed per
    size pair on slices and shared."""
    if not _LATTICE:
        Ta, Cb = _consts()
        rng = np.random.default_rng(11)
        q = rng.integers(-64, 65, (2 * Ta + 3, 3)).astype(np.float32) / 64
        c = rng.integers(-64, 65, (3 * Cb + 2, 3)).astype(np.float32) / 64
        # a tie at a distance: c[5] and c[6] are q[1] -+ 1/64 along x, and nothing is nearer
        q[1] = np.float32(0.5)
        near = np.abs(c - q[1]).max(axis=1) < 1.5 / 64
        c[near] = np.float32(-1.0)
        c[5] = q[1] - np.array([1 / 64, 0, 0], np.float32)
        c[6] = q[1] + np.array([1 / 64, 0, 0], np.float32)
        # duplicates inside every prefix the test uses, and queries that sit on them
        c[3] = c[1]
        c[Cb - 2] = c[0]
        c[Cb] = c[2]
        c[3 * Cb + 1] = c[Cb + 3]
        q[0] = c[1]
        q[Ta] = c[2]
        q[Ta + 1] = c[Cb + 3]
        _LATTICE.update(q=q, c=c, ref={})
    return _LATTICE


def _sizes():
    Ta, Cb = _consts()
    return [1, Ta - 1, Ta, Ta + 1, 2 * Ta + 3], [1, Cb - 1, Cb, Cb + 1, 3 * Cb + 2]


@pytest.mark.parametrize("qi", range(5))
@pytest.mark.parametrize("pi", range(5))
def test_exact_on_a_lattice(dev, pi, qi):
    import ldm_sdf
    L = _lattice()
    P, Q = _sizes()[0][pi], _sizes()[1][qi]
    assert P >= 1 and Q >= 1
    q, c = L["q"][:P], L["c"][:Q]
    if (P, Q) not in L["ref"]:
        L["ref"][(P, Q)] = C.nearest(q, c)
    d2_ref, idx_ref = L["ref"][(P, Q)]
    assert np.array_equal(d2_ref.astype(np.float32).astype(np.float64), d2_ref)   # exact in fp32
    if P >= 2 and Q >= 7:
        assert idx_ref[1] == 5 and d2_ref[1] == 2.0 ** -12       # the planted tie is a tie
        assert idx_ref[0] == 1 and d2_ref[0] == 0.0
    d2, idx = ldm_sdf.nearest_points(torch.from_numpy(q).to(dev), torch.from_numpy(c).to(dev),
                                     return_index=True)
    assert d2.dtype == torch.float32 and idx.dtype == torch.int32
    assert np.array_equal(_bits(d2), d2_ref.astype(np.float32).view(np.int32))
    assert np.array_equal(idx.cpu().numpy().astype(np.int64), idx_ref)
    d2_only = ldm_sdf.nearest_points(torch.from_numpy(q).to(dev), torch.from_numpy(c).to(dev))
    assert np.array_equal(_bits(d2_only), _bits(d2))             # with and without the index


# ------------------------------------------------------------------ 2. accuracy, random clouds
def _accuracy_case(dev, query, cloud, label):
    import ldm_sdf
    d2_ref, _ = C.nearest(query, cloud)
    d2, idx = ldm_sdf.nearest_points(torch.from_numpy(query).to(dev),
                                     torch.from_numpy(cloud).to(dev), return_index=True)
    d2, idx = d2.cpu().numpy().astype(np.float64), idx.cpu().numpy().astype(np.int64)
    assert idx.min() >= 0 and idx.max() < len(cloud)
    rel = np.abs(d2 - d2_ref) / d2_ref
    at_idx = C.pair_d2(query, cloud, idx) / d2_ref
    print(f"{label}: max |d2 - ref| / ref = {rel.max() / U:.3f} u, "
          f"max d(idx) / ref - 1 = {(at_idx.max() - 1) / U:.3f} u, min d2_ref = {d2_ref.min():.3e}")
    assert d2_ref.min() > 0.0
    assert np.all(np.abs(d2 - d2_ref) <= 6 * U * d2_ref)         # no point skipped
    assert np.all(at_idx <= 1 + 12 * U)


def test_accuracy_on_random_clouds(dev):
    Ta, Cb = _consts()
    n = 3 * Cb + 2
    rng = np.random.default_rng(5)
    a = rng.uniform(-1, 1, (n, 3)).astype(np.float32)
    b = (a[rng.permutation(n)] + rng.normal(0, 1e-3, (n, 3))).astype(np.float32)
    far = rng.uniform(-1, 1, (2 * Ta + 3, 3)).astype(np.float32)
    _accuracy_case(dev, a, b, "uniform -> near copy")
    _accuracy_case(dev, b, a, "near copy -> uniform")
    _accuracy_case(dev, far, a, "uniform -> uniform")


# ------------------------------------------------------------------ 3. matrix against points
_MATRIX = {}


def _matrix_case(dev):
    """Five clouds of Ta + 1 points against five of Cb + 2 (both tails, n != m), the near-surface
    pairing on the diagonal; the fp64 reference of both directions, computed once."""
    if not _MATRIX:
        Ta, Cb = _consts()
        n, m = Ta + 1, Cb + 2
        rng = np.random.default_rng(9)
        a = rng.uniform(-1, 1, (5, n, 3)).astype(np.float32)
        b = rng.uniform(-1, 1, (5, m, 3)).astype(np.float32)
        for k in range(5):
            take = rng.permutation(n)[:min(n, m)]
            b[k, :len(take)] = a[k, take] + rng.normal(0, 1e-3, (len(take), 3)).astype(np.float32)
        _MATRIX.update(a=a, b=b, ab=C.directed_matrix(a, b), ba=C.directed_matrix(b, a),
                       ta=torch.from_numpy(a).to(dev), tb=torch.from_numpy(b).to(dev))
    return _MATRIX


@pytest.mark.parametrize("R", [1, 3, 5])
@pytest.mark.parametrize("S", [1, 3, 5])
def test_matrix_against_points(dev, S, R):
    import ldm_sdf
    M = _matrix_case(dev)
    ta, tb = M["ta"][:S], M["tb"][:R]
    d_ab, d_ba_t = ldm_sdf.chamfer_matrix(ta, tb, directed=True)
    assert d_ab.shape == (S, R) and d_ba_t.shape == (S, R) and d_ab.dtype == torch.float32
    cd = ldm_sdf.chamfer_matrix(ta, tb)
    assert np.array_equal(_bits(cd), _bits(d_ab + d_ba_t))
    got_ab, got_ba = d_ab.cpu().numpy().astype(np.float64), d_ba_t.t().cpu().numpy().astype(np.float64)
    worst_pts = worst_ref = 0.0
    for s in range(S):
        for r in range(R):
            for got, x, y, ref in ((got_ab[s, r], ta[s], tb[r], M["ab"][s, r]),
                                   (got_ba[r, s], tb[r], ta[s], M["ba"][r, s])):
                mean = float(ldm_sdf.nearest_points(x, y).cpu().numpy().astype(np.float64).mean())
                worst_pts = max(worst_pts, abs(got - mean) / mean)
                worst_ref = max(worst_ref, abs(got - ref) / ref)
    print(f"S = {S}, R = {R}: against the fp64 mean of nearest_points {worst_pts / U:.3f} u, "
          f"against the fp64 reference {worst_ref / U:.3f} u")
    assert worst_pts <= 2.0 ** -23
    assert worst_ref <= 8 * U


def test_within_set_matrix(dev):
    import ldm_sdf
    M = _matrix_case(dev)
    d, d_t = ldm_sdf.chamfer_matrix(M["ta"], M["ta"], directed=True)
    w = ldm_sdf.chamfer_matrix(M["ta"])
    assert np.array_equal(_bits(w), _bits(d + d.t()))
    assert np.array_equal(_bits(d_t), _bits(d.t()))
    assert np.array_equal(_bits(w), _bits(w.t().contiguous()))
    assert np.array_equal(_bits(torch.diagonal(w)), np.zeros(5, np.int32))
    off = w.cpu().numpy()[~np.eye(5, dtype=bool)]
    assert np.all(off > 0)


# ------------------------------------------------------------------ 4. bitwise invariance
def test_entry_is_the_same_alone_permuted_and_in_every_launch_form(dev):
    import ldm_sdf
    from ldm_sdf import metrics
    Ta, Cb = _consts()
    side = max(2, math.isqrt(metrics.spread_below() - 1) + 1)    # side^2 >= spread_below
    assert side * side >= metrics.spread_below() > 5 * 3
    g = torch.Generator().manual_seed(21)
    a = (torch.rand(side, Ta + 1, 3, generator=g) * 2 - 1).to(dev)
    b = (torch.rand(side, Cb + 2, 3, generator=g) * 2 - 1).to(dev)
    big = ldm_sdf.chamfer_matrix(a, b, directed=True)            # one workgroup per entry
    small = ldm_sdf.chamfer_matrix(a[:5], b[:3], directed=True)  # each entry spread and split
    again = ldm_sdf.chamfer_matrix(a, b, directed=True)
    ps, pr = torch.tensor([3, 0, 4, 2, 1], device=dev), torch.tensor([2, 0, 1], device=dev)
    perm = ldm_sdf.chamfer_matrix(a[:5][ps], b[:3][pr], directed=True)
    for k in range(2):
        assert np.array_equal(_bits(big[k]), _bits(again[k]))    # run to run
        assert np.array_equal(_bits(big[k][:5, :3]), _bits(small[k]))
        assert np.array_equal(_bits(perm[k]), _bits(small[k][ps][:, pr]))
        for s, r in ((0, 0), (4, 2), (2, 1), (side - 1, side - 1)):
            one = ldm_sdf.chamfer_matrix(a[s:s + 1], b[r:r + 1], directed=True)
            assert np.array_equal(_bits(one[k]), _bits(big[k][s:s + 1, r:r + 1]))
    # a cloud of at most one tile: one workgroup per entry whatever the batch
    one = ldm_sdf.chamfer_matrix(a[:1, :Ta], b[:1], directed=True)
    many = ldm_sdf.chamfer_matrix(a[:, :Ta].contiguous(), b, directed=True)
    assert np.array_equal(_bits(one[0]), _bits(many[0][:1, :1]))
    assert np.array_equal(_bits(one[1]), _bits(many[1][:1, :1]))


def test_points_split_and_one_pass_agree(dev):
    import ldm_sdf
    from ldm_sdf import metrics
    Ta, Cb = _consts()
    P = metrics.split_below() + 5
    g = torch.Generator().manual_seed(22)
    q = (torch.rand(P, 3, generator=g) * 2 - 1).to(dev)
    c = (torch.rand(Cb + 2, 3, generator=g) * 2 - 1).to(dev)
    c[Cb + 1] = c[7]                                             # a tie across the split units
    q[5] = c[7]
    d2, idx = ldm_sdf.nearest_points(q, c, return_index=True)    # all of the cloud per thread
    part = 2 * Ta + 3
    d2s, idxs = ldm_sdf.nearest_points(q[:part], c, return_index=True)   # split over the cloud
    assert np.array_equal(_bits(d2[:part]), _bits(d2s)) and torch.equal(idx[:part], idxs)
    assert int(idx[5]) == 7 and float(d2[5]) == 0.0
    d2n = ldm_sdf.nearest_points(q, c)
    assert np.array_equal(_bits(d2n), _bits(d2))
    d2one, idxone = ldm_sdf.nearest_points(q[part - 1:part], c, return_index=True)
    assert np.array_equal(_bits(d2one), _bits(d2[part - 1:part])) and int(idxone) == int(idx[part - 1])


def test_long_cloud_in_both_matrix_forms(dev):
    """More points than one pass of the spread form keeps in memory: the carried fp64 sum
    against one workgroup per entry, bit for bit, and against the fp64 mean of the minima."""
    import ldm_sdf
    from ldm_sdf import metrics
    n, R = metrics.split_below() + 5, metrics.spread_below()
    g = torch.Generator().manual_seed(23)
    a = (torch.rand(1, n, 3, generator=g) * 2 - 1).to(dev)
    b = (torch.rand(R, 2, 3, generator=g) * 2 - 1).to(dev)
    batch = ldm_sdf.chamfer_matrix(a, b, directed=True)[0]       # R entries: no spreading
    for r in (0, R - 1):
        one = ldm_sdf.chamfer_matrix(a, b[r:r + 1], directed=True)[0]
        assert np.array_equal(_bits(one), _bits(batch[:, r:r + 1]))
        mean = float(ldm_sdf.nearest_points(a[0], b[r]).cpu().numpy().astype(np.float64).mean())
        assert abs(float(one) - mean) <= 2.0 ** -23 * mean


# ------------------------------------------------------------------ 5. edges
def test_edges(dev):
    import ldm_sdf
    g = torch.Generator().manual_seed(31)
    a = (torch.rand(3, 40, 3, generator=g) * 2 - 1).to(dev)
    b = (torch.rand(2, 50, 3, generator=g) * 2 - 1).to(dev)
    empty = torch.empty(0, 40, 3, device=dev)
    assert ldm_sdf.chamfer_matrix(empty, b).shape == (0, 2)
    assert ldm_sdf.chamfer_matrix(a, empty).shape == (3, 0)
    assert ldm_sdf.chamfer_matrix(empty).shape == (0, 0)
    assert ldm_sdf.nearest_points(a[0][:0], b[0]).shape == (0,)
    with pytest.raises(ldm_sdf.LdmError):
        ldm_sdf.nearest_points(a[0], b[0][:0])
    with pytest.raises(ldm_sdf.LdmError):
        ldm_sdf.chamfer_matrix(a, torch.empty(2, 0, 3, device=dev))
    # n = m = 1
    p, q = a[0, :1], b[0, :1]
    want = float(((p.double() - q.double()) ** 2).sum())
    got = ldm_sdf.chamfer_distance(p, q)
    assert got.dim() == 0 and abs(float(got) - 2 * want) <= 2 * 6 * U * want + 2 * U * want
    d2, idx = ldm_sdf.nearest_points(p, q, return_index=True)
    assert int(idx) == 0 and abs(float(d2) - want) <= 6 * U * want
    # non-contiguous inputs
    wide = (torch.rand(3, 40, 6, generator=g) * 2 - 1).to(dev)
    nc = wide[:, :, ::2]
    assert not nc.is_contiguous()
    assert np.array_equal(_bits(ldm_sdf.chamfer_matrix(nc, b)),
                          _bits(ldm_sdf.chamfer_matrix(nc.contiguous(), b)))
    assert np.array_equal(_bits(ldm_sdf.nearest_points(nc[0], b[0])),
                          _bits(ldm_sdf.nearest_points(nc[0].contiguous(), b[0])))
    # non-finite coordinates raise
    for bad in (float("nan"), float("inf"), float("-inf")):
        x = a.clone()
        x[1, 7, 2] = bad
        with pytest.raises(ldm_sdf.LdmError, match="non-finite"):
            ldm_sdf.chamfer_matrix(x, b)
        with pytest.raises(ldm_sdf.LdmError, match="non-finite"):
            ldm_sdf.chamfer_matrix(b, x)
        with pytest.raises(ldm_sdf.LdmError, match="non-finite"):
            ldm_sdf.chamfer_matrix(x)
        with pytest.raises(ldm_sdf.LdmError, match="non-finite"):
            ldm_sdf.nearest_points(x[1], b[0])
        with pytest.raises(ldm_sdf.LdmError, match="non-finite"):
            ldm_sdf.nearest_points(b[0], x[1])
        with pytest.raises(ldm_sdf.LdmError, match="non-finite"):
            ldm_sdf.chamfer_distance(x[1], b[0])
    # a cloud with itself
    Ta, Cb = _consts()
    big = (torch.rand(Ta + Cb + 3, 3, generator=g) * 2 - 1).to(dev)
    for x in (a[0], big):
        z = ldm_sdf.chamfer_distance(x, x)
        assert z.dim() == 0 and float(z) == 0.0 and not math.copysign(1, float(z)) < 0


# ------------------------------------------------------------------ 6. end to end
def test_spheres_through_sample_surface(dev):
    """Concentric spheres of radius r and r': every point's nearest point of the other surface
    is |r - r'| away, so CD = 2 (r - r')^2 for the surfaces.  The clouds are samples: the nearest
    sample lies an angle theta off the foot point, and d^2 = (r - r')^2 + 2 r r' (1 - cos theta),
    about r r' theta^2 more.  n points spread uniformly over a sphere have, around any spot,
    E[theta^2] = 4 / n for the nearest of them (density n / 4 pi per steradian, E = 1 / (pi
    density)), so each direction gains 4 r r' / n and CD exceeds 2 (r - r')^2 by about
    8 r r' / n: 5.9e-4 at r = 0.5, r' = 0.6, n = 4096, next to 2e-2.  The meshes are icospheres
    of 5120 faces, so a sample sits inside its sphere by a sagitta s >= 0, measured on the clouds
    themselves; the two move |r - r'| by at most s + s' and d^2 by at most
    2 |r - r'| (s + s') + (s + s')^2.  The bound is three times the expected excess plus twice
    that: a property of the sampling, checked on the fp64 reference; the kernel is held to the
    reference at 8u."""
    import ldm_sdf
    from tests import mesh_sdf_reference as M
    r0, r1, n = 0.5, 0.6, 4096
    g = torch.Generator().manual_seed(41)
    clouds = []
    for r in (r0, r1):
        v, f = M.icosphere(4, radius=r)
        xyz, _ = ldm_sdf.sample_surface(torch.from_numpy(v).to(dev), torch.from_numpy(f).to(dev),
                                        n, generator=g)
        assert xyz.shape == (n, 3) and xyz.dtype == torch.float32
        clouds.append(xyz)
    got = float(ldm_sdf.chamfer_distance(*clouds))
    ref = float(C.chamfer_matrix(clouds[0].cpu().numpy()[None], clouds[1].cpu().numpy()[None])[0, 0])
    ideal = 2 * (r0 - r1) ** 2
    excess = 8 * r0 * r1 / n
    ss = sum(float((r - x.double().norm(dim=1)).max()) for r, x in zip((r0, r1), clouds))
    assert 0.0 <= ss <= 4e-3
    sag = 2 * (2 * abs(r0 - r1) * ss + ss * ss)
    print(f"CD {got:.6e}, fp64 reference {ref:.6e}, 2 (r - r')^2 = {ideal:.6e}, "
          f"expected excess {excess:.2e}")
    assert abs(got - ref) <= 8 * U * ref
    assert abs(ref - ideal) <= 3 * excess + sag


def test_shape_clouds_and_evaluate_generation(dev):
    import ldm_sdf
    from ldm_sdf import SDFDecoder
    from oracle import ref_cpu as R
    p = R.make_decoder_params(seed=1234)
    dec = SDFDecoder(256, weights=p.weights, biases=p.biases)
    # the latent of tests/test_gpu_band.py that has a surface, and three near it (the fp64
    # oracle has positive and negative voxels for each at N = 32); the second seed-47 latent
    # is negative on the whole box (oracle maximum -0.146): no zero crossing
    z0 = torch.randn(1, 256, generator=torch.Generator().manual_seed(0)) * 0.1
    noise = torch.randn(1, 256, generator=torch.Generator().manual_seed(5))
    lat = torch.cat([z0, z0 * 0.8, z0 * 1.2, z0 + 0.02 * noise]).to(dev)
    hollow = (torch.randn(2, 256, generator=torch.Generator().manual_seed(47)) * 0.1)[1:].to(dev)
    kw = dict(dtype="fp32", band=float("inf"))
    g = torch.Generator().manual_seed(43)
    clouds = ldm_sdf.shape_clouds(dec, lat, 32, 512, generator=g, batch=3, **kw)
    assert clouds.shape == (4, 512, 3) and clouds.dtype == torch.float32 and clouds.is_cuda
    assert bool(torch.isfinite(clouds).all()) and float(clouds.abs().max()) <= 1.0
    res = ldm_sdf.evaluate_generation(clouds, clouds)
    assert res["mmd"] == 0.0 and res["cov"] == 1.0 and res["1nna"] == 0.0
    assert res["cd_gr"].shape == (4, 4) and np.array_equal(_bits(res["cd_gr"]), _bits(res["cd_gg"]))
    assert np.array_equal(_bits(res["cd_gg"]), _bits(res["cd_rr"]))
    off = res["cd_gr"].cpu().numpy()[~np.eye(4, dtype=bool)]
    assert np.all(off > 0)                                       # four different shapes
    # against the fp64 reference
    want = C.chamfer_matrix(clouds.cpu().numpy())
    assert np.all(np.abs(res["cd_gg"].cpu().numpy() - want) <= 8 * U * want)
    # a shape without a surface: an error naming it, or dropped with skip_empty
    mixed = torch.cat([lat[:1], hollow, lat[1:2]])
    with pytest.raises(ldm_sdf.LdmError, match=r"\[1\]"):
        ldm_sdf.shape_clouds(dec, mixed, 32, 64, **kw)
    kept_clouds, kept = ldm_sdf.shape_clouds(dec, mixed, 32, 64, skip_empty=True, **kw)
    assert kept.tolist() == [0, 2] and kept_clouds.shape == (2, 64, 3)
