"""``mesh_sdf`` on the MI355X against the fp64 reference tests/mesh_sdf_reference.py
(DESIGN.md §16): distance, closest face, winding number and sign on closed, open, degenerate
and marching-cubes meshes; ragged face and point counts in both launch forms; bitwise batch
invariance across the forms; the edges; the round trip through the project's own mesher; and
``sample_sdf`` end to end into the SdfSamples files the trainer reads.

Bounds: distance 2e-6 (the project's fp32 bound); winding 1e-3 (worst-case
linear accumulation over 6480 faces is F 2^-24 = 4e-4; the sign needs 0.5).  Measured maxima
are printed by each test and recorded in DESIGN.md §16."""
import os

import numpy as np
import pytest
import torch

from tests import mesh_sdf_reference as M

pytestmark = pytest.mark.gpu

D_TOL, W_TOL = 2e-6, 1e-3
MESHES = ["cube", "icosphere", "hemisphere", "degenerate", "torus"]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import ldm_sdf
    ldm_sdf.load_library()
    return torch.device("cuda", 0)


def _torus_mesh(dev):
    """The torus of tests/test_gpu_mc.py at N = 48 through the project's marching cubes:
    6480 faces, slivers included."""
    import ldm_sdf
    from oracle import ref_mc
    c = ref_mc._coords(48)
    z, y, x = np.meshgrid(c, c, c, indexing="ij")
    tor = (np.sqrt((np.sqrt(x * x + y * y) - 0.5) ** 2 + z * z) - 0.2).astype(np.float32)
    v, f = ldm_sdf.marching_cubes(torch.from_numpy(tor).to(dev))
    return v.cpu().numpy(), f.cpu().numpy()


def _points(v, f, seed):
    """1000 uniform in [-1, 1]^3 and 1000 surface points perturbed by N(0, 0.0005), fp32."""
    rng = np.random.default_rng(seed)
    near = M.surface_points(v, f, 1000, rng) + rng.normal(0, 0.0005 ** 0.5, (1000, 3))
    return np.concatenate([rng.uniform(-1, 1, (1000, 3)), near]).astype(np.float32)


class Case:
    """One mesh, its 2000 points, the fp64 reference and the GPU result, each computed once."""

    def __init__(self, dev, name, v, f, seed):
        self.dev, self.name = dev, name
        self.v, self.f = np.ascontiguousarray(v, np.float32), np.ascontiguousarray(f, np.int32)
        self.p = _points(self.v, self.f, seed)
        self._ref, self._gpu = {}, None

    def ref(self, F=None):
        """(sdf, closest, winding, d) of the first ``F`` faces, fp64."""
        F = len(self.f) if F is None else F
        if F not in self._ref:
            self._ref[F] = M.mesh_sdf_ref(self.v, self.f[:F], self.p)
        return self._ref[F]

    def run(self, F=None, P=None, pts=None):
        import ldm_sdf
        F = len(self.f) if F is None else F
        p = self.p[:P] if pts is None else pts
        out = ldm_sdf.mesh_sdf(torch.from_numpy(self.v).to(self.dev),
                               torch.from_numpy(self.f[:F]).to(self.dev),
                               torch.from_numpy(p).to(self.dev),
                               return_closest=True, return_winding=True)
        return tuple(x.cpu().numpy() for x in out)

    def gpu(self):
        if self._gpu is None:
            self._gpu = self.run()
        return self._gpu


@pytest.fixture(scope="module")
def cases(dev):
    made = {}

    def get(name):
        if name not in made:
            v, f = {"cube": M.cube_mesh, "icosphere": M.icosphere, "hemisphere": M.hemisphere,
                    "degenerate": M.cube_with_degenerates,
                    "torus": lambda: _torus_mesh(dev)}[name]()
            made[name] = Case(dev, name, v, f, seed=100 + MESHES.index(name))
        return made[name]
    return get


def _check_against(case, got, ref, rows=slice(None)):
    """Distance, closest face and winding of ``got`` against the reference rows ``rows``."""
    sdf, closest, w = got
    rsdf, _, rw, rd = (x[rows] for x in ref)
    assert sdf.dtype == np.float32 and closest.dtype == np.int32 and w.dtype == np.float32
    assert np.isfinite(sdf).all() and np.isfinite(w).all()
    d_err = np.abs(np.abs(sdf.astype(np.float64)) - rd).max()
    w_err = np.abs(w.astype(np.float64) - rw).max()
    # indices are not compared (fp32 and fp64 break near-ties differently): the returned face
    # must be as close, in fp64, as the closest one
    F = len(case.f)
    assert ((closest >= 0) & (closest < F)).all()
    slack = (M.dist_to_face(case.v, case.f, case.p[rows], closest) - rd).max()
    print(f"{case.name}: max |d - d_ref| = {d_err:.3e}, max |w - w_ref| = {w_err:.3e}, "
          f"closest-face slack = {slack:.3e}")
    assert d_err <= D_TOL
    assert slack <= D_TOL
    assert w_err <= W_TOL
    assert np.array_equal(np.signbit(sdf), w > 0.5), "the sign is not the winding rule"


@pytest.mark.parametrize("name", MESHES)
def test_distance_closest_winding(cases, name):
    case = cases(name)
    if name == "torus":
        assert len(case.f) == 6480
    _check_against(case, case.gpu(), case.ref())


@pytest.mark.parametrize("name", MESHES)
def test_sign(cases, name):
    case = cases(name)
    sdf = case.gpu()[0]
    rsdf, _, rw, rd = case.ref()
    use = rd >= 1e-4
    if name == "hemisphere":
        use &= np.abs(rw - 0.5) >= 0.05
    skipped = 1.0 - use.mean()
    bad = int(((sdf < 0) != (rsdf < 0))[use].sum())
    print(f"{name}: {skipped:.2%} of the points skipped, {bad} sign mismatches")
    assert skipped <= 0.05
    assert bad == 0


def test_ragged_faces_and_points_in_both_forms(cases):
    """F in {1, chunk - 1, chunk, chunk + 1, 6480} (prefixes of the torus: open meshes) times
    P in {1, 63, 64, 65, 257, 2000}: every tail, one chunk and many."""
    import ldm_sdf
    chunk = ldm_sdf.meshsdf.face_chunk()
    case = cases("torus")
    assert chunk + 1 < len(case.f) and ldm_sdf.meshsdf.split_below() > 2000
    for F in (1, chunk - 1, chunk, chunk + 1, len(case.f)):
        ref = case.ref(F)
        sub = Case.__new__(Case)
        sub.__dict__.update(case.__dict__)
        sub.f, sub.name = case.f[:F], f"torus[:{F}]"
        for P in (1, 63, 64, 65, 257, 2000):
            got = sub.run(P=P)
            assert all(len(x) == P for x in got)
            _check_against(sub, got, ref, slice(0, P))


@pytest.fixture(scope="module")
def big(dev, cases):
    """The torus' 2000 points followed by uniform ones, up to 1000 past the switch between the
    launch forms, and the one-pass result on all of them."""
    import ldm_sdf
    case = cases("torus")
    n = ldm_sdf.meshsdf.split_below() + 1000
    extra = np.random.default_rng(9).uniform(-1, 1, (n - 2000, 3)).astype(np.float32)
    pts = np.concatenate([case.p, extra])
    return pts, case.run(pts=pts)


def test_either_side_of_the_split_switch(cases, big):
    """P = split_below - 1 runs split over face chunks, P = split_below in one pass: the rows
    they share are bitwise equal, and the first 2000 meet the reference."""
    import ldm_sdf
    case = cases("torus")
    sb = ldm_sdf.meshsdf.split_below()
    pts, full = big
    for P in (sb - 1, sb, sb + 1):
        got = case.run(pts=pts[:P])
        for a, b in zip(got, full):
            assert np.array_equal(a.view(np.uint32), b[:P].view(np.uint32)), P
        _check_against(case, tuple(x[:2000] for x in got), case.ref())


def test_a_point_alone_equals_its_row_in_any_batch(cases, big):
    """Bitwise, in all three outputs, across the launch forms: alone (split), among 2000
    (split) and among thousands (one pass)."""
    case = cases("torus")
    pts, full = big
    batch = case.gpu()
    for a, b in zip(batch, full):
        assert np.array_equal(a.view(np.uint32), b[:2000].view(np.uint32))
    for i in list(range(0, 2000, 143)) + [1999, 1000]:
        alone = case.run(pts=case.p[i:i + 1])
        for a, b in zip(alone, batch):
            assert a.view(np.uint32)[0] == b.view(np.uint32)[i], i
    # one chunk only (no split form exists): alone against the batch
    cube = cases("cube")
    for i in (0, 999, 1500):
        for a, b in zip(cube.run(pts=cube.p[i:i + 1]), cube.gpu()):
            assert a.view(np.uint32)[0] == b.view(np.uint32)[i]


@pytest.mark.parametrize("name", ["torus", "hemisphere"])
def test_two_calls_are_bitwise_equal(cases, name):
    case = cases(name)
    for a, b in zip(case.run(), case.gpu()):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


def test_ties_and_zero_area_faces(cases):
    cube, deg = cases("cube"), cases("degenerate")
    # every face twice: the first copy wins every tie
    dup = Case.__new__(Case)
    dup.__dict__.update(cube.__dict__)
    dup.f = np.concatenate([cube.f, cube.f])
    sdf, closest, w = dup.run()
    assert (closest < 12).all()
    assert np.array_equal(sdf, cube.gpu()[0])
    # on the collinear face, between two of its corners: no solid angle from it, and d = 0 --
    # exactly at the first point (its foot has the dyadic parameter 1/2), within the distance
    # bound at the second (parameter 2/3, rounded)
    on = np.array([[0.8125, 0.875, 0.875], [0.625, 0.875, 0.875]], np.float32)
    sdf, closest, w = deg.run(pts=on)
    assert sdf[0] == 0.0 and np.abs(sdf).max() <= D_TOL and (closest >= 12).all()
    assert np.array_equal(w.view(np.uint32), cube.run(pts=on)[2].view(np.uint32))
    assert np.abs(w).max() <= W_TOL
    only = Case.__new__(Case)
    only.__dict__.update(deg.__dict__)
    only.f = deg.f[12:]
    sdf, closest, w = only.run(pts=on)
    assert sdf[0] == 0.0 and np.abs(sdf).max() <= D_TOL and np.array_equal(w, [0.0, 0.0])


def test_edges(dev, cases):
    import ldm_sdf
    cube = cases("cube")
    v, f = torch.from_numpy(cube.v).to(dev), torch.from_numpy(cube.f).to(dev)
    p = torch.from_numpy(cube.p[:100]).to(dev)
    sdf, closest, w = ldm_sdf.mesh_sdf(v, f, p[:0], return_closest=True, return_winding=True)
    assert sdf.shape == (0,) and closest.shape == (0,) and w.shape == (0,)
    sdf, closest, w = ldm_sdf.mesh_sdf(v, f[:0], p, return_closest=True, return_winding=True)
    assert bool(torch.isposinf(sdf).all()) and bool((closest == -1).all()) and bool((w == 0).all())
    assert ldm_sdf.mesh_sdf(v, f, p).shape == (100,)
    only_w = ldm_sdf.mesh_sdf(v, f, p, return_winding=True)
    assert len(only_w) == 2 and only_w[1].dtype == torch.float32
    for bad_index in (len(cube.v), -1):
        fb = f.clone()
        fb[7, 1] = bad_index
        with pytest.raises(ldm_sdf.LdmError):          # the wrapper's min/max over faces
            ldm_sdf.mesh_sdf(v, fb, p)
        with pytest.raises(ldm_sdf.LdmError):          # past it: the kernel clamps and flags
            ldm_sdf.mesh_sdf(v, fb, p, _validated=True)
    torch.cuda.synchronize()
    assert torch.equal(ldm_sdf.mesh_sdf(v, f, p), torch.from_numpy(cube.gpu()[0][:100]).to(dev))
    with pytest.raises(ldm_sdf.LdmError):
        ldm_sdf.mesh_sdf(v, f.float(), p)
    with pytest.raises(ldm_sdf.LdmError):
        ldm_sdf.mesh_sdf(v, f, p.double())


def test_round_trip_through_marching_cubes(dev):
    """An analytic sphere (r = 0.55, N = 64) meshed by the project's marching cubes, then
    ``mesh_sdf``: within a voxel of the field the mesh came from, the same sign beyond one."""
    import ldm_sdf
    from oracle import ref_mc
    N, r = 64, 0.55
    h = 2.0 / (N - 1)
    c = ref_mc._coords(N)
    z, y, x = np.meshgrid(c, c, c, indexing="ij")
    vol = torch.from_numpy((np.sqrt(x * x + y * y + z * z) - r).astype(np.float32)).to(dev)
    v, f = ldm_sdf.marching_cubes(vol)
    rng = np.random.default_rng(11)
    u = rng.standard_normal((1000, 3))
    near = u / np.linalg.norm(u, axis=1, keepdims=True) * (r + rng.normal(0, 0.0005 ** 0.5, (1000, 1)))
    p = np.concatenate([rng.uniform(-1, 1, (1000, 3)), near]).astype(np.float32)
    sdf = ldm_sdf.mesh_sdf(v, f, torch.from_numpy(p).to(dev)).cpu().numpy().astype(np.float64)
    true = np.linalg.norm(p.astype(np.float64), axis=1) - r
    err = np.abs(sdf - true).max()
    print(f"sphere N = 64: {len(f)} faces, max |sdf - (|x| - r)| = {err:.3e} (h = {h:.3e})")
    assert err <= h
    far = np.abs(true) > h
    assert far.sum() > 500 and np.array_equal(sdf[far] < 0, true[far] < 0)


def test_sample_sdf_end_to_end(dev, tmp_path):
    import ldm_sdf
    v, f = M.icosphere()
    v, f = torch.from_numpy(v).to(dev), torch.from_numpy(f).to(dev)
    g = torch.Generator(device=dev).manual_seed(5)
    pos, neg = ldm_sdf.sample_sdf(v, f, 20000, generator=g)
    assert pos.shape[1] == 4 and neg.shape[1] == 4 and pos.dtype == torch.float32
    assert pos.shape[0] + neg.shape[0] == 20000
    assert bool((pos[:, 3] >= 0).all()) and bool((neg[:, 3] < 0).all())
    # 94 % of the points hug the surface on both sides; the uniform 6 % are mostly outside
    assert 0.35 * 20000 < neg.shape[0] < 0.55 * 20000
    near = torch.cat([pos, neg])[:, 3].abs() < 0.25
    assert float(near.float().mean()) > 0.94
    # the rows are what mesh_sdf says of their own points (chunking changes nothing)
    again = ldm_sdf.mesh_sdf(v, f, pos[:, :3].contiguous())
    assert torch.equal(again, pos[:, 3])
    # a CPU generator draws the same way, on the host
    pos2, neg2 = ldm_sdf.sample_sdf(v, f, 1000, generator=torch.Generator().manual_seed(5))
    assert pos2.shape[0] + neg2.shape[0] == 1000 and pos2.is_cuda
    split = {"ds": {"cls": ["ico"]}}
    path = os.path.join(str(tmp_path), "SdfSamples", "ds", "cls", "ico.npz")
    ldm_sdf.data.save_sdf_samples(path, pos, neg)
    ss = ldm_sdf.data.SdfSampleSet.from_split(str(tmp_path), split)
    assert torch.equal(ss.pools[0][0], pos.cpu()) and torch.equal(ss.pools[0][1], neg.cpu())
    xyz, sdf = ss.draw(4096, device=dev, generator=torch.Generator().manual_seed(0))
    assert xyz.shape == (1, 4096, 3) and sdf.shape == (1, 4096) and xyz.is_cuda
    assert bool((sdf[0, :2048] >= 0).all()) and bool((sdf[0, 2048:] < 0).all())
