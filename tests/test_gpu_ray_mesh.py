"""``ray_mesh`` / ``render_mesh`` / ``depth_samples`` on the GPU against the fp64
oracle of tests/ray_mesh_reference.py: parity within a stated bound, watertightness on edge-
and vertex-aimed rays, chunk tails in both launch forms, bitwise batch invariance across the
switch between the forms, ties and edge cases, the renderer, and the depth-map samples against
``mesh_sdf``."""
import numpy as np
import pytest
import torch

from tests import mesh_sdf_reference as M
from tests import ray_mesh_reference as RR

pytestmark = pytest.mark.gpu

MESHES = ["cube", "icosphere", "hemisphere", "degenerate", "torus"]
N_RAYS = 2000


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
    v, f = ldm_sdf.marching_cubes(torch.from_numpy(RR.torus_volume(48)).to(dev))
    return v.cpu().numpy(), f.cpu().numpy()


def _cast(dev, v, f, o, d, **kw):
    """ray_mesh on numpy inputs: numpy ``(t, face, bary)``."""
    import ldm_sdf
    t, face, bary = ldm_sdf.ray_mesh(torch.from_numpy(v).to(dev), torch.from_numpy(f).to(dev),
                                     torch.from_numpy(o).to(dev), torch.from_numpy(d).to(dev),
                                     return_bary=True, **kw)
    assert t.shape == (len(o),) and t.dtype == torch.float32
    assert face.shape == (len(o),) and face.dtype == torch.int32
    assert bary.shape == (len(o), 3) and bary.dtype == torch.float32
    return t.cpu().numpy(), face.cpu().numpy(), bary.cpu().numpy()


def _check_parity(v, f, o, d, got, max_excused, what):
    """The parity rule: mask, t (against the oracle's t and against the fp64 plane of the
    returned face) within 8 u (|o| + t) / |n . d|; a ray may break it only within
    1e-5 (|o| + 1) of a mesh edge, at most ``max_excused`` of them."""
    t, face, bary = got
    t64, f64 = RR.ray_mesh_ref(v, f, o, d)
    hg, hr = face >= 0, f64 >= 0
    assert np.array_equal(hg, np.isfinite(t)) and np.all(t[~hg] == np.inf)
    assert np.all(bary[~hg] == 0)
    both = hg & hr
    bound = np.zeros(len(o))
    bound[both] = RR.t_bound(o[both], d[both], t64[both], RR.face_normals(v, f)[f64[both]])
    err = np.zeros(len(o))
    err[both] = np.abs(t[both].astype(np.float64) - t64[both])
    perr = np.zeros(len(o))
    perr[both] = np.abs(RR.plane_t(v, f, o[both], d[both], face[both]) - t[both])
    bad = (hg != hr) | (err > bound) | (perr > bound)
    ratio = (err[both] / bound[both]).max() if both.any() else 0.0
    print(f"{what}: {both.sum()} hits, {(hg != hr).sum()} mask differences, "
          f"max |t - t64| / bound = {ratio:.3f}, {bad.sum()} rays to excuse")
    if bad.any():
        near = RR.min_edge_distance(v, f, o[bad], d[bad])
        lim = 1e-5 * (np.linalg.norm(o[bad].astype(np.float64), axis=1) + 1)
        assert np.all(near <= lim), f"{what}: a ray away from every edge disagrees: {near}"
    assert bad.sum() <= max_excused, f"{what}: {bad.sum()} rays disagree"
    # the weights belong to the returned face's vertices, in order: they rebuild the hit point
    # (a permutation would be off by an edge length; the tolerance only has to be below that)
    if hg.any():
        w = bary[hg].astype(np.float64)
        assert np.abs(w.sum(1) - 1).max() <= 1e-6 and w.min() >= -1e-5
        p = (w[:, :, None] * v[f[face[hg]]].astype(np.float64)).sum(1)
        q = o[hg].astype(np.float64) + t[hg, None].astype(np.float64) * d[hg]
        ok = ~bad[hg]
        assert np.abs(p - q)[ok].max() <= 1e-4
    return both.sum()


@pytest.fixture(scope="module")
def cases(dev):
    """mesh name -> (v, f, o, d, got): made and cast once, shared by the tests."""
    made = {}

    def get(name):
        if name not in made:
            v, f = {"cube": M.cube_mesh, "icosphere": lambda: M.icosphere(2),
                    "hemisphere": lambda: M.hemisphere(2), "degenerate": M.cube_with_degenerates,
                    "torus": lambda: _torus_mesh(dev)}[name]()
            o, d = RR.random_rays(N_RAYS, seed=10 + MESHES.index(name))
            made[name] = (v, f, o, d, _cast(dev, v, f, o, d))
        return made[name]
    return get


@pytest.mark.parametrize("name", MESHES)
def test_parity_with_fp64(cases, name):
    v, f, o, d, got = cases(name)
    assert len(f) == {"cube": 12, "icosphere": 320, "hemisphere": 152, "degenerate": 15,
                      "torus": 6480}[name]
    hits = _check_parity(v, f, o, d, got, max_excused=2, what=name)
    assert hits >= 150


@pytest.mark.parametrize("name", ["icosphere2", "torus24"])
def test_watertight_on_the_device(dev, name):
    """The rays of tests/test_render_host.py's watertightness test, same criterion, nobody
    excused."""
    v, f, o, d, dist = RR.watertight_case(name)
    t, face, _ = _cast(dev, v, f, o, d)
    worst = float((t.astype(np.float64) - dist).max())
    print(f"{name}: {len(o)} rays, max t - dist = {worst:.3e}")
    assert (face >= 0).all(), f"{(face < 0).sum()} rays missed the mesh"
    assert worst <= RR.WATERTIGHT_SLACK, worst


def test_chunk_tails_in_both_forms(dev, cases):
    """F in {1, chunk - 1, chunk, chunk + 1} (prefixes of the torus: open meshes; the last is
    the split form) times R in {1, 255, 257}, rays aimed at the faces that are there."""
    import ldm_sdf
    chunk = ldm_sdf.render.face_chunk()
    assert chunk == 1024 and ldm_sdf.render.split_below() > 257
    v, f = cases("torus")[:2]
    rng = np.random.default_rng(3)
    for F in (1, chunk - 1, chunk, chunk + 1):
        sub = np.ascontiguousarray(f[:F])
        o, _ = RR.random_rays(257, seed=F)
        target = M.surface_points(v, sub, 257, rng)
        d = RR.unit_dirs_f32(target - o.astype(np.float64))
        full = None
        for R in (257, 255, 1):
            got = _cast(dev, v, sub, o[:R], d[:R])
            hits = _check_parity(v, sub, o[:R], d[:R], got, max_excused=1,
                                 what=f"torus[:{F}] x {R}")
            assert hits >= R * 0.9
            if full is None:
                full = got
            for a, b in zip(got, full):               # a prefix of the rays: the same rows
                assert np.array_equal(_bits(a), _bits(b[:R]))


@pytest.fixture(scope="module")
def big(dev, cases):
    """The torus' 2000 rays followed by more, up to 1000 past the switch between the launch
    forms, cast once in the one-pass form."""
    import ldm_sdf
    v, f, o, d, _ = cases("torus")
    n = ldm_sdf.render.split_below() + 1000
    o2, d2 = RR.random_rays(n - N_RAYS, seed=77)
    o, d = np.concatenate([o, o2]), np.concatenate([d, d2])
    return o, d, _cast(dev, v, f, o, d)


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


def test_either_side_of_the_split_switch(dev, cases, big):
    """The same rays among 2000 (split over face chunks) and among split_below + 1000 (one
    pass): t, face and bary bitwise equal; and one ray alone."""
    import ldm_sdf
    v, f, o, d, small = cases("torus")
    assert len(f) > ldm_sdf.render.face_chunk() and N_RAYS < ldm_sdf.render.split_below()
    bo, bd, large = big
    assert len(bo) > ldm_sdf.render.split_below()
    for a, b in zip(small, large):
        assert np.array_equal(_bits(a), _bits(b[:N_RAYS]))
    hit = np.flatnonzero(small[1] >= 0)
    for i in (int(hit[0]), int(hit[len(hit) // 2]), int(np.flatnonzero(small[1] < 0)[0])):
        alone = _cast(dev, v, f, o[i:i + 1], d[i:i + 1])
        for a, b in zip(alone, small):
            assert np.array_equal(_bits(a), _bits(b[i:i + 1]))
    # across a tile boundary of the split form: rays at other positions, other neighbours
    s = ldm_sdf.render.split_below() - 1
    shifted = _cast(dev, v, f, bo[1000:1000 + s], bd[1000:1000 + s])
    for a, b in zip(shifted, large):
        assert np.array_equal(_bits(a), _bits(b[1000:1000 + s]))


@pytest.mark.parametrize("name", ["torus", "hemisphere"])
def test_two_calls_are_bitwise_equal(dev, cases, name):
    v, f, o, d, got = cases(name)
    again = _cast(dev, v, f, o, d)
    for a, b in zip(got, again):
        assert np.array_equal(_bits(a), _bits(b))


def test_ties_and_edge_cases(dev):
    import ldm_sdf
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, -1], [1, 0, -1], [0, 1, -1]],
                 np.float32)
    o = np.array([[0.25, 0.25, 2.0], [0.3, 0.1, 1.0], [5, 5, 2.0]], np.float32)
    d = np.array([[0, 0, -1], [0, 0, -2], [0, 0, -1]], np.float32)
    # two coincident triangles (either winding): the lower index wins
    for f in ([[0, 1, 2], [0, 1, 2]], [[0, 2, 1], [0, 1, 2]], [[3, 4, 5], [0, 1, 2], [1, 2, 0]]):
        f = np.array(f, np.int32)
        t, face, bary = _cast(dev, v, f, o, d)
        want = 0 if len(f) == 2 else 1
        assert face.tolist() == [want, want, -1] and t.tolist()[:2] == [2.0, 0.5]
        assert np.isinf(t[2]) and np.all(bary[2] == 0)
        assert np.allclose(bary[:2].sum(1), 1, atol=1e-6)
    f = np.array([[0, 1, 2], [3, 4, 5]], np.int32)
    # the range: t_max below the first hit, t_min above it (the far triangle), both inclusive
    t, face, _ = _cast(dev, v, f, o, d, t_max=0.4)
    assert face.tolist() == [-1, -1, -1] and np.all(np.isinf(t))
    t, face, _ = _cast(dev, v, f, o, d, t_min=0.75)
    assert face.tolist() == [0, 1, -1] and t.tolist()[:2] == [2.0, 1.0]
    t, face, _ = _cast(dev, v, f, o, d, t_min=2.0, t_max=2.0)
    assert face.tolist() == [0, -1, -1] and t[0] == 2.0
    with pytest.raises(ldm_sdf.LdmError):
        _cast(dev, v, f, o, d, t_min=1.0, t_max=0.5)
    # F == 0: all misses; R == 0: empty outputs
    t, face, bary = _cast(dev, v, np.zeros((0, 3), np.int32), o, d)
    assert np.all(np.isinf(t)) and np.all(face == -1) and np.all(bary == 0)
    t, face, bary = _cast(dev, v, f, o[:0], d[:0])
    assert t.shape == (0,) and face.shape == (0,) and bary.shape == (0, 3)
    t, face = ldm_sdf.ray_mesh(*(torch.from_numpy(x).to(dev) for x in (v, f, o, d)))
    assert face.tolist() == [0, 0, -1]                      # without bary: a pair
    # a bad face index raises; what the min/max would let through, the kernel clamps and flags
    bad = np.array([[0, 1, 2], [3, 4, 6]], np.int32)
    with pytest.raises(ldm_sdf.LdmError):
        _cast(dev, v, bad, o, d)
    with pytest.raises(ldm_sdf.LdmError):
        _cast(dev, v, np.array([[0, -1, 2]], np.int32), o, d)
    args = [torch.from_numpy(x).to(dev) for x in (v, bad, o, d)]
    *_, flag = ldm_sdf.ops.ray_mesh(*args, 0.0, float("inf"), True)
    assert int(flag.item()) == 1
    *_, flag = ldm_sdf.ops.ray_mesh(args[0], torch.from_numpy(f).to(dev), args[2], args[3], 0.0,
                                    float("inf"), False)
    assert int(flag.item()) == 0


def test_a_non_finite_ray_among_good_ones(dev, cases):
    v, f, o, d, got = cases("icosphere")
    o2, d2 = o.copy(), d.copy()
    o2[3, 1] = np.nan
    o2[70] = np.inf
    d2[130] = 0.0
    d2[200, 0] = np.nan
    d2[300] = [0, -np.inf, 0]
    bad = [3, 70, 130, 200, 300]
    t, face, bary = _cast(dev, v, f, o2, d2)
    assert np.all(np.isinf(t[bad]) & (t[bad] > 0)) and np.all(face[bad] == -1)
    assert np.all(bary[bad] == 0)
    keep = np.ones(len(o), bool)
    keep[bad] = False
    for a, b in zip((t, face, bary), got):
        assert np.array_equal(_bits(a[keep]), _bits(b[keep]))


# ------------------------------------------------------------------------------ the renderer
POSES = [((0.0, 0.0, 2.6), (0, 1, 0)), ((1.7, 1.1, -1.5), (0, 1, 0)), ((-0.4, -2.4, 0.9), (0, 0, 1))]


@pytest.fixture(scope="module")
def sphere(dev):
    v, f = M.icosphere(2)
    return v, f, torch.from_numpy(v).to(dev), torch.from_numpy(f).to(dev)


@pytest.mark.parametrize("pose_id", range(len(POSES)))
def test_render_mesh_against_the_reference(dev, sphere, pose_id):
    import ldm_sdf
    v, f, vt, ft = sphere
    eye, up = POSES[pose_id]
    pose = ldm_sdf.look_at(eye, (0, 0, 0), up)
    H = W = 64
    out = ldm_sdf.render_mesh(vt, ft, pose, 40.0, H, W)
    o, d = out["origins"].cpu().numpy(), out["dirs"].cpu().numpy()
    o_ref, d_ref = RR.camera_rays_ref(RR.look_at_ref(eye, (0, 0, 0), up), 40.0, H, W)
    assert np.array_equal(o, o_ref) and np.abs(d - d_ref).max() <= 2.0 ** -24
    t = out["t"].cpu().numpy().reshape(-1)
    face = out["face"].cpu().numpy().reshape(-1)
    mask = out["mask"].cpu().numpy().reshape(-1)
    assert out["image"].shape == (H, W, 3) and out["image"].dtype == torch.uint8
    assert out["normal"].shape == (H, W, 3) and out["depth"].shape == (H, W)
    assert np.array_equal(mask, face >= 0) and 1000 < mask.sum() < H * W - 500
    # mask and depth against the fp64 image
    t64, f64 = RR.ray_mesh_ref(v, f, o, d)
    hr = f64 >= 0
    both = mask & hr
    bound = np.zeros(H * W)
    bound[both] = RR.t_bound(o[both], d[both], t64[both], RR.face_normals(v, f)[f64[both]])
    fwd = -pose.numpy()[:3, 2]
    cosf = d.astype(np.float64) @ fwd
    depth = out["depth"].cpu().numpy().reshape(-1).astype(np.float64)
    assert np.all(np.isinf(depth[~mask]) & (depth[~mask] > 0))
    derr = np.zeros(H * W)
    derr[both] = np.abs(depth[both] - t64[both] * cosf[both])
    # the bound on t, projected, plus the roundings of the dot product and the product
    bad = (mask != hr) | (derr > bound * cosf + 4 * RR.U24 * np.where(both, t64, 0) * cosf)
    print(f"pose {pose_id}: {mask.sum()} pixels hit, {(mask != hr).sum()} mask differences, "
          f"{bad.sum()} pixels to excuse")
    if bad.any():
        near = RR.min_edge_distance(v, f, o[bad], d[bad])
        assert np.all(near <= 1e-5 * (np.linalg.norm(o[bad].astype(np.float64), axis=1) + 1))
    assert bad.sum() <= 4
    # normals and the image: the same shading applied in numpy to the kernel's own t and face
    n = RR.face_normals(v, f)[np.maximum(face, 0)]
    dh = d.astype(np.float64) / np.linalg.norm(d.astype(np.float64), axis=1, keepdims=True)
    n = np.where(((n * dh).sum(1) > 0)[:, None], -n, n) * mask[:, None]
    got_n = out["normal"].cpu().numpy().reshape(-1, 3)
    assert np.abs(got_n - n).max() <= 1e-5
    want = RR.shade_ref(n, d, mask, background=1.0)
    img = out["image"].cpu().numpy().reshape(-1, 3).astype(np.int64)
    assert np.all(img[:, 0] == img[:, 1]) and np.all(img[:, 0] == img[:, 2])
    assert np.abs(img[:, 0] - want.astype(np.int64)).max() <= 1
    assert np.all(img[~mask] == 255) and img[mask].max() <= 255 and img[mask].min() >= 0
    # vertex normals: the barycentric blend of the kernel's own weights, renormalised
    vn = v / np.linalg.norm(v, axis=1, keepdims=True)
    out2 = ldm_sdf.render_mesh(vt, ft, pose, 40.0, H, W,
                               vertex_normals=torch.from_numpy(vn).to(dev), background=0.25)
    assert torch.equal(out2["t"], out["t"]) and torch.equal(out2["face"], out["face"])
    _, _, bary = ldm_sdf.ray_mesh(vt, ft, out["origins"], out["dirs"], return_bary=True)
    w = bary.cpu().numpy().astype(np.float64)
    blend = (w[:, :, None] * vn.astype(np.float64)[f[np.maximum(face, 0)]]).sum(1)
    blend /= np.maximum(np.linalg.norm(blend, axis=1, keepdims=True), 1e-30)
    blend = np.where(((blend * dh).sum(1) > 0)[:, None], -blend, blend) * mask[:, None]
    got_n2 = out2["normal"].cpu().numpy().reshape(-1, 3)
    assert np.abs(got_n2 - blend).max() <= 1e-5
    # on a sphere the blended normal is close to radial, and smoother than the facets (away
    # from the silhouette, where a blend that leans away from the camera is flipped)
    hitp = o[mask] + t[mask, None] * d[mask]
    radial = hitp / np.linalg.norm(hitp, axis=1, keepdims=True)
    front = (radial * dh[mask]).sum(1) < -0.2
    assert front.sum() > 500
    assert np.abs(got_n2[mask] - radial)[front].max() < np.abs(got_n[mask] - radial)[front].max()
    img2 = out2["image"].cpu().numpy().reshape(-1, 3)
    assert np.all(img2[~mask] == 64)
    assert np.abs(img2[:, 0].astype(np.int64) -
                  RR.shade_ref(blend, d, mask, background=0.25).astype(np.int64)).max() <= 1


def test_render_mesh_of_an_empty_mesh_and_of_nothing_in_view(dev, sphere):
    """``extract_mesh`` returns ``verts[:0], faces[:0]`` for a latent with no zero crossing:
    its image is all background, nothing is gathered, ``depth_samples`` is empty.  The same
    for a mesh the camera does not see."""
    import ldm_sdf
    _, _, vt, ft = sphere
    pose = ldm_sdf.look_at((0, 0, 2.6), (0, 0, 0))
    away = ldm_sdf.look_at((0, 0, 2.6), (0, 0, 5.0))
    H, W = 24, 40
    for v, f, p in ((vt[:0], ft[:0], pose), (vt, ft[:0], pose), (vt, ft, away)):
        for vn in (None, torch.nn.functional.normalize(v, dim=1)):
            out = ldm_sdf.render_mesh(v, f, p, 40.0, H, W, vertex_normals=vn, background=0.5)
            torch.cuda.synchronize()
            assert not bool(out["mask"].any()) and bool((out["face"] == -1).all())
            assert bool(torch.isinf(out["t"]).all()) and bool(torch.isinf(out["depth"]).all())
            assert bool((out["t"] > 0).all()) and bool((out["depth"] > 0).all())
            assert out["normal"].shape == (H, W, 3) and bool((out["normal"] == 0).all())
            assert out["image"].shape == (H, W, 3) and out["image"].dtype == torch.uint8
            assert bool((out["image"] == 128).all())
            xyz, sdf = ldm_sdf.depth_samples(out["origins"], out["dirs"], out["t"], out["normal"])
            assert xyz.shape == (0, 3) and sdf.shape == (0,)
    t, face, bary = ldm_sdf.ray_mesh(vt[:0], ft[:0], out["origins"], out["dirs"],
                                     return_bary=True)
    assert bool(torch.isinf(t).all()) and bool((face == -1).all()) and bool((bary == 0).all())


def test_render_writes_a_png(dev, sphere, tmp_path):
    import ldm_sdf
    _, _, vt, ft = sphere
    out = ldm_sdf.render_mesh(vt, ft, ldm_sdf.look_at((2, 1.5, 2), (0, 0, 0)), 35.0, 48, 80)
    assert out["image"].shape == (48, 80, 3)
    p = str(tmp_path / "sphere.png")
    ldm_sdf.write_png(p, out["image"])
    assert np.array_equal(ldm_sdf.read_png(p), out["image"].cpu().numpy())


def test_depth_samples_against_mesh_sdf(dev, sphere):
    """DeepSDF §6.3's two points per depth pixel: mesh_sdf of the front points is eta, of the
    back points negative and no farther than eta (both to mesh_sdf's fp32 bound, 2e-6)."""
    import ldm_sdf
    _, _, vt, ft = sphere
    eta = 0.01
    out = ldm_sdf.render_mesh(vt, ft, ldm_sdf.look_at((1.2, 0.9, 2.0), (0, 0, 0)), 40.0, 64, 64)
    xyz, sdf = ldm_sdf.depth_samples(out["origins"], out["dirs"], out["t"], out["normal"],
                                     eta=eta)
    M_hit = int(out["mask"].sum())
    assert M_hit > 1000 and xyz.shape == (2 * M_hit, 3) and sdf.shape == (2 * M_hit,)
    assert xyz.is_cuda and xyz.dtype == torch.float32
    assert torch.all(sdf[:M_hit] == eta) and torch.all(sdf[M_hit:] == -eta)
    got = ldm_sdf.mesh_sdf(vt, ft, xyz.contiguous()).cpu().numpy().astype(np.float64)
    front, back = got[:M_hit], got[M_hit:]
    print(f"front: max |sdf - eta| = {np.abs(front - eta).max():.3e}; back: max sdf = "
          f"{back.max():.3e}, max |sdf| - eta = {(np.abs(back) - eta).max():.3e}")
    assert np.abs(front - eta).max() <= 2e-6
    assert np.all(back < 0) and (np.abs(back) - eta).max() <= 2e-6
