"""Sphere tracing of the decoder on the MI355X: the kernels of
csrc/sdf_trace.hip against the numpy restatement BIT FOR BIT on synthetic decoder values and
masks; ``trace_sdf`` against the closed-form ray-octahedron hit of the L1-ball network, against
the stored fp64 run of a real field (tests/golden/sdf_trace_scene.npz) in fp32 and, inside the
measured windows, in the 16-bit types; self-consistency with ``decode_points``; bitwise batch
invariance; brick skipping; ``render_sdf`` against ``render_mesh``; and the edge cases.

Tolerances and how each was obtained: tests/sdf_trace_reference.py."""
import math
import os

import numpy as np
import pytest
import torch

from tests import sdf_trace_reference as T
from tests.test_gpu_band import dev, decoder, l1_decoder  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DTYPES = ["fp32", "bf16", "fp16"]
F32 = np.float32
L1_C, L1_R = 0.7, 0.25
L1_LIP = 0.7 * math.sqrt(3.0)
EPS = 1e-3


def _latent0(dev):
    g = torch.Generator().manual_seed(0)
    return (torch.randn(1, 256, generator=g) * 0.1).to(dev)


@pytest.fixture(scope="module")
def golden():
    return T.load_scene_golden(os.path.join(ROOT, "tests", "golden", T.GOLDEN))


@pytest.fixture(scope="module")
def scene(dev):
    o, d = T.scene_rays()
    return torch.from_numpy(o).to(dev), torch.from_numpy(d).to(dev)


_RUNS = {}


def _scene_run(dev, decoder, scene, dtype, skip=None):
    """``trace_sdf`` of the scene, computed once per (dtype, skip) and shared."""
    import ldm_sdf
    key = (dtype, skip)
    if key not in _RUNS:
        out = ldm_sdf.trace_sdf(decoder, _latent0(dev), scene[0], scene[1], dtype=dtype,
                                skip_resolution=skip, return_points=True, **T.SCENE)
        _RUNS[key] = tuple(x.cpu().numpy() for x in out)
    return _RUNS[key]


# ------------------------------------------------------- 1. kernels == numpy, bit for bit
def _synthetic_rays(R, B, per_shape, seed):
    rng = np.random.default_rng(seed)
    n = B * R if per_shape else R
    o = rng.uniform(-1.7, 1.7, (n, 3))
    d = (rng.uniform(-0.7, 0.7, (n, 3)) - o) * rng.choice([0.3, 1.0, 2.5], (n, 1))
    o, d = o.astype(F32), d.astype(F32)
    k = min(n, 6)                                  # rays the setup refuses, a ray inside the box
    special = np.array([[0, 0, 0, 0, 0, 0], [np.nan, 0, 0, 1, 0, 0], [0, 0, 0, np.inf, 1, 0],
                        [0.1, 0.2, 0.3, 0, 0, -1], [0.5, 1.5, 3, 0, 0, -1],
                        [-1.5, -1.5, -1.5, 1, 1, 1]], F32)[:k]
    if n > 6:
        o[:k], d[:k] = special[:, :3], special[:, 3:]
    return (o.reshape(B, R, 3), d.reshape(B, R, 3)) if per_shape else (o, d)


def _synthetic_values(B, R, K, level, eps, seed):
    """[B, R, K] decoder values: shape 0 stops almost at once, the last shape marches on, the
    specials (exactly eps, below, NaN, huge, -inf) sprinkled in."""
    rng = np.random.default_rng(seed)
    v = (np.abs(rng.standard_normal((B, R, K))) * 0.08 + 0.004).astype(F32) + F32(level)
    v[0] = np.where(rng.random((R, K)) < 0.7, F32(level) - F32(0.01), v[0])
    flat = v.reshape(-1)
    pick = rng.choice(flat.size, max(5, flat.size // 40), replace=False)
    flat[pick[0::5]] = F32(level) + F32(eps)
    flat[pick[1::5]] = F32(level) + F32(eps) * F32(0.5)
    flat[pick[2::5]] = np.nan
    flat[pick[3::5]] = F32(3e38)
    flat[pick[4::5]] = -np.inf
    return v


@pytest.mark.parametrize("R,B,per_shape,N", [(1, 1, False, 0), (63, 3, False, 20),
                                             (64, 1, True, 33), (65, 3, True, 0),
                                             (1000, 3, False, 64), (70000, 3, False, 40),
                                             (70000, 1, False, 0),
                                             # two scan chunks per shape, shapes 1 and 2 start at
                                             # flag addresses that are not 16-byte aligned
                                             (4099, 3, False, 0)])
def test_kernels_equal_reference_bit_for_bit(dev, R, B, per_shape, N):
    from ldm_sdf import ops
    K, level, lip, eps = 6, -0.1, 0.45, 1e-3
    o, d = _synthetic_rays(R, B, per_shape, seed=R + B)
    vals = _synthetic_values(B, R, K, level, eps, seed=R)
    mask = None
    if N:
        nb = T.n_bricks(N)
        mask = (np.random.default_rng(N).random(B * nb ** 3) < 0.3).astype(np.uint8)
    ref = T.trace_reference(lambda b, p, rays, k: vals[b, rays, k], o, d, B, level=level,
                            lipschitz=lip, eps=eps, max_steps=K, t_min=0.05, t_max=3.0,
                            mask=mask, N=N, keep=True)
    st = ops.SdfTraceState(torch.from_numpy(o).to(dev), torch.from_numpy(d).to(dev), B,
                           (-1.0, 1.0), level, lip, eps,
                           None if mask is None else torch.from_numpy(mask).to(dev), N, True)
    ops.sdf_trace_init(st, 0.05, 3.0, K)
    rounds = 0
    for k in range(K):
        counts = st.counts.tolist()
        want = ref["lists"][k] if k < len(ref["lists"]) else [np.zeros(0, np.int32)] * B
        assert counts == [len(w) for w in want], (k, counts)
        P = max(counts)
        if P == 0:
            break
        rounds += 1
        lst = st.list.cpu().numpy()
        xyz = ops.sdf_trace_emit(st, P).cpu().numpy()
        v = np.zeros((B, P), F32)
        for b in range(B):
            n = counts[b]
            assert np.array_equal(lst[b, :n], want[b]), (k, b)
            pts = ref["points"][k][b]
            assert np.array_equal(xyz[b, :n].view(np.uint32), pts.view(np.uint32)), (k, b)
            pad = pts[-1] if n else np.full(3, -1.0, F32)
            assert np.array_equal(xyz[b, n:].view(np.uint32),
                                  np.broadcast_to(pad, (P - n, 3)).copy().view(np.uint32))
            v[b, :n] = vals[b, want[b], k]
            v[b, n:] = np.nan                       # padding values are ignored
        ops.sdf_trace_step(st, torch.from_numpy(v).to(dev))
    if R >= 1000:
        assert rounds == K
    assert np.array_equal(st.status.cpu().numpy(), ref["status"])
    assert np.array_equal(st.steps.cpu().numpy(), ref["steps"])
    assert np.array_equal(st.t.cpu().numpy().view(np.uint32), ref["t_work"].view(np.uint32))
    got = st.xyz_last.cpu().numpy()
    assert np.array_equal(np.isnan(got), np.isnan(ref["xyz"]))
    assert np.array_equal(np.nan_to_num(got).view(np.uint32),
                          np.nan_to_num(ref["xyz"]).view(np.uint32))
    if R >= 1000:                                   # every outcome occurs, in uneven shares
        for s in (T.MISS, T.HIT, T.ACTIVE):
            assert (ref["status"] == s).sum() > 10
        if B == 3:
            act = (ref["status"] == T.ACTIVE).sum(1)
            assert act[2] > 4 * max(act[0], 1)


# --------------------------------------------------------------------- 2. the L1 ball
def _l1_camera(dev):
    import ldm_sdf
    o, d = ldm_sdf.camera_rays(ldm_sdf.look_at((1.1, 0.8, 0.65), (0, 0, 0), (0, 0, 1)), 50.0, 24,
                               24, device=dev)
    return o, d


def _l1_expect(o, d, dtype):
    """Closed form: (sure hit, sure miss, t*, |df/dt| at the entry).  f = tanh(c |x|_1 - r); a
    ray whose smallest f lies in [-delta_T, eps + delta_T] may go either way (a value error of
    delta_T, and a march is only kept from passing f <= 0, not f <= eps)."""
    rho = L1_R / L1_C
    o64, d64 = o.astype(np.float64), d.astype(np.float64)
    t_star, gmin = T.octahedron_hit(o64, d64, rho)
    fmin = np.tanh(L1_C * gmin)
    dT = T.DELTA_T[dtype]
    sure_hit, sure_miss = fmin < -dT, fmin > EPS + dT
    with np.errstate(all="ignore"):
        before = o64 + (np.where(np.isfinite(t_star), t_star, 0.0) - 1e-9)[:, None] * d64
    slope = np.abs((np.sign(before) * d64).sum(1)) * L1_C
    return sure_hit, sure_miss, t_star, slope


@pytest.mark.parametrize("dtype", DTYPES)
def test_l1_ball_against_closed_form(dev, l1_decoder, dtype):
    import ldm_sdf
    o, d = _l1_camera(dev)
    z = _latent0(dev)
    t, st, steps = ldm_sdf.trace_sdf(l1_decoder, z, o, d, lipschitz=L1_LIP, eps=EPS, dtype=dtype)
    t, st = t.cpu().numpy()[0].astype(np.float64), st.cpu().numpy()[0]
    sure_hit, sure_miss, t_star, slope = _l1_expect(o.cpu().numpy(), d.cpu().numpy(), dtype)
    print(f"l1 {dtype}: {sure_hit.sum()} sure hits, {sure_miss.sum()} sure misses of {len(st)}, "
          f"{int(steps.sum())} evaluations")
    assert sure_hit.sum() > 40 and sure_miss.sum() > 200
    assert (sure_hit | sure_miss).mean() >= 0.9
    assert (st[sure_hit] == T.HIT).all() and (st[sure_miss] == T.MISS).all()
    assert (st != T.ACTIVE).all()
    # t in [t* - (eps + delta_T) / |df/dt| - slack, t* + slack]: before the entry f is at least
    # |df/dt| (t* - t) (|x|_1 is convex along the ray), so it is above eps + delta_T farther out;
    # past the entry a value error above eps can carry the ray on until f <= eps - delta_T, and
    # one smallest step (eps / lipschitz) beyond
    dT = T.DELTA_T[dtype]
    h = sure_hit
    late = 1e-5 + (max(dT - EPS, 0.0) / slope[h] + EPS / L1_LIP if dT > EPS else 0.0)
    early = (EPS + dT) / (slope[h] * (1 - (EPS + dT) ** 2)) + 1e-5
    dt = t[h] - t_star[h]
    print(f"   t - t*: [{dt.min():.3e}, {dt.max():.3e}]")
    assert (dt <= late).all() and (dt >= -early).all()


# ------------------------------------------------------------ 3. fp32 parity on a real field
def test_fp32_parity_with_fp64_reference(dev, decoder, scene, golden):
    t, st, steps, _ = _scene_run(dev, decoder, scene, "fp32")
    c = T.compare_runs(golden, st, t, T.STATUS_MARGIN)
    sd = np.abs(steps - golden["steps"])
    same = st == golden["status"]
    tol = T.fp32_t_tol(T.SCENE["lipschitz"], T.SCENE["eps"], int(golden["steps"].max()))
    print(f"fp32 against fp64: {c}, steps differ by <= {sd[same].max()}, t tol {tol:.3e}")
    assert (steps > 0).sum() == 465
    assert c["aside"] <= T.SET_ASIDE_CAP and c["flips"] == 0
    assert c["dt"] <= tol
    assert sd[same].max() <= 1


# --------------------------------------------------------------------- 4. 16-bit parity
@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
def test_lowp_parity_with_fp64_reference(dev, decoder, scene, golden, dtype):
    """Status outside the rays set aside (reference misses of clearance below the dtype's
    status margin, reference hits that the fp64 run with the level lowered by it loses), t of
    the common hits inside the stored window.  Measured on an MI355X before hits could be set
    aside: bf16 turned one reference miss of clearance 9.8e-4 into a hit and one reference hit,
    stopped by fp64 8.7e-5 below eps at its last point in the box, into a miss; its values
    differ from fp64 by 2.529e-3 at most, exactly the CPU emulation's figure."""
    t, st, steps, _ = _scene_run(dev, decoder, scene, dtype)
    c = T.compare_runs(golden, st, t, T.lowp_status_margin(dtype), golden["window"][dtype],
                       golden["lost"][dtype])
    tol = T.lowp_t_tol(dtype, T.SCENE["lipschitz"], T.SCENE["eps"])
    print(f"{dtype} against fp64: {c}, window tol {tol:.3e}")
    assert c["aside"] <= T.SET_ASIDE_CAP and c["flips"] == 0
    assert c["excess"] <= tol


# -------------------------------------------------------------------- 5. self-consistency
@pytest.mark.parametrize("dtype", DTYPES)
def test_hits_and_exhausted_rays_are_what_decode_points_says(dev, decoder, scene, dtype):
    import ldm_sdf
    z = _latent0(dev)
    kw = dict(T.SCENE, max_steps=12)                # few enough to leave rays marching
    t, st, steps, xyz = ldm_sdf.trace_sdf(decoder, z, scene[0], scene[1], dtype=dtype,
                                          return_points=True, **kw)
    ev = steps[0] > 0
    v = ldm_sdf.decode_points(decoder, z, xyz[:, ev], dtype=dtype)[0]
    f = v - torch.tensor(kw["level"], dtype=torch.float32, device=dev)
    eps = torch.tensor(kw["eps"], dtype=torch.float32, device=dev)
    s = st[0][ev]
    assert (s == T.HIT).sum() > 100 and (s == T.ACTIVE).sum() > 50
    assert bool((f[s == T.HIT] <= eps).all())
    assert bool((f[s == T.ACTIVE] > eps).all())
    assert bool((steps[0][st[0] == T.ACTIVE] == 12).all())
    assert bool(torch.isinf(t[st != T.HIT]).all()) and bool(torch.isfinite(t[st == T.HIT]).all())
    assert bool(torch.isnan(xyz[0][~ev]).all())
    hp = scene[0] + t[0][:, None] * scene[1]
    assert bool(((hp - xyz[0])[st[0] == T.HIT].abs() <= 1e-6).all())


# ------------------------------------------------------------------- 6. batch invariance
def test_batch_invariance_bitwise(dev, decoder, scene):
    import ldm_sdf
    o, d = scene
    z = _latent0(dev)
    kw = dict(T.SCENE, dtype="bf16", return_points=True)
    base = ldm_sdf.trace_sdf(decoder, z, o, d, **kw)
    again = ldm_sdf.trace_sdf(decoder, z, o, d, **kw)
    for a, b in zip(base, again):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    perm = torch.randperm(o.shape[0], generator=torch.Generator().manual_seed(5)).to(dev)
    shuf = ldm_sdf.trace_sdf(decoder, z, o[perm], d[perm], **kw)
    for a, b in zip(base, shuf):
        assert torch.equal(a[:, perm].view(torch.int32), b.view(torch.int32))
    st = base[1][0]
    pick = [int(torch.nonzero(st == s)[k]) for s, k in ((T.HIT, 0), (T.HIT, 170), (T.MISS, 200))
            if (st == s).sum() > k]
    pick.append(int(base[2][0].argmax()))           # the ray with the most evaluations
    for r in pick:
        one = ldm_sdf.trace_sdf(decoder, z, o[r:r + 1], d[r:r + 1], **kw)
        for a, b in zip(base, one):
            assert torch.equal(a[:, r:r + 1].view(torch.int32), b.view(torch.int32)), r
    # with other shapes in the batch, shared and per-shape rays
    g = torch.Generator().manual_seed(47)
    others = (torch.randn(2, 256, generator=g) * 0.1).to(dev)
    zz = torch.cat([others[:1], z, others[1:]])
    many = ldm_sdf.trace_sdf(decoder, zz, o, d, **kw)
    rays3 = torch.stack([o.flip(0), o, o]), torch.stack([d.flip(0), d, d])
    many3 = ldm_sdf.trace_sdf(decoder, zz, rays3[0], rays3[1], **kw)
    for a, b, c in zip(base, many, many3):
        assert torch.equal(a[0].view(torch.int32), b[1].view(torch.int32))
        assert torch.equal(a[0].view(torch.int32), c[1].view(torch.int32))
        assert torch.equal(b[0].flip(0).view(torch.int32), c[0].view(torch.int32))


# --------------------------------------------------------------------------- 7. skipping
def _march(dec, z, o, d, dtype, skip, **kw):
    """``trace_sdf``'s loop through the ops wrappers, keeping every emitted point."""
    from ldm_sdf import ops
    dv = z.device
    desc = dec.device_pack(dtype, dv)["desc"]
    beta = ops.decoder_fold(desc, z.float().contiguous())
    B = z.shape[0]
    from ldm_sdf import render
    mask = render.skip_mask(desc, beta, skip, (-1.0, 1.0), kw["level"], kw["lipschitz"], kw["eps"])
    st = ops.SdfTraceState(o, d, B, (-1.0, 1.0), kw["level"], kw["lipschitz"], kw["eps"], mask,
                           skip, False)
    ops.sdf_trace_init(st, 0.0, math.inf, kw["max_steps"])
    pts = []
    for _ in range(kw["max_steps"]):
        counts = st.counts.tolist()
        if max(counts) == 0:
            break
        xyz = ops.sdf_trace_emit(st, max(counts))
        pts += [xyz[b, :n].cpu().numpy() for b, n in enumerate(counts)]
        ops.sdf_trace_step(st, ops.decoder_points_fwd(desc, beta, xyz))
    return st, mask.cpu().numpy(), np.concatenate(pts)


def test_skipping_l1_ball(dev, l1_decoder):
    import ldm_sdf
    o, d = _l1_camera(dev)
    z = _latent0(dev)
    kw = dict(level=0.0, lipschitz=L1_LIP, eps=EPS, max_steps=256)
    t0, s0, n0 = ldm_sdf.trace_sdf(l1_decoder, z, o, d, dtype="fp32", **kw)
    t1, s1, n1 = ldm_sdf.trace_sdf(l1_decoder, z, o, d, dtype="fp32", skip_resolution=64, **kw)
    sure_hit, sure_miss, t_star, slope = _l1_expect(o.cpu().numpy(), d.cpu().numpy(), "fp32")
    clear = torch.from_numpy(sure_hit | sure_miss).to(dev)
    assert torch.equal(s0[0][clear], s1[0][clear])
    print(f"l1 skip: {int(n0.sum())} -> {int(n1.sum())} evaluations")
    assert int(n1.sum()) < int(n0.sum())
    h = torch.from_numpy(sure_hit).to(dev)
    # both stop inside the eps shell before the entry: at most its thickness along the ray apart
    shell = torch.from_numpy((EPS + 2e-6) / (slope[sure_hit] * (1 - EPS ** 2)) + 2e-5).to(dev)
    assert bool(((t0[0][h] - t1[0][h]).abs().double() <= shell).all())
    st, mask, pts = _march(l1_decoder, z, o, d, "fp32", 64, **kw)
    assert torch.equal(st.status, s1) and torch.equal(st.steps, n1)
    nb = T.n_bricks(64)
    bnd = T.bounds(64, T.voxel_size(64, (-1.0, 1.0)), -1.0)
    assert 0 < mask.sum() < 0.2 * mask.size
    assert len(pts) == int(n1.sum()) and T.in_active_brick(pts, mask.reshape(nb, nb, nb), bnd).all()


def test_skipping_real_field(dev, decoder, scene, golden):
    t0, s0, n0, _ = _scene_run(dev, decoder, scene, "fp32")
    t1, s1, n1, _ = _scene_run(dev, decoder, scene, "fp32", skip=64)
    aside = (T.miss_clearance(golden) < T.STATUS_MARGIN)
    assert np.array_equal(s0[~aside], s1[~aside])
    print(f"scene skip: {int(n0.sum())} -> {int(n1.sum())} evaluations")
    assert int(n1.sum()) < int(n0.sum())
    # a sound march of a field within the fp16 margin of fp64 stops inside the stored window
    # (the fp32 field is far inside that margin), whatever points it evaluates on the way
    c = T.compare_runs(golden, s1, t1, T.STATUS_MARGIN, golden["window"]["fp16"])
    tol = T.lowp_t_tol("fp16", T.SCENE["lipschitz"], T.SCENE["eps"])
    both = (s0 == T.HIT) & (s1 == T.HIT)
    dt = np.abs(t0[both].astype(np.float64) - t1[both])
    print(f"   window excess {c['excess']:.3e} (tol {tol:.3e}), |dt| median {np.median(dt):.3e} "
          f"max {dt.max():.3e}")
    assert c["flips"] == 0 and c["excess"] <= tol
    assert np.median(dt) <= T.SCENE["eps"] / T.SCENE["lipschitz"]
    st, mask, pts = _march(decoder, _latent0(dev), scene[0], scene[1], "fp32", 64, **T.SCENE)
    assert np.array_equal(st.status.cpu().numpy(), s1)
    nb = T.n_bricks(64)
    bnd = T.bounds(64, T.voxel_size(64, (-1.0, 1.0)), -1.0)
    assert 0 < mask.sum() < mask.size
    assert T.in_active_brick(pts, mask.reshape(nb, nb, nb), bnd).all()


def test_skipping_keeps_hits_of_rays_that_start_inside(dev, l1_decoder):
    """A box inside the L1 ball (bbox +-0.1, |x|_1 <= 0.3 < 0.357): no brick is outside the
    shape, the middle ones are inactive (f = -0.245, band 0.074).  Every ray hits at its first
    point, with and without skipping: bricks inside the shape are not passed through."""
    import ldm_sdf
    z = _latent0(dev)
    g = torch.Generator().manual_seed(3)
    o = ((torch.rand(200, 3, generator=g) - 0.5) * 0.18).to(dev)
    d = torch.randn(200, 3, generator=g).to(dev)
    kw = dict(bbox=(-0.1, 0.1), lipschitz=L1_LIP, eps=EPS, dtype="fp32")
    t0, s0, n0 = ldm_sdf.trace_sdf(l1_decoder, z, o, d, **kw)
    t1, s1, n1 = ldm_sdf.trace_sdf(l1_decoder, z, o, d, skip_resolution=24, **kw)
    assert bool((s0 == 1).all()) and bool((t0 == 0).all()) and bool((n0 == 1).all())
    assert torch.equal(s0, s1) and torch.equal(t0, t1) and torch.equal(n0, n1)


# ------------------------------------------------------- 8. render_sdf against render_mesh
def test_render_sdf_against_render_mesh(dev, l1_decoder):
    import ldm_sdf
    from tests import decoder_grad_emulation as E
    z = _latent0(dev)
    pose = ldm_sdf.look_at((1.1, 0.8, 0.65), (0, 0, 0), (0, 0, 1))
    H = W = 48
    (v, f), = ldm_sdf.extract_mesh(l1_decoder, z, 64, dtype="fp32", lipschitz=L1_LIP)
    rm = ldm_sdf.render_mesh(v, f, pose, 50.0, H, W)
    rs = ldm_sdf.render_sdf(l1_decoder, torch.cat([z, z]), pose, 50.0, H, W, lipschitz=L1_LIP,
                            eps=EPS, dtype="fp32")
    assert set(rs) == set(rm) - {"face"}
    assert rs["t"].shape == (2, H, W) and rs["normal"].shape == (2, H, W, 3)
    assert rs["image"].shape == (2, H, W, 3) and rs["image"].dtype == torch.uint8
    assert rs["mask"].dtype == torch.bool and rs["depth"].shape == (2, H, W)
    for k in ("t", "mask", "depth", "normal", "image"):
        assert torch.equal(rs[k][0], rs[k][1]), k
    both = rm["mask"] & rs["mask"][0]
    inner = both.clone()                            # away from the silhouette: all 8 neighbours hit
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            inner &= torch.roll(both, (dy, dx), (0, 1))
    inner[0], inner[-1], inner[:, 0], inner[:, -1] = False, False, False, False
    assert int(inner.sum()) > 100
    diag = math.sqrt(3.0) * 2.0 / 63
    dd = (rm["depth"] - rs["depth"][0])[inner].abs()
    cos = (rm["normal"] * rs["normal"][0]).sum(-1)[inner].clamp(-1, 1)
    ang = torch.rad2deg(torch.acos(cos))
    print(f"render: {int(inner.sum())} inner pixels, depth diff max {float(dd.max()):.3e} (voxel "
          f"diagonal {diag:.3e}), normal angle median {float(ang.median()):.3f} deg")
    assert float(dd.max()) <= diag
    assert float(ang.median()) < 4 * E.MEDIAN_ANGLE_FP16_DEG
    assert float((rs["normal"][0][rs["mask"][0]].norm(dim=-1) - 1).abs().max()) <= 1e-5
    assert bool((rs["normal"][0][~rs["mask"][0]] == 0).all())
    assert bool((rs["image"][0][~rs["mask"][0]] == 255).all())
    xyz, sdf = ldm_sdf.depth_samples(rs["origins"], rs["dirs"], rs["t"][0], rs["normal"][0])
    M = int(rs["mask"][0].sum())
    assert xyz.shape == (2 * M, 3) and sdf.shape == (2 * M,) and M > 200
    assert bool(torch.isfinite(xyz).all()) and bool((sdf[:M] > 0).all()) and bool((sdf[M:] < 0).all())


# ------------------------------------------------------------------------ 9. edge cases
def test_edge_cases(dev, l1_decoder):
    import ldm_sdf
    z = _latent0(dev)
    inf, nan = math.inf, math.nan
    o = torch.tensor([[2.0, 0, 0], [2.0, 0, 0], [nan, 0, 0], [2.0, 0, 0], [3.0, 3.0, 0],
                      [0.0, 0, 0], [2.0, 0.05, 0.02], [2.0, 0, inf]], device=dev)
    d = torch.tensor([[0.0, 0, 0], [nan, 0, 0], [-1.0, 0, 0], [-inf, 0, 0], [1.0, 0, 0],
                      [0.0, 0, 1.0], [-2.0, 0, 0], [-1.0, 0, 0]], device=dev)
    kw = dict(lipschitz=L1_LIP, eps=EPS, dtype="fp32")
    t, st, steps = ldm_sdf.trace_sdf(l1_decoder, z, o, d, **kw)
    assert st[0].tolist() == [0, 0, 0, 0, 0, 1, 1, 0]
    assert steps[0].tolist()[:5] == [0, 0, 0, 0, 0] and steps[0][7] == 0
    assert t[0][5] == 0.0 and steps[0][5] == 1                       # starts inside
    rho = L1_R / L1_C
    assert abs(float(t[0][6]) - (2.0 - (rho - 0.07)) / 2) <= 2e-3    # t in units of |d| = 2
    # t_min inside the shape: a hit at t_min; t_max before it: a miss; max_steps = 1
    t, st, steps = ldm_sdf.trace_sdf(l1_decoder, z, o[6:7], d[6:7], t_min=0.9, **kw)
    assert st[0, 0] == 1 and float(t[0, 0]) == np.float32(0.9) and steps[0, 0] == 1
    t, st, steps = ldm_sdf.trace_sdf(l1_decoder, z, o[6:7], d[6:7], t_max=0.7, **kw)
    assert st[0, 0] == 0 and math.isinf(float(t[0, 0])) and steps[0, 0] >= 1
    t, st, steps = ldm_sdf.trace_sdf(l1_decoder, z, o[6:7], d[6:7], max_steps=1, **kw)
    assert st[0, 0] == 2 and math.isinf(float(t[0, 0])) and steps[0, 0] == 1
    # no rays; a 1-D latent
    t, st, steps = ldm_sdf.trace_sdf(l1_decoder, z[0], o[:0], d[:0], **kw)
    assert t.shape == (1, 0) and st.shape == (1, 0)
    for bad in (dict(eps=0.0), dict(lipschitz=-1.0), dict(max_steps=0), dict(t_min=2.0, t_max=1.0),
                dict(bbox=(1.0, 1.0)), dict(skip_resolution=1)):
        with pytest.raises(ValueError):
            ldm_sdf.trace_sdf(l1_decoder, z, o, d, **dict(kw, **bad))
    with pytest.raises(ValueError):
        ldm_sdf.trace_sdf(l1_decoder, z, o, d[:3], **kw)


def test_estimate_lipschitz_l1_ball(dev, l1_decoder):
    """|grad f| = c sqrt(3) (1 - f^2) wherever no coordinate is 0; the grid maximum is where
    |f| is smallest.  resolution 32 has no grid point on a coordinate plane."""
    import ldm_sdf
    from ldm_sdf import ops
    z = torch.cat([_latent0(dev), _latent0(dev) * 2])
    got = ldm_sdf.estimate_lipschitz(l1_decoder, z, 32)
    assert got.shape == (2,)
    xyz = ops.grid_coords(32, device=dev).double()
    f = torch.tanh(L1_C * xyz.abs().sum(1) - L1_R)
    want = L1_LIP * float((1 - f * f).max())
    print(f"estimate_lipschitz: {got.tolist()}, closed form {want:.5f}")
    assert bool(((got.double() - want).abs() <= 0.02 * want).all())
