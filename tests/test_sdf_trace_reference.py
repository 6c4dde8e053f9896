"""CPU checks around the sphere tracer: the numpy restatement
tests/sdf_trace_reference.py against closed forms, its brick walk against brute force, the
header csrc/ray_brick_dda.h run on the host (tests/c/ray_brick_dda_check.cpp) against the
restatement bit for bit, the C error-path checker tests/c/sdf_trace_errors.c (the source
`make check-asan` also runs under host AddressSanitizer), the Python argument checks, and the
stored reference run and tolerance constants of tests/test_gpu_sdf_trace.py re-measured."""
import math
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

from tests import sdf_trace_reference as T
from tests.c_checker import run_c_checker

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "latent-diffusion-models-for-shape-sdfs_amd")
CSRC = os.path.join(PKG, "csrc")
F32 = np.float32


def _camera(eye, n):
    import ldm_sdf
    o, d = ldm_sdf.camera_rays(ldm_sdf.look_at(eye, (0, 0, 0), (0, 0, 1)), 50.0, n, n)
    return o.numpy(), d.numpy()


# --------------------------------------------------------- the reference against closed forms
def test_reference_on_exact_sphere():
    """An exact distance field with lipschitz = 1: every hit lies within eps (in distance, so in
    t for unit directions) before the closed-form entry, never behind it; the misses are the
    closed form's."""
    rad, eps = 0.6, 1e-3
    field = T.point_field(lambda b, p: np.linalg.norm(p.astype(np.float64), axis=1) - rad)
    o, d = _camera((2.2, 1.6, 1.3), 24)
    want = T.sphere_hit(o, d, rad)
    far = T.sphere_hit(o, d, rad + 3 * eps)              # rays that clear the shell: sure misses
    r = T.trace_reference(field, o, d, 1, eps=eps, max_steps=200)
    st, t = r["status"][0], r["t"][0].astype(np.float64)
    sure_hit = np.isfinite(T.sphere_hit(o, d, rad - 3 * eps))
    assert 50 < sure_hit.sum() < 400
    assert (st[sure_hit] == T.HIT).all() and (st[~np.isfinite(far)] == T.MISS).all()
    assert (st != T.ACTIVE).all()
    h = st == T.HIT
    common = h & np.isfinite(want)
    # the stop is the first evaluation within eps of the surface: along the ray that is at
    # most eps / cos(incidence) before the entry; grazing rays are left to the window below
    assert (t[common] <= want[common] + 1e-5).all()
    steep = common & (np.isfinite(T.sphere_hit(o, d, rad * 0.8)))
    assert (want[steep] - t[steep] <= eps / 0.5).all() and steep.sum() > 40
    assert np.isinf(r["t"][0][~h]).all()
    assert (r["steps"][0][st == T.MISS].max() >= 1) and r["steps"][0].max() < 200
    p = r["xyz"][0][h].astype(np.float64)
    assert (np.linalg.norm(p, axis=1) - rad <= eps + 1e-6).all()


def test_reference_inside_start_outside_box_and_exhaustion():
    rad = 0.6
    field = T.point_field(lambda b, p: np.linalg.norm(p.astype(np.float64), axis=1) - rad)
    o = np.array([[0.1, 0.0, 0.0], [3.0, 3.0, 0.0], [3.0, 0.0, 0.0], [0.0, 0.0, 0.0],
                  [np.nan, 0.0, 0.0], [2.0, 0.0, 0.0]], F32)
    d = np.array([[1, 0, 0], [1, 0, 0], [-2, 0, 0], [0, 0, 0], [1, 0, 0], [-1, 0, 0]], F32)
    r = T.trace_reference(field, o, d, 1, max_steps=64)
    assert r["status"][0].tolist() == [T.HIT, T.MISS, T.HIT, T.MISS, T.MISS, T.HIT]
    assert r["t"][0][0] == 0.0 and r["steps"][0][0] == 1          # starts inside: hit at t_min
    assert r["steps"][0][1] == 0 and r["steps"][0][3] == 0 and r["steps"][0][4] == 0
    # t is in units of the direction: |d| = 2 halves it (box entry at x = 1, t = 1)
    assert abs(float(r["t"][0][2]) - (3.0 - rad) / 2) <= 1e-3 and r["t"][0][2] >= 1.0
    assert abs(float(r["t"][0][5]) - (2.0 - rad)) <= 1e-3
    # exhaustion: too few evaluations leave the ray marching, t = +inf
    r1 = T.trace_reference(field, o[5:], d[5:], 1, max_steps=1)
    assert r1["status"][0, 0] == T.ACTIVE and np.isinf(r1["t"][0, 0]) and r1["steps"][0, 0] == 1
    # t_min inside the shape, t_max before it
    r2 = T.trace_reference(field, o[5:], d[5:], 1, t_min=1.7)
    assert r2["status"][0, 0] == T.HIT and r2["t"][0, 0] == F32(1.7) and r2["steps"][0, 0] == 1
    r3 = T.trace_reference(field, o[5:], d[5:], 1, t_max=1.2)
    assert r3["status"][0, 0] == T.MISS and r3["steps"][0, 0] >= 1


def test_octahedron_closed_form():
    rho = 0.25 / 0.7
    o = np.array([[2, 0, 0], [2, 0, 0], [1, 1, 1], [0, 0, 0], [2, 2, 0], [0.0, 0.5, 2.0]], float)
    d = np.array([[-1, 0, 0], [0, 1, 0], [-1, -1, -1], [1, 0, 0], [-1, -1, 0.3], [0, 0, -1]],
                 float)
    t, m = T.octahedron_hit(o, d, rho)
    assert np.allclose(t[[0, 3]], [2 - rho, 0.0]) and np.isinf(t[1]) and np.isinf(t[5])
    assert np.isclose(t[2], 1 - rho / 3)
    assert np.isclose(m[1], 2 - rho) and np.isclose(m[5], 0.5 - rho) and m[0] < 0 and m[3] < 0
    # against dense sampling
    rng = np.random.default_rng(3)
    o = rng.uniform(-1, 1, (200, 3)) * 2
    d = rng.normal(size=(200, 3))
    t, m = T.octahedron_hit(o, d, rho)
    ts = np.linspace(0, 8, 40001)
    val = np.abs(o[:, None, :] + ts[None, :, None] * d[:, None, :]).sum(-1) - rho
    assert np.abs(val.min(1) - m).max() <= 2e-3
    hit = val.min(1) < -2e-3
    assert np.isfinite(t[hit]).all() and np.isinf(t[val.min(1) > 2e-3]).all()
    first = ts[(val <= 0).argmax(1)]
    assert np.abs(first[hit] - t[hit]).max() <= 4e-4


# ------------------------------------------------------------------------- the brick walk
def _walk_rays(N, seed, n=300):
    """Random rays through the box, rays along the axes (also on brick faces) and rays through
    brick corners."""
    rng = np.random.default_rng(seed)
    bnd = T.bounds(N, T.voxel_size(N, (-1.0, 1.0)), -1.0).astype(np.float64)
    o = rng.uniform(-1.6, 1.6, (n, 3))
    d = rng.uniform(-0.8, 0.8, (n, 3)) - o
    d *= rng.choice([0.3, 1.0, 2.5], (n, 1))
    axes_o, axes_d = [], []
    for a in range(3):
        for s in (-1.0, 1.0):
            for c in (0.013, float(bnd[1]), float(bnd[-2]), -0.37):
                oo = np.full(3, c)
                oo[a] = -1.5 * s
                dd = np.zeros(3)
                dd[a] = s
                axes_o.append(oo)
                axes_d.append(dd)
    corner = np.array([[bnd[i], bnd[j], bnd[k]] for i in (1, 2) for j in (1, 2)
                       for k in (1, len(bnd) - 2)])
    co = rng.uniform(-1.5, 1.5, (len(corner), 3))
    o = np.concatenate([o, np.array(axes_o), co, -np.ones((1, 3)) * 1.5])
    d = np.concatenate([d, np.array(axes_d), corner - co, np.ones((1, 3))])
    return o.astype(F32), d.astype(F32)


@pytest.mark.parametrize("N", [20, 33, 64])
def test_walk_against_brute_force(N):
    """N = 20: a last brick 3 voxels thick; N = 33: a last brick without width."""
    nb = T.n_bricks(N)
    bnd = T.bounds(N, T.voxel_size(N, (-1.0, 1.0)), -1.0)
    assert len(bnd) == nb + 1 and (np.diff(bnd) >= 0).all() and bnd[0] == -1.0
    assert (bnd[-1] - bnd[-2] < bnd[1] - bnd[0]) and (N != 33 or bnd[-1] == bnd[-2])
    o, d = _walk_rays(N, seed=N)
    rng = np.random.default_rng(100 + N)
    for density in (0.08, 0.5):
        mask = (rng.random((nb, nb, nb)) < density).astype(np.uint8)
        ok, t0, t1 = T.clip(o, d, -1.0, 1.0, F32(0), F32(np.inf))
        assert 150 < ok.sum()
        i = np.nonzero(ok)[0]
        alive, t = T.skip(o[i], d[i], t0[i], t1[i], mask, bnd)
        assert 20 < alive.sum() < len(i) or density == 0.5
        moved = 0
        for j, r in enumerate(i):
            found = T.walk_brute(o[r], d[r], t0[r], t1[r], mask, bnd)
            tol = 2e-5 * max(1.0, float(t1[r]))
            if alive[j]:
                assert T.in_active_brick(T.point_at(o[r:r + 1], d[r:r + 1], t[j:j + 1]), mask,
                                         bnd)[0], (N, r, "the landing point is in no active brick")
                assert t0[r] <= t[j] <= t1[r]
                moved += t[j] > t0[r]
                if found is not None:            # nothing active before the landing
                    assert t[j] <= found[0] + found[1] + tol, (N, r, t[j], found)
                else:                            # an active sliver between two samples
                    assert t1[r] - t0[r] >= 0
            elif found is not None:              # a miss may overlook a sliver only
                ts = np.linspace(float(t0[r]), float(t1[r]), 20000)
                p = o[r].astype(np.float64) + ts[:, None] * d[r].astype(np.float64)
                cc = (p[..., None] >= bnd[1:nb].astype(np.float64)).sum(-1)
                assert mask[cc[:, 2], cc[:, 1], cc[:, 0]].sum() <= 2, (N, r)
        assert moved > 20


@pytest.fixture(scope="module")
def dda_check(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path_factory.mktemp("dda") / "ray_brick_dda_check")
    r = subprocess.run([cxx, "-O2", "-std=c++17", "-Wall", "-Werror", "-Wno-unknown-pragmas",
                        "-ffp-contract=off", "-I", CSRC,
                        os.path.join(ROOT, "tests", "c", "ray_brick_dda_check.cpp"), "-o", exe],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]

    def run(tmp, o, d, v, N, mask, par):
        src, dst = str(tmp / "in.bin"), str(tmp / "out.bin")
        nb = T.n_bricks(N)
        with open(src, "wb") as fh:
            fh.write(np.array([len(o), N, mask is not None], np.int64).tobytes())
            fh.write(np.array(par, F32).tobytes())
            fh.write((mask if mask is not None else np.zeros(nb ** 3, np.uint8)).tobytes())
            fh.write(np.ascontiguousarray(np.concatenate([o, d, v[:, None]], 1), F32).tobytes())
        r = subprocess.run([exe, src, dst], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and r.stdout.startswith("ray_brick_dda ok"), r.stdout + r.stderr
        out = np.fromfile(dst, np.uint32).reshape(-1, 5)
        return (out[:, 0].astype(np.int32), out[:, 1].copy().view(F32), out[:, 2].copy().view(F32),
                out[:, 3].astype(np.int32), out[:, 4].copy().view(F32))
    return run


@pytest.mark.parametrize("N,use_mask", [(20, True), (33, True), (64, True), (64, False)])
def test_header_equals_reference_bit_for_bit(dda_check, tmp_path, N, use_mask):
    o, d = _walk_rays(N, seed=7 + N, n=2000)
    special = np.array([[0, 0, 0, 0, 0, 0], [np.inf, 0, 0, 1, 0, 0], [0, 0, 0, np.nan, 1, 0],
                        [0.5, 0.5, 3, 0, 0, -1], [0.5, 1.5, 3, 0, 0, -1], [0, 0, 0, 1e-42, 0, 0],
                        [0.3, -0.2, 0.1, 1e30, 1e30, 0], [-1, -1, -1, 1, 1, 1]], F32)
    o = np.concatenate([o, special[:, :3]])
    d = np.concatenate([d, special[:, 3:]])
    rng = np.random.default_rng(N)
    nb = T.n_bricks(N)
    mask = (rng.random(nb ** 3) < 0.15).astype(np.uint8) if use_mask else None
    level, lip, eps = F32(-0.1), F32(0.45), F32(1e-3)
    v = (rng.standard_normal(len(o)) * 0.3).astype(F32)
    v[::7] = level + eps                                  # exactly eps: a hit
    v[1::11] = np.nan
    v[2::13] = 3e38
    v[3::17] = level - F32(0.2)
    par = [-1.0, 1.0, 0.0, 2.5, T.voxel_size(N, (-1, 1)), level, lip, eps]
    st, t, t_end, st2, t2 = dda_check(tmp_path, o, d, v, N, mask, par)
    # the restatement: one round of trace_reference with these values
    r = T.trace_reference(lambda b, p, rays, k: v[rays], o, d, 1, level=level, lipschitz=lip,
                          eps=eps, max_steps=1, t_min=0.0, t_max=2.5, mask=mask, N=N, keep=True)
    r0 = T.trace_reference(lambda b, p, rays, k: v[rays], o, d, 1, level=level, lipschitz=lip,
                           eps=eps, max_steps=1, t_min=0.0, t_max=2.5, mask=mask, N=N)
    started = np.zeros(len(o), bool)
    started[r["lists"][0][0]] = True
    assert np.array_equal(st == T.ACTIVE, started) and 300 < started.sum() < len(o)
    assert not started[[-8, -7, -6, -4]].any() and (st[~started] == T.MISS).all()
    p0 = T.point_at(o[started], d[started], t[started])
    assert np.array_equal(p0.view(np.uint32), r["points"][0][0].view(np.uint32))
    assert np.array_equal(st2[started], r0["status"][0][started])
    assert set(np.unique(st2[started])) == {T.MISS, T.HIT, T.ACTIVE}
    assert np.array_equal(t2[started].view(np.uint32),
                          r0["t_work"][0][started].view(np.uint32)) or \
        np.array_equal(np.where(st2 == T.MISS, np.inf, t2).astype(F32)[started].view(np.uint32),
                       r0["t_work"][0][started].view(np.uint32))
    if use_mask:                                          # every point handed on is in an active brick
        bnd = T.bounds(N, T.voxel_size(N, (-1, 1)), -1.0)
        m3 = mask.reshape(nb, nb, nb)
        for pts in (p0, T.point_at(o, d, t2)[started & (st2 == T.ACTIVE)]):
            assert T.in_active_brick(pts, m3, bnd).all()


def test_sdf_trace_errors_from_c(tmp_path):
    run_c_checker("sdf_trace_errors", tmp_path)


# ------------------------------------------------------------------ the Python argument checks
def test_argument_checks_and_no_cpu_fallback():
    import ldm_sdf
    from oracle import ref_cpu as R
    p = R.make_decoder_params(seed=1234)
    dec = ldm_sdf.SDFDecoder(256, weights=p.weights, biases=p.biases)
    z, o, d = torch.zeros(2, 256), torch.zeros(5, 3), torch.ones(5, 3)
    with pytest.raises(ldm_sdf.LdmError):
        ldm_sdf.trace_sdf(dec, z, o, d)
    with pytest.raises(ldm_sdf.LdmError):
        ldm_sdf.render_sdf(dec, z, ldm_sdf.look_at((0, 0, 3), (0, 0, 0)), 40.0, 4, 4)
    with pytest.raises(ldm_sdf.LdmError):
        ldm_sdf.estimate_lipschitz(dec, z)
    with pytest.raises(ldm_sdf.LdmError):
        ldm_sdf.ops.SdfTraceState(o, d, 2, (-1.0, 1.0), 0.0, 1.0, 1e-3, None, 0, False)
    assert "not a bound" in ldm_sdf.estimate_lipschitz.__doc__.lower().replace("\n", " ")
    for name in ("trace_sdf", "render_sdf", "estimate_lipschitz"):
        assert callable(getattr(ldm_sdf, name)) and name in ldm_sdf.render.__all__


# ---------------------------------------------------- the stored run and the constants
@pytest.fixture(scope="module")
def few_threads():
    n = torch.get_num_threads()
    torch.set_num_threads(min(n, 4))        # 600-point matrix products: more threads only wait
    yield
    torch.set_num_threads(n)


def test_golden_run_is_the_reference(few_threads):
    """tests/golden/sdf_trace_scene.npz is ``trace_reference`` of the scene with the fp64
    oracle, with the issue's census: 465 rays in the box, 347 hits (119 at the box entry), 229
    misses; the fp32 oracle changes no status and moves t by 4.1e-6 at most."""
    g = T.load_scene_golden(os.path.join(ROOT, "tests", "golden", T.GOLDEN))
    r = T.scene_reference("fp64")
    for k in ("t", "t_work", "status", "steps"):
        assert np.array_equal(g[k], r[k]), k
    for k, v in g["hist"].items():
        assert np.array_equal(v, r["hist"][k]), k
    st, steps = r["status"][0], r["steps"][0]
    assert (steps > 0).sum() == 465 and (st == T.HIT).sum() == 347 and (st == T.MISS).sum() == 229
    assert ((st == T.HIT) & (steps == 1)).sum() == 119 and steps.max() < T.SCENE["max_steps"]
    aside = T.miss_clearance(r) < T.STATUS_MARGIN
    assert aside.sum() == 19 and aside.mean() <= T.SET_ASIDE_CAP
    r32 = T.scene_reference("fp32")
    c = T.compare_runs(r, r32["status"], r32["t"], T.STATUS_MARGIN)
    print("fp32 against fp64:", c)
    assert c["flips"] == 0 and c["dt"] <= 4 * 4.1e-6 and np.abs(r32["steps"] - steps).max() <= 1
    assert c["dt"] <= T.fp32_t_tol(T.SCENE["lipschitz"], T.SCENE["eps"], int(steps.max()))


@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
def test_lowp_constants_hold(few_threads, dtype):
    """MEASURED_LOWP re-measured: the emulation's value error is the recorded one (within
    [1/2, 1] of it), it flips no status, its t stays inside the stored window, the rays set
    aside stay under the cap, and the status factor is the largest of 4, 2, 1 that does."""
    m = T.measure_lowp(dtype)
    print(dtype, m, "status margin", T.lowp_status_margin(dtype), "t margin",
          T.lowp_margin(dtype), "tol", T.lowp_t_tol(dtype, T.SCENE["lipschitz"], T.SCENE["eps"]))
    rec = T.MEASURED_LOWP[dtype]
    assert 0.5 * rec["value"] <= m["value"] <= rec["value"]
    assert m["flip"] <= rec["flip"] and m["flips"] == 0
    assert m["excess"] <= rec["excess"]
    assert m["aside"] <= T.SET_ASIDE_CAP
    k = T.LOWP_STATUS_FACTOR[dtype]
    assert k in (4.0, 2.0, 1.0)
    if k < 4.0:                                  # the next larger factor is over the cap
        ref = T.scene_reference("fp64")
        aside = (T.miss_clearance(ref) < T.lowp_status_margin(dtype, 2 * k)) | \
            T.scene_lost(dtype, 2 * k)
        print("   factor", 2 * k, "would set aside", aside.mean())
        assert aside.mean() > T.SET_ASIDE_CAP
    g = T.load_scene_golden(os.path.join(ROOT, "tests", "golden", T.GOLDEN))
    for a, b in zip(g["window"][dtype], T.scene_window(dtype)):
        assert np.array_equal(a, b)
    assert np.array_equal(g["lost"][dtype], T.scene_lost(dtype))
    st = g["status"][0]
    t_lo, t_hi = (x[0] for x in g["window"][dtype])
    assert np.isfinite(t_lo[st == T.HIT]).all() and (t_lo <= g["t"][0] + 1e-6)[st == T.HIT].all()
    assert (t_hi >= g["t"][0] - 1e-6)[st == T.HIT].all()
