"""Numpy restatement of the sphere tracer (csrc/ray_brick_dda.h and
csrc/sdf_trace.hip): the same algorithm with the same fp32 operations in the same order, for any
callable field and an optional brick mask, so that the device's ``t``, status, steps and lists
can be held to it BIT FOR BIT; a brute-force check of the brick walk by dense fp64 sampling;
the closed-form ray-octahedron hit of the L1-ball network; and the tolerance constants of
tests/test_gpu_sdf_trace.py with the way each was obtained."""
import math

import numpy as np

F32 = np.float32
BRICK = 8
MISS, HIT, ACTIVE = 0, 1, 2

# ---- tolerance constants ------------------------------------------------------------------
# §8(c): the decoder's value error per dtype against the fp64 decoder
DELTA_T = {"fp32": 2e-6, "fp16": 2e-3, "bf16": 1e-2}
# Scenes 3 / 4 (seed-1234 decoder, latent randn(seed 0) x 0.1, level -0.1, lipschitz 0.45,
# eps 1e-3, the 24 x 24 camera at (2.2, 1.6, 1.3)); the fp64 reference run is stored in
# tests/golden/sdf_trace_scene.npz (tests/test_sdf_trace_reference.py recomputes it).
#
# STATUS.  A ray's status is ambiguous when a small shift of the field changes it; such rays
# are set aside from the status comparison, at most SET_ASIDE_CAP of all rays.
#   * A ray the reference does NOT hit has a clearance: the smallest f - eps over its
#     evaluations.  It is set aside when that is below the margin.
#   * A ray the reference HITS is set aside when it is no hit in the fp64 run of the scene with
#     the level LOWERED by the margin: its stop is that shallow, and the field never goes
#     deeper behind it.  (The smallest f - eps "before the stop" of a hit says nothing about
#     its status: the last approach of every hit is a run of values just above eps, 228 of the
#     347 hits are below 5 eps there.)  The ray that showed the need: fp64 stops it 8.7e-5
#     below eps at its last evaluation in the box, the bf16 field is 5.8e-4 ABOVE eps at that
#     point (a value error of 6.6e-4, bf16's largest on the scene is 2.5e-3), the ray leaves
#     the box; the fp64 run with the level lowered by eps already loses it.
# fp32: the margin is 5 eps on the misses (19 rays, 3.3 %) and no hit is set aside.  16-bit: one
# margin on both sides, k x the emulation's largest value error against fp64 with k the
# largest of 4, 2, 1 that keeps the rays set aside under the cap -- fp16 4 x 4.2e-4 (2.3 %
# set aside), bf16 1 x 2.6e-3 (3.8 %; 2 x is over the cap); the device's values equal the emulation's at the
# reference's points (largest error 2.529e-3 both), so k covers trajectories, not arithmetic.
# The emulation itself flips no status ("flip" below).
# T.  Two runs of one ray with fields that differ by less than a margin can stop far apart
# where the ray grazes the surface: one stops at the graze, the other passes it and hits what
# lies behind (the bf16 emulation against fp64: three rays, up to 0.97 apart).  No single t
# tolerance holds for such a ray, so a 16-bit common hit is held to the WINDOW
# [t_lo - tol, t_hi + tol] of two more fp64 runs of the scene: t_lo with the level raised by the
# t margin (it stops where f - level <= eps + margin: no field within the margin of fp64 stops
# before the first such point), t_hi with the level lowered by eps + margin (it stops where
# f - level <= -margin: there a field within the margin is below its own level, and a sound
# march cannot pass that).  Both are stored with the golden run.  Where the t_hi run does not
# hit, only the lower end is held.  The t margin is 4 x the emulation's largest value error.
STATUS_MARGIN = 5e-3                       # 5 eps: fp32, reference misses only
LOWP_STATUS_FACTOR = {"fp16": 4.0, "bf16": 1.0}
SET_ASIDE_CAP = 0.05


def fp32_t_tol(lipschitz, eps, steps):
    """One step of stop ambiguity plus §8(c)'s fp32 bound per evaluation; fp32 common hits are
    held to |dt| <= this with no window."""
    return eps / lipschitz + steps * 2e-6 / lipschitz


# 16-bit, measured on a CPU with the lowp emulation (oracle decoder_forward_lowp) against the
# fp64 field by measure_lowp(), re-measured by tests/test_sdf_trace_reference.py:
#   "value"  the largest |lowp - fp64| of the field at the points the fp64 run evaluated
#            (4.17e-4 and 2.53e-3 measured)
#   "flip"   the largest clearance of a ray whose status the emulation flips (none flipped)
#   "excess" by how much the emulation's t leaves the window with tol = 0, at worst (nothing)
# The test's t margin is 4 x value; its tol is 4 x excess, and at least one step at that
# margin, (eps + margin) / lipschitz.
MEASURED_LOWP = {"fp16": {"value": 4.2e-4, "flip": 0.0, "excess": 0.0},
                 "bf16": {"value": 2.6e-3, "flip": 0.0, "excess": 0.0}}


def lowp_margin(dtype):
    """The t margin of the window."""
    return 4.0 * MEASURED_LOWP[dtype]["value"]


def lowp_status_margin(dtype, factor=None):
    return (LOWP_STATUS_FACTOR[dtype] if factor is None else factor) * \
        MEASURED_LOWP[dtype]["value"]


def lowp_t_tol(dtype, lipschitz, eps):
    return max(4.0 * MEASURED_LOWP[dtype]["excess"], (eps + lowp_margin(dtype)) / lipschitz)


# ---- the geometry, as csrc/ray_brick_dda.h ------------------------------------------------
def n_bricks(N):
    return (int(N) + BRICK - 1) // BRICK


def voxel_size(N, bbox):
    return F32((bbox[1] - bbox[0]) / (N - 1))


def bounds(N, vs, origin):
    """The nb + 1 brick boundaries along an axis: fl(fl(min(8 b, N - 1) vs) + origin)."""
    i = np.minimum(BRICK * np.arange(n_bricks(N) + 1), N - 1).astype(F32)
    return (i * F32(vs)).astype(F32) + F32(origin)


def cell(x, bnd):
    """#{b in [1, nb - 1] : x >= bound(b)}"""
    nb = len(bnd) - 1
    return (x[..., None] >= bnd[1:nb]).sum(-1).astype(np.int64)


def point_at(o, d, t):
    with np.errstate(all="ignore"):
        return (o + (t[:, None] * d).astype(F32)).astype(F32)


def dir_len(d):
    xx, yy, zz = d[:, 0] * d[:, 0], d[:, 1] * d[:, 1], d[:, 2] * d[:, 2]
    return np.sqrt(((xx + yy).astype(F32) + zz).astype(F32)).astype(F32)


def clip(o, d, lo, hi, t_min, t_max):
    """(ok, t0, t1) of the slab clip against [lo, hi]^3 and [t_min, t_max]."""
    lo, hi = F32(lo), F32(hi)
    n = len(o)
    ok = np.isfinite(o).all(1) & np.isfinite(d).all(1) & (d != 0).any(1)
    a0, a1 = np.full(n, t_min, F32), np.full(n, t_max, F32)
    with np.errstate(all="ignore"):
        for a in range(3):
            nz = d[:, a] != 0
            inv = (F32(1) / np.where(nz, d[:, a], F32(1))).astype(F32)
            ta = ((lo - o[:, a]) * inv).astype(F32)
            tb = ((hi - o[:, a]) * inv).astype(F32)
            mn, mx = np.where(ta < tb, ta, tb), np.where(ta > tb, ta, tb)
            a0 = np.where(nz, np.where(a0 > mn, a0, mn), a0)
            a1 = np.where(nz, np.where(a1 < mx, a1, mx), a1)
            ok &= nz | ~((o[:, a] < lo) | (o[:, a] > hi))
        ok &= a0 <= a1
    return ok, a0.astype(F32), a1.astype(F32)


def skip(o, d, t, t_end, mask3, bnd):
    """(alive, t') of the 3D-DDA to the next active brick; ``mask3`` is [nb, nb, nb] (z, y, x)
    of the rays' shape."""
    nb = len(bnd) - 1
    n = len(o)
    t = t.astype(F32).copy()
    alive = np.zeros(n, bool)
    todo = np.ones(n, bool)
    c = cell(point_at(o, d, t), bnd)
    step = np.where(d > 0, 1, -1)
    with np.errstate(all="ignore"):
        inv = (F32(1) / np.where(d != 0, d, F32(1))).astype(F32)
        for _ in range(3 * nb + 3):
            idx = np.nonzero(todo)[0]
            if len(idx) == 0:
                break
            cc, tt = c[idx], t[idx]
            act = mask3[cc[:, 2], cc[:, 1], cc[:, 0]].astype(bool)
            alive[idx[act]] = True
            tn = np.full(len(idx), np.inf, F32)
            ax = np.full(len(idx), -1)
            for a in range(3):
                face = bnd[np.clip(np.where(step[idx, a] > 0, cc[:, a] + 1, cc[:, a]), 0, nb)]
                x = ((face - o[idx, a]) * inv[idx, a]).astype(F32)
                take = (d[idx, a] != 0) & ((ax < 0) | (x < tn))
                tn = np.where(take, x, tn)
                ax = np.where(take, a, ax)
            rows = np.arange(len(idx))
            axc = np.maximum(ax, 0)
            cn = cc.copy()
            cn[rows, axc] += step[idx, axc]
            out = (ax < 0) | (cn[rows, axc] < 0) | (cn[rows, axc] >= nb)
            t2 = np.where(tt > tn, tt, tn).astype(F32)
            gone = ~act & (out | ~(t2 <= t_end[idx]))
            go = ~act & ~gone
            c[idx[go]] = cn[go]
            t[idx[go]] = t2[go]
            todo[idx[act | gone]] = False
    return alive, t


def trace_reference(field, origins, dirs, B, *, bbox=(-1.0, 1.0), level=0.0, lipschitz=1.0,
                    eps=1e-3, max_steps=256, t_min=0.0, t_max=math.inf, mask=None, N=0,
                    keep=False):
    """The tracer in numpy.  ``field(b, pts, rays, k)`` returns the values (any float type;
    rounded to fp32) of shape ``b`` at ``pts [n, 3]`` fp32, for its rays ``rays [n]`` in round
    ``k``.  ``origins``, ``dirs``: ``[R, 3]`` or ``[B, R, 3]``.  ``mask``: ``[B nb^3]`` flags for
    an ``N^3`` grid, or None.  Returns a dict: ``t`` (+inf unless hit), ``t_work`` (the state
    array: +inf for a miss), ``status``, ``steps``, ``xyz`` (last evaluated point, NaN for none),
    ``clearance`` (the smallest f - eps over the evaluations that did not stop the ray, +inf for
    none, from the field's own unrounded values), ``hist`` (every evaluation: shape, ray, t,
    f - eps, whether it stopped the ray) with ``hist_xyz`` its points, and with ``keep`` per round
    ``lists`` (per shape the marching rays) and ``points``."""
    o = np.ascontiguousarray(np.broadcast_to(np.asarray(origins, F32), (B,) + origins.shape[-2:]))
    d = np.ascontiguousarray(np.broadcast_to(np.asarray(dirs, F32), (B,) + dirs.shape[-2:]))
    R = o.shape[1]
    lo, hi = F32(bbox[0]), F32(bbox[1])
    level, lipschitz, eps = F32(level), F32(lipschitz), F32(eps)
    bnd = m4 = None
    if mask is not None:
        nb = n_bricks(N)
        bnd = bounds(N, voxel_size(N, bbox), lo)
        m4 = np.asarray(mask).reshape(B, nb, nb, nb)
    t = np.full((B, R), np.inf, F32)
    t_end = np.full((B, R), np.inf, F32)
    status = np.zeros((B, R), np.int32)
    steps = np.zeros((B, R), np.int32)
    xyz = np.full((B, R, 3), np.nan, F32)
    clearance = np.full((B, R), np.inf)
    for b in range(B):
        ok, t0, t1 = clip(o[b], d[b], lo, hi, F32(t_min), F32(t_max))
        if mask is not None and ok.any():
            i = np.nonzero(ok)[0]
            al, t0[i] = skip(o[b][i], d[b][i], t0[i], t1[i], m4[b], bnd)
            ok[i] = al
        t[b] = np.where(ok, t0, np.inf)
        t_end[b] = np.where(ok, t1, np.inf)      # (the device keeps t1 of a clipped miss: unused)
        status[b] = np.where(ok, ACTIVE, MISS)
    lists, points, hist = [], [], []
    for k in range(max_steps):
        cur = [np.nonzero(status[b] == ACTIVE)[0].astype(np.int32) for b in range(B)]
        if max(len(c) for c in cur) == 0:
            break
        if keep:
            lists.append(cur)
            points.append([point_at(o[b][c], d[b][c], t[b][c]) for b, c in enumerate(cur)])
        for b, c in enumerate(cur):
            if len(c) == 0:
                continue
            ob, db, tb = o[b][c], d[b][c], t[b][c]
            p = point_at(ob, db, tb)
            xyz[b, c] = p
            raw = np.asarray(field(b, p, c, k))
            v = raw.astype(F32)
            with np.errstate(all="ignore"):
                f = (v - level).astype(F32)
                hit = ~np.isfinite(f) | (f <= eps)
                den = (lipschitz * dir_len(db)).astype(F32)
                q = (np.where(f > eps, f, eps) / den).astype(F32)
                t2 = (tb + q).astype(F32)
            alive = ~hit & (t2 <= t_end[b][c])
            if mask is not None and alive.any():
                i = np.nonzero(alive)[0]
                al, t2[i] = skip(ob[i], db[i], t2[i], t_end[b][c][i], m4[b], bnd)
                alive[i] = al
            steps[b, c] += 1
            status[b, c] = np.where(hit, HIT, np.where(alive, ACTIVE, MISS))
            t[b, c] = np.where(hit, tb, np.where(alive, t2, np.inf))
            go = ~hit
            clr = raw.astype(np.float64) - float(level) - float(eps)
            clearance[b, c[go]] = np.minimum(clearance[b, c[go]], clr[go])
            hist.append((np.full(len(c), b), c, tb.copy(), clr, hit, p))
    out = {"t": np.where(status == HIT, t, np.inf).astype(F32), "t_work": t, "status": status,
           "steps": steps, "xyz": xyz, "clearance": clearance}
    cat = (lambda i, dt: np.concatenate([h[i] for h in hist]).astype(dt) if hist
           else np.zeros(0, dt))
    out["hist"] = {"b": cat(0, np.int32), "ray": cat(1, np.int32), "t": cat(2, F32),
                   "clr": cat(3, np.float64), "stop": cat(4, bool)}
    out["hist_xyz"] = np.concatenate([h[5] for h in hist]) if hist else np.zeros((0, 3), F32)
    if keep:
        out["lists"], out["points"] = lists, points
    return out


def miss_clearance(ref):
    """Per ray ``[B, R]``: for a ray the reference does not hit the smallest f - eps over its
    evaluations; +inf for a ray that hits or was never evaluated."""
    h, st = ref["hist"], ref["status"]
    out = np.full(st.shape, np.inf)
    use = st[h["b"], h["ray"]] != HIT
    np.minimum.at(out, (h["b"][use], h["ray"][use]), h["clr"][use])
    return out


def point_field(fn):
    """A field of the point alone: ``fn(b, pts)``."""
    return lambda b, pts, rays, k: fn(b, pts)


# ---- brute force for the brick walk -------------------------------------------------------
def brick_of(p, bnd):
    """Brick indices (x, y, z) of points [n, 3] by the rule of cell()."""
    return cell(np.asarray(p, F32), bnd)


def in_active_brick(p, mask3, bnd, tol=4e-6):
    """Whether each point [n, 3] lies in the closure of an active brick, widened by ``tol`` for
    the rounding of o + t d (a ray enters a brick ON its face)."""
    nb = len(bnd) - 1
    p = np.asarray(p, np.float64)
    ok = np.zeros(len(p), bool)
    for sx in (-tol, tol):
        for sy in (-tol, tol):
            for sz in (-tol, tol):
                q = p + np.array([sx, sy, sz])
                c = (q[..., None] >= bnd[1:nb].astype(np.float64)).sum(-1)
                ok |= mask3[c[:, 2], c[:, 1], c[:, 0]].astype(bool)
    return ok


def walk_brute(o, d, t0, t_end, mask3, bnd, samples=20000):
    """Dense fp64 sampling of one ray: the smallest sampled t in [t0, t_end] whose point lies
    in an active brick (None: there is none), with the bricks located in fp64 against the same
    boundaries."""
    nb = len(bnd) - 1
    ts = np.linspace(float(t0), float(t_end), samples)
    p = np.asarray(o, np.float64)[None] + ts[:, None] * np.asarray(d, np.float64)[None]
    c = (p[..., None] >= bnd[1:nb].astype(np.float64)).sum(-1)
    act = mask3[c[:, 2], c[:, 1], c[:, 0]].astype(bool)
    hit = np.nonzero(act)[0]
    return None if len(hit) == 0 else (ts[hit[0]], ts[1] - ts[0])


# ---- closed forms ---------------------------------------------------------------------------
def sphere_hit(o, d, radius):
    """fp64: the smallest t >= 0 with |o + t d| = radius for rays starting outside, +inf for a
    miss; rays starting inside return 0."""
    o, d = np.asarray(o, np.float64), np.asarray(d, np.float64)
    a, b, c = (d * d).sum(1), (o * d).sum(1), (o * o).sum(1) - radius * radius
    disc = b * b - a * c
    with np.errstate(all="ignore"):
        t = (-b - np.sqrt(np.maximum(disc, 0))) / a
    t = np.where((disc >= 0) & (t >= 0), t, np.inf)
    return np.where(c <= 0, 0.0, t)


def octahedron_hit(o, d, rho):
    """fp64: entry t of the rays into the L1 ball |x| + |y| + |z| <= rho (+inf for a miss, 0
    from inside), and the smallest value of |x|_1 - rho along t >= 0."""
    o, d = np.asarray(o, np.float64), np.asarray(d, np.float64)
    n = len(o)
    t_in, t_out = np.zeros(n), np.full(n, np.inf)
    for sx in (-1, 1):
        for sy in (-1, 1):
            for sz in (-1, 1):
                s = np.array([sx, sy, sz], np.float64)
                so, sd = o @ s - rho, d @ s                # s.x - rho <= 0 inside
                with np.errstate(all="ignore"):
                    tc = -so / sd
                t_in = np.where(sd < 0, np.maximum(t_in, tc), t_in)
                t_out = np.where(sd > 0, np.minimum(t_out, tc), t_out)
                t_out = np.where((sd == 0) & (so > 0), -np.inf, t_out)
    t_hit = np.where(t_in <= t_out, t_in, np.inf)
    # |x(t)|_1 is convex and piecewise linear: its minimum over t >= 0 is at 0 or at a zero of
    # a coordinate
    with np.errstate(all="ignore"):
        cand = np.concatenate([np.zeros((n, 1)), np.where(d != 0, -o / d, 0.0)], axis=1)
    cand = np.where(np.isfinite(cand) & (cand > 0), cand, 0.0)
    val = np.abs(o[:, None, :] + cand[:, :, None] * d[:, None, :]).sum(-1) - rho
    return t_hit, val.min(1)


# ---- the camera of scenes 3, 4 and 7 -------------------------------------------------------
SCENE = dict(level=-0.1, lipschitz=0.45, eps=1e-3, max_steps=256)
SCENE_EYE, SCENE_FOV, SCENE_HW = (2.2, 1.6, 1.3), 50.0, 24


def scene_rays():
    """The 576 rays of the 24 x 24 camera at SCENE_EYE looking at the origin, z up."""
    from ldm_sdf import camera_rays, look_at
    o, d = camera_rays(look_at(SCENE_EYE, (0.0, 0.0, 0.0), (0.0, 0.0, 1.0)), SCENE_FOV, SCENE_HW,
                       SCENE_HW)
    return o.numpy(), d.numpy()


def scene_field(kind):
    """The scene's field on a CPU as a ``trace_reference`` callable: "fp64" (the oracle),
    "fp32" (the oracle run in fp32), or "fp16" / "bf16" (the oracle's lowp emulation)."""
    import torch
    from oracle import ref_cpu as R
    p = R.make_decoder_params(seed=1234)
    p32 = p.to(torch.float32)
    z = (torch.randn(1, 256, generator=torch.Generator().manual_seed(0)) * 0.1)

    def fn(b, pts):
        x = torch.from_numpy(np.ascontiguousarray(pts))[None]
        with torch.no_grad():
            if kind == "fp64":
                return R.decoder_forward(p, z.double(), x.double())[0].numpy()
            if kind == "fp32":
                return R.decoder_forward(p32, z.float(), x.float())[0].numpy()
            dt = {"fp16": torch.float16, "bf16": torch.bfloat16}[kind]
            return R.decoder_forward_lowp(p, z.double(), x.double(), dt)[0].numpy()
    return point_field(fn)


_SCENE_CACHE = {}


def scene_reference(kind, level_shift=0.0):
    """``trace_reference`` of the scene with the ``kind`` field (its level moved by
    ``level_shift``), computed once and shared."""
    key = (kind, float(level_shift))
    if key not in _SCENE_CACHE:
        o, d = scene_rays()
        kw = dict(SCENE, level=SCENE["level"] + level_shift)
        _SCENE_CACHE[key] = trace_reference(scene_field(kind), o, d, 1, **kw)
    return _SCENE_CACHE[key]


def scene_window(dtype):
    """(t_lo, t_hi) ``[1, R]`` of the fp64 runs that bracket a ``dtype`` run (see T. above);
    +inf where a run does not hit."""
    m = lowp_margin(dtype)
    return (scene_reference("fp64", m)["t"].astype(np.float64),
            scene_reference("fp64", -(SCENE["eps"] + m))["t"].astype(np.float64))


def scene_lost(dtype, factor=None):
    """``[1, R]`` bool: the rays the fp64 reference hits that are no hit in the fp64 run with
    the level lowered by the ``dtype`` status margin."""
    m = lowp_status_margin(dtype, factor)
    return (scene_reference("fp64")["status"] == HIT) & \
        (scene_reference("fp64", -m)["status"] != HIT)


def compare_runs(ref, got_status, got_t, margin, window=None, lost=None):
    """``got`` against the reference dict ``ref``: the share of rays set aside (reference misses
    of clearance below ``margin`` and the reference hits flagged in ``lost``), status flips
    outside them, the largest clearance of a
    flipped reference miss, the largest |dt| of the common hits, and with a ``window`` (t_lo,
    t_hi) the largest excess of a common hit's t beyond it (an infinite t_hi holds nothing)."""
    st, clr = ref["status"].reshape(-1), miss_clearance(ref).reshape(-1)
    gs, gt = np.asarray(got_status).reshape(-1), np.asarray(got_t, np.float64).reshape(-1)
    aside = clr < margin
    if lost is not None:
        aside = aside | (np.asarray(lost).reshape(-1) & (st == HIT))
    flip = st != gs
    both = (st == HIT) & (gs == HIT)
    dt = np.abs(ref["t"].reshape(-1).astype(np.float64)[both] - gt[both])
    fc = clr[flip]
    out = {"flips": int((flip & ~aside).sum()),
           "flip_clearance": float(fc[np.isfinite(fc)].max()) if np.isfinite(fc).any() else 0.0,
           "dt": float(dt.max()) if dt.size else 0.0}
    if window is not None:
        t_lo, t_hi = (np.asarray(x, np.float64).reshape(-1) for x in window)
        ex = np.maximum(np.maximum(t_lo[both] - gt[both], gt[both] - t_hi[both]), 0.0)
        out["excess"] = float(ex.max()) if ex.size else 0.0
    out["aside"] = float(aside.mean())
    return out


def measure_lowp(dtype):
    """The lowp emulation against the fp64 field on the scene: what MEASURED_LOWP records
    (``excess`` with the margin of the recorded constants)."""
    ref, low = scene_reference("fp64"), scene_reference(dtype)
    v64 = ref["hist"]["clr"] + SCENE["level"] + SCENE["eps"]
    vlo = np.asarray(scene_field(dtype)(0, ref["hist_xyz"], None, 0), np.float64)
    c = compare_runs(ref, low["status"], low["t"], lowp_status_margin(dtype),
                     scene_window(dtype), scene_lost(dtype))
    return {"value": float(np.abs(vlo - v64).max()),
            "flip": compare_runs(ref, low["status"], low["t"], 0.0)["flip_clearance"],
            "excess": c["excess"], "aside": c["aside"], "flips": c["flips"]}


GOLDEN = "sdf_trace_scene.npz"
_GOLDEN_KEYS = ("t", "t_work", "status", "steps")


def save_scene_golden(path):
    r = scene_reference("fp64")
    win = {f"{k}_{dt}": w for dt in ("fp16", "bf16")
           for k, w in zip(("t_lo", "t_hi"), scene_window(dt))}
    win.update({"lost_" + dt: scene_lost(dt) for dt in ("fp16", "bf16")})
    np.savez_compressed(path, **{k: r[k] for k in _GOLDEN_KEYS}, **win,
                        **{"hist_" + k: v for k, v in r["hist"].items()})


def load_scene_golden(path):
    """The stored fp64 run as ``trace_reference`` returns it (without the points), and per
    16-bit dtype its window under ``"window"`` and its shallow hits under ``"lost"``."""
    z = np.load(path)
    r = {k: z[k] for k in _GOLDEN_KEYS}
    r["hist"] = {k: z["hist_" + k] for k in ("b", "ray", "t", "clr", "stop")}
    r["window"] = {dt: (z["t_lo_" + dt], z["t_hi_" + dt]) for dt in ("fp16", "bf16")}
    r["lost"] = {dt: z["lost_" + dt] for dt in ("fp16", "bf16")}
    return r
