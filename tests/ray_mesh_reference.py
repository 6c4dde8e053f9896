"""References for ``ray_mesh``, used by tests/test_ray_mesh_reference.py (known
answers), tests/test_render_host.py (the header, watertightness) and tests/test_gpu_ray_mesh.py
(the kernel).

* ``ray_mesh_ref``: fp64 Möller-Trumbore against every face, the closest hit (both sides of a
  triangle count, edges inclusive, the smaller index on a tie).  The oracle.
* ``pair_emul`` / ``ray_mesh_emul``: the fp32 operation sequence of csrc/ray_tri_pair.h in numpy
  float32, op for op -- the watertight test of Woop, Benthin and Wald.  The C++ header must
  equal it bit for bit.
* ``ray_segment_distance``: fp64 distance between a ray and a segment, which tells a ray that
  grazes a mesh edge (where fp32 and fp64 may honestly disagree) from one that does not.
* the rays the host and the device tests share: ``edge_aimed_rays``, ``random_rays``, and the
  fp64 restatement of the camera and the shading (``camera_rays_ref``, ``shade_ref``).
"""
from __future__ import annotations

import numpy as np

U24 = 2.0 ** -24


def _dot(a, b):
    return (a * b).sum(-1)


# ------------------------------------------------------------------------------- fp64 oracle
def mt_pairs(o, d, a, b, c):
    """fp64 Möller-Trumbore for broadcast ``[..., 3]`` arrays: ``(hit, t, u, v)`` with the hit
    point ``a + u (b - a) + v (c - a)``; ``t`` is not range-checked."""
    e1, e2 = b - a, c - a
    p = np.cross(d, e2)
    det = _dot(e1, p)
    ok = det != 0
    inv = 1.0 / np.where(ok, det, 1.0)
    tv = o - a
    u = _dot(tv, p) * inv
    q = np.cross(tv, e1)
    v = _dot(d, q) * inv
    t = _dot(e2, q) * inv
    return ok & (u >= 0) & (v >= 0) & (u + v <= 1), t, u, v


def ray_mesh_ref(verts, faces, origins, dirs, t_min=0.0, t_max=np.inf, chunk=256):
    """``(t, face)``: fp64 ``[R]`` (``+inf`` for a miss) and int64 ``[R]`` (``-1``)."""
    v = np.asarray(verts, np.float64).reshape(-1, 3)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    o = np.asarray(origins, np.float64).reshape(-1, 3)
    d = np.asarray(dirs, np.float64).reshape(-1, 3)
    R = len(o)
    t_out, face = np.full(R, np.inf), np.full(R, -1, np.int64)
    if len(f) and R:
        a, b, c = v[f[:, 0]][None], v[f[:, 1]][None], v[f[:, 2]][None]
        with np.errstate(all="ignore"):
            for s in range(0, R, chunk):
                hit, t, _, _ = mt_pairs(o[s:s + chunk, None], d[s:s + chunk, None], a, b, c)
                hit &= (t >= t_min) & (t <= t_max)
                t = np.where(hit, t, np.inf)
                i = t.argmin(1)                       # first minimum: the smaller index
                tt = t[np.arange(len(i)), i]
                t_out[s:s + chunk] = tt
                face[s:s + chunk] = np.where(np.isfinite(tt), i, -1)
    return t_out, face


def plane_t(verts, faces, origins, dirs, face_id):
    """fp64 ``t`` at which ray ``i`` meets the plane of face ``face_id[i]``."""
    v = np.asarray(verts, np.float64)
    f = np.asarray(faces, np.int64)[np.asarray(face_id, np.int64)]
    o, d = np.asarray(origins, np.float64), np.asarray(dirs, np.float64)
    a = v[f[:, 0]]
    n = np.cross(v[f[:, 1]] - a, v[f[:, 2]] - a)
    with np.errstate(all="ignore"):
        return _dot(n, a - o) / _dot(n, d)


def face_normals(verts, faces):
    """fp64 unit normals ``[F, 3]`` (zero for a zero-area face)."""
    v = np.asarray(verts, np.float64)
    f = np.asarray(faces, np.int64)
    n = np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]])
    ln = np.linalg.norm(n, axis=1, keepdims=True)
    return n / np.where(ln > 0, ln, 1.0)


def t_bound(origins, dirs, t_ref, normal):
    """The parity bound of the GPU tests: ``8 u (|o| + t) / |n . d^|`` with u = 2^-24: one
    rounding of ``o`` and ``d`` plus the pair's dozen operations, amplified by the obliquity."""
    o, d = np.asarray(origins, np.float64), np.asarray(dirs, np.float64)
    dh = d / np.linalg.norm(d, axis=1, keepdims=True)
    cos = np.abs(_dot(normal, dh))
    with np.errstate(all="ignore"):
        return 8 * U24 * (np.linalg.norm(o, axis=1) + t_ref * np.linalg.norm(d, axis=1)) / cos


def ray_segment_distance(o, d, p, q):
    """fp64 distance between the rays ``o + t d, t >= 0`` and the segments ``p q``, for
    broadcast ``[..., 3]`` arrays (clamped closest points, Ericson §5.1.9 with the ray's
    parameter clamped below only)."""
    o, d, p, q = (np.asarray(x, np.float64) for x in (o, d, p, q))
    e = q - p
    r = o - p
    a, ee, fz = _dot(d, d), _dot(e, e), _dot(e, r)
    b, cc = _dot(d, e), _dot(d, r)
    den = a * ee - b * b
    with np.errstate(all="ignore"):
        s = np.where(den > 0, (b * fz - cc * ee) / np.where(den > 0, den, 1.0), 0.0)
        s = np.maximum(s, 0.0)
        t = np.where(ee > 0, (b * s + fz) / np.where(ee > 0, ee, 1.0), 0.0)
        t = np.clip(t, 0.0, 1.0)
        s = np.maximum((t * b - cc) / np.where(a > 0, a, 1.0), 0.0)
    diff = (o + s[..., None] * d) - (p + t[..., None] * e)
    return np.sqrt(_dot(diff, diff))


def mesh_edges(faces):
    """Unique undirected edges ``[E, 2]`` (int64) of a face list."""
    f = np.asarray(faces, np.int64)
    e = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    return np.unique(np.sort(e, axis=1), axis=0)


def min_edge_distance(verts, faces, origins, dirs, chunk=64):
    """fp64 distance from each ray to the nearest mesh edge."""
    v = np.asarray(verts, np.float64)
    e = mesh_edges(faces)
    p, q = v[e[:, 0]][None], v[e[:, 1]][None]
    o, d = np.asarray(origins, np.float64), np.asarray(dirs, np.float64)
    out = np.empty(len(o))
    for s in range(0, len(o), chunk):
        out[s:s + chunk] = ray_segment_distance(o[s:s + chunk, None], d[s:s + chunk, None],
                                                p, q).min(1)
    return out


# ------------------------------------------------------------------------ the fp32 emulation
def _sel(x, k):
    return np.take_along_axis(x, k[..., None], -1)[..., 0]


def ray_setup_emul(o, d):
    """``kx, ky, kz, Sx, Sy, Sz, ok`` of csrc/ray_tri_pair.h's ``ray_setup`` for ``[..., 3]``
    float32 arrays."""
    o, d = np.asarray(o, np.float32), np.asarray(d, np.float32)
    ad = np.abs(d)
    kz = np.zeros(d.shape[:-1], np.int64)
    m = ad[..., 0]
    g = ad[..., 1] > m
    kz, m = np.where(g, 1, kz), np.where(g, ad[..., 1], m)
    kz = np.where(ad[..., 2] > m, 2, kz)
    kx = (kz + 1) % 3
    ky = (kx + 1) % 3
    dk = _sel(d, kz)
    neg = dk < 0
    kx, ky = np.where(neg, ky, kx), np.where(neg, kx, ky)
    with np.errstate(all="ignore"):
        Sx, Sy, Sz = _sel(d, kx) / dk, _sel(d, ky) / dk, np.float32(1) / dk
    ok = (dk != 0) & np.isfinite(dk) & np.isfinite(o).all(-1)
    return kx, ky, kz, Sx, Sy, Sz, ok


def pair_emul(o, d, a, b, c, t_min=0.0, t_max=np.inf):
    """The pair of csrc/ray_tri_pair.h in numpy float32 for broadcast ``[..., 3]`` arrays:
    ``(hit, t, bary [..., 3])``, ``t`` and ``bary`` meaningful where ``hit``."""
    o, d, a, b, c = (np.asarray(x, np.float32) for x in (o, d, a, b, c))
    t_min, t_max = np.float32(t_min), np.float32(t_max)
    kx, ky, kz, Sx, Sy, Sz, ok = ray_setup_emul(o, d)
    with np.errstate(all="ignore"):
        sh = []
        for p in (a, b, c):
            q = p - o                                  # q = vertex - o, first
            shape = q.shape[:-1]
            k = _sel(q, np.broadcast_to(kz, shape))
            qx = _sel(q, np.broadcast_to(kx, shape)) - Sx * k
            qy = _sel(q, np.broadcast_to(ky, shape)) - Sy * k
            sh.append((qx, qy, k))
        (Ax, Ay, Ak), (Bx, By, Bk), (Cx, Cy, Ck) = sh
        U = Cx * By - Cy * Bx
        V = Ax * Cy - Ay * Cx
        W = Bx * Ay - By * Ax
        for x in (U, V, W, Ax):
            assert x.dtype == np.float32
        neg = (U < 0) | (V < 0) | (W < 0)
        pos = (U > 0) | (V > 0) | (W > 0)
        det = (U + V) + W
        cand = ~(neg & pos) & (det != 0) & ok
        T = (U * (Sz * Ak) + V * (Sz * Bk)) + W * (Sz * Ck)
        t = T / det
        hit = cand & (t >= t_min) & (t <= t_max)
        bary = np.stack([U / det, V / det, W / det], -1)
    assert t.dtype == np.float32 and bary.dtype == np.float32
    return hit, t, bary


def ray_mesh_emul(verts, faces, origins, dirs, t_min=0.0, t_max=np.inf, chunk=256):
    """``(t [R] float32, face [R] int32, bary [R, 3] float32)``: the lexicographic minimum of
    ``(t, face)`` over the hits of ``pair_emul``; a miss is ``+inf, -1, 0``."""
    v = np.asarray(verts, np.float32).reshape(-1, 3)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    o = np.asarray(origins, np.float32).reshape(-1, 3)
    d = np.asarray(dirs, np.float32).reshape(-1, 3)
    R = len(o)
    t_out = np.full(R, np.inf, np.float32)
    face = np.full(R, -1, np.int32)
    bary = np.zeros((R, 3), np.float32)
    if len(f) and R:
        a, b, c = v[f[:, 0]][None], v[f[:, 1]][None], v[f[:, 2]][None]
        for s in range(0, R, chunk):
            hit, t, w = pair_emul(o[s:s + chunk, None], d[s:s + chunk, None], a, b, c, t_min,
                                  t_max)
            t = np.where(hit, t, np.float32(np.inf))
            i = t.argmin(1)
            rows = np.arange(len(i))
            tt = t[rows, i]
            got = hit[rows, i]
            t_out[s:s + chunk] = np.where(got, tt, np.float32(np.inf))
            face[s:s + chunk] = np.where(got, i, -1)
            bary[s:s + chunk] = np.where(got[:, None], w[rows, i], np.float32(0))
    return t_out, face, bary


# ------------------------------------------------------------------------------ shared rays
def unit_dirs_f32(x):
    """fp64 vectors normalised, then rounded once to float32."""
    x = np.asarray(x, np.float64)
    return (x / np.linalg.norm(x, axis=-1, keepdims=True)).astype(np.float32)


def edge_aimed_rays(verts, faces, seed):
    """Rays aimed at one float32 point on every edge and at every vertex of a mesh, seen nearly
    head-on: origins 2 to 2.5 away, within 30 degrees of the outward normal there (the mean of
    the unit normals of the faces around the edge or vertex).  Returns ``(origins, dirs)``
    float32 (``dirs`` unit to one rounding) and the fp64 ``|target - origin|`` per ray."""
    rng = np.random.default_rng(seed)
    v = np.asarray(verts, np.float64)
    f = np.asarray(faces, np.int64)
    fn = face_normals(verts, faces)
    vn = np.zeros_like(v)
    for k in range(3):
        np.add.at(vn, f[:, k], fn)
    e = mesh_edges(f)
    s = rng.uniform(0.05, 0.95, len(e))[:, None]
    on_edge = (v[e[:, 0]] * (1 - s) + v[e[:, 1]] * s).astype(np.float32).astype(np.float64)
    en = np.zeros((len(e), 3))
    key = {tuple(x): i for i, x in enumerate(e.tolist())}
    for k in range(3):
        pair = np.sort(f[:, [k, (k + 1) % 3]], axis=1)
        np.add.at(en, [key[tuple(x)] for x in pair.tolist()], fn)
    target = np.concatenate([on_edge, v])
    n = np.concatenate([en, vn])
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    # a direction within 30 degrees of n: n + tan(30 deg) r, |r| <= 1
    r = rng.standard_normal(n.shape)
    r *= (rng.random(len(n)) ** (1 / 3) / np.linalg.norm(r, axis=1))[:, None]
    out = n + np.tan(np.pi / 6) * r
    out /= np.linalg.norm(out, axis=1, keepdims=True)
    origin = (target + out * rng.uniform(2.0, 2.5, len(n))[:, None]).astype(np.float32)
    dirs = unit_dirs_f32(target - origin.astype(np.float64))
    return origin, dirs, np.linalg.norm(target - origin.astype(np.float64), axis=1)


def random_rays(n, seed):
    """``n`` rays with origins at radius 1.2 to 3 aimed at targets uniform in the ball of radius
    0.85: float32 ``(origins, dirs)``, directions unit to one rounding."""
    rng = np.random.default_rng(seed)

    def ball(m):
        x = rng.standard_normal((m, 3))
        return x / np.linalg.norm(x, axis=1, keepdims=True)
    o = (ball(n) * rng.uniform(1.2, 3.0, (n, 1))).astype(np.float32)
    target = ball(n) * (0.85 * rng.random((n, 1)) ** (1 / 3))
    return o, unit_dirs_f32(target - o.astype(np.float64))


def torus_volume(N):
    """The torus of tests/test_gpu_mc.py on the oracle's grid, float32 ``[N, N, N]``."""
    from oracle import ref_mc
    c = ref_mc._coords(N)
    z, y, x = np.meshgrid(c, c, c, indexing="ij")
    return (np.sqrt((np.sqrt(x * x + y * y) - 0.5) ** 2 + z * z) - 0.2).astype(np.float32)


def torus_mesh_cpu(N=24):
    """The CPU oracle's marching-cubes mesh of the ``N^3`` torus: closed, consistently wound."""
    from oracle import ref_mc
    return ref_mc.marching_cubes(torus_volume(N))


WATERTIGHT_MESHES = ("icosphere1", "icosphere2", "icosphere3", "torus24")
WATERTIGHT_SLACK = 2e-6        # DESIGN.md §16's fp32 distance bound


def watertight_case(name):
    """``(verts, faces, origins, dirs, dist)`` of one of ``WATERTIGHT_MESHES``: the mesh and
    its edge- and vertex-aimed rays (a fixed seed per mesh)."""
    from tests import mesh_sdf_reference as M
    i = WATERTIGHT_MESHES.index(name)
    v, f = torus_mesh_cpu(24) if name == "torus24" else M.icosphere(i + 1)
    return (v, f) + edge_aimed_rays(v, f, seed=100 + i)


def is_closed_and_oriented(faces):
    """Every directed edge has its opposite exactly once (and occurs once itself)."""
    f = np.asarray(faces, np.int64)
    e = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    fwd = sorted(map(tuple, e.tolist()))
    back = sorted(map(tuple, e[:, ::-1].tolist()))
    return fwd == back and len(set(fwd)) == len(fwd)


# ------------------------------------------------------------------- camera, shading (fp64)
def look_at_ref(eye, target, up=(0.0, 1.0, 0.0)):
    """Camera-to-world pose ``[4, 4]`` fp64 by Gram-Schmidt: the camera's backward axis is
    ``eye - target`` normalised, its up axis is ``up`` with the backward part removed, its
    right axis completes the right-handed frame; the last column is the eye."""
    eye, target, up = (np.asarray(x, np.float64) for x in (eye, target, up))
    back = eye - target
    back /= np.linalg.norm(back)
    true_up = up - (up @ back) * back
    true_up /= np.linalg.norm(true_up)
    pose = np.eye(4)
    pose[:3, 0], pose[:3, 1], pose[:3, 2], pose[:3, 3] = np.cross(true_up, back), true_up, back, eye
    return pose


def camera_rays_ref(pose, fov_y_deg, height, width):
    """Pinhole rays by the intrinsics: focal length ``f = (height / 2) / tan(fov_y / 2)`` in
    pixels, principal point at the image centre, pixel ``(r, c)`` seen through the point
    ``(c + 1/2, r + 1/2)``, y down in the image and up in the camera, which looks along -z.
    Float32 ``(origins, dirs)`` in row-major pixel order."""
    pose = np.asarray(pose, np.float64)
    f = (height / 2) / np.tan(np.radians(fov_y_deg) / 2)
    d = np.empty((height, width, 3))
    for r in range(height):
        for c in range(width):
            cam = np.array([(c + 0.5 - width / 2) / f, -(r + 0.5 - height / 2) / f, -1.0])
            d[r, c] = pose[:3, :3] @ cam
    d = d.reshape(-1, 3)
    o = np.broadcast_to(pose[:3, 3], d.shape)
    return o.astype(np.float32), unit_dirs_f32(d)


def shade_ref(normals, dirs, mask, background=1.0):
    """Headlight Lambert ``|n . d^|`` as uint8 grey ``[R]`` (rounded to nearest), the
    background value off the mesh."""
    n, d = np.asarray(normals, np.float64), np.asarray(dirs, np.float64)
    dh = d / np.linalg.norm(d, axis=1, keepdims=True)
    lam = np.where(mask, np.abs(_dot(n, dh)), background)
    return np.clip(np.floor(lam * 255 + 0.5), 0, 255).astype(np.uint8)
