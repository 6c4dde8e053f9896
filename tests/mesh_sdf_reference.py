"""fp64 numpy restatement of ``mesh_sdf``'s three definitions, the reference of
tests/test_mesh_sdf_reference.py (known answers) and tests/test_gpu_mesh_sdf.py (the kernel).

Brute force over every point-triangle pair, chunked over points.

* distance: exact closest point on a triangle in Voronoi-region form (Ericson, Real-Time
  Collision Detection §5.1.5); a division whose denominator is exactly 0 yields 0, so a
  zero-area triangle behaves as its segment or point.
* closest face: the lexicographic minimum of ``(d^2, index)``.
* winding number: ``w = sum_f Omega_f / 4 pi`` with Van Oosterom-Strackee's
  ``Omega = 2 atan2(A . (B x C), |A||B||C| + (A.B)|C| + (B.C)|A| + (C.A)|B|)``; a pair whose
  triple product is exactly 0 contributes 0.
* sign: ``sdf = -d`` if ``w > 0.5`` else ``+d``.
"""
from __future__ import annotations

import numpy as np


def _dot(a, b):
    return (a * b).sum(-1)


def _sdiv(n, d):
    """n / d, 0 where d == 0."""
    ok = d != 0
    return np.where(ok, n / np.where(ok, d, 1.0), 0.0)


def closest_uv(p, a, b, c):
    """Barycentric ``(v, w)`` of the closest point ``a + v (b - a) + w (c - a)`` for broadcast
    arrays ``[..., 3]``, regions tested in Ericson's order A, B, AB, C, AC, BC, face."""
    ab, ac = b - a, c - a
    ap, bp, cp = p - a, p - b, p - c
    d1, d2 = _dot(ab, ap), _dot(ac, ap)
    d3, d4 = _dot(ab, bp), _dot(ac, bp)
    d5, d6 = _dot(ab, cp), _dot(ac, cp)
    vc = d1 * d4 - d3 * d2
    vb = d5 * d2 - d1 * d6
    va = d3 * d6 - d5 * d4
    one, zero = np.ones_like(d1), np.zeros_like(d1)
    # face region first, every earlier region then overrides it (reverse priority)
    nv, nw, den = vb, vc, va + vb + vc
    bc = (va <= 0) & (d4 - d3 >= 0) & (d5 - d6 >= 0)                 # edge BC: b + t (c - b)
    nw, den = np.where(bc, d4 - d3, nw), np.where(bc, (d4 - d3) + (d5 - d6), den)
    for m, mv, mw, md in (
            ((vb <= 0) & (d2 >= 0) & (d6 <= 0), zero, d2, d2 - d6),  # edge AC
            ((d6 >= 0) & (d5 <= d6), zero, one, one),                # vertex C
            ((vc <= 0) & (d1 >= 0) & (d3 <= 0), d1, zero, d1 - d3),  # edge AB
            ((d3 >= 0) & (d4 <= d3), one, zero, one),                # vertex B
            ((d1 <= 0) & (d2 <= 0), zero, zero, one)):               # vertex A
        nv, nw, den = np.where(m, mv, nv), np.where(m, mw, nw), np.where(m, md, den)
        bc = bc & ~m
    v, w = _sdiv(nv, den), _sdiv(nw, den)
    v = np.where(bc, 1.0 - w, v)              # a zero-length edge b == c is the point b
    return v, w


def pair_dist2(p, a, b, c):
    """Squared distance point-triangle for broadcast ``[..., 3]`` arrays."""
    v, w = closest_uv(p, a, b, c)
    diff = (p - a) - v[..., None] * (b - a) - w[..., None] * (c - a)
    return _dot(diff, diff)


def pair_solid_angle_half(p, a, b, c):
    """``Omega / 2`` of the triangle seen from ``p`` (0 where the triple product is 0)."""
    A, B, C = a - p, b - p, c - p
    det = _dot(A, np.cross(B, C))
    la, lb, lc = (np.sqrt(_dot(x, x)) for x in (A, B, C))
    den = la * lb * lc + _dot(A, B) * lc + _dot(B, C) * la + _dot(C, A) * lb
    return np.where(det == 0, 0.0, np.arctan2(det, den))


def mesh_sdf_ref(verts, faces, points, chunk=256):
    """``(sdf, closest, winding, d)`` as fp64 / int64 arrays ``[P]``."""
    v = np.asarray(verts, np.float64).reshape(-1, 3)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    pts = np.asarray(points, np.float64).reshape(-1, 3)
    P, F = len(pts), len(f)
    d = np.full(P, np.inf)
    closest = np.full(P, -1, np.int64)
    wind = np.zeros(P)
    if F and P:
        a, b, c = v[f[:, 0]][None], v[f[:, 1]][None], v[f[:, 2]][None]
        for s in range(0, P, chunk):
            p = pts[s:s + chunk, None, :]
            d2 = pair_dist2(p, a, b, c)
            i = d2.argmin(1)                  # first minimum: the smaller index wins a tie
            closest[s:s + chunk] = i
            d[s:s + chunk] = np.sqrt(d2[np.arange(len(i)), i])
            wind[s:s + chunk] = pair_solid_angle_half(p, a, b, c).sum(1) / (2 * np.pi)
    sdf = np.where(wind > 0.5, -d, d)
    return sdf, closest, wind, d


def dist_to_face(verts, faces, points, face_id):
    """fp64 distance from ``points[i]`` to the one face ``face_id[i]``."""
    v = np.asarray(verts, np.float64)
    f = np.asarray(faces, np.int64)[np.asarray(face_id, np.int64)]
    p = np.asarray(points, np.float64)
    return np.sqrt(pair_dist2(p, v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]))


# ------------------------------------------------------------------------------ test meshes
def cube_mesh(h=0.5):
    """12 outward-facing triangles, corners at +-h."""
    v = np.array([[x, y, z] for z in (-h, h) for y in (-h, h) for x in (-h, h)], np.float32)
    quads = [(0, 2, 3, 1), (4, 5, 7, 6), (0, 1, 5, 4), (2, 6, 7, 3), (0, 4, 6, 2), (1, 3, 7, 5)]
    f = []
    for q in quads:
        f += [(q[0], q[1], q[2]), (q[0], q[2], q[3])]
    return v, np.array(f, np.int32)


def box_sdf(p, h=0.5):
    q = np.abs(np.asarray(p, np.float64)) - h
    return np.linalg.norm(np.maximum(q, 0), axis=-1) + np.minimum(q.max(-1), 0)


def icosphere(subdiv=2, radius=0.8):
    """Icosahedron subdivided ``subdiv`` times (20 * 4^subdiv faces), outward winding."""
    t = (1 + 5 ** 0.5) / 2
    v = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t),
         (0, 1, -t), (t, 0, -1), (t, 0, 1), (-t, 0, -1), (-t, 0, 1)]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4),
         (11, 10, 2), (10, 7, 6), (7, 1, 8), (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9),
         (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    v = [np.array(x, np.float64) / np.linalg.norm(x) for x in v]
    for _ in range(subdiv):
        mid, nf = {}, []

        def m(i, j):
            k = (min(i, j), max(i, j))
            if k not in mid:
                x = v[i] + v[j]
                v.append(x / np.linalg.norm(x))
                mid[k] = len(v) - 1
            return mid[k]
        for a, b, c in f:
            ab, bc, ca = m(a, b), m(b, c), m(c, a)
            nf += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = nf
    return (np.array(v) * radius).astype(np.float32), np.array(f, np.int32)


def hemisphere(subdiv=2, radius=0.8):
    """The icosphere's faces whose centroid has z > 0: an open mesh."""
    v, f = icosphere(subdiv, radius)
    keep = v[f].mean(1)[:, 2] > 0
    return v, np.ascontiguousarray(f[keep])


def cube_with_degenerates():
    """The cube plus three zero-area faces on dyadic coordinates (exact in fp32 and fp64):
    ``[i, i, i]``, a collinear triple and ``[i, j, j]``."""
    v, f = cube_mesh()
    extra = np.array([[0.875, 0.875, 0.875], [0.75, 0.875, 0.875], [0.5, 0.875, 0.875]],
                     np.float32)
    n = len(v)
    deg = np.array([[n, n, n], [n, n + 1, n + 2], [n, n + 2, n + 2]], np.int32)
    return np.concatenate([v, extra]), np.concatenate([f, deg])


def surface_points(verts, faces, n, rng):
    """``n`` area-weighted surface points (fp64) of a mesh."""
    v = np.asarray(verts, np.float64)
    f = np.asarray(faces, np.int64)
    a, b, c = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
    area = 0.5 * np.linalg.norm(np.cross(b - a, c - a), axis=1)
    i = rng.choice(len(f), size=n, p=area / area.sum())
    r1, r2 = np.sqrt(rng.random(n)), rng.random(n)
    return (a[i] * (1 - r1)[:, None] + b[i] * (r1 * (1 - r2))[:, None] +
            c[i] * (r1 * r2)[:, None])
