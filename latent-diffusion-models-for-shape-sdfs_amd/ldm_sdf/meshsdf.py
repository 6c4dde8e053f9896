"""Meshes -> DeepSDF training samples: the first stage of the path.

``mesh_sdf`` runs the HIP kernels of ``csrc/mesh_sdf.hip``: for every query point the distance
to the closest triangle (every point-triangle pair, no acceleration structure), that triangle's
index and the generalized winding number, whose comparison with 0.5 signs the distance on
meshes that are not watertight.  ``normalize_mesh``, ``sample_surface`` and ``sample_sdf``
follow DeepSDF's ``PreprocessMesh`` recipe around it; they are torch plumbing.

A point's outputs are a pure function of the point and the mesh: bitwise the same whether it is
evaluated alone or among a million others.
"""
from __future__ import annotations

import math
from typing import Optional, Sequence, Tuple

import torch

from . import _capi as capi

__all__ = ["mesh_sdf", "normalize_mesh", "sample_surface", "sample_sdf", "face_chunk",
           "split_below"]

# points per ``mesh_sdf`` call of ``sample_sdf`` (above ``split_below()``: the one-pass form)
POINT_CHUNK = 1 << 19


def face_chunk() -> int:
    """Faces per chunk of the kernel's fixed summation shape (a compile-time constant)."""
    return int(capi.load().ldm_mesh_sdf_face_chunk())


def split_below() -> int:
    """Calls with fewer points than this (and more than one face chunk) split the launch over
    face chunks and add the partials in chunk order: the same sums, more workgroups."""
    return int(capi.load().ldm_mesh_sdf_split_below())


def _check_mesh(verts: torch.Tensor, faces: torch.Tensor) -> None:
    if verts.dim() != 2 or verts.shape[1] != 3 or verts.dtype != torch.float32:
        raise capi.LdmError("mesh: verts must be a float32 [V, 3] tensor")
    if faces.dim() != 2 or faces.shape[1] != 3 or faces.dtype not in (torch.int32, torch.int64):
        raise capi.LdmError("mesh: faces must be an int32 [F, 3] tensor")


def _check_indices(verts: torch.Tensor, faces: torch.Tensor) -> None:
    if faces.shape[0] == 0:
        return
    lo, hi = (int(x) for x in torch.stack(torch.aminmax(faces)).cpu())
    if lo < 0 or hi >= verts.shape[0]:
        raise capi.LdmError(f"mesh: face indices span [{lo}, {hi}], outside the "
                            f"{verts.shape[0]} vertices")


def mesh_sdf(verts: torch.Tensor, faces: torch.Tensor, points: torch.Tensor, *,
             return_closest: bool = False, return_winding: bool = False,
             _validated: bool = False):
    """Signed distance ``[P]`` from ``points [P, 3]`` to the triangle soup ``verts [V, 3]``
    fp32, ``faces [F, 3]`` int32: ``-d`` where the winding number exceeds 0.5, else ``+d``.

    With ``return_closest`` / ``return_winding`` the result is a tuple that also carries the
    closest face ``[P]`` int32 (the smaller index on a tie) and the winding number ``[P]``.
    No faces give ``+inf``, ``-1`` and ``0``.  Device tensors only; a face index outside
    ``[0, V)`` raises ``LdmError`` (checked with one min/max over ``faces``; the kernel clamps
    and flags what would still get through).
    """
    capi.require_device(verts, faces, points)
    _check_mesh(verts, faces)
    if points.dim() != 2 or points.shape[1] != 3 or points.dtype != torch.float32:
        raise capi.LdmError("mesh_sdf: points must be a float32 [P, 3] tensor")
    if not (verts.device == faces.device == points.device):
        raise capi.LdmError("mesh_sdf: verts, faces and points must share a device")
    if not _validated:
        _check_indices(verts, faces)
    dev = points.device
    V, F, P = verts.shape[0], faces.shape[0], points.shape[0]
    if F > 0 and V == 0:
        raise capi.LdmError("mesh_sdf: faces without vertices")
    verts, points = verts.contiguous(), points.contiguous()
    faces = faces.to(torch.int32).contiguous()
    sdf = torch.empty(P, device=dev, dtype=torch.float32)
    closest = torch.empty(P, device=dev, dtype=torch.int32) if return_closest else None
    winding = torch.empty(P, device=dev, dtype=torch.float32) if return_winding else None
    if P > 0:
        lib = capi.load()
        ws = torch.empty(lib.ldm_mesh_sdf_ws_bytes(F, P), device=dev, dtype=torch.uint8)
        flag = torch.empty(1, device=dev, dtype=torch.int32)
        with torch.cuda.device(dev):
            capi.check(lib.ldm_mesh_sdf(capi.ptr(verts), V, capi.ptr(faces), F,
                                        capi.ptr(points), P, capi.ptr(sdf), capi.ptr(closest),
                                        capi.ptr(winding), capi.ptr(flag), capi.ptr(ws),
                                        ws.numel(), capi.stream_handle(dev)), "ldm_mesh_sdf")
        if int(flag.item()) != 0:
            raise capi.LdmError("mesh_sdf: a face index outside [0, V) was clamped by the "
                                "kernel; the outputs are meaningless")
    out = (sdf,) + ((closest,) if return_closest else ()) + ((winding,) if return_winding else ())
    return out[0] if len(out) == 1 else out


def normalize_mesh(verts: torch.Tensor, buffer: float = 1.03):
    """DeepSDF's normalisation: the bounding-box centre to the origin and the farthest vertex
    to radius ``1 / buffer``.  Returns ``(verts_n, offset, scale)`` with ``verts_n = (verts +
    offset) * scale``; ``offset`` is a CPU float32 ``[3]`` tensor and ``scale`` a float, the
    pair ``write_ply(offset=, scale=)`` undoes (``p / scale - offset``)."""
    v = torch.as_tensor(verts, dtype=torch.float32)
    if v.dim() != 2 or v.shape[1] != 3 or v.shape[0] == 0:
        raise ValueError("normalize_mesh: verts must be a non-empty [V, 3] tensor")
    centre = (v.amax(0) + v.amin(0)) * 0.5
    offset = -centre
    far = float((v + offset).norm(dim=1).max())
    if not far > 0.0:
        raise ValueError("normalize_mesh: all vertices coincide")
    scale = 1.0 / (far * float(buffer))
    return (v + offset) * scale, offset.cpu(), scale


def _rand(shape, dev, generator, normal=False, dtype=torch.float32):
    """Uniform [0, 1) or standard normal on ``dev``, drawn where the generator lives."""
    gdev = generator.device if generator is not None else dev
    fn = torch.randn if normal else torch.rand
    return fn(shape, generator=generator, device=gdev, dtype=dtype).to(dev)


def sample_surface(verts: torch.Tensor, faces: torch.Tensor, n: int,
                   generator: Optional[torch.Generator] = None
                   ) -> Tuple[torch.Tensor, torch.Tensor]:
    """``n`` points uniform over the surface: a face picked by area (fp64 CDF,
    ``torch.searchsorted``; a zero-area face is never picked) and uniform barycentric
    coordinates.  Returns ``(xyz [n, 3] fp32, face_id [n] int64)`` on ``verts``' device."""
    _check_mesh(verts, faces)
    if faces.shape[0] == 0:
        raise ValueError("sample_surface: the mesh has no faces")
    dev = verts.device
    tri = verts.double()[faces.long()]                         # [F, 3, 3]
    a, b, c = tri[:, 0], tri[:, 1], tri[:, 2]
    area = torch.linalg.cross(b - a, c - a).norm(dim=1) * 0.5
    cdf = torch.cumsum(area, 0)
    if not float(cdf[-1]) > 0.0:
        raise ValueError("sample_surface: the mesh has no area")
    u = _rand((n, 3), dev, generator, dtype=torch.float64)
    fid = torch.searchsorted(cdf, u[:, 0] * cdf[-1], right=True).clamp_(max=faces.shape[0] - 1)
    r1, r2 = u[:, 1].sqrt()[:, None], u[:, 2][:, None]
    xyz = a[fid] * (1 - r1) + b[fid] * (r1 * (1 - r2)) + c[fid] * (r1 * r2)
    return xyz.float(), fid


def sample_sdf(verts: torch.Tensor, faces: torch.Tensor, n: int = 500_000, *,
               variances: Sequence[float] = (0.005, 0.0005), near_fraction: float = 47 / 50,
               generator: Optional[torch.Generator] = None
               ) -> Tuple[torch.Tensor, torch.Tensor]:
    """DeepSDF's ``PreprocessMesh`` recipe on a normalised mesh: ``near_fraction * n / 2``
    surface points, each perturbed once by ``N(0, variances[0])`` and once by ``N(0,
    variances[1])``, the rest of the ``n`` uniform in ``[-1, 1]^3``; all through ``mesh_sdf``
    (in chunks of ``POINT_CHUNK`` points).  Returns ``(pos, neg)``: ``[., 4]`` fp32 rows
    ``(x, y, z, sdf)`` with ``sdf >= 0`` and ``sdf < 0``."""
    capi.require_device(verts, faces)
    _check_mesh(verts, faces)
    _check_indices(verts, faces)
    n = int(n)
    if n < 0 or not 0.0 <= near_fraction <= 1.0 or len(variances) != 2:
        raise ValueError("sample_sdf: n >= 0, near_fraction in [0, 1], two variances")
    dev = verts.device
    ns = int(near_fraction * n / 2)
    parts = []
    if ns > 0:
        surf, _ = sample_surface(verts, faces, ns, generator)
        for var in variances:
            parts.append(surf + _rand((ns, 3), dev, generator, normal=True) * math.sqrt(var))
    parts.append(_rand((n - 2 * ns, 3), dev, generator) * 2.0 - 1.0)
    xyz = torch.cat(parts).contiguous()
    sdf = torch.cat([mesh_sdf(verts, faces, xyz[s:s + POINT_CHUNK], _validated=True)
                     for s in range(0, max(n, 1), POINT_CHUNK)])
    rows = torch.cat([xyz, sdf[:, None]], dim=1)
    keep = sdf >= 0
    return rows[keep], rows[~keep]
