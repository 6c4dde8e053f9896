"""Ray casting against meshes: renders and depth-map SDF samples.

``ray_mesh`` runs the HIP kernels of ``csrc/ray_mesh.hip``: the closest intersection of every
ray with every triangle (no acceleration structure), by the watertight test of Woop, Benthin
and Wald in plain fp32 -- a ray through a shared edge or vertex of a closed mesh never slips
between the triangles.  Around it, as torch and host plumbing: a pinhole camera (``look_at``,
``camera_rays``), ``render_mesh`` (mask, depth, normals, a headlight-shaded image),
``write_png`` / ``read_png``, and ``depth_samples``, DeepSDF §6.3's two SDF samples per depth
pixel, shaped for ``fit_latents``.

A ray's outputs are a pure function of the ray, the mesh and the bounds: bitwise the same
whether it is cast alone or among a million others.
"""
from __future__ import annotations

import math
import struct
import zlib
from typing import Dict, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _capi as capi
from . import ops
from .meshsdf import _check_indices, _check_mesh

__all__ = ["ray_mesh", "look_at", "camera_rays", "render_mesh", "write_png", "read_png",
           "depth_samples", "face_chunk", "split_below", "trace_sdf", "render_sdf",
           "estimate_lipschitz", "skip_mask"]


def face_chunk() -> int:
    """Faces per workgroup of the split launch form (a compile-time constant)."""
    return int(capi.load().ldm_ray_mesh_face_chunk())


def split_below() -> int:
    """Calls with fewer rays than this (and more than one face chunk) split the launch over
    face chunks and take the minimum of the partials: the same result, more workgroups."""
    return int(capi.load().ldm_ray_mesh_split_below())


def ray_mesh(verts: torch.Tensor, faces: torch.Tensor, origins: torch.Tensor,
             dirs: torch.Tensor, *, t_min: float = 0.0, t_max: float = math.inf,
             return_bary: bool = False):
    """Closest hit of the rays ``origins + t dirs`` (``[R, 3]`` fp32; ``dirs`` need not be
    unit) with the triangle soup ``verts [V, 3]`` fp32, ``faces [F, 3]`` int32, for ``t`` in
    ``[t_min, t_max]``; both sides of a triangle count.

    Returns ``t [R]`` (``+inf`` for a miss) and ``face [R]`` int32 (the smaller index on a tie,
    ``-1`` for a miss), and with ``return_bary`` the weights ``[R, 3]`` of the face's three
    vertices at the hit (0 for a miss).  A ray with a zero or non-finite direction or a
    non-finite origin misses.  Device tensors only; a face index outside ``[0, V)`` raises
    ``LdmError`` (checked with one min/max over ``faces``; the kernel clamps and flags what
    would still get through).
    """
    capi.require_device(verts, faces, origins, dirs)
    _check_mesh(verts, faces)
    for name, x in (("origins", origins), ("dirs", dirs)):
        if x.dim() != 2 or x.shape[1] != 3 or x.dtype != torch.float32:
            raise capi.LdmError(f"ray_mesh: {name} must be a float32 [R, 3] tensor")
    if origins.shape[0] != dirs.shape[0]:
        raise capi.LdmError("ray_mesh: origins and dirs must have the same number of rays")
    if not (verts.device == faces.device == origins.device == dirs.device):
        raise capi.LdmError("ray_mesh: verts, faces, origins and dirs must share a device")
    t_min, t_max = float(t_min), float(t_max)
    if not t_min <= t_max:
        raise capi.LdmError(f"ray_mesh: need t_min <= t_max, got [{t_min}, {t_max}]")
    _check_indices(verts, faces)
    if faces.shape[0] > 0 and verts.shape[0] == 0:
        raise capi.LdmError("ray_mesh: faces without vertices")
    t, face, bary, flag = ops.ray_mesh(verts.contiguous(), faces.to(torch.int32).contiguous(),
                                       origins.contiguous(), dirs.contiguous(), t_min, t_max,
                                       return_bary)
    if origins.shape[0] > 0 and int(flag.item()) != 0:
        raise capi.LdmError("ray_mesh: a face index outside [0, V) was clamped by the kernel; "
                            "the outputs are meaningless")
    return (t, face, bary) if return_bary else (t, face)


# ------------------------------------------------------------------------------ the camera
def look_at(eye: Sequence[float], target: Sequence[float],
            up: Sequence[float] = (0.0, 1.0, 0.0)) -> torch.Tensor:
    """Camera-to-world pose ``[4, 4]`` (fp64, CPU) of a camera at ``eye`` looking at
    ``target``: the columns are the camera's right, up and backward axes (it looks along its
    own -z, OpenGL's convention) and its position."""
    e, tg, u = (np.asarray(x.tolist() if isinstance(x, torch.Tensor) else x, np.float64)
                for x in (eye, target, up))
    fwd = tg - e
    n = np.linalg.norm(fwd)
    if not n > 0:
        raise ValueError("look_at: eye and target coincide")
    fwd = fwd / n
    right = np.cross(fwd, u)
    n = np.linalg.norm(right)
    if not n > 0:
        raise ValueError("look_at: up is parallel to the viewing direction")
    right = right / n
    pose = np.eye(4)
    pose[:3, 0], pose[:3, 1], pose[:3, 2], pose[:3, 3] = right, np.cross(right, fwd), -fwd, e
    return torch.from_numpy(pose)


def _pose64(pose) -> np.ndarray:
    p = pose.detach().cpu().numpy() if isinstance(pose, torch.Tensor) else np.asarray(pose)
    p = p.astype(np.float64)
    if p.shape != (4, 4):
        raise ValueError("pose must be [4, 4]")
    return p


def camera_rays(pose, fov_y_deg: float, height: int, width: int,
                device=None) -> Tuple[torch.Tensor, torch.Tensor]:
    """Rays of a pinhole camera through the pixel centres, row 0 at the top: ``origins, dirs
    [height * width, 3]`` fp32 in row-major pixel order, on ``device`` (default: the CPU).
    ``fov_y_deg`` is the full vertical field of view.  The directions are computed in fp64 on
    the host, normalised, and rounded once to fp32."""
    p = _pose64(pose)
    height, width = int(height), int(width)
    if height <= 0 or width <= 0 or not 0.0 < fov_y_deg < 180.0:
        raise ValueError("camera_rays: height, width > 0 and 0 < fov_y_deg < 180")
    th = math.tan(math.radians(fov_y_deg) / 2)
    y = (1 - 2 * (np.arange(height) + 0.5) / height) * th
    x = (2 * (np.arange(width) + 0.5) / width - 1) * th * (width / height)
    xx, yy = np.meshgrid(x, y)
    cam = np.stack([xx, yy, -np.ones_like(xx)], -1).reshape(-1, 3)
    d = cam @ p[:3, :3].T
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    o = np.broadcast_to(p[:3, 3], d.shape)
    origins = torch.from_numpy(np.ascontiguousarray(o.astype(np.float32)))
    dirs = torch.from_numpy(d.astype(np.float32))
    return (origins, dirs) if device is None else (origins.to(device), dirs.to(device))


def _facing(n: torch.Tensor, d: torch.Tensor) -> torch.Tensor:
    """``n`` normalised (zero stays zero) and flipped to face the viewer of direction ``d``."""
    n = n / n.norm(dim=-1, keepdim=True).clamp_min(1e-30)
    return torch.where(((n * d).sum(-1, keepdim=True) > 0), -n, n)


def render_mesh(verts: torch.Tensor, faces: torch.Tensor, pose, fov_y_deg: float, height: int,
                width: int, *, vertex_normals: Optional[torch.Tensor] = None,
                background: float = 1.0) -> Dict[str, torch.Tensor]:
    """One image of a mesh from a pinhole camera (``look_at``, ``camera_rays``).  Returns

    * ``t [H, W]``, ``face [H, W]`` (int32): ``ray_mesh``'s outputs per pixel;
    * ``mask [H, W]`` (bool): the pixels that hit;
    * ``depth [H, W]``: the hit's distance along the camera's forward axis, ``+inf`` off the
      mesh;
    * ``normal [H, W, 3]``: the unit face normal, or with ``vertex_normals [V, 3]`` (for
      instance ``mesh.vertex_normals``) their barycentric blend renormalised; flipped to face
      the camera, zero off the mesh;
    * ``image [H, W, 3]`` (uint8): headlight Lambert shading ``|n . d|``, ``background`` (0..1)
      elsewhere;
    * ``origins``, ``dirs [H W, 3]``: the rays, as ``depth_samples`` takes them.

    The rays go through the HIP kernel; the shading is elementwise torch work over the pixels.
    """
    capi.require_device(verts, faces, vertex_normals)
    dev = verts.device
    p = _pose64(pose)
    o, d = camera_rays(p, fov_y_deg, height, width, device=dev)
    t, face, bary = ray_mesh(verts, faces, o, d, return_bary=True)
    if vertex_normals is not None and vertex_normals.shape != verts.shape:
        raise capi.LdmError("render_mesh: vertex_normals must be [V, 3] like verts")
    mask = face >= 0
    # gather over the hit pixels only: a mesh without faces (extract_mesh of a latent with no
    # zero crossing) has no row to read, and its image is all background
    hit = mask.nonzero()[:, 0]
    tri = faces.long()[face[hit].long()]                               # [M, 3]
    if vertex_normals is None:
        a, b, c = verts[tri[:, 0]], verts[tri[:, 1]], verts[tri[:, 2]]
        nh = torch.linalg.cross(b - a, c - a)
    else:
        nh = (vertex_normals.float()[tri] * bary[hit][:, :, None]).sum(1)
    n = torch.zeros_like(d)
    n[hit] = _facing(nh, d[hit])
    fwd = torch.tensor((-p[:3, 2]).astype(np.float32), device=dev)
    inf = torch.full_like(t, math.inf)
    depth = torch.where(mask, t * (d * fwd).sum(-1), inf)
    lam = torch.where(mask, (n * d).sum(-1).abs(), torch.full_like(t, float(background)))
    grey = (lam * 255.0 + 0.5).floor().clamp(0, 255).to(torch.uint8)
    H, W = int(height), int(width)
    return {"t": t.view(H, W), "face": face.view(H, W), "mask": mask.view(H, W),
            "depth": depth.view(H, W), "normal": n.view(H, W, 3),
            "image": grey.view(H, W, 1).expand(H, W, 3).contiguous(), "origins": o, "dirs": d}


def depth_samples(origins: torch.Tensor, dirs: torch.Tensor, t: torch.Tensor,
                  normals: torch.Tensor, *, eta: float = 0.01
                  ) -> Tuple[torch.Tensor, torch.Tensor]:
    """DeepSDF §6.3's samples of a depth map: for each of the ``M`` rays that hit (finite
    ``t``), the surface point ``p = o + t d`` moved by ``eta`` along the normal toward the
    camera, with SDF ``+eta``, and by ``eta`` away from it, with ``-eta``.  ``normals`` are per
    ray (``render_mesh``'s ``normal``; any leading shape over the rays); they are renormalised
    and flipped to face the ray's origin.  Returns ``xyz [2 M, 3]`` and ``sdf [2 M]`` -- the
    front points first -- so that ``xyz[None], sdf[None]`` go straight into ``fit_latents``."""
    o, d = origins.reshape(-1, 3), dirs.reshape(-1, 3)
    t, n = t.reshape(-1), normals.reshape(-1, 3)
    if not (o.shape[0] == d.shape[0] == t.shape[0] == n.shape[0]):
        raise ValueError("depth_samples: origins, dirs, t and normals must cover the same rays")
    hit = torch.isfinite(t)
    o, d, t, n = o[hit], d[hit], t[hit], n[hit]
    p = o + t[:, None] * d
    n = _facing(n.to(p.dtype), d)
    eta = float(eta)
    xyz = torch.cat([p + eta * n, p - eta * n])
    M = p.shape[0]
    sdf = torch.cat([torch.full((M,), eta, dtype=p.dtype, device=p.device),
                     torch.full((M,), -eta, dtype=p.dtype, device=p.device)])
    return xyz, sdf


# ------------------------------------------------------- sphere tracing
def _shade(mask, n, d, background):
    """``render_mesh``'s headlight Lambert image from facing unit normals (any leading shape)."""
    lam = torch.where(mask, (n * d).sum(-1).abs(),
                      torch.full(mask.shape, float(background), device=n.device))
    grey = (lam * 255.0 + 0.5).floor().clamp(0, 255).to(torch.uint8)
    return grey[..., None].expand(*grey.shape, 3).contiguous()


def skip_mask(desc, beta: torch.Tensor, N: int, bbox, level: float, lipschitz: float,
              eps: float) -> torch.Tensor:
    """The brick flags ``[B nb^3]`` (uint8) that ``trace_sdf`` skips by, for an ``N^3`` grid:
    ``decode_band``'s sequence (lattice coordinates, the decoder on them, ``band_classify``) with
    ``band = lipschitz 4 sqrt(3) voxel_size + eps``, and on top of its ``active`` flags every
    inactive brick that lies INSIDE the shape (corner-0 value <= level; all corners of an
    inactive brick are on one side).  A ray may only pass through bricks that are wholly
    outside: in a brick inside the shape its next evaluation is a hit, as without a mask."""
    B, nb = beta.shape[0], ops._nb(N)
    band = float(lipschitz) * 4.0 * math.sqrt(3.0) * ops.voxel_size(N, bbox) + float(eps)
    lat = ops.band_lattice_coords(N, bbox, device=beta.device)[None].expand(B, -1, -1).contiguous()
    coarse = ops.decoder_points_fwd(desc, beta, lat)
    active, _, _ = ops.band_classify(coarse, N, level, band)
    inside = coarse.view(B, nb + 1, nb + 1, nb + 1)[:, :nb, :nb, :nb] <= float(level)
    return torch.where(inside.reshape(-1), torch.ones_like(active), active).contiguous()


def trace_sdf(decoder, latents: torch.Tensor, origins: torch.Tensor, dirs: torch.Tensor, *,
              bbox: Tuple[float, float] = (-1.0, 1.0), level: float = 0.0,
              lipschitz: float = 1.0, eps: float = 1e-3, max_steps: int = 256,
              t_min: float = 0.0, t_max: float = math.inf, dtype: str = "auto",
              skip_resolution: Optional[int] = None, return_points: bool = False):
    """Sphere tracing of the decoded field of ``latents [B, L]``: the rays ``origins + t dirs``
    (``[R, 3]`` shared by the shapes, or ``[B, R, 3]``; fp32, ``dirs`` need not be unit and
    ``t`` is in units of it, as in ``ray_mesh``) marched inside ``bbox^3`` and ``[t_min, t_max]``
    to the first point with ``f = sdf - level <= eps``.

    A ray steps by ``max(f, eps) / (lipschitz |d|)``: it cannot pass through the surface of a
    field that changes by at most ``lipschitz`` per unit length.  A trained DeepSDF is not an
    exact distance; ``lipschitz`` is the caller's knob (``estimate_lipschitz`` measures a
    starting value), and a value below the field's true slope can step over thin parts.

    Returns ``t [B, R]`` (``+inf`` unless the ray hit), ``status [B, R]`` int32 (0 miss, 1 hit,
    2 still marching after ``max_steps`` evaluations), ``steps [B, R]`` int32 (decoder
    evaluations of the ray), and with ``return_points`` the point ``[B, R, 3]`` each ray was
    last evaluated at (NaN for a ray that never was).  A ray with a non-finite origin or a zero
    or non-finite direction misses.

    ``skip_resolution=N`` classifies the 8^3-voxel bricks of an ``N^3`` grid as ``decode_band``
    does (band ``lipschitz 4 sqrt(3) voxel_size + eps``) and moves every ray through the bricks
    that lie wholly OUTSIDE the shape without evaluating the decoder there (``skip_mask``); its
    soundness is ``decode_band``'s.  Bricks wholly inside the shape are not passed through: a
    ray that starts inside the shape hits at its first point, as without skipping.

    Each round is one decoder launch over all shapes (``decode_points``'s kernel, ``dtype`` as
    in ``decode``) and one read of ``B`` counts back to the host.  A ray's outputs are bitwise
    the same alone, in any batch and in any order of the rays."""
    from .api import resolve_decode_dtype
    capi.require_device(latents, origins, dirs)
    if latents.dim() == 1:
        latents = latents[None]
    if latents.dim() != 2 or latents.shape[1] != decoder.latent_dim:
        raise ValueError(f"latents must be [B, {decoder.latent_dim}]")
    B = latents.shape[0]
    if origins.shape != dirs.shape or origins.dim() not in (2, 3) or origins.shape[-1] != 3 \
            or (origins.dim() == 3 and origins.shape[0] != B):
        raise ValueError("trace_sdf: origins and dirs must both be [R, 3] or [B, R, 3]")
    lo, hi = float(bbox[0]), float(bbox[1])
    level, lipschitz, eps = float(level), float(lipschitz), float(eps)
    t_min, t_max, max_steps = float(t_min), float(t_max), int(max_steps)
    if not (math.isfinite(lo) and math.isfinite(hi) and lo < hi):
        raise ValueError("trace_sdf: bbox must be finite with lo < hi")
    if not (eps > 0.0 and math.isfinite(eps)) or not (lipschitz > 0.0 and math.isfinite(lipschitz)):
        raise ValueError("trace_sdf: eps and lipschitz must be positive and finite")
    if max_steps < 1 or not t_min <= t_max or math.isnan(level):
        raise ValueError("trace_sdf: need max_steps >= 1, t_min <= t_max and a level")
    if skip_resolution is not None and int(skip_resolution) < 2:
        raise ValueError("trace_sdf: skip_resolution must be >= 2")
    dev = latents.device
    if origins.device != dev or dirs.device != dev:
        raise capi.LdmError("trace_sdf: latents, origins and dirs must share a device")
    dtype = resolve_decode_dtype(dtype, latents)
    desc = decoder.device_pack(dtype, dev)["desc"]
    beta = ops.decoder_fold(desc, latents.float().contiguous())
    mask, N = None, 0
    if skip_resolution is not None:
        N = int(skip_resolution)
        mask = skip_mask(desc, beta, N, bbox, level, lipschitz, eps)
    st = ops.SdfTraceState(origins.float().contiguous(), dirs.float().contiguous(), B, bbox,
                           level, lipschitz, eps, mask, N, return_points)
    if st.R > 0:
        ops.sdf_trace_init(st, t_min, t_max, max_steps)
        pts = vals = dws = None
        for _ in range(max_steps):
            P = max(st.counts.tolist())              # the round's one synchronisation
            if P == 0:
                break
            if pts is None:                          # the counts only fall: sized once
                pts = torch.empty(B * P * 3, device=dev)
                vals = torch.empty(B * P, device=dev)
                dws = torch.empty(max(capi.load().ldm_workspace_bytes_layout(
                    capi.LDM_OP_DECODER_POINTS, B, P, desc.dtype, desc.layout), 16),
                    device=dev, dtype=torch.uint8)
            xyz = ops.sdf_trace_emit(st, P, pts[:B * P * 3].view(B, P, 3))
            ops.sdf_trace_step(st, ops.decoder_points_fwd(desc, beta, xyz,
                                                          vals[:B * P].view(B, P), dws))
    t = torch.where(st.status == 1, st.t, torch.full_like(st.t, math.inf))
    out = (t, st.status, st.steps)
    return out + (st.xyz_last,) if return_points else out


def render_sdf(decoder, latents: torch.Tensor, pose, fov_y_deg: float, height: int, width: int,
               *, background: float = 1.0, **trace_kw) -> Dict[str, torch.Tensor]:
    """Images of the decoded shapes ``latents [B, L]`` from one pinhole camera, without a
    mesh: ``trace_sdf`` on the camera's rays (``trace_kw`` are its keyword arguments).  The
    dict has ``render_mesh``'s entries except ``face``, batched: ``t``, ``mask``, ``depth``
    ``[B, H, W]``, ``normal [B, H, W, 3]`` -- the field's gradient at the hit points
    (``sdf_grad``, fp16), normalised and flipped to face the camera, zero off the shape --
    ``image [B, H, W, 3]`` uint8 with the same headlight Lambert shading, and ``origins``,
    ``dirs [H W, 3]``.  ``t[b]`` and ``normal[b]`` go into ``depth_samples`` unchanged."""
    from .grad import sdf_grad
    capi.require_device(latents)
    if latents.dim() == 1:
        latents = latents[None]
    dev = latents.device
    p = _pose64(pose)
    o, d = camera_rays(p, fov_y_deg, height, width, device=dev)
    trace_kw.pop("return_points", None)
    t, status, _, xyz = trace_sdf(decoder, latents, o, d, return_points=True, **trace_kw)
    mask = status == 1
    B, H, W = latents.shape[0], int(height), int(width)
    pts = torch.where(mask[..., None], xyz, torch.zeros_like(xyz))
    _, g = sdf_grad(decoder, latents, pts)
    n = torch.where(mask[..., None], _facing(g, d[None]), torch.zeros_like(g))
    fwd = torch.tensor((-p[:3, 2]).astype(np.float32), device=dev)
    depth = torch.where(mask, t * (d * fwd).sum(-1)[None], torch.full_like(t, math.inf))
    return {"t": t.view(B, H, W), "mask": mask.view(B, H, W), "depth": depth.view(B, H, W),
            "normal": n.view(B, H, W, 3),
            "image": _shade(mask, n, d[None], background).view(B, H, W, 3),
            "origins": o, "dirs": d}


def estimate_lipschitz(decoder, latents: torch.Tensor, resolution: int = 32, *,
                       bbox: Tuple[float, float] = (-1.0, 1.0),
                       dtype: str = "fp16") -> torch.Tensor:
    """The largest gradient norm ``|grad sdf|`` that ``sdf_grad`` finds on a ``resolution^3``
    grid over ``bbox^3``, per shape: ``[B]``.  An ESTIMATE FROM SAMPLES, NOT A BOUND: the
    gradient of a ReLU network is piecewise constant and a steeper piece can lie between the
    samples, so multiply by a margin before using it as ``trace_sdf``'s or ``decode_band``'s
    ``lipschitz``."""
    from .grad import sdf_grad
    capi.require_device(latents)
    if int(resolution) < 2:
        raise ValueError("resolution must be >= 2")
    if latents.dim() == 1:
        latents = latents[None]
    xyz = ops.grid_coords(int(resolution), bbox=bbox, device=latents.device)
    _, g = sdf_grad(decoder, latents, xyz, dtype=dtype)
    return g.norm(dim=-1).amax(dim=1)


# ------------------------------------------------------------------------------------ PNG
_PNG_SIG = b"\x89PNG\r\n\x1a\n"


def _chunk(kind: bytes, data: bytes) -> bytes:
    return (struct.pack(">I", len(data)) + kind + data +
            struct.pack(">I", zlib.crc32(kind + data) & 0xffffffff))


def write_png(path: str, image) -> None:
    """An 8-bit PNG of ``image``: uint8 ``[H, W]`` (grey) or ``[H, W, 3]`` (RGB), a tensor or
    an array.  Non-interlaced, filter 0 on every row; ``zlib`` and ``struct`` only."""
    a = image.detach().cpu().numpy() if isinstance(image, torch.Tensor) else np.asarray(image)
    if a.dtype != np.uint8 or a.ndim not in (2, 3) or (a.ndim == 3 and a.shape[2] != 3) \
            or a.shape[0] == 0 or a.shape[1] == 0:
        raise ValueError("write_png: image must be uint8 [H, W] or [H, W, 3], not empty")
    H, W = a.shape[:2]
    rows = np.ascontiguousarray(a).reshape(H, -1)
    raw = np.concatenate([np.zeros((H, 1), np.uint8), rows], axis=1).tobytes()
    ihdr = struct.pack(">IIBBBBB", W, H, 8, 0 if a.ndim == 2 else 2, 0, 0, 0)
    with open(path, "wb") as fh:
        fh.write(_PNG_SIG + _chunk(b"IHDR", ihdr) + _chunk(b"IDAT", zlib.compress(raw, 6)) +
                 _chunk(b"IEND", b""))


def read_png(path: str) -> np.ndarray:
    """The uint8 array ``[H, W]`` or ``[H, W, 3]`` of an 8-bit grey or RGB, non-interlaced
    PNG (all five row filters); anything else is a ``ValueError`` that names the file."""
    with open(path, "rb") as fh:
        data = fh.read()
    if data[:8] != _PNG_SIG:
        raise ValueError(f"{path}: not a PNG file")
    pos, idat, head = 8, [], None
    while pos + 8 <= len(data):
        n, kind = struct.unpack(">I4s", data[pos:pos + 8])
        body = data[pos + 8:pos + 8 + n]
        if len(body) != n or pos + 12 + n > len(data):
            raise ValueError(f"{path}: chunk {kind!r} is cut short")
        if struct.unpack(">I", data[pos + 8 + n:pos + 12 + n])[0] != \
                zlib.crc32(kind + body) & 0xffffffff:
            raise ValueError(f"{path}: chunk {kind!r} fails its CRC")
        if kind == b"IHDR":
            head = struct.unpack(">IIBBBBB", body)
        elif kind == b"IDAT":
            idat.append(body)
        elif kind == b"IEND":
            break
        pos += 12 + n
    if head is None or not idat:
        raise ValueError(f"{path}: no IHDR or no IDAT chunk")
    W, H, depth, ctype, comp, filt, lace = head
    if depth != 8 or ctype not in (0, 2) or comp or filt or lace or W == 0 or H == 0:
        raise ValueError(f"{path}: only 8-bit grey or RGB, non-interlaced PNGs are read")
    bpp = 1 if ctype == 0 else 3
    stride = W * bpp
    try:
        raw = zlib.decompress(b"".join(idat))
    except zlib.error as e:
        raise ValueError(f"{path}: {e}") from None
    if len(raw) != H * (stride + 1):
        raise ValueError(f"{path}: {len(raw)} bytes of image data, expected {H * (stride + 1)}")
    out = np.zeros((H, stride), np.uint8)
    prev = bytearray(stride)
    for r in range(H):
        f = raw[r * (stride + 1)]
        cur = bytearray(raw[r * (stride + 1) + 1:(r + 1) * (stride + 1)])
        if f == 1:
            for i in range(bpp, stride):
                cur[i] = (cur[i] + cur[i - bpp]) & 255
        elif f == 2:
            for i in range(stride):
                cur[i] = (cur[i] + prev[i]) & 255
        elif f == 3:
            for i in range(stride):
                left = cur[i - bpp] if i >= bpp else 0
                cur[i] = (cur[i] + ((left + prev[i]) >> 1)) & 255
        elif f == 4:
            for i in range(stride):
                a = cur[i - bpp] if i >= bpp else 0
                b = prev[i]
                c = prev[i - bpp] if i >= bpp else 0
                pa, pb, pc = abs(b - c), abs(a - c), abs(a + b - 2 * c)
                pred = a if pa <= pb and pa <= pc else (b if pb <= pc else c)
                cur[i] = (cur[i] + pred) & 255
        elif f != 0:
            raise ValueError(f"{path}: row {r} has filter type {f}")
        out[r] = np.frombuffer(bytes(cur), np.uint8)
        prev = cur
    return out.reshape(H, W) if ctype == 0 else out.reshape(H, W, 3)
