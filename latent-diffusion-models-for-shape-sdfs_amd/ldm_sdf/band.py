"""Narrow-band decode: mesh a shape without decoding the dense volume.

The dense grid is cut into 8^3 bricks.  The decoder is evaluated on the bricks' corner lattice
(a subset of the fine grid), a brick is *active* when its corners say the level set can pass
through it, only active bricks are decoded (the decoder kernel's brick mode), and every other
brick is filled with its corner-0 value.  Every voxel of an active brick equals ``decode``'s
value bit for bit; marching cubes on the result gives the dense volume's mesh whenever the band
covers the surface.

    brick    voxels [8b, min(8b + 8, N)) per axis; nb = ceil(N / 8); id = (bz nb + by) nb + bx;
             global id = shape nb^3 + id
    lattice  per axis the nb + 1 fine-grid indices min(8b, N - 1)
    active   min over the 8 corners of |v - level| <= band, or the corners not all on one side
             of level (v > level against v <= level), or a corner not finite
    band     default lipschitz * 4 sqrt(3) * voxel_size: half a brick's diagonal, so for a
             ``lipschitz``-Lipschitz field every brick the surface touches is active
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import List, Optional, Tuple

import numpy as np
import torch

from . import _capi as capi
from . import ops
from .api import resolve_decode_dtype
from .mesh import marching_cubes, vertex_normals
from .models import SDFDecoder

BRICK = 8


def n_bricks(N: int) -> int:
    """Bricks per axis of an ``N^3`` grid."""
    return (int(N) + BRICK - 1) // BRICK


def lattice_indices(N: int) -> np.ndarray:
    """The ``nb + 1`` fine-grid indices of the brick lattice along one axis."""
    return np.minimum(BRICK * np.arange(n_bricks(N) + 1, dtype=np.int64), int(N) - 1)


@dataclass
class BandInfo:
    """What ``decode_band`` decided, as device tensors (reading them is the caller's sync)."""
    coarse: torch.Tensor     # [B, nb+1, nb+1, nb+1] lattice values (= the dense values there)
    active: torch.Tensor     # bool [B, nb, nb, nb]
    bricks: torch.Tensor     # int32 [B*nb^3]: the first ``count`` entries, ascending global ids
    count: torch.Tensor      # int32 [1]
    band: float


def decode_band(decoder: SDFDecoder, latents: torch.Tensor, resolution: int, *,
                bbox: Tuple[float, float] = (-1.0, 1.0), dtype: str = "auto", level: float = 0.0,
                band: Optional[float] = None, lipschitz: float = 1.0,
                out: Optional[torch.Tensor] = None, return_info: bool = False):
    """``decode``'s ``[B, N, N, N]`` volume with only the bricks near ``level`` decoded.

    Every voxel of an active brick holds ``decode``'s value bit for bit; every voxel of an
    inactive brick holds the brick's corner-0 value (the field at the brick's first voxel), so
    the volume carries the sign of the field everywhere but not its values away from the
    surface.  ``band`` is the half-width in field units (default ``lipschitz * 4 sqrt(3) *
    voxel_size``): for a field that changes faster than ``lipschitz`` per unit length a brick
    the surface cuts without reaching a corner's band can be missed -- it is the caller's knob;
    ``band=float("inf")`` decodes every brick.  ``dtype`` resolves as in ``decode``.  Nothing is
    read back to the host (with an explicit ``dtype``).  With ``return_info`` the result is
    ``(vol, BandInfo)``.

    There is no ``group`` argument: sharding the brick list over ranks is out of scope.
    """
    N = int(resolution)
    if N < 2:
        raise ValueError("resolution must be >= 2")
    capi.require_device(latents)
    if latents.dim() == 1:
        latents = latents[None]
    if latents.shape[1] != decoder.latent_dim:
        raise ValueError(f"latents must be [B, {decoder.latent_dim}]")
    vs = ops.voxel_size(N, bbox)
    if band is None:
        band = float(lipschitz) * 4.0 * math.sqrt(3.0) * vs
    band = float(band)
    if not band >= 0.0:
        raise ValueError("band must be >= 0")
    dtype = resolve_decode_dtype(dtype, latents)
    dev = latents.device
    desc = decoder.device_pack(dtype, dev)["desc"]
    beta = ops.decoder_fold(desc, latents.float().contiguous())
    B, nb = latents.shape[0], n_bricks(N)
    vol = out if out is not None else torch.empty(B, N, N, N, device=dev)
    if vol.shape != (B, N, N, N) or vol.dtype != torch.float32 or not vol.is_contiguous():
        raise capi.LdmError("decode_band: out must be a contiguous float32 [B, N, N, N]")
    xyz = ops.band_lattice_coords(N, bbox, device=dev)[None].expand(B, -1, -1).contiguous()
    coarse = ops.decoder_points_fwd(desc, beta, xyz)
    active, bricks, count = ops.band_classify(coarse, N, level, band)
    ops.band_fill(coarse, active, N, vol)
    ops.decoder_bricks_fwd(desc, beta, N, bricks, count, vol, bbox)
    if not return_info:
        return vol
    return vol, BandInfo(coarse.view(B, nb + 1, nb + 1, nb + 1),
                         active.view(B, nb, nb, nb).bool(), bricks, count, band)


def extract_mesh(decoder: SDFDecoder, latents: torch.Tensor, resolution: int, *,
                 normals: bool = False, **kw) -> List[Tuple[torch.Tensor, ...]]:
    """``decode_band`` then ``marching_cubes`` per shape at the same ``level`` and ``bbox``:
    a list of ``(verts, faces)``, or with ``normals`` of ``(verts, faces, normals)`` -- the
    field's unit gradient at every vertex (``mesh.vertex_normals``, fp16).  The other keyword
    arguments are ``decode_band``'s."""
    kw.pop("return_info", None)
    level, bbox = kw.get("level", 0.0), kw.get("bbox", (-1.0, 1.0))
    vol = decode_band(decoder, latents, resolution, **kw)
    meshes = [marching_cubes(vol[b], level, bbox) for b in range(vol.shape[0])]
    if not normals:
        return meshes
    lat = latents if latents.dim() > 1 else latents[None]
    return [(v, f, vertex_normals(decoder, lat[b], v)) for b, (v, f) in enumerate(meshes)]
