"""Evaluation of reconstructed and generated shapes: the last stage of the path.

``nearest_points`` and ``chamfer_matrix`` run the HIP kernels of ``csrc/chamfer.hip``: every
point pair, squared distances, ``D(a -> b) = mean_i min_j |a_i - b_j|^2`` and ``CD(a, b) =
D(a -> b) + D(b -> a)`` as in DeepSDF's evaluation and PointFlow.  ``generation_metrics`` turns
Chamfer matrices into MMD, COV and 1-NNA (Achlioptas et al.; Yang et al., PointFlow); it is pure
torch on any device.  ``shape_clouds`` draws the clouds from latents through ``extract_mesh`` and
``sample_surface``.

An entry of a matrix is a pure function of its two clouds: bitwise the same alone or in any
batch, at any position, from run to run.
"""
from __future__ import annotations

from typing import Dict, Optional

import torch

from . import _capi as capi

__all__ = ["nearest_points", "chamfer_matrix", "chamfer_distance", "generation_metrics",
           "evaluate_generation", "shape_clouds", "tile_a", "chunk_b", "split_below",
           "spread_below"]


def tile_a() -> int:
    """Points of the first cloud per workgroup tile (a compile-time constant)."""
    return int(capi.load().ldm_chamfer_tile_a())


def chunk_b() -> int:
    """Points of the second cloud per split unit (a compile-time constant)."""
    return int(capi.load().ldm_chamfer_chunk_b())


def split_below() -> int:
    """``nearest_points`` with fewer query points than this (and more than ``chunk_b()`` cloud
    points) splits the cloud over workgroups and takes the minimum of the partials."""
    return int(capi.load().ldm_chamfer_split_below())


def spread_below() -> int:
    """A matrix with fewer entries than this (and more than ``tile_a()`` points per first
    cloud) spreads each entry over workgroups: the same sums, more workgroups."""
    return int(capi.load().ldm_chamfer_spread_below())


def _check_cloud(t: torch.Tensor, dims: int, what: str) -> None:
    if not isinstance(t, torch.Tensor) or t.dim() != dims or t.shape[-1] != 3 \
            or t.dtype != torch.float32:
        shape = "[n, 3]" if dims == 2 else "[S, n, 3]"
        raise capi.LdmError(f"{what} must be a float32 {shape} tensor")


def _check_finite(t: torch.Tensor, what: str) -> None:
    if t.numel() and not bool(torch.isfinite(t).all()):
        raise capi.LdmError(f"{what} has a non-finite coordinate (the kernels' minimum drops "
                            "a NaN instead of propagating it)")


def nearest_points(query: torch.Tensor, cloud: torch.Tensor, *, return_index: bool = False,
                   _validated: bool = False):
    """Squared distance ``[P]`` from each of ``query [P, 3]`` to its nearest point of ``cloud
    [Q, 3]`` (fp32, device tensors); with ``return_index`` also its index ``[P]`` int32, the
    smaller index on a tie.  A non-finite coordinate raises ``LdmError``."""
    _check_cloud(query, 2, "nearest_points: query")
    _check_cloud(cloud, 2, "nearest_points: cloud")
    capi.require_device(query, cloud)
    if query.device != cloud.device:
        raise capi.LdmError("nearest_points: query and cloud must share a device")
    P, Q = query.shape[0], cloud.shape[0]
    if P > 0 and Q == 0:
        raise capi.LdmError("nearest_points: the cloud is empty")
    if not _validated:
        _check_finite(query, "nearest_points: query")
        _check_finite(cloud, "nearest_points: cloud")
    dev = query.device
    query, cloud = query.contiguous(), cloud.contiguous()
    d2 = torch.empty(P, device=dev, dtype=torch.float32)
    idx = torch.empty(P, device=dev, dtype=torch.int32) if return_index else None
    if P > 0:
        lib = capi.load()
        ws = torch.empty(lib.ldm_nearest_points_ws_bytes(P, Q), device=dev, dtype=torch.uint8)
        with torch.cuda.device(dev):
            capi.check(lib.ldm_nearest_points(capi.ptr(query), P, capi.ptr(cloud), Q,
                                              capi.ptr(d2), capi.ptr(idx), capi.ptr(ws),
                                              ws.numel(), capi.stream_handle(dev)),
                       "ldm_nearest_points")
    return (d2, idx) if return_index else d2


def _directed(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """``out[s, r] = D(a_s -> b_r)``; contiguous, checked inputs."""
    S, n, R, m = a.shape[0], a.shape[1], b.shape[0], b.shape[1]
    out = torch.empty(S, R, device=a.device, dtype=torch.float32)
    if S > 0 and R > 0:
        lib = capi.load()
        ws = torch.empty(lib.ldm_chamfer_ws_bytes(S, n, R, m), device=a.device, dtype=torch.uint8)
        with torch.cuda.device(a.device):
            capi.check(lib.ldm_chamfer_matrix(capi.ptr(a), S, n, capi.ptr(b), R, m, capi.ptr(out),
                                              capi.ptr(ws), ws.numel(),
                                              capi.stream_handle(a.device)), "ldm_chamfer_matrix")
    return out


def chamfer_matrix(a: torch.Tensor, b: Optional[torch.Tensor] = None, *, directed: bool = False,
                   _validated: bool = False):
    """Chamfer distances ``[S, R]`` between the clouds ``a [S, n, 3]`` and ``b [R, m, 3]``
    (fp32, device tensors): ``CD(a_s, b_r) = D_ab[s, r] + D_ba[r, s]``.  ``b=None`` is the
    within-set matrix ``D + D^T`` from one directed pass (symmetric, zero diagonal).  With
    ``directed`` the pair ``(D_ab, D_ba^T)`` is returned instead of its sum.  A non-finite
    coordinate raises ``LdmError``."""
    _check_cloud(a, 3, "chamfer_matrix: a")
    if b is not None:
        _check_cloud(b, 3, "chamfer_matrix: b")
    capi.require_device(a, b)
    if b is not None:
        if a.device != b.device:
            raise capi.LdmError("chamfer_matrix: a and b must share a device")
    other = a if b is None else b
    if a.shape[0] > 0 and other.shape[0] > 0 and (a.shape[1] == 0 or other.shape[1] == 0):
        raise capi.LdmError("chamfer_matrix: empty clouds have no distance")
    if not _validated:
        _check_finite(a, "chamfer_matrix: a")
        if b is not None:
            _check_finite(b, "chamfer_matrix: b")
    a = a.contiguous()
    if b is None:
        d_ab = _directed(a, a)
        d_ba_t = d_ab.t()
    else:
        b = b.contiguous()
        d_ab = _directed(a, b)
        d_ba_t = _directed(b, a).t()
    return (d_ab, d_ba_t) if directed else d_ab + d_ba_t


def chamfer_distance(a: torch.Tensor, b: torch.Tensor, *, _validated: bool = False
                     ) -> torch.Tensor:
    """``CD(a, b)`` of two clouds ``[n, 3]`` and ``[m, 3]`` as a 0-d tensor: the ``S = R = 1``
    case of ``chamfer_matrix`` (DeepSDF's reconstruction metric at 30 000 points each)."""
    _check_cloud(a, 2, "chamfer_distance: a")
    _check_cloud(b, 2, "chamfer_distance: b")
    capi.require_device(a, b)
    if a.shape[0] == 0 or b.shape[0] == 0:
        raise capi.LdmError("chamfer_distance: an empty cloud has no distance")
    return chamfer_matrix(a[None], b[None], _validated=_validated)[0, 0]


def _first_argmin(d: torch.Tensor) -> torch.Tensor:
    """Row-wise argmin, the smallest index on a tie (``torch.argmin`` promises no order)."""
    n = d.shape[1]
    cols = torch.arange(n, device=d.device).expand_as(d)
    hit = d == d.amin(dim=1, keepdim=True)
    return torch.where(hit, cols, torch.full_like(cols, n)).amin(dim=1)


def generation_metrics(cd_gr: torch.Tensor, cd_gg: torch.Tensor, cd_rr: torch.Tensor
                       ) -> Dict[str, float]:
    """MMD, COV and 1-NNA from the Chamfer matrices between a generated set G (``S`` shapes)
    and a reference set R: ``cd_gr [S, R]``, ``cd_gg [S, S]``, ``cd_rr [R, R]``.  Pure torch,
    any device.

    * ``mmd``: mean over the reference set of ``min_s cd_gr[s, r]``
    * ``cov``: ``|{argmin_r cd_gr[s, r] : s}| / R``
    * ``1nna``: in the merged set G then R, each element's nearest neighbour other than itself
      (the smallest merged index on a tie); the fraction whose neighbour is in its own set.
      0.5 is the best a generator can do, 1 the worst.
    """
    for t, name in ((cd_gr, "cd_gr"), (cd_gg, "cd_gg"), (cd_rr, "cd_rr")):
        if not isinstance(t, torch.Tensor) or t.dim() != 2 or not t.is_floating_point():
            raise ValueError(f"generation_metrics: {name} must be a floating-point matrix")
    S, R = cd_gr.shape
    if S == 0 or R == 0 or cd_gg.shape != (S, S) or cd_rr.shape != (R, R):
        raise ValueError("generation_metrics: expected non-empty cd_gr [S, R], cd_gg [S, S], "
                         f"cd_rr [R, R]; got {tuple(cd_gr.shape)}, {tuple(cd_gg.shape)}, "
                         f"{tuple(cd_rr.shape)}")
    cd_gr, cd_gg, cd_rr = cd_gr.double(), cd_gg.double(), cd_rr.double()
    mmd = float(cd_gr.amin(dim=0).mean())
    cov = int(torch.unique(_first_argmin(cd_gr)).numel()) / R
    full = torch.cat([torch.cat([cd_gg, cd_gr], dim=1), torch.cat([cd_gr.t(), cd_rr], dim=1)])
    full.fill_diagonal_(float("inf"))
    nn = _first_argmin(full)
    own = torch.arange(S + R, device=nn.device) < S
    nna = float(((nn < S) == own).double().mean())
    return {"mmd": mmd, "cov": cov, "1nna": nna}


def evaluate_generation(gen_clouds: torch.Tensor, ref_clouds: torch.Tensor, *,
                        _validated: bool = False) -> Dict[str, object]:
    """MMD-CD, COV-CD and 1-NNA-CD of ``gen_clouds [S, n, 3]`` against ``ref_clouds [R, m, 3]``:
    four directed passes (G -> R, R -> G, G -> G, R -> R), then ``generation_metrics``.  The
    result also carries the three matrices under ``cd_gr``, ``cd_gg`` and ``cd_rr``."""
    cd_gr = chamfer_matrix(gen_clouds, ref_clouds, _validated=_validated)
    cd_gg = chamfer_matrix(gen_clouds, _validated=True)
    cd_rr = chamfer_matrix(ref_clouds, _validated=True)
    out: Dict[str, object] = dict(generation_metrics(cd_gr, cd_gg, cd_rr))
    out.update(cd_gr=cd_gr, cd_gg=cd_gg, cd_rr=cd_rr)
    return out


def shape_clouds(decoder, latents: torch.Tensor, resolution: int, n_points: int, *,
                 generator: Optional[torch.Generator] = None, batch: int = 8,
                 skip_empty: bool = False, **extract_mesh_kw):
    """``[B, n_points, 3]`` surface points of the shapes ``latents [B, D]`` decode to:
    ``extract_mesh`` at ``resolution`` (``batch`` shapes per call; the other keyword arguments
    are its own), then ``sample_surface`` per shape.  A shape whose mesh has no area raises
    ``LdmError`` naming the shape indices; with ``skip_empty`` the clouds of the rest are
    returned together with the kept indices (int64, on the latents' device)."""
    from .band import extract_mesh
    from .meshsdf import sample_surface
    lat = latents if latents.dim() > 1 else latents[None]
    extract_mesh_kw.pop("normals", None)
    clouds, kept, empty = [], [], []
    for b0 in range(0, lat.shape[0], max(int(batch), 1)):
        meshes = extract_mesh(decoder, lat[b0:b0 + max(int(batch), 1)], resolution,
                              **extract_mesh_kw)
        for k, (verts, faces) in enumerate(meshes):
            try:
                if faces.shape[0] == 0:
                    raise ValueError("no faces")
                xyz, _ = sample_surface(verts, faces, int(n_points), generator)
            except ValueError:
                empty.append(b0 + k)
                continue
            clouds.append(xyz)
            kept.append(b0 + k)
    if empty and not skip_empty:
        raise capi.LdmError(f"shape_clouds: the meshes of shapes {empty} have no area "
                            f"(no zero crossing at resolution {resolution}?)")
    out = (torch.stack(clouds) if clouds
           else torch.empty(0, int(n_points), 3, device=lat.device, dtype=torch.float32))
    if skip_empty:
        return out, torch.tensor(kept, device=lat.device, dtype=torch.int64)
    return out
