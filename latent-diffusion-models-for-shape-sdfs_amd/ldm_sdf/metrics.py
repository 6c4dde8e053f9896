"""Evaluation of reconstructed and generated shapes: the last stage of the path.

``nearest_points`` and ``chamfer_matrix`` run the HIP kernels of ``csrc/chamfer.hip``: every
point pair, squared distances, ``D(a -> b) = mean_i min_j |a_i - b_j|^2`` and ``CD(a, b) =
D(a -> b) + D(b -> a)`` as in DeepSDF's evaluation and PointFlow.  ``generation_metrics`` turns
Chamfer matrices into MMD, COV and 1-NNA (Achlioptas et al.; Yang et al., PointFlow); it is pure
torch on any device.  ``shape_clouds`` draws the clouds from latents through ``extract_mesh`` and
``sample_surface``.

``emd_matrix`` and ``emd_distance`` run the auction kernel of ``csrc/emd.hip``:
the earth mover's distance ``(1/n) min_pi sum_i |a_i - b_pi(i)|`` of clouds of equal size, from a
real assignment whose cost is within ``eps + emd_slack(extent)`` of the optimum.

An entry of a matrix is a pure function of its two clouds: bitwise the same alone or in any
batch, at any position, from run to run.
"""
from __future__ import annotations

from typing import Dict, Optional

import torch

from . import _capi as capi

__all__ = ["nearest_points", "chamfer_matrix", "chamfer_distance", "generation_metrics",
           "evaluate_generation", "shape_clouds", "tile_a", "chunk_b", "split_below",
           "spread_below", "emd_matrix", "emd_distance", "emd_max_points", "emd_min_eps",
           "emd_slack", "emd_default_max_rounds"]


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


def emd_max_points() -> int:
    """Most points per cloud ``emd_matrix`` takes (one workgroup keeps a pair in LDS)."""
    return int(capi.load().ldm_emd_max_points())


def emd_slack(extent: float) -> float:
    """What fp32 rounding adds to ``eps`` in the bound ``cost <= EMD + eps + slack`` for clouds
    whose common bounding box has the diagonal ``extent``."""
    return float(capi.load().ldm_emd_slack(float(extent)))


def emd_min_eps(extent: float) -> float:
    """The smallest ``eps`` accepted at that extent: ``8 emd_slack(extent)``."""
    return float(capi.load().ldm_emd_min_eps(float(extent)))


def emd_default_max_rounds(n: int) -> int:
    """The default cap on auction rounds per entry for clouds of ``n`` points."""
    return int(capi.load().ldm_emd_default_max_rounds(int(n)))


def _extent_bound(a: torch.Tensor, b: Optional[torch.Tensor]) -> float:
    """fp32 upper bound of the bounding-box diagonal of all the clouds together."""
    lo, hi = a.amin(dim=(0, 1)), a.amax(dim=(0, 1))
    if b is not None:
        lo, hi = torch.minimum(lo, b.amin(dim=(0, 1))), torch.maximum(hi, b.amax(dim=(0, 1)))
    diag = float(torch.linalg.vector_norm((hi - lo).double()))
    return float(torch.tensor(diag * (1 + 2.0 ** -20), dtype=torch.float64).float()
                 .nextafter(torch.tensor(float("inf"))))


def _emd(a: torch.Tensor, b: Optional[torch.Tensor], eps: float, max_rounds: Optional[int],
         want_assign: bool, what: str, validated: bool = False):
    """``(out [S, R], assign or None, rounds [S, R])``; raises for unconverged entries."""
    _check_cloud(a, 3, f"{what}: a")
    if b is not None:
        _check_cloud(b, 3, f"{what}: b")
    capi.require_device(a, b)
    other = a if b is None else b
    if a.device != other.device:
        raise capi.LdmError(f"{what}: a and b must share a device")
    S, R, n = a.shape[0], other.shape[0], a.shape[1]
    if other.shape[1] != n:
        raise capi.LdmError(f"{what}: clouds of {n} and {other.shape[1]} points: the earth "
                            "mover's distance here is between clouds of the same size")
    if max_rounds is not None and int(max_rounds) < 1:
        raise capi.LdmError(f"{what}: max_rounds must be at least 1 (None: the default)")
    dev = a.device
    out = torch.empty(S, R, device=dev, dtype=torch.float32)
    rounds = torch.zeros(S, R, device=dev, dtype=torch.int32)
    assign = torch.empty(S, R, n, device=dev, dtype=torch.int32) if want_assign else None
    if S == 0 or R == 0:
        return out, assign, rounds
    if n == 0:
        raise capi.LdmError(f"{what}: empty clouds have no distance")
    lib = capi.load()
    if n > lib.ldm_emd_max_points():
        raise capi.LdmError(f"{what}: {n} points per cloud is above emd_max_points() = "
                            f"{lib.ldm_emd_max_points()}")
    if not validated:
        _check_finite(a, f"{what}: a")
        if b is not None:
            _check_finite(b, f"{what}: b")
    extent = _extent_bound(a, b)
    if not (eps > 0 and eps >= lib.ldm_emd_min_eps(extent)):
        raise capi.LdmError(f"{what}: eps = {eps:g} is below emd_min_eps({extent:g}) = "
                            f"{lib.ldm_emd_min_eps(extent):g}, the floor under which fp32 "
                            "rounding is no longer small against eps")
    a = a.contiguous()
    bb = a if b is None else b.contiguous()
    unconv = torch.zeros(1, device=dev, dtype=torch.int32)
    ws = torch.empty(lib.ldm_emd_ws_bytes(S, R, n), device=dev, dtype=torch.uint8)
    with torch.cuda.device(dev):
        capi.check(lib.ldm_emd_matrix(capi.ptr(a), S, capi.ptr(bb), R, n, float(eps), extent,
                                      0 if max_rounds is None else int(max_rounds),
                                      1 if b is None else 0, capi.ptr(out), capi.ptr(assign),
                                      capi.ptr(rounds), capi.ptr(unconv), capi.ptr(ws),
                                      ws.numel(), capi.stream_handle(dev)), "ldm_emd_matrix")
    if int(unconv.item()):
        bad = torch.nonzero(torch.isnan(out)).tolist()
        cap = emd_default_max_rounds(n) if max_rounds is None else int(max_rounds)
        raise capi.LdmError(f"{what}: {len(bad)} entries did not converge within {cap} rounds "
                            f"(or left the price range): {[tuple(e) for e in bad[:16]]}"
                            + (" ..." if len(bad) > 16 else ""))
    return out, assign, rounds


def emd_matrix(a: torch.Tensor, b: Optional[torch.Tensor] = None, *, eps: float = 1e-4,
               max_rounds: Optional[int] = None, return_rounds: bool = False,
               _validated: bool = False):
    """Earth mover's distances ``[S, R]`` between the clouds ``a [S, n, 3]`` and ``b [R, n, 3]``
    (fp32, device tensors, the same ``n``): each entry is the cost of a real assignment, at most
    ``eps + emd_slack(extent)`` above the optimum.  ``b=None`` is the within-set matrix
    (symmetric, zero diagonal; only ``s < r`` is computed).  ``max_rounds`` caps the auction
    rounds per entry (default ``emd_default_max_rounds(n)``); an entry that hits it raises
    ``LdmError`` naming it.  With ``return_rounds`` also the rounds per entry ``[S, R]`` int32.
    A non-finite coordinate, ``n`` above ``emd_max_points()`` or an ``eps`` below
    ``emd_min_eps(extent)`` raises ``LdmError``."""
    out, _, rounds = _emd(a, b, eps, max_rounds, False, "emd_matrix", _validated)
    return (out, rounds) if return_rounds else out


def emd_distance(a: torch.Tensor, b: torch.Tensor, *, eps: float = 1e-4,
                 return_assignment: bool = False):
    """``EMD(a, b)`` of two clouds ``[n, 3]`` as a 0-d tensor; with ``return_assignment`` also
    ``pi [n]`` int32, the point of ``b`` each point of ``a`` is matched to.  One workgroup does
    the pair."""
    _check_cloud(a, 2, "emd_distance: a")
    _check_cloud(b, 2, "emd_distance: b")
    capi.require_device(a, b)
    out, assign, _ = _emd(a[None], b[None], eps, None, return_assignment, "emd_distance")
    return (out[0, 0], assign[0, 0]) if return_assignment else out[0, 0]


def evaluate_generation(gen_clouds: torch.Tensor, ref_clouds: torch.Tensor, *,
                        metrics=("cd",), eps: float = 1e-4,
                        _validated: bool = False) -> Dict[str, object]:
    """MMD-CD, COV-CD and 1-NNA-CD of ``gen_clouds [S, n, 3]`` against ``ref_clouds [R, m, 3]``:
    four directed passes (G -> R, R -> G, G -> G, R -> R), then ``generation_metrics``.  The
    result also carries the three matrices under ``cd_gr``, ``cd_gg`` and ``cd_rr``.

    With ``"emd"`` in ``metrics`` (which needs ``n == m``) the result also has ``mmd_emd``,
    ``cov_emd`` and ``1nna_emd``, ``generation_metrics`` of the earth mover's matrices, and those
    matrices under ``emd_gr``, ``emd_gg`` and ``emd_rr``; ``eps`` is ``emd_matrix``'s."""
    metrics = tuple(metrics)
    if "cd" not in metrics or any(m not in ("cd", "emd") for m in metrics):
        raise capi.LdmError("evaluate_generation: metrics must be ('cd',) or ('cd', 'emd')")
    cd_gr = chamfer_matrix(gen_clouds, ref_clouds, _validated=_validated)
    cd_gg = chamfer_matrix(gen_clouds, _validated=True)
    cd_rr = chamfer_matrix(ref_clouds, _validated=True)
    out: Dict[str, object] = dict(generation_metrics(cd_gr, cd_gg, cd_rr))
    out.update(cd_gr=cd_gr, cd_gg=cd_gg, cd_rr=cd_rr)
    if "emd" in metrics:
        emd_gr = emd_matrix(gen_clouds, ref_clouds, eps=eps, _validated=True)
        emd_gg = emd_matrix(gen_clouds, eps=eps, _validated=True)
        emd_rr = emd_matrix(ref_clouds, eps=eps, _validated=True)
        out.update({k + "_emd": v
                    for k, v in generation_metrics(emd_gr, emd_gg, emd_rr).items()})
        out.update(emd_gr=emd_gr, emd_gg=emd_gg, emd_rr=emd_rr)
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
