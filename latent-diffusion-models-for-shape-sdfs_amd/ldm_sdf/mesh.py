"""C18: marching cubes on decoded SDF volumes + PLY export.

``marching_cubes`` runs the HIP passes of ``csrc/mc.hip`` (``ldm_mc_count`` ->
read the two counts -> ``ldm_mc_emit``) on the volume where decode left it; conventions and
the generated case table are DESIGN.md §10.  ``write_ply`` writes the binary PLY DeepSDF's
``convert_sdf_samples_to_ply`` writes (host I/O); ``read_ply`` and ``read_obj`` read triangle
meshes back for ``meshsdf`` (pure numpy parsers: nothing in a file is executed).
"""
from __future__ import annotations

import ctypes as C
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _capi as capi
from . import dist as ldist
from .ops import voxel_size


def mc_table() -> Tuple[np.ndarray, np.ndarray]:
    """The library's compile-time generated case table: (tri [256, 16] int8, ntri [256] u8)."""
    tri = np.zeros((256, 16), np.int8)
    ntri = np.zeros(256, np.uint8)
    capi.check(capi.load().ldm_mc_table(tri.ctypes.data, ntri.ctypes.data), "ldm_mc_table")
    return tri, ntri


def marching_cubes(volume: torch.Tensor, level: float = 0.0, bbox=(-1.0, 1.0),
                   ws: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """Iso-surface of ``volume [N, N, N]`` (z slowest, as ``decode`` returns it) at ``level``.

    Returns device tensors ``verts [V, 3]`` (x, y, z on the A1 grid over ``bbox``) and
    ``faces [F, 3]`` int32, outward (toward larger values) winding.  One host sync (the two
    counts) sits between the passes.
    """
    capi.require_device(volume)
    if volume.dim() != 3 or len(set(volume.shape)) != 1 or volume.dtype != torch.float32:
        raise capi.LdmError("marching_cubes: volume must be a float32 [N, N, N] tensor")
    volume = volume.contiguous()
    N = volume.shape[0]
    dev = volume.device
    lib = capi.load()
    need = lib.ldm_mc_workspace_bytes(N)
    if ws is None or ws.numel() < need:
        ws = torch.empty(need, device=dev, dtype=torch.uint8)
    counts = torch.empty(2, device=dev, dtype=torch.int32)
    s = capi.stream_handle(dev)
    capi.check(lib.ldm_mc_count(volume.data_ptr(), N, float(level), ws.data_ptr(), ws.numel(),
                                counts.data_ptr(), s), "ldm_mc_count")
    nv, nf = (int(x) for x in counts.cpu())
    verts = torch.empty(max(nv, 1), 3, device=dev, dtype=torch.float32)
    faces = torch.empty(max(nf, 1), 3, device=dev, dtype=torch.int32)
    capi.check(lib.ldm_mc_emit(volume.data_ptr(), N, float(level), voxel_size(N, bbox),
                               float(bbox[0]), ws.data_ptr(), ws.numel(), verts.data_ptr(),
                               faces.data_ptr(), s), "ldm_mc_emit")
    return verts[:nv], faces[:nf]


def marching_cubes_batch(volumes: torch.Tensor, level: float = 0.0, bbox=(-1.0, 1.0),
                         group=None) -> List[Tuple[int, torch.Tensor, torch.Tensor]]:
    """Mesh a batch ``[B, N, N, N]``; with a process group each rank meshes the shapes
    ``b = rank, rank + W, ...`` of the (all-gathered) batch.  Returns (b, verts, faces)."""
    world, rank = ldist.world_and_rank(group)
    ws = torch.empty(capi.load().ldm_mc_workspace_bytes(volumes.shape[-1]),
                     device=volumes.device, dtype=torch.uint8)
    return [(b, *marching_cubes(volumes[b], level, bbox, ws=ws))
            for b in range(rank, volumes.shape[0], world)]


def vertex_normals(decoder, latent: torch.Tensor, verts: torch.Tensor, *,
                   dtype: str = "fp16") -> torch.Tensor:
    """Unit normals ``[V, 3]`` of the decoder's level set at ``verts [V, 3]``: the field's own
    gradient ``grad f / |grad f|`` (``sdf_grad``), the zero vector where the gradient vanishes.
    They point toward larger values, the side ``marching_cubes``' winding faces.  ``latent`` is
    one shape's code ``[L]`` (or ``[1, L]``)."""
    from .grad import sdf_grad
    capi.require_device(latent, verts)
    if verts.dim() != 2 or verts.shape[1] != 3:
        raise ValueError("vertex_normals: verts must be [V, 3]")
    if verts.shape[0] == 0:
        return torch.zeros(0, 3, device=verts.device, dtype=torch.float32)
    _, g = sdf_grad(decoder, latent.reshape(1, -1), verts[None], dtype=dtype)
    g = g[0]
    n = g.norm(dim=1, keepdim=True)
    return torch.where(n > 0, g / n.clamp_min(torch.finfo(torch.float32).tiny),
                       torch.zeros_like(g))


def write_ply(path: str, verts, faces, offset: Optional[Sequence[float]] = None,
              scale: Optional[float] = None, normals=None) -> None:
    """Binary little-endian PLY (vertex float x, y, z; face ``list uchar int``), as DeepSDF's
    ``convert_sdf_samples_to_ply`` writes it; ``offset``/``scale`` undo a normalisation
    (``p / scale - offset``) when given.  ``normals [V, 3]`` adds the vertex properties
    ``nx ny nz``; without it the file is what it always was."""
    v = verts.detach().cpu().numpy() if isinstance(verts, torch.Tensor) else np.asarray(verts)
    f = faces.detach().cpu().numpy() if isinstance(faces, torch.Tensor) else np.asarray(faces)
    v = v.astype("<f4")
    if scale is not None:
        v = v / np.float32(scale)
    if offset is not None:
        v = v - np.asarray(offset, np.float32)
    props = "property float x\nproperty float y\nproperty float z\n"
    if normals is not None:
        nrm = (normals.detach().cpu().numpy() if isinstance(normals, torch.Tensor)
               else np.asarray(normals)).astype("<f4")
        if nrm.shape != v.shape:
            raise ValueError(f"write_ply: normals {nrm.shape} do not match verts {v.shape}")
        v = np.concatenate([v.reshape(-1, 3), nrm.reshape(-1, 3)], axis=1)
        props += "property float nx\nproperty float ny\nproperty float nz\n"
    head = ("ply\nformat binary_little_endian 1.0\n"
            f"element vertex {len(v)}\n{props}"
            f"element face {len(f)}\nproperty list uchar int vertex_indices\nend_header\n")
    rec = np.zeros(len(f), dtype=[("n", "u1"), ("v", "<i4", (3,))])
    rec["n"] = 3
    rec["v"] = f
    with open(path, "wb") as fh:
        fh.write(head.encode("ascii"))
        fh.write(np.ascontiguousarray(v, "<f4").tobytes())
        fh.write(rec.tobytes())


_PLY_TYPES = {"char": "i1", "int8": "i1", "uchar": "u1", "uint8": "u1", "short": "i2",
              "int16": "i2", "ushort": "u2", "uint16": "u2", "int": "i4", "int32": "i4",
              "uint": "u4", "uint32": "u4", "float": "f4", "float32": "f4", "double": "f8",
              "float64": "f8"}


def read_ply(path: str) -> Tuple[np.ndarray, np.ndarray]:
    """``(verts [V, 3] float32, faces [F, 3] int32)`` of a triangle PLY: the binary
    little-endian file ``write_ply`` writes (with or without normals; further scalar vertex
    properties are skipped) or its ASCII form.  Every face must be a triangle."""
    with open(path, "rb") as fh:
        raw = fh.read()
    end = raw.find(b"end_header")
    if not raw.startswith(b"ply") or end < 0:
        raise ValueError(f"{path}: not a PLY file")
    nl = raw.find(b"\n", end)
    if nl < 0:
        raise ValueError(f"{path}: truncated PLY header")
    body = raw[nl + 1:]
    fmt, elems = None, []          # elems: [name, count, [(kind, name, types...)]]
    for line in raw[:end].decode("ascii", "replace").splitlines():
        t = line.split()
        if not t or t[0] in ("ply", "comment", "obj_info"):
            continue
        if t[0] == "format" and len(t) >= 2:
            fmt = t[1]
        elif t[0] == "element" and len(t) == 3 and t[2].isdigit():
            elems.append([t[1], int(t[2]), []])
        elif t[0] == "property" and elems:
            types = t[2:4] if t[1] == "list" else t[1:2]
            if len(t) != (5 if t[1] == "list" else 3) or any(k not in _PLY_TYPES for k in types):
                raise ValueError(f"{path}: unsupported PLY property {line!r}")
            if t[1] == "list":
                elems[-1][2].append(("list", t[4], _PLY_TYPES[t[2]], _PLY_TYPES[t[3]]))
            else:
                elems[-1][2].append(("scalar", t[2], _PLY_TYPES[t[1]]))
        else:
            raise ValueError(f"{path}: unexpected PLY header line {line!r}")
    if fmt not in ("binary_little_endian", "ascii"):
        raise ValueError(f"{path}: PLY format {fmt!r} is not supported")
    verts = faces = None
    tokens = body.split() if fmt == "ascii" else None
    pos = 0
    for name, count, props in elems:
        lists = [p for p in props if p[0] == "list"]
        if lists and (len(props) != 1 or name != "face"):
            raise ValueError(f"{path}: list properties are read on a face element alone")
        if name == "face":
            if not lists:
                raise ValueError(f"{path}: the face element has no index list")
            _, _, ct, it = lists[0]
            if fmt == "ascii":
                # face by face, each by its own count token: a polygon is refused where it
                # stands, never read as the start of the next face
                idx = np.empty((count, 3), np.int64)
                for k in range(count):
                    try:
                        n = int(tokens[pos])
                        idx[k] = [int(x) for x in tokens[pos + 1:pos + 4]] if n == 3 else 0
                    except (IndexError, ValueError, OverflowError):
                        raise ValueError(f"{path}: face {k} of {count} is cut short or not "
                                         f"integers") from None
                    if n != 3:
                        raise ValueError(f"{path}: only triangle faces are supported")
                    pos += 4
            else:
                # fixed records of three indices: every face before the first polygon is a
                # triangle, so that polygon's count is read where it stands and refused
                dt = np.dtype([("n", "<" + ct), ("v", "<" + it, (3,))])
                if pos + dt.itemsize * count > len(body):
                    raise ValueError(f"{path}: the face element is cut short")
                rec = np.frombuffer(body, dt, count, pos)
                pos += dt.itemsize * count
                if count and not (rec["n"] == 3).all():
                    raise ValueError(f"{path}: only triangle faces are supported")
                idx = rec["v"]
            faces = np.ascontiguousarray(idx).astype(np.int64)
            continue
        names = [p[1] for p in props]
        if fmt == "ascii":
            if pos + len(props) * count > len(tokens):
                raise ValueError(f"{path}: the {name} element is cut short")
            try:
                a = np.array(tokens[pos:pos + len(props) * count], dtype=np.float64)
            except ValueError:
                raise ValueError(f"{path}: the {name} element holds a non-number") from None
            a = a.reshape(count, len(props))
            pos += len(props) * count
            cols = {nm: a[:, i] for i, nm in enumerate(names)}
        else:
            dt = np.dtype([(nm, "<" + p[2]) for nm, p in zip(names, props)])
            if pos + dt.itemsize * count > len(body):
                raise ValueError(f"{path}: the {name} element is cut short")
            rec = np.frombuffer(body, dt, count, pos)
            pos += dt.itemsize * count
            cols = {nm: rec[nm] for nm in names}
        if name == "vertex":
            if not all(k in cols for k in "xyz"):
                raise ValueError(f"{path}: the vertex element needs x, y, z")
            verts = np.stack([cols[k] for k in "xyz"], axis=1).astype(np.float32)
    if verts is None or faces is None:
        raise ValueError(f"{path}: PLY without a vertex and a face element")
    if len(faces) and (faces.min() < 0 or faces.max() >= len(verts)):
        raise ValueError(f"{path}: face index outside the {len(verts)} vertices")
    return verts, faces.astype(np.int32)


def read_obj(path: str) -> Tuple[np.ndarray, np.ndarray]:
    """``(verts [V, 3] float32, faces [F, 3] int32)`` of a Wavefront OBJ: ``v`` and ``f``
    lines, ``f a/b/c`` forms (the vertex index is taken), negative (relative) indices, and
    polygons fan-triangulated from their first corner.  Everything else is skipped."""
    verts, faces = [], []
    with open(path, "r", errors="replace") as fh:
        for ln, line in enumerate(fh, 1):
            t = line.split()
            if not t:
                continue
            if t[0] == "v":
                if len(t) < 4:
                    raise ValueError(f"{path}:{ln}: a vertex needs three coordinates")
                verts.append((float(t[1]), float(t[2]), float(t[3])))
            elif t[0] == "f":
                idx = []
                for tok in t[1:]:
                    i = int(tok.split("/")[0])
                    i = i - 1 if i > 0 else len(verts) + i
                    if i < 0 or i >= len(verts):
                        raise ValueError(f"{path}:{ln}: face index {tok!r} out of range")
                    idx.append(i)
                if len(idx) < 3:
                    raise ValueError(f"{path}:{ln}: a face needs three corners")
                faces += [(idx[0], idx[k], idx[k + 1]) for k in range(1, len(idx) - 1)]
    return (np.array(verts, np.float32).reshape(-1, 3), np.array(faces, np.int32).reshape(-1, 3))
