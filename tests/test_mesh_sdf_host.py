"""CPU checks around ``mesh_sdf``: mesh normalisation and the PLY round trip,
the PLY / OBJ readers, the SdfSamples writer, surface sampling, the no-CPU-fallback rule, and
the C error-path checker tests/c/mesh_sdf_errors.c (the source `make check-asan` also runs
under host AddressSanitizer)."""
import os

import numpy as np
import pytest
import torch

from tests import mesh_sdf_reference as M
from tests.c_checker import run_c_checker


def test_normalize_then_write_ply_restores_the_mesh(tmp_path):
    import ldm_sdf
    rng = np.random.default_rng(3)
    v = (rng.uniform(-1, 1, (200, 3)) * [30.0, 8.0, 2.5] + [100.0, -40.0, 7.0]).astype(np.float32)
    f = rng.integers(0, 200, (50, 3)).astype(np.int32)
    vn, offset, scale = ldm_sdf.normalize_mesh(torch.from_numpy(v), buffer=1.03)
    vn = vn.numpy()
    # DeepSDF's convention: bounding-box centre at the origin, farthest vertex at 1 / buffer
    assert np.abs(vn.max(0) + vn.min(0)).max() <= 1e-6
    assert abs(np.linalg.norm(vn, axis=1).max() - 1 / 1.03) <= 1e-6
    assert np.allclose(vn, (v + offset.numpy()) * np.float32(scale), rtol=0, atol=1e-6)
    path = str(tmp_path / "m.ply")
    ldm_sdf.write_ply(path, vn, f, offset=offset, scale=scale)
    v2, f2 = ldm_sdf.read_ply(path)
    assert v2.dtype == np.float32 and f2.dtype == np.int32 and np.array_equal(f2, f)
    # three fp32 roundings (the product, the quotient, the difference) at the size of v
    assert np.abs(v2 - v).max() <= 4 * np.abs(v).max() * 2.0 ** -24


def test_read_ply_binary_with_normals_and_ascii(tmp_path):
    import ldm_sdf
    v, f = M.icosphere(1)
    n = v / np.linalg.norm(v, axis=1, keepdims=True)
    p1, p2, p3 = (str(tmp_path / x) for x in ("a.ply", "b.ply", "c.ply"))
    ldm_sdf.write_ply(p1, v, f)
    ldm_sdf.write_ply(p2, v, f, normals=n)
    for p in (p1, p2):
        v2, f2 = ldm_sdf.read_ply(p)
        assert np.array_equal(v2, v) and np.array_equal(f2, f)
    with open(p3, "w") as fh:
        fh.write("ply\nformat ascii 1.0\ncomment made by hand\n"
                 f"element vertex {len(v)}\nproperty float x\nproperty float y\n"
                 "property float z\nproperty uchar red\n"
                 f"element face {len(f)}\nproperty list uchar int vertex_indices\nend_header\n")
        for row in v:
            fh.write(" ".join(repr(float(x)) for x in row) + " 255\n")
        for row in f:
            fh.write("3 " + " ".join(str(int(x)) for x in row) + "\n")
    v3, f3 = ldm_sdf.read_ply(p3)
    assert np.array_equal(v3, v) and np.array_equal(f3, f)


def test_read_ply_rejects_what_it_cannot_read(tmp_path):
    import ldm_sdf
    bad = tmp_path / "x.ply"
    bad.write_bytes(b"not a ply")
    with pytest.raises(ValueError):
        ldm_sdf.read_ply(str(bad))
    bad.write_bytes(b"ply\nformat binary_big_endian 1.0\nelement vertex 0\nproperty float x\n"
                    b"property float y\nproperty float z\nelement face 0\n"
                    b"property list uchar int vertex_indices\nend_header\n")
    with pytest.raises(ValueError):
        ldm_sdf.read_ply(str(bad))
    quad = ("ply\nformat ascii 1.0\nelement vertex 4\nproperty float x\nproperty float y\n"
            "property float z\nelement face 1\nproperty list uchar int vertex_indices\n"
            "end_header\n0 0 0\n1 0 0\n1 1 0\n0 1 0\n4 0 1 2 3\n")
    bad.write_text(quad)
    with pytest.raises(ValueError):
        ldm_sdf.read_ply(str(bad))
    bad.write_text(quad.replace("4 0 1 2 3", "3 0 1 9"))        # index past the vertices
    with pytest.raises(ValueError):
        ldm_sdf.read_ply(str(bad))


def test_read_ply_malformed_files_raise_value_error_with_the_path(tmp_path):
    """Every malformed input is a ValueError that names the file: an unknown property type
    (once a KeyError), polygons among the triangles, a body cut short."""
    import ldm_sdf
    bad = tmp_path / "y.ply"
    head = ("ply\nformat ascii 1.0\nelement vertex 5\nproperty float x\nproperty float y\n"
            "property float z\nelement face 3\nproperty list uchar int vertex_indices\n"
            "end_header\n")
    vs = "0 0 0\n1 0 0\n1 1 0\n0 1 0\n0 0 1\n"
    good = head + vs + "3 0 1 2\n3 0 2 3\n3 0 1 4\n"
    bad.write_text(good)
    v, f = ldm_sdf.read_ply(str(bad))
    assert v.shape == (5, 3) and f.tolist() == [[0, 1, 2], [0, 2, 3], [0, 1, 4]]
    # unknown types, a list without a name, a quad among the triangles, a quad and a segment
    # that fill three faces' worth of tokens, a face and a file cut short, non-numbers
    cases = [good.replace("property float z", "property half z"),
             good.replace("list uchar int", "list uchar int128"),
             good.replace("list uchar int vertex_indices", "list uchar int"),
             head + vs + "3 0 1 2\n4 0 2 3 4\n3 0 1 4\n",
             head + vs + "3 0 1 2\n4 0 2 3 3\n2 1 4\n",
             head + vs + "3 0 1 2\n3 0 2 3\n3 0 1\n",
             head + vs + "3 0 1 2\n3 0 2 3\n3 0 1 x\n",
             head + vs,
             good.replace("element face 3", "element face three")]
    for text in cases:
        bad.write_text(text)
        with pytest.raises(ValueError, match="y.ply"):
            ldm_sdf.read_ply(str(bad))
    # binary: a quad among the triangles, and a face element cut short
    p = str(tmp_path / "z.ply")
    ldm_sdf.write_ply(p, v, f)
    raw = open(p, "rb").read()
    cut = tmp_path / "cut.ply"
    cut.write_bytes(raw[:-5])
    with pytest.raises(ValueError, match="cut.ply"):
        ldm_sdf.read_ply(str(cut))
    rec = np.dtype([("n", "u1"), ("v", "<i4", (3,))]).itemsize
    body = bytearray(raw)
    body[len(raw) - 2 * rec] = 4                                 # the second face's count
    cut.write_bytes(bytes(body))
    with pytest.raises(ValueError, match="cut.ply"):
        ldm_sdf.read_ply(str(cut))


def test_read_obj_forms(tmp_path):
    import ldm_sdf
    p = tmp_path / "m.obj"
    p.write_text("# a comment\nmtllib x.mtl\no thing\n"
                 "v 0 0 0\nv 1 0 0\nv 1 1 0\nv 0 1 0\nv 0.5 0.5 1 1.0\n"
                 "vt 0 0\nvn 0 0 1\n"
                 "f 1 2 3\n"              # plain
                 "f 1/1/1 3/1/1 4/1/1\n"  # v/vt/vn
                 "f 1//1 2//1 5//1\n"     # v//vn
                 "f -5 -4 -3 -2\n"        # negative, a quad: fan from its first corner
                 "s off\nusemtl m\n"
                 "f 1 2 3 4 5\n")         # a pentagon
    v, f = ldm_sdf.read_obj(str(p))
    assert v.dtype == np.float32 and v.shape == (5, 3) and f.dtype == np.int32
    assert np.array_equal(v[4], [0.5, 0.5, 1.0])
    assert f.tolist() == [[0, 1, 2], [0, 2, 3], [0, 1, 4], [0, 1, 2], [0, 2, 3],
                          [0, 1, 2], [0, 2, 3], [0, 3, 4]]
    p.write_text("v 0 0 0\nv 1 0 0\nv 0 1 0\nf 1 2 4\n")
    with pytest.raises(ValueError):
        ldm_sdf.read_obj(str(p))
    p.write_text("v 0 0 0\nv 1 0 0\nv 0 1 0\nf 0 1 2\n")         # OBJ indices start at 1
    with pytest.raises(ValueError):
        ldm_sdf.read_obj(str(p))
    p.write_text("v 0 0 0\nv 1 0 0\n")
    v, f = ldm_sdf.read_obj(str(p))
    assert v.shape == (2, 3) and f.shape == (0, 3)


def test_save_sdf_samples_round_trip_is_bitwise(tmp_path):
    import ldm_sdf
    rng = np.random.default_rng(5)
    pos = rng.standard_normal((37, 4)).astype(np.float32)
    neg = rng.standard_normal((23, 4)).astype(np.float32)
    pos[:, 3] = np.abs(pos[:, 3])
    neg[:, 3] = -np.abs(neg[:, 3])
    pos[0, 3] = 0.0
    neg[1, 3] = -1e-42                         # a denormal survives
    split = {"ds": {"cls": ["a", "b"]}}
    for inst, (p, n) in (("a", (pos, neg)), ("b", (torch.from_numpy(neg * -1), torch.from_numpy(pos * -1)))):
        path = os.path.join(str(tmp_path), "SdfSamples", "ds", "cls", inst + ".npz")
        ldm_sdf.data.save_sdf_samples(path, p, n)
        assert os.path.exists(path)
    p2, n2 = ldm_sdf.data.load_sdf_samples(os.path.join(str(tmp_path), "SdfSamples", "ds", "cls",
                                                        "a.npz"))
    assert p2.dtype == torch.float32
    assert np.array_equal(p2.numpy().view(np.uint32), pos.view(np.uint32))
    assert np.array_equal(n2.numpy().view(np.uint32), neg.view(np.uint32))
    ss = ldm_sdf.data.SdfSampleSet.from_split(str(tmp_path), split)
    assert len(ss) == 2
    xyz, sdf = ss.draw(16, generator=torch.Generator().manual_seed(0))
    assert xyz.shape == (2, 16, 3) and sdf.shape == (2, 16)
    assert (sdf[0, :8] >= 0).all() and (sdf[0, 8:] < 0).all()
    with pytest.raises(ValueError):
        ldm_sdf.data.save_sdf_samples(str(tmp_path / "x.npz"), pos[:, :3], neg)


def test_sample_surface_is_area_weighted_and_on_the_surface():
    import ldm_sdf
    v, f = M.cube_with_degenerates()
    # one cube quad refined would change the counts; here every quad has the same area
    g = torch.Generator().manual_seed(7)
    xyz, fid = ldm_sdf.sample_surface(torch.from_numpy(v), torch.from_numpy(f), 12000, g)
    assert xyz.shape == (12000, 3) and xyz.dtype == torch.float32 and fid.shape == (12000,)
    assert int(fid.max()) < 12, "a zero-area face was picked"
    counts = np.bincount(fid.numpy(), minlength=12)
    assert np.abs(counts - 1000).max() <= 5 * (1000 * 11 / 12) ** 0.5     # 5 sigma, binomial
    assert np.abs(M.box_sdf(xyz.numpy())).max() <= 1e-6
    # the point lies in the face it names, uniformly: the centroid of a face's samples is its own
    tri = v[f[0]].astype(np.float64)
    got = xyz[fid == 0].double().numpy().mean(0)
    assert np.abs(got - tri.mean(0)).max() <= 5 * 0.25 / counts[0] ** 0.5
    xyz2, fid2 = ldm_sdf.sample_surface(torch.from_numpy(v), torch.from_numpy(f), 12000,
                                        torch.Generator().manual_seed(7))
    assert torch.equal(xyz, xyz2) and torch.equal(fid, fid2)


def test_cpu_tensors_raise():
    import ldm_sdf
    v, f = M.cube_mesh()
    v, f, p = torch.from_numpy(v), torch.from_numpy(f), torch.zeros(4, 3)
    with pytest.raises(ldm_sdf.LdmError):
        ldm_sdf.mesh_sdf(v, f, p)
    with pytest.raises(ldm_sdf.LdmError):
        ldm_sdf.sample_sdf(v, f, 100)


def test_summation_constants_are_exported():
    import ldm_sdf
    assert ldm_sdf.meshsdf.face_chunk() >= 64
    assert ldm_sdf.meshsdf.split_below() >= 1
    assert ldm_sdf.meshsdf.POINT_CHUNK >= ldm_sdf.meshsdf.split_below()


def test_mesh_sdf_errors_from_c(tmp_path):
    run_c_checker("mesh_sdf_errors", tmp_path)
