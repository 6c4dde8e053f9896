"""Decoder input gradients, the host side (no GPU): the argument checks of the new C-ABI entry
points from C (tests/c/grad_errors.c, the source `make check-asan` also runs under host
AddressSanitizer) and through ctypes, the workspace size formula, the packing, the PLY writer
with and without normals, and the Python API's argument checks."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

from tests.c_checker import run_c_checker

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, EALIGN, ENOSPC, ENOSYS = -22, -14, -28, -38
A = 0x7f0000000000          # fake device addresses: never dereferenced by the host checks


def test_grad_errors_from_c(tmp_path):
    run_c_checker("grad_errors", tmp_path)


@pytest.mark.parametrize("B,P", [(1, 1), (1, 64), (1, 65), (3, 197), (64, 16384), (3, 6000)])
def test_workspace_size_formula(B, P):
    """[tiles][2][512] fp32 partial sums + one fp32 loss partial per tile (rounded up to 256 B),
    tiles = B ceil(P / 64)."""
    from ldm_sdf import _capi as capi, ops
    tiles = B * -(-P // ops.GRAD_TILE)
    want = tiles * 2 * 512 * 4 + -(-tiles * 4 // 256) * 256
    for code in (capi.LDM_F16, capi.LDM_BF16):
        assert capi.load().ldm_decoder_grad_ws_bytes(B, P, code) == want
        assert ops.decoder_grad_ws_bytes(B, P, code) == want
    assert capi.load().ldm_decoder_grad_ws_bytes(B, P, capi.LDM_F32) == 0


def test_workspace_size_invalid():
    from ldm_sdf import _capi as capi
    lib = capi.load()
    for B, P in ((0, 8), (8, 0), (-1, 8), (65536, 8), (1 << 15, 1 << 16)):
        assert lib.ldm_decoder_grad_ws_bytes(B, P, capi.LDM_F16) == 0


def _desc(capi, **kw):
    d = capi.DecoderGrad(abi_version=capi.ABI_VERSION, dtype=capi.LDM_F16, skip_width=253,
                         latent_dim=256, bias=A + 0x100000, wxyz=A + 0x200000, wz=A + 0x300000,
                         w_last=A + 0x400000, b_last=0.0)
    for l in range(1, 8):
        d.w[l] = A + 0x1000000 * l
        d.wt[l] = A + 0x1000000 * (l + 8)
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def test_entry_points_reject_bad_arguments_through_ctypes():
    from ldm_sdf import _capi as capi
    lib = capi.load()
    f = A + 0x10000000
    need = lib.ldm_decoder_grad_ws_bytes(2, 100, capi.LDM_F16)
    d = _desc(capi)

    def call(**k):
        return lib.ldm_decoder_points_grad(
            k.get("desc", C.byref(d)), k.get("beta", f), k.get("xyz", f + 0x1000), k.get("B", 2),
            k.get("P", 100), k.get("gt", None), k.get("delta", 0.0), 0.005,
            k.get("sdf", f + 0x2000), k.get("dxyz", f + 0x3000), k.get("dbeta", f + 0x4000),
            k.get("loss", None), k.get("ws", f + 0x100000), k.get("ws_bytes", need), None)
    assert call(desc=None) == EINVAL and call(beta=None) == EINVAL and call(sdf=None) == EINVAL
    assert call(B=0) == EINVAL and call(P=0) == EINVAL
    assert call(beta=f + 4) == EALIGN and call(ws=f + 0x100010) == EALIGN
    assert call(ws_bytes=need - 1) == ENOSPC and b"workspace" in lib.ldm_last_error()
    assert call(loss=f + 0x5000) == EINVAL and b"gt" in lib.ldm_last_error()
    assert call(gt=f + 0x6000, delta=0.0) == EINVAL
    assert call(desc=C.byref(_desc(capi, dtype=capi.LDM_F32))) == ENOSYS
    assert call(desc=C.byref(_desc(capi, abi_version=capi.ABI_VERSION - 1))) == EINVAL
    assert lib.ldm_decoder_fold_bwd(C.byref(d), None, 2, f, None) == EINVAL
    assert lib.ldm_decoder_fold_bwd(C.byref(d), f, 0, f + 0x1000, None) == EINVAL
    assert lib.ldm_decoder_fold_bwd(C.byref(_desc(capi, wz=None)), f, 2, f + 0x1000, None) == EINVAL


def test_descriptor_layout_matches_c(tmp_path):
    from ldm_sdf import _capi as capi
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        pytest.skip("no C compiler")
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "ldm_sdf.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu %zu\\n", sizeof(ldm_decoder_grad_t),'
                   ' offsetof(ldm_decoder_grad_t, w), offsetof(ldm_decoder_grad_t, wt),'
                   ' offsetof(ldm_decoder_grad_t, bias), offsetof(ldm_decoder_grad_t, b_last));'
                   ' return 0; }\n')
    exe = str(tmp_path / "layout")
    subprocess.run([cc, "-I", os.path.join(ROOT, "include"), str(src), "-o", exe], check=True)
    got = [int(x) for x in subprocess.run([exe], capture_output=True, text=True).stdout.split()]
    G = capi.DecoderGrad
    assert got == [C.sizeof(G), G.w.offset, G.wt.offset, G.bias.offset, G.b_last.offset]


@pytest.mark.parametrize("kind,dtype", [("deepsdf", "fp16"), ("widen", "bf16")])
def test_pack_decoder_grad(kind, dtype):
    """Row-major and transposed copies in T, zero padded to 256 at skip width 253; fp32 biases
    with the folded layers' rows left zero."""
    from ldm_sdf import pack
    from tests import decoder_grad_emulation as E
    p = E.make_params(kind)
    L, dt = p.latent_dim, E.DTYPES[dtype]
    h = pack.pack_decoder_grad(p.weights, p.biases, L, dtype)
    hs = p.weights[3].shape[0]
    S = 256 if hs == 253 else 512
    assert h["skip_width"] == hs and h["latent_dim"] == L
    for l in range(1, 8):
        M, K = (S if l == 3 else 512), (S if l == 4 else 512)
        assert h["w"][l].shape == (M, K) and h["w"][l].dtype == dt
        assert h["wt"][l].shape == (K, M) and h["wt"][l].is_contiguous()
        assert torch.equal(h["wt"][l], h["w"][l].T)
        src = p.weights[l][:, :hs] if l == 4 else p.weights[l]
        assert torch.equal(h["w"][l][:src.shape[0], :src.shape[1]], src.float().to(dt))
        assert float(h["w"][l][src.shape[0]:].abs().sum()) == 0
        assert float(h["w"][l][:, src.shape[1]:].abs().sum()) == 0
    assert h["bias"].shape == (8, 512) and float(h["bias"][[0, 4]].abs().sum()) == 0
    assert torch.equal(h["bias"][3, :hs], p.biases[3].float())
    assert torch.equal(h["w_last"], p.weights[8][0].float())
    assert torch.equal(h["wz"][1], p.weights[4][:, hs:hs + L].float())
    assert torch.equal(h["wxyz"][0], p.weights[0][:, L:].float())
    with pytest.raises(ValueError):
        pack.pack_decoder_grad(p.weights, p.biases, L, "fp32")


def _fixture_mesh():
    from oracle import ref_mc
    g = np.linspace(-1, 1, 12, dtype=np.float32)
    z, y, x = np.meshgrid(g, g, g, indexing="ij")
    vol = (np.sqrt(x * x + y * y + z * z) - 0.6).astype(np.float32)
    return ref_mc.marching_cubes(vol, 0.0)[:2]


def test_write_ply_without_normals_is_byte_identical(tmp_path):
    """Without the argument the file is, byte for byte, what ``write_ply`` wrote before it took
    normals: tests/golden/sphere12_parent*.ply were written by that version from this fixture
    mesh (plain, and with offset / scale).  The oracle's writer agrees too."""
    import ldm_sdf
    from oracle import ref_mc
    v, f = _fixture_mesh()
    assert len(v) > 50 and len(f) > 50
    gold = os.path.join(ROOT, "tests", "golden", "sphere12_parent.ply")
    gold_os = os.path.join(ROOT, "tests", "golden", "sphere12_parent_offset_scale.ply")
    a, b = str(tmp_path / "a.ply"), str(tmp_path / "b.ply")
    ldm_sdf.write_ply(a, torch.from_numpy(v), torch.from_numpy(f))
    assert open(a, "rb").read() == open(gold, "rb").read()
    ref_mc.write_ply(b, v, f)
    assert open(b, "rb").read() == open(gold, "rb").read()
    assert b"nx" not in open(a, "rb").read().split(b"end_header\n")[0]
    ldm_sdf.write_ply(a, v, f, normals=None)
    assert open(a, "rb").read() == open(gold, "rb").read()
    ldm_sdf.write_ply(a, v, f, offset=[0.1, 0.2, 0.3], scale=2.0)
    assert open(a, "rb").read() == open(gold_os, "rb").read()


def test_write_ply_with_normals_round_trips(tmp_path):
    import ldm_sdf
    v, f = _fixture_mesh()
    n = v / np.linalg.norm(v, axis=1, keepdims=True)
    path = str(tmp_path / "n.ply")
    ldm_sdf.write_ply(path, v, f, normals=torch.from_numpy(n))
    raw = open(path, "rb").read()
    head, body = raw.split(b"end_header\n", 1)
    lines = head.decode().split("\n")
    assert lines[:3] == ["ply", "format binary_little_endian 1.0", f"element vertex {len(v)}"]
    assert lines[3:9] == [f"property float {k}" for k in ("x", "y", "z", "nx", "ny", "nz")]
    vn = np.frombuffer(body[:len(v) * 24], "<f4").reshape(-1, 6)
    assert np.array_equal(vn[:, :3], v) and np.array_equal(vn[:, 3:], n.astype("<f4"))
    rec = np.frombuffer(body[len(v) * 24:], dtype=[("n", "u1"), ("v", "<i4", (3,))])
    assert len(rec) == len(f) and np.all(rec["n"] == 3) and np.array_equal(rec["v"], f)
    with pytest.raises(ValueError):
        ldm_sdf.write_ply(path, v, f, normals=n[:-1])


def test_python_argument_checks():
    import ldm_sdf
    dec = ldm_sdf.SDFDecoder(256, seed=1234)
    z, xyz, sdf = torch.zeros(2, 256), torch.zeros(2, 10, 3), torch.zeros(2, 10)
    for dt in ("fp32", "auto", "f16"):
        with pytest.raises(ldm_sdf.LdmError):
            ldm_sdf.sdf_grad(dec, z, xyz, dtype=dt)
        with pytest.raises(ldm_sdf.LdmError):
            ldm_sdf.fit_latents(dec, xyz, sdf, dtype=dt)
        with pytest.raises(ldm_sdf.LdmError):
            dec.device_pack_grad(dt, "cpu")
    # CPU tensors: no fallback
    with pytest.raises(ldm_sdf.LdmError):
        ldm_sdf.sdf_grad(dec, z, xyz)
    with pytest.raises(ldm_sdf.LdmError):
        ldm_sdf.fit_latents(dec, xyz, sdf, steps=1)
    with pytest.raises(ldm_sdf.LdmError):
        ldm_sdf.vertex_normals(dec, z[0], xyz[0])
    with pytest.raises(ldm_sdf.LdmError):
        ldm_sdf.extract_mesh(dec, z, 16, normals=True)
    # shapes and values
    for bad in (dict(xyz=xyz[:, :, :2]), dict(sdf=sdf[:, :5]), dict(steps=-1),
                dict(samples_per_shape=0), dict(delta=0.0), dict(lr=0.0),
                dict(latents=torch.zeros(3, 256))):
        kw = dict(xyz=xyz, sdf=sdf)
        kw.update(bad)
        x, s = kw.pop("xyz"), kw.pop("sdf")
        with pytest.raises(ValueError):
            ldm_sdf.fit_latents(dec, x, s, **kw)
