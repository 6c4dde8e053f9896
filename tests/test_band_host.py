"""Narrow-band decode, the host side (no GPU): the brick / lattice helpers against the numpy
reference, the workspace size, and the argument checks of every new C-ABI entry point -- from
Python through ctypes and from C (tests/c/band_errors.c, the source `make check-asan` also runs
under host AddressSanitizer)."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import band_reference as BR
from tests.c_checker import run_c_checker

EINVAL, EALIGN, ENOSPC = -22, -14, -28
A = 0x7f0000000000          # fake device addresses: never dereferenced by the host checks


@pytest.mark.parametrize("N", [2, 8, 9, 16, 17, 33, 40, 44, 256])
def test_helpers_match_reference(N):
    import ldm_sdf
    assert ldm_sdf.n_bricks(N) == BR.n_bricks(N) == -(-N // 8)
    got = ldm_sdf.lattice_indices(N)
    assert np.array_equal(got, BR.lattice_indices(N))
    assert len(got) == ldm_sdf.n_bricks(N) + 1 and got[0] == 0 and got[-1] == N - 1
    assert np.all(np.diff(got) >= 0)


def test_workspace_bytes_positive_and_monotone():
    from ldm_sdf import _capi as capi
    lib = capi.load()
    prev = 0
    for N in (2, 8, 9, 64, 256, 512, 1024):
        cur = lib.ldm_band_workspace_bytes(1, N)
        assert cur > 0 and cur >= prev
        prev = cur
    prev = 0
    for B in (1, 2, 16, 64):
        cur = lib.ldm_band_workspace_bytes(B, 512)
        assert cur > 0 and cur >= prev
        prev = cur
    assert lib.ldm_band_workspace_bytes(64, 512) > lib.ldm_band_workspace_bytes(1, 8)
    assert lib.ldm_band_workspace_bytes(0, 64) == 0 and lib.ldm_band_workspace_bytes(1, 1) == 0


def _bf16_desc(capi):
    return capi.Decoder(abi_version=capi.ABI_VERSION, dtype=capi.LDM_BF16, hidden=512,
                        skip_width=253, latent_dim=256, n_stages=384, weights=A + 0x1000,
                        wz=A + 0x2000, bz=A + 0x3000, wxyz=A + 0x4000, w_last=A + 0x5000,
                        b_last=0.0, layout=capi.LAYOUT_SPLIT)


def test_entry_points_reject_bad_arguments_without_gpu():
    from ldm_sdf import _capi as capi
    lib = capi.load()
    err = lambda: lib.ldm_last_error()                                        # noqa: E731
    f, u8, i32, cnt, ws = A + 0x10000, A + 0x20000, A + 0x30000, A + 0x40000, A + 0x50000
    big = 1 << 20

    assert lib.ldm_band_lattice_coords(1, 0.1, -1.0, f, None) == EINVAL
    assert lib.ldm_band_lattice_coords(16, 0.1, -1.0, None, None) == EINVAL
    assert lib.ldm_band_lattice_coords(16, 0.1, -1.0, f + 2, None) == EALIGN

    need = lib.ldm_band_workspace_bytes(2, 44)
    cl = lambda **k: lib.ldm_band_classify(                                   # noqa: E731
        k.get("coarse", f), k.get("B", 2), k.get("N", 44), 0.0, k.get("band", 0.05),
        k.get("active", u8), k.get("bricks", i32), k.get("count", cnt), k.get("ws", ws),
        k.get("ws_bytes", need), None)
    assert cl(coarse=None) == EINVAL and cl(active=None) == EINVAL
    assert cl(bricks=None) == EINVAL and cl(count=None) == EINVAL and cl(ws=None) == EINVAL
    assert cl(N=1) == EINVAL and cl(B=0) == EINVAL
    assert cl(B=big, N=512) == EINVAL and b"31 bits" in err()                 # B nb^3 >= 2^31
    assert cl(band=-1.0) == EINVAL and cl(band=float("nan")) == EINVAL
    assert cl(active=u8 + 8) == EALIGN and cl(ws=ws + 16) == EALIGN and cl(bricks=i32 + 2) == EALIGN
    assert cl(ws_bytes=need - 1) == ENOSPC and cl(ws_bytes=0) == ENOSPC and b"workspace" in err()

    fl = lambda **k: lib.ldm_band_fill(k.get("coarse", f), k.get("active", u8), k.get("B", 2),  # noqa: E731
                                       k.get("N", 44), k.get("out", f + 0x100), None)
    assert fl(coarse=None) == EINVAL and fl(active=None) == EINVAL and fl(out=None) == EINVAL
    assert fl(N=1) == EINVAL and fl(B=0) == EINVAL and fl(B=big, N=512) == EINVAL
    assert fl(out=f + 4) == EALIGN

    d = _bf16_desc(capi)
    dws = lib.ldm_workspace_bytes_layout(capi.LDM_OP_DECODER_GRID, 2, 44, d.dtype, d.layout)
    assert dws > 0
    bf = lambda **k: lib.ldm_decoder_bricks_fwd(                              # noqa: E731
        k.get("desc", C.byref(d)), k.get("beta", f), k.get("B", 2), k.get("N", 44), 0.05, -1.0,
        k.get("bricks", i32), k.get("count", cnt), k.get("out", f + 0x100), k.get("ws", ws),
        k.get("ws_bytes", dws), None)
    assert bf(desc=None) == EINVAL and bf(beta=None) == EINVAL and bf(out=None) == EINVAL
    assert bf(bricks=None) == EINVAL and bf(count=None) == EINVAL
    assert bf(N=1) == EINVAL and bf(B=0) == EINVAL
    assert bf(B=big, N=512) == EINVAL and b"31 bits" in err()
    assert bf(bricks=i32 + 1) == EALIGN and bf(beta=f + 4) == EALIGN
    assert bf(ws_bytes=dws - 1) == ENOSPC and bf(ws=None, ws_bytes=0) == ENOSPC
    stale = _bf16_desc(capi)
    stale.abi_version -= 1
    assert bf(desc=C.byref(stale)) == EINVAL


def test_decode_band_host_errors():
    import ldm_sdf
    dec = ldm_sdf.SDFDecoder(256, seed=1234)
    z = torch.zeros(1, 256)
    with pytest.raises(ldm_sdf.LdmError):
        ldm_sdf.decode_band(dec, z, 16)
    with pytest.raises(ldm_sdf.LdmError):
        ldm_sdf.extract_mesh(dec, z, 16)
    for n in (1, 0, -3):
        with pytest.raises(ValueError):
            ldm_sdf.decode_band(dec, z, n)


def test_reference_rule_on_a_hand_case():
    """The reference itself, on a case small enough to read: N = 9 (2 bricks per axis, the
    second one voxel thick, its two lattice corners coinciding at index 8)."""
    assert list(BR.lattice_indices(9)) == [0, 8, 8]
    coarse = np.full((1, 3, 3, 3), 1.0, np.float32)
    act = BR.active_rule(coarse, 0.0, 0.5)
    assert act.shape == (1, 2, 2, 2) and not act.any()
    coarse[0, 0, 0, 0] = 0.5                      # exactly level + band: brick 0 only
    assert list(BR.brick_list(BR.active_rule(coarse, 0.0, 0.5))) == [0]
    coarse[0, 0, 0, 0] = -3.0                     # far, but a sign change
    assert list(BR.brick_list(BR.active_rule(coarse, 0.0, 0.5))) == [0]
    coarse[0, 0, 0, 0] = 1.0
    coarse[0, 2, 2, 2] = np.nan                   # the far corner of brick 7 only
    assert list(BR.brick_list(BR.active_rule(coarse, 0.0, 0.5))) == [7]
    assert BR.active_rule(coarse, 0.0, np.inf).all()
    vol = np.ones((9, 9, 9), np.float32)
    vol[4, 4, 4] = -1.0
    need = BR.needed_voxels(vol, 0.0)
    assert need.sum() == 27 and need[3:6, 3:6, 3:6].all()
    f = BR.fill(np.arange(27, dtype=np.float32).reshape(1, 3, 3, 3), 9)
    assert f.shape == (1, 9, 9, 9) and f[0, 0, 0, 7] == 0 and f[0, 0, 0, 8] == 1 and f[0, 8, 8, 8] == 13


def test_band_errors_from_c(tmp_path):
    run_c_checker("band_errors", tmp_path)
