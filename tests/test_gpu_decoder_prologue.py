"""The split decoder's tile prologue (csrc/decoder_fs.hip, DESIGN.md §4 "tile prologue"): the
voxel indices of a tile come from ONE scalar decomposition of its first point plus a per-lane
carry (dec::grid_voxel, csrc/grid_index.h), and layer 0 goes from the matrix pipe to LDS through
VGPR temporaries written by an inline-asm MFMA.

* grid mode against points mode fed ``ops.grid_coords``, bit for bit, at the sizes where the index
  path can go wrong: N below the lane span (2, 3, 5: several carries per lane offset), one ragged
  tile in one workgroup, N = 127 / 128 / 129 around the tile's 128 points, slabs that start at
  k0 > 0, ragged tails.  Both modes share layer 0, so this cannot see a layer-0 hazard;
* a fixed-bits check that can: sha1 of the outputs of three of those cases and of the golden 32^3
  decode against ``golden/decoder_fs_bits.json``, recorded on an MI355X from a build of the
  commit BEFORE the prologue change (never regenerated from the code under test).
"""
import hashlib
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(__file__), "golden")
# (B, N, k0, k1)
SIZES = [(1, 2, 0, 2), (1, 5, 0, 5), (3, 3, 1, 3), (2, 31, 0, 31), (2, 127, 120, 127),
         (2, 128, 0, 8), (2, 129, 125, 129), (2, 200, 197, 200)]
BITS_SIZES = [(1, 5, 0, 5), (2, 127, 120, 127), (2, 129, 125, 129)]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import ldm_sdf
    ldm_sdf.load_library()
    return torch.device("cuda", 0)


def make_decoder(widen=False):
    from ldm_sdf import SDFDecoder
    from oracle import ref_cpu as R
    if widen:
        p = R.make_decoder_params(L=1024, widen_skip=True, seed=1235)
        return SDFDecoder(1024, weights=p.weights, biases=p.biases)
    p = R.make_decoder_params(seed=1234)
    return SDFDecoder(256, weights=p.weights, biases=p.biases)


@pytest.fixture(scope="module")
def decoder():
    return make_decoder()


def grid_and_points(dev, dec, dtype, B, N, k0, k1):
    from ldm_sdf import ops
    g = torch.Generator().manual_seed(1000 * N + 10 * k0 + B)
    z = (torch.randn(B, dec.latent_dim, generator=g) * 0.1).to(dev)
    desc = dec.device_pack(dtype, dev)["desc"]
    beta = ops.decoder_fold(desc, z)
    xyz = ops.grid_coords(N, k0, k1, device=dev)[None].expand(B, -1, -1).contiguous()
    grid = ops.decoder_grid_fwd(desc, beta, N, k0, k1)
    pts = ops.decoder_points_fwd(desc, beta, xyz)
    return grid, pts


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("B,N,k0,k1", SIZES)
def test_grid_equals_points_bitwise(dev, decoder, dtype, B, N, k0, k1):
    grid, pts = grid_and_points(dev, decoder, dtype, B, N, k0, k1)
    assert grid.shape == (B, k1 - k0, N, N)
    assert torch.equal(grid.reshape(B, -1), pts)


def test_grid_equals_points_bitwise_widen_skip(dev):
    """dec_fs_kernel<.., 512, ..>: the same prologue in front of the 512-wide layer 3."""
    grid, pts = grid_and_points(dev, make_decoder(widen=True), "fp16", 2, 129, 125, 129)
    assert torch.equal(grid.reshape(2, -1), pts)


def _sha(t):
    return hashlib.sha1(np.ascontiguousarray(t.cpu().numpy()).tobytes()).hexdigest()


def output_bits(dev, dec, dtype):
    """{case: sha1 of the fp32 output bytes}; also what recorded golden/decoder_fs_bits.json."""
    import ldm_sdf
    out = {}
    for B, N, k0, k1 in BITS_SIZES:
        grid, _ = grid_and_points(dev, dec, dtype, B, N, k0, k1)
        out[f"grid_{B}_{N}_{k0}_{k1}"] = _sha(grid)
    z = torch.from_numpy(np.load(os.path.join(GOLD, "decoder_small.npz"))["z"]).to(dev)
    out["golden_32"] = _sha(ldm_sdf.decode(dec, z, 32, dtype=dtype))
    return out


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
def test_output_bits_are_the_recorded_ones(dev, decoder, dtype):
    want = json.load(open(os.path.join(GOLD, "decoder_fs_bits.json")))[dtype]
    got = output_bits(dev, decoder, dtype)
    assert got == want
