"""Fixed-bits checks of the split decoder's epilogue windows (csrc/decoder_fs.hip, DESIGN.md §4
"epilogue windows"): moving the accumulator reads of a finished set from the start of a part
into its MFMA gaps changes where every element is read, never what is computed, so the outputs
stay bit for bit what they were.

``golden/decoder_fs_bits.json`` covers the DeepSDF decoder in grid mode.  This file adds the
instances it leaves out, as sha1 of the fp32 outputs against ``golden/decoder_fs_bits_windows.json``,
recorded on an MI355X from a build of the commit BEFORE the window change (``record()`` below;
never regenerated from the code under test):
  * the widen-skip decoder (512-wide layer 3: dec_fs_kernel<.., 512, ..>), both dtypes, on
    (B, N, k0, k1) = (2, 129, 125, 129) -- about 1,040 tiles, so several tiles per workgroup and
    the accumulator set carried around the tile loop -- and on (1, 5, 0, 5), one ragged tile: the
    drain after the loop;
  * the DeepSDF decoder, both dtypes, in points mode on the coordinates of that 129-grid slab;
  * bricks mode, both decoders and dtypes, on the full brick list of a 16^3 grid of 2 shapes.
"""
import hashlib
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(__file__), "golden")
BITS = os.path.join(GOLD, "decoder_fs_bits_windows.json")
WIDEN_GRIDS = [(2, 129, 125, 129), (1, 5, 0, 5)]
DTYPES = ["bf16", "fp16"]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import ldm_sdf
    ldm_sdf.load_library()
    return torch.device("cuda", 0)


def make_decoder(widen):
    from ldm_sdf import SDFDecoder
    from oracle import ref_cpu as R
    if widen:
        p = R.make_decoder_params(L=1024, widen_skip=True, seed=1235)
        return SDFDecoder(1024, weights=p.weights, biases=p.biases)
    p = R.make_decoder_params(seed=1234)
    return SDFDecoder(256, weights=p.weights, biases=p.biases)


def _sha(t):
    return hashlib.sha1(np.ascontiguousarray(t.cpu().numpy()).tobytes()).hexdigest()


def _fold(dev, dec, dtype, B, seed):
    from ldm_sdf import ops
    g = torch.Generator().manual_seed(seed)
    z = (torch.randn(B, dec.latent_dim, generator=g) * 0.1).to(dev)
    desc = dec.device_pack(dtype, dev)["desc"]
    return desc, ops.decoder_fold(desc, z)


def grid_bits(dev, dec, dtype, B, N, k0, k1):
    from ldm_sdf import ops
    desc, beta = _fold(dev, dec, dtype, B, 1000 * N + 10 * k0 + B)
    return _sha(ops.decoder_grid_fwd(desc, beta, N, k0, k1))


def points_bits(dev, dec, dtype):
    from ldm_sdf import ops
    B = 2
    desc, beta = _fold(dev, dec, dtype, B, 77)
    xyz = ops.grid_coords(129, 125, 129, device=dev)[None].expand(B, -1, -1).contiguous()
    return _sha(ops.decoder_points_fwd(desc, beta, xyz))


def bricks_bits(dev, dec, dtype):
    """Every brick of a 16^3 grid of 2 shapes: 16 bricks, 64 tiles."""
    from ldm_sdf import ops
    B, N = 2, 16
    desc, beta = _fold(dev, dec, dtype, B, 78)
    n = B * (N // 8) ** 3
    bricks = torch.arange(n, dtype=torch.int32, device=dev)
    count = torch.tensor([n], dtype=torch.int32, device=dev)
    out = torch.zeros(B, N, N, N, device=dev)
    return _sha(ops.decoder_bricks_fwd(desc, beta, N, bricks, count, out))


def output_bits(dev):
    """{case: sha1}: what the tests compare and what record() wrote."""
    out = {}
    for widen in (False, True):
        dec = make_decoder(widen)
        w = "widen" if widen else "deepsdf"
        for dt in DTYPES:
            if widen:
                for B, N, k0, k1 in WIDEN_GRIDS:
                    out[f"{w}_{dt}_grid_{B}_{N}_{k0}_{k1}"] = grid_bits(dev, dec, dt, B, N, k0, k1)
            else:
                out[f"{w}_{dt}_points_129"] = points_bits(dev, dec, dt)
            out[f"{w}_{dt}_bricks_16"] = bricks_bits(dev, dec, dt)
    return out


@pytest.fixture(scope="module")
def want():
    return json.load(open(BITS))


@pytest.fixture(scope="module")
def decoders():
    return {False: make_decoder(False), True: make_decoder(True)}


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("B,N,k0,k1", WIDEN_GRIDS)
def test_widen_skip_grid_bits(dev, decoders, want, dtype, B, N, k0, k1):
    got = grid_bits(dev, decoders[True], dtype, B, N, k0, k1)
    assert got == want[f"widen_{dtype}_grid_{B}_{N}_{k0}_{k1}"]


@pytest.mark.parametrize("dtype", DTYPES)
def test_deepsdf_points_bits(dev, decoders, want, dtype):
    assert points_bits(dev, decoders[False], dtype) == want[f"deepsdf_{dtype}_points_129"]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("widen", [False, True])
def test_bricks_bits(dev, decoders, want, dtype, widen):
    w = "widen" if widen else "deepsdf"
    assert bricks_bits(dev, decoders[widen], dtype) == want[f"{w}_{dtype}_bricks_16"]


def record(path):
    """Write the table from the library that is loaded: run on the PARENT build only."""
    import ldm_sdf
    ldm_sdf.load_library()
    bits = output_bits(torch.device("cuda", 0))
    with open(path, "w") as f:
        json.dump(bits, f, indent=1, sort_keys=True)
        f.write("\n")
    return bits
