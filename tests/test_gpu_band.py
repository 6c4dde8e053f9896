"""Narrow-band decode on the MI355X: the classify / compaction passes against
the numpy reference, and ``decode_band`` held to ``decode`` BIT FOR BIT -- on every voxel when
every brick is active, on every voxel of an active brick otherwise -- and to a bitwise-equal
mesh whenever the dense volume's own crossing cells lie in active bricks.

Decoders are those of tests/test_gpu_decoder.py (seed 1234 at L = 256; the widen-skip decoder
at L = 1024 where named); latents are randn(seed 47) x 0.1."""
import math

import numpy as np
import pytest
import torch

from tests import band_reference as BR

pytestmark = pytest.mark.gpu
DTYPES = ["fp32", "bf16", "fp16"]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import ldm_sdf
    ldm_sdf.load_library()
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def decoder():
    from ldm_sdf import SDFDecoder
    from oracle import ref_cpu as R
    p = R.make_decoder_params(seed=1234)
    return SDFDecoder(256, weights=p.weights, biases=p.biases)


@pytest.fixture(scope="module")
def widen_decoder():
    from ldm_sdf import SDFDecoder
    from tests.test_decode_contract import decoder_params
    p = decoder_params("widen")
    return SDFDecoder(1024, weights=p.weights, biases=p.biases)


@pytest.fixture(scope="module")
def l1_decoder():
    """The L1-ball network of tests/test_oracle.py::test_analytic_l1_network at L = 256,
    H = 512: sdf = tanh(c (|x| + |y| + |z|) - r), c = 0.7, r = 0.25."""
    from ldm_sdf import SDFDecoder
    from oracle import ref_cpu as R
    L = 256
    p = R.make_decoder_params(L=L, H=512, seed=0)
    for w, b in zip(p.weights, p.biases):
        w.zero_()
        b.zero_()
    for a in range(3):
        p.weights[0][2 * a, L + a] = 1.0
        p.weights[0][2 * a + 1, L + a] = -1.0
    for l in range(1, 8):
        for c in range(6):
            p.weights[l][c, c] = 1.0
    p.weights[8][0, :6] = 0.7
    p.biases[8][0] = -0.25
    return SDFDecoder(L, weights=p.weights, biases=p.biases)


def _latents(dev, L=256):
    g = torch.Generator().manual_seed(47)
    return (torch.randn(2, L, generator=g) * 0.1).to(dev)


def _latent0(dev):
    """The config-4 latent (randn(seed 0) x 0.1, one shape).  The seed-47 field of the seed-1234
    decoder is negative on the whole box at N = 44 (fp32 oracle: max -4.3e-3 and -0.145, 31 and
    0 of 216 bricks active at band 0.05), so it has no surface to mesh; this latent has one
    (oracle: 83 of 216 bricks active at band 0.05, 3332 needed voxels, 0 missed at 0.05 and at
    0.01)."""
    g = torch.Generator().manual_seed(0)
    return (torch.randn(1, 256, generator=g) * 0.1).to(dev)


_DENSE = {}


def _dense(key, dec, z, N, dtype):
    """The dense decode of a case, computed once and shared (never modified)."""
    import ldm_sdf
    if key not in _DENSE:
        _DENSE[key] = ldm_sdf.decode(dec, z, N, dtype=dtype)
    return _DENSE[key]


# ------------------------------------------------------------------ 1. classify vs reference
def _synthetic_coarse(N, B, level, band, seed):
    nb = BR.n_bricks(N)
    rng = np.random.default_rng(seed)
    c = (rng.standard_normal((B, nb + 1, nb + 1, nb + 1)) * 0.3 + level + 0.5).astype(np.float32)
    flat = c.reshape(-1)
    pick = rng.choice(flat.size, 7, replace=False)
    flat[pick[0]] = flat[pick[1]] = np.float32(level)
    if np.isfinite(band):
        flat[pick[2]] = flat[pick[3]] = np.float32(level) + np.float32(band)
        flat[pick[4]] = flat[pick[5]] = np.float32(level) - np.float32(band)
    flat[pick[6]] = np.nan
    return c


@pytest.mark.parametrize("band", [0.125, 0.0, math.inf])
@pytest.mark.parametrize("N", [9, 33, 40, 44])
def test_classify_matches_reference(dev, N, band):
    from ldm_sdf import ops
    B, level = 3, 0.25             # level, band and level +- band are exact in fp32
    coarse = _synthetic_coarse(N, B, level, band, seed=N)
    want = BR.active_rule(coarse, level, band)
    if band == 0.125:              # the synthetic field exercises both outcomes
        assert 0 < want.sum() < want.size
    active, bricks, count = ops.band_classify(torch.from_numpy(coarse).to(dev), N, level, band)
    n = int(count.item())
    wl = BR.brick_list(want)
    assert np.array_equal(active.cpu().numpy().astype(bool), want.reshape(-1))
    assert n == len(wl)
    got = bricks[:n].cpu().numpy()
    assert np.array_equal(got, wl) and np.all(np.diff(got) > 0)
    if band == math.inf:
        assert n == B * BR.n_bricks(N) ** 3


def test_classify_spans_scan_chunks(dev):
    """B nb^3 = 3 * 17^3 = 14739 bricks: four 4096-brick scan chunks, the last one ragged."""
    from ldm_sdf import ops
    N, B = 130, 3
    coarse = _synthetic_coarse(N, B, 0.25, 0.125, seed=5)
    want = BR.active_rule(coarse, 0.25, 0.125)
    active, bricks, count = ops.band_classify(torch.from_numpy(coarse).to(dev), N, 0.25, 0.125)
    n = int(count.item())
    assert np.array_equal(active.cpu().numpy().astype(bool), want.reshape(-1))
    assert np.array_equal(bricks[:n].cpu().numpy(), BR.brick_list(want))


def test_lattice_coords_bit_exact(dev):
    from ldm_sdf import ops
    from oracle import ref_cpu as R
    for N in (9, 33, 40, 44):
        ix = BR.lattice_indices(N)
        fine = R.grid_coords_np(N, 0, N).reshape(N, N, N, 3)
        want = fine[ix[:, None, None], ix[None, :, None], ix[None, None, :]].reshape(-1, 3)
        got = ops.band_lattice_coords(N, device=dev).cpu().numpy()
        assert np.array_equal(got.view(np.uint32), np.ascontiguousarray(want).view(np.uint32))


# -------------------------------------------------- 2. all bricks active == dense, bitwise
@pytest.mark.parametrize("N", [33, 40, 44])
@pytest.mark.parametrize("dtype", DTYPES)
def test_all_active_equals_dense_bitwise(dev, decoder, dtype, N):
    """N = 33: a last brick one voxel thick; 40: exact; 44: ragged by 4.  B = 2 puts a shape
    boundary inside a workgroup's walk."""
    import ldm_sdf
    z = _latents(dev)
    dense = _dense(("d", dtype, N), decoder, z, N, dtype)
    vol, info = ldm_sdf.decode_band(decoder, z, N, dtype=dtype, band=math.inf, return_info=True)
    assert int(info.count.item()) == 2 * BR.n_bricks(N) ** 3 and bool(info.active.all())
    assert torch.equal(vol, dense)


def test_all_active_equals_dense_bitwise_widen_fp16(dev, widen_decoder):
    import ldm_sdf
    z = _latents(dev, 1024)
    dense = ldm_sdf.decode(widen_decoder, z, 20, dtype="fp16")
    vol = ldm_sdf.decode_band(widen_decoder, z, 20, dtype="fp16", band=math.inf)
    assert torch.equal(vol, dense)


# ------------------------------------------------------------- 3. band decode at N = 44
@pytest.mark.parametrize("dtype", DTYPES)
def test_band_decode_n44(dev, decoder, dtype):
    import ldm_sdf
    N, B, band = 44, 2, 0.05
    z = _latents(dev)
    dense = _dense(("d", dtype, N), decoder, z, N, dtype).cpu().numpy()
    vol, info = ldm_sdf.decode_band(decoder, z, N, dtype=dtype, band=band, return_info=True)
    vol = vol.cpu().numpy()
    coarse = info.coarse.cpu().numpy()
    nb = BR.n_bricks(N)
    assert coarse.shape == (B, nb + 1, nb + 1, nb + 1) and info.band == band
    assert np.array_equal(coarse.view(np.uint32), BR.lattice_of(dense).view(np.uint32))
    want = BR.active_rule(coarse, 0.0, band)
    got = info.active.cpu().numpy()
    assert got.shape == (B, nb, nb, nb) and np.array_equal(got, want)
    n = int(info.count.item())
    assert np.array_equal(info.bricks[:n].cpu().numpy(), BR.brick_list(want))
    print(f"{dtype}: active bricks per shape {want.reshape(B, -1).sum(1)} of {nb ** 3}")
    assert want.sum() >= 1 and (~want).sum() >= 0.25 * want.size
    on = BR.brick_to_voxels(want, N)
    assert np.array_equal(vol.view(np.uint32)[on], dense.view(np.uint32)[on])
    fill = BR.fill(coarse, N)
    assert np.array_equal(vol.view(np.uint32)[~on], fill.view(np.uint32)[~on])


# --------------------------------------------------------------- 4. bitwise-equal mesh
def _mesh_case(dev, dec, z, N, band, dtype, key, min_inactive=None):
    import ldm_sdf
    B = z.shape[0]
    dense_t = _dense(key, dec, z, N, dtype)
    dense = dense_t.cpu().numpy()
    # precondition, from the dense volume alone: every voxel marching cubes needs lies in a
    # brick the reference rule marks active
    want = BR.active_rule(BR.lattice_of(dense), 0.0, band)
    for b in range(B):
        missed = BR.needed_voxels(dense[b], 0.0) & ~BR.brick_to_voxels(want[b], N)
        assert missed.sum() == 0, (b, int(missed.sum()))
    if min_inactive is not None:
        assert (~want).sum() >= min_inactive * want.size
    vol = ldm_sdf.decode_band(dec, z, N, dtype=dtype, band=band)
    n_faces = 0
    for b in range(B):
        v0, f0 = ldm_sdf.marching_cubes(dense_t[b])
        v1, f1 = ldm_sdf.marching_cubes(vol[b])
        # a dense volume with a crossing cell has a mesh
        assert (len(f0) > 0) == bool(BR.needed_voxels(dense[b], 0.0).any())
        n_faces += len(f0)
        assert np.array_equal(v1.cpu().numpy().view(np.uint32), v0.cpu().numpy().view(np.uint32))
        assert np.array_equal(f1.cpu().numpy(), f0.cpu().numpy())
    return n_faces


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_mesh_equal_l1_ball(dev, l1_decoder, dtype):
    """|grad| of c (|x| + |y| + |z|) is c sqrt(3), and over half a brick (4 voxels per axis) the
    field moves at most 12 c vs: that is the band, + 1e-2 for the 16-bit rounding."""
    N = 64
    band = 12 * 0.7 * (2.0 / (N - 1)) + 1e-2
    z = _latents(dev)[:1]
    assert _mesh_case(dev, l1_decoder, z, N, band, dtype, ("l1", dtype, N), min_inactive=0.5) > 0


def test_mesh_equal_seed1234_bf16(dev, decoder):
    """The seed-47 pair as stated (both meshes are empty: that field has no zero crossing in the
    box, see _latent0), and the config-4 latent, whose surface crosses 83 of 216 bricks."""
    assert _mesh_case(dev, decoder, _latents(dev), 44, 0.05, "bf16", ("d", "bf16", 44)) == 0
    assert _mesh_case(dev, decoder, _latent0(dev), 44, 0.05, "bf16", ("d0", "bf16", 44)) > 0


# ---------------------------------------------------------------------- 5. extract_mesh
def test_extract_mesh_equals_decode_band_then_mc(dev, decoder):
    import ldm_sdf
    z = torch.cat([_latent0(dev), _latents(dev)[:1]])       # B = 2; shape 0 has a surface
    meshes = ldm_sdf.extract_mesh(decoder, z, 44, dtype="bf16", band=0.05)
    vol = ldm_sdf.decode_band(decoder, z, 44, dtype="bf16", band=0.05)
    assert len(meshes) == 2 and len(meshes[0][1]) > 0
    for b, (v, f) in enumerate(meshes):
        v0, f0 = ldm_sdf.marching_cubes(vol[b])
        assert torch.equal(v, v0) and torch.equal(f, f0)
    lv = ldm_sdf.extract_mesh(decoder, z, 44, dtype="bf16", band=0.05, level=-0.05,
                              bbox=(-0.5, 1.5))
    vol = ldm_sdf.decode_band(decoder, z, 44, dtype="bf16", band=0.05, level=-0.05,
                              bbox=(-0.5, 1.5))
    for b, (v, f) in enumerate(lv):
        v0, f0 = ldm_sdf.marching_cubes(vol[b], -0.05, (-0.5, 1.5))
        assert torch.equal(v, v0) and torch.equal(f, f0)


# -------------------------------------------------------------------- 6. no active brick
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_no_active_brick(dev, dtype):
    """A zero-weight decoder whose last bias makes the field tanh(0.3) everywhere, band = 0:
    count 0 (the zero-tile launch), the volume is the constant, the mesh is empty."""
    import ldm_sdf
    from oracle import ref_cpu as R
    p = R.make_decoder_params(seed=0)
    for w, b in zip(p.weights, p.biases):
        w.zero_()
        b.zero_()
    p.biases[-1].fill_(0.3)
    dec = ldm_sdf.SDFDecoder(256, weights=p.weights, biases=p.biases)
    z = _latents(dev)
    vol, info = ldm_sdf.decode_band(dec, z, 20, dtype=dtype, band=0.0, return_info=True)
    assert int(info.count.item()) == 0 and not bool(info.active.any())
    c = np.float32(np.tanh(np.float32(0.3)))
    assert float((vol - float(c)).abs().max()) <= 1e-6
    assert bool((vol == vol[0, 0, 0, 0]).all())
    v, f = ldm_sdf.marching_cubes(vol[0])
    assert len(v) == 0 and len(f) == 0
    assert all(len(f) == 0 for _, f in ldm_sdf.extract_mesh(dec, z, 20, dtype=dtype, band=0.0))


# --------------------------------------------------------------- 7. determinism and out=
def test_deterministic_into_out(dev, decoder):
    import ldm_sdf
    z = _latents(dev)
    out = torch.full((2, 44, 44, 44), float("nan"), device=dev)
    v1, i1 = ldm_sdf.decode_band(decoder, z, 44, dtype="bf16", band=0.05, out=out,
                                 return_info=True)
    assert v1.data_ptr() == out.data_ptr() and bool(torch.isfinite(out).all())
    first, n1 = out.clone(), int(i1.count.item())
    l1 = i1.bricks[:n1].clone()
    v2, i2 = ldm_sdf.decode_band(decoder, z, 44, dtype="bf16", band=0.05, out=out,
                                 return_info=True)
    n2 = int(i2.count.item())
    assert n1 == n2 and torch.equal(l1, i2.bricks[:n2]) and torch.equal(first, v2)
