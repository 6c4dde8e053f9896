"""T2/T3 decoder parity on the MI355X: HIP kernels through the C ABI vs the oracle / goldens.

Tolerances (measured CPU deviations): grid coordinates bit-exact; fp32
kernel max-abs <= 2e-6 vs fp64; fp16 <= 2e-3; bf16 <= 1e-2.
"""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(__file__), "golden")
TOL = {"fp32": 2e-6, "fp16": 2e-3, "bf16": 1e-2}


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import ldm_sdf
    ldm_sdf.load_library()
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def small():
    return dict(np.load(os.path.join(GOLD, "decoder_small.npz")))


@pytest.fixture(scope="module")
def decoder():
    from ldm_sdf import SDFDecoder
    from oracle import ref_cpu as R
    p = R.make_decoder_params(seed=1234)
    return SDFDecoder(256, weights=p.weights, biases=p.biases)


def test_native_library_is_loaded(dev):
    import ldm_sdf._capi as capi
    lib = capi.load()
    assert lib.ldm_abi_version() == capi.ABI_VERSION
    maps = open("/proc/self/maps").read()
    assert "libldm_sdf.so" in maps


@pytest.mark.parametrize("N,k0,k1", [(2, 0, 2), (32, 0, 32), (33, 5, 20), (128, 0, 128),
                                     (256, 100, 103), (512, 511, 512)])
def test_grid_coords_bit_exact(dev, N, k0, k1):
    from ldm_sdf import ops
    from oracle import ref_cpu as R
    got = ops.grid_coords(N, k0, k1, device=dev).cpu().numpy()
    want = R.grid_coords_np(N, k0, k1)
    assert got.shape == want.shape
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


def test_fold_matches_oracle(dev, decoder, small):
    from ldm_sdf import ops
    from oracle import ref_cpu as R
    z = torch.from_numpy(small["z"])
    pk = decoder.device_pack("fp32", dev)
    beta = ops.decoder_fold(pk["desc"], z.to(dev)).cpu().double()
    p = R.make_decoder_params(seed=1234)
    want = R.latent_fold(p, z.double())
    assert (beta - want).abs().max() < 1e-5


@pytest.mark.parametrize("dtype", ["fp32", "fp16", "bf16"])
def test_decode_grid_32_vs_golden(dev, decoder, small, dtype):
    import ldm_sdf
    z = torch.from_numpy(small["z"]).to(dev)
    sdf = ldm_sdf.decode(decoder, z, 32, dtype=dtype).cpu().double().numpy()
    want = small["sdf_grid"].reshape(2, 32, 32, 32)
    err = np.abs(sdf - want).max()
    assert err <= TOL[dtype], (dtype, err)
    assert np.isfinite(sdf).all()


@pytest.mark.parametrize("dtype", ["fp32", "fp16", "bf16"])
def test_decode_points_ragged_vs_golden(dev, decoder, small, dtype):
    import ldm_sdf
    z = torch.from_numpy(small["z"]).to(dev)
    pts = torch.from_numpy(small["pts"]).to(dev)          # [2, 1000, 3], 1000 % 128 != 0
    got = ldm_sdf.decode_points(decoder, z, pts, dtype=dtype).cpu().double().numpy()
    err = np.abs(got - small["sdf_pts"]).max()
    assert err <= TOL[dtype], (dtype, err)


@pytest.mark.parametrize("P", [1, 31, 129])
def test_decode_points_tiny(dev, decoder, small, P):
    import ldm_sdf
    from oracle import ref_cpu as R
    z = torch.from_numpy(small["z"][:1]).to(dev)
    pts = torch.from_numpy(small["pts"][:1, :P].copy()).to(dev)
    p = R.make_decoder_params(seed=1234)
    want = R.decoder_forward(p, z.cpu().double(), pts.cpu().double()).numpy()
    for dt in ("fp32", "bf16"):
        got = ldm_sdf.decode_points(decoder, z, pts, dtype=dt).cpu().double().numpy()
        assert np.abs(got - want).max() <= TOL[dt]


def test_widen_skip_fp16(dev):
    import ldm_sdf
    from oracle import ref_cpu as R
    g = dict(np.load(os.path.join(GOLD, "decoder_widen.npz")))
    p = R.make_decoder_params(L=1024, widen_skip=True, seed=1235)
    dec = ldm_sdf.SDFDecoder(1024, weights=p.weights, biases=p.biases)
    assert dec.widen_skip and dec.skip_width == 512
    z = torch.from_numpy(g["z"]).to(dev)
    pts = torch.from_numpy(g["pts"]).to(dev)
    for dt, lay in (("fp16", "split"), ("bf16", "split"), ("fp32", "split")):
        got = ldm_sdf.decode_points(dec, z, pts, dtype=dt).cpu().double().numpy()
        assert np.abs(got - g["sdf_pts"]).max() <= TOL[dt], (dt, lay)
        lowp = R.decoder_forward_lowp(p, z.cpu().double(), pts.cpu().double(),
                                      torch.bfloat16 if dt == "bf16" else torch.float16)
        if dt != "fp32":        # the 16-bit precision contract itself
            assert np.abs(got - lowp.numpy()).max() <= 2e-3, (dt, lay)


@pytest.mark.parametrize("dtype,layout", [("fp32", "split"), ("bf16", "split"),
                                          ("fp16", "split")])
def test_slab_equals_slice_bitwise(dev, decoder, small, dtype, layout):
    """Each point's value is independent of its tile/slab: slabs are bitwise slices."""
    from ldm_sdf import ops
    z = torch.from_numpy(small["z"]).to(dev)
    pk = decoder.device_pack(dtype, dev, layout=layout)
    beta = ops.decoder_fold(pk["desc"], z)
    N = 40
    full = ops.decoder_grid_fwd(pk["desc"], beta, N, 0, N)
    for k0, k1 in [(0, 13), (13, 27), (27, 40), (39, 40)]:
        part = ops.decoder_grid_fwd(pk["desc"], beta, N, k0, k1)
        assert torch.equal(part, full[:, k0:k1])
    # and per-shape independence: shape 1 alone == shape 1 in the batch
    one = ops.decoder_grid_fwd(pk["desc"], beta[1:2].contiguous(), N, 0, N)
    assert torch.equal(one[0], full[1])


def test_many_tiles_persistent_loop_subset(dev, decoder):
    """64^3 x 3 shapes = 6144 tiles (> 1 per CU): spot-check vs the oracle on a subset."""
    import ldm_sdf
    from oracle import ref_cpu as R
    g = torch.Generator().manual_seed(3)
    z = torch.randn(3, 256, generator=g) * 0.1
    N = 64
    sdf = ldm_sdf.decode(decoder, z.to(dev), N, dtype="bf16").cpu()
    idx = torch.randint(0, N ** 3, (3, 600), generator=g)
    grid = torch.from_numpy(R.grid_coords_np(N))
    p = R.make_decoder_params(seed=1234)
    for b in range(3):
        want = R.decoder_forward(p, z[b:b + 1].double(), grid[idx[b]].double())[0]
        got = sdf[b].reshape(-1)[idx[b]].double()
        assert (got - want).abs().max() <= TOL["bf16"]


def test_deterministic(dev, decoder, small):
    import ldm_sdf
    z = torch.from_numpy(small["z"]).to(dev)
    a = ldm_sdf.decode(decoder, z, 48, dtype="bf16")
    b = ldm_sdf.decode(decoder, z, 48, dtype="bf16")
    assert torch.equal(a, b)


def test_errors_are_loud(dev, decoder):
    import ldm_sdf
    from ldm_sdf import LdmError
    with pytest.raises(LdmError):
        ldm_sdf.decode(decoder, torch.zeros(1, 256), 8)      # CPU tensor -> no fallback
    with pytest.raises(ValueError):
        ldm_sdf.decode(decoder, torch.zeros(1, 256, device=dev), 1)


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("scale", [0.1, 0.5])
def test_split_vs_lowp_oracle(dev, decoder, dtype, scale):
    """The feature-split kernel (decoder_fs.hip) on 3 shapes x 1000 random points (8 tiles per
    shape, ragged): within the 16-bit precision-contract oracle's rounding (fp32 summation order
    and rounding-tie flips only), at the synthetic latent scale and at 5x it."""
    import ldm_sdf
    from oracle import ref_cpu as R
    g = torch.Generator().manual_seed(17)
    z = torch.randn(3, 256, generator=g) * scale
    pts = torch.rand(3, 1000, 3, generator=g) * 2 - 1
    p = R.make_decoder_params(seed=1234)
    dt = torch.bfloat16 if dtype == "bf16" else torch.float16
    out = {"split": ldm_sdf.decode_points(decoder, z.to(dev), pts.to(dev),
                                          dtype=dtype).cpu().double()}
    lowp = R.decoder_forward_lowp(p, z.double(), pts.double(), dt)
    # fp32 sums in another order + a rare activation rounding the other way at a 16-bit tie
    # (one ulp of one activation, ~1e-3 downstream; more such ties at larger latents):
    # the median stays at fp32 noise, the max within a third of the rounding error itself
    bound = 3e-3 if scale <= 0.1 else 6e-3
    for lay in ("split",):
        d_lo = (out[lay] - lowp).abs()
        e_lo, m_lo = float(d_lo.max()), float(d_lo.median())
        print(f"{lay} {dtype} z*{scale}: vs lowp max {e_lo:.2e} median {m_lo:.2e}")
        assert m_lo <= 2e-5, (lay, m_lo)
        assert e_lo <= bound, (lay, e_lo)


@pytest.fixture(scope="module")
def widen_decoder():
    from ldm_sdf import SDFDecoder
    from tests.test_decode_contract import decoder_params
    p = decoder_params("widen")
    return SDFDecoder(1024, weights=p.weights, biases=p.biases)


@pytest.fixture(scope="module")
def decoders(decoder, widen_decoder):
    return {"deepsdf": decoder, "widen": widen_decoder}


# --------------------------------------------------------------------------------------------
# dtype="auto" at its thresholds: the pick, and SURVEY §8(c)'s bound for the dtype picked, on the
# calibration set of tests/test_decode_contract.py (whose CPU half holds the 16-bit oracle to the
# same bounds).  Latents are normalised to T * (1 - 1e-3): the device RMS is within fp32 rounding
# of the target, so this is the largest scale at which the pick is certain.
# --------------------------------------------------------------------------------------------
def _auto_threshold(dtype):
    from ldm_sdf import api
    return {"bf16": api.BF16_MAX_LATENT_RMS, "fp16": api.FP16_MAX_LATENT_RMS}[dtype]


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("name", ["deepsdf", "widen"])
def test_auto_contract_at_threshold_points(dev, decoders, name, dtype):
    """decode_points with the default dtype, latents just inside ``dtype``'s threshold: "auto"
    picks ``dtype`` and the result is inside its bound vs the fp64 decoder; vs the 16-bit oracle
    the median stays at fp32 noise (the form of test_split_vs_lowp_oracle)."""
    import ldm_sdf
    from ldm_sdf import api
    from tests.test_decode_contract import SEEDS, calibration_case
    r = _auto_threshold(dtype) * (1 - 1e-3)
    worst = 0.0
    for seed in SEEDS:
        z, pts, want, lowp = calibration_case(name, seed, r, dtype)
        zd = z.to(dev)
        api.clear_auto_cache()
        assert ldm_sdf.resolve_decode_dtype("auto", zd) == dtype
        got = ldm_sdf.decode_points(decoders[name], zd, pts.to(dev)).cpu().double()
        e64 = float((got - want).abs().max())
        d_lo = (got - lowp).abs()
        e_lo, m_lo = float(d_lo.max()), float(d_lo.median())
        print(f"auto contract {name} {dtype} rms {r:.4f} seed {seed}: device vs fp64 max "
              f"{e64:.3e}, vs lowp max {e_lo:.3e} median {m_lo:.2e}")
        assert m_lo <= 2e-5, (name, dtype, seed, m_lo)
        worst = max(worst, e64)
    print(f"auto contract {name} {dtype} rms {r:.4f}: device vs fp64 max over seeds "
          f"{worst:.3e} (bound {TOL[dtype]:.0e})")
    assert worst <= TOL[dtype], (name, dtype, worst)


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("name", ["deepsdf", "widen"])
def test_auto_contract_at_threshold_grid(dev, decoders, name, dtype):
    """The same through decode(): a 17^3 grid (4913 points per shape, a ragged last tile),
    seed 100's latents, vs the fp64 decoder on the oracle's grid coordinates."""
    import ldm_sdf
    from ldm_sdf import api
    from oracle import ref_cpu as R
    from tests.test_decode_contract import calibration_inputs, decoder_params
    p = decoder_params(name)
    z, _ = calibration_inputs(100, p.latent_dim, _auto_threshold(dtype) * (1 - 1e-3))
    zd = z.to(dev)
    api.clear_auto_cache()
    assert ldm_sdf.resolve_decode_dtype("auto", zd) == dtype
    got = ldm_sdf.decode(decoders[name], zd, 17).cpu().double().reshape(4, -1)
    with torch.inference_mode():
        want = R.decoder_forward(p, z.double(), torch.from_numpy(R.grid_coords_np(17)).double())
    err = float((got - want).abs().max())
    print(f"auto contract grid 17^3 {name} {dtype}: device vs fp64 max {err:.3e}")
    assert err <= TOL[dtype], (name, dtype, err)


# --------------------------------------------------------------------------------------------
# Slot independence, bitwise: the value at a point depends on the point and its shape's latent
# only -- not on its tile, 32-point chunk or lane, not on its shape's position in the batch, and
# not on whether the kernel formed the coordinates or read them.
# --------------------------------------------------------------------------------------------
SLOT_CASES = [("deepsdf", "fp32"), ("deepsdf", "bf16"), ("deepsdf", "fp16"),
              ("widen", "fp16"), ("widen", "bf16")]


def _slot_inputs(B, P, L, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, L, generator=g) * 0.1, torch.rand(B, P, 3, generator=g) * 2 - 1, g


@pytest.mark.parametrize("name,dtype", SLOT_CASES)
def test_point_permutation_bitwise(dev, decoders, name, dtype):
    """A random permutation of 1000 points moves every point to another tile, chunk and lane
    (the MFMA B-operand column and the lane that stores the result): same bits."""
    import ldm_sdf
    dec = decoders[name]
    z, pts, g = _slot_inputs(3, 1000, dec.latent_dim, 41)
    perm = torch.randperm(1000, generator=g)
    assert int((perm % 32 != torch.arange(1000) % 32).sum()) > 900
    zd, pd = z.to(dev), pts.to(dev)
    base = ldm_sdf.decode_points(dec, zd, pd, dtype=dtype)
    moved = ldm_sdf.decode_points(dec, zd, pd[:, perm.to(dev)].contiguous(), dtype=dtype)
    assert torch.equal(moved, base[:, perm.to(dev)])


@pytest.mark.parametrize("name,dtype", SLOT_CASES)
def test_shape_permutation_bitwise(dev, decoders, name, dtype):
    """Shapes permuted with no fixed point (3 tiles per shape, the last ragged): every shape gets
    another per-shape aux slot and other tile indices; same bits."""
    import ldm_sdf
    dec = decoders[name]
    z, pts, _ = _slot_inputs(5, 300, dec.latent_dim, 43)
    pb = torch.tensor([2, 0, 4, 1, 3])
    assert bool((pb != torch.arange(5)).all())
    zd, pd = z.to(dev), pts.to(dev)
    base = ldm_sdf.decode_points(dec, zd, pd, dtype=dtype)
    moved = ldm_sdf.decode_points(dec, zd[pb.to(dev)].contiguous(),
                                  pd[pb.to(dev)].contiguous(), dtype=dtype)
    assert torch.equal(moved, base[pb.to(dev)])


@pytest.mark.parametrize("N,k0,k1", [(33, 0, 33), (40, 13, 27), (257, 255, 257)])
@pytest.mark.parametrize("dtype", ["fp32", "bf16", "fp16"])
def test_grid_mode_equals_points_mode_bitwise(dev, decoder, dtype, N, k0, k1):
    """Coordinates formed in the kernel (grid mode) against the same coordinates read from
    memory (points mode, the mode pinned tightly against the 16-bit oracle): a one-voxel slip
    at a fine resolution sits far below the fp64 bounds but not below this.  33^3 x 2 shapes is
    1124 tiles: the persistent loop, the ragged tail and a shape boundary inside a workgroup's
    walk; (257, 255, 257) is a fine grid's last two slabs."""
    from ldm_sdf import ops
    g = torch.Generator().manual_seed(47)
    z = (torch.randn(2, 256, generator=g) * 0.1).to(dev)
    desc = decoder.device_pack(dtype, dev)["desc"]
    beta = ops.decoder_fold(desc, z)
    xyz = ops.grid_coords(N, k0, k1, device=dev)[None].expand(2, -1, -1).contiguous()
    grid = ops.decoder_grid_fwd(desc, beta, N, k0, k1)
    pts = ops.decoder_points_fwd(desc, beta, xyz)
    assert grid.shape == (2, k1 - k0, N, N)
    assert torch.equal(grid.reshape(2, -1), pts)


@pytest.mark.parametrize("dtype", ["fp32", "bf16", "fp16"])
def test_decode_bbox_equals_points_bitwise(dev, decoder, dtype):
    """A non-default box reaches the kernel's coordinates (voxel size and origin) as it reaches
    ``grid_coords``."""
    import ldm_sdf
    from ldm_sdf import ops
    g = torch.Generator().manual_seed(53)
    z = (torch.randn(2, 256, generator=g) * 0.1).to(dev)
    bbox = (-0.5, 1.5)
    xyz = ops.grid_coords(33, bbox=bbox, device=dev)
    assert float(xyz.min()) == -0.5 and abs(float(xyz.max()) - 1.5) < 1e-6
    vol = ldm_sdf.decode(decoder, z, 33, bbox=bbox, dtype=dtype)
    pts = ldm_sdf.decode_points(decoder, z, xyz, dtype=dtype)
    assert torch.equal(vol.reshape(2, -1), pts)


def test_removed_layouts_fail_loudly(dev, decoder):
    """pass8 / quarter (ABI 5) and split16 (ABI 7) descriptors get LDM_ENOSYS, not a kernel."""
    from ldm_sdf import _capi as capi, ops
    from ldm_sdf import LdmError
    pk = decoder.device_pack("bf16", dev)
    beta = ops.decoder_fold(pk["desc"], torch.zeros(1, 256, device=dev))
    keep = pk["desc"].layout
    try:
        for lay in (0, 1, 3):
            pk["desc"].layout = lay
            with pytest.raises(LdmError):
                ops.decoder_grid_fwd(pk["desc"], beta, 8, 0, 8)
    finally:
        pk["desc"].layout = keep
    with pytest.raises(ValueError):
        decoder.device_pack("bf16", dev, layout="split16")
