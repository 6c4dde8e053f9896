"""Small API pieces on the MI355X: the library's latent-RMS reduction behind dtype="auto"
(``ldm_latent_rms_max``, csrc/decoder.hip) against torch, and the "auto" choice it drives."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import ldm_sdf
    ldm_sdf.load_library()
    return torch.device("cuda", 0)


@pytest.mark.parametrize("B,L", [(1, 256), (8, 256), (64, 256), (3, 1024), (1000, 7)])
def test_latent_rms_max_matches_torch(dev, B, L):
    from ldm_sdf import ops
    g = torch.Generator().manual_seed(B * 31 + L)
    z = (torch.randn(B, L, generator=g) * torch.rand(B, 1, generator=g) * 2).to(dev)
    want = float(z.double().pow(2).mean(dim=1).sqrt().max())
    got = ops.latent_rms_max(z)
    assert abs(got - want) <= 1e-6 * want, (got, want)


def _rms_max_ref(z):
    """The CPU reference: torch's max propagates NaN, and a NaN beats an Inf."""
    return float(z.cpu().double().pow(2).mean(dim=1).sqrt().max())


def _same(got, want):
    return (math.isnan(got) and math.isnan(want)) or got == want


def _placements(B, L):
    """(shape, element) of the one non-finite entry: first / last shape (with B = 5 and 9 the
    kernel's wave 0 takes the last shape on its second / third trip), first element, a wave's
    last lane, the row's last element."""
    return [(b, k) for b in sorted({0, B - 1}) for k in (0, 63, L - 1)]


@pytest.mark.parametrize("B", [1, 5, 9])
@pytest.mark.parametrize("bad", [float("nan"), float("inf"), float("-inf")])
def test_latent_rms_max_propagates_non_finite(dev, B, bad):
    """One NaN element anywhere makes the result NaN, one +-Inf element makes it +Inf (a max
    that drops NaN let such a batch pick a 16-bit format)."""
    from ldm_sdf import ops
    L = 256
    g = torch.Generator().manual_seed(B)
    base = torch.randn(B, L, generator=g) * 0.1
    for b, k in _placements(B, L):
        z = base.clone()
        z[b, k] = bad
        want = _rms_max_ref(z)
        assert math.isnan(want) if math.isnan(bad) else want == math.inf
        got = ops.latent_rms_max(z.to(dev))
        assert _same(got, want), (B, b, k, bad, got, want)


@pytest.mark.parametrize("B", [5, 9])
def test_latent_rms_max_nan_beats_inf(dev, B):
    """A NaN in one shape and an Inf in another, in either order, on the same wave (shapes 0 and
    B - 1 here) and on two waves: NaN."""
    from ldm_sdf import ops
    g = torch.Generator().manual_seed(B)
    base = torch.randn(B, 256, generator=g) * 0.1
    for b_nan, b_inf in [(0, B - 1), (B - 1, 0), (0, 1), (1, 0), (2, B - 1)]:
        for inf in (math.inf, -math.inf):
            z = base.clone()
            z[b_nan, 63] = math.nan
            z[b_inf, 0] = inf
            assert math.isnan(_rms_max_ref(z))
            got = ops.latent_rms_max(z.to(dev))
            assert math.isnan(got), (B, b_nan, b_inf, inf, got)


def test_latent_rms_max_nan_short_rows(dev):
    """L = 7 < one wave: most lanes hold no element; the NaN sits in the row's last one."""
    from ldm_sdf import ops
    g = torch.Generator().manual_seed(6)
    base = torch.randn(6, 7, generator=g)
    assert ops.latent_rms_max(base.to(dev)) == pytest.approx(_rms_max_ref(base), rel=1e-6)
    for b in range(6):
        z = base.clone()
        z[b, 6] = math.nan
        assert math.isnan(_rms_max_ref(z))
        got = ops.latent_rms_max(z.to(dev))
        assert math.isnan(got), (b, got)


def _normalised(B, L, rms, seed):
    """Random latents, each shape scaled to ``rms`` (a float or one value per shape)."""
    g = torch.Generator().manual_seed(seed)
    z = torch.randn(B, L, generator=g)
    return z / z.pow(2).mean(dim=1, keepdim=True).sqrt() * torch.as_tensor(rms).reshape(-1, 1)


def _picks(z, dev):
    """("auto" on the device, "auto" on the host) for the same values."""
    from ldm_sdf import api
    api.clear_auto_cache()
    on_dev = api.resolve_decode_dtype("auto", z.to(dev))
    api.clear_auto_cache()
    return on_dev, api.resolve_decode_dtype("auto", z)


@pytest.mark.parametrize("bad", [float("nan"), float("inf"), float("-inf")])
def test_auto_dtype_non_finite_is_fp32(dev, bad):
    """No 16-bit format for a batch whose scale is unknown: device and host both pick fp32."""
    for B, b in ((1, 0), (9, 0), (9, 8), (9, 5)):
        z = _normalised(B, 256, 0.1, seed=B)
        z[b, 63] = bad
        assert _picks(z, dev) == ("fp32", "fp32"), (B, b, bad)


def test_auto_dtype_device_matches_host_at_thresholds(dev):
    """1e-3 either side of each threshold (far more than the fp32 reductions differ by), on
    random per-shape-normalised latents: the pick is the one the constants state, on both."""
    from ldm_sdf import api
    for T, below, above in ((api.BF16_MAX_LATENT_RMS, "bf16", "fp16"),
                            (api.FP16_MAX_LATENT_RMS, "fp16", "fp32")):
        for B, L in ((4, 256), (9, 1024)):
            assert _picks(_normalised(B, L, T * (1 - 1e-3), seed=L + B), dev) == (below, below)
            assert _picks(_normalised(B, L, T * (1 + 1e-3), seed=L + B), dev) == (above, above)


def test_auto_dtype_is_decided_by_the_largest_shape(dev):
    """B = 9 (the ninth shape is wave 0's third): eight shapes at RMS 0.1 and one larger."""
    for last, want in ((0.3, "fp16"), (1.5, "fp32")):
        for pos in (8, 0, 5):
            rms = [0.1] * 9
            rms[pos] = last
            assert _picks(_normalised(9, 256, rms, seed=9), dev) == (want, want), (last, pos)


def test_auto_dtype_on_device(dev):
    import ldm_sdf
    from ldm_sdf import api
    api.clear_auto_cache()
    z = torch.ones(4, 256, device=dev)
    for scale, want in ((0.1, "bf16"), (0.5, "fp16"), (2.0, "fp32")):
        assert ldm_sdf.resolve_decode_dtype("auto", z * scale) == want
