"""The calibration behind ``decode(..., dtype="auto")`` as a test (CPU).

"auto" picks bf16 up to ``api.BF16_MAX_LATENT_RMS``, fp16 up to ``api.FP16_MAX_LATENT_RMS`` and
fp32 above, and promises SURVEY §8(c)'s bound against the fp64 decoder for the dtype it picks
(1e-2 for bf16, 2e-3 for fp16).  Here the 16-bit precision-contract oracle
(``decoder_forward_lowp``: the kernels' roundings, no device in the loop) is held to those bounds
at each threshold and at the two 0.05 steps below it, on a fixed calibration set; the device is
held to them on the same set in tests/test_gpu_decoder.py (``test_auto_contract_*``), which
imports the set from here.

Calibration set: seeds 100..103; per seed 4 latents drawn N(0, 1) and normalised per shape to
RMS r, and per shape 1016 uniform points of [-1, 1]^3 followed by the cube's 8 corners; both
decoders the GPU tests use (DeepSDF L = 256 seed 1234, widen-skip L = 1024 seed 1235).
"""
import functools
import itertools

import pytest
import torch

from oracle import ref_cpu as R

SEEDS = (100, 101, 102, 103)
DECODERS = {"deepsdf": dict(seed=1234), "widen": dict(L=1024, widen_skip=True, seed=1235)}
TOL = {"fp16": 2e-3, "bf16": 1e-2}              # SURVEY §8(c), vs the fp64 decoder
TORCH_DT = {"fp16": torch.float16, "bf16": torch.bfloat16}
STEP = 0.05


@functools.lru_cache(maxsize=None)
def decoder_params(name):
    return R.make_decoder_params(**DECODERS[name])


def calibration_inputs(seed, L, r):
    """(z [4, L] fp32 with per-shape RMS r, pts [4, 1024, 3] fp32) of one seed."""
    g = torch.Generator().manual_seed(seed)
    z = torch.randn(4, L, generator=g)
    z = z / z.pow(2).mean(dim=1, keepdim=True).sqrt() * r
    pts = torch.rand(4, 1016, 3, generator=g) * 2 - 1
    corners = torch.tensor(list(itertools.product((-1.0, 1.0), repeat=3)))
    return z, torch.cat([pts, corners[None].expand(4, 8, 3)], dim=1).contiguous()


@functools.lru_cache(maxsize=None)
def calibration_case(name, seed, r, dtype):
    """One seed of the set with its two references, computed once per process:
    (z, pts, fp64 decoder [4, 1024], ``dtype`` precision-contract oracle [4, 1024])."""
    p = decoder_params(name)
    z, pts = calibration_inputs(seed, p.latent_dim, r)
    with torch.inference_mode():
        want = R.decoder_forward(p, z.double(), pts.double())
        lowp = R.decoder_forward_lowp(p, z.double(), pts.double(), TORCH_DT[dtype])
    return z, pts, want, lowp


def thresholds():
    from ldm_sdf import api
    return {"bf16": api.BF16_MAX_LATENT_RMS, "fp16": api.FP16_MAX_LATENT_RMS}


def test_thresholds_are_multiples_of_the_step():
    for dtype, t in thresholds().items():
        assert abs(t / STEP - round(t / STEP)) < 1e-9 and t > 0, (dtype, t)


@pytest.mark.parametrize("below", [0, 1, 2])
@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("name", list(DECODERS))
def test_lowp_oracle_within_bound_up_to_threshold(name, dtype, below):
    """max |16-bit oracle - fp64 decoder| over the calibration set stays inside §8(c)'s bound at
    the dtype's "auto" threshold and at the two 0.05 steps below it."""
    r = round(thresholds()[dtype] - below * STEP, 10)
    worst = 0.0
    for seed in SEEDS:
        _, _, want, lowp = calibration_case(name, seed, r, dtype)
        e = float((lowp - want).abs().max())
        print(f"calibration {name} {dtype} rms {r:.2f} seed {seed}: max |lowp - fp64| {e:.3e}")
        worst = max(worst, e)
    print(f"calibration {name} {dtype} rms {r:.2f}: max over seeds {worst:.3e} "
          f"(bound {TOL[dtype]:.0e})")
    assert worst <= TOL[dtype], (name, dtype, r, worst)
