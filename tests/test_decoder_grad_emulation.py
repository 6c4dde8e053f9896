"""The frozen-decoder gradient emulation (tests/decoder_grad_emulation.py) on the CPU: it IS the
derivative of its own forward, its noise floors under another fp32 summation order stay below
the committed FLOOR, and every hand-written mistake lands beyond the device tolerance.

Measured on the GPU tests' inputs (3 shapes, P in {1, 63, 65, 197}, both decoders, latent RMS 0.2
and 0.65), fp32-chunk emulation against fp64-product emulation, worst case per dtype:

    dtype  sdf      flipped share (P >= 63)  dxyz of the rest  dbeta    dz       loss (P >= 63)
    fp16   1.0e-3   1.0 - 3.2 %              < 1e-3            2.6e-3   1.6e-3   1.1e-5
    bf16   4.1e-3   1.5 - 6.2 %              < 1e-3            2.8e-3   3.9e-3   8.9e-5

The flipped share (points whose dxyz moves by more than 1e-3 relative) is above the 2 % the
feature's issue expected of an emulation pair: the kernel's backward rounds every delta to T, and
one bf16 (2^-9) or a few fp16 (2^-12) rounding flips of delta already move a point's gradient by
more than 1e-3 without any ReLU unit flipping.  Selecting points by their smallest |a_l| (the
distance to the nearest ReLU kink) halves the fp16 share and leaves bf16's where it is, so the
inputs stay the plain uniform ones.  What the GPU parity test sets aside is measured at ITS
criterion, beyond TOL["dxyz"] = 4e-3 over a case's 978 points
(test_share_beyond_TOL_of_the_emulation_pair): 1.6 - 2.15 % (fp16) and 1.1 - 1.5 % (bf16) per
case; FLIP_CAP is 4 x the worst of them and at most 8 %.  One case of the eight, fp16 on the
widen-skip decoder at RMS 0.65, has 21 of 978 points beyond, 2 more than 2 %.
"""
import math

import pytest
import torch

from tests import decoder_grad_emulation as E

B, PS = 3, (1, 63, 65, 197)


@pytest.fixture(scope="module")
def params():
    return {k: E.make_params(k) for k in ("deepsdf", "widen")}


def _autograd_reference(p, z, xyz, dtype):
    """Autograd through a restatement of the KERNEL's forward map, the roundings to T passed
    straight through (their derivative taken as 1): f, d f / d xyz [B, P, 3], d sum_p f / d z
    [B, L] and the ReLU sign pattern per point.

    Not ``oracle.ref_cpu.decoder_forward_lowp``: that forward is the forward-only kernels' map,
    which rounds Wxyz to T and passes xyz, beta and the biases as a T hi + lo pair (~16 bits),
    while csrc/decoder_grad.hip keeps all of them in fp32.  The two forwards
    differ by more than a rounding of T at the ReLU kinks, so autograd through the oracle's
    cannot pin this backward per point.  This one is written independently of emulate(): plain
    matmuls on [z || xyz] pieces, exact sums where the emulation rounds to fp32."""
    dt = E.DTYPES[dtype]
    q = E.pieces(p)
    hs, W, b = q["hs"], q["W"], q["b"]

    def ste(x):
        return x + (E.rd(x.detach(), dt) - x.detach())

    zz = E.f32(z).requires_grad_(True)
    xx = E.f32(xyz).requires_grad_(True)
    outs, masks = [], []
    for s in range(z.shape[0]):
        beta = [zz[s] @ q["wz"][i].T + b[(0, E.SKIP)[i]] for i in range(2)]
        a = xx[s] @ q["wxyz"][0].T + beta[0]
        m = [a.detach() > 0]
        for l in range(1, 8):
            h = ste(torch.relu(a))
            if l == E.SKIP:
                a = h @ E.rd(W[l][:, :hs], dt).T + xx[s] @ q["wxyz"][1].T + beta[1]
            else:
                a = h @ E.rd(W[l], dt).T + b[l]
            m.append(a.detach() > 0)
        outs.append(torch.tanh(torch.relu(a) @ q["w_last"] + q["b_last"]))
        masks.append(torch.cat(m, dim=1))
    f = torch.stack(outs)
    f.sum().backward()
    return f.detach(), xx.grad, zz.grad, torch.stack(masks)


@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
def test_emulation_is_the_derivative_of_its_forward(params, dtype):
    """With fp64 products the emulation's backward differs from autograd through the same
    forward only by its own roundings: delta is rounded to T before each of the 7 transposed
    products, a relative perturbation of at most u = 2^-11 (fp16) / 2^-8 (bf16) per element and
    product.  To first order an output moves by at most 7 u relative to the sum of the magnitudes
    of its terms.  So: the aggregate dz and the median point sit inside 7 u; and PER POINT, over
    the points whose ReLU sign pattern is the same in both forwards (nearly all: the two differ
    by the fp32 rounding of beta and of the fma chains), the 99th percentile sits inside 7 u and
    every point inside 14 u -- the factor 2 is for the cancellation between terms, which the
    bound relative to the gradient's own norm does not see.  A mistake in the emulation's
    backward that touched a few points only would break the last two.  The values agree to fp32
    rounding of the fold and the fma chains."""
    u = 2.0 ** -11 if dtype == "fp16" else 2.0 ** -8
    p = params["deepsdf"]
    z, xyz, _ = E.make_inputs(p, B, 197, 0.2)
    em = E.emulate(p, z, xyz, dtype)
    f, gx, gz, masks = _autograd_reference(p, z, xyz, dtype)
    dv = float((em["sdf"] - f).abs().max())
    rel = ((em["dxyz"] - gx).norm(dim=2) / gx.norm(dim=2)).reshape(-1)
    same = (masks == em["masks"]).all(dim=2).reshape(-1)
    dz = E.rel_dev(em["dz"], gz)
    print(f"{dtype}: value {dv:.2e}, dxyz rel median {float(rel.median()):.2e} "
          f"max {float(rel.max()):.2e}, dz {dz:.2e}, 7u = {7 * u:.2e}; same sign pattern "
          f"{float(same.double().mean()):.3f} of the points: p99 {float(rel[same].quantile(0.99)):.2e} "
          f"max {float(rel[same].max()):.2e}")
    # the forward: fp32 fold + fma chains against exact sums can flip a rounding to T downstream
    assert dv <= (2e-3 if dtype == "fp16" else 1e-2)
    assert float(rel.median()) <= 7 * u
    assert dz <= 7 * u
    assert float(same.double().mean()) >= 0.95
    assert float(rel[same].quantile(0.99)) <= 7 * u
    assert float(rel[same].max()) <= 14 * u


def _floors(p, rms, dtype, P, loss_mode):
    z, xyz, gt = E.make_inputs(p, B, P, rms)
    g = gt if loss_mode else None
    ref = E.emulate(p, z, xyz, dtype, gt=g, delta=1.0)
    alt = E.emulate(p, z, xyz, dtype, gt=g, delta=1.0, matmul_dtype=torch.float32)
    return E.compare(alt, ref)


@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
def test_noise_floors_stay_below_FLOOR(params, dtype):
    worst = {}
    for kind, rms in E.cases():
        for P in PS:
            for loss_mode in (False, True):
                m = _floors(params[kind], rms, dtype, P, loss_mode)
                if P == 1:                    # a share of 3 points, a mean of 3 terms: see loss_tol
                    m.pop("flipped")
                    m.pop("loss", None)
                print(dtype, kind, rms, P, "loss" if loss_mode else "grad",
                      {k: f"{v:.2e}" for k, v in m.items()})
                for k, v in m.items():
                    worst[k] = max(worst.get(k, 0.0), v)
    print("worst", dtype, {k: f"{v:.2e}" for k, v in worst.items()})
    for k, v in worst.items():
        assert v <= E.FLOOR[dtype][k], (k, v, E.FLOOR[dtype][k])
    # the floors are not slack by more than 4 x either (a constant nobody re-measures)
    for k in ("sdf", "dbeta", "dz"):
        assert worst[k] >= E.FLOOR[dtype][k] / 4, (k, worst[k])
    assert E.TOL[dtype]["dxyz"] == 4 * E.FLOOR[dtype]["dxyz"]


@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
def test_share_beyond_TOL_of_the_emulation_pair(params, dtype):
    """The GPU parity test's own criterion on the CPU: per case, the share of the 3 x (1 + 63 + 65
    + 197) = 978 points whose dxyz lies beyond TOL["dxyz"] between the two emulations.  The
    record holds the worst case, and FLIP_CAP is 4 x the record, at most 8 %."""
    worst = 0.0
    for kind, rms in E.cases():
        bad = total = 0
        for P in PS:
            z, xyz, _ = E.make_inputs(params[kind], B, P, rms)
            ref = E.emulate(params[kind], z, xyz, dtype)
            alt = E.emulate(params[kind], z, xyz, dtype, matmul_dtype=torch.float32)
            bad += round(E.flipped_share(alt["dxyz"], ref["dxyz"], E.TOL[dtype]["dxyz"]) * B * P)
            total += B * P
        print(dtype, kind, rms, f"beyond TOL: {bad} of {total} = {bad / total:.4f}")
        worst = max(worst, bad / total)
    assert _within_record(worst, E.BEYOND_TOL_SHARE[dtype])
    assert E.FLIP_CAP[dtype] == min(4 * E.BEYOND_TOL_SHARE[dtype], 0.08)


@pytest.mark.parametrize("mutant", E.MUTANTS)
@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
def test_every_mutant_lands_beyond_TOL(params, dtype, mutant):
    """Each mistake moves at least one output past the device tolerance -- or, for dxyz, more
    points than FLIP_CAP allows -- on at least one of the GPU parity test's sizes (P = 1: one
    ragged tile; 65: a full tile + a ragged one of 1; 197: 3 full tiles + a ragged one of 5), for
    either decoder."""
    for kind in ("deepsdf", "widen"):
        p = params[kind]
        hit = False
        for P in (1, 65, 197):
            z, xyz, gt = E.make_inputs(p, B, P, 0.65)
            ref = E.emulate(p, z, xyz, dtype, gt=gt, delta=1.0)
            bad = E.emulate(p, z, xyz, dtype, gt=gt, delta=1.0, mutate=mutant)
            m = E.compare(bad, ref)
            share = E.flipped_share(bad["dxyz"], ref["dxyz"], E.TOL[dtype]["dxyz"])
            print(dtype, kind, mutant, P, {k: f"{v:.2e}" for k, v in m.items()},
                  f"share {share:.3f}")
            hit = hit or m["dbeta"] > E.TOL[dtype]["dbeta"] or m["dz"] > E.TOL[dtype]["dz"] \
                or (P > 1 and share > E.FLIP_CAP[dtype])
        assert hit, (kind, mutant)


def test_tile_and_tolerance_constants():
    assert E.TILE == 64
    for dt in ("fp16", "bf16"):
        assert all(math.isclose(E.TOL[dt][k], 4 * E.FLOOR[dt][k]) for k in E.FLOOR[dt])


def _within_record(measured, record):
    return measured <= record <= 1.5 * measured


@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
def test_emulation_vs_fp64_oracle_in_aggregate(params, dtype):
    """What the operand type costs the summed latent gradient, against the fp64 oracle's
    autograd: the record the GPU test multiplies by 4."""
    from oracle import ref_autodecoder as RA
    p = params["deepsdf"]
    z, xyz, gt = E.make_inputs(p, B, 197, 0.2)
    _, g = RA.autodecoder_grads(p, z.double(), xyz.double(), gt.double(), 1.0, 0.0, 100)
    em = E.emulate(p, z, xyz, dtype, gt=gt, delta=1.0)
    dev = E.rel_dev(em["dz"], g["z"])
    print(f"{dtype}: emulation dz vs fp64 oracle {dev:.3e}")
    assert _within_record(dev, E.ORACLE_DZ[dtype])


def test_oracle_fit_halves_the_loss(params):
    """The fit_latents settings of the GPU test through the fp64 oracle with Adam: the loss
    falls by far more than half (0.2772 -> 0.0163), and the record matches."""
    p = params["deepsdf"]
    _, xyz, sdf, z0 = E.fit_case(p)
    _, losses = E.oracle_fit(p, xyz, sdf, z0)
    print(f"oracle fit: {losses[0]:.5f} -> {losses[-1]:.5f}")
    assert losses[-1] <= 0.5 * losses[0]
    assert abs(losses[0] - E.ORACLE_FIT_LOSS[0]) <= 1e-4
    assert abs(losses[-1] - E.ORACLE_FIT_LOSS[1]) <= 1e-4


def test_fp16_normal_angle_record():
    """Median angle of the fp16 emulation's normals to the fp64 decoder's, on the oracle's own
    N = 44 mesh of the config-4 latent."""
    import numpy as np
    from oracle import ref_cpu as R, ref_mc
    p = E.make_params("deepsdf")
    z = torch.randn(1, 256, generator=torch.Generator().manual_seed(0)) * 0.1
    vol = R.decode_grid(p, z.double(), 44)[0].float().numpy()
    v = ref_mc.marching_cubes(vol, 0.0)[0]
    xyz = torch.from_numpy(np.asarray(v, np.float32))[None]
    x = xyz.double().clone().requires_grad_(True)
    R.decoder_forward(p, z.double(), x).sum().backward()
    n64 = x.grad[0] / x.grad[0].norm(dim=1, keepdim=True)
    em = E.emulate(p, z, xyz, "fp16")["dxyz"][0]
    ang = torch.rad2deg(torch.acos(((em / em.norm(dim=1, keepdim=True)) * n64).sum(1).clamp(-1, 1)))
    print(f"{len(v)} vertices, median angle {float(ang.median()):.4f} deg")
    assert len(v) > 500 and _within_record(float(ang.median()), E.MEDIAN_ANGLE_FP16_DEG)
