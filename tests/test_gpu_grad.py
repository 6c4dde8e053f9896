"""Decoder input gradients on the MI355X: csrc/decoder_grad.hip against the CPU
emulation of its own rounding map (tests/decoder_grad_emulation.py: TOL = 4 x the CPU-measured
noise floors; at most FLIP_CAP of a case's points set aside, 4 x the CPU-measured share and 8 %
at the most), a closed-form network, the fp64 oracle in aggregate, and the Python surface built on it (sdf_grad, vertex_normals,
extract_mesh(normals=True), fit_latents).  Per-point gradients are never held to the fp64
decoder with a max bound: a ReLU network's gradient is piecewise constant and 16-bit activation
noise flips near-zero units."""
import numpy as np
import pytest
import torch

from tests import decoder_grad_emulation as E

pytestmark = pytest.mark.gpu
DTYPES = ["fp16", "bf16"]
BOUND = {"fp16": 2e-3, "bf16": 1e-2}              # SURVEY §8(c), vs the fp64 decoder
PS = (1, E.TILE - 1, E.TILE + 1, 3 * E.TILE + 5)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import ldm_sdf
    ldm_sdf.load_library()
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def nets():
    """(oracle params, SDFDecoder) of the two test decoders (seed 1234)."""
    from ldm_sdf import SDFDecoder
    out = {}
    for kind in ("deepsdf", "widen"):
        p = E.make_params(kind)
        out[kind] = (p, SDFDecoder(p.latent_dim, weights=p.weights, biases=p.biases))
    return out


def _device(dec, dev, z, xyz, dtype, gt=None, delta=1.0):
    """One kernel call + reduction + transposed fold, as fp64 CPU tensors."""
    from ldm_sdf import ops
    fdesc = dec.device_pack(dtype, dev)["desc"]
    gdesc = dec.device_pack_grad(dtype, dev)["desc"]
    beta = ops.decoder_fold(fdesc, z.to(dev))
    B, P = xyz.shape[:2]
    kw = {} if gt is None else dict(gt=gt.to(dev), delta=delta, scale=1.0 / (B * P),
                                    want_loss=True)
    out = ops.decoder_points_grad(gdesc, beta, xyz.to(dev), want_dbeta=True, **kw)
    out["dz"] = ops.decoder_fold_bwd(gdesc, out["dbeta"])
    got = {k: v.cpu().double() for k, v in out.items()}
    if "loss" in got:
        got["loss"] = got["loss"][0]
    return got


# ------------------------------------------------------------------------------- known answer
@pytest.mark.parametrize("dtype", DTYPES)
def test_known_answer_l1_ball(dev, dtype):
    """The L1-ball network of tests/test_oracle.py at L = 256, H = 512, f = tanh(c (|x| + |y| +
    |z|) - r): the backward carries rd_T(c) through 7 identity layers (rounding is idempotent),
    so for points off the coordinate planes dxyz = s_p * (+-rd_T(c)) BITWISE per axis, with
    s_p = fl32(1 - f_p^2) of the returned f_p; f matches the closed form at §8(c)'s bound."""
    import ldm_sdf
    from oracle import ref_cpu as R
    L, c, r = 256, 0.7, 0.25
    p = R.make_decoder_params(L=L, H=512, seed=0)
    for w, b in zip(p.weights, p.biases):
        w.zero_()
        b.zero_()
    for a in range(3):
        p.weights[0][2 * a, L + a] = 1.0
        p.weights[0][2 * a + 1, L + a] = -1.0
    for l in range(1, 8):
        for k in range(6):
            p.weights[l][k, k] = 1.0
    p.weights[8][0, :6] = c
    p.biases[8][0] = -r
    dec = ldm_sdf.SDFDecoder(L, weights=p.weights, biases=p.biases)
    g = torch.Generator().manual_seed(5)
    xyz = torch.rand(2, 3 * E.TILE + 5, 3, generator=g) * 2 - 1
    xyz = torch.where(xyz.abs() < 0.05, torch.full_like(xyz, 0.05), xyz)   # off the planes
    z = torch.randn(2, L, generator=g)
    sdf, grad = ldm_sdf.sdf_grad(dec, z.to(dev), xyz.to(dev), dtype=dtype)
    sdf, grad = sdf.cpu(), grad.cpu()
    want = torch.tanh(c * xyz.double().abs().sum(2) - r)
    err = float((sdf.double() - want).abs().max())
    print(f"l1 ball {dtype}: value err {err:.2e}")
    assert err <= BOUND[dtype]
    rdc = torch.tensor(c, dtype=torch.float32).to(E.DTYPES[dtype]).float()
    s = (1.0 - sdf.double() * sdf.double()).float()            # one rounding, as the fma
    expect = s[:, :, None] * (torch.sign(xyz) * rdc)
    assert torch.equal(grad, expect)


# ---------------------------------------------------------------------- parity with the emulation
@pytest.mark.parametrize("loss_mode", [False, True], ids=["grad", "loss"])
@pytest.mark.parametrize("rms", [0.2, 0.65])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind", ["deepsdf", "widen"])
def test_parity_with_emulation(dev, nets, kind, dtype, rms, loss_mode):
    """3 shapes x P in {1, Tp - 1, Tp + 1, 3 Tp + 5}: sdf, dbeta, dz and the loss within TOL per
    size; dxyz within TOL for all but FLIP_CAP of the case's points (the share over the four
    sizes together: 3 points or 195 are too few for a share of their own).  Loss mode runs at
    delta = 1 so that every point sits inside the clamp."""
    p, dec = nets[kind]
    tol = E.TOL[dtype]
    bad = total = 0
    for P in PS:
        z, xyz, gt = E.make_inputs(p, 3, P, rms)
        g = gt if loss_mode else None
        got = _device(dec, dev, z, xyz, dtype, gt=g)
        ref = E.emulate(p, z, xyz, dtype, gt=g, delta=1.0)
        m = E.compare(got, ref)
        share = E.flipped_share(got["dxyz"], ref["dxyz"], tol["dxyz"])
        print(kind, dtype, rms, P, {k: f"{v:.2e}" for k, v in m.items()}, f"beyond TOL {share:.3f}")
        assert m["sdf"] <= tol["sdf"], (P, m)
        assert m["dbeta"] <= tol["dbeta"], (P, m)
        assert m["dz"] <= tol["dz"], (P, m)
        if loss_mode:
            dl = abs(float(got["loss"]) - float(ref["loss"]))
            assert dl <= E.loss_tol(dtype, float(ref["loss"]), 3 * P), (P, dl)
        bad += round(share * 3 * P)
        total += 3 * P
    print(kind, dtype, rms, f"points beyond TOL: {bad} of {total}")
    assert bad / total <= E.FLIP_CAP[dtype], (bad, total)


# ------------------------------------------------------------------------------------- value
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", ["deepsdf", "widen"])
def test_value_within_bound_at_threshold(dev, name, dtype):
    """sdf from the gradient kernel, latents just inside ``dtype``'s "auto" threshold, on the
    calibration set of tests/test_decode_contract.py: within §8(c)'s bound of the fp64 decoder."""
    import ldm_sdf
    from ldm_sdf import api
    from tests.test_decode_contract import SEEDS, calibration_case, decoder_params
    p = decoder_params(name)
    dec = ldm_sdf.SDFDecoder(p.latent_dim, weights=p.weights, biases=p.biases)
    r = {"bf16": api.BF16_MAX_LATENT_RMS, "fp16": api.FP16_MAX_LATENT_RMS}[dtype] * (1 - 1e-3)
    worst = 0.0
    for seed in SEEDS:
        z, pts, want, _ = calibration_case(name, seed, r, dtype)
        sdf, _ = ldm_sdf.sdf_grad(dec, z.to(dev), pts.to(dev), dtype=dtype)
        worst = max(worst, float((sdf.cpu().double() - want).abs().max()))
    print(f"value {name} {dtype} rms {r:.4f}: vs fp64 max {worst:.3e} (bound {BOUND[dtype]:.0e})")
    assert worst <= BOUND[dtype]


# ------------------------------------------------------------------------ fp64 oracle, aggregate
# max|dz - oracle| / max|oracle| of the fp64-product EMULATION against autodecoder_grads' z
# (reg_lambda = 0), 3 x 197 points, delta = 1: measured on the CPU by
# tests/test_decoder_grad_emulation.py::test_emulation_vs_fp64_oracle_in_aggregate
@pytest.mark.parametrize("dtype", DTYPES)
def test_dz_vs_fp64_oracle_in_aggregate(dev, nets, dtype):
    from oracle import ref_autodecoder as RA
    p, dec = nets["deepsdf"]
    z, xyz, gt = E.make_inputs(p, 3, 3 * E.TILE + 5, 0.2)
    got = _device(dec, dev, z, xyz, dtype, gt=gt)
    _, g = RA.autodecoder_grads(p, z.double(), xyz.double(), gt.double(), 1.0, 0.0, 100)
    dev_ = E.rel_dev(got["dz"], g["z"])
    print(f"dz vs fp64 oracle {dtype}: {dev_:.2e} (emulation: {E.ORACLE_DZ[dtype]:.2e})")
    assert dev_ <= 4 * E.ORACLE_DZ[dtype]


# ------------------------------------------------------------------- more tiles than CUs, repeat
def test_more_tiles_than_cus_and_determinism(dev, nets):
    """3 x 6000 points = 282 tiles on 256 CUs: dbeta against the emulation; a second run is
    bitwise equal (no atomics, a fixed reduction order)."""
    p, dec = nets["deepsdf"]
    z, xyz, gt = E.make_inputs(p, 3, 6000, 0.2)
    a = _device(dec, dev, z, xyz, "fp16", gt=gt)
    b = _device(dec, dev, z, xyz, "fp16", gt=gt)
    for k in a:
        assert torch.equal(a[k], b[k]), k
    ref = E.emulate(p, z, xyz, "fp16", gt=gt, delta=1.0)
    m = E.compare(a, ref)
    print("6000 points:", {k: f"{v:.2e}" for k, v in m.items()})
    assert m["dbeta"] <= E.TOL["fp16"]["dbeta"] and m["dz"] <= E.TOL["fp16"]["dz"]
    assert m["sdf"] <= E.TOL["fp16"]["sdf"]
    assert E.flipped_share(a["dxyz"], ref["dxyz"], E.TOL["fp16"]["dxyz"]) <= E.FLIP_CAP["fp16"]


# -------------------------------------------------------------------------------- fit_latents
def test_fit_latents_trajectory_and_frozen_decoder(dev, nets):
    """S = 2 shapes x 2048 oracle-made samples, 50 steps (tests/decoder_grad_emulation.FIT).  The
    fp64 oracle with Adam on the CPU takes the loss from 0.2772 to 0.01633 (a drop of 0.2609,
    94 %; tests/test_decoder_grad_emulation.py re-runs it): the device's first-step dz is within
    TOL of the emulation, its 50-step drop at least 0.8 x the oracle's, and the decoder's
    weights are bitwise what they were."""
    import ldm_sdf
    p, dec = nets["deepsdf"]
    _, xyz, sdf, z0 = E.fit_case(p)
    before = [w.clone() for w in dec.weights] + [b.clone() for b in dec.biases]
    got = _device(dec, dev, z0, xyz, "bf16", gt=sdf, delta=E.FIT["delta"])
    ref = E.emulate(p, z0, xyz, "bf16", gt=sdf, delta=E.FIT["delta"])
    d0 = E.rel_dev(got["dz"], ref["dz"])
    print(f"first-step dz vs emulation: {d0:.2e}")
    assert d0 <= E.TOL["bf16"]["dz"]
    lat, losses = ldm_sdf.fit_latents(
        dec, xyz.to(dev), sdf.to(dev), steps=E.FIT["steps"], samples_per_shape=E.FIT["n"],
        lr=E.FIT["lr"], delta=E.FIT["delta"], reg_lambda=E.FIT["reg_lambda"], dtype="bf16",
        latents=z0.to(dev), return_losses=True)
    drop = losses[0] - losses[-1]
    print(f"fit_latents: loss {losses[0]:.4f} -> {losses[-1]:.4f}, oracle "
          f"{E.ORACLE_FIT_LOSS[0]:.4f} -> {E.ORACLE_FIT_LOSS[1]:.4f}")
    assert lat.shape == (2, 256) and bool(torch.isfinite(lat).all())
    assert abs(losses[0] - E.ORACLE_FIT_LOSS[0]) <= 0.02 * E.ORACLE_FIT_LOSS[0]
    assert drop >= 0.8 * (E.ORACLE_FIT_LOSS[0] - E.ORACLE_FIT_LOSS[1])
    after = dec.weights + dec.biases
    assert all(torch.equal(x, y) for x, y in zip(before, after))


# ----------------------------------------------------------------------------- vertex normals
def test_vertex_normals_and_extract_mesh(dev, nets):
    """The config-4 latent at N = 44 (83 of 216 bricks active)."""
    import ldm_sdf
    from oracle import ref_cpu as R
    p, dec = nets["deepsdf"]
    z = torch.randn(1, 256, generator=torch.Generator().manual_seed(0)) * 0.1
    (v0, f0), = ldm_sdf.extract_mesh(dec, z.to(dev), 44)
    (v, f, n), = ldm_sdf.extract_mesh(dec, z.to(dev), 44, normals=True)
    assert torch.equal(v, v0) and torch.equal(f, f0) and len(v) > 500
    assert n.shape == v.shape and n.dtype == torch.float32
    assert float((n.norm(dim=1) - 1).abs().max()) <= 1e-5
    assert torch.equal(n, ldm_sdf.vertex_normals(dec, z[0].to(dev), v))
    xyz = v.cpu()[None]
    x = xyz.double().clone().requires_grad_(True)
    R.decoder_forward(p, z.double(), x).sum().backward()
    n64 = x.grad[0] / x.grad[0].norm(dim=1, keepdim=True)
    for dtype in DTYPES:
        nd = ldm_sdf.vertex_normals(dec, z[0].to(dev), v, dtype=dtype).cpu().double()
        em = E.emulate(p, z, xyz, dtype)["dxyz"][0]
        ne = em / em.norm(dim=1, keepdim=True)
        share = E.flipped_share(nd, ne, E.TOL[dtype]["dxyz"])
        ang = torch.rad2deg(torch.acos((nd * n64).sum(1).clamp(-1, 1)))
        print(f"normals {dtype}: {len(v)} verts, beyond TOL of the emulation {share:.3f}, "
              f"median angle to fp64 {float(ang.median()):.3f} deg")
        assert share <= E.FLIP_CAP[dtype]
        if dtype == "fp16":
            assert float(ang.median()) < 4 * E.MEDIAN_ANGLE_FP16_DEG
