"""C19 auto-decoder training on the MI355X: the loss / ReLU-backward / segmented-sum /
regulariser kernels against the oracle and torch, the full training step's gradients against
the fp64 oracle (fp32 GEMMs: 1e-4 relative, norm-wise and element-wise), and a short fit that
lowers the loss on analytic sphere SDFs.
The bf16 matrix-core step is compared element by element (loss, every W, b and z) with its CPU
emulation, tests/autodecoder_emulation.py, at that module's TOL = 4 x the measured CPU noise floor.
"""
import pytest
import torch

from tests import autodecoder_emulation as E

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import ldm_sdf
    ldm_sdf.load_library()
    return torch.device("cuda", 0)


def test_relu_bwd(dev):
    from ldm_sdf import ops
    g = torch.Generator().manual_seed(0)
    dy, y = torch.randn(1001, generator=g), torch.randn(1001, generator=g).clamp_min(0)
    got = ops.relu_bwd(dy.to(dev), y.to(dev)).cpu()
    assert torch.equal(got, torch.where(y > 0, dy, torch.zeros_like(dy)))


@pytest.mark.parametrize("n", [1, 1000, 70001])
def test_sdf_l1_loss_matches_oracle(dev, n):
    from ldm_sdf import ops
    g = torch.Generator().manual_seed(n)
    pre = torch.randn(n, generator=g, dtype=torch.float64) * 0.2
    gt = torch.randn(n, generator=g, dtype=torch.float64) * 0.1
    pre[: n // 10] = 0.0                     # pred = 0 exactly, some targets too
    gt[: n // 20] = 0.0
    pre32, gt32 = pre.float(), gt.float()
    loss, grad = ops.sdf_l1_loss(pre32.to(dev), gt32.to(dev), 0.1, 1.0 / n)
    p = pre32.double().requires_grad_(True)
    d = 0.1
    want = (torch.tanh(p).clamp(-d, d) - gt32.double().clamp(-d, d)).abs().sum() / n
    want.backward()
    assert abs(float(loss) - float(want)) <= 1e-5 * float(want) + 1e-7
    assert torch.allclose(grad.cpu().double(), p.grad, rtol=1e-5, atol=1e-9 / n)


def test_colsum_segments(dev):
    from ldm_sdf import ops
    g = torch.Generator().manual_seed(1)
    G = torch.randn(5 * 333, 70, generator=g)
    out = torch.full((5, 70), 2.0)
    got = ops.colsum_segments(G.to(dev), 5, out.to(dev), accumulate=True).cpu()
    want = 2.0 + G.double().reshape(5, 333, 70).sum(1)
    assert (got.double() - want).abs().max() < 1e-4


@pytest.mark.parametrize("rows,cols", [(32768, 512), (20000, 300), (16000, 512), (16384, 4096)])
def test_colsum_tall(dev, rows, cols):
    """ops.colsum on tall inputs: the two-pass form (C19's 32-row bias partials, 32k x 512; a
    row count with only 32-row segments) and the one-pass form on either side of its rule, all
    against the fp64 sum; accumulate adds to what out holds."""
    from ldm_sdf import ops
    g = torch.Generator().manual_seed(rows + cols)
    G = torch.randn(rows, cols, generator=g)
    out = torch.full((cols,), 0.5)
    got = ops.colsum(G.to(dev), out.to(dev), accumulate=True).cpu()
    want = 0.5 + G.double().sum(0)
    assert (got.double() - want).abs().max() < 2e-7 * rows ** 0.5 * 8


def test_latent_reg(dev):
    from ldm_sdf import ops
    g = torch.Generator().manual_seed(2)
    z = torch.randn(7, 256, generator=g)
    z[3] = 0.0                               # zero code: no gradient, no loss
    loss = torch.tensor([0.5], device=dev)
    grad = torch.ones(7, 256, device=dev)
    ops.latent_l2_reg(z.to(dev), 0.25, loss, grad)
    zd = z.double()
    nrm = zd.norm(dim=1)
    assert abs(float(loss) - (0.5 + 0.25 * float(nrm.sum()))) < 1e-5
    want = 1.0 + 0.25 * zd / nrm.clamp_min(1e-300)[:, None]
    want[3] = 1.0
    assert (grad.cpu().double() - want).abs().max() < 1e-6


def _step(dev, case, dtype, **kw):
    """autodecoder_train_step on a constructed case: (loss, {W*, b*, z}) on the device."""
    from ldm_sdf import autodecoder_train_step
    p, z, xyz, sdf, _ = E.inputs(case)
    loss, grads, gz = autodecoder_train_step(E.masters(p, dev), z.to(dev), xyz.to(dev),
                                             sdf.to(dev), dtype=dtype, **kw)
    out = dict(grads)
    out["z"] = gz
    return loss, out


def _layout(case):
    """The step's blocking of the case, from the product's own constants."""
    from ldm_sdf import autodecoder as AD
    assert AD._KQ == E._KQ and AD._KSEG == 64 and AD.WGRAD_TILE == 17
    lay = E.layout(case[0], case[1])
    assert lay["Np"] % AD._KQ == 0 and lay["Np"] - lay["N"] < AD._KQ
    return lay


def test_train_step_fp32_grads_vs_fp64_oracle(dev):
    """fp32 step vs the fp64 oracle on constructed inputs (clear of the loss's discontinuities):
    1e-4 norm-relative AND 1e-4 element-wise (max|dev| / max|ref| per tensor; the oracle's own
    fp32-vs-fp64 floor there is 4.1e-7, tests/test_autodecoder_emulation.py)."""
    from oracle import ref_autodecoder as A
    p, z, xyz, sdf, _ = E.inputs(E.FP32_CASE)
    loss_ref, gref = A.autodecoder_grads(p, z.double(), xyz.double(), sdf.double(),
                                         reg_lambda=1e-2)
    loss, got = _step(dev, E.FP32_CASE, "fp32", reg_lambda=1e-2)
    assert abs(float(loss) - loss_ref) < 1e-4 * abs(loss_ref)
    assert set(got) == set(gref)
    for k in gref:
        g, want = got[k].cpu().double(), gref[k]
        err = float((g - want).norm() / want.norm().clamp_min(1e-30))
        dev_k = E.rel_dev(g, want)
        print(f"fp32 step {k}: norm-relative {err:.2e}, element-wise {dev_k:.2e}")
        assert err < 1e-4, (k, err)
        assert dev_k < 1e-4, (k, dev_k)


# what each bf16 case must reach (a later change of _KQ or KT must not turn one into another):
# (case, Np, KT, nblk, P % 32 == 0 [segments path], P % KT == 0 [broadcast inputs], N % 4)
BF16_CASES = [
    (E.CASE_1x64, 128, 128, 1, True, False, 0),      # non-split-K branch, segments, one shape
    (E.CASE_5x96, 512, 512, 1, True, False, 0),      # segments + gathered inputs, one padding block
    (E.CASE_3x256, 768, 256, 3, True, True, 0),      # segments, broadcast inputs, no padding, split-K
    (E.CASE_3x200, 640, 128, 5, False, False, 0),    # one-hot; blocks straddle shapes; ragged partial
    (E.CASE_2x129, 384, 128, 3, False, False, 2),    # N % 4 != 0 (scalar CbT stores), 126 pad rows
]


def _assert_reaches(case, Np, KT, nblk, segments, broadcast, n_mod4):
    S, P = case[0], case[1]
    lay = _layout(case)
    assert (lay["Np"], lay["KT"], lay["nblk"]) == (Np, KT, nblk), lay
    assert (P % 32 == 0) == segments and (P % KT == 0) == broadcast and lay["N"] % 4 == n_mod4
    return lay


@pytest.mark.parametrize("spec", BF16_CASES, ids=[E.case_id(c[0]) for c in BF16_CASES])
def test_train_step_bf16_grads_elementwise(dev, spec):
    """bf16 step (ldm_gemm_bf16 path) vs its CPU emulation: the loss and EVERY W, b and z
    element-wise within E.TOL (4 x the CPU noise floor); the loss also within 2 % of the fp64
    oracle.  The five shapes reach: the nblk == 1 branch; one all-padding 32-row block behind
    the segments path (gcs[:N // 32]); split-K without padding on broadcast inputs; the one-hot
    path with straddling blocks and a ragged last partial; N % 4 != 0 with 126 padding rows."""
    from oracle import ref_autodecoder as A
    case = spec[0]
    lay = _assert_reaches(*spec)
    N, Np = lay["N"], lay["Np"]
    if case == E.CASE_5x96:
        assert Np // 32 - N // 32 == 1 and N % 32 == 0       # exactly one all-padding block
    if case == E.CASE_3x256:
        assert Np == N
    if case == E.CASE_3x200:
        assert N % 32 == 24 and Np - N == 40 and (case[1] % lay["KT"]) != 0
    if case == E.CASE_2x129:
        assert Np - N == 126
    p, z, xyz, sdf, _ = E.inputs(case)
    want_loss, want = E.reference(case)
    loss, got = _step(dev, case, "bf16")
    E.check_against(float(loss), got, want_loss, want, f"bf16 step {E.case_id(case)}")
    loss64 = A.autodecoder_loss(p, z.double(), xyz.double(), sdf.double())
    assert abs(float(loss) - float(loss64)) < 2e-2 * abs(float(loss64))


def test_train_step_bf16_every_wgrad_tile_gives_the_same_bits(dev):
    """On the 3 x 200 case (split-K over 5 k-blocks, the one-hot product in the same launch):
    wgrad_tile 3 and 14 give every gradient bit for bit as the default 17 does, and a second
    call into the same preallocated grads= dict returns identical bits."""
    case = E.CASE_3x200
    _assert_reaches(*[s for s in BF16_CASES if s[0] == case][0])
    loss0, ref = _step(dev, case, "bf16")
    ref = {k: v.clone() for k, v in ref.items()}
    for tile in (3, 14, 17):
        loss, got = _step(dev, case, "bf16", wgrad_tile=tile)
        assert torch.equal(loss, loss0)
        for k in ref:
            assert torch.equal(got[k], ref[k]), (tile, k, float((got[k] - ref[k]).abs().max()))
    pre = {k: torch.full_like(v, float("nan")) for k, v in ref.items() if k != "z"}
    for _ in range(2):
        loss, got = _step(dev, case, "bf16", grads=pre)
        assert torch.equal(loss, loss0)
        for k in ref:
            assert k == "z" or got[k] is pre[k]
            assert torch.equal(got[k], ref[k]), ("grads= reuse", k)


def test_train_step_bf16_split_k_workspaces_distinct(dev):
    """S == zw (= 320 at L = 256) on the one-hot path (P % 32 != 0) with nblk > 1 k-blocks: the
    W0 gradient (H x zw) and the per-shape sums Gs[0] (S x H) share one split-K launch with
    equal slab sizes.  Each must get its own workspace: the loss and EVERY W, b and
    z element-wise within E.TOL of the CPU emulation."""
    from ldm_sdf import autodecoder as AD
    from oracle import ref_autodecoder as A
    case = E.CASE_320xP
    S, P = case[0], case[1]
    lay = _layout(case)
    zw = AD._layout(E.L, E.H, E.SKIP, E.H - E.L - 3, S, P, torch.bfloat16).zw
    assert S == zw == 320 and P % 32 != 0 and lay["nblk"] > 1
    p, z, xyz, sdf, _ = E.inputs(case)
    want_loss, want = E.reference(case)
    loss, got = _step(dev, case, "bf16")
    E.check_against(float(loss), got, want_loss, want, f"bf16 step {E.case_id(case)}")
    loss64 = A.autodecoder_loss(p, z.double(), xyz.double(), sdf.double())
    assert abs(float(loss) - float(loss64)) < 2e-2 * abs(float(loss64))


def test_fit_lowers_loss_on_spheres(dev):
    """4 spheres of different radii, 2048 samples each: 200 bf16 steps of the full loop
    (decoder Adam + latent Adam) cut the clamped-L1 loss by at least 2x, and the trained
    decoder is what the packed decode path then uses."""
    import ldm_sdf
    g = torch.Generator().manual_seed(0)
    radii = torch.tensor([0.3, 0.45, 0.6, 0.75])
    # DeepSDF-style samples: concentrated near the surface (|sdf| mostly inside the band)
    d = torch.randn(4, 2048, 3, generator=g)
    d = d / d.norm(dim=2, keepdim=True)
    r = radii[:, None] + 0.05 * torch.randn(4, 2048, generator=g)
    xyz = (d * r[..., None]).to(dev)
    sdf = xyz.norm(dim=2) - radii[:, None].to(dev)
    dec = ldm_sdf.SDFDecoder(seed=5)
    # He-normal init (the parity-test init) puts |tanh| >> delta everywhere, where the clamp
    # passes no gradient; start from small outputs as DeepSDF's default init does
    dec.weights[8] = dec.weights[8] * 0.01
    st = ldm_sdf.train_autodecoder(dec, xyz, sdf, steps=200, shapes_per_batch=4,
                                   samples_per_shape=1024, lr_decoder=5e-4, lr_latent=1e-3,
                                   dtype="bf16", generator=torch.Generator(device=dev).manual_seed(1))
    first, last = sum(st.losses[:5]) / 5, sum(st.losses[-5:]) / 5
    print("losses", st.losses[::20])
    assert last < 0.5 * first, (first, last)
    assert torch.equal(dec.weights[0], st.masters["W0"].cpu())
    out = ldm_sdf.decode_points(dec, st.latents[:1], xyz[0, :256], dtype="fp32")
    assert torch.isfinite(out).all()


@pytest.mark.parametrize("compute", ["fp32", "bf16"])
def test_linear_mask_r_epilogue(dev, compute):
    """LDM_EPI_MASK_R (the fused ReLU backward of the G W products): Y = R > 0 ? pre : 0."""
    from ldm_sdf import ops, _capi as capi
    cp = capi.COMPUTE_CODES[compute]
    g = torch.Generator().manual_seed(4)
    G = torch.randn(300, 128, generator=g).to(dev)
    W = torch.randn(128, 200, generator=g).to(dev)          # W.T: [200, 128] rows contiguous
    R = torch.randn(300, 200, generator=g).clamp_min(0).to(dev)
    Y = torch.empty(300, 200, device=dev)
    ops.linear(G, W.T, Y, epi=capi.EPI_MASK_R, R=R, compute=cp)
    rd = (lambda t: t.double()) if compute == "fp32" else (lambda t: t.float().bfloat16().double())
    pre = rd(G) @ rd(W)
    want = torch.where(R.double() > 0, pre, torch.zeros_like(pre))
    assert (Y.double() - want).abs().max() < 1e-4
    assert torch.equal(Y[R == 0], torch.zeros_like(Y[R == 0]))
