"""T2 DDPM-side parity on the MI355X: step / q_sample bit-exact vs the fp32 oracle, the fused
linear kernel vs torch, denoiser forward + 20-step sampling trajectory + training gradients
vs the fp64 oracle / goldens."""
import ctypes
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import ldm_sdf
    ldm_sdf.load_library()
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def den():
    from ldm_sdf import MLPDenoiser
    from oracle import ref_cpu as R
    p = R.make_denoiser_params(seed=4321)
    params = {n: getattr(p, n) for n in ("Wt1", "bt1", "Wt2", "bt2", "Win", "bin", "Wout", "bout")}
    for k in range(p.n_blocks):
        params[f"Wblk{k}"] = p.Wblk[k]
        params[f"bblk{k}"] = p.bblk[k]
    return MLPDenoiser(params=params), p


def test_ddpm_step_bit_exact(dev):
    from ldm_sdf import DDPMSchedule, ops
    from oracle import ref_cpu as R
    sch = DDPMSchedule()
    tab = R.ddpm_tables()
    g = torch.Generator().manual_seed(0)
    x, e, z = (torch.randn(8, 256, generator=g) for _ in range(3))
    for t in (0, 1, 500, 999):
        got = ops.ddpm_step(sch.device(dev)["desc"], x.to(dev), e.to(dev), z.to(dev), t).cpu()
        want = R.ddpm_step(tab, x, e, z, t)
        assert torch.equal(got, want), t


def test_q_sample_bit_exact(dev):
    from ldm_sdf import DDPMSchedule, ops
    from oracle import ref_cpu as R
    sch = DDPMSchedule()
    tab = R.ddpm_tables()
    g = torch.Generator().manual_seed(1)
    x0, e = torch.randn(64, 256, generator=g), torch.randn(64, 256, generator=g)
    t = torch.randint(0, 1000, (64,), generator=g, dtype=torch.int32)
    got = ops.q_sample(sch.device(dev)["desc"], x0.to(dev), e.to(dev), t.to(dev)).cpu()
    assert torch.equal(got, R.q_sample(tab, x0, e, t))


@pytest.mark.parametrize("n,off", [(256000, 0), (1001 * 7, 0), (3, 0), (70001, 1)])
def test_loss_and_grad(dev, n, off):
    """Vector path (aligned, n % 4 tail) and scalar path (1-float offset views)."""
    from ldm_sdf import ops
    g = torch.Generator().manual_seed(2)
    a, b = torch.randn(n + off, generator=g), torch.randn(n + off, generator=g)
    a_d, b_d = a.to(dev)[off:], b.to(dev)[off:]
    a, b = a[off:], b[off:]
    loss, grad = ops.eps_mse_loss(a_d, b_d)
    ad = a.double()
    want = ((ad - b.double()) ** 2).mean()
    assert abs(float(loss) - float(want)) / float(want) < 1e-6
    assert torch.allclose(grad.cpu().double(), 2 * (ad - b.double()) / a.numel(), rtol=1e-6,
                          atol=1e-12)


@pytest.mark.parametrize("wdt", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("Bn,M,K,K2", [(1000, 1024, 1024, 0), (37, 100, 70, 0),
                                       (64, 256, 256, 128), (1, 8, 16, 0)])
def test_linear_forward_and_transposes(dev, wdt, Bn, M, K, K2):
    from ldm_sdf import ops, _capi as capi
    g = torch.Generator().manual_seed(Bn + M)
    X = torch.randn(Bn, K, generator=g).to(dev)
    W = torch.randn(M, K, generator=g).to(dev).to(wdt)
    b = torch.randn(M, generator=g).to(dev)
    Y = torch.empty(Bn, M, device=dev)
    kw = {}
    ref = X.double() @ W.double().T + b.double()
    if K2:
        X2 = torch.randn(Bn, K2, generator=g).to(dev)
        W2 = torch.randn(M, K2, generator=g).to(dev).to(wdt)
        kw = dict(X2=X2, W2=W2)
        ref = ref + X2.double() @ W2.double().T
    ops.linear(X, W, Y, bias=b, **kw)
    tol = 1e-5 * (K + K2) ** 0.5
    assert (Y.double() - ref).abs().max() < tol
    # transposed operands (G^T X and G W forms)
    G = torch.randn(Bn, M, generator=g).to(dev)
    dW = torch.empty(M, K, device=dev)
    ops.linear(G.T, X.T, dW)
    assert (dW.double() - G.double().T @ X.double()).abs().max() < 1e-5 * Bn ** 0.5
    dX = torch.empty(Bn, K, device=dev)
    ops.linear(G, W.T, dX)
    assert (dX.double() - G.double() @ W.double()).abs().max() < 1e-5 * M ** 0.5
    # epilogues
    R_ = torch.randn(Bn, M, generator=g).to(dev)
    A = torch.empty(Bn, M, device=dev)
    ops.linear(X, W, Y, epi=capi.EPI_RESID_SILU, bias=b, R=R_, A_out=A, **kw)
    pre = ref
    assert (A.double() - pre).abs().max() < tol
    want = R_.double() + pre * torch.sigmoid(pre)
    assert (Y.double() - want).abs().max() < 2 * tol
    Y0 = torch.randn(Bn, M, generator=g).to(dev)
    Y1 = Y0.clone()
    ops.linear(X, W, Y1, epi=capi.EPI_ACCUM, **kw)
    assert (Y1.double() - (Y0.double() + ref - b.double())).abs().max() < tol


def test_denoiser_forward_vs_golden(dev, den):
    from ldm_sdf import ops
    model, p = den
    g = dict(np.load(os.path.join(GOLD, "sampling_20.npz")))
    pk = model.device_pack("fp32", dev)
    eps = ops.denoiser_fwd_uniform_t(pk["desc"], torch.from_numpy(g["x_T"]).to(dev), 999)
    want = g["eps_t999"]
    err = np.abs(eps.cpu().double().numpy() - want).max()
    assert err < 1e-4 * max(1.0, np.abs(want).max()), err


@pytest.mark.parametrize("use_graph,persistent", [(False, False), (True, False), (False, True)])
def test_sampling_20_steps_vs_golden(dev, den, use_graph, persistent):
    import ldm_sdf
    model, p = den
    g = dict(np.load(os.path.join(GOLD, "sampling_20.npz")))
    steps = int(g["steps"])
    noise = torch.zeros(1000, 4, 256)
    noise[1000 - steps:] = torch.from_numpy(g["noise_tail"])
    x = ldm_sdf.sample(model, ldm_sdf.DDPMSchedule(), 4, steps=steps, dtype="fp32",
                       x_T=torch.from_numpy(g["x_T"]), noise=noise, device=dev,
                       use_graph=use_graph, persistent=persistent)
    want = g["traj"][-1]
    err = np.abs(x.cpu().double().numpy() - want).max()
    assert err < 1e-4, err


def test_sampling_graph_equals_eager_bf16(dev, den):
    import ldm_sdf
    model, _ = den
    gen = torch.Generator().manual_seed(5)
    xT = torch.randn(8, 256, generator=gen)
    noise = torch.randn(1000, 8, 256, generator=gen)
    sch = ldm_sdf.DDPMSchedule()
    a = ldm_sdf.sample(model, sch, 8, steps=50, x_T=xT, noise=noise, device=dev, use_graph=False,
                       persistent=False)
    b = ldm_sdf.sample(model, sch, 8, steps=50, x_T=xT, noise=noise, device=dev, use_graph=True,
                       persistent=False)
    assert torch.equal(a, b)
    assert torch.isfinite(a).all()


@pytest.mark.parametrize("dtype,n,steps,barrier",
                         [("bf16", 8, 1000, "replica"), ("bf16", 1, 40, "replica"),
                          ("bf16", 5, 40, "replica"), ("bf16", 9, 40, "replica"),
                          ("bf16", 13, 40, "replica"), ("bf16", 16, 200, "replica"),
                          ("bf16", 8, 1000, "xcd"), ("bf16", 1, 40, "xcd"), ("bf16", 5, 40, "xcd"),
                          ("bf16", 16, 40, "xcd"), ("fp32", 8, 40, "xcd"), ("fp32", 13, 40, "xcd"),
                          ("bf16", 8, 200, "flat"), ("fp32", 3, 40, "flat")])
def test_sample_loop_persistent_matches_graph(dev, den, dtype, n, steps, barrier, loop_form):
    """The one-launch loop (ldm_sample_loop) is bit-identical to the per-step launches: same
    k-to-lane mapping, fma order, shuffle reduce and epilogues; every barrier completed.  Every
    form is covered: the XCD-replica loop (bf16 default), the chip-wide loop with the
    XCD-hierarchical barrier (fp32 default) and with the flat counter; the form that actually
    ran is asserted (ldm_sample_loop_last_form)."""
    import ldm_sdf
    from ldm_sdf import ops
    loop_form(barrier)
    model, _ = den
    gen = torch.Generator().manual_seed(11 + n)
    xT = torch.randn(n, 256, generator=gen).to(dev)
    noise = torch.randn(1000, n, 256, generator=gen).to(dev)
    sch = ldm_sdf.DDPMSchedule()
    sp = ldm_sdf.Sampler(model, sch, n, steps=steps, dtype=dtype, device=dev, persistent=True)
    sg = ldm_sdf.Sampler(model, sch, n, steps=steps, dtype=dtype, device=dev, persistent=False)
    a = sp.run(xT, noise).clone()
    assert sp.loop.status() == 0
    want_form = barrier if (barrier != "replica" or dtype == "bf16") else "xcd"
    assert ops.sample_loop_last_form() == want_form, (ops.sample_loop_last_form(), want_form)
    b = sg.run(xT, noise).clone()
    assert torch.isfinite(a).all()
    assert torch.equal(a, b), float((a - b).abs().max())
    # replay: the counter/status words are re-zeroed per call, so a second run is identical
    c = sp.run(xT, noise).clone()
    assert sp.loop.status() == 0 and torch.equal(a, c)


@pytest.fixture
def loop_form():
    """Set the persistent loop's form / spin limit through the explicit C call; restore the
    defaults afterwards."""
    from ldm_sdf import ops

    def set_(form="auto", spin_limit=0, tagged=True):
        ops.sample_loop_config(form, spin_limit, tagged)
    yield set_
    ops.sample_loop_config()


def test_sample_loop_rejects_unsupported(dev):
    """Shapes without a persistent kernel: ENOSYS through the C ABI, graph path in Sampler."""
    import ldm_sdf
    small = ldm_sdf.MLPDenoiser(D=64, H=256, n_blocks=2, seed=3)
    sch = ldm_sdf.DDPMSchedule()
    s = ldm_sdf.Sampler(small, sch, 4, steps=3, dtype="bf16", device=dev)
    assert s.loop is None
    with pytest.raises(RuntimeError):
        ldm_sdf.Sampler(small, sch, 4, steps=3, dtype="bf16", device=dev, persistent=True)


def test_train_step_grads_vs_golden(dev, den):
    import ldm_sdf
    model, _ = den
    g = dict(np.load(os.path.join(GOLD, "train_step.npz")))
    model.to_device(dev)
    loss, grads = ldm_sdf.train_step(model, ldm_sdf.DDPMSchedule(),
                                     torch.from_numpy(g["x0"]).to(dev),
                                     torch.from_numpy(g["t"]).to(dev),
                                     torch.from_numpy(g["eps"]).to(dev), dtype="fp32")
    assert abs(float(loss) - float(g["loss"])) / float(g["loss"]) < 1e-5
    for k, v in grads.items():
        want_norm = float(g["gnorm_" + k])
        assert abs(float(v.double().norm()) - want_norm) <= 1e-4 * want_norm + 1e-9, k
        want = g["g_" + k]
        got = v.cpu().double().numpy()
        got = got if k.startswith("b") else got[:8]
        assert np.abs(got - want).max() <= 1e-4 * np.abs(want).max() + 1e-9, k


def _bf(t):
    """The bf16 rounding the matrix-core path applies to an operand (RNE), back in fp64."""
    return t.float().bfloat16().double()


@pytest.mark.parametrize("wdt", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("Bn,M,K,K2", [(1000, 1024, 1024, 1024), (37, 100, 70, 0),
                                       (64, 256, 256, 128), (1, 8, 16, 0), (129, 65, 200, 3)])
def test_linear_bf16_mfma(dev, wdt, Bn, M, K, K2):
    """compute=BF16 (linear_mfma.hip): equals the fp64 product of the bf16-ROUNDED operands up
    to fp32 accumulation, for the forward, G^T X and G W forms and the epilogues."""
    from ldm_sdf import ops, _capi as capi
    BF = capi.COMPUTE_BF16
    g = torch.Generator().manual_seed(Bn * 7 + M)
    X = torch.randn(Bn, K, generator=g).to(dev)
    W = torch.randn(M, K, generator=g).to(dev).to(wdt)
    b = torch.randn(M, generator=g).to(dev)
    Y = torch.empty(Bn, M, device=dev)
    kw = {}
    ref = _bf(X) @ _bf(W).T + b.double()
    if K2:
        X2 = torch.randn(Bn, K2, generator=g).to(dev)
        W2 = torch.randn(M, K2, generator=g).to(dev).to(wdt)
        kw = dict(X2=X2, W2=W2)
        ref = ref + _bf(X2) @ _bf(W2).T
    tol = 2e-6 * (K + K2) ** 0.5 * 4
    ops.linear(X, W, Y, bias=b, compute=BF, **kw)
    assert (Y.double() - ref).abs().max() < tol
    G = torch.randn(Bn, M, generator=g).to(dev)
    dW = torch.empty(M, K, device=dev)
    ops.linear(G.T, X.T, dW, compute=BF)
    assert (dW.double() - _bf(G).T @ _bf(X)).abs().max() < 8e-6 * Bn ** 0.5
    dX = torch.empty(Bn, K, device=dev)
    ops.linear(G, W.T, dX, compute=BF)
    assert (dX.double() - _bf(G) @ _bf(W)).abs().max() < 8e-6 * M ** 0.5
    R_ = torch.randn(Bn, M, generator=g).to(dev)
    A = torch.empty(Bn, M, device=dev)
    ops.linear(X, W, Y, epi=capi.EPI_RESID_SILU, bias=b, R=R_, A_out=A, compute=BF, **kw)
    assert (A.double() - ref).abs().max() < tol
    assert (Y.double() - (R_.double() + ref * torch.sigmoid(ref))).abs().max() < 2 * tol


@pytest.mark.parametrize("wdt", [torch.float32, torch.bfloat16])
def test_linear_bf16_shallow_chunks(dev, wdt):
    """Calls with >= 2048 workgroups run 64-deep LDS chunks (linear_mfma.hip launch_mfma3):
    k-contiguous and rows-contiguous operands (fp32 X, fp32/bf16 W) at that depth, against the
    fp64 product of the bf16-rounded operands."""
    from ldm_sdf import ops, _capi as capi
    BF = capi.COMPUTE_BF16
    Bn, M, K = 131072, 512, 256          # 2048 x 8 tiles
    g = torch.Generator(device=dev).manual_seed(3)
    Z = torch.randn(K, Bn, device=dev, generator=g)          # X = Z.T: rows contiguous
    X = Z.T.contiguous()
    W = torch.randn(M, K, device=dev, generator=g).to(wdt)
    ref = _bf(X) @ _bf(W).T
    tol = 2e-6 * K ** 0.5 * 4
    for Xv in (X, Z.T):
        Y = torch.empty(Bn, M, device=dev)
        ops.linear(Xv, W, Y, compute=BF)
        assert (Y.double() - ref).abs().max() < tol
    # G W with W as a transposed view (rows-contiguous weight operand), 2048 x 4 tiles
    G = torch.randn(Bn, M, device=dev, generator=g)
    dX = torch.empty(Bn, K, device=dev)
    ops.linear(G, W.T, dX, compute=BF)
    assert (dX.double() - _bf(G) @ _bf(W)).abs().max() < 8e-6 * M ** 0.5


@pytest.mark.parametrize("wdt", [torch.float32, torch.bfloat16])
def test_linear_bf16_rank1(dev, wdt):
    """K = 1 goes to the rank-1 kernel: exactly the bf16-rounded product (+ bias, epilogue),
    bit-equal to the fp64 reference since a product of two bf16 values is exact in fp32."""
    from ldm_sdf import ops, _capi as capi
    BF = capi.COMPUTE_BF16
    g = torch.Generator(device=dev).manual_seed(9)
    Bn, M = 70001, 512
    X = torch.randn(Bn, 1, device=dev, generator=g)
    W8 = torch.randn(1, M, device=dev, generator=g).to(wdt)
    R_ = torch.randn(Bn, M, device=dev, generator=g)
    Y = torch.empty(Bn, M, device=dev)
    ops.linear(X, W8.T, Y, epi=capi.EPI_MASK_R, R=R_, compute=BF)
    want = (_bf(X) * _bf(W8)).float() * (R_ > 0)
    assert torch.equal(Y, want)
    b = torch.randn(M, device=dev, generator=g)
    ops.linear(X, W8.T, Y, bias=b, compute=BF)
    assert torch.equal(Y, (_bf(X) * _bf(W8)).float() + b)


@pytest.mark.parametrize("Bn,M,K,epi", [(1, 512, 300001, "bias"), (64, 70, 100003, "relu"),
                                         (130, 64, 50000, "accum")])
def test_linear_bf16_split_k(dev, Bn, M, K, epi):
    """Few output tiles x long K (C19's G^T X over ~1M samples): the split-K path (workspace
    from ldm_linear_workspace_floats, fixed-order slice reduce) against the fp64 product of
    the bf16-rounded operands, through transposed views, with its epilogues."""
    from ldm_sdf import ops, _capi as capi
    BF = capi.COMPUTE_BF16
    g = torch.Generator().manual_seed(K)
    Gt = torch.randn(K, Bn, generator=g).to(dev)          # X = Gt.T: [Bn, K], k-stride Bn
    Xs = torch.randn(K, M, generator=g).to(dev)           # W = Xs.T: [M, K]
    b = torch.randn(M, generator=g).to(dev)
    Y0 = torch.randn(Bn, M, generator=g).to(dev)
    a = capi.LinearArgs()
    a.Bn, a.M, a.K, a.compute = Bn, M, K, BF
    assert capi.load().ldm_linear_workspace_floats(ctypes.byref(a)) > 0   # split engages
    Y = Y0.clone()
    e = {"bias": capi.EPI_BIAS, "relu": capi.EPI_RELU, "accum": capi.EPI_ACCUM}[epi]
    ops.linear(Gt.T, Xs.T, Y, epi=e, bias=b, compute=BF)
    pre = _bf(Gt).T @ _bf(Xs) + b.double()
    want = {"bias": pre, "relu": pre.clamp_min(0), "accum": Y0.double() + pre}[epi]
    assert (Y.double() - want).abs().max() < 2e-6 * K ** 0.5 * 4


def test_train_step_bf16_grads_close_to_fp64(dev, den):
    """Mixed-precision training step (bf16 weights, matrix-core GEMMs) vs the fp64 oracle's
    autograd: loss within 1e-3 relative, every gradient's norm within 2 %, direction cosine
    >= 0.999 (bf16 operand rounding; the fp32 path is pinned to 1e-4 above)."""
    import ldm_sdf
    model, _ = den
    g = dict(np.load(os.path.join(GOLD, "train_step.npz")))
    model.to_device(dev)
    loss, grads = ldm_sdf.train_step(model, ldm_sdf.DDPMSchedule(),
                                     torch.from_numpy(g["x0"]).to(dev),
                                     torch.from_numpy(g["t"]).to(dev),
                                     torch.from_numpy(g["eps"]).to(dev), dtype="bf16")
    assert abs(float(loss) - float(g["loss"])) / float(g["loss"]) < 1e-3
    for k, v in grads.items():
        want_norm = float(g["gnorm_" + k])
        assert abs(float(v.double().norm()) - want_norm) <= 2e-2 * want_norm + 1e-9, k
        want = torch.from_numpy(g["g_" + k]).double().flatten()
        got = v.cpu().double()
        got = (got if k.startswith("b") else got[:8]).flatten()
        cos = float(got @ want / (got.norm() * want.norm() + 1e-30))
        assert cos >= 0.999, (k, cos)


@pytest.mark.parametrize("wd", [0.0, 0.01])
def test_adamw_step_matches_torch(dev, wd):
    """ldm_adamw_step vs torch.optim.AdamW over 5 steps (fp32 masters), and the fused bf16
    working copy equals the updated master rounded to nearest even."""
    from ldm_sdf import ops
    g = torch.Generator(device=dev).manual_seed(4)
    p = torch.randn(1000, 1031, device=dev, generator=g)
    ref = p.clone().requires_grad_(False)
    opt = torch.optim.AdamW([ref], lr=3e-3, weight_decay=wd)
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    low = torch.empty_like(p, dtype=torch.bfloat16)
    for step in range(1, 6):
        grad = torch.randn(p.shape, device=dev, generator=g)
        ref.grad = grad.clone()
        opt.step()
        ops.adamw_step(p, grad, m, v, low, lr=3e-3, weight_decay=wd, step=step)
    torch.cuda.synchronize()
    assert (p - ref).abs().max() <= 2e-6 * ref.abs().max()
    st = opt.state[ref]
    assert (m - st["exp_avg"]).abs().max() <= 1e-6 * st["exp_avg"].abs().max()
    assert (v - st["exp_avg_sq"]).abs().max() <= 1e-6 * st["exp_avg_sq"].abs().max()
    assert torch.equal(low, p.to(torch.bfloat16))


def test_train_fused_adamw_matches_torch_optimizer(dev, den):
    """train() with the fused AdamW (default) tracks the same run driven by torch's AdamW."""
    import ldm_sdf
    from ldm_sdf import MLPDenoiser
    _, p = den
    params = {n: getattr(p, n) for n in ("Wt1", "bt1", "Wt2", "bt2", "Win", "bin", "Wout", "bout")}
    for k in range(p.n_blocks):
        params[f"Wblk{k}"], params[f"bblk{k}"] = p.Wblk[k], p.bblk[k]
    lat = torch.randn(256, 256, generator=torch.Generator().manual_seed(2)).to(dev) * 0.5
    sch = ldm_sdf.DDPMSchedule()
    runs = []
    for use_torch in (False, True):
        model = MLPDenoiser(params={k: v.clone() for k, v in params.items()})
        model.to_device(dev)
        st = None
        if use_torch:
            st = ldm_sdf.api.TrainState()
            st.masters = {n: model.params[n] for n in model.names()}
            st.optimizer = torch.optim.AdamW(list(st.masters.values()), lr=1e-4, weight_decay=0.0)
        st = ldm_sdf.train(model, sch, lat, steps=5, batch=256, dtype="fp32", state=st,
                           generator=torch.Generator(device=dev).manual_seed(8))
        runs.append((st.losses, {n: t.clone() for n, t in model.params.items()}))
    (la, pa), (lb, pb) = runs
    assert max(abs(a - b) for a, b in zip(la, lb)) <= 1e-5 * max(lb)
    for n in pa:
        assert (pa[n] - pb[n]).abs().max() <= 1e-5 * pb[n].abs().max() + 1e-7, n



# ---- the benched bf16 sampler pinned to the oracle (VERDICT r1 "next" #1) -----------------
def _bf16_rounded_params(p):
    """The oracle's parameters as the bf16 sampling path holds them: every weight matrix
    rounded to bf16 (RNE), biases fp32; arithmetic stays fp64 in the oracle (the GPU path
    computes in fp32 with these weights, E tables included)."""
    from oracle import ref_cpu as R
    bw = lambda w: w.float().bfloat16().double()
    bb = lambda b: b.float().double()
    return R.DenoiserParams(p.D, p.H, p.n_blocks, p.TE, bw(p.Wt1), bb(p.bt1), bw(p.Wt2),
                            bb(p.bt2), bw(p.Win), bb(p.bin), [bw(w) for w in p.Wblk],
                            [bb(b) for b in p.bblk], bw(p.Wout), bb(p.bout))


def _oracle_sample(p, xT, noise, steps):
    from oracle import ref_cpu as R
    emb = torch.from_numpy(R.timestep_embedding_table(1000, 128)).double()
    return R.sample_loop(p, R.ddpm_tables(), emb, xT.double(), noise.double(), steps=steps)


_PATHS = {"eager": dict(use_graph=False, persistent=False),
          "graph": dict(use_graph=True, persistent=False),
          "persistent": dict(use_graph=False, persistent=True)}


@pytest.mark.parametrize("path", list(_PATHS))
def test_sampling_bf16_20_steps_vs_oracle_rounded(dev, den, path):
    """bf16 sampling (ldm_sample_step eager / hipGraph / ldm_sample_loop) on the 20-step golden
    inputs vs the fp64 oracle run on the bf16-ROUNDED weights: |diff| <= 1e-4 (fp32 arithmetic
    only; the oracle's own fp32 run differs from fp64 by 1.2e-6 here)."""
    import ldm_sdf
    model, p = den
    g = dict(np.load(os.path.join(GOLD, "sampling_20.npz")))
    steps = int(g["steps"])
    xT = torch.from_numpy(g["x_T"])
    noise = torch.zeros(1000, xT.shape[0], 256)
    noise[1000 - steps:] = torch.from_numpy(g["noise_tail"])
    x = ldm_sdf.sample(model, ldm_sdf.DDPMSchedule(), xT.shape[0], steps=steps, dtype="bf16",
                       x_T=xT, noise=noise, device=dev, **_PATHS[path]).cpu().double()
    want = _oracle_sample(_bf16_rounded_params(p), xT, noise, steps)
    err = float((x - want).abs().max())
    print(f"bf16 {path} 20 steps vs rounded-weight oracle: max abs {err:.3e}")
    assert err <= 1e-4, err
    # loose: against the UNROUNDED weights the bf16 weight rounding itself shows (5.1e-3 on CPU)
    loose = float((x - _oracle_sample(p, xT, noise, steps)).abs().max())
    print(f"bf16 {path} 20 steps vs unrounded oracle: max abs {loose:.3e}")
    assert loose <= 2e-2, loose


@pytest.mark.parametrize("path", ["graph", "persistent"])
def test_sampling_bf16_1000_steps_b8_vs_oracle_rounded(dev, den, path):
    """The bench configuration (B = 8, T = 1000, bf16) against the fp64 oracle on bf16-rounded
    weights.  The synthetic (untrained) denoiser makes x grow to ~1e8 over 1000 steps, so the
    bound is relative to max|x|: <= 2e-5 (the oracle's own fp32 run: 8e-7).  Against unrounded
    weights the relative difference is the weight rounding's (~9e-3 on CPU): <= 5e-2."""
    import ldm_sdf
    model, p = den
    gen = torch.Generator().manual_seed(5)
    xT = torch.randn(8, 256, generator=gen)
    noise = torch.randn(1000, 8, 256, generator=gen)
    x = ldm_sdf.sample(model, ldm_sdf.DDPMSchedule(), 8, steps=1000, dtype="bf16", x_T=xT,
                       noise=noise, device=dev, **_PATHS[path]).cpu().double()
    want = _oracle_sample(_bf16_rounded_params(p), xT, noise, 1000)
    scale = float(want.abs().max())
    rel = float((x - want).abs().max()) / scale
    print(f"bf16 {path} 1000 steps B=8: max|x| {scale:.3e}, rel err vs rounded {rel:.3e}")
    assert rel <= 2e-5, rel
    loose = float((x - _oracle_sample(p, xT, noise, 1000)).abs().max()) / scale
    print(f"bf16 {path} 1000 steps B=8: rel err vs unrounded {loose:.3e}")
    assert loose <= 5e-2, loose


# ---- the per-step GEMV away from D = 256 / H = 1024 ----------------------------------------
# (D, H) -> batches.  K = 1032: 4 chunks per lane, one live lane in chunk 2, none in chunk 3;
# K = 520: 2 chunks, one live lane in chunk 1; K = 8: a single live lane; K = 2048: 4 chunks,
# every lane live, with M = 8.  B = 8 | 9 straddle the 8- and 16-sample kernels; 15 (H = 1032)
# and 8 (D = 2048) are the largest the 64 KiB LDS check admits.
_GEMV_SHAPES = {(8, 1032): (1, 8, 9, 15), (8, 520): (1, 8, 9, 15), (2048, 8): (1, 8)}
_gemv_nets = {}


def _gemv_net(D, H):
    """(model, fp64 oracle parameters) of a one-block network, built once per shape."""
    from ldm_sdf import MLPDenoiser
    from oracle import ref_cpu as R
    if (D, H) not in _gemv_nets:
        p = R.make_denoiser_params(D, H, n_blocks=1, TE=64, seed=7)
        params = {n: getattr(p, n) for n in ("Wt1", "bt1", "Wt2", "bt2", "Win", "bin", "Wout",
                                             "bout")}
        params["Wblk0"], params["bblk0"] = p.Wblk[0], p.bblk[0]
        _gemv_nets[(D, H)] = MLPDenoiser(D, H, n_blocks=1, TE=64, params=params), p
    return _gemv_nets[(D, H)]


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("D,H,B", [(D, H, B) for (D, H), Bs in _GEMV_SHAPES.items() for B in Bs])
def test_per_step_gemv_shapes_vs_oracle(dev, D, H, B, dtype):
    """ldm_denoiser_fwd_uniform_t (t = 999) and ldm_sample_step (t = 999 and the no-noise t = 0)
    at the chunk counts and partial chunks the D = 256 / H = 1024 tests never reach, against
    the fp64 oracle (for bf16: on the bf16-rounded weight matrices, biases unrounded) within
    test_denoiser_forward_vs_golden's bound 1e-4 max(1, max|want|).  The oracle's own fp32 run
    is 0.2-1.3e-6 from fp64 on these inputs (max|want| 1.7-5.2): two orders of margin over any
    summation order."""
    from ldm_sdf import DDPMSchedule, ops
    from oracle import ref_cpu as R
    model, p = _gemv_net(D, H)
    ref = p if dtype == "fp32" else _bf16_rounded_params(p)
    desc = model.device_pack(dtype, dev)["desc"]
    sch = DDPMSchedule()            # owns the device tables the descriptor points at
    sdesc = sch.device(dev)["desc"]
    tab = R.ddpm_tables()
    emb = torch.from_numpy(R.timestep_embedding_table(1000, 64)).double()
    g = torch.Generator().manual_seed(1000 * D + B)
    x, z = torch.randn(B, D, generator=g), torch.randn(B, D, generator=g)
    x_d, z_d = x.to(dev), z.to(dev)
    ws = torch.empty(2 * B * H, device=dev)

    def check(what, got, want):
        err = float((got.cpu().double() - want).abs().max())
        bound = 1e-4 * max(1.0, float(want.abs().max()))
        print(f"gemv D={D} H={H} B={B} {dtype} {what}: max|want| {float(want.abs().max()):.3f} "
              f"err {err:.3e} bound {bound:.3e}")
        assert err < bound, (what, err, bound)

    for t in (999, 0):
        eps = R.denoiser_forward(ref, x.double(), torch.full((B,), t), emb)
        if t == 999:
            check("fwd t=999", ops.denoiser_fwd_uniform_t(desc, x_d, t), eps)
        out = torch.empty_like(x_d)
        ops.sample_step(desc, sdesc, x_d, z_d, t, out, ws)
        check(f"step t={t}", out, R.ddpm_step(tab, x.double(), eps, z.double(), t))


def test_sample_loop_timeout_surfaces_and_falls_back(dev, den, loop_form):
    """A persistent-loop barrier that gives up must not hand back partial latents silently:
    with a 1-poll spin limit the loop reports status 1, Sampler.run warns, re-runs the sample
    on the per-step path and returns that path's (bit-identical) result."""
    import ldm_sdf
    model, _ = den
    gen = torch.Generator().manual_seed(21)
    xT = torch.randn(8, 256, generator=gen).to(dev)
    noise = torch.randn(1000, 8, 256, generator=gen).to(dev)
    sch = ldm_sdf.DDPMSchedule()
    ref = ldm_sdf.Sampler(model, sch, 8, steps=40, dtype="bf16", device=dev,
                          persistent=False).run(xT, noise).clone()
    loop_form("auto", spin_limit=1)
    sp = ldm_sdf.Sampler(model, sch, 8, steps=40, dtype="bf16", device=dev, persistent=True)
    sp.run(xT, noise, check=False)
    assert sp.loop.status() == 1
    with pytest.warns(RuntimeWarning):
        got = sp.run(xT, noise).clone()
    assert sp.loop_fallbacks == 1
    assert torch.equal(got, ref)
    loop_form()
    assert torch.equal(sp.run(xT, noise), ref) and sp.loop_fallbacks == 1


@pytest.mark.parametrize("persistent", [False, True])
def test_sampler_repacks_after_training(dev, den, persistent):
    """A Sampler built (and its graph captured) BEFORE train() must sample with the trained
    weights AND their rebuilt E tables afterwards (the graph had baked the old
    table addresses in): its result equals a fresh Sampler's, bit for bit."""
    import ldm_sdf
    from ldm_sdf import MLPDenoiser
    _, p = den
    params = {n: getattr(p, n) for n in ("Wt1", "bt1", "Wt2", "bt2", "Win", "bin", "Wout", "bout")}
    for k in range(p.n_blocks):
        params[f"Wblk{k}"], params[f"bblk{k}"] = p.Wblk[k], p.bblk[k]
    model = MLPDenoiser(params={k: v.clone() for k, v in params.items()})
    model.to_device(dev)
    sch = ldm_sdf.DDPMSchedule()
    gen = torch.Generator().manual_seed(31)
    xT = torch.randn(8, 256, generator=gen).to(dev)
    noise = torch.randn(1000, 8, 256, generator=gen).to(dev)
    kw = dict(steps=30, dtype="bf16", device=dev, persistent=persistent)
    old = ldm_sdf.Sampler(model, sch, 8, **kw)
    before = old.run(xT, noise).clone()
    lat = torch.randn(256, 256, generator=torch.Generator().manual_seed(3)).to(dev) * 0.5
    ldm_sdf.train(model, sch, lat, steps=20, batch=256, lr=1e-3, dtype="bf16",
                  generator=torch.Generator(device=dev).manual_seed(4))
    after = old.run(xT, noise).clone()
    fresh = ldm_sdf.Sampler(model, sch, 8, **kw).run(xT, noise).clone()
    assert not torch.equal(before, fresh)          # training changed the network
    assert torch.equal(after, fresh), float((after - fresh).abs().max())


def test_stale_stepper_fails_loudly_and_its_graph_stays_valid(dev, den):
    """a stepper made (and a graph captured from it) OUTSIDE Sampler, then two
    train() calls: calling the stale stepper raises LdmError, and the graph, replayed, still
    reads the tables its stepper holds (the same numbers as before training, no freed memory)."""
    import ldm_sdf
    from ldm_sdf import LdmError, MLPDenoiser
    _, p = den
    params = {n: getattr(p, n) for n in ("Wt1", "bt1", "Wt2", "bt2", "Win", "bin", "Wout", "bout")}
    for k in range(p.n_blocks):
        params[f"Wblk{k}"], params[f"bblk{k}"] = p.Wblk[k], p.bblk[k]
    model = MLPDenoiser(params={k: v.clone() for k, v in params.items()})
    model.to_device(dev)
    sch = ldm_sdf.DDPMSchedule()
    sd = sch.device(dev)["desc"]
    x = torch.randn(4, 256, generator=torch.Generator().manual_seed(5)).to(dev)
    z = torch.zeros_like(x)
    y = torch.empty_like(x)
    step = model.make_stepper(4, "bf16", dev, sd)
    step(x, z, 500, y)
    ref = y.clone()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        step(x, z, 500, y)
    lat = torch.randn(256, 256, generator=torch.Generator().manual_seed(3)).to(dev) * 0.5
    for _ in range(2):
        ldm_sdf.train(model, sch, lat, steps=3, batch=256, lr=1e-3, dtype="bf16")
        ldm_sdf.Sampler(model, sch, 4, steps=2, dtype="bf16", device=dev,
                        persistent=False).run(x, torch.zeros(1000, 4, 256, device=dev))
    with pytest.raises(LdmError):
        step(x, z, 500, y)
    y.zero_()
    g.replay()
    torch.cuda.synchronize()
    # the weights' bf16 working copies are updated in place by AdamW (same addresses), so the
    # replay reads the trained weights with the OLD (retained) E tables: finite, and not the
    # pre-training result
    assert bool(torch.isfinite(y).all()) and not torch.equal(y, ref)


# ---- 1000 steps in a bounded regime (VERDICT r2 "next" #2) ---------------------------------
def bounded_denoiser_params(p):
    """The test denoiser with identity in/out projections (W_in = [I; 0], W_out = [I, 0], zero
    in/out biases) and its four residual blocks and time MLP unchanged.  eps_hat = x + blocks(x,
    t): the identity part is the optimal denoiser of a point mass at 0 up to its 1/sqrt(1-ab_t)
    scale, which makes every reverse step a contraction (c1 (1 - c2) <= sqrt(1 - beta_t) < 1),
    so x stays O(1) for all 1000 steps (max|x| ~1.7 on CPU) while the blocks still move the
    result by O(1) (0.68 max abs vs blocks zeroed): an absolute bound is meaningful."""
    import dataclasses
    D, H = p.D, p.H
    Win = torch.zeros(H, D, dtype=p.Win.dtype)
    Win[:D] = torch.eye(D, dtype=p.Win.dtype)
    Wout = torch.zeros(D, H, dtype=p.Wout.dtype)
    Wout[:, :D] = torch.eye(D, dtype=p.Wout.dtype)
    return dataclasses.replace(p, Win=Win, Wout=Wout, bin=torch.zeros_like(p.bin),
                               bout=torch.zeros_like(p.bout))


def _denoiser_from(p):
    from ldm_sdf import MLPDenoiser
    params = {n: getattr(p, n) for n in ("Wt1", "bt1", "Wt2", "bt2", "Win", "bin", "Wout", "bout")}
    for k in range(p.n_blocks):
        params[f"Wblk{k}"], params[f"bblk{k}"] = p.Wblk[k], p.bblk[k]
    return MLPDenoiser(params={k: v.float() for k, v in params.items()})


BOUNDED_ABS = 1e-4


@pytest.mark.parametrize("n", [8, 13])
@pytest.mark.parametrize("path", ["graph", "persistent"])
def test_sampling_bf16_1000_steps_bounded_vs_oracle(dev, den, loop_form, n, path):
    """The benched sampler (bf16, T = 1000) in a regime where x stays O(1): the default
    XCD-replica loop (asserted) and the hipGraph path against the fp64 oracle on the
    bf16-ROUNDED weights, with an ABSOLUTE per-element bound (BOUNDED_ABS) at T = 1000."""
    import ldm_sdf
    from ldm_sdf import ops
    _, p = den
    q = bounded_denoiser_params(p)
    model = _denoiser_from(q)
    loop_form("auto")
    gen = torch.Generator().manual_seed(77 + n)
    xT = torch.randn(n, 256, generator=gen)
    noise = torch.randn(1000, n, 256, generator=gen)
    x = ldm_sdf.sample(model, ldm_sdf.DDPMSchedule(), n, dtype="bf16", x_T=xT, noise=noise,
                       device=dev, **_PATHS[path]).cpu().double()
    if path == "persistent":
        assert ops.sample_loop_last_form() == "replica"
    want = _oracle_sample(_bf16_rounded_params(q), xT, noise, 1000)
    scale = float(want.abs().max())
    err = float((x - want).abs().max())
    print(f"bounded bf16 {path} T=1000 B={n}: max|x| {scale:.3f}, max abs err {err:.3e}")
    assert 0.2 < scale < 10.0, scale             # the regime really is bounded
    assert err <= BOUNDED_ABS, err


def test_config3_bounded_sample8_then_decode128_unscaled(dev, den):
    """Config 3 on bounded latents: sample(8) through the default loop, then the 128^3 decode
    of those latents AS SAMPLED (no rescaling; ~5x the synthetic-latent scale) with the
    default dtype="auto", which must pick fp16 here (the bf16 rounding error grows with the
    latents' scale and leaves SURVEY §8(c)'s 1e-2 beyond RMS ~0.4: api.BF16_MAX_LATENT_RMS).
    600 random points per shape against (a) the fp64 decoder at the fp16 contract of §8(c),
    2e-3, and (b) the oracle at the fp16 precision contract (decoder_forward_lowp: fp16
    operands, fp64 sums): median within 2e-5 (fp32 summation order), max within the same
    2e-3.  The SDFs are not saturated."""
    import ldm_sdf
    from oracle import ref_cpu as R
    _, p = den
    q = bounded_denoiser_params(p)
    model = _denoiser_from(q)
    gen = torch.Generator().manual_seed(99)
    xT = torch.randn(8, 256, generator=gen)
    noise = torch.randn(1000, 8, 256, generator=gen)
    lat = ldm_sdf.sample(model, ldm_sdf.DDPMSchedule(), 8, dtype="bf16", x_T=xT, noise=noise,
                         device=dev)
    want_lat = _oracle_sample(_bf16_rounded_params(q), xT, noise, 1000)
    assert float((lat.cpu().double() - want_lat).abs().max()) <= BOUNDED_ABS
    rms = float(lat.pow(2).mean(dim=1).sqrt().max())
    assert ldm_sdf.resolve_decode_dtype("auto", lat) == "fp16", rms
    pd = R.make_decoder_params(seed=1234)
    dec = ldm_sdf.SDFDecoder(256, weights=pd.weights, biases=pd.biases)
    N = 128
    vol = ldm_sdf.decode(dec, lat, N)
    assert vol.shape == (8, N, N, N) and bool(torch.isfinite(vol).all())
    assert float((vol.abs() < 0.99).float().mean()) > 0.05     # not saturated at +-1
    grid = torch.from_numpy(R.grid_coords_np(N)).double()
    idx = torch.randint(0, N ** 3, (8, 600), generator=gen)
    got = vol.reshape(8, -1)[torch.arange(8)[:, None], idx.to(dev)].cpu().double()
    zc = lat.cpu().double()
    for b in range(8):
        lowp = R.decoder_forward_lowp(pd, zc[b:b + 1], grid[idx[b]], torch.float16)[0]
        full = R.decoder_forward(pd, zc[b:b + 1], grid[idx[b]])[0]
        e_lo = float((got[b] - lowp).abs().max())
        e_64 = float((got[b] - full).abs().max())
        m_lo = float((got[b] - lowp).abs().median())
        print(f"config3 bounded shape {b} (latent RMS max {rms:.3f}, fp16): vs fp16-contract "
              f"oracle {e_lo:.2e} (median {m_lo:.1e}), vs fp64 {e_64:.2e}")
        assert m_lo <= 2e-5, (b, m_lo)
        assert e_lo <= 2e-3, (b, e_lo)
        assert e_64 <= 2e-3, (b, e_64)
