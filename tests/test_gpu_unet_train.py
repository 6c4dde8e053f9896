"""UNet training on the MI355X: ldm_conv1d_bwd_data / ldm_conv1d_bwd_weight against
fp64 autograd of a torch conv on the forward's own test geometries, the whole-network gradients
of api.train_step against fp64 autograd of the oracle (oracle/ref_unet.py), and api.train against
an fp64 torch.optim.AdamW loop over the oracle.

Bounds (from the issue that introduced the feature; none is derived from the code under test):
  conv gradients: max|err| <= 1e-5 max(1, max|ref|) -- the fp32 conv bound of test_gpu_unet.py;
    the contraction Cout K here is <= 384, below the forward's 1536; the weight-gradient dY is
    scaled by 1 / (B L_out) as the loss does, so its sums are O(1) too;
  network gradients: per tensor max|g - g_ref| <= 1e-4 max|g_ref|, loss 1e-5 relative -- the UNet
    forward bound, ~50x the fp32 floor of the reference (tests/test_unet_train_host.py);
  training: every loss within 1e-4 relative, final parameters within 1e-4 max|p|.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import unet_train_ref as ref

pytestmark = pytest.mark.gpu

TINY = [(64, (16, 32, 48), 16, 32, 50, 3), (72, (8, 24, 40), 16, 32, 50, 5)]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import ldm_sdf
    ldm_sdf.load_library()
    return torch.device("cuda", 0)


# the segment geometries of tests/test_gpu_unet.py::CASES (a copy: that file stays as it is)
CASES = [
    # name, B, [(Cin, L_in, ksize, stride, mode, silu)], Cout
    ("k3s1", 3, [(16, 100, 3, 1, 0, False)], 32),
    ("k3s1_silu_cb_res", 2, [(40, 130, 3, 1, 0, True)], 40),
    ("k3s2", 2, [(33, 257, 3, 2, 0, False)], 70),
    ("up2", 2, [(64, 37, 3, 1, 1, False)], 20),
    ("concat", 2, [(32, 64, 3, 1, 0, True), (20, 64, 3, 1, 0, True)], 24),
    # 40 x 4 = 160 contraction units: all 64 slices of the weight gradient, 2-3 units each
    ("big_b_tile64", 40, [(64, 256, 3, 1, 0, True)], 64),
    ("k3_plus_1x1", 2, [(32, 64, 3, 1, 0, True), (16, 64, 1, 1, 0, False),
                        (16, 64, 1, 1, 0, False)], 32),
    ("k4s2", 2, [(8, 130, 4, 2, 0, False)], 5),
    ("cin1_cout1", 5, [(1, 1024, 3, 1, 0, False)], 1),
    ("up2_direct", 2, [(64, 64, 3, 1, 1, True)], 32),
    ("k3s2_direct", 2, [(32, 128, 3, 2, 0, True)], 48),
    ("k4s2_direct", 3, [(16, 128, 4, 2, 0, False)], 16),
    ("concat_up2_direct", 2, [(64, 32, 3, 1, 1, True), (32, 32, 3, 1, 1, True)], 24),
    ("four_seg_generic", 2, [(32, 64, 3, 1, 0, True), (16, 64, 3, 1, 0, True),
                            (16, 64, 1, 1, 0, False), (64, 64, 1, 1, 0, False)], 32),
    ("c128_tile32_direct", 16, [(128, 128, 3, 1, 0, True)], 128),
]


def _conv_seg(x, w, K, stride, mode, silu):
    """One segment of the forward in torch (x, w any dtype): act, upsample, conv."""
    if silu:
        x = x * torch.sigmoid(x)
    if mode == 1:
        x = F.interpolate(x, scale_factor=2, mode="nearest")
    return F.conv1d(x, w, stride=stride, padding=0 if K == 1 else 1)


def _case_operands(case, wdt):
    """Inputs, one weight per kernel size (segments of one ksize are column blocks of it) and
    the channel offsets, from the case's own seed."""
    name, B, segs, Cout = case
    g = torch.Generator().manual_seed(sum(map(ord, name)))
    tdt = {"fp32": torch.float32, "bf16": torch.bfloat16}[wdt]
    Xs = [torch.randn(B, Cin, L_in, generator=g) for (Cin, L_in, *_r) in segs]
    Ws, offs, c_off = {}, [], {}
    for K in sorted({s[2] for s in segs}):
        Ctot = sum(s[0] for s in segs if s[2] == K)
        Ws[K] = (torch.randn(Cout, Ctot, K, generator=g) / np.sqrt(Ctot * K)).to(tdt)
        c_off[K] = 0
    for (Cin, L_in, K, *_r) in segs:
        offs.append(c_off[K])
        c_off[K] += Cin
    L_out = _conv_seg(Xs[0][:1], Ws[segs[0][2]][:, :segs[0][0]].float(), segs[0][2],
                      segs[0][3], segs[0][4], False).shape[2]
    dY = torch.randn(B, Cout, L_out, generator=g)
    return Xs, Ws, offs, dY, g


@pytest.mark.parametrize("wdt", ["fp32", "bf16"])
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_conv1d_bwd_data_vs_autograd(dev, case, wdt):
    """Every segment on its own, accumulate off and on (on: onto a random dX)."""
    from ldm_sdf import ops
    name, B, segs, Cout = case
    Xs, Ws, offs, dY, g = _case_operands(case, wdt)
    dYd = dY.to(dev)
    for X, (Cin, L_in, K, st, mode, silu), off in zip(Xs, segs, offs):
        x = X.double().requires_grad_(True)
        w = Ws[K].float().double()[:, off:off + Cin]       # bf16: the same rounded weights
        (_conv_seg(x, w, K, st, mode, silu) * dY.double()).sum().backward()
        want = x.grad
        bound = 1e-5 * max(1.0, float(want.abs().max()))
        seg = ops.ConvSegment(X.to(dev), ops.pack_conv_weight(Ws[K].to(dev)), c_off=off,
                              stride=st, mode=mode, silu=silu, pad=0 if K == 1 else 1)
        dX = torch.full((B, Cin, L_in), float("nan"), device=dev)
        ops.conv1d_bwd_data(seg, dYd, dX)
        err = float((dX.cpu().double() - want).abs().max())
        print(f"{name} {wdt} C={Cin} k={K} s={st} mode={mode}: err {err:.2e} (bound {bound:.2e})")
        assert err <= bound, (name, wdt, "store", err)
        base = torch.randn(B, Cin, L_in, generator=g)
        dX2 = base.to(dev)
        ops.conv1d_bwd_data(seg, dYd, dX2, accumulate=True)
        err = float((dX2.cpu().double() - (base.double() + want)).abs().max())
        assert err <= 1e-5 * max(1.0, float((base.double() + want).abs().max())), \
            (name, wdt, "accumulate", err)


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_conv1d_bwd_weight_vs_autograd(dev, case):
    """Whole convs (every segment, one dY scaled as the loss scales it): packed dW per weight,
    dbias, dcbias; zero padding; a second run is bitwise the first."""
    from ldm_sdf import ops
    name, B, segs, Cout = case
    Xs, Ws, offs, dY, _ = _case_operands(case, "fp32")
    dY = dY / (B * dY.shape[2])
    W64 = {K: W.double().requires_grad_(True) for K, W in Ws.items()}
    y = None
    for X, (Cin, L_in, K, st, mode, silu), off in zip(Xs, segs, offs):
        r = _conv_seg(X.double(), W64[K][:, off:off + Cin], K, st, mode, silu)
        y = r if y is None else y + r
    (y * dY.double()).sum().backward()
    dYd = dY.to(dev)
    packs = {K: ops.pack_conv_weight(W.to(dev)) for K, W in Ws.items()}
    dsegs = [ops.ConvSegment(X.to(dev), packs[K], c_off=off, stride=st, mode=mode, silu=silu,
                             pad=0 if K == 1 else 1)
             for X, (Cin, L_in, K, st, mode, silu), off in zip(Xs, segs, offs)]

    def run():
        dW = {K: torch.full_like(p, float("nan")) for K, p in packs.items()}
        db = torch.full((Cout,), float("nan"), device=dev)
        dcb = torch.full((B, Cout), float("nan"), device=dev)
        ops.conv1d_bwd_weight(dsegs, dYd, [dW[s.ksize] for s in dsegs], dbias=db, dcbias=dcb)
        return dW, db, dcb

    dW, db, dcb = run()
    for K, W in Ws.items():
        want = W64[K].grad
        got = ops.unpack_conv_weight(dW[K], Cout, W.shape[1]).cpu().double()
        err = float((got - want).abs().max())
        bound = 1e-5 * max(1.0, float(want.abs().max()))
        print(f"{name} k={K}: dW err {err:.2e} (max|ref| {float(want.abs().max()):.2e})")
        assert err <= bound, (name, K, err)
        # the padding is exactly zero: re-packing the unpadded part gives the same tensor
        assert torch.equal(ops.pack_conv_weight(ops.unpack_conv_weight(dW[K], Cout, W.shape[1])),
                           dW[K]), (name, K, "padding")
        assert float(dW[K][Cout:].abs().sum()) == 0
    want_cb = dY.double().sum(2)
    assert float((dcb.cpu().double() - want_cb).abs().max()) <= \
        1e-5 * max(1.0, float(want_cb.abs().max()))
    want_b = dY.double().sum((0, 2))
    assert float((db.cpu().double() - want_b).abs().max()) <= \
        1e-5 * max(1.0, float(want_b.abs().max()))
    # dbias alone (the per-shape sums go to the workspace)
    db2 = torch.full((Cout,), float("nan"), device=dev)
    ops.conv1d_bwd_weight(dsegs, dYd, [torch.empty_like(packs[s.ksize]) for s in dsegs], dbias=db2)
    assert torch.equal(db2, db)
    dW2, db3, dcb2 = run()
    assert all(torch.equal(dW[K], dW2[K]) for K in dW) and torch.equal(db, db3) and \
        torch.equal(dcb, dcb2)


def _check_grads(grads, loss, want, want_loss, tag):
    worst = 0.0
    for n, gr in want.items():
        got = grads[n].cpu().double()
        assert got.shape == gr.shape, (n, got.shape, gr.shape)
        rel = float((got - gr).abs().max() / gr.abs().max())
        worst = max(worst, rel)
        assert rel <= 1e-4, (tag, n, rel)
    lrel = abs(float(loss) - want_loss) / abs(want_loss)
    print(f"{tag}: worst per-tensor max|dg|/max|g| {worst:.2e}, loss rel {lrel:.2e}")
    assert lrel <= 1e-5, (tag, lrel)


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("net", TINY, ids=["D64", "D72"])
def test_train_step_gradients_tiny(dev, net, dtype):
    """C = (8, 24, 40): every level ragged against 16; D = 72: L = 18 at the bottom; mixed t
    with 0 and T - 1.  bf16 against the oracle on bf16-rounded conv and linear weights."""
    import ldm_sdf
    D, Cc, TE, HT, T, B = net
    want, want_loss = ref.oracle_grads(D, Cc, TE, HT, T, B, torch.float64, dtype == "bf16")
    m = ldm_sdf.UNet1DDenoiser(D=D, C=Cc, TE=TE, HT=HT, T=T, seed=2468)
    x0, t, eps = ref.make_inputs(D, T, B)
    loss, grads = ldm_sdf.train_step(m, ldm_sdf.DDPMSchedule(T=T), x0.to(dev), t.to(dev),
                                     eps.to(dev), dtype=dtype)
    assert sorted(grads) == sorted(m.params) and loss.shape == (1,)
    _check_grads(grads, loss, want, want_loss, f"D{D} {dtype}")


def test_train_step_gradients_full_size(dev):
    """One step of config 5's network (D = 1024, C = (32, 64, 128)) at B = 2."""
    import ldm_sdf
    D, Cc, TE, HT, T, B = 1024, (32, 64, 128), 128, 512, 1000, 2
    want, want_loss = ref.oracle_grads(D, Cc, TE, HT, T, B, torch.float64, False)
    m = ldm_sdf.UNet1DDenoiser(seed=2468)
    x0, t, eps = ref.make_inputs(D, T, B)
    loss, grads = ldm_sdf.train_step(m, ldm_sdf.DDPMSchedule(), x0.to(dev), t.to(dev),
                                     eps.to(dev), dtype="fp32")
    _check_grads(grads, loss, want, want_loss, "full size fp32")


NET = TINY[0][:5]          # the training tests' net: D, C, TE, HT, T
M_LAT, BATCH = 16, 8


def _latents():
    return torch.randn(M_LAT, NET[0], generator=torch.Generator().manual_seed(9)) * 0.5


def _draws(seed, steps):
    """The draws train() makes from a CPU generator, in its order: per step the batch indices,
    t, eps."""
    D, _, _, _, T = NET
    g = torch.Generator().manual_seed(seed)
    out = []
    for _ in range(steps):
        idx = torch.randint(0, M_LAT, (1, BATCH), generator=g)
        t = torch.randint(0, T, (1, BATCH), generator=g, dtype=torch.int32)
        eps = torch.randn(1, BATCH, D, generator=g)
        out.append((idx[0], t[0].long(), eps[0]))
    return out


def _train(dev, steps, dtype="fp32", seed=31, state=None, model=None, gen=None):
    import ldm_sdf
    D, Cc, TE, HT, T = NET
    m = model or ldm_sdf.UNet1DDenoiser(D=D, C=Cc, TE=TE, HT=HT, T=T, seed=2468)
    g = gen or torch.Generator().manual_seed(seed)
    st = ldm_sdf.train(m, ldm_sdf.DDPMSchedule(T=T), _latents().to(dev), steps=steps, batch=BATCH,
                       lr=1e-3, weight_decay=0.01, dtype=dtype, generator=g, state=state)
    return m, st, g


def test_train_fp32_vs_oracle_adamw(dev):
    """20 AdamW steps against fp64 torch.optim.AdamW over the oracle forward on the same draws;
    then the trained denoiser's forward and a 5-step sample() against the oracle ON THE TRAINED
    PARAMETERS (stale packs or E tables fail here)."""
    import ldm_sdf
    from oracle import ref_cpu as R
    from oracle import ref_unet as U
    D, Cc, TE, HT, T = NET
    steps = 20
    up = ref.oracle_params(D, Cc, TE, HT, 2468)
    for v in up.p.values():
        v.requires_grad_(True)
    opt = torch.optim.AdamW(list(up.p.values()), lr=1e-3, weight_decay=0.01)
    tab = R.ddpm_tables(T)
    emb = torch.from_numpy(R.timestep_embedding_table(T, TE)).double()
    lat = _latents()
    want_losses = []
    for idx, t, eps in _draws(31, steps):
        opt.zero_grad()
        loss = ref.oracle_loss(up, tab, emb, lat[idx], t, eps)
        loss.backward()
        opt.step()
        want_losses.append(float(loss.detach()))
    m, st, _ = _train(dev, steps)
    assert st.step == steps and len(st.losses) == steps
    for i, (a, b) in enumerate(zip(st.losses, want_losses)):
        assert abs(a - b) <= 1e-4 * abs(b), (i, a, b)
    for n, v in up.p.items():
        err = float((m.params[n].double() - v.detach()).abs().max())
        assert err <= 1e-4 * float(v.detach().abs().max()), (n, err)
    # sampling right after train(): the oracle on the denoiser's own trained parameters
    upt = U.UNetParams(D, Cc, TE, HT, {k: v.double() for k, v in m.params.items()})
    g = torch.Generator().manual_seed(4)
    x = torch.randn(3, D, generator=g)
    for tt in (0, 17, T - 1):
        got = m.forward_uniform_t(x.to(dev), tt, dtype="fp32").cpu().double()
        want = U.unet_forward(upt, x.double(), torch.full((3,), tt), emb).detach()
        assert float((got - want).abs().max()) <= 1e-4, tt
    noise = torch.randn(T, 3, D, generator=g)
    got = ldm_sdf.sample(m, ldm_sdf.DDPMSchedule(T=T), 3, steps=5, dtype="fp32", x_T=x,
                         noise=noise, device=dev).cpu().double()
    want = U.unet_sample_loop(upt, tab, emb, x.double(), noise.double(), steps=5)
    assert float((got - want).abs().max()) <= 1e-4


def test_train_bf16_packs_and_masters(dev):
    """After a bf16 step every bf16 working weight is bitwise the RNE rounding of its fp32
    master, the padding of the packed masters is still zero, and the masters are bitwise those
    of an fp32 AdamW step (ldm_adamw_step) on the same gradients."""
    import ldm_sdf
    from ldm_sdf import ops
    D, Cc, TE, HT, T = NET
    m0 = ldm_sdf.UNet1DDenoiser(D=D, C=Cc, TE=TE, HT=HT, T=T, seed=2468)
    before = m0.train_masters(dev)
    m, st, _ = _train(dev, 1, dtype="bf16")
    work, grads = st.adam_pack["work"], st.adam_grads
    n_bf16 = 0
    for n, p in st.masters.items():
        if work[n].dtype == torch.bfloat16:
            n_bf16 += 1
            assert torch.equal(work[n], p.to(torch.bfloat16)), n
        else:
            assert work[n] is p
        q = before[n].clone()
        ops.adamw_step(q, grads[n], torch.zeros_like(q), torch.zeros_like(q), None, lr=1e-3,
                       weight_decay=0.01, step=1)
        assert torch.equal(q, p), n
        assert torch.equal(m.import_tensor(n, m.params[n], dev), p), n    # zero padding
    assert n_bf16 == sum(ref.is_weight(n) for n in m.params)


def test_train_save_resume_bitwise(dev, tmp_path):
    """3 steps, TrainState.save, a fresh denoiser loading it, 3 more steps == 6 straight steps,
    bit for bit; and a second identical run equals the first."""
    import ldm_sdf
    from ldm_sdf.api import TrainState
    D, Cc, TE, HT, T = NET
    ref_m, ref_st, _ = _train(dev, 6)
    again_m, again_st, _ = _train(dev, 6)
    a_m, a_st, g = _train(dev, 3)
    path = str(tmp_path / "unet_state.pt")
    a_st.save(path, generator=g)
    b = ldm_sdf.UNet1DDenoiser(D=D, C=Cc, TE=TE, HT=HT, T=T, seed=999)
    g2 = torch.Generator().manual_seed(12345)
    st_b = TrainState.load(path, b, device=dev, generator=g2)
    assert st_b.step == 3 and st_b.hparams == {"lr": 1e-3, "weight_decay": 0.01}
    _, st_b, _ = _train(dev, 3, state=st_b, model=b, gen=g2)
    assert st_b.step == 6 and st_b.losses == ref_st.losses == again_st.losses
    for n in ref_m.params:
        assert torch.equal(b.params[n], ref_m.params[n]), n
        assert torch.equal(again_m.params[n], ref_m.params[n]), n
        for k in (0, 1):
            assert torch.equal(st_b.adam[n][k], ref_st.adam[n][k]), n
            assert torch.equal(again_st.adam[n][k], ref_st.adam[n][k]), n
