"""The bf16 training path through the C ABI on the MI355X (csrc/denoiser_train.hip):
ldm_denoiser_fwd (per-sample t) / ldm_denoiser_bwd / ldm_denoiser_train_step /
ldm_q_sample_loss / ldm_adamw_multi, called through ctypes.

References:
  * a bf16-operand emulation of the oracle (tests/denoiser_emulation.py: oracle/ref_cpu.py's
    network and its backward with every GEMM operand rounded to bf16 as the kernels round it,
    fp64 arithmetic otherwise): the forward output agrees to <= 2e-3 relative to its scale
    (rounding-boundary flips of single operands and fp32 accumulation order are all that
    differ); the loss, EVERY gradient and dx agree ELEMENT-WISE (max|dev| / max|ref| per tensor)
    at denoiser_emulation.TOL = 4 x the CPU noise floor of tests/test_train_emulation.py, which
    also shows that a dropped sample, a zeroed gradient row, a skipped dtemb K-segment and an
    unmasked padding row each land >= 4 x TOL away (the whole-tensor checks below let all four
    through);
  * the fp64 oracle itself (unrounded weights): loss within 1e-3 relative, every gradient at
    cosine >= 0.999 and norm within 2 % (bf16 operand rounding), as the ldm_linear bf16 path;
  * the modular fwd -> q_sample_loss -> bwd sequence against the fused step on the same
    inputs (same activations; the loss gradient enters through fp32 deps instead of the
    epilogue: <= 1e-3 relative);
  * ldm_adamw_multi against ldm_adamw_step bit for bit, and its bf16 copies (both layouts)
    against the RNE-rounded master.
"""
import math

import numpy as np
import pytest
import torch

from tests import denoiser_emulation as E

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import ldm_sdf
    ldm_sdf.load_library()
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def net():
    from ldm_sdf import MLPDenoiser
    from oracle import ref_cpu as R
    p = R.make_denoiser_params(seed=4321)
    params = {n: getattr(p, n) for n in ("Wt1", "bt1", "Wt2", "bt2", "Win", "bin", "Wout", "bout")}
    for k in range(p.n_blocks):
        params[f"Wblk{k}"], params[f"bblk{k}"] = p.Wblk[k], p.bblk[k]
    return MLPDenoiser(params=params), p


def _inputs(B, seed):
    g = torch.Generator().manual_seed(seed)
    x0 = torch.randn(B, 256, generator=g) * 0.5
    t = torch.randint(0, 1000, (B,), generator=g, dtype=torch.int32)
    eps = torch.randn(B, 256, generator=g)
    return x0, t, eps


@pytest.mark.parametrize("B", [1, 37, 64, 200])
def test_denoiser_fwd_per_sample_t(dev, net, B):
    """ldm_denoiser_fwd with per-sample t vs the bf16-emulated oracle (ragged B: padding rows)."""
    from ldm_sdf import ops
    from oracle import ref_cpu as R
    model, p = net
    model.to_device(dev)
    desc = model.device_pack("bf16", dev, with_tables=False)["desc"]
    x0, t, eps = _inputs(B, B)
    ws = ops.train_workspace(desc, B, dev)
    out = torch.empty(B, 256, device=dev)
    ops.denoiser_fwd(desc, x0.to(dev), t.to(dev), ws, out)
    emb = torch.from_numpy(R.timestep_embedding_table(1000, 128)).double()
    want = E.forward(p, x0, t, emb)["eps_hat"]
    scale = float(want.abs().max())
    err = float((out.cpu().double() - want).abs().max()) / scale
    print(f"B={B}: fwd rel err vs bf16-emulated oracle {err:.2e}")
    assert err <= 2e-3, err
    # and vs the exact oracle, loosely (bf16 operands)
    exact = R.denoiser_forward(p, x0.double(), t.long(), emb)
    cos = float((out.cpu().double().flatten() @ exact.flatten())
                / (out.cpu().double().norm() * exact.norm()))
    assert cos >= 0.9995, cos


@pytest.mark.parametrize("B", [64, 1000])
def test_train_step_fused_vs_oracle(dev, net, B):
    """ldm_denoiser_train_step (the config-2 step at B = 1000) vs the fp64 oracle's autograd."""
    from ldm_sdf import ops
    from oracle import ref_cpu as R
    import ldm_sdf
    model, p = net
    model.to_device(dev)
    desc = model.device_pack("bf16", dev, with_tables=False)["desc"]
    sd = ldm_sdf.DDPMSchedule().device(dev)
    x0, t, eps = _inputs(B, 100 + B)
    grads = {n: torch.full_like(model.params[n], float("nan")) for n in model.names()}
    loss = torch.empty(1, device=dev)
    ws = ops.train_workspace(desc, B, dev)
    ops.denoiser_train_step(desc, sd["desc"], x0.to(dev), eps.to(dev), t.to(dev), ws,
                            model.grads_struct(grads), loss)
    emb = torch.from_numpy(R.timestep_embedding_table(1000, 128)).double()
    torch.set_num_threads(min(16, torch.get_num_threads()))
    wl, wg = R.train_step_grads(p, R.ddpm_tables(), emb, x0.double(), eps.double(), t.long())
    assert abs(float(loss) - float(wl)) / float(wl) < 1e-3, (float(loss), float(wl))
    for k, v in grads.items():
        got = v.cpu().double().flatten()
        w = wg[k].flatten()
        assert bool(torch.isfinite(got).all()), k
        cos = float(got @ w / (got.norm() * w.norm() + 1e-30))
        rel = abs(float(got.norm()) - float(w.norm())) / float(w.norm())
        print(f"B={B} {k}: cos {cos:.6f} norm rel {rel:.2e}")
        assert cos >= 0.999 and rel <= 2e-2, (k, cos, rel)


def _device_fused_step(dev, case, poison=False):
    """ldm_denoiser_train_step (the launches) on a case's inputs, gradients pre-filled with NaN;
    ``poison``: the workspace holds 0xFF bytes (NaN as bf16 and as fp32) before its init."""
    import ctypes as C
    import ldm_sdf
    from ldm_sdf import _capi as capi, ops
    net_shape, B, seed = case
    p = E.oracle_net(net_shape)[0]
    model = E.model_of(p)
    model.to_device(dev)
    desc = model.device_pack("bf16", dev, with_tables=False)["desc"]
    sd = ldm_sdf.DDPMSchedule().device(dev)
    x0, t, eps = E.inputs(B, p.D, seed)
    grads = {n: torch.full_like(model.params[n], float("nan")) for n in model.names()}
    loss = torch.full((1,), float("nan"), device=dev)
    ws = ops.train_workspace(desc, B, dev)
    if poison:
        ws.fill_(0xFF)
        capi.check(capi.load().ldm_denoiser_train_ws_init(C.byref(desc), B, ws.data_ptr(),
                                                          capi.stream_handle(dev)),
                   "ldm_denoiser_train_ws_init")
    ops.denoiser_train_step(desc, sd["desc"], x0.to(dev), eps.to(dev), t.to(dev), ws,
                            model.grads_struct(grads), loss)
    torch.cuda.synchronize()
    assert ops.train_step_last_form() == "launches"
    return float(loss), {n: g.cpu() for n, g in grads.items()}


DEFAULT_CASES = [c for c in E.FUSED_CASES if c[0] == E.DEFAULT_NET and c != E.CONFIG2_CASE]
OTHER_CASES = [c for c in E.FUSED_CASES if c[0] != E.DEFAULT_NET]


@pytest.mark.parametrize("case", DEFAULT_CASES, ids=[f"B{c[1]}" for c in DEFAULT_CASES])
def test_train_step_elementwise_vs_emulation(dev, case):
    """The fused step's loss and every gradient, ELEMENT-WISE against the bf16-operand emulation
    (tests/denoiser_emulation.py) at denoiser_emulation.TOL (weights 1.2e-2, biases 4e-3, loss
    1.2e-5 of the tensor's largest magnitude: 4 x the CPU noise floor, and >= 4 x below what a
    dropped sample, a zeroed row, a skipped dtemb segment or an unmasked padding row moves --
    tests/test_train_emulation.py).  B = 1: one live row in a 64-row pad; 37: a ragged band;
    65: the second 64-row band and the third 32-row block hold one live row; 200; 1000: config
    2's size, the only one at which the dtemb launch takes its 128-deep tile and the grouped
    launches their large-batch tile choice.

    Measured on the MI355X, largest deviation per tensor kind (weights / biases / loss):
        B = 1      3.0e-3 / 2.3e-4 / 5.9e-8      B = 37     3.1e-3 / 9.0e-4 / 9.4e-7
        B = 65     1.2e-3 / 5.6e-4 / 2.6e-7      B = 200    9.2e-4 / 5.8e-4 / 6.6e-7
        B = 1000   4.0e-3 / 3.4e-4 / 5.8e-7      config 2   1.2e-3 / 2.7e-4 / 2.9e-7
        (1,256,128,64) 4.1e-4 / 2.0e-4 / 9.3e-8  (2,512,64,128) 5.3e-4 / 2.5e-4 / 8.8e-7
        (8,256,256,64) 4.5e-4 / 1.9e-4 / 6.8e-7  poisoned workspace: the fresh one's figures
        modular B = 65: 6.8e-4 / 3.4e-4, dx 2.0e-4;  B = 200: 7.0e-4 / 3.2e-4, dx 2.9e-4
    (B = 1 and B = 1000, where the 4-sigma last sample dominates the largest elements: one
    flipped bf16 tie in a row of g shows at nearly full size, 2^-8 = 3.9e-3)."""
    got_loss, got = _device_fused_step(dev, case)
    want_loss, want = E.fused_reference(case)
    E.check_against(got_loss, got, want_loss, want, f"B={case[1]}")


@pytest.mark.parametrize("case", OTHER_CASES,
                         ids=[f"nb{c[0][0]}-H{c[0][1]}-D{c[0][2]}-TE{c[0][3]}" for c in OTHER_CASES])
def test_train_step_elementwise_other_networks(dev, case):
    """The networks test_gpu_train_dag.py only compares DAG == launches on -- (n_blocks, H, D,
    TE) = (1, 256, 128, 64), (2, 512, 64, 128), (8, 256, 256, 64) at B = 200 -- element-wise
    against the emulation, same tolerance."""
    got_loss, got = _device_fused_step(dev, case)
    want_loss, want = E.fused_reference(case)
    E.check_against(got_loss, got, want_loss, want, E.case_id(case))


@pytest.mark.parametrize("B", [37, 65])
def test_train_step_poisoned_workspace(dev, B):
    """The step must not depend on what its workspace held: padding rows of every bf16 operand
    are written (as zero) by their producers (denoiser_train.hip's header), and a fresh zeroed
    allocation would hide a producer that does not.  The workspace is filled with 0xFF bytes
    (NaN as bf16 and as fp32) and then initialised as any workspace is; everything must be
    finite and within the element-wise tolerance."""
    case = (E.DEFAULT_NET, B, 100 + B)
    got_loss, got = _device_fused_step(dev, case, poison=True)
    assert math.isfinite(got_loss)
    want_loss, want = E.fused_reference(case)
    E.check_against(got_loss, got, want_loss, want, f"poisoned ws B={B}")


@pytest.mark.parametrize("case", E.MODULAR_CASES, ids=[f"B{c[1]}" for c in E.MODULAR_CASES])
def test_modular_elementwise_vs_emulation(dev, case):
    """denoiser_fwd -> q_sample_loss -> denoiser_bwd: x_t is the emulation's bit for bit (two
    rounded products, one rounded sum), and every gradient and dx agree element-wise with the
    emulation fed the same x_t and the same fp32 deps (there bout is the column sum of deps
    itself)."""
    import ldm_sdf
    from ldm_sdf import ops
    net_shape, B, seed = case
    p, emb, sab, s1mab = E.oracle_net(net_shape)
    model = E.model_of(p)
    model.to_device(dev)
    desc = model.device_pack("bf16", dev, with_tables=False)["desc"]
    sd = ldm_sdf.DDPMSchedule().device(dev)
    x0, t, eps = E.inputs(B, p.D, seed)
    xt = torch.empty(B, p.D, device=dev)
    ops.q_sample_loss(sd["desc"], eps.to(dev), x0=x0.to(dev), t=t.to(dev), xt_out=xt)
    assert torch.equal(xt.cpu(), E.q_sample_f32(sab, s1mab, x0, eps, t))
    ws = ops.train_workspace(desc, B, dev)
    eps_hat = torch.empty(B, p.D, device=dev)
    ops.denoiser_fwd(desc, xt, t.to(dev), ws, eps_hat)
    loss, deps = torch.empty(1, device=dev), torch.empty(B, p.D, device=dev)
    ops.q_sample_loss(sd["desc"], eps.to(dev), eps_hat=eps_hat, loss_out=loss, grad_out=deps)
    grads = {n: torch.full_like(model.params[n], float("nan")) for n in model.names()}
    dx = torch.full((B, p.D), float("nan"), device=dev)
    ops.denoiser_bwd(desc, ws, deps, model.grads_struct(grads), dx)
    torch.cuda.synchronize()
    got = {n: g.cpu() for n, g in grads.items()}
    got["dx"] = dx.cpu()
    torch.set_num_threads(min(16, torch.get_num_threads()))
    want_eps_hat, want = E.fwd_bwd(p, emb, xt.cpu(), t, deps.cpu())
    assert E.rel_dev(eps_hat.cpu(), want_eps_hat) <= 2e-3
    E.check_against(None, got, None, want, f"modular B={B}")


def test_modular_fwd_bwd_matches_fused(dev, net):
    """fwd -> q_sample_loss -> bwd (the three SURVEY §8(b) entry points) == the fused step."""
    from ldm_sdf import ops
    import ldm_sdf
    model, _ = net
    model.to_device(dev)
    desc = model.device_pack("bf16", dev, with_tables=False)["desc"]
    sd = ldm_sdf.DDPMSchedule().device(dev)
    B = 300
    x0, t, eps = (v.to(dev) for v in _inputs(B, 7))
    gf = {n: torch.empty_like(model.params[n]) for n in model.names()}
    gm = {n: torch.empty_like(model.params[n]) for n in model.names()}
    loss_f = torch.empty(1, device=dev)
    ws = ops.train_workspace(desc, B, dev)
    ops.denoiser_train_step(desc, sd["desc"], x0, eps, t, ws, model.grads_struct(gf), loss_f)
    xt = torch.empty(B, 256, device=dev)
    ops.q_sample_loss(sd["desc"], eps, x0=x0, t=t, xt_out=xt)
    want_xt = ops.q_sample(sd["desc"], x0, eps, t)
    assert torch.equal(xt, want_xt)                       # the A9 head is bit-exact
    eps_hat = torch.empty(B, 256, device=dev)
    ops.denoiser_fwd(desc, xt, t, ws, eps_hat)
    loss_m, deps = torch.empty(1, device=dev), torch.empty(B, 256, device=dev)
    ops.q_sample_loss(sd["desc"], eps, eps_hat=eps_hat, loss_out=loss_m, grad_out=deps)
    dx = torch.empty(B, 256, device=dev)
    ops.denoiser_bwd(desc, ws, deps, model.grads_struct(gm), dx)
    assert abs(float(loss_m) - float(loss_f)) <= 1e-5 * float(loss_f)
    for n in gf:
        a, b = gf[n].double(), gm[n].double()
        assert float((a - b).norm() / b.norm()) <= 1e-3, n
    # dx = dL/dx_t against autograd of the bf16-emulated network's first layer chain is covered
    # by the fp64 check below: finite and the right scale
    assert bool(torch.isfinite(dx).all()) and float(dx.abs().max()) > 0


def test_dx_vs_oracle(dev, net):
    """dL/dx_t from ldm_denoiser_bwd vs fp64 autograd of the oracle network."""
    from ldm_sdf import ops
    from oracle import ref_cpu as R
    model, p = net
    model.to_device(dev)
    desc = model.device_pack("bf16", dev, with_tables=False)["desc"]
    B = 128
    x, t, eps = _inputs(B, 11)
    ws = ops.train_workspace(desc, B, dev)
    eps_hat = torch.empty(B, 256, device=dev)
    ops.denoiser_fwd(desc, x.to(dev), t.to(dev), ws, eps_hat)
    deps = (2.0 * (eps_hat.cpu() - eps) / (B * 256)).float()
    grads = {n: torch.empty_like(model.params[n]) for n in model.names()}
    dx = torch.empty(B, 256, device=dev)
    ops.denoiser_bwd(desc, ws, deps.to(dev), model.grads_struct(grads), dx)
    emb = torch.from_numpy(R.timestep_embedding_table(1000, 128)).double()
    xd = x.double().requires_grad_(True)
    with torch.enable_grad():
        out = R.denoiser_forward(p, xd, t.long(), emb)
        ((out - eps.double()) ** 2).mean().backward()
    w = xd.grad.flatten()
    got = dx.cpu().double().flatten()
    cos = float(got @ w / (got.norm() * w.norm()))
    assert cos >= 0.999, cos


def test_adamw_multi_matches_single(dev):
    """One launch over mixed shapes == ldm_adamw_step per tensor, bitwise; bf16 copies RNE."""
    from ldm_sdf import ops
    g = torch.Generator(device=dev).manual_seed(9)
    shapes = [(1024, 2048), (256, 1024), (1000,), (1024, 128), (77, 130), (5,)]
    ps = [torch.randn(s, device=dev, generator=g) for s in shapes]
    ref = [p.clone() for p in ps]
    ms = [torch.zeros_like(p) for p in ps]
    vs = [torch.zeros_like(p) for p in ps]
    mr = [torch.zeros_like(p) for p in ps]
    vr = [torch.zeros_like(p) for p in ps]
    lows = [torch.empty_like(p, dtype=torch.bfloat16) if p.dim() == 2 else None for p in ps]
    lowt = [torch.empty(p.shape[1], p.shape[0], device=dev, dtype=torch.bfloat16)
            if p.dim() == 2 else None for p in ps]
    grads = [torch.empty_like(p) for p in ps]
    table = ops.adamw_table(list(zip(ps, grads, ms, vs, lows, lowt)))
    for step in range(1, 4):
        for gr in grads:
            gr.copy_(torch.randn(gr.shape, device=dev, generator=g))
        ops.adamw_multi(table, lr=3e-3, weight_decay=0.01, step=step, device=dev)
        for i in range(len(ps)):
            ops.adamw_step(ref[i], grads[i], mr[i], vr[i], None, lr=3e-3, weight_decay=0.01,
                           step=step)
    torch.cuda.synchronize()
    for i, p in enumerate(ps):
        assert torch.equal(p, ref[i]) and torch.equal(ms[i], mr[i]) and torch.equal(vs[i], vr[i])
        if lows[i] is not None:
            assert torch.equal(lows[i], p.to(torch.bfloat16))
            assert torch.equal(lowt[i], p.t().contiguous().to(torch.bfloat16))


def test_train_bf16_loop_learns_and_matches_torch_adamw(dev, net):
    """train(dtype='bf16') (fused step + ldm_adamw_multi) tracks the same run driven by
    torch.optim.AdamW over the same fused gradients, and lowers the loss."""
    import ldm_sdf
    from ldm_sdf import MLPDenoiser
    _, p = net
    params = {n: getattr(p, n) for n in ("Wt1", "bt1", "Wt2", "bt2", "Win", "bin", "Wout", "bout")}
    for k in range(p.n_blocks):
        params[f"Wblk{k}"], params[f"bblk{k}"] = p.Wblk[k], p.bblk[k]
    lat = torch.randn(512, 256, generator=torch.Generator().manual_seed(2)).to(dev) * 0.5
    sch = ldm_sdf.DDPMSchedule()
    runs = []
    for use_torch in (False, True):
        model = MLPDenoiser(params={k: v.clone() for k, v in params.items()})
        model.to_device(dev)
        st = None
        if use_torch:
            st = ldm_sdf.api.TrainState()
            st.masters = {n: model.params[n] for n in model.names()}
            st.optimizer = torch.optim.AdamW(list(st.masters.values()), lr=3e-4, weight_decay=0.0)
        st = ldm_sdf.train(model, sch, lat, steps=30, batch=512, lr=3e-4, dtype="bf16", state=st,
                           generator=torch.Generator(device=dev).manual_seed(8))
        runs.append((st.losses, {n: t.clone() for n, t in model.params.items()}))
    (la, pa), (lb, pb) = runs
    assert np.mean(la[-5:]) < np.mean(la[:5])
    # same gradients, same update rule; torch's multi-tensor AdamW orders its fp32 ops
    # differently (ulp-level differences per step), and 30 steps of training amplify them --
    # measured 1.2e-3 relative on the weights (bit-level agreement with torch's single-tensor
    # order is test_adamw_step_matches_torch / test_adamw_multi_matches_single)
    assert max(abs(a - b) for a, b in zip(la, lb)) <= 1e-3 * max(lb)
    for n in pa:
        assert (pa[n] - pb[n]).abs().max() <= 3e-3 * pb[n].abs().max() + 1e-6, n


def test_train_step_adamw_fused_overlap_bitwise(dev, net):
    """ldm_denoiser_train_step_adamw (early weight updates forked onto a side stream) ==
    its hipGraph replays (device AdamW scalars) == the entry point serialised (side = NULL) ==
    ldm_denoiser_train_step + ldm_adamw_multi, bit for bit: losses, fp32 masters, Adam
    moments and both bf16 working copies."""
    import ldm_sdf
    from ldm_sdf import MLPDenoiser
    _, p = net
    params = {n: getattr(p, n) for n in ("Wt1", "bt1", "Wt2", "bt2", "Win", "bin", "Wout", "bout")}
    for k in range(p.n_blocks):
        params[f"Wblk{k}"], params[f"bblk{k}"] = p.Wblk[k], p.bblk[k]
    lat = torch.randn(300, 256, generator=torch.Generator().manual_seed(5)).to(dev) * 0.5
    sch = ldm_sdf.DDPMSchedule()
    runs = []
    for fused, overlap, graph in ((True, True, False), (True, False, True),
                                  (True, False, False), (False, False, False)):
        model = MLPDenoiser(params={k: v.clone() for k, v in params.items()})
        model.to_device(dev)
        gen = torch.Generator(device=dev).manual_seed(3)
        # 40 steps in two calls: graph slots run eagerly in the first 32-step block, are
        # captured, then replay (the second call reuses the state's graphs)
        st = ldm_sdf.train(model, sch, lat, steps=30, batch=300, lr=1e-3, weight_decay=0.01,
                           dtype="bf16", generator=gen, fused_step=fused, overlap=overlap,
                           graph=graph)
        st = ldm_sdf.train(model, sch, lat, steps=10, batch=300, dtype="bf16", generator=gen,
                           state=st, fused_step=fused, overlap=overlap, graph=graph)
        work = model.device_pack("bf16", dev, with_tables=False)
        runs.append((list(st.losses), {n: t.clone() for n, t in model.params.items()},
                     {n: (m.clone(), v.clone()) for n, (m, v) in st.adam.items()},
                     {n: t.clone() for n, t in work.items() if isinstance(t, torch.Tensor)}))
    torch.cuda.synchronize()
    ref = runs[-1]
    for r in runs[:-1]:
        assert r[0] == ref[0]
        for n in ref[1]:
            assert torch.equal(r[1][n], ref[1][n]), n
            assert torch.equal(r[2][n][0], ref[2][n][0]) and torch.equal(r[2][n][1], ref[2][n][1])
        for n in ref[3]:
            assert torch.equal(r[3][n], ref[3][n]), n
