"""The batched sampling loop (ldm_sample_batch) on the MI355X: sampling more than
16 latents per call, element-wise parity with the CPU emulation of its rounding map
(tests/sample_batch_emulation.py) at the tolerance tests/test_sample_batch_emulation.py derives
(TOL = 4 x the measured fp32-vs-fp64-product floor; the mutants it separates are listed there:
a wrong E row, a wrong noise row, z at t = 0, a dropped last row, a leaking padding row -- all
of them at every step count, 20 included), the t = 0 step, buffer bounds, bitwise batch
invariance, graph replay, the distance to the <= 16 path, staleness and chunking.

Networks: S is D = 64, H = 128, 2 blocks (the 64-deep tile); L is the default D = 256, H = 1024,
4 blocks (the 128-deep two-k-group tile).  Inputs come from a seeded host generator."""
import pytest
import torch

from tests import sample_batch_emulation as E

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import ldm_sdf
    ldm_sdf.load_library()
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def nets(dev):
    """{network: MLPDenoiser} over the oracle's parameters, and the schedule."""
    import ldm_sdf
    models = {net: E.model_of(E.oracle_net(net)[0]) for net in (E.NET_S, E.NET_L)}
    return models, ldm_sdf.DDPMSchedule()


def run_direct(model, sch, dev, x_T, noise, t_hi, steps, x2=None, ws=None):
    """ops.sample_batch on device tensors; returns the result view x2[steps & 1]."""
    from ldm_sdf import ops
    desc = model.device_pack("bf16", dev)["desc"]
    n, D = x_T.shape
    if x2 is None:
        x2 = torch.empty(2, n, D, device=dev)
    if ws is None:
        ws = ops.sample_batch_workspace(desc, n, dev)
    x2[0].copy_(x_T)
    ops.sample_batch(desc, sch.device(dev)["desc"], x2, noise, t_hi, steps, ws)
    return x2[steps & 1]


# ---- 1. the gap --------------------------------------------------------------------------------
def test_more_than_16_latents_in_one_call(dev, nets):
    import ldm_sdf
    models, sch = nets
    model = models[E.NET_L]
    g = torch.Generator(device=dev).manual_seed(1)
    a = ldm_sdf.sample(model, sch, 17, steps=3, device=dev, generator=g)
    b = ldm_sdf.sample(model, sch, 17, steps=3, device=dev, generator=g, form="batched")
    for x in (a, b):
        assert x.shape == (17, model.D) and x.dtype == torch.float32
        assert bool(torch.isfinite(x).all())


def test_unsupported_forms_fail_at_construction(dev, nets):
    import ldm_sdf
    models, sch = nets
    for kw in (dict(dtype="fp32"), dict(persistent=False)):
        with pytest.raises(ldm_sdf.LdmError):
            ldm_sdf.Sampler(models[E.NET_S], sch, 17, steps=3, device=dev, **kw)


# ---- 2. emulation parity -------------------------------------------------------------------------
@pytest.mark.parametrize("case", E.PARITY_CASES, ids=E.case_id)
def test_matches_the_emulation(dev, nets, case):
    models, sch = nets
    net, n, t_hi, steps = case
    x_T, noise = E.case_inputs(case)
    got = run_direct(models[net], sch, dev, x_T.to(dev), noise.to(dev), t_hi, steps).cpu()
    assert bool(torch.isfinite(got).all())
    d = E.max_dev(got, E.reference(case))
    print(f"{E.case_id(case)}: max|dev| {d:.2e} (tol {E.TOL[steps]:.1e})")
    assert d <= E.TOL[steps]


# ---- 3. t = 0 ------------------------------------------------------------------------------------
@pytest.mark.parametrize("net,n", [(E.NET_S, 65), (E.NET_L, 17)], ids=["S65", "L17"])
def test_noise_is_not_read_at_t0(dev, nets, net, n):
    models, sch = nets
    x_T, noise = E.inputs(n, net[2], 5, 1, 2)
    noise = noise.to(dev)
    a = run_direct(models[net], sch, dev, x_T.to(dev), noise, 1, 2).clone()
    noise[0] = float("nan")
    b = run_direct(models[net], sch, dev, x_T.to(dev), noise, 1, 2).clone()
    assert bool(torch.isfinite(b).all()) and torch.equal(a, b)
    c = run_direct(models[net], sch, dev, x_T.to(dev), noise, 0, 1)
    assert bool(torch.isfinite(c).all())


# ---- 4. bounds -------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [17, 65])
def test_canaries_around_x_and_workspace_survive(dev, nets, n):
    from ldm_sdf import ops
    models, sch = nets
    model = models[E.NET_S]
    D, pad = model.D, 4096
    x_T, noise = E.inputs(n, D, 9, E.T - 1, 3)
    canary = 12345.678
    big = torch.full((2 * n * D + 2 * pad,), canary, device=dev)
    x2 = big[pad:pad + 2 * n * D].view(2, n, D)
    desc = model.device_pack("bf16", dev)["desc"]
    nbytes = ops.sample_batch_workspace(desc, n, dev).numel()
    raw = torch.full((nbytes + 3 * 256 + 2 * pad,), 0xA5, device=dev, dtype=torch.uint8)
    off = pad + (-(raw.data_ptr() + pad)) % 256
    ws = raw[off:off + nbytes]
    got = run_direct(model, sch, dev, x_T.to(dev), noise.to(dev), E.T - 1, 3, x2=x2, ws=ws)
    assert bool(torch.isfinite(got).all())
    # (3 steps: within the 5-step tolerance, whose floor bounds the 3-step one from above)
    assert E.max_dev(got.cpu(), E.sample(E.NET_S, x_T, noise, E.T - 1, 3)) <= E.TOL[5]
    assert bool((big[:pad] == canary).all()) and bool((big[pad + 2 * n * D:] == canary).all())
    assert bool((raw[:off] == 0xA5).all()) and bool((raw[off + nbytes:] == 0xA5).all())


# ---- 5. batch invariance, bitwise ------------------------------------------------------------------
def test_rows_do_not_depend_on_the_batch(dev, nets):
    models, sch = nets
    model, D, steps = models[E.NET_L], E.NET_L[2], 3
    x17, z17 = E.inputs(17, D, 11, E.T - 1, steps)
    lo = E.T - steps
    out = {}
    for n in (17, 130, 1024):
        g = torch.Generator(device=dev).manual_seed(n)
        x_T = torch.randn(n, D, device=dev, generator=g)
        x_T[:17] = x17.to(dev)
        noise = torch.empty(E.T, n, D, device=dev)       # only rows lo.. are read
        noise[lo:] = torch.randn(steps, n, D, device=dev, generator=g)
        noise[lo:, :17] = z17[lo:].to(dev)
        out[n] = run_direct(model, sch, dev, x_T, noise, E.T - 1, steps)[:17].clone()
        del noise
    assert bool(torch.isfinite(out[17]).all())
    assert torch.equal(out[130], out[17]), float((out[130] - out[17]).abs().max())
    assert torch.equal(out[1024], out[17]), float((out[1024] - out[17]).abs().max())


# ---- 6. replay -------------------------------------------------------------------------------------
def test_graph_replay_equals_eager_and_leaks_no_state(dev, nets):
    import ldm_sdf
    models, sch = nets
    model, D, n, steps = models[E.NET_S], E.NET_S[2], 33, 4
    (xa, za), (xb, zb) = (E.inputs(n, D, s, E.T - 1, steps) for s in (21, 22))
    xa, za, xb, zb = (t.to(dev) for t in (xa, za, xb, zb))
    kw = dict(steps=steps, device=dev)
    eager = ldm_sdf.Sampler(model, sch, n, use_graph=False, **kw)
    graph = ldm_sdf.Sampler(model, sch, n, use_graph=True, **kw)
    assert eager.batched and graph.loop.batched and graph.loop.status() == 0
    a_e = eager.run(xa, za).clone()
    a_g = graph.run(xa, za).clone()
    assert graph.graph is not None and eager.graph is None
    assert torch.equal(a_e, a_g)
    b_g = graph.run(xb, zb).clone()                      # a replay on new inputs
    b_e = eager.run(xb, zb).clone()
    fresh = ldm_sdf.Sampler(model, sch, n, use_graph=False, **kw).run(xb, zb).clone()
    assert not torch.equal(a_g, b_g)
    assert torch.equal(b_g, fresh) and torch.equal(b_e, fresh)
    assert torch.equal(graph.run(xa, za), a_e)


# ---- 7. cross-path ---------------------------------------------------------------------------------
def test_close_to_the_16_row_path(dev, nets):
    import ldm_sdf
    models, sch = nets
    net, n, t_hi, steps = E.CROSS_CASE
    x_T, noise = E.case_inputs(E.CROSS_CASE)
    x_T, noise = x_T.to(dev), noise.to(dev)
    big = ldm_sdf.sample(models[net], sch, n, steps=steps, x_T=x_T, noise=noise, device=dev,
                         form="batched")
    small = ldm_sdf.sample(models[net], sch, 16, steps=steps, x_T=x_T[:16],
                           noise=noise[:, :16].contiguous(), device=dev)
    d = E.max_dev(big[:16].cpu(), small.cpu())
    print(f"batched n = {n} rows 0..15 vs sample(n = 16): {d:.2e} "
          f"(bound {4 * E.ACT_ROUNDING:.1e})")
    assert 0.0 < d <= 4.0 * E.ACT_ROUNDING          # close, and not the same arithmetic


# ---- 8. staleness ----------------------------------------------------------------------------------
def test_stale_loop_raises_and_sampler_repacks(dev, nets):
    import ldm_sdf
    _, sch = nets
    model = E.model_of(E.oracle_net(E.NET_S)[0])         # private: its tables get invalidated
    D, n, steps = E.NET_S[2], 17, 3
    x_T, noise = (t.to(dev) for t in E.inputs(n, D, 31, E.T - 1, steps))
    sd = sch.device(dev)["desc"]
    loop = model.make_loop(n, "bf16", dev, sd)
    assert loop.batched and loop.status() == 0 and loop.keep
    x2 = torch.empty(2, n, D, device=dev)
    x2[0].copy_(x_T)
    loop(x2, noise, E.T - 1, steps)
    ref = x2[steps & 1].clone()
    sampler = ldm_sdf.Sampler(model, sch, n, steps=steps, device=dev)
    assert torch.equal(sampler.run(x_T, noise), ref)
    old = sampler.loop
    model.invalidate_tables()
    with pytest.raises(ldm_sdf.LdmError):
        loop(x2, noise, E.T - 1, steps)
    assert torch.equal(sampler.run(x_T, noise), ref)     # same weights: same tables rebuilt
    assert sampler.loop is not old and sampler.graph is not None


# ---- 9. chunking -----------------------------------------------------------------------------------
def test_chunked_calls_equal_unchunked(dev, nets):
    import ldm_sdf
    models, sch = nets
    model, D, n, steps = models[E.NET_L], E.NET_L[2], 40, 3
    x_T, noise = (t.to(dev) for t in E.inputs(n, D, 41, E.T - 1, steps))
    kw = dict(steps=steps, x_T=x_T, noise=noise, device=dev)
    whole = ldm_sdf.sample(model, sch, n, form="batched", **kw)
    assert torch.equal(ldm_sdf.sample(model, sch, n, form="batched", chunk=24, **kw), whole)
    assert torch.equal(ldm_sdf.sample(model, sch, n, form="batched", chunk=7, **kw), whole)
    by16 = ldm_sdf.sample(model, sch, n, form="loop16", **kw)
    parts = [ldm_sdf.sample(model, sch, hi - lo, steps=steps, x_T=x_T[lo:hi],
                            noise=noise[:, lo:hi].contiguous(), device=dev)
             for lo, hi in ((0, 16), (16, 32), (32, 40))]
    assert torch.equal(by16, torch.cat(parts))
    assert not torch.equal(by16, whole)                  # fp32 against bf16 activations
