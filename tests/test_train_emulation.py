"""The reference of the element-wise bf16 training-gradient tests, tested on the CPU.

tests/denoiser_emulation.py restates the fused training step (csrc/denoiser_train.hip) in
plain torch with the kernels' bf16 operand roundings; tests/test_gpu_train_capi.py compares the
device with it element by element.  Here, with no GPU, for every (network, B, inputs) case those
tests run (metric per tensor: max|a - b| / max|b|):

(a) the fp64 emulation against the fp64 oracle's autograd (oracle/ref_cpu.train_step_grads):
    the emulation is the same network, bf16 operand rounding apart.  Measured over the cases:
    weights <= 8.2e-3 (the 8-block network; 7.9e-3 at B = 1), biases <= 5.2e-3, loss <= 6.1e-4
    relative, dx (modular cases) <= 2.8e-3; asserted at about twice that (ORACLE_BOUND).
(b) the noise floor: the emulation with fp32 products (one thread, so the order does not depend
    on the machine's CPU count) against the one with fp64 products -- an fp32 summation order
    and the bf16 rounding ties it flips downstream, which is all that separates the device from
    the fp64 emulation too.  Measured:

        case                      weights   biases    dx        loss
        default net  B = 1        2.5e-3    8.3e-5    5.1e-7    7.7e-9
        default net  B = 37       1.3e-3    6.6e-4    7.9e-4    8.0e-7
        default net  B = 65       1.6e-3    6.3e-4    4.9e-4    1.4e-6
        default net  B = 200      9.0e-4    7.9e-4    5.7e-4    2.5e-6
        default net  B = 1000     3.9e-4    3.6e-4    6.5e-4    3.9e-7
        config 2     B = 1000     4.9e-4    2.4e-4    8.3e-4    5.1e-7
        (1,256,128,64)  B = 200   6.3e-4    3.0e-4    8.4e-4    8.5e-7
        (2,512,64,128)  B = 200   4.4e-4    2.2e-4    4.5e-4    1.1e-6
        (8,256,256,64)  B = 200   5.5e-4    2.7e-4    4.7e-4    2.9e-7
        modular      B = 65       1.6e-3    3.1e-4    2.1e-4    -
        modular      B = 200      6.7e-4    3.4e-4    2.9e-4    -

    At B = 1 a weight gradient is the outer product of two bf16 vectors, so the floor there is
    quantised: zero, or one flipped tie, which moves a whole row by one bf16 ulp (2^-8 .. 2^-7
    of its value; here it hit a row at 0.6 of the largest).
    denoiser_emulation.FLOOR holds the largest per tensor kind, rounded up (weights 3.0e-3,
    biases 1.0e-3, dx 1.0e-3, loss 3.0e-6), and the device tolerance is TOL = 4 x FLOOR (weights
    1.2e-2, biases 4e-3, dx 4e-3, loss 1.2e-5): the device's summation order (32 x 32 MFMA
    blocks, k-group split) is a third order, and tie flips are discrete, so the maximum moves
    by small factors between orders.  Asserted: every measured floor <= FLOOR.
(c) mutants of the reference -- the mistakes the whole-tensor cosine checks let through -- each
    land >= 4 x TOL away on at least one tensor the GPU test of that case compares (smallest
    deviation over the cases, on the tensor that shows it best):
      * the last live sample's contribution removed: 3.2e-1 (weights, config 2; 4 x TOL =
        4.8e-2);
      * one output row of a weight gradient zeroed, for EVERY weight tensor, the row of median
        magnitude (a row that is ~0 anyway cannot be missed): 6.5e-2 (Wt1 at B = 1);
      * one K-segment of the dtemb product skipped, for the first, middle and last segment:
        3.0e-1 (the 8-block network);
      * the first padding row of g_k unmasked, for the first, middle and last block (only the
        bias partial moves: the row's partners in the K = Bp products are zero padding):
        3.9e-2 (biases, config 2; 4 x TOL = 1.6e-2).
    The last sample of every case carries noise at 4 sigma (denoiser_emulation.inputs): with
    unit noise, one sample among 1000 moves the gradients by only 1e-2 .. 5e-2, which 4 x TOL
    does not clear in every case.
"""
import contextlib
import functools

import pytest
import torch

from tests import denoiser_emulation as E

CASES = E.FUSED_CASES
IDS = [E.case_id(c) for c in CASES]
MOD_IDS = [E.case_id(c) for c in E.MODULAR_CASES]
# (a): about twice the largest deviation measured over the cases (docstring)
ORACLE_BOUND = {"weights": 1.7e-2, "biases": 1.1e-2, "loss": 1.3e-3, "dx": 6e-3}
MARGIN = 4.0


@contextlib.contextmanager
def _one_thread():
    """The fp32 products' summation order must not depend on how many CPUs the machine has."""
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        yield
    finally:
        torch.set_num_threads(n)


def _kinds(got, want):
    out = {}
    for n in want:
        k = "dx" if n == "dx" else E.kind(n)
        out[k] = max(out.get(k, 0.0), E.rel_dev(got[n], want[n]))
    return out


@functools.lru_cache(maxsize=None)
def _modular(case):
    """The modular path's inputs on the CPU: x_t, and deps from the emulated forward."""
    net, B, seed = case
    p, emb, sab, s1mab = E.oracle_net(net)
    x0, t, eps = E.inputs(B, net[2], seed)
    xt = E.q_sample_f32(sab, s1mab, x0, eps, t)
    eps_hat = E.forward(p, xt, t, emb)["eps_hat"]
    deps = (2.0 * (eps_hat - eps.double()) / (B * net[2])).float()
    return xt, t, eps, deps, E.fwd_bwd(p, emb, xt, t, deps)[1]


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_emulation_vs_fp64_oracle(case):
    """(a) the emulation is the oracle's network: loss and all gradients within ORACLE_BOUND."""
    from oracle import ref_cpu as R
    net, B, seed = case
    p, emb, _, _ = E.oracle_net(net)
    x0, t, eps = E.inputs(B, net[2], seed)
    loss, grads = E.fused_reference(case)
    want_loss, want = R.train_step_grads(p, R.ddpm_tables(), emb, x0.double(), eps.double(),
                                         t.long())
    assert set(want) == set(grads) - {"dx"}
    dev = _kinds(grads, want)
    dev["loss"] = abs(loss - float(want_loss)) / float(want_loss)
    print(f"{E.case_id(case)} emulation vs oracle: " +
          ", ".join(f"{k} {v:.2e}" for k, v in dev.items()))
    for k, v in dev.items():
        assert v <= ORACLE_BOUND[k], (k, v)


@pytest.mark.parametrize("case", E.MODULAR_CASES, ids=MOD_IDS)
def test_emulation_modular_vs_fp64_oracle(case):
    """(a) on the modular path: gradients and dx against fp64 autograd fed the same deps."""
    from oracle import ref_cpu as R
    net, B, seed = case
    p, emb, _, _ = E.oracle_net(net)
    xt, t, eps, deps, grads = _modular(case)
    params = p.map(lambda w: w.detach().clone().requires_grad_(True))
    x = xt.double().requires_grad_(True)
    with torch.enable_grad():
        R.denoiser_forward(params, x, t.long(), emb).backward(deps.double())
    want = {n: getattr(params, n).grad for n in ("Wt1", "bt1", "Wt2", "bt2", "Win", "bin", "Wout",
                                                 "bout")}
    for k in range(p.n_blocks):
        want[f"Wblk{k}"], want[f"bblk{k}"] = params.Wblk[k].grad, params.bblk[k].grad
    want["dx"] = x.grad
    dev = _kinds(grads, want)
    print(f"{E.case_id(case)} modular emulation vs oracle: " +
          ", ".join(f"{k} {v:.2e}" for k, v in dev.items()))
    for k, v in dev.items():
        assert v <= ORACLE_BOUND[k], (k, v)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_noise_floor_below_recorded(case):
    """(b) fp32-product emulation vs fp64-product emulation: every floor <= FLOOR = TOL / 4."""
    net, B, seed = case
    p, emb, sab, s1mab = E.oracle_net(net)
    x0, t, eps = E.inputs(B, net[2], seed)
    loss, grads = E.fused_reference(case)
    with _one_thread():
        loss32, g32 = E.train_step(p, sab, s1mab, emb, x0, eps, t, matmul_dtype=torch.float32)
    floor = _kinds(g32, grads)
    floor["loss"] = abs(loss32 - loss) / loss
    print(f"{E.case_id(case)} floor: " + ", ".join(f"{k} {v:.2e}" for k, v in floor.items()))
    for k, v in floor.items():
        assert v <= E.FLOOR[k], (k, v)
        assert E.TOL[k] == MARGIN * E.FLOOR[k]


@pytest.mark.parametrize("case", E.MODULAR_CASES, ids=MOD_IDS)
def test_noise_floor_modular_below_recorded(case):
    """(b) on the modular path (same fp32 deps into both)."""
    net, B, seed = case
    p, emb, _, _ = E.oracle_net(net)
    xt, t, eps, deps, grads = _modular(case)
    with _one_thread():
        g32 = E.fwd_bwd(p, emb, xt, t, deps, matmul_dtype=torch.float32)[1]
    floor = _kinds(g32, grads)
    print(f"{E.case_id(case)} modular floor: " +
          ", ".join(f"{k} {v:.2e}" for k, v in floor.items()))
    for k, v in floor.items():
        assert v <= E.FLOOR[k], (k, v)


def _segments(nb):
    return sorted({0, nb // 2, nb - 1})


def _assert_mutant_caught(label, mutant, ref, compared):
    """At least one compared tensor deviates by >= MARGIN x its tolerance."""
    dev = {n: E.rel_dev(mutant[n], ref[n]) for n in compared}
    ratio = {n: d / E.TOL["dx" if n == "dx" else E.kind(n)] for n, d in dev.items()}
    best = max(ratio, key=ratio.get)
    print(f"{label}: largest deviation / tolerance {ratio[best]:.1f} on {best} "
          f"({dev[best]:.2e})")
    assert ratio[best] >= MARGIN, (label, best, dev[best])


def _mutants(label, p, s, go, ref, compared):
    B = go.shape[0]
    drop = E.backward(p, s, go, mutate={"drop_sample": True})
    _assert_mutant_caught(f"{label} dropped last sample", drop, ref, compared)
    for k in _segments(p.n_blocks):
        _assert_mutant_caught(f"{label} dtemb segment {k} skipped",
                              E.backward(p, s, go, mutate={"skip_dtemb_seg": k}), ref, compared)
        assert B % 64 != 0          # the case has padding rows
        _assert_mutant_caught(f"{label} padding row of g_{k} unmasked",
                              E.backward(p, s, go, mutate={"pad_g": k}), ref, compared)
    for n in compared:
        if n != "dx" and E.kind(n) == E.WEIGHTS:
            row = int(ref[n].abs().amax(1).argsort()[ref[n].shape[0] // 2])
            _assert_mutant_caught(f"{label} row {row} of {n} zeroed", E.zero_row(ref, n, row),
                                  ref, [n])


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_mutants_exceed_tolerance(case):
    """(c) every mutant of the fused step lands >= 4 x TOL away on a tensor the step returns
    (dx is not an output of the fused step)."""
    p = E.oracle_net(case[0])[0]
    _, s, go = E.fused_state(case)
    _, ref = E.fused_reference(case)
    _mutants(E.case_id(case), p, s, go, ref, [n for n in ref if n != "dx"])


@pytest.mark.parametrize("case", E.MODULAR_CASES, ids=MOD_IDS)
def test_mutants_modular_exceed_tolerance(case):
    """(c) on the modular path, dx included."""
    net, B, seed = case
    p, emb, _, _ = E.oracle_net(net)
    xt, t, eps, deps, ref = _modular(case)
    s = E.forward(p, xt, t, emb)
    _mutants(E.case_id(case) + " modular", p, s, E.f32(deps), ref, list(ref))
