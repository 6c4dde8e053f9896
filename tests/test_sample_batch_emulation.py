"""CPU checks of tests/sample_batch_emulation.py, the reference of the batched sampling loop's
GPU tests (tests/test_gpu_sample_batch.py): for every (network, n, t_hi, steps) those tests run,

  * the noise floor -- the emulation with fp32 products against the one with fp64 products:
    another summation order and the bf16 ties it flips -- stays below FLOOR[steps], so the GPU
    tolerance TOL = 4 x FLOOR is 4 x a measured quantity, not a guess;
  * every deliberate mistake (MUTANTS) lands at least 2 x TOL away in every case that claims it
    (sample_batch_emulation.claims): wrong E row and dropped / leaked last row everywhere, wrong
    noise row wherever noise is read, z at t = 0 in the t = 0 step.  Every mutant separates at
    every step count, 20 included, so no claim is withdrawn;
  * the distance to the rounded-weight oracle with unrounded activations, which the existing
    <= 16 kernels compute, stays below ACT_ROUNDING on the cross-path case.

Figures of record (max |difference| of the final latents, this file's own measurement; the
single-step floor of the default network is one flipped bf16 tie, not accumulated rounding):
  floor, largest per step count      1: 7.0e-5    5: 2.7e-4    20: 8.4e-4
  closest claimed mutant, in TOL     1: 2.6 (e_row, small net, t = 1)   5: 6.7 (e_row)
                                     20: 2.8 (e_row, default net); every other mutant >= 200
  rounded vs unrounded activations   4.4e-4; a wrong E row against the unrounded oracle: 7.4e-3
"""
import pytest
import torch

from tests import sample_batch_emulation as E


@pytest.mark.parametrize("case", E.PARITY_CASES, ids=E.case_id)
def test_floor_and_mutants(case):
    net, n, t_hi, steps = case
    x_T, noise = E.case_inputs(case)
    ref = E.reference(case)
    assert bool(torch.isfinite(ref).all()) and ref.shape == x_T.shape
    floor = E.max_dev(E.sample(net, x_T, noise, t_hi, steps, matmul_dtype=torch.float32), ref)
    print(f"{E.case_id(case)} floor {floor:.2e} (FLOOR {E.FLOOR[steps]:.1e}) "
          f"max|x| {float(ref.abs().max()):.2f}")
    dist = {}
    for m in E.MUTANTS:
        if E.claims(m, t_hi, steps):
            dist[m] = E.max_dev(E.sample(net, x_T, noise, t_hi, steps, mutate=m), ref)
            print(f"{E.case_id(case)} mutant {m}: {dist[m]:.2e} = {dist[m] / E.TOL[steps]:.1f} TOL")
    assert floor <= E.FLOOR[steps]
    bad = {m: d for m, d in dist.items() if not d >= 2.0 * E.TOL[steps]}
    assert not bad, bad


def test_unclaimed_mutants_are_noops():
    """The two claims that are withheld are withheld because the mutant changes nothing there."""
    case = (E.NET_S, 17, 0, 1)
    x_T, noise = E.case_inputs(case)
    assert torch.equal(E.sample(E.NET_S, x_T, noise, 0, 1, mutate="noise_row"), E.reference(case))
    case = (E.NET_S, 17, 999, 5)
    x_T, noise = E.case_inputs(case)
    assert torch.equal(E.sample(E.NET_S, x_T, noise, 999, 5, mutate="z_at_0"), E.reference(case))


def test_activation_rounding():
    net, n, t_hi, steps = E.CROSS_CASE
    x_T, noise = E.case_inputs(E.CROSS_CASE)
    a = E.reference(E.CROSS_CASE)[:16]
    b = E.sample(net, x_T[:16], noise[:, :16], t_hi, steps, round_activations=False)
    d = E.max_dev(a, b)
    print(f"{E.case_id(E.CROSS_CASE)} rounded vs unrounded activations: {d:.2e} "
          f"(ACT_ROUNDING {E.ACT_ROUNDING:.1e})")
    assert d <= E.ACT_ROUNDING
    # the bound separates the two paths from a wrong E row on this case as well
    m = E.max_dev(E.sample(net, x_T, noise, t_hi, steps, mutate="e_row")[:16], b)
    print(f"  e_row mutant vs the unrounded oracle: {m:.2e}")
    assert m >= 4.0 * E.ACT_ROUNDING


def test_emulation_matches_the_oracle_loop_without_rounding():
    """With nothing rounded but the weights, the emulation is oracle.ref_cpu.sample_loop on the
    rounded-weight network (the reference today's <= 16 tests use), to fp32 resolution."""
    from oracle import ref_cpu as R
    p, emb, tab = E.oracle_net(E.NET_S)
    x_T, noise = E.inputs(5, E.NET_S[2], 3, E.T - 1, 3)
    pr = p.map(lambda w: w.float().bfloat16().double() if w.dim() == 2 else w.float().double())
    want = R.sample_loop(pr, tab, emb, x_T.double(), noise.double(), steps=3)
    got = E.sample(E.NET_S, x_T, noise, E.T - 1, 3, round_activations=False)
    assert E.max_dev(got, want) < 2e-5
