"""The reference of the element-wise bf16 auto-decoder gradient tests, tested on the CPU.

tests/autodecoder_emulation.py restates the bf16 auto-decoder step
(ldm_sdf/autodecoder.py::_train_step_gemm_bf16) in plain torch with the kernels' bf16 operand
roundings; tests/test_gpu_autodecoder.py compares the device with it element by element.  Here,
with no GPU, for every case those tests run (metric per tensor: max|a - b| / max|b|; kinds:
weights W0..W8, biases b0..b8, z, relative loss):

(a) the fp64 emulation against the fp64 oracle's autograd (oracle/ref_autodecoder.py): the
    emulation is the same network, bf16 operand rounding apart.  Measured over the cases: weights
    1.1e-2 .. 2.1e-1 (1 x 64), biases 7.4e-3 .. 1.1e-1, z 1.8e-2 .. 5.1e-2, loss <= 9.8e-4, cosine
    >= 0.9972 per tensor; asserted at about twice the largest (ORACLE_BOUND).
(b) the noise floor: the emulation with fp32 accumulation in a fixed order (32-wide K chunks
    added in fp32, so the figure does not depend on the machine's BLAS or CPU count) against the
    one with fp64 products -- an fp32 summation order and the bf16 rounding ties it flips
    downstream, which is all that separates the device from the fp64 emulation too.  Measured:

        case (S x P, seed)   weights   biases    z         loss      max |pre| deviation
        1 x 64     s21       4.1e-4    2.9e-4    1.4e-4    2.0e-5    4.2e-5
        5 x 96     s42       2.0e-3    1.2e-3    1.4e-3    6.4e-6    2.3e-4
        3 x 256    s23       1.8e-3    1.5e-3    1.2e-3    5.7e-6    2.4e-4
        3 x 200    s54       1.8e-3    2.3e-3    1.2e-3    2.7e-6    2.6e-4
        2 x 129    s45       4.7e-3    3.1e-3    2.1e-3    4.5e-6    2.1e-4
        320 x 72   s26       4.7e-4    3.4e-4    4.2e-3    1.6e-7    4.9e-4

    autodecoder_emulation.FLOOR holds the largest per kind, rounded up (weights 5.0e-3, biases
    3.5e-3, z 5.0e-3, loss 2.5e-5) and the device tolerance is TOL = 4 x FLOOR (weights 2.0e-2,
    biases 1.4e-2, z 2.0e-2, loss 1.0e-4): the device's summation order is a third order, and
    tie flips are discrete.  Asserted: every measured floor <= FLOOR.
    The floor is one draw of a heavy-tailed figure: one flipped tie in a heavy sample's
    activations moves that sample's whole contribution by a bf16 ulp, and at small N one sample
    is a large share.  Over a dozen seeds, and with a BLAS fp32 order instead of the fixed one,
    the same cases gave weights 4e-4 .. 2e-2 at 1 x 64 and 2.5e-3 .. 1.0e-2 at 2 x 129 and
    3 x 200.  The seeds above are the ones with the lowest floors among those tried, so TOL is on
    the tight side of that spread; the 4 x margin is what covers the device's own draw.
    The z floor is set by the 320-shape case (few samples per shape, 320 x 256 entries to take
    the maximum over); at P = 40 it was 9e-3, hence P = 72.
    Inputs (asserted per case): 100 % of the samples inside the clamp band (>= 90 % required),
    0.8 .. 8.6 % of the candidates rejected (<= 25 %), every sample >= MARGIN = 5e-3 from a
    discontinuity of the loss, and 4 x the largest |pre| deviation (4.9e-4) <= MARGIN.
    The fp32 step test's inputs (3 x 129): the oracle in fp32 vs fp64 deviates by 4.1e-7
    element-wise, below a quarter of 1e-4, so that test asserts the project's 1e-4.
(c) mutants of the reference -- the mistakes the whole-tensor cosine checks let through -- each
    land >= 4 x TOL away on at least one tensor (smallest deviation / TOL over the cases):
      * one k-block (KT samples, one split-K slice) left out of dW0, dW4h, dW4z or dW8 -- the
        first, the middle and the last block at least half of whose rows are live: 8.0 (dW8,
        3 x 200).  Cases with 1 < nblk and N <= 1024; in the 320 x 72 case a block is 1 / 45 of
        the samples (2 % of a gradient that adds up coherently), below 4 x TOL = 8 % by
        construction, as is one sample of 23 040;
      * the last live sample (4 .. 10 x outside the unit cube) contributes to nothing: 4.4 (W0,
        3 x 256).  Cases with N <= 1024;
      * the ragged last 32-row partial left out of db0: 4.3 (3 x 200, 24 rows of 600).  The
        deeper biases add up more coherently and the same partial stays below 4 x TOL on
        some of them (seen on b4, b6, b7); the 2-row ragged partial of 2 x 129 is 0.8 % of the rows and cannot show;
      * the 32-row block that straddles shapes 0 / 1 counted wholly to shape 0 in G4 / G0: 5.9
        (z, 3 x 200; cases with P % 32 != 0);
      * the W4z gradient cut from the padded offset hsp instead of hs: 34.3 (W4, 320 x 72);
      * one output row of a weight gradient zeroed, for EVERY weight tensor, the row of median
        magnitude: 3.2 (W6 at 2 x 129 and 320 x 72) .. 50 (W8 has one row).  A median row of the deep layers is
        only 6 .. 8 % of the tensor's largest element, whatever the seed or the outlier, so
        this mutant is held to 2 x TOL on the tensor itself: after a device noise of a whole
        TOL in the other direction it is still outside TOL.
"""
import contextlib

import pytest
import torch

from tests import autodecoder_emulation as E

CASES = E.CASES
IDS = [E.case_id(c) for c in CASES]
# (a): about twice the largest deviation measured over the cases (docstring)
ORACLE_BOUND = {"weights": 0.4, "biases": 0.2, "z": 0.1, "loss": 2e-3}
MARGIN = 4.0
SMALL_N = 1024          # up to here one sample / one k-block is a visible share of a gradient
ROW_MARGIN = 2.0        # zeroed-row mutants: still > TOL away after a device noise of TOL
NAMES = [f"W{l}" for l in range(9)] + [f"b{l}" for l in range(9)] + ["z"]


@contextlib.contextmanager
def _one_thread():
    """torch's own fp32 kernels (the fp32 oracle run) must not depend on the CPU count."""
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        yield
    finally:
        torch.set_num_threads(n)


def _kinds(got, want):
    out = {}
    for n in want:
        out[E.kind(n)] = max(out.get(E.kind(n), 0.0), E.rel_dev(got[n], want[n]))
    return out


@pytest.mark.parametrize("case", CASES + [E.FP32_CASE], ids=IDS + [E.case_id(E.FP32_CASE)])
def test_inputs_clear_of_the_discontinuities(case):
    """The constructed inputs: >= 90 % of the samples inside the clamp band (they carry
    gradient), every sample >= MARGIN from a discontinuity of the loss, the pool rejects at most
    25 % of the candidates, and the last sample is the outlier inside the band."""
    p, z, xyz, sdf, stats = E.inputs(case)
    S, P = case[0], case[1]
    print(f"{E.case_id(case)} inputs: live {stats['live']:.3f}, rejected {stats['rejected']:.3f}, "
          f"smallest gap {stats['gap']:.2e}")
    assert tuple(xyz.shape) == (S, P, 3) and tuple(sdf.shape) == (S, P) and tuple(z.shape) == (S, E.L)
    assert stats["live"] >= 0.90
    assert stats["rejected"] <= 0.25
    assert stats["gap"] >= E.MARGIN
    assert float(xyz[-1, -1].abs().max()) > 1.0 >= float(xyz.reshape(-1, 3)[:-1].abs().max())
    s, g8, _ = E.state(case) if case in CASES else (None, E.loss_terms(
        E.forward(p, z, xyz)["pre"], sdf)[1], None)
    assert float(g8[-1].abs()) > 0.0


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_emulation_vs_fp64_oracle(case):
    """(a) the emulation is the oracle's network: loss and all gradients within ORACLE_BOUND."""
    from oracle import ref_autodecoder as A
    p, z, xyz, sdf, _ = E.inputs(case)
    loss, grads = E.reference(case)
    want_loss, want = A.autodecoder_grads(p, z.double(), xyz.double(), sdf.double())
    assert set(want) == set(grads) == set(NAMES)
    dev = _kinds(grads, want)
    dev["loss"] = abs(loss - want_loss) / want_loss
    cos = min(float(grads[n].flatten() @ want[n].flatten() /
                    (grads[n].norm() * want[n].norm())) for n in NAMES)
    print(f"{E.case_id(case)} emulation vs oracle: " +
          ", ".join(f"{k} {v:.2e}" for k, v in dev.items()) + f", smallest cosine {cos:.4f}")
    for k, v in dev.items():
        assert v <= ORACLE_BOUND[k], (k, v)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_noise_floor_below_recorded(case):
    """(b) fp32-product emulation vs fp64-product emulation: every floor <= FLOOR = TOL / 4, and
    the input margin covers 4 x the largest |pre| deviation."""
    p, z, xyz, sdf, _ = E.inputs(case)
    loss, grads = E.reference(case)
    with _one_thread():
        loss32, g32, pre32 = E.train_step(p, z, xyz, sdf, matmul_dtype=torch.float32)
    floor = _kinds(g32, grads)
    floor["loss"] = abs(loss32 - loss) / loss
    pre_dev = float((pre32 - E.state(case)[0]["pre"]).abs().max())
    print(f"{E.case_id(case)} floor: " + ", ".join(f"{k} {v:.2e}" for k, v in floor.items()) +
          f", max |pre| deviation {pre_dev:.2e}")
    assert set(floor) == set(E.FLOOR)
    for k, v in floor.items():
        assert v <= E.FLOOR[k], (k, v)
        assert E.TOL[k] == MARGIN * E.FLOOR[k]
    assert 4.0 * pre_dev <= E.MARGIN, pre_dev


def test_fp32_oracle_floor():
    """The fp32 step test's bound: the oracle's autograd in fp32 against fp64 on that test's
    inputs stays below a quarter of 1e-4 element-wise, so the project's 1e-4 holds there."""
    from oracle import ref_autodecoder as A
    p, z, xyz, sdf, _ = E.inputs(E.FP32_CASE)
    _, want = A.autodecoder_grads(p, z.double(), xyz.double(), sdf.double(), reg_lambda=1e-2)
    with _one_thread():
        _, got = A.autodecoder_grads(p.to(torch.float32), z, xyz, sdf, reg_lambda=1e-2)
    worst = max(E.rel_dev(got[n], want[n]) for n in NAMES)
    print(f"fp32 oracle vs fp64 oracle: largest element-wise deviation {worst:.2e}")
    assert worst <= 0.25 * 1e-4


def _ratio(label, mutant, ref, compared=NAMES):
    """(label, the largest deviation / tolerance over the compared tensors, tensor, deviation)."""
    dev = {n: E.rel_dev(mutant[n], ref[n]) for n in compared}
    ratio = {n: d / E.TOL[E.kind(n)] for n, d in dev.items()}
    best = max(ratio, key=ratio.get)
    return label, ratio[best], best, dev[best]


def mutant_ratios(case):
    """Every mutant of (c) on one case: [(label, deviation / tolerance, tensor, deviation)]."""
    S, P = case[0], case[1]
    lay = E.layout(S, P)
    N, KT, nblk = lay["N"], lay["KT"], lay["nblk"]
    s, g8, _ = E.state(case)
    _, ref = E.reference(case)
    out = []
    if N <= SMALL_N:
        out.append(_ratio("last live sample dropped",
                          E.backward(s, g8, mutate={"drop_sample": True}), ref))
    if nblk > 1 and N <= SMALL_N:                     # split-K: one slice left out of the sum
        last = (N - KT // 2) // KT     # the last k-block at least half of whose rows are live
        for name in ("W0", "W4h", "W4z", "W8"):
            for k in sorted({0, last // 2, last}):
                out.append(_ratio(f"k-block {k} left out of d{name}",
                                  E.backward(s, g8, mutate={"drop_kblock": (name, k)}), ref))
    for l in ((0,) if N % 32 >= 8 else ()):
        out.append(_ratio(f"last 32-row partial left out of db{l}",
                          E.backward(s, g8, mutate={"drop_bias_partial": l}), ref))
    if S > 1 and P % 32 != 0:
        out.append(_ratio("straddling block counted to shape 0",
                          E.backward(s, g8, mutate={"straddle": True}), ref))
    for n in NAMES:
        if E.kind(n) == E.WEIGHTS:
            row = int(ref[n].abs().amax(1).argsort()[ref[n].shape[0] // 2])
            out.append(_ratio(f"row {row} of {n} zeroed", E.zero_row(ref, n, row), ref, [n])
                       + (ROW_MARGIN,))
    out.append(_ratio("W4z gradient cut from the padded offset",
                      E.w4z_from_padded_offset(ref, s["hs"]), ref))
    return out


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_mutants_exceed_tolerance(case):
    """(c) every mutant lands >= 4 x TOL (zeroed rows: >= 2 x TOL on the tensor itself) away on
    a tensor the GPU test of the case compares (it compares all of them)."""
    rows = mutant_ratios(case)
    for label, r, best, d, *need in rows:
        print(f"{E.case_id(case)} {label}: largest deviation / tolerance {r:.1f} on {best} "
              f"({d:.2e})")
    missed = [(label, best, d) for label, r, best, d, *need in rows
              if not r >= (need[0] if need else MARGIN)]
    assert not missed, missed
