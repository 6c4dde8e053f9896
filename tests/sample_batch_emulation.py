"""CPU emulation of the batched sampling loop's arithmetic (TEST INFRASTRUCTURE).

Follows csrc/sample_batch.hip and the epilogues of csrc/gemm_tile.h, in the pattern of
tests/denoiser_emulation.py: the oracle's network (oracle/ref_cpu.py) with every GEMM operand
rounded to bf16 (RNE, from the fp32 value the device holds) exactly where the kernels round, and
nowhere else.  Everything else is fp64 except the A8 update, which is fp32 operation by operation
as on the device, so the result differs from the device only by the fp32 accumulation order and
the bf16 rounding ties that order flips downstream.  ``matmul_dtype=torch.float32`` runs the
products in fp32 (another summation order) to measure that noise floor on the CPU
(tests/test_sample_batch_emulation.py).

Rounding map (weights: the fp32 masters rounded to bf16; biases: the fp32 masters):

    E_k[t]  = bf(U_k) temb(t) + b_k, temb(t) = bf(Wt2) SiLU(bf(Wt1) e(t) + bt1) + bt2,
              activations unrounded, the table stored in fp32 (ldm_sdf.ops.build_e_tables)
    x as the in-projection operand : bf(x)           (x itself stays fp32 in the update)
    h_0     = bf(x) bf(Win)^T + bin                  fp32 stream + bf16 operand copy
    a_k     = bf(h_k) bf(W_k)^T + E_k[t]             fp32 accumulate, E_k[t] fp32
    h_{k+1} = h_k + SiLU(a_k)                        fp32 stream
    eps     = bf(h_nb) bf(Wout)^T + bout             rounded to fp32
    x'      = fl(fl(c1 fl(x - fl(c2 eps))) + fl(sigma z))   fp32, no contraction; z skipped at t = 0

``mutate`` applies one deliberate mistake (MUTANTS); the CPU test shows where each lands beyond
the GPU tolerance:
    "e_row"      E_k[t - 1] instead of E_k[t]  (E_k[1] at t = 0)
    "noise_row"  noise[t - 1] instead of noise[t]
    "z_at_0"     z applied at t = 0 too
    "drop_last"  the last live row is never written: it keeps its x_T
    "pad_leak"   a padding row leaks into row B - 1: its in-projection operand is the zero row
"""
from __future__ import annotations

import functools
from typing import Optional

import torch

from tests.denoiser_emulation import bf, f32, model_of, silu  # noqa: F401  (model_of: re-export)

MUTANTS = ("e_row", "noise_row", "z_at_0", "drop_last", "pad_leak")

# ---- the cases the GPU tests run ---------------------------------------------------------------
# a network is (n_blocks, H, D, TE); a case is (network, n, t_hi, steps)
NET_S = (2, 128, 64, 128)
NET_L = (4, 1024, 256, 128)
T = 1000
RUNS = [(999, 1), (500, 1), (1, 1), (0, 1), (999, 5), (999, 20)]     # (t_hi, steps)
PARITY_CASES = [(NET_S, n, t_hi, steps) for n in (17, 64, 65) for t_hi, steps in RUNS] + \
    [(NET_L, 17, t_hi, steps) for t_hi, steps in RUNS]
CROSS_CASE = (NET_L, 32, 999, 5)        # rows 0..15 against the existing sample(n = 16)

# Device tolerance, metric max|a - b| over the final latents (|x| is 4-6): 4 x the largest CPU
# noise floor (fp32-product emulation vs fp64-product emulation) over every parity case with
# that many steps.  FLOOR holds those largest floors, rounded up;
# tests/test_sample_batch_emulation.py re-measures them, asserts they stay below FLOOR, and
# asserts every mutant lands >= 2 x TOL away in every case that CLAIMS it.
FLOOR = {1: 8.0e-5, 5: 3.0e-4, 20: 1.0e-3}
TOL = {k: 4.0 * v for k, v in FLOOR.items()}
# The emulation's distance to the rounded-weight oracle with UNROUNDED activations (what the
# existing <= 16 kernels compute), CROSS_CASE rows 0..15, rounded up: the cost of rounding the
# activations to bf16.  The cross-path GPU test allows 4 x this.
ACT_ROUNDING = 5.0e-4


def claims(mutant: str, t_hi: int, steps: int) -> bool:
    """Whether the GPU parity case (t_hi, steps) relies on catching ``mutant``."""
    if mutant == "noise_row":
        return t_hi > 0                      # no noise is read in the t = 0 step
    if mutant == "z_at_0":
        return t_hi - steps + 1 == 0         # only a run that reaches t = 0
    return True


def case_id(case) -> str:
    (nb, H, D, TE), n, t_hi, steps = case
    return f"nb{nb}-H{H}-D{D}-n{n}-t{t_hi}-s{steps}"


@functools.lru_cache(maxsize=None)
def oracle_net(net):
    """(oracle parameters, fp64 embedding table, DDPM tables) of a network."""
    from oracle import ref_cpu as R
    nb, H, D, TE = net
    return (R.make_denoiser_params(D=D, H=H, n_blocks=nb, TE=TE, seed=4321),
            torch.from_numpy(R.timestep_embedding_table(T, TE)).double(), R.ddpm_tables(T))


@functools.lru_cache(maxsize=None)
def e_tables(net):
    """[E_k] fp32-valued fp64 [T][H]: the tabulated block biases from bf16-rounded weights."""
    p, emb, _ = oracle_net(net)
    H = p.H
    temb = silu(emb @ bf(p.Wt1).T + f32(p.bt1)) @ bf(p.Wt2).T + f32(p.bt2)
    return [f32(temb @ bf(p.Wblk[k])[:, H:].T + f32(p.bblk[k])) for k in range(p.n_blocks)]


def inputs(n: int, D: int, seed: int, t_hi: int = T - 1, steps: int = T):
    """(x_T [n, D], noise [T, n, D]) from a seeded host generator: unit normal; only the noise
    rows a run from ``t_hi`` over ``steps`` steps can read (and the row below, which the
    "noise_row" mutant reads) are drawn, the others are zero."""
    g = torch.Generator().manual_seed(seed)
    x_T = torch.randn(n, D, generator=g)
    noise = torch.zeros(T, n, D)
    lo = max(t_hi - steps, 0)
    noise[lo:t_hi + 1] = torch.randn(t_hi + 1 - lo, n, D, generator=g)
    return x_T, noise


def case_inputs(case):
    net, n, t_hi, steps = case
    return inputs(n, net[2], 1000 * n + 7 * t_hi + steps, t_hi, steps)


def sample(net, x_T: torch.Tensor, noise: torch.Tensor, t_hi: int, steps: int,
           matmul_dtype=torch.float64, mutate: Optional[str] = None,
           round_activations: bool = True) -> torch.Tensor:
    """The loop t_hi .. t_hi-steps+1 on x_T (fp32 values): the final x, fp32.
    ``round_activations=False``: the rounded-weight oracle with unrounded activations (what the
    <= 16 GEMV kernels compute)."""
    assert mutate is None or mutate in MUTANTS
    p, _, tab = oracle_net(net)
    E = e_tables(net)
    H = p.H
    rb = bf if round_activations else f32

    def mm(a, b):      # both operands hold bf16 values (exact in fp32); only the summation differs
        return (a.to(matmul_dtype) @ b.to(matmul_dtype)).double()

    Win, Wout = bf(p.Win), bf(p.Wout)
    Wk = [bf(w)[:, :H] for w in p.Wblk]
    c1t, c2t, sgt = (torch.from_numpy(tab.f32(k)) for k in ("c1", "c2", "sigma"))
    x = x_T.float().clone()
    for t in range(t_hi, t_hi - steps, -1):
        te = t if mutate != "e_row" else (t - 1 if t > 0 else 1)
        xb = rb(x)
        if mutate == "pad_leak":
            xb[-1] = 0.0
        h = mm(xb, Win.T) + f32(p.bin)
        for k in range(p.n_blocks):
            a = mm(rb(h), Wk[k].T) + E[k][te]
            h = h + silu(a)                      # the fp32 residual stream: unrounded
        eps = (mm(rb(h), Wout.T) + f32(p.bout)).float()
        y = c1t[t] * (x - c2t[t] * eps)          # fp32, one rounding per operation
        if t > 0 or mutate == "z_at_0":
            z = noise[t - 1 if (mutate == "noise_row" and t > 0) else t].float()
            y = y + sgt[t] * z
        if mutate == "drop_last":
            y[-1] = x_T[-1].float()
        x = y
    return x


@functools.lru_cache(maxsize=None)
def reference(case) -> torch.Tensor:
    """The fp64-product emulation of a case, computed once per process and shared (read-only)."""
    net, n, t_hi, steps = case
    x_T, noise = case_inputs(case)
    torch.set_num_threads(min(16, torch.get_num_threads()))
    return sample(net, x_T, noise, t_hi, steps)


def max_dev(a: torch.Tensor, b: torch.Tensor) -> float:
    return float((a.double() - b.double()).abs().max())
