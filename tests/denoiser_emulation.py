"""CPU emulation of the bf16 training step's arithmetic (TEST INFRASTRUCTURE).

Follows csrc/denoiser_train.hip forward() / backward() / finalize() and the epilogue of
csrc/gemm_tile.h: the oracle's network (oracle/ref_cpu.py) and its hand-written backward, with
every GEMM operand rounded to bf16 (RNE, from the fp32 value the device holds) exactly where
the kernels round, and nowhere else.  Everything else is fp64, so the result differs from the
device only by the fp32 accumulation order and the bf16 rounding ties that order flips
downstream.  ``matmul_dtype=torch.float32`` runs the products in fp32 (another summation order)
to measure that noise floor on the CPU (tests/test_train_emulation.py).

Rounding map (weights: the fp32 masters rounded to bf16; biases: the fp32 masters):

forward
    xt      = fl32(fl32(sqrt_ab[t] x0) + fl32(sqrt_1mab[t] eps))   (prep_inputs_kernel, no FMA)
    a_t     = bf(e) bf(Wt1)^T + bt1        fp32;   u = SiLU(a_t)   stored as bf16 only
    temb    = bf(u) bf(Wt2)^T + bt2        stored as bf16 only
    h_0     = bf(xt) bf(Win)^T + bin       fp32 residual stream + its bf16 copy (the operand)
    a_k     = bf(h_k) bf(W_k)^T + bf(temb) bf(U_k)^T + b_k   fp32;   h_{k+1} = h_k + SiLU(a_k)
    d       = bf(h_nb) bf(Wout)^T + bout - eps;   go = scale d, scale = fl32(2 / (B D))
    loss    = sum d^2 / (B D)
backward (g enters every product as bf16)
    dWout   = bf(go)^T bf(h_nb);           dh_nb = bf(go) bf(Wout)
    g_k     = dh_{k+1} SiLU'(a_k);         dW_k = bf(g_k)^T bf(h_k);  dU_k = bf(g_k)^T bf(temb)
    dh_k    = dh_{k+1} + bf(g_k) bf(W_k)   fp32 stream
    dtemb   = sum_k bf(g_k) bf(U_k)        one product over n_blocks K-segments, bf16 only
    dWt2    = bf(dtemb)^T bf(u);           gt = (bf(dtemb) bf(Wt2)) SiLU'(a_t)
    dWt1    = bf(gt)^T bf(e);  dWin = bf(dh_0)^T bf(xt);  dx = bf(dh_0) bf(Win)
    biases  = column sums of the epilogue's fp32 values BEFORE the bf16 pack:
              bout <- go, bblk_k <- g_k, bin <- dh_0, bt2 <- dtemb, bt1 <- gt
    modular path (ldm_denoiser_bwd, caller's fp32 deps): go = deps, bout <- deps itself.

``mutate`` applies one deliberate mistake to the emulation (the mistakes the whole-tensor cosine
checks let through); the CPU test shows each of them lands beyond the GPU tolerance:
    {"drop_sample": True}    the last live sample contributes to no gradient
    {"skip_dtemb_seg": k}    K-segment k of the dtemb product is skipped
    {"pad_g": k}             the first padding row of g_k is not masked (M_valid off by one): it
                             holds a copy of the last live row and enters the bias partial and
                             the K = Bp weight-gradient products
(zeroing one output row of a finished gradient needs no hook).
"""
from __future__ import annotations

import functools
from typing import Dict, Optional

import numpy as np
import torch

WEIGHTS, BIASES = "weights", "biases"

# Device tolerance per tensor kind, metric max|a - b| / max|b| per tensor: 4 x the largest CPU
# noise floor (fp32-product emulation vs fp64-product emulation) over every (network, B) the GPU
# tests use.  FLOOR holds those largest floors, rounded up; tests/test_train_emulation.py
# re-measures them, asserts they stay below FLOOR, and asserts every mutant lands >= 4 x TOL.
FLOOR = {"weights": 3.0e-3, "biases": 1.0e-3, "loss": 3.0e-6, "dx": 1.0e-3}
TOL = {k: 4.0 * v for k, v in FLOOR.items()}


def kind(name: str) -> str:
    return WEIGHTS if name.startswith("W") else BIASES


def rel_dev(a: torch.Tensor, b: torch.Tensor) -> float:
    """max|a - b| / max|b| (b: the reference)."""
    return float((a.double() - b.double()).abs().max()) / float(b.double().abs().max())


def bf(x: torch.Tensor) -> torch.Tensor:
    """RNE to bf16 from the fp32 value, back as fp64."""
    return x.float().bfloat16().double()


def f32(x: torch.Tensor) -> torch.Tensor:
    return x.float().double()


def silu(a: torch.Tensor) -> torch.Tensor:
    return a * torch.sigmoid(a)


def silu_grad(a: torch.Tensor) -> torch.Tensor:
    s = torch.sigmoid(a)
    return s * (1.0 + a * (1.0 - s))


def q_sample_f32(sqrt_ab: np.ndarray, sqrt_1mab: np.ndarray, x0: torch.Tensor,
                 eps: torch.Tensor, t: torch.Tensor) -> torch.Tensor:
    """x_t in fp32 as prep_inputs_kernel forms it: two rounded products, one rounded sum."""
    a = torch.from_numpy(sqrt_ab.astype(np.float32))[t.long()][:, None] * x0.float()
    e = torch.from_numpy(sqrt_1mab.astype(np.float32))[t.long()][:, None] * eps.float()
    return a + e


def _mm(matmul_dtype):
    def mm(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
        # both operands hold bf16 values (exact in fp32); only the summation differs
        return (a.to(matmul_dtype) @ b.to(matmul_dtype)).double()
    return mm


def forward(p, xt: torch.Tensor, t: torch.Tensor, emb: torch.Tensor,
            matmul_dtype=torch.float64) -> Dict[str, object]:
    """The forward on x_t (fp32 values) with per-sample t; returns eps_hat and what the backward
    reads (the device's saved workspace)."""
    mm = _mm(matmul_dtype)
    H = p.H
    s = {"xt_b": bf(xt), "e_b": bf(emb[t.long()])}
    s["a_t"] = mm(s["e_b"], bf(p.Wt1).T) + f32(p.bt1)
    s["u_b"] = bf(silu(s["a_t"]))
    s["temb_b"] = bf(mm(s["u_b"], bf(p.Wt2).T) + f32(p.bt2))
    h = mm(s["xt_b"], bf(p.Win).T) + f32(p.bin)
    s["h_b"], s["a"] = [bf(h)], []
    for k in range(p.n_blocks):
        W = bf(p.Wblk[k])
        a = mm(s["h_b"][k], W[:, :H].T) + mm(s["temb_b"], W[:, H:].T) + f32(p.bblk[k])
        h = h + silu(a)                          # the fp32 residual stream: unrounded
        s["a"].append(a)
        s["h_b"].append(bf(h))
    s["eps_hat"] = mm(s["h_b"][-1], bf(p.Wout).T) + f32(p.bout)
    return s


def backward(p, s: Dict[str, object], go: torch.Tensor, matmul_dtype=torch.float64,
             mutate: Optional[dict] = None) -> Dict[str, torch.Tensor]:
    """Every gradient (named as MLPDenoiser.names()) and dx from go = dL/d eps_hat (fp32
    values, the epilogue's or the caller's deps)."""
    mm = _mm(matmul_dtype)
    mutate = mutate or {}
    H, nb = p.H, p.n_blocks
    go = go.double()
    if mutate.get("drop_sample"):
        go = go.clone()
        go[-1] = 0.0
    pad_k = mutate.get("pad_g", -1)
    g = {}
    go_b = bf(go)
    g["bout"] = go.sum(0)
    g["Wout"] = mm(go_b.T, s["h_b"][nb])
    dh = mm(go_b, bf(p.Wout))
    gk_b = [None] * nb
    for k in range(nb - 1, -1, -1):
        gk = dh * silu_grad(s["a"][k])
        # the mutant's padding row of g_k: its partners in the K = Bp products (h_k, temb) are 0
        # in padding, so only the bias partial moves
        g[f"bblk{k}"] = gk.sum(0) + (gk[-1] if k == pad_k else 0.0)
        gk_b[k] = bf(gk)
        W = bf(p.Wblk[k])
        g[f"Wblk{k}"] = torch.cat([mm(gk_b[k].T, s["h_b"][k]), mm(gk_b[k].T, s["temb_b"])], 1)
        dh = dh + mm(gk_b[k], W[:, :H])
    g["bin"] = dh.sum(0)
    dh0_b = bf(dh)
    skip = mutate.get("skip_dtemb_seg", -1)
    segs = [k for k in range(nb) if k != skip]
    if segs:                                     # ONE product over the K-segments
        dtemb = mm(torch.cat([gk_b[k] for k in segs], 1),
                   torch.cat([bf(p.Wblk[k])[:, H:] for k in segs], 0))
    else:
        dtemb = torch.zeros_like(dh)
    g["bt2"] = dtemb.sum(0)
    dtemb_b = bf(dtemb)
    g["Wt2"] = mm(dtemb_b.T, s["u_b"])
    gt = mm(dtemb_b, bf(p.Wt2)) * silu_grad(s["a_t"])
    g["bt1"] = gt.sum(0)
    g["Wt1"] = mm(bf(gt).T, s["e_b"])
    g["Win"] = mm(dh0_b.T, s["xt_b"])
    g["dx"] = mm(dh0_b, bf(p.Win))
    return g


def prepare(p, sqrt_ab: np.ndarray, sqrt_1mab: np.ndarray, emb: torch.Tensor,
            x0: torch.Tensor, eps: torch.Tensor, t: torch.Tensor, matmul_dtype=torch.float64):
    """The fused step up to the LOSS epilogue: (loss, saved state, go)."""
    B, D = x0.shape
    xt = q_sample_f32(sqrt_ab, sqrt_1mab, x0, eps, t)
    s = forward(p, xt, t, emb, matmul_dtype)
    d = s["eps_hat"] - f32(eps)
    n = np.float32(B) * np.float32(D)
    loss = float((d * d).sum()) / float(n)
    go = float(np.float32(2.0) / n) * d
    return loss, s, go


def train_step(p, sqrt_ab: np.ndarray, sqrt_1mab: np.ndarray, emb: torch.Tensor,
               x0: torch.Tensor, eps: torch.Tensor, t: torch.Tensor,
               matmul_dtype=torch.float64, mutate: Optional[dict] = None):
    """The fused step (ldm_denoiser_train_step): (loss, {name: grad, "dx": dx})."""
    loss, s, go = prepare(p, sqrt_ab, sqrt_1mab, emb, x0, eps, t, matmul_dtype)
    return loss, backward(p, s, go, matmul_dtype, mutate)


def fwd_bwd(p, emb: torch.Tensor, xt: torch.Tensor, t: torch.Tensor, deps: torch.Tensor,
            matmul_dtype=torch.float64, mutate: Optional[dict] = None):
    """The modular path (ldm_denoiser_fwd on x_t, ldm_denoiser_bwd on the caller's fp32 deps):
    (eps_hat, {name: grad, "dx": dx})."""
    s = forward(p, xt, t, emb, matmul_dtype)
    return s["eps_hat"], backward(p, s, f32(deps), matmul_dtype, mutate)


def zero_row(grads: Dict[str, torch.Tensor], name: str, row: int) -> Dict[str, torch.Tensor]:
    """The 'one output row of a weight gradient is zeroed' mutant."""
    out = dict(grads)
    out[name] = grads[name].clone()
    out[name][row] = 0.0
    return out


def inputs(B: int, D: int, seed: int, outlier: float = 4.0):
    """(x0, t, eps) of one step: latents at the synthetic scale 0.5, uniform t, unit noise.  The
    LAST sample's noise is scaled by ``outlier``: its residual, and so its share of every
    gradient, is a few times a typical sample's, which keeps a step that loses the last live row
    (or lets the padding row after it in) >= 4 x the tolerance away even among 1000 samples."""
    g = torch.Generator().manual_seed(seed)
    x0 = torch.randn(B, D, generator=g) * 0.5
    t = torch.randint(0, 1000, (B,), generator=g, dtype=torch.int32)
    eps = torch.randn(B, D, generator=g)
    eps[-1] *= outlier
    return x0, t, eps


# ---- the cases the GPU tests run (and whose floors / mutants the CPU test measures) ----------
# a network is (n_blocks, H, D, TE); a case is (network, B, input seed)
DEFAULT_NET = (4, 1024, 256, 128)
OTHER_NETS = [(1, 256, 128, 64), (2, 512, 64, 128), (8, 256, 256, 64)]
CONFIG2_CASE = (DEFAULT_NET, 1000, 2024)
FUSED_CASES = [(DEFAULT_NET, B, 100 + B) for B in (1, 37, 65, 200, 1000)] + \
    [(net, 200, 300 + net[0]) for net in OTHER_NETS] + [CONFIG2_CASE]
MODULAR_CASES = [(DEFAULT_NET, 65, 165), (DEFAULT_NET, 200, 300)]


def case_id(case) -> str:
    (nb, H, D, TE), B, seed = case
    return f"nb{nb}-H{H}-D{D}-TE{TE}-B{B}-s{seed}"


@functools.lru_cache(maxsize=None)
def oracle_net(net):
    """(oracle parameters, fp64 embedding table, fp32 sqrt_ab, fp32 sqrt_1mab) of a network."""
    from oracle import ref_cpu as R
    nb, H, D, TE = net
    tab = R.ddpm_tables()
    return (R.make_denoiser_params(D=D, H=H, n_blocks=nb, TE=TE, seed=4321),
            torch.from_numpy(R.timestep_embedding_table(1000, TE)).double(),
            tab.f32("sqrt_ab"), tab.f32("sqrt_1mab"))


def model_of(p):
    """The oracle's parameters as an ldm_sdf.MLPDenoiser (fp32 masters)."""
    from ldm_sdf import MLPDenoiser
    params = {n: getattr(p, n) for n in ("Wt1", "bt1", "Wt2", "bt2", "Win", "bin", "Wout", "bout")}
    for k in range(p.n_blocks):
        params[f"Wblk{k}"], params[f"bblk{k}"] = p.Wblk[k], p.bblk[k]
    return MLPDenoiser(D=p.D, H=p.H, n_blocks=p.n_blocks, TE=p.TE, params=params)


@functools.lru_cache(maxsize=None)
def fused_state(case):
    """(loss, saved state, go) of a fused case's fp64 emulation, computed once per process."""
    net, B, seed = case
    p, emb, sab, s1mab = oracle_net(net)
    x0, t, eps = inputs(B, net[2], seed)
    torch.set_num_threads(min(16, torch.get_num_threads()))
    return prepare(p, sab, s1mab, emb, x0, eps, t)


@functools.lru_cache(maxsize=None)
def fused_reference(case):
    """(loss, {name: grad, "dx": dx}) of a fused case: the fp64 emulation, computed once per
    process and shared (read-only) by the tests that compare against it."""
    loss, s, go = fused_state(case)
    return loss, backward(oracle_net(case[0])[0], s, go)


def check_against(got_loss, got: Dict[str, torch.Tensor], want_loss, want: Dict[str, torch.Tensor],
                  label: str) -> Dict[str, float]:
    """Element-wise comparison at TOL: prints every figure first, then asserts.  Returns the
    largest deviation per tensor kind."""
    worst = {}
    rows = []
    if got_loss is not None:
        worst["loss"] = abs(float(got_loss) - float(want_loss)) / abs(float(want_loss))
        rows.append(("loss", "loss", worst["loss"], True))
    for n, g in got.items():
        k = "dx" if n == "dx" else kind(n)
        finite = bool(torch.isfinite(g).all())
        d = rel_dev(g.detach().cpu(), want[n]) if finite else float("inf")
        worst[k] = max(worst.get(k, 0.0), d)
        rows.append((n, k, d, finite))
    for n, k, d, finite in rows:
        print(f"{label} {n}: max|dev|/max|ref| {d:.2e} (tol {TOL[k]:.1e})")
    print(f"{label} worst per kind: " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()))
    bad = [(n, d) for n, k, d, finite in rows if not finite or not d <= TOL[k]]
    assert not bad, (label, bad)
    return worst
