"""CPU emulation of the bf16 auto-decoder training step's arithmetic (TEST INFRASTRUCTURE).

Follows ldm_sdf/autodecoder.py::_train_step_gemm_bf16, the epilogue of csrc/gemm_tile.h (modes
RELU and RELU_BWD, the 32-row column sums of keep[], the bf16 pack) and sdf_l1_term /
latent_reg_kernel of csrc/autodecoder.hip: the oracle's network (oracle/ref_autodecoder.py) and a
hand-written backward, with every GEMM operand rounded to bf16 (RNE, from the fp32 value the
device holds) exactly where the kernels round, and nowhere else.  Everything else is fp64, so the
result differs from the device only by the fp32 accumulation order and the bf16 rounding ties
that order flips downstream.  ``matmul_dtype=torch.float32`` accumulates the products in fp32
(another summation order, fixed: 32-wide K chunks) to measure that noise floor on the CPU
(tests/test_autodecoder_emulation.py).

Rounding map (W_l, b_l: the fp32 masters; bf(W_l): their bf16 working copies; N = S P samples,
shape-major; hs = 253 the skip width, L = 256):

forward
    Zx      = bf([z_s || xyz])                        one row per sample
    h_l     = bf(relu(fl32(h_{l-1} bf(W_l)^T + b_l)))         l = 0..7, h_{-1} = Zx
    layer 4 = two K segments of one product: h_3 bf(W_4[:, :hs])^T + Zx bf(W_4[:, hs:])^T
    layer 3's three padding columns (253 -> 256) are zero weights and biases: they add nothing
    pre     = h_7 bf(W_8)^T + b_8                     fp32, never rounded to bf16
loss (sdf_l1_term on the fp32 pre; delta and scale = 1 / N are fp32 values)
    pred    = tanh(pre);  diff = clamp(pred, delta) - clamp(sdf, delta)
    loss    = scale sum |diff| + coef sum_s |z_s|,    coef = lambda min(1, epoch / 100) / S
    g_8     = scale sign(diff) (1 - pred^2) if -delta <= pred <= delta (inclusive), else 0
backward (g enters every product as bf16)
    db_8    = sum g_8 (unrounded);  dW_8 = bf(g_8)^T h_7;  g_7 = [h_7 > 0] (bf(g_8) bf(W_8))
    dW_l    = bf(g_l)^T h_{l-1}     (l = 0 and the second half of layer 4: Zx),  l = 7..0
    db_l    = column sum of the fp32 g_l BEFORE the bf16 pack (32-row partials of keep[])
    g_{l-1} = [h_{l-1} > 0] (bf(g_l) bf(W_l))         l = 4: only the W_4[:, :hs] columns
latent gradient (an fp32 product on the fp32 MASTERS, not the bf16 copies)
    gz      = G_4 W_4[:, hs:hs+L] + G_0 W_0[:, :L] + coef z_s / |z_s|
    G_l     = per-shape sum of the fp32 g_l when P % 32 == 0 (colsum_segments of the partials),
              of the bf16-ROUNDED g_l otherwise (the one-hot split-K product)

``mutate`` applies one deliberate mistake to the emulation (the mistakes the whole-tensor cosine
checks let through); the CPU test shows each of them lands beyond the GPU tolerance:
    {"drop_kblock": (name, k)}   k-block k (KT samples, one split-K slice) is left out of the
                                 weight-gradient sum ``name`` (W0..W3, W4h, W4z, W5..W8)
    {"drop_sample": True}        the last live sample contributes to nothing
    {"drop_bias_partial": l}     the last 32-row partial that holds live rows (the ragged one
                                 when N % 32 != 0) is left out of db_l
    {"straddle": True}           the 32-row block that straddles shapes 0 / 1 is counted wholly
                                 to shape 0 in G_4 and G_0
(zeroing one output row of a finished gradient, and cutting the W4z gradient from the padded
offset, need no hook: zero_row, w4z_from_padded_offset).
"""
from __future__ import annotations

import functools
from typing import Dict, Optional

import numpy as np
import torch

WEIGHTS, BIASES, Z = "weights", "biases", "z"
L, H, SKIP = 256, 512, 4
CLAMP_DIST = 0.1
CODE_REG_LAMBDA = 1e-4
_KQ = 128                  # ldm_sdf.autodecoder._KQ: row padding of the sample axis

# Device tolerance per tensor kind, metric max|a - b| / max|b| per tensor: 4 x the largest CPU
# noise floor (fp32-product emulation vs fp64-product emulation) over CASES.  FLOOR holds those
# largest floors, rounded up; tests/test_autodecoder_emulation.py re-measures them, asserts they
# stay below FLOOR, and asserts every mutant lands >= 4 x TOL (a zeroed row: >= 2 x TOL).
FLOOR = {"weights": 5.0e-3, "biases": 3.5e-3, "z": 5.0e-3, "loss": 2.5e-5}
TOL = {k: 4.0 * v for k, v in FLOOR.items()}

# Input construction: every kept sample's reference tanh(pre) stays MARGIN away from +-delta,
# and inside the band |clamp(pred) - clamp(sdf)| >= MARGIN, so no summation order flips a
# sample's gradient.  MARGIN >= 4 x the largest |pre| deviation between the fp32-product and the
# fp64-product forward over CASES (measured: tests/test_autodecoder_emulation.py).
MARGIN = 5e-3
TARGET_RADIUS = 0.5        # sdf = 0.3 (|xyz| - TARGET_RADIUS)
_OUT = 64                  # candidates for the outlier sample
W8_SCALE = 0.25            # the master W8: keeps >= 90 % of the samples inside the clamp band


def kind(name: str) -> str:
    return WEIGHTS if name.startswith("W") else BIASES if name.startswith("b") else Z


def rel_dev(a: torch.Tensor, b: torch.Tensor) -> float:
    """max|a - b| / max|b| (b: the reference)."""
    return float((a.double() - b.double()).abs().max()) / float(b.double().abs().max())


def bf(x: torch.Tensor) -> torch.Tensor:
    """RNE to bf16 from the fp32 value, back as fp64."""
    return x.float().bfloat16().double()


def f32(x: torch.Tensor) -> torch.Tensor:
    return x.float().double()


_KCHUNK = 32


def _mm(matmul_dtype):
    """fp64: one fp64 product.  fp32: fp32 accumulation in a FIXED order -- the K axis in chunks
    of 32, each chunk's partial product formed in fp64 and rounded to fp32, the partials added
    in fp32 in ascending order -- so the measured floor does not depend on the machine's BLAS."""
    def mm(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
        if matmul_dtype == torch.float64:
            return a.double() @ b.double()
        acc = None
        for k0 in range(0, a.shape[1], _KCHUNK):
            part = (a[:, k0:k0 + _KCHUNK].double() @ b[k0:k0 + _KCHUNK].double()).float()
            acc = part if acc is None else acc + part
        return acc.double()
    return mm


def layout(S: int, P: int) -> Dict[str, int]:
    """The step's padding and blocking of the sample axis (autodecoder.py): N, Np, KT, nblk."""
    N = S * P
    Np = -(-N // _KQ) * _KQ
    KT = next(kt for kt in (8192, 4096, 2048, 1024, 512, 256, 128) if Np % kt == 0)
    return {"N": N, "Np": Np, "KT": KT, "nblk": Np // KT}


def forward(p, z: torch.Tensor, xyz: torch.Tensor, matmul_dtype=torch.float64):
    """The forward on z [S, L], xyz [S, P, 3] (fp32 values): what the backward reads (Zx, the
    bf16 post-activations h, the bf16 weights) and pre [N]."""
    mm = _mm(matmul_dtype)
    S, P, _ = xyz.shape
    W = [f32(w) for w in p.weights]
    b = [f32(x) for x in p.biases]
    Wb = [bf(w) for w in W]
    hs = W[SKIP - 1].shape[0]
    Zx = bf(torch.cat([f32(z)[:, None, :].expand(S, P, L), f32(xyz)], 2).reshape(S * P, L + 3))
    h, x = [], Zx
    for l in range(8):
        if l == SKIP:
            a = mm(x, Wb[l][:, :hs].T) + mm(Zx, Wb[l][:, hs:].T) + b[l]
        else:
            a = mm(x, Wb[l].T) + b[l]
        x = bf(torch.relu(a))
        h.append(x)
    pre = (mm(x, Wb[8].T) + b[8]).reshape(-1)
    return {"S": S, "P": P, "hs": hs, "W": W, "Wb": Wb, "Zx": Zx, "h": h, "pre": pre, "z": f32(z)}


def loss_terms(pre: torch.Tensor, sdf: torch.Tensor, delta: float = CLAMP_DIST):
    """sdf_l1_term: (scale sum |diff|, g8 [N]) on pre [N], sdf [N]."""
    d = float(np.float32(delta))
    scale = float(np.float32(1.0 / pre.numel()))
    pred = torch.tanh(pre)
    diff = pred.clamp(-d, d) - f32(sdf).reshape(-1).clamp(-d, d)
    inside = (pred >= -d) & (pred <= d)
    g8 = torch.where(inside, scale * torch.sign(diff) * (1.0 - pred * pred), torch.zeros_like(pre))
    return scale * float(diff.abs().sum()), g8


def backward(s, g8: torch.Tensor, matmul_dtype=torch.float64, mutate: Optional[dict] = None,
             reg_lambda: float = CODE_REG_LAMBDA, epoch: int = 100) -> Dict[str, torch.Tensor]:
    """Every gradient (``W{l}``, ``b{l}``, ``z``) from g8 = dL/d pre (fp32 values)."""
    mm = _mm(matmul_dtype)
    mutate = mutate or {}
    S, P, hs, W, Wb, Zx, h = s["S"], s["P"], s["hs"], s["W"], s["Wb"], s["Zx"], s["h"]
    N = S * P
    KT = layout(S, P)["KT"]
    g8 = g8.double().reshape(N, 1)
    if mutate.get("drop_sample"):
        g8 = g8.clone()
        g8[-1] = 0.0

    def wgrad(name, gb, x):
        if mutate.get("drop_kblock", (None, 0))[0] == name:
            k = mutate["drop_kblock"][1]
            gb = gb.clone()
            gb[k * KT:(k + 1) * KT] = 0.0
        return mm(gb.T, x)

    def colsum(l, g):
        out = g.sum(0)
        if mutate.get("drop_bias_partial", -1) == l:
            out = out - g[32 * ((N - 1) // 32):].sum(0)
        return out

    owner = torch.arange(N) // P
    if mutate.get("straddle"):
        assert S > 1 and P % 32 != 0
        owner[32 * (P // 32):32 * (P // 32) + 32] = 0

    def per_shape(g, gb):
        src = g if P % 32 == 0 else gb           # colsum_segments of the fp32 partials / one-hot
        return torch.zeros(S, src.shape[1], dtype=torch.float64).index_add_(0, owner, src)

    out = {}
    gb = bf(g8)
    out["b8"] = g8.sum(0)
    out["W8"] = wgrad("W8", gb, h[7])
    g = torch.where(h[7] > 0, mm(gb, Wb[8]), torch.zeros_like(h[7]))
    G = {}
    for l in range(7, -1, -1):
        gb = bf(g)
        out[f"b{l}"] = colsum(l, g)
        if l == SKIP:
            out[f"W{l}"] = torch.cat([wgrad("W4h", gb, h[l - 1]), wgrad("W4z", gb, Zx)], 1)
        else:
            out[f"W{l}"] = wgrad(f"W{l}", gb, Zx if l == 0 else h[l - 1])
        if l in (SKIP, 0):
            G[l] = per_shape(g, gb)
        if l > 0:
            Wd = Wb[l][:, :hs] if l == SKIP else Wb[l]
            g = torch.where(h[l - 1] > 0, mm(gb, Wd), torch.zeros_like(h[l - 1]))
    gz = mm(G[SKIP], W[SKIP][:, hs:hs + L]) + mm(G[0], W[0][:, :L])
    coef = reg_lambda * min(1.0, epoch / 100.0) / S
    nrm = s["z"].norm(dim=1, keepdim=True)
    out["z"] = gz + coef * s["z"] / nrm.clamp_min(1e-300)
    return out


def reg_loss(z: torch.Tensor, reg_lambda: float = CODE_REG_LAMBDA, epoch: int = 100) -> float:
    return reg_lambda * min(1.0, epoch / 100.0) / z.shape[0] * float(f32(z).norm(dim=1).sum())


def train_step(p, z, xyz, sdf, matmul_dtype=torch.float64, mutate: Optional[dict] = None,
               reg_lambda: float = CODE_REG_LAMBDA, epoch: int = 100):
    """The step (autodecoder_train_step, dtype="bf16"): (loss, {name: grad}, pre)."""
    s = forward(p, z, xyz, matmul_dtype)
    l1, g8 = loss_terms(s["pre"], sdf)
    grads = backward(s, g8, matmul_dtype, mutate, reg_lambda, epoch)
    return l1 + reg_loss(z, reg_lambda, epoch), grads, s["pre"]


def zero_row(grads: Dict[str, torch.Tensor], name: str, row: int) -> Dict[str, torch.Tensor]:
    """The 'one output row of a weight gradient is zeroed' mutant."""
    out = dict(grads)
    out[name] = grads[name].clone()
    out[name][row] = 0.0
    return out


def w4z_from_padded_offset(grads: Dict[str, torch.Tensor], hs: int) -> Dict[str, torch.Tensor]:
    """The 'W4z gradient cut at the wrong offset' mutant: the skip layer's gradient is
    [dW4h (hs columns, padded to hsp) || dW4z]; the master's [:, hs:] block must come from
    offset hsp of that, not hs (which gives the padding's zero columns, then dW4z shifted)."""
    hsp = -(-hs // 64) * 64
    out = dict(grads)
    W4 = grads[f"W{SKIP}"]
    padded = torch.cat([W4[:, :hs], torch.zeros(W4.shape[0], hsp - hs, dtype=W4.dtype),
                        W4[:, hs:]], 1)
    out[f"W{SKIP}"] = torch.cat([W4[:, :hs], padded[:, hs:hs + L + 3]], 1)
    return out


# ---- the cases the GPU tests run (and whose floors / mutants the CPU test measures) ----------
# a case is (S, P, seed, outlier): the last live sample lies on a cube up to outlier x the unit
# cube, which makes its share of the weight gradients several times a typical sample's, so that
# a step that loses it lands >= 4 x TOL away.  Seeds: the floors move with the seed (one flipped
# tie in a heavy sample), these are the lowest of the few tried per case.
CASE_1x64 = (1, 64, 21, 6.0)
CASE_5x96 = (5, 96, 42, 6.0)
CASE_3x256 = (3, 256, 23, 8.0)
CASE_3x200 = (3, 200, 54, 10.0)
CASE_2x129 = (2, 129, 45, 4.0)
CASE_320xP = (320, 72, 26, 6.0)
CASES = [CASE_1x64, CASE_5x96, CASE_3x256, CASE_3x200, CASE_2x129, CASE_320xP]
FP32_CASE = (3, 129, 27, 3.0)      # the fp32 step test (not a bf16 case: no floor of its own)


def case_id(case) -> str:
    return f"S{case[0]}-P{case[1]}-s{case[2]}"


@functools.lru_cache(maxsize=None)
def inputs(case):
    """(p, z, xyz, sdf, stats) of a case, deterministic, CPU only.  p: the oracle's DeepSDF
    8 x 512 decoder (He-normal, seed) with fp32-representable values and W8 scaled by W8_SCALE;
    z [S, L] ~ N(0, 1/256); xyz [S, P, 3]; sdf [S, P] = 0.3 (|xyz| - 0.5).  Per shape the
    points are the first P of a seeded pool (uniform in the unit cube) whose reference (fp64
    emulation) tanh(pre) is >= MARGIN from +-delta and, inside the band, whose
    |clamp(pred) - clamp(sdf)| >= MARGIN; the last sample of the last shape comes from a pool
    on cubes shrinking from ``outlier`` x the unit cube, under the same rule, and must lie
    inside the band (it carries gradient).  stats: 'rejected' (share of the examined candidates not kept), 'live' (share of
    kept samples inside the band), 'gap' (smallest distance to a discontinuity)."""
    from oracle import ref_cpu as R
    S, P, seed, outlier = case
    torch.set_num_threads(min(16, torch.get_num_threads()))
    p = R.make_decoder_params(seed=seed)
    p.weights[8] = p.weights[8] * W8_SCALE
    p = R.DecoderParams(p.latent_dim, p.hidden, p.n_hidden, p.skip, p.widen_skip,
                        [f32(w) for w in p.weights], [f32(b) for b in p.biases])
    assert (p.latent_dim, p.hidden, p.skip) == (L, H, SKIP)
    g = torch.Generator().manual_seed(seed)
    z = (torch.randn(S, L, generator=g, dtype=torch.float64) / 16).float()
    M = 2 * P + _OUT
    pool = (torch.rand(S, M, 3, generator=g, dtype=torch.float64) * 2 - 1).float()
    # the last shape's last-sample candidates: on the surface of a cube, outlier x the unit
    # cube for the first, shrinking towards it (the first admissible one is the heaviest)
    scale = 1.0 + (outlier - 1.0) * (1.0 - torch.arange(_OUT) / _OUT)
    pool[-1, -_OUT:] *= (scale / pool[-1, -_OUT:].abs().amax(1))[:, None]

    def target(x):
        return ((x.double().norm(dim=-1) - TARGET_RADIUS) * 0.3).float()

    d = float(np.float32(CLAMP_DIST))
    fwd = forward(p, z, pool)
    pred = torch.tanh(fwd["pre"]).reshape(S, M)
    tgt = target(pool)
    edge = torch.minimum((pred - d).abs(), (pred + d).abs())
    inside = pred.abs() <= d
    tie = (pred.clamp(-d, d) - tgt.double().clamp(-d, d)).abs()
    gap = torch.where(inside, torch.minimum(edge, tie), edge)
    ok = gap >= MARGIN
    xyz = torch.empty(S, P, 3)
    examined = kept = 0
    for sidx in range(S):
        n_body = P - 1 if sidx == S - 1 else P
        idx = torch.nonzero(ok[sidx, :M - _OUT]).reshape(-1)[:n_body]
        assert idx.numel() == n_body, "candidate pool exhausted"
        xyz[sidx, :n_body] = pool[sidx, idx]
        examined += (int(idx[-1]) + 1) if n_body else 0
        kept += n_body
    last = torch.nonzero(ok[-1, M - _OUT:] & inside[-1, M - _OUT:]).reshape(-1)
    assert last.numel() > 0, "no admissible outlier sample"
    xyz[-1, -1] = pool[-1, M - _OUT + int(last[0])]
    examined += int(last[0]) + 1
    kept += 1
    sdf = target(xyz)
    fwd = forward(p, z, xyz)
    pred = torch.tanh(fwd["pre"])
    tie = (pred.clamp(-d, d) - sdf.double().reshape(-1).clamp(-d, d)).abs()
    edge = torch.minimum((pred - d).abs(), (pred + d).abs())
    live = pred.abs() <= d
    stats = {"rejected": 1.0 - kept / examined, "live": float(live.double().mean()),
             "gap": float(torch.where(live, torch.minimum(edge, tie), edge).min())}
    return p, z, xyz, sdf, stats


@functools.lru_cache(maxsize=None)
def state(case):
    """(saved forward state, g8, loss) of a case's fp64 emulation, computed once per process."""
    p, z, xyz, sdf, _ = inputs(case)
    s = forward(p, z, xyz)
    l1, g8 = loss_terms(s["pre"], sdf)
    return s, g8, l1 + reg_loss(z)


@functools.lru_cache(maxsize=None)
def reference(case):
    """(loss, {name: grad}) of a case: the fp64 emulation, computed once per process and shared
    (read-only) by the tests that compare against it."""
    s, g8, loss = state(case)
    return loss, backward(s, g8)


def masters(p, dev) -> Dict[str, torch.Tensor]:
    """The oracle's parameters as autodecoder_train_step's fp32 masters on ``dev``."""
    m = {}
    for l in range(9):
        m[f"W{l}"] = p.weights[l].float().to(dev)
        m[f"b{l}"] = p.biases[l].float().to(dev)
    return m


def check_against(got_loss, got: Dict[str, torch.Tensor], want_loss, want: Dict[str, torch.Tensor],
                  label: str, tol: Optional[Dict[str, float]] = None) -> Dict[str, float]:
    """Element-wise comparison of the loss and EVERY tensor of ``want`` at TOL: prints every
    figure first, then asserts.  Returns the largest deviation per tensor kind."""
    tol = tol or TOL
    assert set(got) == set(want), (sorted(got), sorted(want))
    worst = {"loss": abs(float(got_loss) - float(want_loss)) / abs(float(want_loss))}
    rows = [("loss", "loss", worst["loss"], True)]
    for n in want:
        k = kind(n)
        t = got[n].detach().cpu()
        assert tuple(t.shape) == tuple(want[n].shape), (n, tuple(t.shape))
        finite = bool(torch.isfinite(t).all())
        d = rel_dev(t, want[n]) if finite else float("inf")
        worst[k] = max(worst.get(k, 0.0), d)
        rows.append((n, k, d, finite))
    for n, k, d, finite in rows:
        print(f"{label} {n}: max|dev|/max|ref| {d:.2e} (tol {tol[k]:.1e})")
    print(f"{label} worst per kind: " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()))
    bad = [(n, d) for n, k, d, finite in rows if not finite or not d <= tol[k]]
    assert not bad, (label, bad)
    return worst
