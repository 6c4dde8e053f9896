"""CPU emulation of the frozen-decoder gradient kernel's arithmetic (TEST INFRASTRUCTURE).

Follows csrc/decoder_grad.hip: the oracle's network (oracle/ref_cpu.py) and a hand-written
backward, in fp64, with every operand rounded where the kernel rounds and nowhere else.  What is
left between this and the device is the fp32 summation order and the rounding ties / ReLU sign
flips that order causes downstream.  ``matmul_dtype=torch.float32`` accumulates every product in
fp32 in a FIXED order (32-wide K chunks, as tests/autodecoder_emulation.py) to measure that floor
on the CPU (tests/test_decoder_grad_emulation.py).

Rounding map (T = fp16 / bf16, rd = RNE to T from the fp32 value, W_l the fp32 weights):
    beta    = fl32(wz z + bz)                      summed exactly (the device: fp64), rounded once
    a_0     = fma chain beta_0 + Wxyz_0 xyz        fp32 (x, y, z in that order), nothing in T
    a_l     = rd(W_l) rd(relu(a_{l-1})) + b_l      fp32 accumulation starting from the fp32 bias;
                                                   l = 4: from the fp32 chain beta_4 + Wxyz_4 xyz
    pre     = w_last . relu(a_7) + b_last          fp32 weights, a_7 unrounded
    m_l     = [a_l > 0]
    delta_7 = m_7 . w_last
    delta_{l-1} = m_{l-1} . (rd(W_l)^T rd(delta_l))      l = 7..1; l = 4: the h columns only
    dxyz    = s_p (Wxyz_0^T delta_0 + Wxyz_4^T delta_4)   from the unrounded deltas
    dbeta_i = sum_p s_p delta_i,p                  per tile of 64 points, then the tiles in order
    dz      = fl32(wz_0^T dbeta_0 + wz_4^T dbeta_4)       summed exactly, rounded once
    s_p     = 1 - f_p^2 (one rounding), f = fl32(tanh(pre)); loss mode: sdf_l1_term's d / d pre
    loss    = scale sum_p |clamp(f_p) - clamp(gt_p)|

``mutate`` applies one deliberate mistake (the ones a whole-tensor check lets through); the CPU
test shows each lands beyond the device tolerance on at least one output:
    "ragged_tail"    the clamped duplicate of a shape's last point, which fills a ragged tile, is
                     counted once into dbeta
    "drop_last_tile" the last tile of every shape is left out of dbeta
    "l4_full"        layer 4's backward runs over the z || xyz columns too: their products land
                     on the first L + 3 (at most skip-width) rows of delta_3
    "mask_shift"     m_5 is taken from layer 6
    "no_xyz4"        delta_4's xyz term is left out of dxyz
"""
from __future__ import annotations

from typing import Dict, Optional

import numpy as np
import torch

TILE = 64                  # csrc/decoder_grad.hip kGTp
_KCHUNK = 32
H, SKIP = 512, 4
DTYPES = {"fp16": torch.float16, "bf16": torch.bfloat16}
MUTANTS = ("ragged_tail", "drop_last_tile", "l4_full", "mask_shift", "no_xyz4")

# A point whose dxyz differs from the reference's by more than FLIP_REL (2-norm, relative) counts
# as flipped: some ReLU unit changed sign and the piecewise-constant gradient jumped.
FLIP_REL = 1e-3

# Floors: the largest deviation between the fp32-chunk and the fp64-product emulation over
# cases() x P in {1, 63, 65, 197} x both modes, rounded up (tests/test_decoder_grad_emulation.py
# re-measures them and asserts they stay below).  "sdf": max abs; "flipped": the share of flipped
# points (P >= 63); "dxyz": the largest relative deviation among the other points; "dbeta", "dz":
# max|a - b| / max|b|; "loss": relative, P >= 63 (see loss_tol).
# Measured worst case:   sdf      flipped  dxyz     dbeta    dz       loss
#                 fp16   1.0e-3   3.2 %    9.8e-4   2.6e-3   1.6e-3   1.1e-5
#                 bf16   4.1e-3   6.2 %    1.0e-3   2.8e-3   3.9e-3   8.9e-5
FLOOR = {
    "fp16": {"sdf": 1.2e-3, "flipped": 0.035, "dxyz": 1.0e-3, "dbeta": 3.0e-3, "dz": 2.0e-3,
             "loss": 3.0e-5},
    "bf16": {"sdf": 5.0e-3, "flipped": 0.065, "dxyz": 1.0e-3, "dbeta": 3.0e-3, "dz": 4.5e-3,
             "loss": 1.0e-4},
}
# Device tolerance: 4 x the floor (the device's summation order is a third, equally valid one).
TOL = {dt: {k: 4.0 * v for k, v in f.items()} for dt, f in FLOOR.items()}
# The share of a case's points (3 shapes x P in {1, 63, 65, 197} together, 978 points) whose dxyz
# lies beyond TOL["dxyz"] = 4e-3 of the reference -- the criterion the GPU parity test uses --
# measured between the two emulations: fp16 1.6 - 2.15 %, bf16 1.1 - 1.5 % per case, rounded up
# (tests/test_decoder_grad_emulation.py re-measures it).  One case of eight, fp16 / widen-skip /
# RMS 0.65, has 21 points of 978 beyond, 2 over the 2 % the feature's issue asked of the inputs.
BEYOND_TOL_SHARE = {"fp16": 0.022, "bf16": 0.016}
# ... and the share a GPU test may set aside: 4 x that, at most 8 % (fp16: 8 %, 3.7 x the worst
# case and 4.6 - 4.9 x the other three; bf16: 6.4 %)
FLIP_CAP = {dt: min(4.0 * v, 0.08) for dt, v in BEYOND_TOL_SHARE.items()}


def loss_tol(dtype: str, loss_ref: float, n_points: int) -> float:
    """Absolute tolerance of the loss.  The loss is the mean of |clamp f - clamp gt| over the
    points, so it moves by at most the largest |delta f|: TOL sdf.  From 3 x 63 points on, the
    mean holds the measured relative floor, which is far tighter."""
    return TOL[dtype]["sdf"] if n_points < 3 * 63 else TOL[dtype]["loss"] * abs(loss_ref)


def f32(x: torch.Tensor) -> torch.Tensor:
    return x.float().double()


def rd(x: torch.Tensor, dt: torch.dtype) -> torch.Tensor:
    return x.float().to(dt).double()


def rel_dev(a: torch.Tensor, b: torch.Tensor) -> float:
    """max|a - b| / max|b| (b: the reference)."""
    return float((a.double() - b.double()).abs().max()) / max(float(b.double().abs().max()), 1e-300)


def _mm(matmul_dtype):
    """acc + a @ b.  fp64: one fp64 product.  fp32: the K axis in chunks of 32, each chunk's
    partial formed in fp64 and rounded to fp32, added to the fp32 accumulator in order."""
    def mm(a, b, acc=None):
        if matmul_dtype == torch.float64:
            r = a.double() @ b.double()
            return r if acc is None else r + acc
        out = None if acc is None else acc.float()
        for k0 in range(0, a.shape[1], _KCHUNK):
            part = (a[:, k0:k0 + _KCHUNK].double() @ b[k0:k0 + _KCHUNK].double()).float()
            out = part if out is None else out + part
        return out.double()
    return mm


def _chain(beta, wxyz, x3):
    """fp32 fma chain beta + wx x + wy y + wz z (one rounding per step): [P, H]."""
    v = beta[None, :].expand(x3.shape[0], -1)
    for ax in range(3):
        v = f32(v + wxyz[None, :, ax] * x3[:, ax:ax + 1])
    return v


def pieces(p) -> Dict[str, object]:
    """The decoder's fp32 weights split as the kernel sees them (fp64 tensors of fp32 values)."""
    L = p.latent_dim
    W = [f32(w) for w in p.weights]
    b = [f32(x) for x in p.biases]
    hs = W[SKIP - 1].shape[0]
    return {"L": L, "hs": hs, "W": W, "b": b,
            "wz": [W[0][:, :L], W[SKIP][:, hs:hs + L]],
            "wxyz": [W[0][:, L:L + 3], W[SKIP][:, hs + L:hs + L + 3]],
            "w_last": W[8][0], "b_last": b[8][0]}


def emulate(p, z: torch.Tensor, xyz: torch.Tensor, dtype: str, *, gt: Optional[torch.Tensor] = None,
            delta: float = 1.0, matmul_dtype=torch.float64, mutate: Optional[str] = None,
            tile: int = TILE) -> Dict[str, torch.Tensor]:
    """z [B, L], xyz [B, P, 3] (fp32 values) -> sdf [B, P], dxyz [B, P, 3], dbeta [B, 2, H],
    dz [B, L], s [B, P] and, with gt [B, P] (loss mode, scale = 1 / (B P)), loss."""
    assert mutate is None or mutate in MUTANTS
    dt = DTYPES[dtype]
    mm = _mm(matmul_dtype)
    q = pieces(p)
    L, hs, W, b = q["L"], q["hs"], q["W"], q["b"]
    B, P, _ = xyz.shape
    zz = f32(z)
    beta = [f32(zz @ q["wz"][i].T + b[(0, SKIP)[i]]) for i in range(2)]       # [B, H] each
    Wr = [None] + [rd(W[l][:, :hs] if l == SKIP else W[l], dt) for l in range(1, 8)]
    d32 = float(np.float32(delta))
    scale = float(np.float32(1.0 / (B * P)))
    out = {k: [] for k in ("sdf", "dxyz", "dbeta", "s", "margin", "masks")}
    loss = 0.0
    for s_i in range(B):
        x3 = f32(xyz[s_i])
        a = _chain(beta[0][s_i], q["wxyz"][0], x3)
        masks = [a > 0]
        margin = a.abs().min(dim=1).values
        for l in range(1, 8):
            h = rd(torch.relu(a), dt)
            init = _chain(beta[1][s_i], q["wxyz"][1], x3) if l == SKIP \
                else b[l][None, :].expand(P, -1)
            a = mm(h, Wr[l].T, init)
            masks.append(a > 0)
            margin = torch.minimum(margin, a.abs().min(dim=1).values)
        pre = mm(torch.relu(a), q["w_last"][:, None])[:, 0] + q["b_last"]
        f = f32(torch.tanh(pre))
        if gt is None:
            s = f32(1.0 - f * f)
        else:
            g = f32(gt[s_i])
            diff = f.clamp(-d32, d32) - g.clamp(-d32, d32)
            s = torch.where((f >= -d32) & (f <= d32), scale * torch.sign(diff) * (1.0 - f * f),
                            torch.zeros_like(f))
            loss = loss + diff.abs().sum()
        d = masks[7].double() * q["w_last"][None, :]
        deltas = {}
        for l in range(7, 0, -1):
            m = masks[l - 1]
            if mutate == "mask_shift" and l - 1 == 5:
                m = masks[6]
            nd = mm(rd(d, dt), Wr[l])
            if mutate == "l4_full" and l == SKIP:
                extra = rd(d, dt) @ rd(W[SKIP][:, hs:], dt)          # the z || xyz columns
                n = min(hs, extra.shape[1])
                nd = nd.clone()
                nd[:, :n] += extra[:, :n]
            d = m.double() * nd
            if l - 1 in (0, SKIP):
                deltas[l - 1] = d
        g4 = deltas[SKIP] @ q["wxyz"][1]
        if mutate == "no_xyz4":
            g4 = torch.zeros_like(g4)
        dxyz = s[:, None] * (deltas[0] @ q["wxyz"][0] + g4)
        db = []
        for li in (0, SKIP):
            sd = s[:, None] * deltas[li]
            tiles = [sd[t0:t0 + tile].sum(0) for t0 in range(0, P, tile)]
            if mutate == "ragged_tail" and P % tile:
                tiles[-1] = tiles[-1] + sd[-1]
            if mutate == "drop_last_tile":
                tiles[-1] = torch.zeros_like(tiles[-1])
            if matmul_dtype == torch.float64:
                db.append(torch.stack(tiles).sum(0))
            else:
                acc = tiles[0].float()
                for t in tiles[1:]:
                    acc = acc + t.float()
                db.append(acc.double())
        out["sdf"].append(f)
        out["dxyz"].append(dxyz)
        out["dbeta"].append(torch.stack(db))
        out["s"].append(s)
        out["margin"].append(margin)
        out["masks"].append(torch.cat(masks, dim=1))
    res = {k: torch.stack(v) for k, v in out.items()}
    dbf = f32(res["dbeta"])
    res["dz"] = f32(dbf[:, 0] @ q["wz"][0] + dbf[:, 1] @ q["wz"][1])
    if gt is not None:
        res["loss"] = torch.as_tensor(scale * float(loss), dtype=torch.float64)
    return res


def compare(got: Dict[str, torch.Tensor], ref: Dict[str, torch.Tensor]) -> Dict[str, float]:
    """The metrics FLOOR / TOL are stated in, ``got`` against ``ref``."""
    dg, dr = got["dxyz"].double().reshape(-1, 3), ref["dxyz"].double().reshape(-1, 3)
    rel = (dg - dr).norm(dim=1) / dr.norm(dim=1).clamp_min(1e-30)
    keep = rel <= FLIP_REL
    m = {"sdf": float((got["sdf"].double() - ref["sdf"].double()).abs().max()),
         "flipped": float((~keep).double().mean()),
         "dxyz": float(rel[keep].max()) if bool(keep.any()) else 0.0,
         "dbeta": rel_dev(got["dbeta"], ref["dbeta"]), "dz": rel_dev(got["dz"], ref["dz"])}
    if "loss" in ref:
        m["loss"] = abs(float(got["loss"]) - float(ref["loss"])) / abs(float(ref["loss"]))
    return m


def flipped_share(got_dxyz: torch.Tensor, ref_dxyz: torch.Tensor, tol: float) -> float:
    """Share of points whose dxyz is further than ``tol`` (2-norm, relative) from the reference."""
    dg, dr = got_dxyz.double().reshape(-1, 3), ref_dxyz.double().reshape(-1, 3)
    rel = (dg - dr).norm(dim=1) / dr.norm(dim=1).clamp_min(1e-30)
    return float((rel > tol).double().mean())


# ------------------------------------------------------------------------------------- inputs
def make_params(kind: str):
    """The two test decoders (seed 1234): "deepsdf" (L = 256, skip width 253) and "widen"
    (L = 1024, widen-skip, skip width 512).  fp32-representable weights."""
    from oracle import ref_cpu as R
    p = R.make_decoder_params(seed=1234) if kind == "deepsdf" else \
        R.make_decoder_params(L=1024, widen_skip=True, seed=1234)
    return p.to(torch.float32).to(torch.float64)


def make_inputs(p, B: int, P: int, rms: float, seed: int = 100):
    """Latents (seed 100) normalised to ``rms`` per shape, uniform points, and a target field
    0.3 (|x| - 0.5) for the loss mode.  fp32 tensors."""
    g = torch.Generator().manual_seed(seed)
    z = torch.randn(B, p.latent_dim, generator=g, dtype=torch.float64)
    z = z * (rms / z.pow(2).mean(dim=1, keepdim=True).sqrt())
    xyz = torch.rand(B, P, 3, generator=g, dtype=torch.float64) * 2 - 1
    gt = 0.3 * (xyz.norm(dim=2) - 0.5)
    return z.float(), xyz.float(), gt.float()


def cases():
    """(decoder kind, latent RMS) of the parity tests."""
    return [(k, r) for k in ("deepsdf", "widen") for r in (0.2, 0.65)]


# ------------------------------------------------------------------- fit_latents trajectory
FIT = dict(S=2, n=2048, steps=50, lr=5e-3, delta=1.0, reg_lambda=1e-4, init_std=0.01,
           target_rms=0.3)


def fit_case(p):
    """The frozen-decoder fit of the GPU test: 2 shapes x 2048 uniform points whose SDF the fp64
    oracle decoder produces from known latents (seed 7, RMS 0.3); codes start at N(0, 0.01^2)
    (seed 8).  fp32 tensors (z_true, xyz, sdf, z0)."""
    from oracle import ref_cpu as R
    g = torch.Generator().manual_seed(7)
    zt = torch.randn(FIT["S"], p.latent_dim, generator=g, dtype=torch.float64)
    zt = zt * (FIT["target_rms"] / zt.pow(2).mean(dim=1, keepdim=True).sqrt())
    xyz = (torch.rand(FIT["S"], FIT["n"], 3, generator=g, dtype=torch.float64) * 2 - 1).float()
    sdf = R.decoder_forward(p, zt.float().double(), xyz.double()).float()
    z0 = (torch.randn(FIT["S"], p.latent_dim, generator=torch.Generator().manual_seed(8))
          * FIT["init_std"]).float()
    return zt.float(), xyz, sdf, z0


def oracle_fit(p, xyz, sdf, z0, steps=None):
    """fit_latents' loop on the fp64 oracle: autodecoder_loss at epoch 100, torch Adam, the
    learning rate divided by 10 at steps // 2, all samples every step.  Returns (z, losses)."""
    from oracle import ref_autodecoder as RA
    steps = FIT["steps"] if steps is None else steps
    z = z0.double().clone().requires_grad_(True)
    opt = torch.optim.Adam([z], lr=FIT["lr"])
    losses = []
    for step in range(steps):
        if step == steps // 2 and step > 0:
            for g in opt.param_groups:
                g["lr"] = FIT["lr"] / 10.0
        opt.zero_grad()
        loss = RA.autodecoder_loss(p, z, xyz.double(), sdf.double(), FIT["delta"],
                                   FIT["reg_lambda"], 100)
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    return z.detach(), losses


# Recorded CPU measurements the GPU tests hold the device to (each re-measured by
# tests/test_decoder_grad_emulation.py, which asserts the record is not below the measurement and
# not more than 1.5 x above it):
# max|dz - oracle| / max|oracle|, fp64-product emulation against autodecoder_grads' z (loss
# mode, delta 1, reg_lambda 0) on make_inputs(deepsdf, 3, 197, 0.2): 4.2e-3 / 1.16e-2
ORACLE_DZ = {"fp16": 4.5e-3, "bf16": 1.25e-2}
# oracle_fit on fit_case(deepsdf): the loss before step 0 and before step 49
ORACLE_FIT_LOSS = (0.2772, 0.01633)
# median angle between the fp16 emulation's and the fp64 decoder's normals at the vertices of the
# oracle's N = 44 mesh of the config-4 latent (randn(seed 0) x 0.1): 0.029 degrees
MEDIAN_ANGLE_FP16_DEG = 0.03
