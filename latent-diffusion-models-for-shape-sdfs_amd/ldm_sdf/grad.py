"""Derivatives of the decoder with respect to its INPUT, weights frozen.

``sdf_grad``     the field and its spatial gradient at arbitrary points (normals of the surface).
``fit_latents``  DeepSDF's ``reconstruct``: latents fitted to the SDF samples of unseen shapes
                 with the decoder fixed.

Both run ``csrc/decoder_grad.hip``: forward and backward of a 64-point tile in one launch,
16-bit operands, only the ReLU sign bits kept.  There is no fp32 gradient kernel and no CPU path.
"""
from __future__ import annotations

from typing import List, Optional, Tuple

import torch

from . import _capi as capi
from . import ops
from .autodecoder import CLAMP_DIST, CODE_REG_LAMBDA
from .models import SDFDecoder


def _grad_dtype(dtype: str, what: str) -> str:
    if dtype not in ("fp16", "bf16"):
        raise capi.LdmError(f"{what}: dtype must be 'fp16' or 'bf16' (got {dtype!r}; there is no "
                            "fp32 gradient kernel)")
    return dtype


def sdf_grad(decoder: SDFDecoder, latents: torch.Tensor, xyz: torch.Tensor, *,
             dtype: str = "fp16") -> Tuple[torch.Tensor, torch.Tensor]:
    """``(sdf [B, P], grad [B, P, 3])``: the decoder's value and its gradient with respect to
    xyz at xyz ``[B, P, 3]`` (or ``[P, 3]`` shared).  ``dtype`` "fp16" (default: the gradient of
    a ReLU network is piecewise constant, and fp16's activation noise flips far fewer near-zero
    units than bf16's) or "bf16"."""
    _grad_dtype(dtype, "sdf_grad")
    capi.require_device(latents, xyz)
    if latents.dim() == 1:
        latents = latents[None]
    if latents.shape[1] != decoder.latent_dim:
        raise ValueError(f"latents must be [B, {decoder.latent_dim}]")
    B = latents.shape[0]
    if xyz.dim() == 2:
        xyz = xyz[None].expand(B, -1, -1)
    if xyz.dim() != 3 or xyz.shape[0] != B or xyz.shape[2] != 3:
        raise ValueError("xyz must be [B, P, 3] or [P, 3]")
    dev = latents.device
    fdesc = decoder.device_pack(dtype, dev)["desc"]
    gdesc = decoder.device_pack_grad(dtype, dev)["desc"]
    beta = ops.decoder_fold(fdesc, latents.float().contiguous())
    out = ops.decoder_points_grad(gdesc, beta, xyz.float().contiguous())
    return out["sdf"], out["dxyz"]


def fit_latents(decoder: SDFDecoder, xyz: torch.Tensor, sdf: torch.Tensor, *, steps: int = 800,
                samples_per_shape: int = 8000, lr: float = 5e-3, delta: float = CLAMP_DIST,
                reg_lambda: float = CODE_REG_LAMBDA, init_std: float = 0.01,
                generator: Optional[torch.Generator] = None, dtype: str = "bf16",
                latents: Optional[torch.Tensor] = None, return_losses: bool = False):
    """Latents ``[S, L]`` fitted to the SDF samples xyz ``[S, n, 3]``, sdf ``[S, n]`` of S shapes
    with the decoder FROZEN (DeepSDF ``reconstruct``): ``decoder.weights`` are not touched.

    The objective is the auto-decoder loss at epoch 100: clamped L1 / (S P) plus
    ``reg_lambda`` times the mean code norm.  Each step draws ``samples_per_shape`` samples per
    shape, runs the gradient kernel in loss mode, the transposed fold and the code regulariser,
    then ``torch.optim.Adam`` on the latent table; the learning rate drops tenfold at
    ``steps // 2``.  Codes start at N(0, ``init_std``^2) unless ``latents`` (a starting table,
    not modified) is given.  ``dtype`` "bf16" (default: the latent gradient is a sum over the
    points and bf16's is good to 1-2 %) or "fp16".  Losses stay on the device until the end;
    ``return_losses`` adds the per-step loss list to the result."""
    _grad_dtype(dtype, "fit_latents")
    if xyz.dim() != 3 or xyz.shape[2] != 3 or tuple(sdf.shape) != tuple(xyz.shape[:2]):
        raise ValueError("fit_latents: xyz must be [S, n, 3] and sdf [S, n]")
    if steps < 0 or samples_per_shape < 1:
        raise ValueError("fit_latents: steps >= 0 and samples_per_shape >= 1")
    if not delta > 0.0 or not lr > 0.0:
        raise ValueError("fit_latents: delta and lr must be > 0")
    S, n = sdf.shape
    L = decoder.latent_dim
    if latents is not None and tuple(latents.shape) != (S, L):
        raise ValueError(f"fit_latents: latents must be [{S}, {L}]")
    capi.require_device(xyz, sdf, latents)
    dev = xyz.device
    P = min(int(samples_per_shape), n)
    if latents is not None:
        lat = latents.detach().float().clone().contiguous()
    else:
        seed = 0 if generator is None else int(
            torch.randint(0, 2 ** 31, (1,), generator=generator, device=generator.device))
        gen = torch.Generator().manual_seed(seed)
        lat = (torch.randn(S, L, generator=gen) * float(init_std)).to(dev)
    fdesc = decoder.device_pack(dtype, dev)["desc"]
    gdesc = decoder.device_pack_grad(dtype, dev)["desc"]
    xyz = xyz.float().contiguous()
    sdf = sdf.float().contiguous()
    opt = torch.optim.Adam([lat], lr=lr)
    grad = torch.empty_like(lat)
    ws = torch.empty(max(ops.decoder_grad_ws_bytes(S, P, gdesc.dtype), 256), device=dev,
                     dtype=torch.uint8)
    losses: List[torch.Tensor] = []
    for step in range(steps):
        if step == steps // 2 and step > 0:
            for g in opt.param_groups:
                g["lr"] = lr / 10.0
        if P < n:
            pidx = torch.randint(0, n, (S, P), device=dev, generator=generator)
            pts = torch.gather(xyz, 1, pidx[:, :, None].expand(-1, -1, 3)).contiguous()
            tgt = torch.gather(sdf, 1, pidx).contiguous()
        else:
            pts, tgt = xyz, sdf
        beta = ops.decoder_fold(fdesc, lat)
        out = ops.decoder_points_grad(gdesc, beta, pts, gt=tgt, delta=delta,
                                      scale=1.0 / (S * P), want_dxyz=False, want_dbeta=True,
                                      want_loss=True, ws=ws)
        ops.decoder_fold_bwd(gdesc, out["dbeta"], out=grad)
        ops.latent_l2_reg(lat, reg_lambda / S, out["loss"], grad)
        lat.grad = grad
        opt.step()
        if return_losses:
            losses.append(out["loss"])
    lat.grad = None
    if return_losses:
        return lat, ops.read_back_losses(losses)
    return lat
