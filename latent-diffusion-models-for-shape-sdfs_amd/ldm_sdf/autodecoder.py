"""C19: DeepSDF auto-decoder training.

The step before the hot path: it fits the decoder weights and one latent code per shape to
SDF samples, producing the latents that the diffusion model is then trained on and the
decoder that decodes them.  Objective: ``oracle/ref_autodecoder.py`` (DeepSDF's clamped L1 on
``tanh`` outputs plus the per-sample latent L2 regulariser; no dropout).

Every FLOP runs in ``libldm_sdf.so``; torch provides memory, the copies that build the padded
operands and Adam (plumbing), as in ``api.train``.  ``autodecoder_train_step`` has two paths:

* ``dtype="bf16"`` (the default, and the one ``bench.py`` measures), ``_train_step_gemm_bf16``:
  every product is an ``ldm_gemm_bf16`` problem.  Each activation ``h_l`` and gradient ``g_l``
  is kept once, in bf16, in both layouts: [Np, w] (the A operand of the next product, the ReLU
  mask of the G W products) and k-blocked [w, Np] (the B operand of the weight gradients, whose
  sum runs over the samples).  The epilogues write both (``Cb`` / ``CbT``), apply ReLU or its
  backward (``relu_bwd`` on the saved post-activation) and emit the 32-row column sums that
  become the bias gradients; the weight gradients are split-K, one slice per sample block.
* ``dtype="fp32"``, ``_train_step_linear_fp32``: exact fp32 products on ``ldm_linear`` (forward
  with the ReLU epilogue, ``G W`` with ``LDM_EPI_MASK_R``, ``G^T X`` on transposed views),
  ``ldm_colsum`` for the biases and ``ldm_colsum_segments`` for the per-shape latent gradients.

Both share the loss (``ldm_sdf_l1_loss``), the code regulariser (``ldm_latent_l2_reg``) and ONE
padded working layout, ``_Layout``: ``work_weights`` rebuilds it from the fp32 masters each
step, ``master_grads`` cuts the gradients back out of it.  The paths differ in its numbers only:

* ``Zx`` = ``[z_s || xyz || 0]`` (the input of layer 0, the second segment of layer ``skip``) is
  ``zw`` columns wide: L + 3 rounded up to 8 in fp32 (264; 16-byte rows in bf16 too), to a GEMM
  K segment of 64 in bf16 (320).
* Layer ``skip - 1`` (``hs`` = 253 outputs) is padded to ``hsp`` rows with zero weights and
  biases (a multiple of 4 in fp32, of 64 in bf16: 256 either way), so its ReLU output has zero
  columns past ``hs``.  Layer ``skip`` is two segments, ``h3 · W4h^T + Zx · W4z^T``.
* bf16 also pads the N = S P samples to ``Np`` rows (a multiple of ``_KQ``; rows >= N zero),
  cut into ``nblk`` blocks of ``KT``: the K slices of the weight gradients.
"""
from __future__ import annotations

import functools
import math
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Tuple

import torch

from . import _capi as capi
from . import dist as ldist
from . import ops
from .models import SDFDecoder

__all__ = ["AutoDecoderState", "autodecoder_train_step", "train_autodecoder", "CLAMP_DIST",
           "CODE_REG_LAMBDA"]

CLAMP_DIST = 0.1          # DeepSDF ClampingDistance
CODE_REG_LAMBDA = 1e-4    # DeepSDF CodeRegularizationLambda

_KQ = 128          # row padding of the sample axis (the K of the weight-gradient products)
# ldm_gemm_bf16 tile of the weight-gradient products (128 x 128: each slice walks KT = 8192
# samples, long enough for the bigger tile's per-CU operand economy); tuning runs pass
# ``wgrad_tile`` to autodecoder_train_step (the product reads no environment variable).
# Round 6 sweep (scripts/ad_wgrad_ab.py, profiles/r06am): the persistent 128 x 128 tile on a
# 2-deep ring (17) 30.9-31.1 ms/step, 14 31.0, the earlier 3 31.3-31.9, others 32-34; same bits
WGRAD_TILE = 17
_KSEG = 64         # bf16 padding of [z || xyz] and of the skip width (a GEMM K segment)


def _check_decoder(dec: SDFDecoder) -> Tuple[int, int]:
    if dec.widen_skip or dec.n_hidden != 8 or dec.skip != 4:
        raise capi.LdmError("auto-decoder training supports the DeepSDF 8-layer decoder with the "
                            "latent re-injected at layer 4 (skip width H - L - 3)")
    return dec.latent_dim, dec.hidden


def _round_up(n: int, m: int) -> int:
    return -(-n // m) * m


@dataclass(frozen=True)
class _Layout:
    """The padded working layout of one step (module doc): every size its stages share."""
    L: int
    H: int
    skip: int
    S: int
    P: int
    dtype: torch.dtype    # of the working weights
    row_pad: int          # hs (the skip width) is padded to a multiple of this: hsp
    col_pad: int          # L + 3 ([z || xyz]) to a multiple of this: zw
    hs: int
    hsp: int
    zw: int
    N: int                # S * P samples, padded to Np rows = nblk blocks of KT
    Np: int
    nblk: int
    KT: int


def _layout(L: int, H: int, skip: int, hs: int, S: int, P: int, dtype: torch.dtype) -> _Layout:
    N = S * P
    if dtype == torch.bfloat16:
        row_pad = col_pad = _KSEG
        Np = _round_up(N, _KQ)
        KT = next(kt for kt in (8192, 4096, 2048, 1024, 512, 256, 128) if Np % kt == 0)
        nblk = Np // KT
    else:
        row_pad, col_pad, Np, KT, nblk = 4, 8, N, N, 1
    return _Layout(L=L, H=H, skip=skip, S=S, P=P, dtype=dtype, row_pad=row_pad, col_pad=col_pad,
                   hs=hs, hsp=_round_up(hs, row_pad), zw=_round_up(L + 3, col_pad),
                   N=N, Np=Np, nblk=nblk, KT=KT)


def _zero_padded(src: torch.Tensor, shape, dtype: torch.dtype) -> torch.Tensor:
    out = torch.zeros(shape, device=src.device, dtype=dtype)
    out[tuple(slice(n) for n in src.shape)] = src
    return out


def work_weights(masters: Dict[str, torch.Tensor], L: int, H: int, skip: int,
                 dtype: torch.dtype, row_pad: int = 4, col_pad: int = 8
                 ) -> Dict[str, torch.Tensor]:
    """Padded working copies (see module doc) of the fp32 masters ``W{l}``/``b{l}``: ``W{l}``
    in ``dtype`` with the skip layer as ``W4h`` / ``W4z``, and layer ``skip - 1``'s padded fp32
    bias ``b{skip-1}p``.  The defaults are the fp32 path's pads.  Pure data movement; also used
    on CPU tensors by the host-logic tests."""
    zw = _round_up(L + 3, col_pad)
    hs = masters[f"W{skip - 1}"].shape[0]             # skip width, 253 for L=256, H=512
    hsp = _round_up(hs, row_pad)
    Ws = masters[f"W{skip}"]
    w = {f"W{l}": masters[f"W{l}"].to(dtype) for l in range(1, 9) if l not in (skip - 1, skip)}
    w["W0"] = _zero_padded(masters["W0"], (H, zw), dtype)
    w[f"W{skip - 1}"] = _zero_padded(masters[f"W{skip - 1}"], (hsp, H), dtype)
    w[f"b{skip - 1}p"] = _zero_padded(masters[f"b{skip - 1}"], (hsp,), torch.float32)
    w["W4h"] = _zero_padded(Ws[:, :hs], (H, hsp), dtype)
    w["W4z"] = _zero_padded(Ws[:, hs:], (H, zw), dtype)
    return w


def _working(masters: Dict[str, torch.Tensor], lay: _Layout):
    """(weights, biases) of a step in layout ``lay``: ``work_weights`` and the fp32 biases
    ``b{l}``, layer ``skip - 1``'s being the padded one."""
    w = work_weights(masters, lay.L, lay.H, lay.skip, lay.dtype, lay.row_pad, lay.col_pad)
    b = {f"b{l}": masters[f"b{l}"].contiguous() for l in range(9)}
    b[f"b{lay.skip - 1}"] = w.pop(f"b{lay.skip - 1}p")
    return w, b


def master_grads(gw: Dict[str, torch.Tensor], L: int, skip: int, hs: int,
                 out: Dict[str, torch.Tensor]) -> None:
    """Cut the padded working gradients (``W{l}`` with ``W4h`` / ``W4z`` at the skip, ``b{l}``)
    back to the master shapes (into ``out``)."""
    for l in range(9):
        Wm, bm = out[f"W{l}"], out[f"b{l}"]
        bm.copy_(gw[f"b{l}"][:bm.shape[0]])
        if l == skip:
            Wm[:, :hs].copy_(gw["W4h"][:, :hs])
            Wm[:, hs:].copy_(gw["W4z"][:, :L + 3])
        else:
            Wm.copy_(gw[f"W{l}"][:Wm.shape[0], :Wm.shape[1]])


def autodecoder_train_step(masters: Dict[str, torch.Tensor], z: torch.Tensor, xyz: torch.Tensor,
                           sdf: torch.Tensor, *, latent_dim: int = 256, hidden: int = 512,
                           skip: int = 4, delta: float = CLAMP_DIST,
                           reg_lambda: float = CODE_REG_LAMBDA, epoch: int = 100,
                           dtype: str = "bf16",
                           grads: Optional[Dict[str, torch.Tensor]] = None,
                           wgrad_tile: Optional[int] = None
                           ) -> Tuple[torch.Tensor, Dict[str, torch.Tensor], torch.Tensor]:
    """One forward/backward of the DeepSDF objective on a batch of S shapes x P samples.

    masters: fp32 device ``W0..W8``, ``b0..b8`` (torch ``nn.Linear`` layout, latent columns
    first: ``[z || xyz]`` and ``[h || z || xyz]`` at the skip).  z: [S, L] the batch's codes,
    xyz: [S, P, 3], sdf: [S, P].  ``dtype`` "fp32": exact fp32 GEMMs; "bf16": matrix-core
    GEMMs with bf16-rounded operands, fp32 accumulation.
    Returns (loss [1], weight grads keyed like ``masters``, latent grads [S, L]).
    """
    capi.require_device(z, xyz, sdf, masters["W0"])
    L = latent_dim
    S, P = sdf.shape
    if tuple(z.shape) != (S, L) or tuple(xyz.shape) != (S, P, 3):
        raise capi.LdmError(f"autodecoder_train_step: z{tuple(z.shape)} xyz{tuple(xyz.shape)} "
                            f"sdf{tuple(sdf.shape)}")
    if dtype not in ("bf16", "fp32"):
        raise capi.LdmError(f"autodecoder_train_step: dtype 'bf16' or 'fp32', got {dtype!r}")
    lay = _layout(L, hidden, skip, masters[f"W{skip - 1}"].shape[0], S, P,
                  torch.bfloat16 if dtype == "bf16" else torch.float32)
    z = z.contiguous()
    if dtype == "bf16":
        loss, gw, gz = _train_step_gemm_bf16(
            masters, z, xyz, sdf, lay, delta, WGRAD_TILE if wgrad_tile is None else wgrad_tile)
    else:
        loss, gw, gz = _train_step_linear_fp32(masters, z, xyz, sdf, lay, delta)
    # both paths' tail: the code regulariser (added to loss and gz) and the cut-back
    coef = reg_lambda * min(1.0, epoch / 100.0) / S
    if coef != 0.0:
        ops.latent_l2_reg(z, coef, loss, gz)
    if grads is None:
        grads = {k: torch.empty_like(v) for k, v in masters.items()}
    master_grads(gw, L, skip, lay.hs, grads)
    return loss, grads, gz


def _train_step_linear_fp32(masters, z, xyz, sdf, lay: _Layout, delta):
    """Exact fp32 step on ``ldm_linear`` (module doc): (loss, padded weight
    gradients, latent gradients) before the code regulariser."""
    dev = z.device
    cp = capi.COMPUTE_FP32
    L, H, skip, S, N, hsp, zw = lay.L, lay.H, lay.skip, lay.S, lay.N, lay.hsp, lay.zw
    w, b = _working(masters, lay)
    f32 = dict(device=dev, dtype=torch.float32)

    # ---- inputs: Zx = [z_s || xyz || 0] per sample
    owner = torch.arange(S, device=dev, dtype=torch.int32).repeat_interleave(lay.P)
    Zx = torch.zeros(N, zw, **f32)
    Zx[:, :L].copy_(ops.gather_rows(z, owner))
    Zx[:, L:L + 3].copy_(xyz.reshape(N, 3))

    # ---- forward (post-ReLU activations kept for the backward)
    RELU = capi.EPI_RELU
    h: List[torch.Tensor] = []
    x = Zx
    for l in range(8):
        width = hsp if l == skip - 1 else H
        y = torch.empty(N, width, **f32)
        if l == skip:
            ops.linear(x, w["W4h"], y, epi=RELU, bias=b[f"b{l}"], X2=Zx, W2=w["W4z"], compute=cp)
        else:
            ops.linear(x, w[f"W{l}"], y, epi=RELU, bias=b[f"b{l}"], compute=cp)
        h.append(y)
        x = y
    pre = torch.empty(N, 1, **f32)
    ops.linear(x, w["W8"], pre, bias=b["b8"], compute=cp)
    loss, g = ops.sdf_l1_loss(pre, sdf.contiguous(), delta, 1.0 / N)

    # ---- backward
    gw: Dict[str, torch.Tensor] = {}
    dz = torch.empty(N, L, **f32)
    for l in range(8, -1, -1):
        xin = Zx if l == 0 else h[l - 1]
        if l == skip:
            gw["W4h"] = torch.empty(H, hsp, **f32)
            gw["W4z"] = torch.empty(H, zw, **f32)
            ops.linear(g.T, xin.T, gw["W4h"], compute=cp)
            ops.linear(g.T, Zx.T, gw["W4z"], compute=cp)
            ops.linear(g, w["W4z"][:, :L].t().contiguous(), dz, compute=cp)   # latent part, layer 4
        else:
            gw[f"W{l}"] = torch.empty(w[f"W{l}"].shape, **f32)
            ops.linear(g.T, xin.T, gw[f"W{l}"], compute=cp)
        gw[f"b{l}"] = torch.empty(g.shape[1], **f32)
        ops.colsum(g, gw[f"b{l}"])
        if l == 0:
            ops.linear(g, w["W0"][:, :L].t().contiguous(), dz, epi=capi.EPI_ACCUM, compute=cp)
            break
        Wd = w["W4h"] if l == skip else w[f"W{l}"]
        dh = torch.empty(N, Wd.shape[1], **f32)       # ReLU backward fused: R = post-act.
        # G W with W transposed once (a 512 x 512 copy): both operands then run along k, so the
        # GEMM stages them with 16-byte row loads instead of 2-byte transposing LDS stores
        # (4.6 -> ~2.8 ms per 1M x 512 x 512 product; same products, same k order).
        ops.linear(g, Wd.t().contiguous(), dh, epi=capi.EPI_MASK_R, R=h[l - 1], compute=cp)
        g = dh

    gz = torch.empty(S, L, **f32)
    ops.colsum_segments(dz, S, gz)
    return loss, gw, gz


def _owner_index(S: int, P: int, Np: int, dev) -> torch.Tensor:
    """[Np] long: the shape that owns each padded sample row (shape-major: row m belongs to
    shape m // P); the padding rows >= S P get S, one past the last shape."""
    N = S * P
    owner_pad = torch.full((Np,), S, device=dev, dtype=torch.long)
    owner_pad[:N] = torch.arange(S, device=dev).repeat_interleave(P)
    return owner_pad


def _ad_inputs(z, xyz, S, P, Np, zw, KT, gather=False):
    """The bf16 step's input operand in both layouts: ``Zx`` [Np, zw] = [z_s || xyz || 0] per
    sample (rows >= N zero) and ``ZxT`` [Np / KT, zw, KT], its k-blocked transpose.  Samples are
    shape-major (sample m belongs to shape m // P), so the code columns are a broadcast of z per
    shape: when P is a multiple of KT every block lies in one shape and both layouts are written
    by broadcast copies (round 6: the index gathers of [N, L] took ≈ 1 ms of the 64 x 16384
    step); else (or ``gather``) by the per-sample gathers.  Same values either way
    (``tests/test_autodecoder_inputs.py``).  Every sample-axis (transposed) operand of the step
    is k-BLOCKED like ``ZxT``: a weight-gradient slice is one block, so the rows it streams lie
    KT * 2 bytes apart instead of 2 MB apart (one page per row: 9 us per k-step, TLB-bound)."""
    L = z.shape[1]
    N = S * P
    nblk = Np // KT
    dev = z.device
    bf = dict(device=dev, dtype=torch.bfloat16)
    Zx = torch.zeros(Np, zw, **bf)
    ZxT = torch.zeros(nblk, zw, KT, **bf)
    if not gather and P % KT == 0:
        zb = z.to(torch.bfloat16)
        Zx[:N].view(S, P, zw)[:, :, :L] = zb[:, None, :]
        ZxT[:N // KT].view(S, P // KT, zw, KT)[:, :, :L, :] = zb[:, None, :, None]
    else:
        owner_pad = _owner_index(S, P, Np, dev)
        Zx[:N, :L] = z[owner_pad[:N]]
        zT = torch.zeros(L, S + 1, **bf)          # column S: the padding rows' zero code
        zT[:, :S] = z.t()
        ZxT.permute(1, 0, 2)[:L] = zT[:, owner_pad.view(nblk, KT)]
    Zx[:N, L:L + 3] = xyz.reshape(N, 3)
    xyz_pad = torch.zeros(Np, 3, device=dev, dtype=torch.float32)
    xyz_pad[:N] = xyz.reshape(N, 3)
    ZxT.permute(1, 0, 2)[L:L + 3] = xyz_pad.t().reshape(3, nblk, KT).to(torch.bfloat16)
    return Zx, ZxT


def _train_step_gemm_bf16(masters, z, xyz, sdf, lay: _Layout, delta, wgrad_tile):
    """bf16 matrix-core step on ``ldm_gemm_bf16`` (module doc; include/ldm_sdf.h; DESIGN.md
    §11): (loss, padded weight gradients, latent gradients) before the code regulariser.
    Numerics: operands rounded to bf16 (RNE), fp32 accumulation -- as ``ldm_linear``'s bf16."""
    N = lay.N
    w, WT, bias = _weights_bf16(masters, lay)
    Zx, ZxT = _ad_inputs(z, xyz, lay.S, lay.P, lay.Np, lay.zw, lay.KT)
    h, hT, pre = _forward_bf16(w, bias, Zx, lay)
    loss, g8 = ops.sdf_l1_loss(pre[:N].reshape(N, 1), sdf.reshape(N, 1).contiguous(), delta,
                               1.0 / N)
    gw, gcs, Gs = _backward_bf16(WT, g8, h, hT, ZxT, lay, wgrad_tile)
    _bias_sums_bf16(gcs, gw)
    return loss, gw, _latent_grad_bf16(masters, gcs, Gs, lay)


def _weights_bf16(masters, lay: _Layout):
    """(w, WT, bias): the bf16 working weights, their transposes for the G W products (none
    for ``W0`` and ``W4z``: no gradient is taken through ``Zx``) and the fp32 biases."""
    w, bias = _working(masters, lay)
    WT = {k: v.t().contiguous() for k, v in w.items() if k not in ("W0", "W4z", "W8")}
    # the 512 -> 1 layer as a K = 64 product for its backward (g8 in column 0, zeros beside)
    WT["W8"] = torch.zeros(lay.H, _KSEG, device=w["W8"].device, dtype=torch.bfloat16)
    WT["W8"][:, 0] = w["W8"].reshape(-1)
    return w, WT, bias


def _forward_bf16(w, bias, Zx, lay: _Layout):
    """(h, hT, pre): ``h_l = ReLU(...)`` in bf16 in both layouts (rows >= N written as zeros),
    l = 0..7, and the fp32 ``pre`` [Np, 1] of the last layer."""
    N, Np, KT = lay.N, lay.Np, lay.KT
    bf = dict(device=Zx.device, dtype=torch.bfloat16)
    h, hT = [], []
    x = Zx
    for l in range(8):
        width = lay.hsp if l == lay.skip - 1 else lay.H
        y = torch.empty(Np, width, **bf)
        yT = torch.empty(lay.nblk, width, KT, **bf)
        segs = ([(x, w["W4h"]), (Zx, w["W4z"])] if l == lay.skip else [(x, w[f"W{l}"])])
        ops.gemm([ops.gemm_problem(segs, Np, width, mode="relu", M_valid=N, bias=bias[f"b{l}"],
                                   Cb=y, CbT=yT, ct_blk=KT)])
        h.append(y)
        hT.append(yT)
        x = y
    pre = torch.empty(Np, 1, device=Zx.device, dtype=torch.float32)
    ops.gemm([ops.gemm_problem([(x, w["W8"])], Np, 1, M_valid=N, bias=bias["b8"], C=pre)])
    return h, hT, pre


def _wgrad(ws_cache, lay: _Layout, gT, xT, M_, N_, out, slot):
    """The problem out [M_, N_] fp32 = sum over the samples of gT x xT^T; gT [nblk, M_, KT] and
    xT [nblk, N_, KT] blocked: split-K with one slice per block.  `slot` = the problem's
    index within its launch (its own split-K workspace, from the step's ``ws_cache``)."""
    nblk, KT = lay.nblk, lay.KT
    if nblk == 1:
        return ops.gemm_problem([(gT[0], xT[0])], M_, N_, C=out)
    # keyed by (size, slot in the launch's problem list): two problems of ONE launch must
    # never share partial slabs, even when their sizes agree (e.g. S == zw on the one-hot
    # path); launches run in stream order, so reuse across launches is safe
    n = nblk * M_ * N_
    ws = ws_cache.get((n, slot))
    if ws is None:
        ws = ws_cache[(n, slot)] = torch.empty(n, device=out.device, dtype=torch.float32)
    return ops.gemm_problem([(gT[0], xT[0])], M_, N_, C=out, k_split=nblk, ws=ws,
                            slices=(gT.shape[1] * KT, xT.shape[1] * KT))


def _gw_relu_bwd(g, WdT, R, lay: _Layout):
    """(g_prev, g_prev^T, column sums): ``(g W) * [R > 0]`` for g [Np, wout] and W^T = WdT
    [win, wout], in bf16 in both layouts, with the fp32 sums of each 32-row block."""
    Np, KT, win = lay.Np, lay.KT, R.shape[1]
    g_prev = torch.empty(Np, win, device=g.device, dtype=torch.bfloat16)
    gT_prev = torch.empty(lay.nblk, win, KT, device=g.device, dtype=torch.bfloat16)
    cs = torch.empty(-(-Np // 32), win, device=g.device, dtype=torch.float32)
    ops.gemm([ops.gemm_problem([(g, WdT)], Np, win, mode="relu_bwd", M_valid=lay.N, Rb=R,
                               Cb=g_prev, CbT=gT_prev, colsum=cs, ct_blk=KT)])
    return g_prev, gT_prev, cs


def _backward_bf16(WT, g8, h, hT, ZxT, lay: _Layout, wgrad_tile):
    """(gw, gcs, Gs) from g8 = dL/d pre [N, 1]: the padded weight gradients (and ``b8``), the
    32-row column sums of every g_l (bias / latent gradients), and on the one-hot path the
    per-shape column sums of g_skip and g_0.  Layer 8 runs its G W product before its weight
    gradient, the others after (the launch order the step has always had)."""
    H, skip, S, N, Np, KT, nblk = lay.H, lay.skip, lay.S, lay.N, lay.Np, lay.KT, lay.nblk
    dev = g8.device
    f32 = dict(device=dev, dtype=torch.float32)
    wg = functools.partial(_wgrad, {}, lay)      # one workspace cache for the whole step
    # layer 8: dW8 = g8^T h7, db8 = sum g8; g7 = (g8 w8) * [h7 > 0]
    g8b = torch.zeros(Np, _KSEG, device=dev, dtype=torch.bfloat16)
    g8b[:N, 0] = g8.reshape(N)
    g8row = g8b[:, 0].contiguous().reshape(nblk, 1, KT)      # blocked [nblk][1][KT]
    gw = {"W8": torch.empty(1, H, **f32), "b8": torch.empty(1, **f32)}
    ops.colsum(g8.reshape(N, 1), gw["b8"])
    gcs = {}                                       # g_l per 32-row block sums (bias / latent)
    g, gT, gcs[7] = _gw_relu_bwd(g8b, WT["W8"], h[7], lay)
    ops.gemm([wg(g8row, hT[7], 1, H, gw["W8"], 0)], tile=wgrad_tile)
    Gs = {}                                        # per-shape column sums of g_skip and g_0
    onehot = None
    if lay.P % 32:                                 # 32-row blocks straddle shapes: a one-hot
        sid = torch.arange(S, device=dev)[:, None, None]   # product sums each shape's rows
        owner_pad = _owner_index(S, lay.P, Np, dev)
        onehot = (owner_pad.view(1, nblk, KT) == sid).to(torch.bfloat16).permute(1, 0, 2)
        onehot = onehot.contiguous()               # blocked [nblk][S][KT]
    for l in range(7, -1, -1):
        # g = dL/d pre_l (bf16, both layouts); its column sums are gcs[l]
        xT = ZxT if l == 0 else hT[l - 1]
        if l == skip:
            gw["W4h"] = torch.empty(H, lay.hsp, **f32)
            gw["W4z"] = torch.empty(H, lay.zw, **f32)
            probs = [wg(gT, xT, H, lay.hsp, gw["W4h"], 0),
                     wg(gT, ZxT, H, lay.zw, gw["W4z"], 1)]
        else:
            wout, win = gT.shape[1], xT.shape[1]
            gw[f"W{l}"] = torch.empty(wout, win, **f32)
            probs = [wg(gT, xT, wout, win, gw[f"W{l}"], 0)]
        if onehot is not None and l in (skip, 0):
            Gs[l] = torch.empty(S, H, **f32)
            probs.append(wg(onehot, gT, S, H, Gs[l], len(probs)))
        # weight gradients (long K per slice): larger tiles than the 1M-row G W product, so
        # their own launch
        ops.gemm(probs, tile=wgrad_tile)
        if l > 0:
            g, gT, gcs[l - 1] = _gw_relu_bwd(g, WT["W4h" if l == skip else f"W{l}"], h[l - 1],
                                             lay)
    return gw, gcs, Gs


def _bias_sums_bf16(gcs, gw) -> None:
    """``gw["b{l}"]``, l = 0..7: the column sums of the 32-row partials ``gcs[l]``."""
    for l in range(8):
        gw[f"b{l}"] = torch.empty(gcs[l].shape[1], device=gcs[l].device, dtype=torch.float32)
        ops.colsum(gcs[l], gw[f"b{l}"])


def _latent_grad_bf16(masters, gcs, Gs, lay: _Layout):
    """gz [S, L] without an [N, L] product: per shape, sum_p (g4 W4z + g0 W0)[:, :L] = (the
    per-shape column sums of g4 and g0) x the masters' latent columns, [S, H] x [H, L] in fp32."""
    L, skip, S, hs = lay.L, lay.skip, lay.S, lay.hs
    f32 = dict(device=gcs[0].device, dtype=torch.float32)
    if not lay.P % 32:                             # shape s = 32-row blocks [s P/32, (s+1) P/32)
        Gs = {}
        for l in (skip, 0):
            Gs[l] = torch.empty(S, lay.H, **f32)
            ops.colsum_segments(gcs[l][:lay.N // 32].contiguous(), S, Gs[l])
    gz = torch.empty(S, L, **f32)
    ops.linear(Gs[skip], masters[f"W{skip}"][:, hs:hs + L].t(), gz, compute=capi.COMPUTE_FP32)
    ops.linear(Gs[0], masters["W0"][:, :L].t(), gz, epi=capi.EPI_ACCUM,
               compute=capi.COMPUTE_FP32)
    return gz


@dataclass
class AutoDecoderState:
    step: int = 0
    losses: List[float] = field(default_factory=list)
    masters: Optional[Dict[str, torch.Tensor]] = None
    latents: Optional[torch.Tensor] = None            # [n_shapes, L] fp32, device
    optimizer: Optional[torch.optim.Optimizer] = None
    lat_optimizer: Optional[torch.optim.Optimizer] = None


def train_autodecoder(decoder: SDFDecoder, xyz: torch.Tensor, sdf: torch.Tensor, *, steps: int,
                      shapes_per_batch: Optional[int] = None,
                      samples_per_shape: Optional[int] = None, lr_decoder: float = 5e-4,
                      lr_latent: float = 1e-3, delta: float = CLAMP_DIST,
                      reg_lambda: float = CODE_REG_LAMBDA, epoch: Optional[int] = None,
                      dtype: str = "bf16", generator: Optional[torch.Generator] = None,
                      state: Optional[AutoDecoderState] = None, group=None) -> AutoDecoderState:
    """Fit the decoder and one latent per shape to SDF samples (DeepSDF auto-decoder).

    xyz: [n_shapes, n_samples, 3], sdf: [n_shapes, n_samples] on the GPU.  Each step draws
    ``shapes_per_batch`` shapes (without replacement) and ``samples_per_shape`` samples of each
    (DeepSDF: 64 scenes x 16384 samples).  Codes start at N(0, 1/L) (CodeInitStdDev 1 / sqrt L);
    both parameter sets use Adam.  Data parallel over the group: every rank draws the same
    shapes, takes its contiguous share of them, and the weight gradients are all-reduced
    (averaged).  The latents are replicated; each rank updates its own shapes' rows and the
    updated rows are all-reduced, so all ranks keep the same table.  ``decoder``'s weights are
    updated in place at the end.
    """
    capi.require_device(xyz, sdf)
    device = xyz.device
    L, H = _check_decoder(decoder)
    n_shapes, n_samples = sdf.shape
    S = min(shapes_per_batch or n_shapes, n_shapes)
    P = min(samples_per_shape or n_samples, n_samples)
    world, rank = ldist.world_and_rank(group)
    if state is None:
        state = AutoDecoderState()
        state.masters = {}
        for l in range(9):
            state.masters[f"W{l}"] = decoder.weights[l].to(device).clone()
            state.masters[f"b{l}"] = decoder.biases[l].to(device).clone()
        seed = 0 if generator is None else int(
            torch.randint(0, 2 ** 31, (1,), generator=generator, device=generator.device))
        gen = torch.Generator().manual_seed(seed)
        state.latents = (torch.randn(n_shapes, L, generator=gen) / math.sqrt(L)).to(device)
        state.optimizer = torch.optim.Adam(list(state.masters.values()), lr=lr_decoder)
        state.lat_optimizer = torch.optim.Adam([state.latents], lr=lr_latent)
    grads = {k: torch.empty_like(v) for k, v in state.masters.items()}
    lat_grad = torch.zeros_like(state.latents)
    for _ in range(steps):
        sidx = torch.randperm(n_shapes, device=device, generator=generator)[:S]
        pidx = torch.randint(0, n_samples, (S, P), device=device, generator=generator)
        lo, hi = ldist.batch_shard(S, rank, world)
        mine = sidx[lo:hi]
        pts = torch.gather(xyz[mine], 1, pidx[lo:hi, :, None].expand(-1, -1, 3)).contiguous()
        tgt = torch.gather(sdf[mine], 1, pidx[lo:hi]).contiguous()
        z = state.latents[mine].contiguous()
        ep = state.step if epoch is None else epoch
        loss, grads, gz = autodecoder_train_step(
            state.masters, z, pts, tgt, latent_dim=L, hidden=H, skip=decoder.skip, delta=delta,
            reg_lambda=reg_lambda, epoch=ep, dtype=dtype, grads=grads)
        ldist.allreduce_mean_([grads[k] for k in state.masters], group=group)
        lat_grad.zero_()
        lat_grad[mine] = gz * ((hi - lo) / S)     # this rank's share of the batch mean
        ldist.allreduce_sum_([lat_grad], group=group)
        for k, p in state.masters.items():
            p.grad = grads[k]
        state.latents.grad = lat_grad
        state.optimizer.step()
        state.lat_optimizer.step()
        state.step += 1
        state.losses.append(loss)
    ops.read_back_losses(state.losses)
    for l in range(9):
        decoder.weights[l] = state.masters[f"W{l}"].detach().to("cpu").contiguous()
        decoder.biases[l] = state.masters[f"b{l}"].detach().to("cpu").contiguous()
    decoder.invalidate()
    return state
