"""C17: 1D-UNet eps-denoiser over a latent code seen as a 1-channel signal (config 5:
1024-d latents).  Architecture: DESIGN.md §9 (the same network as ``oracle/ref_unet.py``).

Every conv runs in ``ldm_conv1d`` (``csrc/unet.hip``); a forward is 18 launches:

    conv_in | Res_0 (2) | down0 | Res_1 (2) | down1 | Res_2 (2) | Res_3 (2) | up1 |
    Res_4 (2, concat as two segments) | up0 | Res_5 (2) | conv_out + DDPM step (A8)

``unet_plan`` (records of buffer and weight NAMES) and ``unet_shapes`` are the only description
of that network: ``bind_plan`` turns them into ``ConvArgs`` (the sampler per step, the trainer
once), ``backward_schedule`` reverses the plan by name, buffers and ``step_cost`` derive from both.

The timestep-embedding MLP and each block's projection are tabulated for all t once per
weight version (``E_i[t] = P_i temb(t) + b1_i``, fp32 ``[T, Cout_i]``), so a sampling step
reads one table row per block as a per-channel bias (A5's table trick, as for the MLP).

Training (``UNetTrainer``) runs the same 18 convs at per-sample timesteps and
walks them in reverse through ``ldm_conv1d_bwd_weight`` / ``ldm_conv1d_bwd_data``
(``csrc/unet_bwd.hip``).
"""
from __future__ import annotations

import ctypes
import functools
import math
from dataclasses import dataclass
from typing import Callable, Dict, List, Optional, Sequence, Tuple

import torch

from . import _capi as capi
from . import ops
from .models import timestep_embedding_table


CONV_SUFFIXES = (".w", ".w1", ".w2", ".ws")


def is_conv_weight(name: str) -> bool:
    return name.endswith(CONV_SUFFIXES)


def is_linear_weight(name: str) -> bool:
    return name.startswith("W") or name.endswith(".p")


def unet_res_specs(C: Tuple[int, int, int]) -> List[Tuple[int, int]]:
    """(cin, cout) of the six residual blocks in execution order."""
    c0, c1, c2 = C
    return [(c0, c0), (c1, c1), (c2, c2), (c2, c2), (2 * c1, c1), (2 * c0, c0)]


# ------------------------------------------------------------------------------- the plan
@dataclass(frozen=True)
class Seg:
    """One operand of a conv: input buffer, weight, the operand's ordinal among those that read
    this weight (> 0: a later operand of a concat weight), tap geometry, SiLU on the input."""
    x: str
    w: str
    ordinal: int = 0
    stride: int = 1
    mode: int = capi.CONV_DIRECT
    silu: bool = False
    ksize: int = 3


@dataclass(frozen=True)
class ConvRec:
    """One ``ldm_conv1d`` launch: output buffer, operands, bias names, the residual block whose
    projection supplies the per-channel bias (``cb``) and the identity-residual buffer."""
    out: str
    segs: Tuple[Seg, ...]
    bias: Optional[str] = None
    bias2: Optional[str] = None
    cb: Optional[int] = None
    R: Optional[str] = None


@functools.lru_cache(maxsize=None)
def unet_plan(C: Tuple[int, int, int], fused_concat: bool = False) -> Tuple[ConvRec, ...]:
    """The 18 convs in launch order.  ``fused_concat``: the sampler's ``n == 1`` form, where
    res4 / res5 read the skip concat ``[u || s]`` as ONE buffer ``cat1`` / ``cat0`` whose halves
    the producers wrote (one staging segment fewer in their two convs)."""
    P: List[ConvRec] = []

    def conv(out, x, w, **geom):
        P.append(ConvRec(out, (Seg(x, w + ".w", **geom),), bias=w + ".b"))

    def res(i, xin, a, y):
        P.append(ConvRec(a, tuple(Seg(xi, f"res{i}.w1", k, silu=True)
                                  for k, xi in enumerate(xin)), cb=i))
        main = Seg(a, f"res{i}.w2", silu=True)
        ci, co = unet_res_specs(C)[i]
        if ci != co:            # 1x1 shortcut: further segments of the second conv
            short = tuple(Seg(xi, f"res{i}.ws", k, ksize=1) for k, xi in enumerate(xin))
            P.append(ConvRec(y, (main,) + short, bias=f"res{i}.b2", bias2=f"res{i}.bs"))
        else:
            P.append(ConvRec(y, (main,), bias=f"res{i}.b2", R=xin[0]))

    conv("h0", "x", "conv_in")
    res(0, ["h0"], "a0", "s0")
    conv("d0", "s0", "down0", stride=2)
    res(1, ["d0"], "a1", "s1")
    conv("d1", "s1", "down1", stride=2)
    res(2, ["d1"], "a2", "m0")
    res(3, ["m0"], "a3", "m1")
    conv("u1", "m1", "up1", mode=capi.CONV_UP2)
    res(4, ["cat1"] if fused_concat else ["u1", "s1"], "a4", "r4")
    conv("u0", "r4", "up0", mode=capi.CONV_UP2)
    res(5, ["cat0"] if fused_concat else ["u0", "s0"], "a5", "r5")
    conv("eps", "r5", "conv_out", silu=True)
    return tuple(P)


def unet_shapes(D: int, C: Tuple[int, int, int]) -> Dict[str, Tuple[int, int]]:
    """(channels, length) of every buffer a plan names (``cat*``: the fused form's concats)."""
    c0, c1, c2 = C
    l0, l1, l2 = (c0, D), (c1, D // 2), (c2, D // 4)
    groups = ((("x",), (1, D)), (("h0", "a0", "s0"), l0), (("d0", "a1", "s1"), l1),
              (("d1", "a2", "m0", "a3", "m1"), l2), (("u1", "a4", "r4"), l1),
              (("u0", "a5", "r5"), l0), (("eps",), (1, D)),
              (("cat1",), (2 * c1, D // 2)), (("cat0",), (2 * c0, D)))
    return {n: s for names, s in groups for n in names}


# The two layouts of a concat conv's weight: where an operand's input channels start, given the
# channel counts of the operands before it.
def sample_c_off(before: Sequence[int]) -> int:
    """``device_pack``: ``pack_conv_weight`` of the WHOLE weight.  ``conv1d_args`` rejects a start
    that is no multiple of 16 (ragged widths at n > 1; the n == 1 fused form has one operand)."""
    return sum(before)


def train_c_off(before: Sequence[int]) -> int:
    """``UNet1DDenoiser.pack_train``: each operand packed on its own, padded to 16 channels."""
    return sum(ops._r16(c) for c in before)


def bind_segments(rec: ConvRec, weights, bufs, c_off: Callable) -> List[ops.ConvSegment]:
    """The ``ConvSegment`` list of one record over named weights and buffers."""
    out = []
    for s in rec.segs:
        off = 0
        if s.ordinal:
            off = c_off([bufs[o.x].shape[1] for o in rec.segs
                         if o.w == s.w and o.ordinal < s.ordinal])
        out.append(ops.ConvSegment(bufs[s.x], weights[s.w], c_off=off, stride=s.stride,
                                   mode=s.mode, silu=s.silu))
    return out


def bind_plan(plan: Sequence[ConvRec], weights, bufs, cbias: Callable, c_off: Callable,
              ddpm: Optional[dict] = None) -> List[capi.ConvArgs]:
    """A plan -> the ``ldm_conv1d`` argument structs.  ``cbias(i)`` gives block i's per-channel
    bias tensor and its batch stride ``scb``; ``ddpm`` (``xlat``, ``z``, ``sched``, ``t``) puts
    the A8 reverse step into the last conv's epilogue."""
    calls = []
    for r in plan:
        kw = {}
        if r.cb is not None:
            kw["cbias"], kw["scb"] = cbias(r.cb)
        if ddpm is not None and r is plan[-1]:
            kw.update(ddpm, epi=capi.CONV_EPI_DDPM)
        calls.append(ops.conv1d_args(                       # an absent name stays None
            bind_segments(r, weights, bufs, c_off), bufs[r.out], bias=r.bias and weights[r.bias],
            bias2=r.bias2 and weights[r.bias2], R=r.R and bufs[r.R], **kw))
    return calls


def backward_schedule(plan: Sequence[ConvRec]) -> List[tuple]:
    """The backward of a plan, by name: the convs in reverse, each as

        ("w", k, dbias, cb)       weight gradient of conv k: bias gradient name, block of dcbias
        ("copy", bias2, bias)     the shortcut's bias shares the output: same sums
        ("alias", R, out)         identity residual: R's gradient STARTS as out's (one buffer)
        ("d", k, j, accumulate)   data gradient of segment j of conv k; an activation's gradient
                                  is written by its first consumer here, accumulated by the later
    The network input ``x`` gets no data gradient."""
    sched: List[tuple] = []
    have = {plan[-1].out}
    for k, r in reversed(list(enumerate(plan))):
        sched.append(("w", k, r.bias if r.cb is None else f"res{r.cb}.b1", r.cb))
        if r.bias2 is not None:
            sched.append(("copy", r.bias2, r.bias))
        if r.R is not None:
            if r.R in have:
                raise capi.LdmError("UNetTrainer: identity residual after another consumer")
            have.add(r.R)
            sched.append(("alias", r.R, r.out))
        for j, s in enumerate(r.segs):
            if s.x == "x":
                continue
            sched.append(("d", k, j, s.x in have))
            have.add(s.x)
    return sched


def make_work(masters: Dict[str, torch.Tensor], dtype: str) -> Dict[str, torch.Tensor]:
    """The weights the kernels read: the fp32 masters themselves, or bf16 copies (RNE) of every
    conv / linear weight with the fp32 biases."""
    if dtype == "fp32":
        return dict(masters)
    if dtype != "bf16":
        raise capi.LdmError(f"UNet training dtype {dtype!r} (fp32 | bf16)")
    return {n: v.to(torch.bfloat16) if is_conv_weight(n) or is_linear_weight(n) else v
            for n, v in masters.items()}


class UNet1DDenoiser:
    """eps-prediction 1D-UNet (D divisible by 4; channels ``C = (c0, c1, c2)``).

    ``params`` are fp32 master tensors named as in ``oracle/ref_unet.py``; the initialiser
    draws them in the same order from the same generator, so one seed is one network on
    both sides.
    """

    def __init__(self, D: int = 1024, C: Tuple[int, int, int] = (32, 64, 128), TE: int = 128,
                 HT: int = 512, T: int = 1000, seed: int = 2468,
                 params: Optional[Dict[str, torch.Tensor]] = None):
        if D % 4:
            raise ValueError("UNet1D needs D divisible by 4 (two stride-2 levels)")
        self.D, self.C, self.TE, self.HT, self.T = D, tuple(C), TE, HT, T
        if params is None:
            params = self._init(seed)
        self.params = {k: v.detach().to("cpu", torch.float32).contiguous()
                       for k, v in params.items()}
        self.emb_table = torch.from_numpy(timestep_embedding_table(T, TE))
        self._dev: Dict[Tuple[str, torch.device], Dict[str, object]] = {}
        self._trainers: Dict[tuple, "UNetTrainer"] = {}

    def _init(self, seed: int) -> Dict[str, torch.Tensor]:
        g = torch.Generator().manual_seed(seed)
        p: Dict[str, torch.Tensor] = {}

        def w(name, shape, fan_in, gain=1.0):
            p[name] = torch.randn(*shape, generator=g, dtype=torch.float64) * math.sqrt(gain / fan_in)

        def b(name, n):
            p[name] = torch.randn(n, generator=g, dtype=torch.float64) * 0.01

        c0, c1, c2 = self.C
        HT, TE = self.HT, self.TE
        w("Wt1", (HT, TE), TE); b("bt1", HT)
        w("Wt2", (HT, HT), HT); b("bt2", HT)
        w("conv_in.w", (c0, 1, 3), 3, 2.0); b("conv_in.b", c0)
        for i, (ci, co) in enumerate(unet_res_specs(self.C)):
            w(f"res{i}.w1", (co, ci, 3), 3 * ci, 2.0); b(f"res{i}.b1", co)
            w(f"res{i}.p", (co, HT), HT)
            w(f"res{i}.w2", (co, co, 3), 3 * co, 2.0 / 12.0); b(f"res{i}.b2", co)
            if ci != co:
                w(f"res{i}.ws", (co, ci, 1), ci); b(f"res{i}.bs", co)
        w("down0.w", (c1, c0, 3), 3 * c0); b("down0.b", c1)
        w("down1.w", (c2, c1, 3), 3 * c1); b("down1.b", c2)
        w("up1.w", (c1, c2, 3), 3 * c2); b("up1.b", c1)
        w("up0.w", (c0, c1, 3), 3 * c1); b("up0.b", c0)
        w("conv_out.w", (1, c0, 3), 3 * c0); b("conv_out.b", 1)
        return p

    def n_params(self) -> int:
        return sum(v.numel() for v in self.params.values())

    def step_cost(self, n: int, weight_bytes: int = 2) -> Dict[str, float]:
        """Algorithmic work of one reverse step at batch ``n`` (bench.py config5.unet_roofline):
        FLOPs = 2 n Cout L_out Cin k summed over the convs (the 1x1 shortcuts are segments of
        their block's second conv: 18 launches); bytes = every weight once (``weight_bytes`` per
        element) + every fp32 activation a conv reads (input window, identity residual) and
        writes, + the latent in / out of the step."""
        sh = unet_shapes(self.D, self.C)
        plan = unet_plan(self.C)
        flops = wbytes = abytes = 0
        for r in plan:
            co, Lout = sh[r.out]
            for s in r.segs:
                ci, Lin = sh[s.x]
                flops += 2 * n * co * Lout * ci * s.ksize
                wbytes += weight_bytes * co * ci * s.ksize
                # the output write is counted once per weight: a 1x1 shortcut as its own conv
                abytes += 4 * n * (ci * Lin + (0 if s.ordinal else co * Lout))
            if r.R is not None:
                abytes += 4 * n * co * Lout
        return {"flops": float(flops), "bytes": float(wbytes + abytes),
                "weight_bytes": float(wbytes), "activation_bytes": float(abytes),
                "launches": len(plan)}

    def invalidate(self) -> None:
        self._dev.clear()
        self._trainers = {}

    # ------------------------------------------------------------------------- training
    def names(self) -> List[str]:
        return list(self.params)

    def _first_half(self, name: str) -> Optional[int]:
        """Channels of the first operand of a decoder-side concat conv ([u || s]), else None."""
        for r in unet_plan(self.C):
            xs = [s.x for s in r.segs if s.w == name]
            if len(xs) > 1:
                return unet_shapes(self.D, self.C)[xs[0]][0]
        return None

    def pack_train(self, name: str, v: torch.Tensor) -> torch.Tensor:
        """Torch layout -> training layout (device tensors): conv weights packed for the matrix
        cores; a concat conv's two operands are packed side by side, EACH padded to 16 channels,
        so the second segment starts at a multiple of 16 whatever the widths (for widths that
        are multiples of 16 this is ``pack_conv_weight`` of the whole weight)."""
        if not is_conv_weight(name):
            return v.contiguous().clone()
        c = self._first_half(name)
        if c is None:
            return ops.pack_conv_weight(v)
        return torch.cat([ops.pack_conv_weight(v[:, :c]), ops.pack_conv_weight(v[:, c:])], dim=2)

    def unpack_train(self, name: str, v: torch.Tensor) -> torch.Tensor:
        """The inverse of ``pack_train`` (device tensors)."""
        if not is_conv_weight(name):
            return v
        co, cw, _ = self.params[name].shape
        c = self._first_half(name)
        if c is None:
            return ops.unpack_conv_weight(v, co, cw)
        h = ops._r16(c)
        return torch.cat([ops.unpack_conv_weight(v[:, :, :h].contiguous(), co, c),
                          ops.unpack_conv_weight(v[:, :, h:].contiguous(), co, cw - c)], dim=1)

    def export_tensor(self, name: str, v: torch.Tensor) -> torch.Tensor:
        """A training-layout tensor -> torch layout on the host."""
        return self.unpack_train(name, v).detach().to("cpu", torch.float32).contiguous()

    def import_tensor(self, name: str, v: torch.Tensor, device) -> torch.Tensor:
        """A torch-layout tensor -> the training layout on ``device`` (fp32)."""
        return self.pack_train(name, v.detach().to(device, torch.float32))

    def train_masters(self, device) -> Dict[str, torch.Tensor]:
        """fp32 masters in the training layout (a fresh copy of ``params``)."""
        return {n: self.import_tensor(n, v, device) for n, v in self.params.items()}

    def trainer(self, dtype: str, device, B: int) -> "UNetTrainer":
        """A cached trainer over ``params`` as they were when it was built (``api.train_step``);
        ``invalidate()`` drops it, as it drops the sampling packs."""
        key = (dtype, torch.device(device), B)
        if key not in self._trainers:
            masters = self.train_masters(device)
            self._trainers[key] = UNetTrainer(self, masters, make_work(masters, dtype), B, device)
        return self._trainers[key]

    # ------------------------------------------------------------------------- device pack
    def device_pack(self, dtype: str, device) -> Dict[str, object]:
        """Weights in ``dtype`` (fp32 | bf16; biases fp32) on ``device`` plus the per-block
        E tables ``[T, Cout_i]`` computed on the device (ldm_linear)."""
        device = torch.device(device)
        key = (dtype, device)
        if key in self._dev:
            return self._dev[key]
        wdt = {"fp32": torch.float32, "bf16": torch.bfloat16}[dtype]
        dev: Dict[str, object] = {}
        for n, v in self.params.items():
            v = v.to(device)
            if is_conv_weight(n):         # matrix-core packing of the whole weight (sample_c_off)
                dev[n] = ops.pack_conv_weight(v.to(wdt))
            elif is_linear_weight(n):     # [out][in]
                dev[n] = v.to(wdt).contiguous()
            else:
                dev[n] = v.to(torch.float32).contiguous()
        emb = self.emb_table.to(device).contiguous()
        temb = ops.temb_forward(dev, emb, self.HT)                      # [T, HT]
        for i, (_, co) in enumerate(unet_res_specs(self.C)):
            E = torch.empty(self.T, co, device=device, dtype=torch.float32)
            ops.linear(temb, dev[f"res{i}.p"], E, epi=capi.EPI_BIAS, bias=dev[f"res{i}.b1"])
            dev[f"etab{i}"] = E
        self._dev[key] = dev
        return dev

    # ------------------------------------------------------------------------- forward
    def buffers(self, n: int, device) -> Dict[str, torch.Tensor]:
        """Activation buffers for a batch of ``n`` (allocated once per sampler), by plan name;
        ``a3`` is ``a2`` again (nothing reads res2's inner activation after res3 starts)."""
        sh = unet_shapes(self.D, self.C)
        f = lambda name: torch.empty(n, *sh[name], device=device, dtype=torch.float32)  # noqa
        b = {name: f(name) for name in sh if name not in ("x", "a3", "cat1", "cat0")}
        b["a3"] = b["a2"]
        if n == 1:
            # the decoder-side skip concats [u || s] as ONE buffer whose halves the producers
            # write (unet_plan's fused_concat); a channel slice is contiguous only at n = 1
            for lvl in (1, 0):
                cat, c = f(f"cat{lvl}"), sh[f"u{lvl}"][0]
                b[f"cat{lvl}"], b[f"u{lvl}"], b[f"s{lvl}"] = cat, cat[:, :c], cat[:, c:]
        return b

    def step_args(self, dev: Dict[str, object], buf: Dict[str, torch.Tensor], x: torch.Tensor,
                  t: int, *, out: torch.Tensor, sched=None, z: Optional[torch.Tensor] = None,
                  cbias: Optional[List[torch.Tensor]] = None) -> List[capi.ConvArgs]:
        """The 18 ``ldm_conv1d`` calls of one forward at a batch-uniform ``t``.

        With ``sched`` the last call writes the A8 reverse step ``x_{t-1}`` into ``out``
        ([n, D]); without, it writes eps_hat.  ``cbias`` overrides the tabulated per-block
        bias rows (training: per-sample ``[n, Cout_i]``)."""
        n = x.shape[0]
        bufs = {**buf, "x": x.view(n, 1, self.D), "eps": out.view(n, 1, self.D)}
        cb = ((lambda i: (dev[f"etab{i}"][t], 0)) if cbias is None else
              (lambda i: (cbias[i], cbias[i].shape[1])))
        ddpm = None if sched is None else dict(xlat=x, z=z, sched=sched, t=t)
        return bind_plan(unet_plan(self.C, "cat1" in buf), dev, bufs, cb, sample_c_off, ddpm)

    def forward_uniform_t(self, x: torch.Tensor, t: int, dtype: str = "bf16") -> torch.Tensor:
        """eps_hat = UNet(x, t) for a batch sharing one timestep (device tensors)."""
        capi.require_device(x)
        dev = self.device_pack(dtype, x.device)
        buf = self.buffers(x.shape[0], x.device)
        eps = torch.empty(x.shape[0], self.D, device=x.device, dtype=torch.float32)
        x = x.float().contiguous()
        for a in self.step_args(dev, buf, x, t, out=eps):
            ops.conv1d_launch(a, x.device)
        return eps

    def make_stepper(self, n: int, dtype: str, device, sched_desc):
        """Callable ``step(x, z, t, x_out)`` = one fused reverse step (for ``api.Sampler``)."""
        dev = self.device_pack(dtype, device)
        buf = self.buffers(n, device)

        def step(x, z, t, x_out):
            for a in self.step_args(dev, buf, x, t, out=x_out, sched=sched_desc, z=z):
                ops.conv1d_launch(a, device)
        return step


class UNetTrainer:
    """One training forward/backward of the UNet at per-sample timesteps for a fixed batch
    (DESIGN.md §15).  Every buffer and every C argument struct is built once; a step only
    launches: q_sample, the timestep MLP, 18 ``ldm_conv1d``, eps-MSE, then the 18 convs in
    reverse (``ldm_conv1d_bwd_weight`` per conv, ``ldm_conv1d_bwd_data`` per segment, in this
    fixed order: no atomics) and the timestep-MLP backward (``ldm_linear`` exact fp32,
    ``ldm_silu_bwd``, ``ldm_colsum``).

    ``masters`` / ``work``: training-layout tensors (convs packed; ``work`` is what the kernels
    read).  ``grads``: fp32, conv weights in the packed layout (zero padding), the rest in
    parameter shape."""

    def __init__(self, model: UNet1DDenoiser, masters, work, B: int, device):
        self.model, self.masters, self.work, self.B = model, masters, work, B
        self.device = device = torch.device(device)
        f = lambda *s: torch.empty(*s, device=device, dtype=torch.float32)  # noqa: E731
        self.plan = unet_plan(model.C)
        used = {s.x for r in self.plan for s in r.segs} | {r.out for r in self.plan}
        # every activation the backward needs is kept (the sampler reuses a2 for res2 / res3)
        self.act = {n: f(B, *s) for n, s in unet_shapes(model.D, model.C).items() if n in used}
        self.grads = {n: torch.zeros_like(v) for n, v in masters.items()}
        specs = unet_res_specs(model.C)
        self.cb = [f(B, co) for _, co in specs]
        self.dcb = [f(B, co) for _, co in specs]
        self.dtemb, self.du = f(B, model.HT), f(B, model.HT)
        self.emb = model.emb_table.to(device).contiguous()
        self.fwd = bind_plan(self.plan, work, self.act,
                             lambda i: (self.cb[i], self.cb[i].shape[1]), train_c_off)
        self._bind_backward()

    def _bind_backward(self) -> None:
        """``backward_schedule`` over tensors: the argument structs in launch order (``bwd``),
        the bias copies, one gradient buffer per activation (``G``) and the workspace."""
        plan, act, grads = self.plan, self.act, self.grads
        segs = [bind_segments(r, self.work, act, train_c_off) for r in plan]
        G: Dict[str, torch.Tensor] = {"eps": torch.empty_like(act["eps"])}
        self.g_eps = G["eps"]
        self.bwd: List[tuple] = []
        self.copies: List[tuple] = []
        ws_need = 1
        for kind, *e in backward_schedule(plan):
            if kind == "w":
                k, dbias, cb = e
                wa = ops.conv1d_bwd_weight_args(
                    segs[k], G[plan[k].out], [grads[s.w] for s in plan[k].segs],
                    dbias=grads[dbias], dcbias=None if cb is None else self.dcb[cb])
                ws_need = max(ws_need, ops.conv1d_bwd_weight_ws_floats(wa))
                self.bwd.append(("w", wa))
            elif kind == "copy":
                self.copies.append((grads[e[0]], grads[e[1]]))
            elif kind == "alias":
                G[e[0]] = G[e[1]]
            else:
                k, j, accumulate = e
                x = plan[k].segs[j].x
                if not accumulate:
                    G[x] = torch.empty_like(act[x])
                self.bwd.append(("d", ops.conv1d_bwd_data_args(segs[k][j], G[plan[k].out], G[x],
                                                               accumulate)))
        self.G = G
        self.ws = torch.empty(ws_need, device=self.device, dtype=torch.float32)
        for kind, a in self.bwd:
            if kind == "w":
                a.ws, a.ws_floats = self.ws.data_ptr(), self.ws.numel()

    def step(self, sched_desc, x0: torch.Tensor, t: torch.Tensor, eps: torch.Tensor
             ) -> torch.Tensor:
        """q_sample -> forward -> eps-MSE -> every gradient (into ``grads``); the loss [1]."""
        m, work, grads, B = self.model, self.work, self.grads, self.B
        capi.require_device(x0, t, eps)
        if tuple(x0.shape) != (B, m.D) or tuple(eps.shape) != (B, m.D) or t.numel() != B:
            raise capi.LdmError(f"UNetTrainer: built for x0 / eps [{B}, {m.D}] and t [{B}]")
        x0, eps = x0.float().contiguous(), eps.float().contiguous()
        t = t.to(torch.int32).contiguous()
        lib, st = capi.load(), capi.stream_handle(self.device)
        capi.check(lib.ldm_q_sample(ctypes.byref(sched_desc), x0.data_ptr(), eps.data_ptr(),
                                    t.data_ptr(), B, m.D, self.act["x"].data_ptr(), st),
                   "ldm_q_sample")
        sv: dict = {}
        temb = ops.temb_forward(work, ops.gather_rows(self.emb, t), m.HT, save=sv)
        for i in range(6):
            ops.linear(temb, work[f"res{i}.p"], self.cb[i], epi=capi.EPI_BIAS,
                       bias=work[f"res{i}.b1"])
        for a in self.fwd:
            capi.check(lib.ldm_conv1d(ctypes.byref(a), st), "ldm_conv1d")
        loss = torch.empty(1, device=self.device, dtype=torch.float32)
        capi.check(lib.ldm_eps_mse_loss(self.act["eps"].data_ptr(), eps.data_ptr(), eps.numel(),
                                        loss.data_ptr(), self.g_eps.data_ptr(), st),
                   "ldm_eps_mse_loss")
        for kind, a in self.bwd:
            if kind == "w":
                capi.check(lib.ldm_conv1d_bwd_weight(ctypes.byref(a), st), "ldm_conv1d_bwd_weight")
            else:
                capi.check(lib.ldm_conv1d_bwd_data(ctypes.byref(a), st), "ldm_conv1d_bwd_data")
        for dst, src in self.copies:
            dst.copy_(src)
        # cbias_i = P_i temb + b1_i: dP_i = dcb_i^T temb, dtemb = sum_i dcb_i P_i (block order)
        for i in range(6):
            ops.linear(self.dcb[i].T, temb.T, grads[f"res{i}.p"])
            ops.linear(self.dcb[i], work[f"res{i}.p"].T, self.dtemb,
                       epi=capi.EPI_BIAS if i == 0 else capi.EPI_ACCUM)
        # temb = Wt2 u + bt2, u = SiLU(a_t), a_t = Wt1 e + bt1
        ops.linear(self.dtemb.T, sv["u"].T, grads["Wt2"])
        ops.colsum(self.dtemb, grads["bt2"])
        ops.linear(self.dtemb, work["Wt2"].T, self.du)
        gt = ops.silu_bwd(self.du, sv["a_t"])
        ops.linear(gt.T, sv["e"].T, grads["Wt1"])
        ops.colsum(gt, grads["bt1"])
        return loss

    def export_grads(self) -> Dict[str, torch.Tensor]:
        """The gradients in torch layout, on the device (conv weights unpacked)."""
        return {n: self.model.unpack_train(n, g) for n, g in self.grads.items()}
