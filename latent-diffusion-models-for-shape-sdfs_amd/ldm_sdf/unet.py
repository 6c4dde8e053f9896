"""C17: 1D-UNet eps-denoiser over a latent code seen as a 1-channel signal (config 5:
1024-d latents).  Architecture: DESIGN.md §9 (the same network as ``oracle/ref_unet.py``).

Every conv runs in ``ldm_conv1d`` (``csrc/unet.hip``); a reverse step is 18 launches:

    conv_in | Res_0 (2) | down0 | Res_1 (2) | down1 | Res_2 (2) | Res_3 (2) | up1 |
    Res_4 (2, concat as two segments) | up0 | Res_5 (2) | conv_out + DDPM step (A8)

The timestep-embedding MLP and each block's projection are tabulated for all t once per
weight version (``E_i[t] = P_i temb(t) + b1_i``, fp32 ``[T, Cout_i]``), so a sampling step
reads one table row per block as a per-channel bias (A5's table trick, as for the MLP).

Training (``UNetTrainer``) runs the same 18 convs at per-sample timesteps and
walks them in reverse through ``ldm_conv1d_bwd_weight`` / ``ldm_conv1d_bwd_data``
(``csrc/unet_bwd.hip``).
"""
from __future__ import annotations

import math
from typing import Dict, List, Optional, Tuple

import torch

from . import _capi as capi
from . import ops
from .models import timestep_embedding_table


CONV_SUFFIXES = (".w", ".w1", ".w2", ".ws")


def is_conv_weight(name: str) -> bool:
    return name.endswith(CONV_SUFFIXES)


def is_linear_weight(name: str) -> bool:
    return name.startswith("W") or name.endswith(".p")


def make_work(masters: Dict[str, torch.Tensor], dtype: str) -> Dict[str, torch.Tensor]:
    """The weights the kernels read: the fp32 masters themselves, or bf16 copies (RNE) of every
    conv / linear weight with the fp32 biases."""
    if dtype == "fp32":
        return dict(masters)
    if dtype != "bf16":
        raise capi.LdmError(f"UNet training dtype {dtype!r} (fp32 | bf16)")
    return {n: v.to(torch.bfloat16) if is_conv_weight(n) or is_linear_weight(n) else v
            for n, v in masters.items()}


def unet_res_specs(C: Tuple[int, int, int]) -> List[Tuple[int, int]]:
    """(cin, cout) of the six residual blocks in execution order."""
    c0, c1, c2 = C
    return [(c0, c0), (c1, c1), (c2, c2), (c2, c2), (2 * c1, c1), (2 * c0, c0)]


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

    def conv_list(self) -> List[Tuple[str, int, int, int, int, int, bool]]:
        """The 18 convs of one forward, in launch order: (name, cin (all segments, the 1x1
        shortcut's included as k=1 taps below), cout, k, L_in, L_out, identity residual)."""
        c0, c1, c2 = self.C
        D = self.D
        out = [("conv_in", 1, c0, 3, D, D, False)]
        lv = {0: (c0, D), 1: (c1, D // 2), 2: (c2, D // 4), 3: (c2, D // 4), 4: (c1, D // 2),
              5: (c0, D)}

        def res(i):
            ci, co = unet_res_specs(self.C)[i]
            L = lv[i][1]
            out.append((f"res{i}.w1", ci, co, 3, L, L, False))
            out.append((f"res{i}.w2", co, co, 3, L, L, ci == co))
            if ci != co:
                out.append((f"res{i}.ws", ci, co, 1, L, L, False))
        res(0)
        out.append(("down0", c0, c1, 3, D, D // 2, False))
        res(1)
        out.append(("down1", c1, c2, 3, D // 2, D // 4, False))
        res(2)
        res(3)
        out.append(("up1", c2, c1, 3, D // 4, D // 2, False))
        res(4)
        out.append(("up0", c1, c0, 3, D // 2, D, False))
        res(5)
        out.append(("conv_out", c0, 1, 3, D, D, False))
        return out

    def step_cost(self, n: int, weight_bytes: int = 2) -> Dict[str, float]:
        """Algorithmic work of one reverse step at batch ``n`` (bench.py config5.unet_roofline):
        FLOPs = 2 n Cout L_out Cin k summed over the convs (the 1x1 shortcuts are segments of
        their block's second conv: 18 launches); bytes = every weight once (``weight_bytes`` per
        element) + every fp32 activation a conv reads (input window, identity residual) and
        writes, + the latent in / out of the step."""
        flops = 0
        wbytes = 0
        abytes = 0
        for (_, ci, co, k, Lin, Lout, ident) in self.conv_list():
            flops += 2 * n * co * Lout * ci * k
            wbytes += weight_bytes * co * ci * k
            abytes += 4 * n * (ci * Lin + co * Lout + (co * Lout if ident else 0))
        return {"flops": float(flops), "bytes": float(wbytes + abytes),
                "weight_bytes": float(wbytes), "activation_bytes": float(abytes),
                "launches": 18}

    def invalidate(self) -> None:
        self._dev.clear()
        self._trainers = {}

    # ------------------------------------------------------------------------- training
    def names(self) -> List[str]:
        return list(self.params)

    def _first_half(self, name: str) -> Optional[int]:
        """Channels of the first operand of a decoder-side concat conv ([u || s]), else None."""
        c0, c1, _ = self.C
        return {"res4.w1": c1, "res4.ws": c1, "res5.w1": c0, "res5.ws": c0}.get(name)

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
        tr = getattr(self, "_trainers", {})
        if key not in tr:
            masters = self.train_masters(device)
            tr[key] = UNetTrainer(self, masters, make_work(masters, dtype), B, device)
            self._trainers = tr
        return tr[key]

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
            if n.endswith((".w", ".w1", ".w2", ".ws")):        # conv: matrix-core packing
                dev[n] = ops.pack_conv_weight(v.to(wdt))
            elif n.startswith("W") or n.endswith(".p"):       # linear [out][in]
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
        """Activation buffers for a batch of ``n`` (allocated once per sampler)."""
        c0, c1, c2 = self.C
        D = self.D
        f = lambda *s: torch.empty(*s, device=device, dtype=torch.float32)  # noqa: E731
        b = {"h0": f(n, c0, D), "a0": f(n, c0, D), "s0": f(n, c0, D),
             "d0": f(n, c1, D // 2), "a1": f(n, c1, D // 2), "s1": f(n, c1, D // 2),
             "d1": f(n, c2, D // 4), "a2": f(n, c2, D // 4), "m0": f(n, c2, D // 4),
             "m1": f(n, c2, D // 4), "u1": f(n, c1, D // 2), "a4": f(n, c1, D // 2),
             "r4": f(n, c1, D // 2), "u0": f(n, c0, D), "a5": f(n, c0, D),
             "r5": f(n, c0, D), "eps": f(n, 1, D)}
        if n == 1:
            # the decoder-side skip concats [u || s] as ONE buffer whose halves the producers
            # write: res4 / res5 then read it as one segment (one staging segment fewer in
            # their two convs); a channel slice is contiguous only at n = 1
            for lvl, c in ((1, c1), (0, c0)):
                cat = f(1, 2 * c, D >> lvl)
                b[f"cat{lvl}"], b[f"u{lvl}"], b[f"s{lvl}"] = cat, cat[:, :c], cat[:, c:]
        return b

    def step_args(self, dev: Dict[str, object], buf: Dict[str, torch.Tensor], x: torch.Tensor,
                  t: int, *, out: torch.Tensor, sched=None, z: Optional[torch.Tensor] = None,
                  cbias: Optional[List[torch.Tensor]] = None) -> List[capi.ConvArgs]:
        """The 18 ``ldm_conv1d`` calls of one forward at a batch-uniform ``t``.

        With ``sched`` the last call writes the A8 reverse step ``x_{t-1}`` into ``out``
        ([n, D]); without, it writes eps_hat.  ``cbias`` overrides the tabulated per-block
        bias rows (training: per-sample ``[n, Cout_i]``)."""
        S = ops.ConvSegment
        UP2 = capi.CONV_UP2
        n = x.shape[0]
        calls: List[capi.ConvArgs] = []

        def cb(i):
            if cbias is not None:
                return dict(cbias=cbias[i], scb=cbias[i].shape[1])
            return dict(cbias=dev[f"etab{i}"][t], scb=0)

        def res(i, xin: List[torch.Tensor], a, y):
            w1, w2 = dev[f"res{i}.w1"], dev[f"res{i}.w2"]
            segs, off = [], 0
            for xi in xin:
                segs.append(S(xi, w1, c_off=off, silu=True))
                off += xi.shape[1]
            calls.append(ops.conv1d_args(segs, a, **cb(i)))
            segs2 = [S(a, w2, silu=True)]
            if f"res{i}.ws" in dev:
                ws, off = dev[f"res{i}.ws"], 0
                for xi in xin:
                    segs2.append(S(xi, ws, c_off=off))
                    off += xi.shape[1]
                calls.append(ops.conv1d_args(segs2, y, bias=dev[f"res{i}.b2"],
                                             bias2=dev[f"res{i}.bs"]))
            else:
                calls.append(ops.conv1d_args(segs2, y, bias=dev[f"res{i}.b2"], R=xin[0]))

        b = buf
        x3 = x.view(n, 1, self.D)
        calls.append(ops.conv1d_args([S(x3, dev["conv_in.w"])], b["h0"], bias=dev["conv_in.b"]))
        res(0, [b["h0"]], b["a0"], b["s0"])
        calls.append(ops.conv1d_args([S(b["s0"], dev["down0.w"], stride=2)], b["d0"],
                                     bias=dev["down0.b"]))
        res(1, [b["d0"]], b["a1"], b["s1"])
        calls.append(ops.conv1d_args([S(b["s1"], dev["down1.w"], stride=2)], b["d1"],
                                     bias=dev["down1.b"]))
        res(2, [b["d1"]], b["a2"], b["m0"])
        res(3, [b["m0"]], b["a2"], b["m1"])
        calls.append(ops.conv1d_args([S(b["m1"], dev["up1.w"], mode=UP2)], b["u1"],
                                     bias=dev["up1.b"]))
        res(4, [b["cat1"]] if "cat1" in b else [b["u1"], b["s1"]], b["a4"], b["r4"])
        calls.append(ops.conv1d_args([S(b["r4"], dev["up0.w"], mode=UP2)], b["u0"],
                                     bias=dev["up0.b"]))
        res(5, [b["cat0"]] if "cat0" in b else [b["u0"], b["s0"]], b["a5"], b["r5"])
        last = [S(b["r5"], dev["conv_out.w"], silu=True)]
        if sched is not None:
            calls.append(ops.conv1d_args(last, out.view(n, 1, self.D), bias=dev["conv_out.b"],
                                         epi=capi.CONV_EPI_DDPM, xlat=x, z=z, sched=sched, t=t))
        else:
            calls.append(ops.conv1d_args(last, out.view(n, 1, self.D), bias=dev["conv_out.b"]))
        return calls

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
        c0, c1, c2 = model.C
        D = model.D
        f = lambda *s: torch.empty(*s, device=device, dtype=torch.float32)  # noqa: E731
        shapes = {"x": (1, D), "h0": (c0, D), "a0": (c0, D), "s0": (c0, D),
                  "d0": (c1, D // 2), "a1": (c1, D // 2), "s1": (c1, D // 2),
                  "d1": (c2, D // 4), "a2": (c2, D // 4), "m0": (c2, D // 4),
                  "a3": (c2, D // 4), "m1": (c2, D // 4), "u1": (c1, D // 2),
                  "a4": (c1, D // 2), "r4": (c1, D // 2), "u0": (c0, D), "a5": (c0, D),
                  "r5": (c0, D), "eps": (1, D)}
        # every activation the backward needs is kept (the sampler reuses a2 for res2 / res3)
        self.act = {n: f(B, *s) for n, s in shapes.items()}
        self.grads = {n: torch.zeros_like(v) for n, v in masters.items()}
        specs = unet_res_specs(model.C)
        self.cb = [f(B, co) for _, co in specs]
        self.dcb = [f(B, co) for _, co in specs]
        self.loss = f(1)
        self.dtemb, self.du = f(B, model.HT), f(B, model.HT)
        self.emb = model.emb_table.to(device).contiguous()
        self._build()

    def plan(self) -> List[dict]:
        """The 18 convs in launch order: output buffer, segments (input buffer, weight, channel
        offset, stride, mode, SiLU), biases, the block whose projection is the per-sample
        bias, and the identity residual."""
        UP2 = capi.CONV_UP2
        P: List[dict] = []

        def conv(out, segs, bias=None, bias2=None, cb=None, R=None):
            P.append(dict(out=out, segs=segs, bias=bias, bias2=bias2, cb=cb, R=R))

        def res(i, xin, a, y):
            segs, off = [], 0
            for xi in xin:
                segs.append((xi, f"res{i}.w1", off, 1, 0, True))
                off += ops._r16(self.act[xi].shape[1])      # UNet1DDenoiser.pack_train
            conv(a, segs, cb=i)
            segs2 = [(a, f"res{i}.w2", 0, 1, 0, True)]
            if f"res{i}.ws" in self.masters:
                off = 0
                for xi in xin:
                    segs2.append((xi, f"res{i}.ws", off, 1, 0, False))
                    off += ops._r16(self.act[xi].shape[1])
                conv(y, segs2, bias=f"res{i}.b2", bias2=f"res{i}.bs")
            else:
                conv(y, segs2, bias=f"res{i}.b2", R=xin[0])

        conv("h0", [("x", "conv_in.w", 0, 1, 0, False)], bias="conv_in.b")
        res(0, ["h0"], "a0", "s0")
        conv("d0", [("s0", "down0.w", 0, 2, 0, False)], bias="down0.b")
        res(1, ["d0"], "a1", "s1")
        conv("d1", [("s1", "down1.w", 0, 2, 0, False)], bias="down1.b")
        res(2, ["d1"], "a2", "m0")
        res(3, ["m0"], "a3", "m1")
        conv("u1", [("m1", "up1.w", 0, 1, UP2, False)], bias="up1.b")
        res(4, ["u1", "s1"], "a4", "r4")
        conv("u0", [("r4", "up0.w", 0, 1, UP2, False)], bias="up0.b")
        res(5, ["u0", "s0"], "a5", "r5")
        conv("eps", [("r5", "conv_out.w", 0, 1, 0, True)], bias="conv_out.b")
        return P

    def _build(self) -> None:
        S = ops.ConvSegment
        act, work, grads = self.act, self.work, self.grads
        self.fwd: List[capi.ConvArgs] = []
        recs = []
        for r in self.plan():
            segs = [S(act[xi], work[w], c_off=off, stride=st, mode=mode, silu=silu)
                    for (xi, w, off, st, mode, silu) in r["segs"]]
            kw = {}
            if r["cb"] is not None:
                kw = dict(cbias=self.cb[r["cb"]], scb=self.cb[r["cb"]].shape[1])
            self.fwd.append(ops.conv1d_args(
                segs, act[r["out"]], bias=None if r["bias"] is None else work[r["bias"]],
                bias2=None if r["bias2"] is None else work[r["bias2"]],
                R=None if r["R"] is None else act[r["R"]], **kw))
            recs.append((r, segs))
        # the backward: convs in reverse; an activation's gradient buffer is written by its
        # first consumer (in this order) and accumulated by the later ones; an identity
        # residual makes the block input's gradient START as the block output's (one buffer)
        G: Dict[str, torch.Tensor] = {"eps": torch.empty_like(act["eps"])}
        self.g_eps = G["eps"]
        self.bwd: List[tuple] = []
        self.copies: List[tuple] = []
        ws_need = 1
        for r, segs in reversed(recs):
            dY = G[r["out"]]
            i = r["cb"]
            wa = ops.conv1d_bwd_weight_args(
                segs, dY, [grads[w] for (_, w, *_r) in r["segs"]],
                dbias=grads[f"res{i}.b1"] if i is not None else grads[r["bias"]],
                dcbias=self.dcb[i] if i is not None else None)
            ws_need = max(ws_need, ops.conv1d_bwd_weight_ws_floats(wa))
            self.bwd.append(("w", wa))
            if r["bias2"] is not None:       # the shortcut's bias shares the output: same sums
                self.copies.append((grads[r["bias2"]], grads[r["bias"]]))
            if r["R"] is not None:
                if r["R"] in G:
                    raise capi.LdmError("UNetTrainer: identity residual after another consumer")
                G[r["R"]] = dY
            for seg, (xi, *_r) in zip(segs, r["segs"]):
                if xi == "x":
                    continue                 # conv_in needs no data gradient
                accumulate = xi in G
                if not accumulate:
                    G[xi] = torch.empty_like(act[xi])
                self.bwd.append(("d", ops.conv1d_bwd_data_args(seg, dY, G[xi], accumulate)))
        self.G = G
        self.ws = torch.empty(ws_need, device=self.device, dtype=torch.float32)
        for kind, a in self.bwd:
            if kind == "w":
                a.ws, a.ws_floats = self.ws.data_ptr(), self.ws.numel()

    def step(self, sched_desc, x0: torch.Tensor, t: torch.Tensor, eps: torch.Tensor
             ) -> torch.Tensor:
        """q_sample -> forward -> eps-MSE -> every gradient (into ``grads``); the loss [1]."""
        import ctypes as C
        m, work, grads, B = self.model, self.work, self.grads, self.B
        capi.require_device(x0, t, eps)
        if tuple(x0.shape) != (B, m.D) or tuple(eps.shape) != (B, m.D) or t.numel() != B:
            raise capi.LdmError(f"UNetTrainer: built for x0 / eps [{B}, {m.D}] and t [{B}]")
        x0, eps = x0.float().contiguous(), eps.float().contiguous()
        t = t.to(torch.int32).contiguous()
        lib, st = capi.load(), capi.stream_handle(self.device)
        capi.check(lib.ldm_q_sample(C.byref(sched_desc), x0.data_ptr(), eps.data_ptr(),
                                    t.data_ptr(), B, m.D, self.act["x"].data_ptr(), st),
                   "ldm_q_sample")
        sv: dict = {}
        temb = ops.temb_forward(work, ops.gather_rows(self.emb, t), m.HT, save=sv)
        for i in range(6):
            ops.linear(temb, work[f"res{i}.p"], self.cb[i], epi=capi.EPI_BIAS,
                       bias=work[f"res{i}.b1"])
        for a in self.fwd:
            capi.check(lib.ldm_conv1d(C.byref(a), st), "ldm_conv1d")
        loss = torch.empty(1, device=self.device, dtype=torch.float32)
        capi.check(lib.ldm_eps_mse_loss(self.act["eps"].data_ptr(), eps.data_ptr(), eps.numel(),
                                        loss.data_ptr(), self.g_eps.data_ptr(), st),
                   "ldm_eps_mse_loss")
        for kind, a in self.bwd:
            if kind == "w":
                capi.check(lib.ldm_conv1d_bwd_weight(C.byref(a), st), "ldm_conv1d_bwd_weight")
            else:
                capi.check(lib.ldm_conv1d_bwd_data(C.byref(a), st), "ldm_conv1d_bwd_data")
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
