"""One training step of config 5's 1D-UNet (D = 1024, C = (32, 64, 128), B = 64) against what a
user would write without it: the same network in torch.nn.functional.conv1d with autograd on the
same GPU.

In ONE process, the legs alternating per repetition, HIP events around each, 3 warm-ups and the
median of 10 (the form of scripts/bench_grad.py):

  step       UNetTrainer.step (q_sample, forward, eps-MSE, every gradient) in fp32 and bf16
             weights; steps/s; the fraction of the fp32 MFMA peak at 3 x step_cost(B)["flops"]
             (forward + data gradient + weight gradient).
  torch      the torch / autograd network below (its own copy: the product and the scripts do not
             import oracle/), fp32, same inputs; the ratio as measured.  If torch's conv path
             cannot run on the machine the error text is recorded instead.
  breakdown  one fp32 step launch by launch: a HIP event pair around every C call, summed by kind.

Prints one JSON line; --out also writes it to a file.

    python scripts/bench_unet_train.py [--out FILE] [--batch 64] [--peak-tflops 157.3]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "latent-diffusion-models-for-shape-sdfs_amd")]
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402
import ldm_sdf  # noqa: E402
from ldm_sdf import _capi as capi  # noqa: E402

WARM, REPS = 3, 10


def timed(fn):
    e0, e1 = torch.cuda.Event(True), torch.cuda.Event(True)
    e0.record()
    r = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), r


def stats(ts):
    return {"median_ms": statistics.median(ts), "min_ms": min(ts), "max_ms": max(ts), "n": len(ts)}


def alternate(fns):
    ts = {k: [] for k in fns}
    last = {}
    for r in range(WARM + REPS):
        for k, fn in fns.items():
            t, last[k] = timed(fn)
            if r >= WARM:
                ts[k].append(t)
    return {k: stats(v) for k, v in ts.items()}, last


# ---- the torch leg: DESIGN.md §9's network, written the way a user would --------------------
def silu(x):
    return x * torch.sigmoid(x)


def torch_res(p, i, x, temb):
    a = F.conv1d(silu(x), p[f"res{i}.w1"], p[f"res{i}.b1"], padding=1)
    a = a + (temb @ p[f"res{i}.p"].T)[:, :, None]
    y = F.conv1d(silu(a), p[f"res{i}.w2"], p[f"res{i}.b2"], padding=1)
    if f"res{i}.ws" in p:
        return y + F.conv1d(x, p[f"res{i}.ws"], p[f"res{i}.bs"])
    return y + x


def torch_unet(p, x, e):
    temb = silu(e @ p["Wt1"].T + p["bt1"]) @ p["Wt2"].T + p["bt2"]
    h = F.conv1d(x[:, None, :], p["conv_in.w"], p["conv_in.b"], padding=1)
    s0 = torch_res(p, 0, h, temb)
    h = F.conv1d(s0, p["down0.w"], p["down0.b"], stride=2, padding=1)
    s1 = torch_res(p, 1, h, temb)
    h = F.conv1d(s1, p["down1.w"], p["down1.b"], stride=2, padding=1)
    h = torch_res(p, 3, torch_res(p, 2, h, temb), temb)
    h = F.conv1d(F.interpolate(h, scale_factor=2, mode="nearest"), p["up1.w"], p["up1.b"], padding=1)
    h = torch_res(p, 4, torch.cat([h, s1], dim=1), temb)
    h = F.conv1d(F.interpolate(h, scale_factor=2, mode="nearest"), p["up0.w"], p["up0.b"], padding=1)
    h = torch_res(p, 5, torch.cat([h, s0], dim=1), temb)
    return F.conv1d(silu(h), p["conv_out.w"], p["conv_out.b"], padding=1)[:, 0, :]


def breakdown(tr, sdesc, x0, t, eps):
    """One step with a HIP event pair around every C call of the library, summed by entry point
    (the events serialise nothing: the calls already run in stream order)."""
    lib = capi.load()
    names = ["ldm_q_sample", "ldm_gather_rows", "ldm_linear", "ldm_conv1d", "ldm_eps_mse_loss",
             "ldm_conv1d_bwd_weight", "ldm_conv1d_bwd_data", "ldm_silu_bwd", "ldm_colsum"]
    marks = []

    class Timed:
        def __init__(self, name, fn):
            self.name, self.fn = name, fn

        def __call__(self, *a):
            e0, e1 = torch.cuda.Event(True), torch.cuda.Event(True)
            e0.record()
            rc = self.fn(*a)
            e1.record()
            marks.append((self.name, e0, e1))
            return rc

    class Shim:
        def __getattr__(self, n):
            f = getattr(lib, n)
            return Timed(n, f) if n in names else f

    real = capi.load
    capi.load = lambda: Shim()
    try:
        tr.step(sdesc, x0, t, eps)
        torch.cuda.synchronize()
    finally:
        capi.load = real
    out = {}
    for n, e0, e1 in marks:
        d = out.setdefault(n, {"calls": 0, "ms": 0.0})
        d["calls"] += 1
        d["ms"] += e0.elapsed_time(e1)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--peak-tflops", type=float, default=157.3,
                    help="fp32 matrix (v_mfma_f32_16x16x4_f32) peak of the device")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    B = args.batch
    m = ldm_sdf.UNet1DDenoiser(seed=2468)
    sch = ldm_sdf.DDPMSchedule()
    sdesc = sch.device(dev)["desc"]
    g = torch.Generator().manual_seed(0)
    x0 = (torch.randn(B, m.D, generator=g) * 0.5).to(dev)
    eps = torch.randn(B, m.D, generator=g).to(dev)
    t = torch.randint(0, m.T, (B,), generator=g, dtype=torch.int32).to(dev)
    flops = 3 * m.step_cost(B)["flops"]
    res = {"metric": "UNet training step (config 5 network)", "D": m.D, "C": list(m.C), "B": B,
           "warmup": WARM, "reps": REPS, "timer": "hipEvent pair per step, median",
           "device": torch.cuda.get_device_name(0), "flops_per_step": flops,
           "peak_tflops": args.peak_tflops}

    tr = {dt: m.trainer(dt, dev, B) for dt in ("fp32", "bf16")}
    legs = {dt: (lambda d=dt: tr[d].step(sdesc, x0, t, eps)) for dt in tr}

    # the torch leg (fp32 parameters on the device, autograd)
    p = {n: v.to(dev).requires_grad_(True) for n, v in m.params.items()}
    emb = m.emb_table.to(dev)
    sa = torch.from_numpy(sch.tables64["sqrt_ab"]).float().to(dev)
    sb = torch.from_numpy(sch.tables64["sqrt_1mab"]).float().to(dev)

    def torch_step():
        for v in p.values():
            v.grad = None
        tl = t.long()
        xt = sa[tl][:, None] * x0 + sb[tl][:, None] * eps
        loss = ((eps - torch_unet(p, xt, emb[tl])) ** 2).mean()
        loss.backward()
        return loss.detach().reshape(1)

    try:
        torch_step()
        torch.cuda.synchronize()
        legs["torch_autograd_fp32"] = torch_step
    except Exception as e:  # noqa: BLE001  (recorded, not hidden: the torch leg is optional)
        res["torch_autograd_fp32"] = {"error": f"{type(e).__name__}: {str(e)[:300]}"}

    ts, last = alternate(legs)
    for k, v in ts.items():
        s = v["median_ms"] * 1e-3
        res[k] = {**v, "steps_per_s": 1.0 / s, "tflops": flops / s / 1e12,
                  "fraction_of_fp32_mfma_peak": flops / s / (args.peak_tflops * 1e12),
                  "loss": float(last[k])}
    if "torch_autograd_fp32" in ts:
        for dt in tr:
            res[dt]["speedup_vs_torch"] = ts["torch_autograd_fp32"]["median_ms"] / \
                ts[dt]["median_ms"]
        gt = tr["fp32"].export_grads()          # of the last fp32 step: the same inputs
        res["max_rel_grad_diff_vs_torch"] = max(
            float((gt[n] - p[n].grad).abs().max() / p[n].grad.abs().max()) for n in p)
    res["breakdown_fp32"] = breakdown(tr["fp32"], sdesc, x0, t, eps)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
