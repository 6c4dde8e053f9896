"""Decoder input gradients against the routes a user had before them.

In ONE process, the two routes of each comparison alternating per repetition, HIP events around
each, 3 warm-ups and the median of 10 (the form of scripts/bench_band.py):

  normals   the vertices of the config-4 256^3 mesh (decoder seed 1234, latent randn(seed 0) x
            0.1): ``sdf_grad`` against central differences, six ``decode_points`` calls.
  latent    64 shapes x 16384 samples: gradient kernel (loss mode) + reduction +
            ``ldm_decoder_fold_bwd`` against ``autodecoder_train_step`` -- which ALSO computes
            every weight gradient, most of its work; it is the only route to a latent gradient
            without this kernel.
  rate      points/s of the kernel alone and the fraction of the dense 16-bit peak at
            2 x 2 x forward MACs per point (forward + backward, 2 flops per MAC).

Prints one JSON line; --out also writes it to a file.

    python scripts/bench_grad.py [--out FILE] [--peak-tflops 2516]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "latent-diffusion-models-for-shape-sdfs_amd")]
import torch  # noqa: E402
import ldm_sdf  # noqa: E402
from ldm_sdf import ops  # noqa: E402

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


def forward_macs(skip_width):
    s = 256 if skip_width == 253 else 512           # the padded widths the kernel multiplies
    return 5 * 512 * 512 + 2 * 512 * s + 512 * 3 * 2 + 512


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--peak-tflops", type=float, default=2516.0,
                    help="dense fp16 / bf16 matrix peak of the device")
    ap.add_argument("--grid", type=int, default=256)
    ap.add_argument("--fd-step", type=float, default=1e-3)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    dec = ldm_sdf.SDFDecoder(256, seed=1234)
    res = {"metric": "decoder input gradients vs the routes without them", "warmup": WARM,
           "reps": REPS, "timer": "hipEvent pair per call, median",
           "device": torch.cuda.get_device_name(0)}

    # ---- normals
    z = (torch.randn(1, 256, generator=torch.Generator().manual_seed(0)) * 0.1).to(dev)
    vol = ldm_sdf.decode(dec, z, args.grid, dtype="bf16")
    verts, faces = ldm_sdf.marching_cubes(vol[0])
    del vol
    pts = verts[None].contiguous()
    h = args.fd_step
    offs = torch.tensor([[h, 0, 0], [-h, 0, 0], [0, h, 0], [0, -h, 0], [0, 0, h], [0, 0, -h]],
                        device=dev)

    def central():
        f = [ldm_sdf.decode_points(dec, z, pts + offs[i], dtype="fp16") for i in range(6)]
        return torch.stack([f[0] - f[1], f[2] - f[3], f[4] - f[5]], dim=2) / (2 * h)

    def kernel_normals():
        return ldm_sdf.sdf_grad(dec, z, pts, dtype="fp16")[1]

    t, last = alternate({"sdf_grad": kernel_normals, "central_differences": central})
    a, b = last["sdf_grad"][0], last["central_differences"][0]
    cos = torch.nn.functional.cosine_similarity(a, b, dim=1)
    res["normals"] = {"vertices": int(verts.shape[0]), "grid": args.grid, "dtype": "fp16",
                      "fd_step": h, **t,
                      "speedup": t["central_differences"]["median_ms"] / t["sdf_grad"]["median_ms"],
                      "median_angle_deg_between_routes":
                          float(torch.rad2deg(torch.acos(cos.clamp(-1, 1))).median())}

    # ---- latent gradient
    S, P, L = 64, 16384, 256
    g = torch.Generator().manual_seed(1)
    zz = (torch.randn(S, L, generator=g) * 0.1).to(dev)
    xyz = (torch.rand(S, P, 3, generator=g) * 2 - 1).to(dev)
    gt = (0.3 * (xyz.norm(dim=2) - 0.5)).contiguous()
    fdesc = dec.device_pack("bf16", dev)["desc"]
    gdesc = dec.device_pack_grad("bf16", dev)["desc"]
    ws = torch.empty(ops.decoder_grad_ws_bytes(S, P, gdesc.dtype), device=dev, dtype=torch.uint8)
    dz = torch.empty(S, L, device=dev)

    def frozen():
        beta = ops.decoder_fold(fdesc, zz)
        out = ops.decoder_points_grad(gdesc, beta, xyz, gt=gt, delta=0.1, scale=1.0 / (S * P),
                                      want_dxyz=False, want_dbeta=True, want_loss=True, ws=ws)
        return ops.decoder_fold_bwd(gdesc, out["dbeta"], out=dz)

    masters = {}
    for l in range(9):
        masters[f"W{l}"] = dec.weights[l].to(dev).clone()
        masters[f"b{l}"] = dec.biases[l].to(dev).clone()
    grads = {k: torch.empty_like(v) for k, v in masters.items()}

    def train_step():
        return ldm_sdf.autodecoder_train_step(masters, zz, xyz, gt, latent_dim=L, hidden=512,
                                              skip=4, delta=0.1, reg_lambda=0.0, epoch=100,
                                              dtype="bf16", grads=grads)[2]

    t, last = alternate({"frozen_kernel": frozen, "autodecoder_train_step": train_step})
    gz = last["autodecoder_train_step"]
    res["latent_gradient"] = {
        "shapes": S, "samples": P, "dtype": "bf16", **t,
        "note": "autodecoder_train_step also computes all weight gradients",
        "speedup": t["autodecoder_train_step"]["median_ms"] / t["frozen_kernel"]["median_ms"],
        "dz_max_rel_between_routes": float((last["frozen_kernel"] - gz).abs().max() /
                                           gz.abs().max())}

    # ---- the kernel alone
    rate = {}
    beta = ops.decoder_fold(fdesc, zz)
    for dtype in ("fp16", "bf16"):
        gd = dec.device_pack_grad(dtype, dev)["desc"]
        t, _ = alternate({"k": lambda: ops.decoder_points_grad(gd, beta, xyz, ws=ws)})
        ms = t["k"]["median_ms"]
        flops = 2 * 2 * forward_macs(253) * S * P
        rate[dtype] = {"median_ms": ms, "points_per_s": S * P / (ms * 1e-3),
                       "tflops": flops / (ms * 1e-3) / 1e12,
                       "fraction_of_peak": flops / (ms * 1e-3) / (args.peak_tflops * 1e12)}
    res["kernel_rate"] = {"points": S * P, "forward_macs_per_point": forward_macs(253),
                          "peak_tflops": args.peak_tflops, **rate}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
