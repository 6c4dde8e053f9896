"""The Chamfer kernels at the sizes their users run.

    generation      ldm_sdf.evaluate_generation on --shapes x --shapes clouds of --points points
                    (512 x 512 x 2048: four directed passes, 4.4e12 point pairs); HIP events,
                    3 warm-ups and the median of 10
    reconstruction  ldm_sdf.chamfer_distance of two clouds of --recon-points points (30 000:
                    DeepSDF's own evaluation), same timing
    baseline        the same formulas (the differences first) as a chunked torch brute force on
                    the same GPU, written here, on the sub-block of the first --baseline-shapes x
                    --baseline-shapes (generated, reference) clouds; one distance tensor serves
                    both directions, so its rate counts two directed pairs per distance.
                    1 warm-up and the median of 3, scaled to the whole evaluation by pair count
Reports directed pairs/s, the agreement of the two on the sub-block, and the fraction of the fp32
VALU issue rate that the kernel's inner loop implies: VALU_PER_PAIR instructions per pair,
counted from `make asm` (csrc/build/chamfer.s, the main loop of chamfer_batch_kernel: 208 VALU
instructions per 8 second-cloud points x 4 first-cloud points; none packed, none
transcendental), each wave64 instruction taking 2 cycles of its SIMD.  Prints one JSON line;
--out also writes it to a file.

    python scripts/bench_chamfer.py [--shapes 512] [--points 2048] [--recon-points 30000]
                                    [--baseline-shapes 8] [--label TEXT]
                                    [--out profiles/chamfer/bench.json]
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
from ldm_sdf import metrics  # noqa: E402

WARM, REPS = 3, 10
VALU_PER_PAIR = 6.5      # 3 v_sub, v_mul, 2 v_fmac, half a v_min3


def timed(fn):
    e0, e1 = torch.cuda.Event(True), torch.cuda.Event(True)
    e0.record()
    r = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), r


def stats(ts):
    return {"median_ms": statistics.median(ts), "min_ms": min(ts), "max_ms": max(ts), "n": len(ts)}


def run(fn, warm=WARM, reps=REPS):
    ts = []
    for r in range(warm + reps):
        t, out = timed(fn)
        if r >= warm:
            ts.append(t)
    return stats(ts), out


def make_clouds(S, n, dev, seed):
    """Points on spheres of a radius per shape in [0.4, 0.9] with 2 % radial noise: clouds that
    look like surfaces.  The kernels' time does not depend on the coordinates."""
    g = torch.Generator(device=dev).manual_seed(seed)
    x = torch.randn(S, n, 3, device=dev, generator=g)
    x = x / x.norm(dim=-1, keepdim=True)
    rad = 0.4 + 0.5 * torch.rand(S, 1, 1, device=dev, generator=g)
    return (x * rad * (1 + 0.02 * torch.randn(S, n, 1, device=dev, generator=g))).contiguous()


def torch_chamfer(a, b):
    """CD [S, R] of a [S, n, 3], b [R, m, 3]: the chunked brute force, one first-set cloud
    against all of b per step (R n m distances and their three differences in memory)."""
    S, R = a.shape[0], b.shape[0]
    d_ab = torch.empty(S, R, device=a.device)
    d_ba = torch.empty(R, S, device=a.device)
    for s in range(S):
        diff = a[s][None, :, None, :] - b[:, None, :, :]         # [R, n, m, 3]
        d2 = (diff * diff).sum(-1)
        d_ab[s] = d2.min(2).values.double().mean(1).float()
        d_ba[:, s] = d2.min(1).values.double().mean(1).float()
    return d_ab + d_ba.t()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", type=int, default=512)
    ap.add_argument("--points", type=int, default=2048)
    ap.add_argument("--recon-points", type=int, default=30000)
    ap.add_argument("--baseline-shapes", type=int, default=8)
    ap.add_argument("--clock-mhz", type=float, default=2400.0,
                    help="engine clock the VALU issue rate is taken at (MI355X peak: 2400)")
    ap.add_argument("--label", default=None,
                    help="free text kept in the record, e.g. what a development build changed")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    S, n = args.shapes, args.points
    gen, ref = make_clouds(S, n, dev, 0), make_clouds(S, n, dev, 1)
    prop = torch.cuda.get_device_properties(0)
    issue_rate = prop.multi_processor_count * 4 * args.clock_mhz * 1e6 / 2 * 64
    res = {"metric": "chamfer: every point pair, directed pairs per second",
           "device": torch.cuda.get_device_name(0), "warmup": WARM, "reps": REPS,
           "timer": "hipEvent pair per call, median", "tile_a": metrics.tile_a(),
           "chunk_b": metrics.chunk_b(), "split_below": metrics.split_below(),
           "spread_below": metrics.spread_below(), "valu_per_pair": VALU_PER_PAIR,
           "compute_units": prop.multi_processor_count, "clock_mhz": args.clock_mhz}

    k, out = run(lambda: ldm_sdf.evaluate_generation(gen, ref, _validated=True))
    pairs = 4 * S * S * n * n
    rate = pairs / (k["median_ms"] * 1e-3)
    res["generation"] = {"shapes": S, "points": n, "directed_pairs": pairs, "kernel": k,
                         "pairs_per_s": rate, "valu_instruction_fraction":
                         rate * VALU_PER_PAIR / issue_rate,
                         "mmd": out["mmd"], "cov": out["cov"], "1nna": out["1nna"]}

    m = args.recon_points
    a1, b1 = make_clouds(1, m, dev, 2)[0], make_clouds(1, m, dev, 3)[0]
    kr, cd = run(lambda: ldm_sdf.chamfer_distance(a1, b1, _validated=True))
    rrate = 2 * m * m / (kr["median_ms"] * 1e-3)
    res["reconstruction"] = {"points": m, "directed_pairs": 2 * m * m, "kernel": kr,
                             "pairs_per_s": rrate, "chamfer_distance": float(cd)}

    nb = min(args.baseline_shapes, S)
    if nb > 0:
        b, base = run(lambda: torch_chamfer(gen[:nb], ref[:nb]), warm=1, reps=3)
        bpairs = 2 * nb * nb * n * n
        brate = bpairs / (b["median_ms"] * 1e-3)
        sub = out["cd_gr"][:nb, :nb]
        res["baseline"] = {"sub_block": f"the first {nb} generated x the first {nb} reference "
                           f"clouds of {n} points, both directions", "directed_pairs": bpairs,
                           "torch": b, "pairs_per_s": brate,
                           "ms_for_the_whole_evaluation": b["median_ms"] * pairs / bpairs,
                           "speedup_vs_torch": rate / brate,
                           "max_rel_difference": float(((sub - base).abs() / base).max())}
        if m * m <= 1 << 30:
            b1s, base1 = run(lambda: torch_chamfer(a1[None], b1[None]), warm=1, reps=3)
            res["baseline"]["reconstruction"] = {
                "torch": b1s, "pairs_per_s": 2 * m * m / (b1s["median_ms"] * 1e-3),
                "speedup_vs_torch": b1s["median_ms"] / kr["median_ms"],
                "rel_difference": float((cd - base1[0, 0]).abs() / base1[0, 0])}
    if args.label:
        res["label"] = args.label
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
