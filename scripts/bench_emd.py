"""The earth mover's distance kernel at the sizes its users run.

    generation      ldm_sdf.evaluate_generation(metrics=("cd", "emd")) on --shapes x --shapes clouds
                    of --points points (S^2 + S (S - 1) assignment problems of 2048 x 2048 at
                    S = 512), and the same call with the Chamfer half alone; HIP events, --warm
                    warm-ups and the median of --reps (3 and 10 unless a run says otherwise)
    pair            ldm_sdf.emd_distance of two clouds of 500 points (DeepSDF's evaluation) and of
                    --points points: one workgroup, one compute unit
    rounds          auction rounds per entry of the generated x reference matrix: min / median / max,
                    against the default cap
    baseline        scipy.optimize.linear_sum_assignment on the host for the first
                    --baseline-pairs (generated, reference) pairs, cost matrix included, scaled to
                    the whole evaluation by pair count; and how far above that exact optimum the
                    kernel's entries are
Prints one JSON line; --out also writes it to a file.

    python scripts/bench_emd.py [--shapes 512] [--points 2048] [--baseline-pairs 8]
                                [--warm 3] [--reps 10] [--label TEXT]
                                [--out profiles/emd/bench.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "latent-diffusion-models-for-shape-sdfs_amd")]
import numpy as np  # noqa: E402
import torch  # noqa: E402
import ldm_sdf  # noqa: E402
from ldm_sdf import metrics  # noqa: E402
from scripts.bench_chamfer import make_clouds, run  # noqa: E402


def hungarian(a, b):
    """Exact EMD of two clouds on the host, fp64, and the seconds it took."""
    from scipy.optimize import linear_sum_assignment
    t0 = time.perf_counter()
    a, b = a.double().cpu().numpy(), b.double().cpu().numpy()
    d = np.sqrt(((a[:, None, :] - b[None, :, :]) ** 2).sum(-1))
    rows, cols = linear_sum_assignment(d)
    return float(d[rows, cols].mean()), time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", type=int, default=512)
    ap.add_argument("--points", type=int, default=2048)
    ap.add_argument("--baseline-pairs", type=int, default=8)
    ap.add_argument("--warm", type=int, default=3)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--eps", type=float, default=1e-4)
    ap.add_argument("--label", default=None,
                    help="free text kept in the record, e.g. what a development build changed")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    S, n, eps = args.shapes, args.points, args.eps
    gen, ref = make_clouds(S, n, dev, 0), make_clouds(S, n, dev, 1)
    res = {"metric": "earth mover's distance: eps-scaled auction, one workgroup per pair",
           "device": torch.cuda.get_device_name(0), "warmup": args.warm, "reps": args.reps,
           "timer": "hipEvent pair per call, median", "eps": eps,
           "max_points": metrics.emd_max_points(),
           "default_max_rounds": metrics.emd_default_max_rounds(n),
           "compute_units": torch.cuda.get_device_properties(0).multi_processor_count}

    k, out = run(lambda: ldm_sdf.evaluate_generation(gen, ref, metrics=("cd", "emd"), eps=eps,
                                                     _validated=True), args.warm, args.reps)
    kc, _ = run(lambda: ldm_sdf.evaluate_generation(gen, ref, _validated=True), args.warm,
                args.reps)
    pairs = S * S + S * (S - 1)
    emd_ms = k["median_ms"] - kc["median_ms"]
    res["generation"] = {"shapes": S, "points": n, "assignment_problems": pairs, "cd_and_emd": k,
                         "cd_only": kc, "emd_ms": emd_ms,
                         "problems_per_s": pairs / (emd_ms * 1e-3),
                         **{m: out[m] for m in ("mmd", "cov", "1nna", "mmd_emd", "cov_emd",
                                                "1nna_emd")}}

    _, rounds = ldm_sdf.emd_matrix(gen, ref, eps=eps, return_rounds=True, _validated=True)
    rounds = rounds.flatten().cpu().numpy()
    res["rounds"] = {"min": int(rounds.min()), "median": float(np.median(rounds)),
                     "max": int(rounds.max()), "per_point_median": float(np.median(rounds)) / n}

    res["pair"] = {}
    for m in sorted({500, n}):
        a1, b1 = make_clouds(1, m, dev, 2)[0], make_clouds(1, m, dev, 3)[0]
        kp, d = run(lambda: ldm_sdf.emd_distance(a1, b1, eps=eps), args.warm, args.reps)
        _, r1 = ldm_sdf.emd_matrix(a1[None], b1[None], eps=eps, return_rounds=True)
        exact, sec = hungarian(a1, b1)
        res["pair"][str(m)] = {"points": m, "kernel": kp, "emd": float(d), "rounds": int(r1),
                               "us_per_round": kp["median_ms"] * 1e3 / max(int(r1), 1),
                               "host_hungarian_ms": sec * 1e3, "above_exact": float(d) - exact}

    nb = min(args.baseline_pairs, S)
    if nb > 0:
        exact, secs = zip(*(hungarian(gen[i], ref[i]) for i in range(nb)))
        got = out["emd_gr"].diagonal()[:nb].double().cpu().numpy()
        per_pair = statistics.median(secs)
        res["baseline"] = {"what": f"linear_sum_assignment on the host, fp64, the first {nb} "
                           f"(generated, reference) pairs of {n} points, one thread",
                           "seconds_per_pair": {"median": per_pair, "min": min(secs),
                                                "max": max(secs)},
                           "s_for_the_whole_evaluation": per_pair * pairs,
                           "speedup_vs_host": per_pair * pairs / (emd_ms * 1e-3),
                           "kernel_above_exact": {"min": float((got - exact).min()),
                                                  "max": float((got - exact).max())},
                           "bound": eps + metrics.emd_slack(metrics._extent_bound(gen, ref))}
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
