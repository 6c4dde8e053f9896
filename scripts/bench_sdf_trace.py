"""``render_sdf`` against the mesh route: a picture of a decoded shape by sphere
tracing, with and without brick skipping, against ``extract_mesh`` + ``render_mesh``.

    view   a 512 x 512 view of the config-4 shape (seed-1234 decoder, latent randn(seed 0) x 0.1,
           bf16): render_sdf, render_sdf(skip_resolution=64) and extract_mesh(256) + render_mesh,
           the routes alternating in one process
    batch  64 shapes (the config-4 latent and randn(seed 1) x 0.1 rows) at 128 x 128: render_sdf
           with and without skipping against a Python loop of extract_mesh(128) + render_mesh
HIP events, 3 warm-ups and the median of 10.  Besides the times: decoder evaluations per ray,
and the share of a trace's time spent outside the decoder launches (an event pair around every
ldm_decoder_points_fwd of one instrumented march).  ``lipschitz`` is estimate_lipschitz x 1.25
of the shapes, recorded.  No speed-up is promised: what is measured is what is written.

Each GPU step runs in a child process of its own under `timeout`; a step that fails ends the
run.  Prints one JSON line; --out also writes it to a file.

    python scripts/bench_sdf_trace.py [--out profiles/sdf_trace/bench.json]
"""
import argparse
import json
import math
import os
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "latent-diffusion-models-for-shape-sdfs_amd")]

WARM, REPS = 3, 10
STEP_TIMEOUT_S = {"view": 300, "batch": 420}
EYE, FOV, LEVEL, EPS, MAX_STEPS, SKIP = (2.2, 1.6, 1.3), 50.0, 0.0, 1e-3, 256, 64


def timed(fn):
    import torch
    e0, e1 = torch.cuda.Event(True), torch.cuda.Event(True)
    e0.record()
    r = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), r


def stats(ts):
    return {"median_ms": statistics.median(ts), "min_ms": min(ts), "max_ms": max(ts), "n": len(ts)}


def setup(n_shapes):
    import torch
    import ldm_sdf
    from oracle import ref_cpu as R
    dev = torch.device("cuda", 0)
    p = R.make_decoder_params(seed=1234)
    dec = ldm_sdf.SDFDecoder(256, weights=p.weights, biases=p.biases)
    z = torch.randn(1, 256, generator=torch.Generator().manual_seed(0)) * 0.1
    if n_shapes > 1:
        more = torch.randn(n_shapes - 1, 256, generator=torch.Generator().manual_seed(1)) * 0.1
        z = torch.cat([z, more])
    z = z.to(dev)
    lip = float(ldm_sdf.estimate_lipschitz(dec, z, 32).max()) * 1.25
    pose = ldm_sdf.look_at(EYE, (0.0, 0.0, 0.0), (0.0, 0.0, 1.0))
    return dev, dec, z, lip, pose


def decoder_share(dec, z, o, d, lip, skip):
    """One instrumented march: (total ms, ms inside the decoder launches, rounds)."""
    import torch
    from ldm_sdf import ops, render
    dev = z.device
    desc = dec.device_pack("bf16", dev)["desc"]
    B = z.shape[0]
    ev = []
    e0, e1 = torch.cuda.Event(True), torch.cuda.Event(True)
    e0.record()
    beta = ops.decoder_fold(desc, z.float().contiguous())
    mask, N = None, 0
    if skip:
        N = skip
        mask = render.skip_mask(desc, beta, N, (-1.0, 1.0), LEVEL, lip, EPS)
    st = ops.SdfTraceState(o, d, B, (-1.0, 1.0), LEVEL, lip, EPS, mask, N, False)
    ops.sdf_trace_init(st, 0.0, math.inf, MAX_STEPS)
    for _ in range(MAX_STEPS):
        P = max(st.counts.tolist())
        if P == 0:
            break
        xyz = ops.sdf_trace_emit(st, P)
        a, b = torch.cuda.Event(True), torch.cuda.Event(True)
        a.record()
        vals = ops.decoder_points_fwd(desc, beta, xyz)
        b.record()
        ev.append((a, b))
        ops.sdf_trace_step(st, vals)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), sum(a.elapsed_time(b) for a, b in ev), len(ev)


def run_routes(routes):
    """The routes alternating: {name: stats} after WARM + REPS passes over all of them."""
    ts = {k: [] for k in routes}
    for r in range(WARM + REPS):
        for k, fn in routes.items():
            t, _ = timed(fn)
            if r >= WARM:
                ts[k].append(t)
    return {k: stats(v) for k, v in ts.items()}


def step(args, n_shapes, size, grid):
    import torch
    import ldm_sdf
    dev, dec, z, lip, pose = setup(n_shapes)
    kw = dict(level=LEVEL, lipschitz=lip, eps=EPS, max_steps=MAX_STEPS, dtype="bf16")

    def mesh_route():
        out = []
        for v, f in ldm_sdf.extract_mesh(dec, z, grid, dtype="bf16", level=LEVEL, lipschitz=lip):
            out.append(ldm_sdf.render_mesh(v, f, pose, FOV, size, size)["image"])
        return out
    routes = {"render_sdf": lambda: ldm_sdf.render_sdf(dec, z, pose, FOV, size, size, **kw),
              "render_sdf_skip": lambda: ldm_sdf.render_sdf(dec, z, pose, FOV, size, size,
                                                            skip_resolution=SKIP, **kw),
              "mesh_route": mesh_route}
    res = {"shapes": n_shapes, "image": size, "mesh_grid": grid, "lipschitz": lip,
           "device": torch.cuda.get_device_name(0), "warmup": WARM, "reps": REPS,
           "timer": "hipEvent pair per call, median; routes alternate in one process"}
    res.update(run_routes(routes))
    o, d = ldm_sdf.camera_rays(pose, FOV, size, size, device=dev)
    for name, skip in (("trace", None), ("trace_skip", SKIP)):
        t, st, steps = ldm_sdf.trace_sdf(dec, z, o, d, skip_resolution=skip, **kw)
        total, inside, rounds = decoder_share(dec, z, o, d, lip, skip)
        res[name] = {"evaluations_per_ray": float(steps.sum()) / steps.numel(),
                     "hit_fraction": float((st == 1).float().mean()),
                     "exhausted_fraction": float((st == 2).float().mean()), "rounds": rounds,
                     "march_ms": total, "decoder_ms": inside,
                     "share_outside_decoder": 1.0 - inside / total}
    res["faces"] = [int(f.shape[0]) for _, f in
                    ldm_sdf.extract_mesh(dec, z[:4], grid, dtype="bf16", lipschitz=lip)]
    res["render_sdf_over_mesh_route"] = res["render_sdf"]["median_ms"] / \
        res["mesh_route"]["median_ms"]
    res["render_sdf_skip_over_mesh_route"] = res["render_sdf_skip"]["median_ms"] / \
        res["mesh_route"]["median_ms"]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--step", default=None, choices=sorted(STEP_TIMEOUT_S),
                    help="(internal) run one GPU step in this process and print its record")
    args = ap.parse_args()
    if args.step:
        rec = step(args, 1, 512, 256) if args.step == "view" else step(args, 64, 128, 128)
        print(json.dumps(rec))
        return 0
    res = {"metric": "render_sdf against extract_mesh + render_mesh"}
    for name in ("view", "batch"):
        with tempfile.TemporaryFile("w+") as out:
            cmd = ["timeout", "-k", "10", str(STEP_TIMEOUT_S[name]), sys.executable,
                   os.path.abspath(__file__), "--step", name]
            rc = subprocess.run(cmd, stdout=out).returncode
            if rc != 0:
                print(f"bench_sdf_trace: step {name} ended with status {rc}; stopping",
                      file=sys.stderr)
                return rc
            out.seek(0)
            res[name] = json.loads(out.read().strip().splitlines()[-1])
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
