"""``ray_mesh`` at rendering size: a 512 x 512 image of the marching-cubes mesh of
the 256^3 torus that scripts/bench_mesh_sdf.py uses (~1.8 10^5 faces), every ray-triangle pair
evaluated.

    kernel    the ldm_ray_mesh call (pack + trace; ops.ray_mesh, outputs t, face and bary) on all
              rays of the image; HIP events, 3 warm-ups and the median of 10
    baseline  the same watertight test as a chunked torch brute force on the same GPU, written
              here, on --baseline-rays rays from the middle of the image, where the mesh is (its
              rate in pairs/s is what is compared), 1 warm-up and the median of 3
Reports ms, pairs/s, the agreement of the two, and the fraction of the fp32 VALU issue rate that
the kernel's inner loop implies: VALU_PER_PAIR instructions per pair, counted from `make asm`
(csrc/build/ray_mesh.s, the loop of ray_trace_kernel<true> without the hit branch; DESIGN.md
§19), each wave64 instruction taking 2 cycles of its SIMD; ISSUE_SLOTS_PER_PAIR would count
packed fp32 and transcendental instructions twice, as §16 prices them -- that path has none.

Each GPU step runs in a child process of its own under `timeout`; a step that fails ends the
run.  Prints one JSON line; --out also writes it to a file.

    python scripts/bench_ray_mesh.py [--size 512] [--grid 256] [--baseline-rays 4096]
                                     [--label TEXT] [--out profiles/ray_mesh/bench.json]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "latent-diffusion-models-for-shape-sdfs_amd")]

WARM, REPS = 3, 10
STEP_TIMEOUT_S = {"kernel": 240, "baseline": 240}
# the loop of the trace kernel, per ray-triangle pair of a wave in which no lane hits: 59 VALU
# instructions (9 v_sub for q, 18 v_cndmask for the axis permutation, 6 + 6 for the shear, 6 + 3
# for the edge functions, 11 for the sign tests and det), none packed, none transcendental; the
# 30 of the hit branch (one v_rcp_f32 among them) run only when some lane is inside the triangle
VALU_PER_PAIR = 59
ISSUE_SLOTS_PER_PAIR = 59


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


def scene(args):
    """The mesh and the rays, remade identically by every step."""
    import torch
    import ldm_sdf
    dev = torch.device("cuda", 0)
    c = torch.linspace(-1.0, 1.0, args.grid, device=dev)
    z, y, x = torch.meshgrid(c, c, c, indexing="ij")
    vol = (((x * x + y * y).sqrt() - 0.5) ** 2 + z * z).sqrt() - 0.2
    v, f = ldm_sdf.marching_cubes(vol.contiguous())
    v, _, _ = ldm_sdf.normalize_mesh(v)
    pose = ldm_sdf.look_at((1.6, 1.2, 1.8), (0.0, 0.0, 0.0))
    o, d = ldm_sdf.camera_rays(pose, 40.0, args.size, args.size, device=dev)
    return v.contiguous(), f.contiguous(), o, d


def _sel(x, k):
    return x.gather(-1, k[..., None])[..., 0]


def torch_ray_mesh(verts, faces, o, d, pair_budget=1 << 22):
    """The watertight test of csrc/ray_tri_pair.h as chunked torch fp32: ``(t, face)``."""
    import torch
    fl = faces.long()
    tri = [verts[fl[:, k]] for k in range(3)]                       # [F, 3] each
    F = faces.shape[0]
    step = max(1, pair_budget // max(1, F))
    ts, fs = [], []
    inf = torch.tensor(float("inf"), device=o.device)
    for s in range(0, o.shape[0], step):
        oo, dd = o[s:s + step], d[s:s + step]
        kz = dd.abs().argmax(1)
        kx, ky = (kz + 1) % 3, (kz + 2) % 3
        dk = _sel(dd, kz)
        neg = dk < 0
        kx, ky = torch.where(neg, ky, kx), torch.where(neg, kx, ky)
        Sx, Sy, Sz = _sel(dd, kx) / dk, _sel(dd, ky) / dk, 1.0 / dk
        sh = []
        for p in tri:
            q = p[None] - oo[:, None]                                # [R, F, 3]
            n = q.shape[:2]
            k = _sel(q, kz[:, None].expand(n))
            sh.append((_sel(q, kx[:, None].expand(n)) - Sx[:, None] * k,
                       _sel(q, ky[:, None].expand(n)) - Sy[:, None] * k, k))
        (Ax, Ay, Ak), (Bx, By, Bk), (Cx, Cy, Ck) = sh
        U, V, W = Cx * By - Cy * Bx, Ax * Cy - Ay * Cx, Bx * Ay - By * Ax
        mixed = ((U < 0) | (V < 0) | (W < 0)) & ((U > 0) | (V > 0) | (W > 0))
        det = (U + V) + W
        Sz = Sz[:, None]
        t = ((U * (Sz * Ak) + V * (Sz * Bk)) + W * (Sz * Ck)) / det
        hit = ~mixed & (det != 0) & (t >= 0)
        t = torch.where(hit, t, inf)
        tt, ff = t.min(1)
        ts.append(tt)
        fs.append(torch.where(torch.isfinite(tt), ff, torch.full_like(ff, -1)))
    return torch.cat(ts), torch.cat(fs)


def step_kernel(args):
    import torch
    from ldm_sdf import ops, render
    v, f, o, d = scene(args)
    ts = []
    for r in range(WARM + REPS):
        t, (tt, face, bary, flag) = timed(lambda: ops.ray_mesh(v, f, o, d, 0.0, float("inf"),
                                                               True))
        if r >= WARM:
            ts.append(t)
    k = stats(ts)
    R, F = o.shape[0], f.shape[0]
    rate = R * F / (k["median_ms"] * 1e-3)
    prop = torch.cuda.get_device_properties(0)
    issue_rate = prop.multi_processor_count * 4 * args.clock_mhz * 1e6 / 2 * 64
    return {"device": torch.cuda.get_device_name(0), "faces": F, "vertices": int(v.shape[0]),
            "rays": R, "pairs": R * F, "face_chunk": render.face_chunk(),
            "split_below": render.split_below(),
            "form": "split" if R < render.split_below() and F > render.face_chunk()
            else "one pass",
            "warmup": WARM, "reps": REPS, "timer": "hipEvent pair per call, median",
            "kernel": k, "kernel_pairs_per_s": rate, "valu_per_pair": VALU_PER_PAIR,
            "issue_slots_per_pair": ISSUE_SLOTS_PER_PAIR,
            "compute_units": prop.multi_processor_count, "clock_mhz": args.clock_mhz,
            "valu_instruction_fraction": rate * VALU_PER_PAIR / issue_rate,
            "valu_issue_fraction": rate * ISSUE_SLOTS_PER_PAIR / issue_rate,
            "hit_fraction": float((face >= 0).float().mean()), "flag": int(flag.item())}


def step_baseline(args):
    from ldm_sdf import ops
    v, f, o, d = scene(args)
    nb = min(args.baseline_rays, o.shape[0])
    # rows from the middle of the image, where the mesh is
    s = (o.shape[0] - nb) // 2
    o, d = o[s:s + nb].contiguous(), d[s:s + nb].contiguous()
    bts = []
    for r in range(1 + 3):
        t, (bt, bf) = timed(lambda: torch_ray_mesh(v, f, o, d))
        if r >= 1:
            bts.append(t)
    b = stats(bts)
    kt, kf, _, _ = ops.ray_mesh(v, f, o, d, 0.0, float("inf"), False)
    both = (kf >= 0) & (bf >= 0)
    return {"baseline": b, "baseline_rays": nb,
            "baseline_pairs_per_s": nb * f.shape[0] / (b["median_ms"] * 1e-3),
            "baseline_hit_fraction": float((bf >= 0).float().mean()),
            "mask_mismatches": int(((kf >= 0) != (bf >= 0)).sum()),
            "face_mismatches": int((kf != bf.int()).sum()),
            "max_abs_t_difference": float((kt[both] - bt[both]).abs().max()) if both.any()
            else 0.0}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=512, help="image height and width")
    ap.add_argument("--grid", type=int, default=256)
    ap.add_argument("--baseline-rays", type=int, default=4096)
    ap.add_argument("--clock-mhz", type=float, default=2400.0,
                    help="engine clock the VALU issue rate is taken at (MI355X peak: 2400)")
    ap.add_argument("--label", default=None,
                    help="free text kept in the record, e.g. what a development build changed")
    ap.add_argument("--out", default=None)
    ap.add_argument("--step", default=None, choices=sorted(STEP_TIMEOUT_S),
                    help="(internal) run one GPU step in this process and print its record")
    args = ap.parse_args()
    if args.step:
        print(json.dumps({"kernel": step_kernel, "baseline": step_baseline}[args.step](args)))
        return 0
    res = {"metric": "ray_mesh: every ray-triangle pair of one image", "image": args.size,
           "grid": args.grid, "shape": "torus"}
    steps = ["kernel"] + (["baseline"] if args.baseline_rays > 0 else [])
    for step in steps:
        with tempfile.TemporaryFile("w+") as out:
            cmd = ["timeout", "-k", "10", str(STEP_TIMEOUT_S[step]), sys.executable,
                   os.path.abspath(__file__), "--step", step, "--size", str(args.size), "--grid",
                   str(args.grid), "--baseline-rays", str(args.baseline_rays), "--clock-mhz",
                   str(args.clock_mhz)]
            rc = subprocess.run(cmd, stdout=out).returncode
            if rc != 0:
                print(f"bench_ray_mesh: step {step} ended with status {rc}; stopping",
                      file=sys.stderr)
                return rc
            out.seek(0)
            res.update(json.loads(out.read().strip().splitlines()[-1]))
    if "baseline_pairs_per_s" in res:
        res["speedup_vs_torch"] = res["kernel_pairs_per_s"] / res["baseline_pairs_per_s"]
        res["baseline_ms_for_all_rays"] = (res["baseline"]["median_ms"] * res["rays"] /
                                           res["baseline_rays"])
    if args.label:
        res["label"] = args.label
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
