"""``mesh_sdf`` at DeepSDF's working size: the 500 000 ``sample_sdf`` points of
one shape against the marching-cubes mesh of a 256^3 volume (~10^5 faces), every pair evaluated.

    kernel    ldm_sdf.mesh_sdf on all points, in sample_sdf's point chunks; HIP events, 3
              warm-ups and the median of 10
    baseline  the same formulas as a chunked torch brute force on the same GPU, written here,
              on the first --baseline-points points (it is far too slow for all of them; its
              rate in pairs/s is what is compared), 1 warm-up and the median of 3
Reports pairs/s, the agreement of the two, and the fraction of the fp32 VALU issue rate that the
kernel's inner loop implies: VALU_PER_PAIR instructions per pair, counted from `make asm`
(csrc/build/mesh_sdf.s, the loop of mesh_eval_kernel<false>), each wave64
instruction taking 2 cycles of its SIMD; ISSUE_SLOTS_PER_PAIR counts the packed fp32 and the
transcendental instructions twice.  Prints one JSON line; --out also writes it to a file.

    python scripts/bench_mesh_sdf.py [--shape torus|sphere|decoded] [--points 500000]
                                     [--point-chunk N] [--baseline-points N] [--label TEXT]
                                     [--out profiles/mesh_sdf/bench.json]
"""
import argparse
import json
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "latent-diffusion-models-for-shape-sdfs_amd")]
import torch  # noqa: E402
import ldm_sdf  # noqa: E402
from ldm_sdf import meshsdf  # noqa: E402

WARM, REPS = 3, 10
# inner loop of the eval kernel, per point-triangle pair: 156 VALU instructions, 30 of them
# packed fp32 (v_pk_fma / mul / add_f32: two plain instructions' worth of issue) and 5 v_rcp /
# v_sqrt (which hold the issue port twice as long)
VALU_PER_PAIR = 156
ISSUE_SLOTS_PER_PAIR = 156 + 30 + 5


def timed(fn):
    e0, e1 = torch.cuda.Event(True), torch.cuda.Event(True)
    e0.record()
    r = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), r


def stats(ts):
    return {"median_ms": statistics.median(ts), "min_ms": min(ts), "max_ms": max(ts), "n": len(ts)}


def shape_volume(kind, N, dev):
    c = torch.linspace(-1.0, 1.0, N, device=dev)
    z, y, x = torch.meshgrid(c, c, c, indexing="ij")
    if kind == "torus":
        return (((x * x + y * y).sqrt() - 0.5) ** 2 + z * z).sqrt() - 0.2
    if kind == "sphere":
        return (x * x + y * y + z * z).sqrt() - 0.55
    dec = ldm_sdf.SDFDecoder(256, seed=1234)
    lat = (torch.randn(1, 256, generator=torch.Generator().manual_seed(0)) * 0.1).to(dev)
    return ldm_sdf.decode(dec, lat, N, dtype="bf16")[0]


def _dot(a, b):
    return (a * b).sum(-1)


def _sdiv(n, d):
    ok = d != 0
    return torch.where(ok, n / torch.where(ok, d, torch.ones_like(d)), torch.zeros_like(n))


def torch_pairs(p, a, b, c):
    """(d^2, half solid angle) [Pc, F] of the definitions in DESIGN.md §16, fp32, in torch."""
    ab, ac = b - a, c - a
    ap, bp, cp = p - a, p - b, p - c
    d1, d2, d3 = _dot(ab, ap), _dot(ac, ap), _dot(ab, bp)
    d4, d5, d6 = _dot(ac, bp), _dot(ab, cp), _dot(ac, cp)
    vc, vb, va = d1 * d4 - d3 * d2, d5 * d2 - d1 * d6, d3 * d6 - d5 * d4
    one, zero = torch.ones_like(d1), torch.zeros_like(d1)
    nv, nw, den = vb, vc, va + vb + vc
    bc = (va <= 0) & (d4 - d3 >= 0) & (d5 - d6 >= 0)
    nw, den = torch.where(bc, d4 - d3, nw), torch.where(bc, (d4 - d3) + (d5 - d6), den)
    for m, mv, mw, md in (((vb <= 0) & (d2 >= 0) & (d6 <= 0), zero, d2, d2 - d6),
                          ((d6 >= 0) & (d5 <= d6), zero, one, one),
                          ((vc <= 0) & (d1 >= 0) & (d3 <= 0), d1, zero, d1 - d3),
                          ((d3 >= 0) & (d4 <= d3), one, zero, one),
                          ((d1 <= 0) & (d2 <= 0), zero, zero, one)):
        nv, nw, den = torch.where(m, mv, nv), torch.where(m, mw, nw), torch.where(m, md, den)
        bc = bc & ~m
    v, w = _sdiv(nv, den), _sdiv(nw, den)
    v = torch.where(bc, 1 - w, v)
    q = ap - v[..., None] * ab - w[..., None] * ac
    det = -_dot(ap, torch.linalg.cross(bp, cp))
    la, lb, lc = ap.norm(dim=-1), bp.norm(dim=-1), cp.norm(dim=-1)
    dn = la * lb * lc + _dot(ap, bp) * lc + _dot(bp, cp) * la + _dot(cp, ap) * lb
    return _dot(q, q), torch.where(det == 0, zero, torch.atan2(det, dn))


def torch_mesh_sdf(verts, faces, points, pair_budget=1 << 22):
    """The chunked brute force: ``pair_budget`` pairs per step bound its temporaries."""
    f = faces.long()
    a, b, c = verts[f[:, 0]][None], verts[f[:, 1]][None], verts[f[:, 2]][None]
    step = max(1, pair_budget // max(1, faces.shape[0]))
    out = []
    for s in range(0, points.shape[0], step):
        d2, h = torch_pairs(points[s:s + step, None, :], a, b, c)
        w = h.sum(1) / (2 * math.pi)
        d = d2.min(1).values.sqrt()
        out.append(torch.where(w > 0.5, -d, d))
    return torch.cat(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="torus", choices=["torus", "sphere", "decoded"])
    ap.add_argument("--grid", type=int, default=256)
    ap.add_argument("--points", type=int, default=500_000)
    ap.add_argument("--baseline-points", type=int, default=8192)
    ap.add_argument("--clock-mhz", type=float, default=2400.0,
                    help="engine clock the VALU issue rate is taken at (MI355X peak: 2400)")
    ap.add_argument("--point-chunk", type=int, default=meshsdf.POINT_CHUNK,
                    help="points per mesh_sdf call (default: sample_sdf's own)")
    ap.add_argument("--label", default=None,
                    help="free text kept in the record, e.g. what a development build changed")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    v, f = ldm_sdf.marching_cubes(shape_volume(args.shape, args.grid, dev).contiguous())
    v, _, _ = ldm_sdf.normalize_mesh(v)
    v = v.contiguous()
    g = torch.Generator(device=dev).manual_seed(0)
    pos, neg = ldm_sdf.sample_sdf(v, f, args.points, generator=g)
    pts = torch.cat([pos, neg])[:, :3].contiguous()
    pts = pts[torch.randperm(pts.shape[0], device=dev, generator=g)].contiguous()
    P, F = pts.shape[0], f.shape[0]

    def kernel():
        return torch.cat([ldm_sdf.mesh_sdf(v, f, pts[s:s + args.point_chunk], _validated=True)
                          for s in range(0, P, args.point_chunk)])

    ts = []
    for r in range(WARM + REPS):
        t, sdf = timed(kernel)
        if r >= WARM:
            ts.append(t)
    k = stats(ts)
    pairs = P * F
    rate = pairs / (k["median_ms"] * 1e-3)
    prop = torch.cuda.get_device_properties(0)
    clock_hz = args.clock_mhz * 1e6
    simds = prop.multi_processor_count * 4
    issue_rate = simds * clock_hz / 2 * 64            # lane-instructions per second
    res = {"metric": "mesh_sdf: every point-triangle pair of one shape's sample_sdf points",
           "device": torch.cuda.get_device_name(0), "shape": args.shape, "grid": args.grid,
           "faces": F, "vertices": int(v.shape[0]), "points": P, "pairs": pairs,
           "point_chunk": args.point_chunk, "face_chunk": meshsdf.face_chunk(),
           "warmup": WARM, "reps": REPS, "timer": "hipEvent pair per call, median",
           "kernel": k, "kernel_pairs_per_s": rate,
           "valu_per_pair": VALU_PER_PAIR, "issue_slots_per_pair": ISSUE_SLOTS_PER_PAIR,
           "compute_units": prop.multi_processor_count, "clock_mhz": args.clock_mhz,
           "valu_instruction_fraction": rate * VALU_PER_PAIR / issue_rate,
           "valu_issue_fraction": rate * ISSUE_SLOTS_PER_PAIR / issue_rate,
           "inside_fraction": float((sdf < 0).float().mean())}
    nb = min(args.baseline_points, P)
    if nb > 0:
        bts = []
        for r in range(1 + 3):
            t, bsdf = timed(lambda: torch_mesh_sdf(v, f, pts[:nb]))
            if r >= 1:
                bts.append(t)
        b = stats(bts)
        brate = nb * F / (b["median_ms"] * 1e-3)
        diff = (bsdf.abs() - sdf[:nb].abs()).abs()
        res.update({"baseline": b, "baseline_points": nb, "baseline_pairs_per_s": brate,
                    "baseline_ms_for_all_points": b["median_ms"] * P / nb,
                    "speedup_vs_torch": rate / brate,
                    "max_abs_distance_difference": float(diff.max()),
                    "sign_mismatches": int(((bsdf < 0) != (sdf[:nb] < 0)).sum())})
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
