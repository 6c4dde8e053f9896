"""Narrow-band decode against the dense decode, one shape to a mesh.

Config-4 inputs (decoder seed 1234, latent randn(seed 0) x 0.1, bf16), one shape, at each
resolution in --grids.  In ONE process, alternating per repetition:
    dense   decode + marching_cubes
    band    decode_band + marching_cubes, at each --lipschitz setting
HIP events around each, 3 warm-ups and the median of 10 (the §8(d) form).  Then per setting the
stages on their own (coarse = lattice coordinates + points decode, classify, fill, bricks), the
per-tile time of the decoder's brick mode against its grid mode in the same run (a tile is 128
points in both), the same with every brick active, and whether the two meshes are equal.
Prints one JSON line; --out also writes it to a file.

    python scripts/bench_band.py [--grids 256 512] [--lipschitz 1.0 0.5] [--out FILE]
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
    """fns: name -> callable; WARM + REPS rounds, each running every callable once."""
    ts = {k: [] for k in fns}
    last = {}
    for r in range(WARM + REPS):
        for k, fn in fns.items():
            t, last[k] = timed(fn)
            if r >= WARM:
                ts[k].append(t)
    return {k: stats(v) for k, v in ts.items()}, last


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grids", type=int, nargs="+", default=[256, 512])
    ap.add_argument("--lipschitz", type=float, nargs="+", default=[1.0, 0.5])
    ap.add_argument("--dtype", default="bf16")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    dec = ldm_sdf.SDFDecoder(256, seed=1234)
    z = (torch.randn(1, 256, generator=torch.Generator().manual_seed(0)) * 0.1).to(dev)
    desc = dec.device_pack(args.dtype, dev)["desc"]
    beta = ops.decoder_fold(desc, z)
    res = {"metric": "one shape to a mesh: dense decode + marching cubes vs narrow-band decode "
                     "+ marching cubes", "dtype": args.dtype, "warmup": WARM, "reps": REPS,
           "timer": "hipEvent pair per call, median", "device": torch.cuda.get_device_name(0),
           "grids": {}}
    for N in args.grids:
        nb = ldm_sdf.n_bricks(N)
        vol = torch.empty(1, N, N, N, device=dev)
        bvol = torch.empty(1, N, N, N, device=dev)

        def dense():
            ldm_sdf.decode(dec, z, N, dtype=args.dtype, out=vol)
            return ldm_sdf.marching_cubes(vol[0])

        def band(lip):
            def run():
                ldm_sdf.decode_band(dec, z, N, dtype=args.dtype, lipschitz=lip, out=bvol)
                return ldm_sdf.marching_cubes(bvol[0])
            return run

        fns = {"dense": dense}
        for lip in args.lipschitz:
            fns[f"band_L{lip:g}"] = band(lip)
        e2e, last = alternate(fns)
        g = {"N": N, "bricks": nb ** 3, "dense_tiles": N ** 3 // 128 + (N ** 3 % 128 > 0),
             "end_to_end": e2e, "settings": {}}

        # the decoder alone in grid mode, same run: the per-tile yardstick
        grid_t, _ = alternate({"grid": lambda: ops.decoder_grid_fwd(desc, beta, N, 0, N, out=vol)})
        g["grid_decode"] = grid_t["grid"]
        grid_tile_us = grid_t["grid"]["median_ms"] * 1e3 / g["dense_tiles"]
        g["grid_us_per_tile"] = grid_tile_us
        v0, f0 = last["dense"]

        for lip in list(args.lipschitz) + [math.inf]:
            vs = ops.voxel_size(N)
            bw = math.inf if lip == math.inf else lip * 4.0 * math.sqrt(3.0) * vs
            xyz = ops.band_lattice_coords(N, device=dev)[None].contiguous()
            coarse = ops.decoder_points_fwd(desc, beta, xyz)
            active, bricks, count = ops.band_classify(coarse, N, 0.0, bw)
            n_act = int(count.item())
            st, _ = alternate({
                "coarse": lambda: ops.decoder_points_fwd(
                    desc, beta, ops.band_lattice_coords(N, device=dev)[None].contiguous()),
                "classify": lambda: ops.band_classify(coarse, N, 0.0, bw),
                "fill": lambda: ops.band_fill(coarse, active, N, bvol),
                "bricks": lambda: ops.decoder_bricks_fwd(desc, beta, N, bricks, count, bvol),
            })
            tiles = 4 * n_act
            us_tile = st["bricks"]["median_ms"] * 1e3 / max(tiles, 1)
            s = {"band": bw if math.isfinite(bw) else "inf", "active_bricks": n_act,
                 "active_fraction": n_act / nb ** 3, "stages": st, "brick_tiles": tiles,
                 "coarse_tiles": -(-(nb + 1) ** 3 // 128),
                 "bricks_us_per_tile": us_tile, "bricks_over_grid_per_tile": us_tile / grid_tile_us,
                 "predicted_ms": (-(-(nb + 1) ** 3 // 128) + tiles) * grid_tile_us * 1e-3}
            if lip != math.inf:
                key = f"band_L{lip:g}"
                v1, f1 = last[key]
                s["mesh_equal"] = bool(v1.shape == v0.shape and f1.shape == f0.shape and
                                       torch.equal(v1, v0) and torch.equal(f1, f0))
                s["faces"] = int(f1.shape[0])
                s["end_to_end_ms"] = e2e[key]["median_ms"]
                s["speedup_vs_dense"] = e2e["dense"]["median_ms"] / e2e[key]["median_ms"]
            else:
                ops.band_fill(coarse, active, N, bvol)
                ops.decoder_bricks_fwd(desc, beta, N, bricks, count, bvol)
                s["volume_equal_dense"] = bool(torch.equal(bvol, vol))
            g["settings"]["all_active" if lip == math.inf else f"lipschitz_{lip:g}"] = s
        g["dense_faces"] = int(f0.shape[0])
        res["grids"][str(N)] = g
        del vol, bvol
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
