"""Meshes -> DeepSDF training samples on the GPU: what DeepSDF's
``preprocess_data.py`` + ``PreprocessMesh`` do, for a folder of meshes and a split JSON.

For every ``{dataset: {class: [instance, ...]}}`` entry of the split the mesh is looked up as
``<mesh_dir>/<class>/<instance>/models/model_normalized.obj`` (the ShapeNet layout) or
``<mesh_dir>/<class>/<instance>.{obj,ply}``, normalised (bounding-box centre to the origin,
farthest vertex to radius 1 / 1.03), sampled with ``ldm_sdf.sample_sdf`` and written as

    <out>/SdfSamples/<dataset>/<class>/<instance>.npz                pos, neg: [n, 4] float32
    <out>/NormalizationParameters/<dataset>/<class>/<instance>.npz   offset [3], scale

the layout ``SdfSampleSet.from_split(<out>, split)`` reads.  An existing output is kept unless
--overwrite.  Prints one JSON line per shape and a summary line.

    python scripts/preprocess_meshes.py MESH_DIR SPLIT.json OUT [--points 500000] [--seed 0]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "latent-diffusion-models-for-shape-sdfs_amd")]
import numpy as np  # noqa: E402
import torch  # noqa: E402
import ldm_sdf  # noqa: E402


def find_mesh(mesh_dir, cls, inst):
    for rel in (os.path.join(cls, inst, "models", "model_normalized.obj"),
                os.path.join(cls, inst + ".obj"), os.path.join(cls, inst + ".ply"),
                os.path.join(cls, inst, "model.obj"), os.path.join(cls, inst, "model.ply")):
        p = os.path.join(mesh_dir, rel)
        if os.path.isfile(p):
            return p
    return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mesh_dir")
    ap.add_argument("split")
    ap.add_argument("out")
    ap.add_argument("--points", type=int, default=500_000)
    ap.add_argument("--buffer", type=float, default=1.03)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--overwrite", action="store_true")
    args = ap.parse_args()
    with open(args.split) as fh:
        split = json.load(fh)
    dev = torch.device("cuda", 0)
    ldm_sdf.load_library()
    done = skipped = missing = 0
    k = 0
    for ds, classes in split.items():
        for cls, insts in classes.items():
            for inst in insts:
                k += 1
                dst = os.path.join(args.out, "SdfSamples", ds, cls, inst + ".npz")
                if os.path.exists(dst) and not args.overwrite:
                    skipped += 1
                    continue
                src = find_mesh(args.mesh_dir, cls, inst)
                if src is None:
                    missing += 1
                    print(json.dumps({"instance": f"{ds}/{cls}/{inst}", "error": "no mesh file"}))
                    continue
                t0 = time.time()
                read = ldm_sdf.read_ply if src.endswith(".ply") else ldm_sdf.read_obj
                v, f = read(src)
                if len(f) == 0:
                    missing += 1
                    print(json.dumps({"instance": f"{ds}/{cls}/{inst}", "error": "no faces"}))
                    continue
                vn, offset, scale = ldm_sdf.normalize_mesh(torch.from_numpy(v), args.buffer)
                g = torch.Generator(device=dev).manual_seed(args.seed + k)
                pos, neg = ldm_sdf.sample_sdf(vn.to(dev).contiguous(), torch.from_numpy(f).to(dev),
                                              args.points, generator=g)
                ldm_sdf.data.save_sdf_samples(dst, pos, neg)
                npath = os.path.join(args.out, "NormalizationParameters", ds, cls, inst + ".npz")
                os.makedirs(os.path.dirname(npath), exist_ok=True)
                with open(npath, "wb") as fh:
                    np.savez(fh, offset=offset.numpy(), scale=np.float32(scale))
                done += 1
                print(json.dumps({"instance": f"{ds}/{cls}/{inst}", "mesh": src,
                                  "faces": int(len(f)), "pos": int(pos.shape[0]),
                                  "neg": int(neg.shape[0]), "seconds": time.time() - t0}))
    print(json.dumps({"written": done, "kept": skipped, "failed": missing}))
    return 1 if missing else 0


if __name__ == "__main__":
    sys.exit(main())
