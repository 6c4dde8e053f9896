"""Sampling more than 16 latents per call: the matrix-core loop against groups of 16 through the
persistent GEMV loop.

The default network (D = 256, H = 1024, 4 blocks, bf16), T = 1000, --steps reverse steps from
t = T - 1.  Per n in --sizes, the two forms ``ldm_sdf.sample`` chooses between, each as the
sequence of loops it runs (``api.sample_groups``), inputs already in place:

    batched   groups of at most --chunk rows through ldm_sample_batch, the single C call
              captured as a graph and replayed (what Sampler does by default); also timed
              eager, and for n above the chunk as one unchunked call
    loop16    groups of <= 16 rows through ldm_sample_loop, the existing persistent loop, which
              the batched form does not touch: the baseline, measured in the same process

and, once, that persistent loop at B = 8 and B = 16 on its own.  HIP events around the whole
sequence, 3 warm-ups and the median of 10.  Reports shape-steps/s (n x steps / time), the
fraction of the dense bf16 peak at 2 x 4 718 592 flop per shape-step, and the crossover: the
smallest measured n from which "batched" is at least as fast at every larger measured n
(``api.BATCHED_FROM``).  Prints one JSON line; --out also writes it to a file.

    python scripts/bench_sample_batch.py [--sizes 17,32,64,128,256,1024,4096] [--steps 200]
                                         [--chunk 1024] [--out profiles/sample_batch/bench.json]
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
from ldm_sdf import api  # noqa: E402

WARM, REPS = 3, 10
PEAK_BF16_TFLOPS = 2516.6                 # MI355X dense bf16
MACS_PER_SHAPE_STEP = 4_718_592           # 256*1024 + 4*1024*1024 + 1024*256


def timed(fn):
    e0, e1 = torch.cuda.Event(True), torch.cuda.Event(True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def run(fn):
    ts = [timed(fn) for _ in range(WARM + REPS)][WARM:]
    return {"median_ms": statistics.median(ts), "min_ms": min(ts), "max_ms": max(ts), "n": len(ts)}


def rate(n, steps, k):
    r = n * steps / (k["median_ms"] * 1e-3)
    return {"kernel": k, "shape_steps_per_s": r,
            "bf16_peak_fraction": r * 2 * MACS_PER_SHAPE_STEP / (PEAK_BF16_TFLOPS * 1e12)}


class Loops:
    """One primed Sampler per group size; ``sequence(groups)`` is the callable that runs every
    group's loop back to back (the groups of one size share buffers: the time does not depend
    on the values)."""

    def __init__(self, model, sch, steps, dev, **kw):
        self.model, self.sch, self.steps, self.dev, self.kw = model, sch, steps, dev, kw
        self.by_size = {}

    def sampler(self, c):
        if c not in self.by_size:
            s = ldm_sdf.Sampler(self.model, self.sch, c, steps=self.steps, device=self.dev,
                                **self.kw)
            g = torch.Generator(device=self.dev).manual_seed(c)
            x_T = torch.randn(c, self.model.D, device=self.dev, generator=g)
            s.noise[self.sch.T - self.steps:].normal_(generator=g)
            s.noise[:self.sch.T - self.steps].zero_()
            s.run(x_T, s.noise[:0])           # primes (and, with use_graph, captures) the loop
            assert bool(torch.isfinite(s.result).all())
            self.by_size[c] = s
        return self.by_size[c]

    def sequence(self, groups):
        calls = []
        for lo, hi in groups:
            s = self.sampler(hi - lo)
            if s.graph is not None:
                calls.append(s.graph.replay)
            else:
                calls.append(lambda s=s: s.loop(s.x2, s.noise, self.sch.T - 1, self.steps))
        return lambda: [c() for c in calls]

    def drop(self):
        self.by_size.clear()
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="17,32,64,128,256,1024,4096")
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--chunk", type=int, default=api.SAMPLE_CHUNK)
    ap.add_argument("--label", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    sizes = sorted(int(s) for s in args.sizes.split(","))
    model, sch = ldm_sdf.MLPDenoiser(seed=4321), ldm_sdf.DDPMSchedule()
    steps = args.steps
    res = {"metric": "DDPM sampling, default MLP denoiser bf16: shape-steps per second",
           "device": torch.cuda.get_device_name(0), "warmup": WARM, "reps": REPS,
           "timer": "hipEvent pair around the whole sequence of loops, median",
           "steps": steps, "T": sch.T, "chunk": args.chunk,
           "flop_per_shape_step": 2 * MACS_PER_SHAPE_STEP, "bf16_peak_tflops": PEAK_BF16_TFLOPS,
           "batched_from_in_library": api.BATCHED_FROM, "sizes": {}}

    small = Loops(model, sch, steps, dev)                          # ldm_sample_loop, B <= 16
    res["persistent_loop"] = {f"B{b}": rate(b, steps, run(small.sequence([(0, b)])))
                              for b in (8, 16)}
    graph = Loops(model, sch, steps, dev, batched=True, use_graph=True)
    eager = Loops(model, sch, steps, dev, batched=True, use_graph=False)
    for n in sizes:
        g16 = api.sample_groups(n, "loop16")[1]
        gb = api.sample_groups(n, "batched", args.chunk)[1]
        row = {"loop16": rate(n, steps, run(small.sequence(g16))), "loop16_groups": len(g16),
               "batched": rate(n, steps, run(graph.sequence(gb))), "batched_groups": len(gb)}
        graph.drop()
        row["batched_eager"] = rate(n, steps, run(eager.sequence(gb)))
        if len(gb) > 1:
            eager.drop()
            row["batched_one_call_eager"] = rate(n, steps, run(eager.sequence([(0, n)])))
        eager.drop()
        row["batched_over_loop16"] = row["batched"]["shape_steps_per_s"] / \
            row["loop16"]["shape_steps_per_s"]
        res["sizes"][str(n)] = row
        print(f"n {n}: batched {row['batched']['shape_steps_per_s']:.3e} "
              f"(eager {row['batched_eager']['shape_steps_per_s']:.3e}) loop16 "
              f"{row['loop16']['shape_steps_per_s']:.3e} shape-steps/s "
              f"x{row['batched_over_loop16']:.2f}", file=sys.stderr, flush=True)
    wins = [res["sizes"][str(n)]["batched_over_loop16"] >= 1.0 for n in sizes]
    cross = None
    for i, n in enumerate(sizes):
        if all(wins[i:]):
            cross = n
            break
    res["crossover_n"] = cross
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
