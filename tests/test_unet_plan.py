"""The 1D-UNet's single launch plan on the host (ldm_sdf/unet.py; no GPU):

* ``step_cost`` keeps the numbers the hand-written conv list gave;
* the 18 ``ConvArgs`` that ``step_args`` builds -- every scalar field, every pointer as
  (tensor name, byte offset) -- equal tests/golden/unet_launch_table.json, recorded with
  ``launch_table`` below from the commit before the plan existed;
* the backward schedule the trainer binds: order, write-before-accumulate, counts.
"""
import ctypes
import json
import os

import pytest
import torch

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "unet_launch_table.json")
TINY = dict(D=72, C=(8, 24, 40), TE=16, HT=32, T=50)      # ragged channel tails
T_STEP = 7
CASES = {"default_n1": ({}, 1, False), "default_n2": ({}, 2, False),
         "default_n1_ddpm": ({}, 1, True), "default_n2_ddpm": ({}, 2, True),
         "ragged_n1": (TINY, 1, False)}


def launch_table(model, n, ddpm=False):
    """``step_args`` on host tensors, as JSON-able data: per call every int field, the segments in
    use, and every pointer as [name, byte offset] into the tensor that holds it (the largest, by
    name on a tie: a view resolves to its base, an alias to its first name) or None."""
    from ldm_sdf import DDPMSchedule, ops
    from ldm_sdf.unet import is_conv_weight
    dev = {k: ops.pack_conv_weight(v) if is_conv_weight(k) else v for k, v in model.params.items()}
    for i in range(6):
        dev[f"etab{i}"] = torch.zeros(model.T, dev[f"res{i}.b1"].numel())
    buf = model.buffers(n, "cpu")
    named = {**dev, **buf, "x": torch.zeros(n, model.D), "out": torch.zeros(n, model.D)}
    kw = {}
    if ddpm:
        sd = DDPMSchedule(model.T).device("cpu")
        named.update({f"sched.{k}": v for k, v in sd.items() if isinstance(v, torch.Tensor)})
        named["z"] = torch.zeros(n, model.D)
        kw = dict(sched=sd["desc"], z=named["z"])

    def where(p):
        if not p:
            return None
        hits = [(-v.numel() * v.element_size(), k, p - v.data_ptr()) for k, v in named.items()
                if v.data_ptr() <= p < v.data_ptr() + v.numel() * v.element_size()]
        _, name, off = min(hits)
        return [name, off]

    def dump(st, n_seg):
        d = {}
        for name, ty in st._fields_:
            v = getattr(st, name)
            if ty is ctypes.c_void_p:
                d[name] = where(v)
            elif isinstance(v, ctypes.Array):
                d[name] = [dump(v[i], 0) for i in range(n_seg)]
            else:
                d[name] = int(v)
        return d

    calls = model.step_args(dev, buf, named["x"], T_STEP, out=named["out"], **kw)
    return [dump(a, a.n_seg) for a in calls]


def test_step_cost_numbers():
    from ldm_sdf import UNet1DDenoiser
    m = UNet1DDenoiser()
    assert m.step_cost(1) == dict(flops=264634368, bytes=6728064, weight_bytes=690560,
                                  activation_bytes=6037504, launches=18)
    for n, fl, by, ab in ((8, 2117074944, 48990592, 48300032),
                          (64, 16936599552, 387090816, 386400256)):
        c = m.step_cost(n)
        assert (c["flops"], c["bytes"], c["activation_bytes"]) == (fl, by, ab)
    c = m.step_cost(8, weight_bytes=4)
    assert (c["bytes"], c["weight_bytes"]) == (49681152, 1381120)
    assert UNet1DDenoiser(**TINY).step_cost(3) == dict(
        flops=5985792, bytes=473248, weight_bytes=74080, activation_bytes=399168, launches=18)


@pytest.mark.parametrize("case", sorted(CASES))
def test_launch_table_vs_golden(case):
    from ldm_sdf import UNet1DDenoiser
    kw, n, ddpm = CASES[case]
    with open(GOLD) as fh:
        want = json.load(fh)[case]
    got = launch_table(UNet1DDenoiser(**kw), n, ddpm)
    assert len(got) == len(want) == 18
    for k, (g, w) in enumerate(zip(got, want)):
        assert g == w, f"{case}: conv {k}"


def test_ragged_concat_at_n2_still_raises():
    """Widths that are no multiples of 16 put the second concat operand at a channel offset the
    sampling pack cannot serve: an error, not a different read."""
    from ldm_sdf import LdmError, UNet1DDenoiser
    with pytest.raises(LdmError, match="channels 24"):
        launch_table(UNet1DDenoiser(**TINY), 2)


def test_plan_names_have_shapes_and_fused_form():
    from ldm_sdf.unet import unet_plan, unet_shapes
    sh = unet_shapes(72, (8, 24, 40))
    plain, fused = unet_plan((8, 24, 40)), unet_plan((8, 24, 40), True)
    for plan in (plain, fused):
        assert len(plan) == 18
        assert {s.x for r in plan for s in r.segs} | {r.out for r in plan} <= set(sh)
    # the fused form: res4 / res5 read one buffer; one segment fewer in each of their two convs
    diff = [k for k in range(18) if plain[k] != fused[k]]
    assert [plain[k].out for k in diff] == ["a4", "r4", "a5", "r5"]
    assert all(len(plain[k].segs) == len(fused[k].segs) + 1 for k in diff)
    assert sh["cat1"] == (48, 36) and sh["cat0"] == (16, 72)


@pytest.mark.parametrize("C", [(32, 64, 128), (8, 24, 40)])
def test_backward_schedule(C):
    from ldm_sdf.unet import backward_schedule, unet_plan
    plan = unet_plan(C)
    sched = backward_schedule(plan)
    assert sched[0][:2] == ("w", 17) and plan[17].segs[0].w == "conv_out.w"
    assert [e[1] for e in sched if e[0] == "w"] == list(range(17, -1, -1))
    first, accum = {}, {}
    for pos, e in enumerate(sched):
        if e[0] == "alias":
            assert e[1] not in first                   # the block input's gradient STARTS here
            first[e[1]] = pos
        elif e[0] == "d":
            x = plan[e[1]].segs[e[2]].x
            if e[3]:
                assert x in first, f"{x}: accumulated before written"
                accum[x] = accum.get(x, 0) + 1
            else:
                assert x not in first, f"{x}: written twice"
                first[x] = pos
    acts = {s.x for r in plan for s in r.segs} | {r.out for r in plan}
    assert set(first) == acts - {"x", "eps"}            # eps: the loss writes its gradient
    # a block input is read by the block's first conv and its shortcut / identity: one
    # accumulation; the skips s0 / s1 feed a down conv and a decoder block: one more
    blocks_in = {"h0", "d0", "d1", "m0", "u1", "u0"}
    assert accum == {**{x: 1 for x in blocks_in}, "s0": 2, "s1": 2}
    n_w = sum(e[0] == "w" for e in sched)
    n_d = sum(e[0] == "d" for e in sched)
    assert n_w == 18 and n_d == sum(len(r.segs) for r in plan) - 1
    assert n_w + n_d == 41                              # len(UNetTrainer.bwd) before the plan
    assert [e[1:] for e in sched if e[0] == "copy"] == [("res5.bs", "res5.b2"),
                                                        ("res4.bs", "res4.b2")]
