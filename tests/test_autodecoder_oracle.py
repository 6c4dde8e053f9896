"""C19 (auto-decoder training) on the CPU: the oracle's objective pinned by known answers and
finite differences, and the product's host-side working layout (pure data movement)."""
import math

import pytest
import torch

from oracle import ref_cpu as R
from oracle import ref_autodecoder as A


def _tiny(seed=3):
    return R.make_decoder_params(L=4, H=16, n_hidden=8, skip=4, seed=seed)


def test_loss_zero_when_prediction_matches():
    p = _tiny()
    g = torch.Generator().manual_seed(0)
    z = torch.randn(2, 4, generator=g, dtype=torch.float64) * 0.3
    xyz = torch.rand(2, 5, 3, generator=g, dtype=torch.float64) * 2 - 1
    sdf = R.decoder_forward(p, z, xyz).detach()
    assert float(A.autodecoder_loss(p, z, xyz, sdf, reg_lambda=0.0)) == 0.0
    # targets far outside the clamp band on the same side as the prediction's clamp: only
    # the clamped parts differ
    big = torch.full_like(sdf, 5.0)
    pred_c = sdf.clamp(-0.1, 0.1)
    want = (pred_c - 0.1).abs().mean()
    assert abs(float(A.autodecoder_loss(p, z, xyz, big, reg_lambda=0.0)) - float(want)) < 1e-15


def test_code_regulariser_known_answer():
    """reg = lambda * min(1, epoch/100) * sum_samples |z| / N = lambda * w * mean_s |z_s|."""
    p = _tiny()
    z = torch.tensor([[3.0, 4.0, 0.0, 0.0], [0.0, 0.0, 0.0, 1.0]], dtype=torch.float64)
    xyz = torch.zeros(2, 3, 3, dtype=torch.float64)
    sdf = R.decoder_forward(p, z, xyz).detach()
    for epoch, w in ((100, 1.0), (50, 0.5), (250, 1.0)):
        got = float(A.autodecoder_loss(p, z, xyz, sdf, reg_lambda=0.01, epoch=epoch))
        assert abs(got - 0.01 * w * (5.0 + 1.0) / 2) < 1e-15


def test_oracle_gradients_match_finite_differences():
    """The float64 autograd the GPU parity tests compare against, against central differences
    (targets inside the clamp band, so the loss is smooth except on measure-zero kinks)."""
    p = _tiny(seed=11)
    g = torch.Generator().manual_seed(1)
    z = torch.randn(2, 4, generator=g, dtype=torch.float64) * 0.5
    xyz = torch.rand(2, 6, 3, generator=g, dtype=torch.float64) * 2 - 1
    sdf = (torch.rand(2, 6, generator=g, dtype=torch.float64) - 0.5) * 0.15
    loss, gr = A.autodecoder_grads(p, z, xyz, sdf, reg_lambda=0.05)
    eps = 1e-6

    def f(pp, zz):
        return float(A.autodecoder_loss(pp, zz, xyz, sdf, reg_lambda=0.05))

    for l in (0, 3, 4, 8):
        for (i, j) in ((0, 0), (1, 2)):
            W = p.weights[l]
            if i >= W.shape[0] or j >= W.shape[1]:
                continue
            hi, lo = p.to(torch.float64), p.to(torch.float64)
            hi.weights[l] = W.clone(); hi.weights[l][i, j] += eps
            lo.weights[l] = W.clone(); lo.weights[l][i, j] -= eps
            fd = (f(hi, z) - f(lo, z)) / (2 * eps)
            assert abs(fd - float(gr[f"W{l}"][i, j])) < 1e-6 * max(1.0, abs(fd)), (l, i, j)
    for (s, c) in ((0, 0), (1, 3)):
        zh, zl = z.clone(), z.clone()
        zh[s, c] += eps
        zl[s, c] -= eps
        fd = (f(p, zh) - f(p, zl)) / (2 * eps)
        assert abs(fd - float(gr["z"][s, c])) < 1e-6 * max(1.0, abs(fd))
    assert loss > 0


def _random_masters(L=256, H=512):
    g = torch.Generator().manual_seed(5)
    m = {}
    for l, (i, o) in enumerate(R.decoder_layer_dims(L, H)):
        m[f"W{l}"] = torch.randn(o, i, generator=g)
        m[f"b{l}"] = torch.randn(o, generator=g)
    return m


# (working dtype, (row_pad, col_pad) or None for work_weights' defaults, zw): the fp32 path's
# pads, the bf16 path's pads on exact fp32 values, and the bf16 path as it runs
@pytest.mark.parametrize("dtype,pads,zw", [(torch.float32, None, 264),
                                           (torch.float32, (64, 64), 320),
                                           (torch.bfloat16, (64, 64), 320)],
                         ids=["fp32-4-8", "fp32-64-64", "bf16-64-64"])
def test_work_layout_round_trip(dtype, pads, zw):
    """work_weights pads, master_grads cuts back: every shape is the padded one, every pad is
    zero, every other element is the master's in the working dtype, and with the padded weights
    fed back in as 'gradients' the masters (rounded to the working dtype) come out unchanged."""
    from ldm_sdf.autodecoder import master_grads, work_weights
    L, H, skip, hs = 256, 512, 4, 253
    m = _random_masters(L, H)
    w = work_weights(m, L, H, skip, dtype, *(pads or ()))
    assert {k: tuple(w[k].shape) for k in ("W0", "W3", "W4h", "W4z", "b3p")} == {
        "W0": (H, zw), "W3": (256, H), "W4h": (H, 256), "W4z": (H, zw), "b3p": (256,)}
    assert float(w["W0"][:, 259:].abs().sum()) == 0
    assert float(w["W3"][253:].abs().sum()) == 0
    assert float(w["b3p"][253:].abs().sum()) == 0
    assert float(w["W4h"][:, 253:].abs().sum()) == 0 and float(w["W4z"][:, 259:].abs().sum()) == 0
    assert all(w[k].dtype == dtype for k in w if k != "b3p") and w["b3p"].dtype == torch.float32
    assert torch.equal(w["W4h"][:, :hs], m["W4"][:, :hs].to(dtype))
    assert torch.equal(w["W4z"][:, :L + 3], m["W4"][:, hs:].to(dtype))
    gw = dict(w)
    for l in range(9):
        gw[f"b{l}"] = m[f"b{l}"]
    gw["b3"] = w["b3p"]
    out = {k: torch.empty_like(v) for k, v in m.items()}
    master_grads(gw, L, skip, hs, out)
    for k in m:
        want = m[k] if k.startswith("b") else m[k].to(dtype).float()
        assert torch.equal(out[k], want), k


def test_layout_matches_the_emulations():
    """The product's one layout record: the fp32 pads give hsp 256 / zw 264 with no row padding
    or blocking; the bf16 blocking of the sample axis is the emulation's independent
    restatement (E.layout) and the expected (N, Np, KT, nblk) on every GPU-test case and on the
    benchmark's 64 x 16384."""
    from ldm_sdf import autodecoder as AD
    from tests import autodecoder_emulation as E
    assert (AD._KQ, AD._KSEG) == (E._KQ, 64)
    f = AD._layout(256, 512, 4, 253, 3, 129, torch.float32)
    assert (f.row_pad, f.col_pad, f.hs, f.hsp, f.zw) == (4, 8, 253, 256, 264)
    assert (f.N, f.Np, f.KT, f.nblk) == (387, 387, 387, 1)
    want = {E.CASE_1x64[:2]: (64, 128, 128, 1), E.CASE_5x96[:2]: (480, 512, 512, 1),
            E.CASE_3x256[:2]: (768, 768, 256, 3), E.CASE_3x200[:2]: (600, 640, 128, 5),
            E.CASE_2x129[:2]: (258, 384, 128, 3), E.CASE_320xP[:2]: (23040, 23040, 512, 45),
            (64, 16384): (1048576, 1048576, 8192, 128)}
    assert set(c[:2] for c in E.CASES) < set(want)
    for (S, P), nums in want.items():
        b = AD._layout(E.L, E.H, E.SKIP, 253, S, P, torch.bfloat16)
        assert (b.row_pad, b.col_pad, b.hs, b.hsp, b.zw) == (64, 64, 253, 256, 320)
        assert (b.N, b.Np, b.KT, b.nblk) == nums, (S, P)
        e = E.layout(S, P)
        assert (e["N"], e["Np"], e["KT"], e["nblk"]) == nums, (S, P)
