"""UNet training, the host side (no GPU): the argument checks of the conv1d backward entry points
from C (tests/c/unet_bwd_errors.c, the source `make check-asan` also runs under host
AddressSanitizer), the packed-layout round trip, the workspace size formula, the Python API's
argument checks, and the fp32 floor of the gradient and training references the GPU tests
(tests/test_gpu_unet_train.py) compare against."""
import ctypes as C
import os
import shutil
import subprocess

import pytest
import torch

from tests.c_checker import run_c_checker

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
A = 0x7f0000000000          # fake device addresses: never dereferenced by the host checks

# the GPU tests' tiny nets: (D, C, TE, HT, T, B)
TINY = [(64, (16, 32, 48), 16, 32, 50, 3), (72, (8, 24, 40), 16, 32, 50, 5)]


def test_unet_bwd_errors_from_c(tmp_path):
    run_c_checker("unet_bwd_errors", tmp_path)


@pytest.mark.parametrize("shape", [(1, 1, 3), (5, 8, 4), (20, 33, 3), (70, 40, 1), (33, 52, 3),
                                   (128, 128, 3), (17, 16, 1)])
@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
def test_unpack_is_the_inverse_of_pack(shape, dt):
    from ldm_sdf import LdmError, ops
    Cout, Cw, K = shape
    W = torch.randn(*shape, generator=torch.Generator().manual_seed(Cout * 1000 + Cw)).to(dt)
    Wp = ops.pack_conv_weight(W)
    back = ops.unpack_conv_weight(Wp, Cout, Cw)
    assert back.shape == W.shape and back.is_contiguous() and torch.equal(back, W)
    # the padding of a packed tensor built from the unpadded part is zero: re-packing the
    # unpacked part reproduces the pack exactly (rows Cout.., columns outside perm16(0..Cw))
    assert torch.equal(ops.pack_conv_weight(back), Wp)
    r16 = lambda n: (n + 15) // 16 * 16  # noqa: E731
    assert float(Wp[Cout:].abs().sum()) == 0
    pad_cols = sorted(set(range(r16(Cw))) - set(ops.perm16_index(r16(Cw))[:Cw].tolist()))
    assert len(pad_cols) == r16(Cw) - Cw and float(Wp[:, :, pad_cols].abs().sum()) == 0
    with pytest.raises(LdmError):
        ops.unpack_conv_weight(Wp, Cout + 16, Cw)


def _wargs(capi, B, Cout, L_out, segs, dbias, dcbias):
    a = capi.ConvBwdWeightArgs()
    a.B, a.Cout, a.L_out, a.n_seg = B, Cout, L_out, len(segs)
    for i, (Cs, K) in enumerate(segs):
        g = a.seg[i]
        g.X, g.C, g.L_in, g.ksize, g.stride, g.pad = A + 0x100000 * i, Cs, L_out, K, 1, K // 2
        g.kstride = (Cs + 15) // 16 * 16
        g.ldw = K * g.kstride
        a.dW[i] = A + 0x10000000 * (i + 1)
    a.dY = A + 0x80000000
    a.dbias = A + 0x90000000 if dbias else None
    a.dcbias = A + 0xa0000000 if dcbias else None
    return a


@pytest.mark.parametrize("B,Cout,L_out,segs", [
    (1, 1, 1, [(1, 3)]), (3, 32, 100, [(16, 3)]), (2, 24, 64, [(32, 3), (20, 3)]),
    (40, 64, 256, [(64, 3)]), (2, 32, 64, [(32, 3), (16, 1), (16, 1)]),
    (64, 128, 256, [(128, 3)]), (5, 1, 1024, [(1, 3)]), (2, 70, 129, [(33, 3)]),
    (64, 32, 1024, [(64, 3)]), (64, 512, 1024, [(512, 3)])])
def test_workspace_size_formula(B, Cout, L_out, segs):
    """S slices of one packed partial each, S = min(64, B ceil(L_out / 64)), a partial =
    sum_s Cout16 ksize_s round16(C_s) floats; + B Cout when dbias is asked for without dcbias."""
    from ldm_sdf import _capi as capi
    lib = capi.load()
    r16 = lambda n: (n + 15) // 16 * 16  # noqa: E731
    S = min(64, B * -(-L_out // 64))
    part = sum(r16(Cout) * K * r16(Cs) for Cs, K in segs)
    for dbias, dcbias in ((False, False), (True, False), (True, True), (False, True)):
        a = _wargs(capi, B, Cout, L_out, segs, dbias, dcbias)
        want = S * part + (B * Cout if dbias and not dcbias else 0)
        assert lib.ldm_conv1d_bwd_weight_ws_floats(C.byref(a)) == want
    assert lib.ldm_conv1d_bwd_weight_ws_floats(None) == 0


def test_entry_points_reject_bad_arguments_through_ctypes():
    from ldm_sdf import _capi as capi
    lib = capi.load()
    EINVAL, EALIGN, ENOSPC, ENOSYS = -22, -14, -28, -38
    a = _wargs(capi, 2, 24, 64, [(32, 3), (20, 3)], True, False)
    need = lib.ldm_conv1d_bwd_weight_ws_floats(C.byref(a))
    a.ws, a.ws_floats = A + 0xb0000000, need - 1
    assert lib.ldm_conv1d_bwd_weight(C.byref(a), None) == ENOSPC
    assert b"workspace" in lib.ldm_last_error()
    a.ws_floats = need
    a.seg[1].ksize = 5
    assert lib.ldm_conv1d_bwd_weight(C.byref(a), None) == ENOSYS
    a.seg[1].ksize = 3
    a.dW[1] = A + 0x20000000 + 4
    assert lib.ldm_conv1d_bwd_weight(C.byref(a), None) == EALIGN
    d = capi.ConvBwdDataArgs()
    assert lib.ldm_conv1d_bwd_data(C.byref(d), None) == EINVAL
    assert lib.ldm_conv1d_bwd_data(None, None) == EINVAL


def test_struct_layouts_match_c(tmp_path):
    from ldm_sdf import _capi as capi
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        pytest.skip("no C compiler")
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "ldm_sdf.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu %zu %zu\\n",'
                   ' sizeof(ldm_conv1d_bwd_data_args_t), offsetof(ldm_conv1d_bwd_data_args_t, seg),'
                   ' offsetof(ldm_conv1d_bwd_data_args_t, dX), sizeof(ldm_conv1d_bwd_weight_args_t),'
                   ' offsetof(ldm_conv1d_bwd_weight_args_t, dW),'
                   ' offsetof(ldm_conv1d_bwd_weight_args_t, ws_floats)); return 0; }\n')
    exe = str(tmp_path / "layout")
    subprocess.run([cc, "-I", os.path.join(ROOT, "include"), str(src), "-o", exe], check=True)
    got = [int(x) for x in subprocess.run([exe], capture_output=True, text=True).stdout.split()]
    D, W = capi.ConvBwdDataArgs, capi.ConvBwdWeightArgs
    assert got == [C.sizeof(D), D.seg.offset, D.dX.offset, C.sizeof(W), W.dW.offset,
                   W.ws_floats.offset]


def test_python_argument_checks(monkeypatch):
    import ldm_sdf
    from ldm_sdf import dist as ldist, ops
    m = ldm_sdf.UNet1DDenoiser(D=64, C=(16, 32, 48), TE=16, HT=32, T=50, seed=1)
    sch = ldm_sdf.DDPMSchedule(T=50)
    x0, eps = torch.zeros(3, 64), torch.zeros(3, 64)
    t = torch.zeros(3, dtype=torch.int32)
    # CPU tensors: no fallback
    with pytest.raises(ldm_sdf.LdmError):
        ldm_sdf.train_step(m, sch, x0, t, eps, dtype="fp32")
    with pytest.raises(ldm_sdf.LdmError):
        ldm_sdf.train(m, sch, x0, steps=1, dtype="fp32")
    with pytest.raises(ldm_sdf.LdmError):
        ops.conv1d_bwd_data(ops.ConvSegment(torch.zeros(1, 16, 8), torch.zeros(16, 3, 16)),
                            torch.zeros(1, 16, 8), torch.zeros(1, 16, 8))
    with pytest.raises(ldm_sdf.LdmError):
        ops.conv1d_bwd_weight([ops.ConvSegment(torch.zeros(1, 16, 8), torch.zeros(16, 3, 16))],
                              torch.zeros(1, 16, 8), torch.zeros(16, 3, 16))
    # options the UNet path does not have: refused, not ignored
    with pytest.raises(ValueError, match="graph"):
        ldm_sdf.train(m, sch, x0, steps=1, graph=True)
    with pytest.raises(ValueError, match="overlap"):
        ldm_sdf.train(m, sch, x0, steps=1, overlap=True)
    monkeypatch.setattr(ldist, "world_and_rank", lambda group=None: (2, 0))
    with pytest.raises(ValueError, match="data-parallel"):
        ldm_sdf.train(m, sch, x0, steps=1)
    with pytest.raises(ValueError, match="data-parallel"):
        ldm_sdf.train_step(m, sch, x0, t, eps)


@pytest.mark.parametrize("net", TINY, ids=["D64", "D72"])
def test_fp32_gradient_floor(net):
    """The fp32 floor of the reference itself: fp32 torch autograd against fp64 autograd of
    oracle.ref_unet.unet_forward + eps_mse_loss on the GPU tests' tiny nets.  Worst per-tensor
    max|dg| / max|g| measured 2.1e-6 (D = 64) and 4.8e-7 (D = 72); asserted <= 1e-5 so that
    the GPU tests' 1e-4 keeps its margin."""
    from tests.unet_train_ref import oracle_grads
    D, Cc, TE, HT, T, B = net
    g64, l64 = oracle_grads(D, Cc, TE, HT, T, B, torch.float64)
    g32, l32 = oracle_grads(D, Cc, TE, HT, T, B, torch.float32)
    worst = max(float((g32[n].double() - g64[n]).abs().max() / g64[n].abs().max()) for n in g64)
    print(f"fp32 vs fp64 autograd, worst per-tensor max|dg|/max|g| = {worst:.2e}; "
          f"loss rel {abs(l32 - l64) / abs(l64):.2e}")
    assert worst <= 1e-5
