"""CPU checks of the batched sampling loop's host side: the argument errors
``ldm_sample_batch`` returns before any launch (through ctypes, on fake device addresses that
are never dereferenced), the workspace size, the pure grouping function behind
``sample(form=...)``, and the C error-path checker tests/c/sample_batch_errors.c (the source
`make check-asan` also runs under host AddressSanitizer)."""
import ctypes as C

import pytest

from tests.c_checker import run_c_checker


EINVAL, EALIGN, ENOSYS, ENOSPC = -22, -14, -38, -28
_next = [0x7f0000000000]


def fake() -> int:
    """A distinct, 4 KiB aligned address host code never dereferences."""
    _next[0] += 0x1000000
    return _next[0]


def denoiser(D=256, H=1024, nb=4, dtype="bf16"):
    from ldm_sdf import _capi as capi
    w = capi.Denoiser()
    w.abi_version = capi.ABI_VERSION
    w.dtype = capi.DTYPE_CODES[dtype]
    w.D, w.H, w.n_blocks, w.TE, w.T = D, H, nb, 128, 1000
    w.w_in, w.b_in, w.w_out, w.b_out = fake(), fake(), fake(), fake()
    for k in range(nb):
        w.w_blk[k], w.b_blk[k], w.e_tab[k] = fake(), fake(), fake()
    return w


def sched(T=1000):
    from ldm_sdf import _capi as capi
    sc = capi.Sched()
    sc.abi_version = capi.ABI_VERSION
    sc.T = T
    sc.c1, sc.c2, sc.sigma = fake(), fake(), fake()
    return sc


def call(w, sc, *, x=None, noise=None, t_hi=999, steps=3, B=100, ws=None, ws_bytes=None):
    from ldm_sdf import _capi as capi
    lib = capi.load()
    x = fake() if x is None else x
    noise = fake() if noise is None else noise
    ws = fake() if ws is None else ws
    if ws_bytes is None:
        ws_bytes = lib.ldm_sample_batch_ws_bytes(C.byref(w), B) if w is not None else 1 << 30
    rc = lib.ldm_sample_batch(C.byref(w) if w is not None else None,
                              C.byref(sc) if sc is not None else None, x, noise, t_hi, steps, B,
                              ws, ws_bytes, None)
    if rc != 0:
        assert lib.ldm_last_error(), "an error code without a message"
    return rc


def test_descriptor_errors():
    from ldm_sdf import _capi as capi
    assert call(None, sched()) == EINVAL
    assert call(denoiser(), None) == EINVAL
    w = denoiser()
    w.abi_version = capi.ABI_VERSION + 1
    assert call(w, sched()) == EINVAL
    sc = sched()
    sc.abi_version = 0
    assert call(denoiser(), sc) == EINVAL
    assert call(denoiser(dtype="fp32"), sched()) == ENOSYS
    assert call(denoiser(D=200), sched()) == EINVAL
    assert call(denoiser(H=1000), sched()) == EINVAL
    assert call(denoiser(D=32), sched()) == EINVAL
    w = denoiser()
    w.e_tab[1] = None
    assert call(w, sched()) == EINVAL
    w = denoiser()
    w.n_blocks = capi.MAX_BLOCKS + 1
    assert call(w, sched()) == EINVAL


def test_schedule_range_errors():
    w, sc = denoiser(), sched()
    for t_hi, steps in ((1000, 1), (-1, 1), (999, 0), (999, 1001), (4, 6), (0, 2)):
        assert call(w, sc, t_hi=t_hi, steps=steps) == EINVAL, (t_hi, steps)
    assert call(w, sched(T=500), t_hi=999, steps=1) == EINVAL
    assert call(w, sc, B=0) == EINVAL


def test_workspace_and_alignment_errors():
    from ldm_sdf import _capi as capi
    lib = capi.load()
    w, sc = denoiser(), sched()
    need = lib.ldm_sample_batch_ws_bytes(C.byref(w), 100)
    assert call(w, sc, ws_bytes=need - 1) == ENOSPC
    assert call(w, sc, ws_bytes=0) == ENOSPC
    assert call(w, sc, B=65, ws_bytes=lib.ldm_sample_batch_ws_bytes(C.byref(w), 64)) == ENOSPC
    assert call(w, sc, x=fake() + 4) == EALIGN
    assert call(w, sc, ws=fake() + 128) == EALIGN
    assert call(w, sc, ws=fake() + 16) == EALIGN


def test_workspace_size_steps_at_the_64_row_tile():
    from ldm_sdf import _capi as capi
    lib = capi.load()
    for D, H in ((256, 1024), (64, 128)):
        w = denoiser(D=D, H=H, nb=2)
        size = [lib.ldm_sample_batch_ws_bytes(C.byref(w), b) for b in range(1, 131)]
        assert len(set(size[:64])) == 1 and size[0] == 64 * (2 * D + 8 * H + 4 * H)
        assert size[64] > size[63] and len(set(size[64:128])) == 1 and size[128] > size[127]
        assert all(s % 256 == 0 for s in size)
        assert lib.ldm_sample_batch_supported(C.byref(w), 17) == 1
    assert lib.ldm_sample_batch_ws_bytes(C.byref(denoiser(dtype="fp32")), 17) == 0
    assert lib.ldm_sample_batch_supported(C.byref(denoiser(dtype="fp32")), 17) == 0
    # the stated upper limit: 2^31 / max(D, H) rows
    w = denoiser()
    assert lib.ldm_sample_batch_supported(C.byref(w), 1 << 21) == 1
    assert lib.ldm_sample_batch_supported(C.byref(w), (1 << 21) + 1) == 0
    assert call(w, sched(), B=(1 << 21) + 1, ws_bytes=1 << 62) == ENOSYS


def test_sample_groups():
    from ldm_sdf import api
    g = api.sample_groups
    assert g(1) == ("single", [(0, 1)])
    assert g(16) == ("single", [(0, 16)])
    assert g(17) == ("loop16", [(0, 16), (16, 17)])
    assert 16 < api.BATCHED_FROM
    assert g(api.BATCHED_FROM - 1)[0] in ("single", "loop16")
    assert g(api.BATCHED_FROM)[0] == "batched"
    assert g(512, "auto", None, 64) == ("batched", [(0, 512)])
    assert g(1025, "batched") == ("batched", [(0, 1024), (1024, 1025)])
    assert g(40, "batched", 24) == ("batched", [(0, 24), (24, 40)])
    assert g(40, "loop16") == ("loop16", [(0, 16), (16, 32), (32, 40)])
    assert g(40, "loop16", 24) == ("loop16", [(0, 16), (16, 32), (32, 40)])   # chunk: batched only
    assert g(8, "batched") == ("batched", [(0, 8)])
    assert g(8, "loop16") == ("loop16", [(0, 8)])
    assert g(40, "auto", None, 32) == ("batched", [(0, 40)])
    assert g(40, "auto", None, 41) == ("loop16", [(0, 16), (16, 32), (32, 40)])
    for n in (1, 16, 17, 40, 64, 1000, 4097):
        for form in api.SAMPLE_FORMS:
            for chunk in (None, 1, 24, 5000):
                kind, groups = g(n, form, chunk)
                assert groups[0][0] == 0 and groups[-1][1] == n
                assert all(a[1] == b[0] for a, b in zip(groups, groups[1:]))
                assert all(lo < hi for lo, hi in groups)
                cap = 16 if kind in ("single", "loop16") else (chunk or api.SAMPLE_CHUNK)
                assert max(hi - lo for lo, hi in groups) <= cap


def test_unknown_form_and_bad_sizes():
    import ldm_sdf
    from ldm_sdf import api
    with pytest.raises(ValueError):
        api.sample_groups(40, "mfma")
    with pytest.raises(ValueError):
        api.sample_groups(0)
    with pytest.raises(ValueError):
        api.sample_groups(40, "batched", 0)
    # sample() refuses the form before it touches a device
    with pytest.raises(ValueError):
        ldm_sdf.sample(ldm_sdf.MLPDenoiser(D=64, H=128, n_blocks=1), ldm_sdf.DDPMSchedule(), 40,
                       form="mfma")


def test_sample_batch_errors_from_c(tmp_path):
    run_c_checker("sample_batch_errors", tmp_path)
