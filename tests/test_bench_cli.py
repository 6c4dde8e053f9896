"""bench.py's command line: a plain run is the headline alone (``--full`` adds the other legs),
``--steps`` sets the number of timed steps, and ``--dump-outputs DIR`` writes what the last timed
step computed -- whole when small, a fixed seeded sample when large -- which must equal
``ldm_sdf.decode`` of the same seeded inputs bit for bit."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FULL_ONLY = ("decode_b1", "ddpm", "mc", "config5", "train", "autodecoder", "cpu_baseline")


def _bench():
    import bench          # the repository root is on sys.path (tests/conftest.py)
    return bench


def _parse(bench, argv, monkeypatch):
    monkeypatch.setattr(sys, "argv", ["bench.py"] + argv)
    return bench.parse()


def test_full_is_off_by_default(monkeypatch):
    bench = _bench()
    a = _parse(bench, ["--gpus", "1", "--steps", "7", "--warmup", "2"], monkeypatch)
    assert (a.full, a.dump_outputs, a.steps, a.warmup) == (False, None, 7, 2)
    a = _parse(bench, ["--full", "--dump-outputs", "d"], monkeypatch)
    assert a.full and a.dump_outputs == "d"


@pytest.mark.parametrize("argv", [["--steps", "0"], ["--warmup", "-1"]])
def test_rejects_no_timed_steps(argv, monkeypatch):
    bench = _bench()
    with pytest.raises(SystemExit) as e:
        _parse(bench, argv, monkeypatch)
    assert e.value.code == 2


def test_dump_small_volume_is_whole(tmp_path):
    bench = _bench()
    vol = torch.arange(2 * 5 * 5 * 5, dtype=torch.float32).reshape(2, 5, 5, 5)
    bench.dump_outputs(str(tmp_path / "a" / "b"), vol)
    got = np.load(tmp_path / "a" / "b" / "sdf.npy")
    assert got.dtype == np.float32 and got.shape == (250,)
    assert np.array_equal(got, vol.reshape(-1).numpy())


def test_dump_large_volume_is_a_fixed_sample(tmp_path, monkeypatch):
    """Above the cap: exactly the cap's count of values, at the same ascending flat indices in
    every call, spread over the whole volume (value == flat index here)."""
    bench = _bench()
    monkeypatch.setattr(bench, "DUMP_MAX_ELEMS", 1000)
    vol = torch.arange(3 * 16 * 16 * 16, dtype=torch.float32).reshape(3, 16, 16, 16)
    bench.dump_outputs(str(tmp_path / "one"), vol)
    bench.dump_outputs(str(tmp_path / "two"), vol.clone())
    one, two = np.load(tmp_path / "one" / "sdf.npy"), np.load(tmp_path / "two" / "sdf.npy")
    assert one.dtype == np.float32 and one.shape == (1000,)
    assert np.array_equal(one, two)
    assert np.all(np.diff(one) >= 0) and one[0] >= 0 and one[-1] < vol.numel()
    assert one[0] < vol.numel() // 10 and one[-1] > vol.numel() - vol.numel() // 10
    assert bench.DUMP_MAX_ELEMS * 4 <= 64 * 1024 * 1024


@pytest.mark.gpu
def test_plain_run_headline_and_dump(tmp_path):
    """One plain run at a small size: the result line has the headline fields and none of the
    ``--full`` legs, ``ms_per_step`` x ``--steps`` is the timed region ``value`` was computed
    from, and the dumped volume equals ``ldm_sdf.decode`` on the bench's seeded inputs."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    B, N, steps = 3, 24, 2
    out = tmp_path / "dump"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps",
                        str(steps), "--warmup", "1", "--batch", str(B), "--grid", str(N),
                        "--dump-outputs", str(out)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, r.stdout[-2000:]
    res = json.loads(lines[0])
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in res, k
    assert not [k for k in FULL_ONLY if k in res]
    assert res["steps"] == steps and res["step_time_events"]["n"] == steps
    assert res["unit"] == "queries/s" and res["higher_is_better"] is True
    want_value = B * N ** 3 / (res["ms_per_step"] * 1e-3)
    assert abs(res["value"] - want_value) <= 1e-9 * want_value
    assert os.listdir(out) == ["sdf.npy"]
    got = np.load(out / "sdf.npy")
    assert got.dtype == np.float32 and got.shape == (B * N ** 3,)

    import ldm_sdf
    ldm_sdf.load_library()
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev).manual_seed(0)
    latents = torch.randn(B, 256, device=dev, generator=gen) * 0.1
    vol = ldm_sdf.decode(ldm_sdf.SDFDecoder(256, seed=1234), latents, N, dtype=res["dtype"])
    assert np.array_equal(got, vol.reshape(-1).cpu().numpy())
