"""The earth mover's distance on the MI355X against tests/emd_reference.py: the
returned assignment is a permutation whose fp64 cost is within eps + slack of the Hungarian
optimum, the returned value is that cost to a few u, entries are pure functions of their clouds
bit for bit, the round cap ends a launch, and MMD / COV / 1-NNA over EMD match the exact ones.

Bounds (u = 2^-24), none of them measured:
  cost - optimum in [0, eps + slack], slack = emd_slack(extent) = 55 u extent: eps-complementary
      slackness, 5 u (extent + price cap) for the fp32 values and bids with the price cap at
      8 extents, and 5 u extent twice for the fp32 distances (the assignment's and the optimum's)
  |out - cost| <= 6 u cost: a pair distance is within 5 u (the header), the fp64 sum adds
      nothing visible, the final rounding u
MMD is a mean of matrix entries, so it cannot equal the exact one bit for bit: it is held to
[-6 u, eps + slack + 6 u] around it.  COV and 1-NNA are counts and are equal exactly: the seed
is chosen (and checked here) so that no argmin hangs on a difference under 2 (eps + slack).

Measured on the MI355X (this file, printed before each assertion; profiles/emd/test_gpu_emd.txt):
  test_assignment_is_within_eps_of_the_optimum   cost - optimum at most 2.5e-7 (uniform, 1025
                                      points; 0 in 20 of the 22 cases) against 1.1e-4;
                                      |out - cost| at most 0.81 u; rounds 8 to 4541 against caps
                                      of 33 280 to 295 168
  test_generation_metrics_over_emd    entries -2.0e-8 to 2.0e-6 from the exact ones
"""
import numpy as np
import pytest
import torch

from tests import chamfer_reference as C
from tests import emd_reference as E

pytestmark = pytest.mark.gpu
U = 2.0 ** -24
EPS = 1e-4
FP64_NOISE = 1e-12          # summation order of a few thousand fp64 terms of size <= 4


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import ldm_sdf
    ldm_sdf.load_library()
    return torch.device("cuda", 0)


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32).numpy()


def _slack(a, b):
    from ldm_sdf import metrics
    # the Python layer rounds the extent up by a few 2^-20 before it asks the library
    return metrics.emd_slack(E.extent(a, b) * (1 + 2.0 ** -18))


_REF = {}


def _reference(kind, n):
    """(a, b, optimum) of a case, the Hungarian solve done once."""
    if (kind, n) not in _REF:
        a, b = E.case(kind, n)
        _REF[kind, n] = (a, b, E.emd(a, b))
    return _REF[kind, n]


# --------------------------------------------------------------- 1. the bound, case by case
@pytest.mark.parametrize("kind,n", E.cases())
def test_assignment_is_within_eps_of_the_optimum(dev, kind, n):
    import ldm_sdf
    from ldm_sdf import metrics
    a, b, opt = _reference(kind, n)
    ta, tb = torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev)
    val, pi = ldm_sdf.emd_distance(ta, tb, eps=EPS, return_assignment=True)
    _, rounds = ldm_sdf.emd_matrix(ta[None], tb[None], eps=EPS, return_rounds=True)
    pi = pi.cpu().numpy()
    assert pi.dtype == np.int32 and sorted(pi.tolist()) == list(range(n))
    cost = E.assignment_cost(a, b, pi)
    slack = _slack(a, b)
    val = float(val)
    print(f"{kind} n={n}: cost - opt = {cost - opt:.3e} (eps + slack = {EPS + slack:.3e}), "
          f"|out - cost| / cost = {abs(val - cost) / max(cost, 1e-300) / U:.2f} u, "
          f"rounds = {int(rounds)} (cap {metrics.emd_default_max_rounds(n)})")
    assert -FP64_NOISE <= cost - opt <= EPS + slack
    assert abs(val - cost) <= 6 * U * cost
    assert 0 <= int(rounds) < metrics.emd_default_max_rounds(n)
    assert (int(rounds) == 0) == (n == 1)
    if kind == "translated":
        assert opt == pytest.approx(0.3, rel=1e-6)


# ------------------------------------------------------------------------------- 2. purity
def _batch(dev, S, n, seed):
    rng = np.random.default_rng(seed)
    scale = rng.uniform(0.4, 1.0, (S, 1, 1))
    return torch.from_numpy((rng.uniform(-1, 1, (S, n, 3)) * scale).astype(np.float32)).to(dev)


def test_entries_are_pure_functions_of_their_clouds(dev):
    import ldm_sdf
    a, b = _batch(dev, 5, 65, 21), _batch(dev, 3, 65, 22)
    m = ldm_sdf.emd_matrix(a, b, eps=EPS)
    assert m.shape == (5, 3) and m.dtype == torch.float32
    assert np.array_equal(_bits(ldm_sdf.emd_matrix(a, b, eps=EPS)), _bits(m))       # a second run
    for s, r in ((0, 0), (4, 2), (2, 1)):
        one = ldm_sdf.emd_matrix(a[s:s + 1], b[r:r + 1], eps=EPS)
        assert _bits(one)[0, 0] == _bits(m)[s, r]
        assert _bits(ldm_sdf.emd_distance(a[s], b[r], eps=EPS)) == _bits(m)[s, r]
    ps, pr = torch.tensor([3, 0, 4, 1, 2], device=dev), torch.tensor([2, 0, 1], device=dev)
    assert np.array_equal(_bits(ldm_sdf.emd_matrix(a[ps], b[pr], eps=EPS)),
                          _bits(m[ps][:, pr]))


def test_within_set_matrix(dev):
    import ldm_sdf
    from ldm_sdf import metrics
    a = _batch(dev, 5, 63, 23)
    m, rounds = ldm_sdf.emd_matrix(a, eps=EPS, return_rounds=True)
    assert np.array_equal(_bits(m), _bits(m.t()))
    assert np.all(_bits(m.diagonal()) == 0)                  # +0.0, not merely small
    assert np.array_equal(rounds.cpu().numpy(), rounds.t().cpu().numpy())
    for s in range(5):
        for r in range(s + 1, 5):
            assert _bits(ldm_sdf.emd_matrix(a[s:s + 1], a[r:r + 1], eps=EPS))[0, 0] == \
                _bits(m)[s, r]
    # the assignments: the identity on the diagonal, the inverse permutation below it
    out, assign, _ = metrics._emd(a, None, EPS, None, True, "test")
    assert np.array_equal(_bits(out), _bits(m))
    assign = assign.cpu().numpy()
    for s in range(5):
        assert np.array_equal(assign[s, s], np.arange(63))
        for r in range(s + 1, 5):
            assert sorted(assign[s, r].tolist()) == list(range(63))
            assert np.array_equal(assign[r, s][assign[s, r]], np.arange(63))


# ---------------------------------------------------------------------------- 3. round cap
def test_round_cap_names_the_entry_and_leaves_no_trace(dev):
    import ldm_sdf
    a, b = _batch(dev, 2, 64, 24), _batch(dev, 2, 64, 25)
    before, rounds = ldm_sdf.emd_matrix(a, b, eps=EPS, return_rounds=True)
    assert int(rounds.min()) > 4
    with pytest.raises(ldm_sdf.LdmError, match=r"4 entries.*\(0, 0\).*\(1, 1\)"):
        ldm_sdf.emd_matrix(a, b, eps=EPS, max_rounds=1)
    assert np.array_equal(_bits(ldm_sdf.emd_matrix(a, b, eps=EPS)), _bits(before))


# ------------------------------------------------------------------------------ 4. metrics
_METRICS_SEED = 1


def _metric_clouds():
    rng = np.random.default_rng(_METRICS_SEED)
    scale = lambda k: rng.uniform(0.3, 1.0, (k, 1, 1))                      # noqa: E731
    g = (rng.uniform(-1, 1, (6, 64, 3)) * scale(6)).astype(np.float32)
    r = (rng.uniform(-1, 1, (5, 64, 3)) * scale(5)).astype(np.float32)
    return g, r


def _argmin_margin(gr, gg, rr):
    """Smallest gap between the two smallest entries of any row an argmin is taken over."""
    full = np.block([[gg, gr], [gr.T, rr]]).copy()
    np.fill_diagonal(full, np.inf)
    gaps = [np.diff(np.sort(row)[:2])[0] for row in list(gr) + list(full)]
    return float(min(gaps))


def test_generation_metrics_over_emd(dev):
    import ldm_sdf
    from ldm_sdf import metrics
    g, r = _metric_clouds()
    gr, gg, rr = E.emd_matrix(g, r), E.emd_matrix(g), E.emd_matrix(r)
    both = np.concatenate([g.reshape(-1, 3), r.reshape(-1, 3)])
    tol = EPS + metrics.emd_slack(E.extent(both, both) * (1 + 2.0 ** -18))
    assert _argmin_margin(gr, gg, rr) > 2 * tol, "choose another _METRICS_SEED"
    want = C.generation_metrics(gr, gg, rr)
    tg, tr = torch.from_numpy(g).to(dev), torch.from_numpy(r).to(dev)
    got = ldm_sdf.evaluate_generation(tg, tr, metrics=("cd", "emd"))
    for name, ref in (("emd_gr", gr), ("emd_gg", gg), ("emd_rr", rr)):
        d = got[name].double().cpu().numpy() - ref
        print(f"{name}: entry - exact in [{d.min():.3e}, {d.max():.3e}] (bound {tol:.3e})")
        assert np.all(d >= -6 * U * ref - FP64_NOISE) and np.all(d <= tol + 6 * U * ref)
    assert got["cov_emd"] == want["cov"] and got["1nna_emd"] == want["1nna"]
    assert -6 * U * want["mmd"] <= got["mmd_emd"] - want["mmd"] <= tol + 6 * U * want["mmd"]
    # the *_emd numbers are generation_metrics, unchanged, on the EMD matrices
    assert ldm_sdf.generation_metrics(got["emd_gr"], got["emd_gg"], got["emd_rr"]) == \
        {k[:-4]: got[k] for k in ("mmd_emd", "cov_emd", "1nna_emd")}
    # and the Chamfer half is what it was
    cd = ldm_sdf.evaluate_generation(tg, tr)
    assert sorted(cd) == ["1nna", "cd_gg", "cd_gr", "cd_rr", "cov", "mmd"]
    assert sorted(got) == sorted(list(cd) + ["1nna_emd", "cov_emd", "mmd_emd", "emd_gg",
                                             "emd_gr", "emd_rr"])
    for k, v in cd.items():
        if isinstance(v, torch.Tensor):
            assert np.array_equal(_bits(v), _bits(got[k]))
        else:
            assert v == got[k]


# ------------------------------------------------------------------------------- 5. errors
def test_errors(dev):
    import ldm_sdf
    from ldm_sdf import metrics
    a = torch.rand(2, 8, 3, device=dev)
    with pytest.raises(ldm_sdf.LdmError, match="same size"):
        ldm_sdf.emd_matrix(a, torch.rand(2, 9, 3, device=dev))
    with pytest.raises(ldm_sdf.LdmError, match="same size"):
        ldm_sdf.emd_distance(a[0], torch.rand(7, 3, device=dev))
    with pytest.raises(ldm_sdf.LdmError, match="same size"):
        ldm_sdf.evaluate_generation(a, torch.rand(2, 9, 3, device=dev), metrics=("cd", "emd"))
    big = torch.zeros(1, metrics.emd_max_points() + 1, 3, device=dev)
    with pytest.raises(ldm_sdf.LdmError, match="emd_max_points"):
        ldm_sdf.emd_matrix(big)
    with pytest.raises(ldm_sdf.LdmError, match="emd_min_eps"):
        ldm_sdf.emd_matrix(a, eps=1e-7)
    with pytest.raises(ldm_sdf.LdmError, match="emd_min_eps"):
        ldm_sdf.emd_matrix(a, eps=0.0)
    with pytest.raises(ldm_sdf.LdmError, match="GPU only"):
        ldm_sdf.emd_matrix(a, a.cpu())
    bad = a.clone()
    bad[1, 3, 2] = float("nan")
    with pytest.raises(ldm_sdf.LdmError, match="non-finite"):
        ldm_sdf.emd_matrix(a, bad)
    with pytest.raises(ldm_sdf.LdmError, match="non-finite"):
        ldm_sdf.emd_distance(bad[1], a[0])
    with pytest.raises(ldm_sdf.LdmError, match="max_rounds"):
        ldm_sdf.emd_matrix(a, max_rounds=0)
    assert ldm_sdf.emd_matrix(a[:0], a).shape == (0, 2)
