"""CPU checks of ldm_sdf.metrics: MMD / COV / 1-NNA on hand-made matrices and
against tests/chamfer_reference.py, the argument errors of the Python layer, the exported
constants, and the C error-path checker tests/c/chamfer_errors.c (the source `make check-asan`
also runs under host AddressSanitizer)."""

import numpy as np
import pytest
import torch

from tests import chamfer_reference as C
from tests.c_checker import run_c_checker


def _t(x):
    return torch.tensor(x, dtype=torch.float32)


def test_hand_made_3x3():
    import ldm_sdf
    cd_gr = _t([[1, 5, 6], [4, 2, 7], [8, 9, 3]])
    cd_gg = _t([[0, 10, 10], [10, 0, 10], [10, 10, 0]])
    cd_rr = _t([[0, .5, 20], [.5, 0, 20], [20, 20, 0]])
    m = ldm_sdf.generation_metrics(cd_gr, cd_gg, cd_rr)
    # column minima 1, 2, 3; the row argmins 0, 1, 2 cover every reference
    assert m["mmd"] == 2.0 and m["cov"] == 1.0
    # every g is nearest a reference (1, 2, 3 < 10); r0 and r1 are nearest each other (0.5);
    # r2 is nearest g2 (3 < 20): two of six have their neighbour in their own set
    assert m["1nna"] == pytest.approx(2 / 6, abs=1e-15)
    assert all(type(v) in (float, int) for v in m.values())
    m = ldm_sdf.generation_metrics(_t([[1, 5, 6], [2, 4, 7], [8, 9, 3]]), cd_gg, cd_rr)
    assert m["mmd"] == pytest.approx(8 / 3, abs=1e-15) and m["cov"] == pytest.approx(2 / 3)


def test_identical_sets():
    import ldm_sdf
    rng = np.random.default_rng(1)
    d = rng.uniform(1, 2, (5, 5))
    d = d + d.T
    np.fill_diagonal(d, 0.0)
    m = ldm_sdf.generation_metrics(*(torch.from_numpy(d),) * 3)
    # every element's nearest other is its twin in the other set (0, the smaller merged index
    # among the zeros being the twin itself for R, and for G the only zero off the diagonal)
    assert m == {"mmd": 0.0, "cov": 1.0, "1nna": 0.0}


def test_two_separated_clusters():
    import ldm_sdf
    S, R = 4, 3
    near = lambda n: torch.full((n, n), 0.01) - 0.01 * torch.eye(n)   # noqa: E731
    m = ldm_sdf.generation_metrics(torch.full((S, R), 100.0), near(S), near(R))
    assert m["1nna"] == 1.0 and m["mmd"] == 100.0 and m["cov"] == pytest.approx(1 / R)


def test_all_generated_nearest_one_reference():
    import ldm_sdf
    S, R = 5, 4
    cd_gr = torch.full((S, R), 3.0)
    cd_gr[:, 2] = torch.tensor([1.0, 1.5, 0.5, 2.0, 2.5])
    m = ldm_sdf.generation_metrics(cd_gr, torch.ones(S, S), torch.ones(R, R))
    assert m["cov"] == 1 / R


def test_ties_go_to_the_smaller_merged_index():
    import ldm_sdf
    # g0: g1 (merged 1) and r0 (merged 2) tie at 1 -> g1, its own set; g1 -> g0, own; r0 -> g0
    m = ldm_sdf.generation_metrics(_t([[1], [3]]), _t([[0, 1], [1, 0]]), _t([[0]]))
    assert m["1nna"] == pytest.approx(2 / 3, abs=1e-15)
    # r0 (merged 1): g0 (merged 0) and r1 (merged 2) tie at 1 -> g0, the other set;
    # r1 -> r0, own; g0 -> r0, other
    m = ldm_sdf.generation_metrics(_t([[1, 5]]), _t([[0]]), _t([[0, 1], [1, 0]]))
    assert m["1nna"] == pytest.approx(1 / 3, abs=1e-15)
    # COV: a row whose minimum is attained twice counts the smaller column
    m = ldm_sdf.generation_metrics(_t([[2, 2, 5], [2, 7, 2]]), _t([[0, 1], [1, 0]]),
                                   torch.ones(3, 3))
    assert m["cov"] == pytest.approx(1 / 3)


@pytest.mark.parametrize("S,R,seed", [(1, 1, 0), (7, 4, 1), (12, 30, 2)])
def test_agrees_with_the_reference_on_random_matrices(S, R, seed):
    import ldm_sdf
    rng = np.random.default_rng(seed)

    def sym(n):
        d = rng.integers(1, 6, (n, n)).astype(np.float64) / 4      # small integers: many ties
        d = d + d.T
        np.fill_diagonal(d, 0.0)
        return d

    cd_gr = rng.integers(1, 8, (S, R)).astype(np.float64) / 4
    cd_gg, cd_rr = sym(S), sym(R)
    got = ldm_sdf.generation_metrics(*(torch.from_numpy(x) for x in (cd_gr, cd_gg, cd_rr)))
    want = C.generation_metrics(cd_gr, cd_gg, cd_rr)
    assert got["mmd"] == pytest.approx(want["mmd"], rel=1e-15)
    assert got["cov"] == want["cov"] and got["1nna"] == want["1nna"]


def test_generation_metrics_rejects_bad_matrices():
    import ldm_sdf
    ok = torch.ones(2, 3)
    for args in ((ok, torch.ones(3, 3), torch.ones(3, 3)), (ok, torch.ones(2, 2), torch.ones(2, 2)),
                 (torch.ones(6), torch.ones(2, 2), torch.ones(3, 3)),
                 (torch.ones(0, 3), torch.ones(0, 0), torch.ones(3, 3)),
                 (ok.long(), torch.ones(2, 2), torch.ones(3, 3))):
        with pytest.raises(ValueError):
            ldm_sdf.generation_metrics(*args)


def test_cpu_tensors_raise_ldm_error():
    import ldm_sdf
    a, b = torch.zeros(4, 3), torch.ones(5, 3)
    with pytest.raises(ldm_sdf.LdmError, match="GPU only"):
        ldm_sdf.nearest_points(a, b)
    with pytest.raises(ldm_sdf.LdmError, match="GPU only"):
        ldm_sdf.chamfer_matrix(a[None], b[None])
    with pytest.raises(ldm_sdf.LdmError, match="GPU only"):
        ldm_sdf.chamfer_matrix(a[None])
    with pytest.raises(ldm_sdf.LdmError, match="GPU only"):
        ldm_sdf.chamfer_distance(a, b)
    with pytest.raises(ldm_sdf.LdmError, match="GPU only"):
        ldm_sdf.evaluate_generation(a[None], b[None])


def test_shape_and_dtype_errors():
    import ldm_sdf
    good2, good3 = torch.zeros(4, 3), torch.zeros(2, 4, 3)
    bad2 = [torch.zeros(4, 2), torch.zeros(4, 3, dtype=torch.float64), torch.zeros(3),
            torch.zeros(1, 4, 3), torch.zeros(4, 3, dtype=torch.int32), np.zeros((4, 3))]
    bad3 = [torch.zeros(4, 3), torch.zeros(2, 4, 2), torch.zeros(2, 4, 3, dtype=torch.float16),
            torch.zeros(1, 2, 4, 3)]
    for t in bad2:
        for args in ((t, good2), (good2, t)):
            with pytest.raises(ldm_sdf.LdmError, match="float32 \\[n, 3\\]"):
                ldm_sdf.nearest_points(*args)
            with pytest.raises(ldm_sdf.LdmError, match="float32 \\[n, 3\\]"):
                ldm_sdf.chamfer_distance(*args)
    for t in bad3:
        with pytest.raises(ldm_sdf.LdmError, match="float32 \\[S, n, 3\\]"):
            ldm_sdf.chamfer_matrix(t)
        with pytest.raises(ldm_sdf.LdmError, match="float32 \\[S, n, 3\\]"):
            ldm_sdf.chamfer_matrix(good3, t)
        with pytest.raises(ldm_sdf.LdmError, match="float32 \\[S, n, 3\\]"):
            ldm_sdf.evaluate_generation(t, good3)


def test_exported_constants():
    from ldm_sdf import metrics
    assert metrics.tile_a() >= 1 and metrics.chunk_b() >= 1
    assert metrics.split_below() >= 1 and metrics.spread_below() >= 1


def test_chamfer_errors_from_c(tmp_path):
    run_c_checker("chamfer_errors", tmp_path)
