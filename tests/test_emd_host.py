"""CPU checks of the earth mover's distance: the host functions against
tests/emd_reference.py, the default round cap against the reference auction's round counts on
the exact inputs of tests/test_gpu_emd.py, the argument errors of the Python layer that need no
GPU, and the C error-path checker tests/c/emd_errors.c (the source `make check-asan` also runs
under host AddressSanitizer)."""

import numpy as np
import pytest
import torch

from tests import emd_reference as E
from tests.c_checker import run_c_checker


def test_host_functions_agree_with_the_reference():
    from ldm_sdf import metrics
    assert metrics.emd_max_points() >= 2048
    for ext in (0.0, 1.0, 2 * 3 ** 0.5, 17.25):
        assert metrics.emd_slack(ext) == E.slack(ext)
        assert metrics.emd_min_eps(ext) == E.min_eps(ext)
    # the default eps is accepted for clouds anywhere in [-1, 1]^3
    assert metrics.emd_min_eps(2 * 3 ** 0.5 * (1 + 2.0 ** -19)) < 1e-4
    assert metrics.emd_default_max_rounds(0) == 0
    assert metrics.emd_default_max_rounds(metrics.emd_max_points() + 1) == 0


@pytest.mark.parametrize("kind,n", E.cases())
def test_reference_auction_stays_under_an_eighth_of_the_default_cap(kind, n):
    from ldm_sdf import metrics
    a, b = E.case(kind, n)
    r = E.auction(a, b, 1e-4)
    assert r["pi"] is not None
    assert r["rounds"] <= metrics.emd_default_max_rounds(n) // 8
    # and its prices under a quarter of the cap the fp32 slack is derived from
    assert r["max_price"] <= E.PRICE_CAP_EXTENTS * E.extent(a, b) / 4


def test_cpu_tensors_raise_ldm_error():
    import ldm_sdf
    a, b = torch.zeros(4, 3), torch.ones(4, 3)
    with pytest.raises(ldm_sdf.LdmError, match="GPU only"):
        ldm_sdf.emd_distance(a, b)
    with pytest.raises(ldm_sdf.LdmError, match="GPU only"):
        ldm_sdf.emd_matrix(a[None], b[None])
    with pytest.raises(ldm_sdf.LdmError, match="GPU only"):
        ldm_sdf.emd_matrix(a[None])
    with pytest.raises(ldm_sdf.LdmError, match="GPU only"):
        ldm_sdf.evaluate_generation(a[None], b[None], metrics=("cd", "emd"))


def test_shape_and_dtype_errors():
    import ldm_sdf
    good2, good3 = torch.zeros(4, 3), torch.zeros(2, 4, 3)
    for t in (torch.zeros(4, 2), torch.zeros(4, 3, dtype=torch.float64), torch.zeros(1, 4, 3),
              np.zeros((4, 3))):
        for args in ((t, good2), (good2, t)):
            with pytest.raises(ldm_sdf.LdmError, match="float32 \\[n, 3\\]"):
                ldm_sdf.emd_distance(*args)
    for t in (torch.zeros(4, 3), torch.zeros(2, 4, 2), torch.zeros(2, 4, 3, dtype=torch.float16)):
        with pytest.raises(ldm_sdf.LdmError, match="float32 \\[S, n, 3\\]"):
            ldm_sdf.emd_matrix(t)
        with pytest.raises(ldm_sdf.LdmError, match="float32 \\[S, n, 3\\]"):
            ldm_sdf.emd_matrix(good3, t)


def test_unknown_metric_is_refused():
    import ldm_sdf
    g = torch.zeros(2, 4, 3)
    for metrics in (("emd",), ("cd", "f-score"), ()):
        with pytest.raises(ldm_sdf.LdmError, match="metrics must be"):
            ldm_sdf.evaluate_generation(g, g, metrics=metrics)


def test_emd_errors_from_c(tmp_path):
    run_c_checker("emd_errors", tmp_path)
