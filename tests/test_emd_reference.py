"""Known answers for tests/emd_reference.py, the fp64 reference of the earth mover's distance
(DESIGN.md §18): the exact solver, and the auction whose rules the kernel follows."""
import math

import numpy as np
import pytest

from tests import emd_reference as E


def _cloud(n, seed):
    return np.random.default_rng(seed).uniform(-1, 1, (n, 3))


def test_identical_and_permuted_clouds_give_zero():
    a = _cloud(40, 0)
    assert E.emd(a, a) == 0.0
    perm = np.random.default_rng(1).permutation(40)
    cost, pi = E.hungarian(a, a[perm])
    assert cost == 0.0
    assert np.array_equal(perm[pi], np.arange(40))          # b[pi[i]] is a[i]


def test_translated_copy_gives_the_length_of_the_translation():
    # sum_i |a_i - b_pi(i)| >= |sum_i (a_i - b_pi(i))| = n |v| for every pi: the identity is optimal
    a = _cloud(50, 2)
    v = np.array([0.3, -0.2, 0.6])
    assert E.emd(a, a + v) == pytest.approx(float(np.linalg.norm(v)), rel=1e-14)


def test_two_points_by_hand():
    a = [[0, 0, 0], [1, 0, 0]]
    b = [[1, 1, 0], [0, 2, 0]]
    # identity: sqrt(2) + sqrt(5) = 3.650; swap: 2 + 1 = 3
    cost, pi = E.hungarian(a, b)
    assert cost == pytest.approx(1.5, rel=1e-15) and pi.tolist() == [1, 0]


def test_three_points_by_hand():
    a = [[0, 0, 0], [4, 0, 0], [0, 3, 0]]
    b = [[0, 3, 1], [0, 0, 2], [4, 0, 3]]
    # the vertical matches cost 2 + 3 + 1 = 6; every other permutation has a leg of length >= 3
    # in the plane on top of the heights (the next best, a0-b0 a1-b2 a2-b1: sqrt10 + 3 + sqrt13)
    cost, pi = E.hungarian(a, b)
    assert cost == pytest.approx(2.0, rel=1e-15) and pi.tolist() == [1, 2, 0]
    assert E.assignment_cost(a, b, [0, 2, 1]) == pytest.approx(
        (math.sqrt(10) + 3 + math.sqrt(13)) / 3, rel=1e-15)


def test_collinear_points_match_in_sorted_order():
    rng = np.random.default_rng(3)
    x, y = rng.uniform(-1, 1, 30), rng.uniform(-1, 1, 30)
    d = np.array([1.0, 2.0, -2.0]) / 3
    cost = E.emd(x[:, None] * d, y[:, None] * d)
    assert cost == pytest.approx(float(np.abs(np.sort(x) - np.sort(y)).mean()), rel=1e-13)


def test_unequal_or_empty_clouds_are_refused():
    with pytest.raises(ValueError):
        E.emd(_cloud(3, 0), _cloud(4, 0))
    with pytest.raises(ValueError):
        E.emd(np.zeros((0, 3)), np.zeros((0, 3)))


def test_matrix_is_symmetric_with_zero_diagonal():
    a = np.stack([_cloud(12, s) for s in range(4)])
    m = E.emd_matrix(a)
    assert np.array_equal(m, m.T) and np.all(np.diag(m) == 0)
    assert m[1, 3] == E.emd_matrix(a[1:2], a[3:4])[0, 0]


@pytest.mark.parametrize("n,seed", [(1, 0), (2, 1), (17, 2), (64, 3), (150, 4)])
@pytest.mark.parametrize("eps", [1e-2, 1e-4])
def test_auction_cost_is_within_eps_of_the_optimum(n, seed, eps):
    a, b = _cloud(n, seed), _cloud(n, seed + 100)
    r = E.auction(a, b, eps)
    assert sorted(r["pi"].tolist()) == list(range(n))
    opt = E.emd(a, b)
    assert -1e-13 <= r["cost"] - opt <= eps + 1e-13


def test_auction_with_duplicates_and_ties():
    a, b = E.case("lattice", 257)
    r = E.auction(a, b, 1e-4)
    assert sorted(r["pi"].tolist()) == list(range(257))
    assert -1e-13 <= r["cost"] - E.emd(a, b) <= 1e-4 + 1e-13


def test_auction_round_cap():
    a, b = _cloud(64, 5), _cloud(64, 6)
    full = E.auction(a, b, 1e-4)
    assert full["rounds"] > 4
    cut = E.auction(a, b, 1e-4, max_rounds=1)
    assert cut["pi"] is None and cut["rounds"] == 1 and math.isnan(cut["cost"])


def test_theta_changes_the_path_not_the_bound():
    a, b = _cloud(80, 7), _cloud(80, 8)
    opt = E.emd(a, b)
    for theta in (2.0, 4.0, 8.0):
        assert -1e-13 <= E.auction(a, b, 1e-3, theta=theta)["cost"] - opt <= 1e-3 + 1e-13
