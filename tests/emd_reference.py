"""fp64 restatement of the earth mover's distance and of the auction that computes it on the GPU
(DESIGN.md §18), in numpy: the reference the GPU tests compare against.  Known answers pin it in
tests/test_emd_reference.py.

EMD(a, b) = (1/n) min over permutations pi of sum_i |a_i - b_pi(i)|, Euclidean, equal sizes only.
``hungarian`` is exact (scipy's linear_sum_assignment); ``auction`` is the eps-scaled Jacobi
auction with the kernel's rules (tie for best: the smaller object; tie for an object: the smaller
bidder; eps from max(eps, extent / 4) down by theta per phase, prices kept, owners cleared) and
also reports its round count and largest price, which the default round cap and the price cap of
the kernel come from.
"""
import numpy as np

U32 = 2.0 ** -24
THETA = 4.0
SLACK_U = 55.0          # ldm_emd_slack(extent) = 55 u extent
PRICE_CAP_EXTENTS = 8.0


def pair_dist(a, b):
    """fp64 |a_i - b_j| as an [n, m] matrix (the differences first)."""
    a = np.asarray(a, dtype=np.float64).reshape(-1, 3)
    b = np.asarray(b, dtype=np.float64).reshape(-1, 3)
    diff = a[:, None, :] - b[None, :, :]
    return np.sqrt(diff[..., 0] * diff[..., 0] + diff[..., 1] * diff[..., 1]
                   + diff[..., 2] * diff[..., 2])


def _same_size(a, b):
    a = np.asarray(a, dtype=np.float64).reshape(-1, 3)
    b = np.asarray(b, dtype=np.float64).reshape(-1, 3)
    if a.shape[0] != b.shape[0] or a.shape[0] == 0:
        raise ValueError("emd: clouds must have the same, non-zero size")
    return a, b


def extent(a, b):
    """Diagonal of the bounding box of both clouds."""
    p = np.concatenate([np.asarray(a, np.float64).reshape(-1, 3),
                        np.asarray(b, np.float64).reshape(-1, 3)])
    return float(np.linalg.norm(p.max(axis=0) - p.min(axis=0)))


def slack(ext):
    return SLACK_U * U32 * ext


def min_eps(ext):
    return 8.0 * slack(ext)


def assignment_cost(a, b, pi):
    """(1/n) sum_i |a_i - b_pi(i)| in fp64."""
    a, b = _same_size(a, b)
    d = a - b[np.asarray(pi)]
    return float(np.sqrt((d * d).sum(axis=1)).sum() / a.shape[0])


def hungarian(a, b):
    """(EMD, pi): the exact optimum."""
    from scipy.optimize import linear_sum_assignment
    a, b = _same_size(a, b)
    rows, cols = linear_sum_assignment(pair_dist(a, b))
    pi = np.empty(a.shape[0], dtype=np.int64)
    pi[rows] = cols
    return assignment_cost(a, b, pi), pi


def emd(a, b):
    return hungarian(a, b)[0]


def emd_matrix(a, b=None):
    """Exact EMD(a_s, b_r); ``b=None``: the within-set matrix (symmetric, zero diagonal)."""
    if b is None:
        S = len(a)
        out = np.zeros((S, S))
        for s in range(S):
            for r in range(s + 1, S):
                out[s, r] = out[r, s] = emd(a[s], a[r])
        return out
    return np.array([[emd(x, y) for y in b] for x in a])


def auction(a, b, eps=1e-4, theta=THETA, max_rounds=None):
    """The kernel's auction in fp64.  Returns a dict: ``pi`` (or None when ``max_rounds`` was
    hit), ``cost``, ``rounds``, ``max_price``, ``evals`` (bidder x object evaluations)."""
    a, b = _same_size(a, b)
    n = a.shape[0]
    if n == 1:
        return dict(pi=np.zeros(1, np.int64), cost=assignment_cost(a, b, [0]), rounds=0,
                    max_price=0.0, evals=0)
    D = pair_dist(a, b)
    price = np.zeros(n)
    e = max(eps, 0.25 * extent(a, b))
    rounds = evals = 0
    max_price = 0.0
    while True:
        price -= price.min()            # a common constant changes no bid; it bounds the prices
        owner = np.full(n, -1, dtype=np.int64)
        unassigned = np.arange(n)
        while unassigned.size:
            if max_rounds is not None and rounds >= max_rounds:
                return dict(pi=None, cost=float("nan"), rounds=rounds,
                            max_price=max(max_price, float(price.max())), evals=evals)
            k = unassigned.size
            T = D[unassigned] + price[None, :]
            j1 = np.argmin(T, axis=1)                           # the first minimum
            t1 = T[np.arange(k), j1]
            T[np.arange(k), j1] = np.inf
            t2 = T.min(axis=1)
            bid = price[j1] + ((t2 - t1) + e)
            # per object: the highest bid, the smallest bidder on a tie
            order = np.lexsort((unassigned, -bid, j1))
            first = np.ones(k, dtype=bool)
            first[1:] = j1[order][1:] != j1[order][:-1]
            win = order[first]
            lost = np.ones(k, dtype=bool)
            lost[win] = False
            objs = j1[win]
            displaced = owner[objs]
            owner[objs] = unassigned[win]
            price[objs] = bid[win]
            unassigned = np.concatenate([unassigned[lost], displaced[displaced >= 0]])
            rounds += 1
            evals += k * n
        max_price = max(max_price, float(price.max()))
        if e <= eps:
            break
        e = max(eps, e / theta)
    pi = np.empty(n, dtype=np.int64)
    pi[owner] = np.arange(n)
    return dict(pi=pi, cost=assignment_cost(a, b, pi), rounds=rounds,
                max_price=max_price, evals=evals)


# ---- the inputs of tests/test_gpu_emd.py (and of the CPU test that sizes the round cap) -------
SIZES = (1, 2, 63, 64, 65, 257, 1025)


def case(kind, n):
    """A pair of fp32 clouds [n, 3]: 'uniform', 'permuted' (a permuted copy + N(0, 1e-3)),
    'translated' (a copy moved by (0.3, 0, 0)), 'lattice' (7 values per axis: duplicates and
    ties everywhere)."""
    seed = {"uniform": 1, "permuted": 2, "translated": 3, "lattice": 4}[kind]
    rng = np.random.default_rng(1000 * seed + n)
    a = rng.uniform(-1, 1, (n, 3)).astype(np.float32)
    if kind == "uniform":
        b = rng.uniform(-1, 1, (n, 3)).astype(np.float32)
    elif kind == "permuted":
        b = (a[rng.permutation(n)] + rng.normal(0, 1e-3, (n, 3))).astype(np.float32)
    elif kind == "translated":
        b = (a + np.array([0.3, 0, 0], np.float32)).astype(np.float32)
    else:
        a = (rng.integers(0, 7, (n, 3)) / 4 - 0.75).astype(np.float32)
        b = (rng.integers(0, 7, (n, 3)) / 4 - 0.75).astype(np.float32)
    return a, b


def cases():
    out = [(kind, n) for n in SIZES for kind in ("uniform", "permuted", "translated")]
    out.append(("lattice", 257))
    return out
