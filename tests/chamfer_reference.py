"""fp64 restatement of the Chamfer kernels and the generation metrics, in numpy
and chunked: the reference the GPU tests compare against.  Known answers pin it in
tests/test_chamfer_reference.py.

Squared distances throughout: D(a -> b) = mean_i min_j |a_i - b_j|^2, CD = D(a -> b) + D(b -> a).
"""
import numpy as np

CHUNK = 1 << 22   # pairs per block of the brute force


def nearest(q, c):
    """(d2 [P] fp64, idx [P] int64): the lexicographic minimum of (d^2, index) over ``c``."""
    q = np.asarray(q, dtype=np.float64).reshape(-1, 3)
    c = np.asarray(c, dtype=np.float64).reshape(-1, 3)
    if c.shape[0] == 0:
        raise ValueError("nearest: the cloud is empty")
    d2 = np.empty(q.shape[0])
    idx = np.empty(q.shape[0], dtype=np.int64)
    rows = max(1, CHUNK // c.shape[0])
    for i0 in range(0, q.shape[0], rows):
        diff = q[i0:i0 + rows, None, :] - c[None, :, :]          # the differences first
        d = diff[..., 0] * diff[..., 0] + diff[..., 1] * diff[..., 1] + diff[..., 2] * diff[..., 2]
        j = np.argmin(d, axis=1)                                  # numpy: the first minimum
        d2[i0:i0 + rows] = d[np.arange(d.shape[0]), j]
        idx[i0:i0 + rows] = j
    return d2, idx


def pair_d2(q, c, idx):
    """fp64 |q_i - c_idx[i]|^2."""
    diff = np.asarray(q, dtype=np.float64) - np.asarray(c, dtype=np.float64)[np.asarray(idx)]
    return (diff * diff).sum(axis=1)


def directed(a, b):
    """D(a -> b)."""
    return float(nearest(a, b)[0].mean())


def directed_matrix(a, b):
    """out[s, r] = D(a_s -> b_r) for a [S, n, 3], b [R, m, 3]."""
    out = np.empty((len(a), len(b)))
    for s in range(len(a)):
        for r in range(len(b)):
            out[s, r] = directed(a[s], b[r])
    return out


def chamfer_matrix(a, b=None):
    """CD(a_s, b_r); ``b=None``: the within-set matrix."""
    if b is None:
        d = directed_matrix(a, a)
        return d + d.T
    return directed_matrix(a, b) + directed_matrix(b, a).T


def first_argmin(d):
    return np.argmin(d, axis=1)        # numpy documents the first occurrence


def generation_metrics(cd_gr, cd_gg, cd_rr):
    """MMD, COV, 1-NNA; merged indices G first, the smallest merged index wins a tie."""
    cd_gr, cd_gg, cd_rr = (np.asarray(x, dtype=np.float64) for x in (cd_gr, cd_gg, cd_rr))
    S, R = cd_gr.shape
    mmd = float(cd_gr.min(axis=0).mean())
    cov = len(set(first_argmin(cd_gr).tolist())) / R
    full = np.block([[cd_gg, cd_gr], [cd_gr.T, cd_rr]]).copy()
    np.fill_diagonal(full, np.inf)
    nn = first_argmin(full)
    own = np.arange(S + R) < S
    return {"mmd": mmd, "cov": cov, "1nna": float(((nn < S) == own).mean())}
