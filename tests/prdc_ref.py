"""fp64 numpy references of the precision / recall / density / coverage primitives (mg_knn_radius2 and
mg_manifold_counts, csrc/mg_eval.hip) and the bounds their tests use.

The device evaluates D(a, b) = (sq_a + sq_b) - 2 dot(a, b) in fp64 with the fp32 MFMA dot.  With u = 2^-24, for any
pair
  |D_dev(a, b) - D_exact(a, b)| <= E(a, b) = 2 (d + 1) u sum_k |a_k| |b_k| + 2^-40 (sq_a + sq_b)
((d + 1) u sum |a_k| |b_k|: the fp32 fma chain of eval_ref.py, times the 2 in front of the dot; the second term
covers the fp64 norm sums and the two fp64 additions with a wide margin).  Order statistics and minima move by at
most the largest perturbation of their inputs:
  |radius2_dev[i] - radius2_exact[i]| <= Erad[i] = max_{j != i} E(i, j)
  |dmin2_dev[a] - dmin2_exact[a]| <= max_b E(a, b)
and a membership test D(a, b) <= radius2[b] is decided when |D_exact - radius2_exact[b]| exceeds E(a, b) (the radii
handed to the kernel are the reference's own) or E(a, b) + Erad[b] (the radii come from the device).
"""
import numpy as np

from eval_ref import U


def sqdist(A, B):
    """fp64 [na, nb] of |a - b|^2 as (sq_a + sq_b) - 2 <a, b> (exact on small-integer data)."""
    A, B = A.astype(np.float64), B.astype(np.float64)
    return ((A * A).sum(1)[:, None] + (B * B).sum(1)[None, :]) - 2.0 * (A @ B.T)


def pair_bound(A, B):
    """E(a, b) for every pair, [na, nb]."""
    A, B = A.astype(np.float64), B.astype(np.float64)
    d = A.shape[1]
    return (2.0 * (d + 1) * U * (np.abs(A) @ np.abs(B).T)
            + 2.0 ** -40 * ((A * A).sum(1)[:, None] + (B * B).sum(1)[None, :]))


def ref_radius2(X, k):
    """(sq, radius2, Erad): the rows' squared norms, the k-th smallest of {D(x_i, x_j) : j != i} (self left out by
    index: a duplicate row is a neighbour at distance 0) and the bound of each radius."""
    X64 = X.astype(np.float64)
    n = len(X)
    assert 1 <= k < n
    D, E = sqdist(X, X), pair_bound(X, X)
    D[np.arange(n), np.arange(n)] = np.inf
    E[np.arange(n), np.arange(n)] = 0.0
    return (X64 * X64).sum(1), np.sort(D, axis=1)[:, k - 1], E.max(1)


def ref_counts(A, B, radius2B):
    """(count, dmin2) by the definition: count[a] = #{b : D(a, b) <= radius2B[b]}, dmin2[a] = min_b D(a, b)."""
    D = sqdist(A, B)
    return (D <= np.asarray(radius2B)[None, :]).sum(1), D.min(1)


def count_intervals(A, B, radius2B, radius_err=None):
    """(lower, upper, undecided, dmin2, dmin_bound) per row of A: ``lower`` counts the pairs that are inside and
    decided, ``upper`` adds the row's undecided pairs, ``undecided`` marks the rows that have any; a pair is decided
    when |D - radius2B[b]| > E(a, b) + radius_err[b] (``radius_err``: Erad of B when the kernel is given device
    radii, None when it is given ``radius2B`` itself)."""
    D, E = sqdist(A, B), pair_bound(A, B)
    r = np.asarray(radius2B, np.float64)[None, :]
    tol = E if radius_err is None else E + np.asarray(radius_err)[None, :]
    decided = np.abs(D - r) > tol
    lower = ((D <= r) & decided).sum(1)
    upper = lower + (~decided).sum(1)
    return lower, upper, (~decided).any(1), D.min(1), E.max(1)


def prdc_intervals(F, R, k):
    """The exact (precision, recall, density, coverage) of generated rows F against real rows R in fp64, the interval
    of each when every undecided test (device radii: E + Erad) is resolved either way, and the numbers of F rows and R
    rows with an undecided test: (exact, lo, hi, undecided_f, undecided_r), the first three dicts."""
    n, m = len(F), len(R)
    _, rad_f, erad_f = ref_radius2(F, k)
    _, rad_r, erad_r = ref_radius2(R, k)
    lo_fr, up_fr, und_f, _, _ = count_intervals(F, R, rad_r, erad_r)
    lo_rf, up_rf, und_r, dmin_rf, dmin_b = count_intervals(R, F, rad_f, erad_f)
    c_fr, _ = ref_counts(F, R, rad_r)
    c_rf, _ = ref_counts(R, F, rad_f)
    cov_decided = np.abs(dmin_rf - rad_r) > dmin_b + erad_r
    cov_in = dmin_rf <= rad_r
    exact = {"precision": (c_fr > 0).mean(), "recall": (c_rf > 0).mean(), "density": c_fr.sum() / (k * n),
             "coverage": cov_in.mean()}
    lo = {"precision": (lo_fr > 0).mean(), "recall": (lo_rf > 0).mean(), "density": lo_fr.sum() / (k * n),
          "coverage": (cov_in & cov_decided).mean()}
    hi = {"precision": (up_fr > 0).mean(), "recall": (up_rf > 0).mean(), "density": up_fr.sum() / (k * n),
          "coverage": (cov_in | ~cov_decided).mean()}
    return exact, lo, hi, int(und_f.sum()), int((und_r | ~cov_decided).sum())
