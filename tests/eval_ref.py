"""fp64 numpy references of the evaluation kernels (csrc/mg_eval.hip), shared by their tests.

Bound of the kernel sums, with u = 2^-24, t = gamma g + coef0 and A_ij = sum_k |x_ik| |y_jk| in fp64:
  |S_dev - S_ref| <= 1.01 * sum_pairs [3 t^2 |gamma| (d + 1) u A + 5 u |t|^3]
((d + 1) u A: a d-long fp32 fma chain in any order plus the rounding of gamma g; 5 u |t|^3: the rounding of + coef0,
three times through the cube, and the cube's two multiplies; the fp64 accumulation is below 2^-40 sum |k|).
"""
import numpy as np

U = 2.0 ** -24


def ref_sums(X, Y, gamma, coef0):
    """fp64 (S_xx, S_yy, S_xy) of k(a, b) = (gamma <a, b> + coef0)^3 and the bound of each."""
    X, Y = X.astype(np.float64), Y.astype(np.float64)
    d = X.shape[1]
    out, bound = [], []
    for A, B, offdiag in ((X, X, True), (Y, Y, True), (X, Y, False)):
        t = gamma * (A @ B.T) + coef0
        k = t ** 3
        e = 3 * t * t * abs(gamma) * (d + 1) * U * (np.abs(A) @ np.abs(B).T) + 5 * U * np.abs(t) ** 3
        if offdiag:
            np.fill_diagonal(k, 0.0)
            np.fill_diagonal(e, 0.0)
        out.append(k.sum())
        bound.append(1.01 * e.sum())
    return np.array(out), np.array(bound)


def ref_rank(I, T, group):
    """(rank, diag, S) by the definition, in fp64: s_ij = <I_i, T_j>, rank[i] = the number of j in row i's group with
    s_ij > s_ii, plus those below i with s_ij == s_ii."""
    S = I.astype(np.float64) @ T.astype(np.float64).T
    n = len(I)
    rank, diag = np.zeros(n, np.int64), np.zeros(n)
    for i in range(n):
        g0 = (i // group) * group
        js = np.arange(g0, min(g0 + group, n))
        s = S[i, js]
        rank[i] = ((s > S[i, i]) & (js != i)).sum() + ((s == S[i, i]) & (js < i)).sum()
        diag[i] = S[i, i]
    return rank, diag, S


def margins(S, group):
    """min over the other j of row i's group of |s_ij - s_ii| (inf for a group of one)."""
    n = len(S)
    out = np.full(n, np.inf)
    for i in range(n):
        g0 = (i // group) * group
        gap = np.abs(S[i, g0:min(g0 + group, n)] - S[i, i])
        gap[i - g0] = np.inf
        out[i] = gap.min()
    return out
