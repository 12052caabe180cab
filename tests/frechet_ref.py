"""fp64 numpy references for the Fréchet-distance tests: raw moments with their rounding bound, the mean / covariance
formula, and the closed-form distance between Gaussians whose covariances commute."""
import numpy as np

U = 2.0 ** -53  # unit roundoff of fp64


def moments(X):
    """(s1 [d], s2 [d, d]) of the rows of X in fp64 (products of fp32 entries are exact there)."""
    X64 = np.asarray(X, dtype=np.float64)
    return X64.sum(0), X64.T @ X64


def moment_bounds(X, old1=None, old2=None):
    """The rounding bounds of include/moegan_hip.h for one summation of the n rows: (n + 2) 2^-53 (sum_i |x_ij| +
    |old_j|) for s1 and (n + 2) 2^-53 (sum_i |x_ij x_ik| + |old_jk|) for s2.  Any fp64 summation order obeys them, so
    two summations (the device's and numpy's) differ by at most twice them."""
    A = np.abs(np.asarray(X, dtype=np.float64))
    n = A.shape[0]
    b1, b2 = A.sum(0), A.T @ A
    if old1 is not None:
        b1 = b1 + np.abs(old1)
    if old2 is not None:
        b2 = b2 + np.abs(old2)
    return (n + 2) * U * b1, (n + 2) * U * b2


def mean_cov(X):
    X64 = np.asarray(X, dtype=np.float64)
    return X64.mean(0), np.cov(X64, rowvar=False)


def commuting_pair(d, seed):
    """(mu1, S1, mu2, S2, a, b): covariances Q diag(a) Q^T and Q diag(b) Q^T with one random orthogonal Q and spectra
    drawn in [0.25, 4]."""
    rng = np.random.default_rng(seed)
    Q, _ = np.linalg.qr(rng.standard_normal((d, d)))
    a, b = rng.uniform(0.25, 4.0, d), rng.uniform(0.25, 4.0, d)
    S1, S2 = (Q * a) @ Q.T, (Q * b) @ Q.T
    return rng.standard_normal(d), 0.5 * (S1 + S1.T), rng.standard_normal(d), 0.5 * (S2 + S2.T), a, b


def frechet_commuting(mu1, a, mu2, b):
    """|mu1 - mu2|^2 + sum_i (sqrt(a_i) - sqrt(b_i))^2: the distance when the covariances share eigenvectors."""
    diff = np.asarray(mu1, dtype=np.float64) - np.asarray(mu2, dtype=np.float64)
    return float(diff @ diff + ((np.sqrt(a) - np.sqrt(b)) ** 2).sum())


def general_pair(d, seed):
    """Two well-conditioned covariances that do not commute (Wishart draws of 4 d rows plus 0.1 I) and two means."""
    rng = np.random.default_rng(seed)
    A, B = rng.standard_normal((4 * d, d)), rng.standard_normal((4 * d, d)) * rng.uniform(0.5, 1.5, d)
    S1, S2 = A.T @ A / (4 * d) + 0.1 * np.eye(d), B.T @ B / (4 * d) + 0.1 * np.eye(d)
    return rng.standard_normal(d), 0.5 * (S1 + S1.T), rng.standard_normal(d), 0.5 * (S2 + S2.T)


def frechet_bar(d):
    """Absolute bar of the closed-form comparison at spectra in [0.25, 4]: 256 d^2 2^-53 (a backward-stable symmetric
    eigensolver moves an eigenvalue of M = R S2 R by O(d u |M|), |M| <= 16, sqrt(lambda_min) >= 1 / 4, and d square
    roots are summed: about 32 d^2 u times a modest constant)."""
    return 256.0 * d * d * U


def self_bar(d, sigma):
    """|FD(x, x)| <= d^1.5 2^-26 |sigma|_2: each zero eigenvalue of the product comes back as about
    sqrt(d u) |sigma|."""
    return d ** 1.5 * 2.0 ** -26 * float(np.linalg.norm(np.asarray(sigma, dtype=np.float64), 2))
