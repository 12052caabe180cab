"""The two precision / recall / density / coverage kernels (csrc/mg_eval.hip) against fp64 numpy: mg_knn_radius2 and
mg_manifold_counts.

Both take their dots on the exact-fp32 MFMA and their squared distances in fp64, so small-integer data, whose every
dot, norm and distance is exact, must come back **equal** to the reference -- with duplicate rows inside a set
(radius 0 when a row has k duplicates), a duplicate across the two sets and ties exactly at the radius planted -- and
random data must stay inside the bounds of prdc_ref.py: every radius within Erad, every row's count between the
pairs that are decided inside and those plus the row's undecided pairs, every minimum within its bound.  The kernels
work on 64 x 64 tiles and split the column tiles over segments, so the shapes cover one tile, 63 / 64 / 65 rows, a
ragged last tile and several segments; k = n - 1 and k = 16; d of one partial k chunk and of many.  Features are
strided views (ld = d + 4) of buffers whose padding columns and rows past the end hold NaN: anything read out of
range poisons the result.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from moegan_mi import _lib as L  # noqa: E402
from moegan_mi import ops  # noqa: E402

from prdc_ref import count_intervals, ref_counts, ref_radius2, sqdist  # noqa: E402

DEV = "cuda"
# (545 rows: nine column tiles over eight segments of two, so four segments hold two tiles, one the ragged tile alone
# and three none)
RADIUS_EXACT = [(2, 4, 1), (3, 8, 2), (17, 8, 16), (63, 12, 3), (64, 12, 3), (65, 12, 3), (129, 64, 5), (257, 512, 5),
                (545, 8, 3)]
COUNT_EXACT = [(1, 1, 4), (5, 4, 8), (65, 63, 12), (63, 65, 12), (257, 130, 512), (70, 545, 8)]
RADIUS_RANDOM = [(33, 36, 3), (129, 64, 5), (257, 512, 5)]
COUNT_RANDOM = [(33, 31, 36), (65, 63, 12), (129, 127, 64), (257, 130, 512)]
RATIOS = {}  # the largest error / bound seen by the random-data tests, printed by each


def _padded(a):
    """Device view [n, d] with ld = d + 4 of a NaN-filled [n + 3, d + 4] buffer holding ``a``."""
    n, d = a.shape
    buf = torch.full((n + 3, d + 4), float("nan"), device=DEV, dtype=torch.float32)
    buf[:n, :d] = torch.from_numpy(a).to(DEV)
    v = buf[:n, :d]
    assert v.stride() == (d + 4, 1)
    return v


def _random_pair(n, m, d):
    rng = np.random.default_rng(7 * n + 3 * m + d)
    X = (0.5 * rng.standard_normal((n, d))).astype(np.float32)
    Y = (0.5 * rng.standard_normal((m, d)) + 0.02).astype(np.float32)
    return X, Y


def _f64(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(DEV)


def _integer_rows(rng, n, d, k):
    """Integers in [-3, 3] with, where n allows, k + 1 identical rows spread over the set (each has k duplicates:
    radius 0; two identical rows otherwise) and two rows at the same distance 1 from a third (a tie in its list)."""
    X = rng.integers(-3, 4, (n, d)).astype(np.float32)
    if n >= 3:
        copies = k + 1 if n >= k + 3 else 2
        idx = np.unique(np.concatenate([[0, n - 1], rng.choice(n, copies, replace=False)]))[:copies]
        X[idx] = X[idx[0]]
    if n >= 12:
        free = [i for i in range(n) if not (X[i] == X[0]).all()]
        t, p, q = free[0], free[len(free) // 2], free[-1]
        X[t, 0] = 0
        X[p], X[q] = X[t], X[t]
        X[p, 0], X[q, 0] = 1, -1
    return X


def test_binding():
    for name in ("mg_knn_radius2", "mg_manifold_counts"):
        assert name in L.exported_symbols()
        assert L.ARGNAMES[name][-1] == "stream"
        assert hasattr(L.lib(), name)


@pytest.mark.parametrize("n,d,k", RADIUS_EXACT)
def test_radius_exact(n, d, k):
    rng = np.random.default_rng(100 * n + 10 * d + k)
    X = _integer_rows(rng, n, d, k)
    want_sq, want_r2, _ = ref_radius2(X, k)
    if n >= k + 3:
        assert want_r2[0] == 0.0  # the planted duplicates
    sq, r2 = ops.knn_radius2(_padded(X), k)
    assert sq.dtype == torch.float64 and r2.dtype == torch.float64
    sq, r2 = sq.cpu().numpy(), r2.cpu().numpy()
    assert (sq == want_sq).all(), (sq, want_sq)
    assert (r2 == want_r2).all(), (np.nonzero(r2 != want_r2), r2, want_r2)


@pytest.mark.parametrize("na,nb,d", COUNT_EXACT)
def test_counts_exact(na, nb, d):
    rng = np.random.default_rng(1000 * na + nb + d)
    k = min(3, nb - 1)
    B = _integer_rows(rng, nb, d, max(k, 1))
    A = rng.integers(-3, 4, (na, d)).astype(np.float32)
    if nb >= 2:
        _, r2B, _ = ref_radius2(B, k)
        A[0] = B[nb - 1]  # a duplicate across the sets
        if na >= 5:
            # a copy of the k-th nearest neighbour of B's row 1: exactly at that row's radius
            D = sqdist(B, B)
            D[1, 1] = np.inf
            A[na - 1] = B[np.argsort(D[1], kind="stable")[k - 1]]
            assert (sqdist(A, B)[na - 1, 1] == r2B[1])
    else:
        r2B = sqdist(A, B)[0]  # one row on each side: the pair sits exactly at the radius
    sqA, sqB = (A.astype(np.float64) ** 2).sum(1), (B.astype(np.float64) ** 2).sum(1)
    want_count, want_dmin = ref_counts(A, B, r2B)
    count, dmin = ops.manifold_counts(_padded(A), _f64(sqA), _padded(B), _f64(sqB), _f64(r2B))
    assert count.dtype == torch.int32 and dmin.dtype == torch.float64
    count, dmin = count.cpu().numpy(), dmin.cpu().numpy()
    assert (count == want_count).all(), (count, want_count)
    assert (dmin == want_dmin).all(), (dmin, want_dmin)


@pytest.mark.parametrize("n,d,k", RADIUS_RANDOM)
def test_radius_random(n, d, k):
    X, _ = _random_pair(n, n, d)
    want_sq, want_r2, erad = ref_radius2(X, k)
    sq, r2 = (t.cpu().numpy() for t in ops.knn_radius2(_padded(X), k))
    ratio = (np.abs(r2 - want_r2) / erad).max()
    RATIOS["radius2"] = max(RATIOS.get("radius2", 0.0), ratio)
    print("radius", (n, d, k), "largest error / bound", ratio, "so far", RATIOS)
    assert np.isfinite(r2).all()
    assert (np.abs(sq - want_sq) <= 2.0 ** -40 * want_sq).all()
    assert (np.abs(r2 - want_r2) <= erad).all()


@pytest.mark.parametrize("na,nb,d", COUNT_RANDOM)
def test_counts_random(na, nb, d):
    k = 5
    A, B = _random_pair(na, nb, d)
    sqB, r2B, _ = ref_radius2(B, k)
    sqA = (A.astype(np.float64) ** 2).sum(1)
    lower, upper, undecided, want_dmin, dmin_bound = count_intervals(A, B, r2B)
    print("counts", (na, nb, d), "undecided rows", int(undecided.sum()), "of", na)
    assert undecided.sum() <= na // 16  # (on the reference, before the device is consulted)
    count, dmin = ops.manifold_counts(_padded(A), _f64(sqA), _padded(B), _f64(sqB), _f64(r2B))
    count, dmin = count.cpu().numpy(), dmin.cpu().numpy()
    ratio = (np.abs(dmin - want_dmin) / dmin_bound).max()
    RATIOS["dmin2"] = max(RATIOS.get("dmin2", 0.0), ratio)
    print("counts", (na, nb, d), "dmin2 largest error / bound", ratio, "so far", RATIOS)
    assert ((lower <= count) & (count <= upper)).all(), (count, lower, upper)
    assert (np.abs(dmin - want_dmin) <= dmin_bound).all()


def test_repeatable():
    X, Y = _random_pair(257, 130, 512)
    x, y = _padded(X), _padded(Y)
    a = ops.knn_radius2(y, 5)
    b = ops.knn_radius2(y, 5)
    sqx, _ = ops.knn_radius2(x, 5)
    for s, t in zip(a, b):
        assert s.cpu().numpy().tobytes() == t.cpu().numpy().tobytes()
    c = ops.manifold_counts(x, sqx, y, a[0], a[1])
    e = ops.manifold_counts(x, sqx, y, a[0], a[1])
    for s, t in zip(c, e):
        assert s.cpu().numpy().tobytes() == t.cpu().numpy().tobytes()


def _raw(name, *args):
    rc = getattr(L.lib(), name)(*args)
    return rc, L.lib().mg_last_error().decode()


@pytest.mark.parametrize("what", ["k=0", "k=17", "k=n", "d=6", "d=1028", "work"])
def test_rejected_arguments(what):
    n, d, k = 8, 8, 3
    nwork_knn, nwork_counts = n * k, 2 * n  # one column segment at 8 rows
    if what == "k=0":
        k = 0
    elif what == "k=17":
        k = 17
    elif what == "k=n":
        k = n
    elif what == "d=6":
        d = 6
    elif what == "d=1028":
        d = 1028
    else:
        nwork_knn, nwork_counts = nwork_knn - 1, nwork_counts - 1  # one double too small
    ld = 1032
    X = torch.ones(8, ld, device=DEV)
    Y = torch.ones(8, ld, device=DEV)
    f64 = lambda rows, v: torch.full((rows,), v, device=DEV, dtype=torch.float64)  # noqa: E731
    work, sq, r2 = f64(64, -7.0), f64(8, -7.0), f64(8, -7.0)
    sqA, sqB, r2B = f64(8, 8.0), f64(8, 8.0), f64(8, 1.0)
    count = torch.full((8,), -7, device=DEV, dtype=torch.int32)
    dmin = f64(8, -7.0)
    p = L.ptr
    rc, msg = _raw("mg_knn_radius2", p(X), ld, n, d, k, p(work), nwork_knn, p(sq), p(r2), L.stream())
    assert rc != 0 and "mg_knn_radius2" in msg, (rc, msg)
    assert what != "work" or "work buffer too small" in msg, msg
    if not what.startswith("k="):
        rc, msg = _raw("mg_manifold_counts", p(X), ld, n, p(sqA), p(Y), ld, n, p(sqB), p(r2B), d, p(work), nwork_counts,
                       p(count), p(dmin), L.stream())
        assert rc != 0 and "mg_manifold_counts" in msg, (rc, msg)
    torch.cuda.synchronize()
    assert (work == -7).all() and (sq == -7).all() and (r2 == -7).all() and (count == -7).all() and (dmin == -7).all()
