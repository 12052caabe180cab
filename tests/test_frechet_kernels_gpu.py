"""mg_feature_moments (csrc/mg_eval.hip) against fp64 numpy: s1[j] = sum_i x_ij and s2[j][k] = sum_i x_ij x_ik.

Every fp32 entry is widened to fp64 before the fp64 MFMA, so a product is exact and the fp64 additions are the only
roundings.  Integer-valued rows with |x| <= 64 keep every partial sum an integer below 2^32, so the device and numpy
are both exact and must agree **bitwise**, whatever order either adds in; Gaussian rows with a nonzero mean must stay
within twice the bound of frechet_ref.moment_bounds (one summation's bound for the device, one for numpy).  The kernel
works on 64 x 64 column tiles (ci <= cj), stages 32 rows at a time, feeds the MFMA four rows per step and cuts the rows
into S(n, d) segments (ops.moment_segments), so the shapes cover: one row; the MFMA's k edge (3, 4, 5 rows); the staging
edge (63, 64, 65 rows); a partial second column tile (d = 68, 132); the first shape with S > 1 (257 rows at d = 64:
S = 2); a ragged last segment (513 rows at d = 68: S = 3 segments of 172, 172 and 169 rows); the workload's width.
Features are strided views (ld = d + 4) of buffers whose padding columns and rows past the end hold NaN: anything
read out of range poisons the result.
"""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from moegan_mi import _lib as L  # noqa: E402
from moegan_mi import ops  # noqa: E402

from frechet_ref import moment_bounds, moments  # noqa: E402

DEV = "cuda"
EXACT = [(1, 4), (3, 4), (4, 20), (5, 68), (63, 64), (64, 64), (65, 132), (257, 64), (513, 68), (1000, 512)]
RANDOM = [(300, 512), (129, 68)]


def _padded(a):
    """Device view [n, d] with ld = d + 4 of a NaN-filled [n + 3, d + 4] buffer holding ``a``."""
    n, d = a.shape
    buf = torch.full((n + 3, d + 4), float("nan"), device=DEV, dtype=torch.float32)
    buf[:n, :d] = torch.from_numpy(a).to(DEV)
    v = buf[:n, :d]
    assert v.stride() == (d + 4, 1)
    return v


def _integer_rows(n, d):
    """Integers in [-64, 64], no symmetry between the columns (column j is shifted by j mod 7)."""
    rng = np.random.default_rng(1000 * n + d)
    X = rng.integers(-57, 58, (n, d)) + (np.arange(d) % 7)
    assert np.abs(X).max() <= 64
    return X.astype(np.float32)


def _gaussian_rows(n, d):
    rng = np.random.default_rng(7 * n + d)
    return (0.5 * rng.standard_normal((n, d)) + 0.3).astype(np.float32)


def _same_bytes(a, b):
    return np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


def test_binding():
    assert "mg_feature_moments" in L.exported_symbols()
    assert L.ARGNAMES["mg_feature_moments"] == ["X", "ldx", "n", "d", "work", "nwork", "s1", "s2", "accumulate",
                                                "stream"]
    assert hasattr(L.lib(), "mg_feature_moments")


def test_segment_helper():
    # the shapes the docstring names: S = 1, S = 2, three ragged segments, and the cap of 16 at the workload's width
    assert ops.moment_segments(256, 64) == 1 and ops.moment_segments(257, 64) == 2
    assert ops.moment_segments(513, 68) == 3 and ops.moment_segments(1000, 512) == 4
    assert ops.moment_segments(10000, 512) == 16 and ops.moment_segments(1 << 20, 1024) == 8


@pytest.mark.parametrize("n,d", EXACT)
def test_exact(n, d):
    X = _integer_rows(n, d)
    want1, want2 = moments(X)
    s1, s2 = ops.feature_moments(_padded(X))
    assert s1.dtype == torch.float64 and s2.dtype == torch.float64
    assert tuple(s1.shape) == (d,) and tuple(s2.shape) == (d, d)
    s1, s2 = s1.cpu().numpy(), s2.cpu().numpy()
    assert _same_bytes(s1, want1), (s1, want1)
    assert _same_bytes(s2, want2), np.argwhere(s2 != want2)[:8]
    assert _same_bytes(s2, s2.T)


def test_accumulate():
    n, d = 300, 68
    X = _integer_rows(n, d)
    x = _padded(X)
    one1, one2 = ops.feature_moments(x)
    s1 = torch.zeros(d, device=DEV, dtype=torch.float64)
    s2 = torch.zeros(d, d, device=DEV, dtype=torch.float64)
    for lo, hi in ((0, 270), (270, 299), (299, 300)):  # three unequal batches, the last a single row
        r1, r2 = ops.feature_moments(x[lo:hi], s1, s2, accumulate=True)
        assert r1 is s1 and r2 is s2
    assert _same_bytes(s1.cpu().numpy(), one1.cpu().numpy())
    assert _same_bytes(s2.cpu().numpy(), one2.cpu().numpy())
    # accumulate=False overwrites: nothing of a NaN-filled output survives
    s1.fill_(float("nan"))
    s2.fill_(float("nan"))
    ops.feature_moments(x, s1, s2, accumulate=False)
    assert _same_bytes(s1.cpu().numpy(), one1.cpu().numpy())
    assert _same_bytes(s2.cpu().numpy(), one2.cpu().numpy())
    with pytest.raises(L.MGError):
        ops.feature_moments(x, accumulate=True)  # nothing to add to


@pytest.mark.parametrize("n,d", RANDOM)
def test_random(n, d):
    X = _gaussian_rows(n, d)
    want1, want2 = moments(X)
    b1, b2 = moment_bounds(X)
    s1, s2 = (t.cpu().numpy() for t in ops.feature_moments(_padded(X)))
    assert np.isfinite(s1).all() and np.isfinite(s2).all()
    e1, e2 = np.abs(s1 - want1), np.abs(s2 - want2)
    print("moments", (n, d), "largest error / (2 x bound): s1", (e1 / (2 * b1)).max(), "s2", (e2 / (2 * b2)).max())
    assert (e1 <= 2 * b1).all()
    assert (e2 <= 2 * b2).all()
    assert _same_bytes(s2, s2.T)
    # ... and on top of earlier sums: the bound's |old| term
    old1, old2 = moments(_gaussian_rows(40, d))
    t1, t2 = torch.from_numpy(old1).to(DEV), torch.from_numpy(old2).to(DEV)
    ops.feature_moments(_padded(X), t1, t2, accumulate=True)
    b1, b2 = moment_bounds(X, old1, old2)
    assert (np.abs(t1.cpu().numpy() - (old1 + want1)) <= 2 * b1).all()
    assert (np.abs(t2.cpu().numpy() - (old2 + want2)) <= 2 * b2).all()


def test_repeatable():
    x = _padded(_gaussian_rows(300, 512))
    a = ops.feature_moments(x)
    b = ops.feature_moments(x)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        c = ops.feature_moments(x)
    side.synchronize()
    for s, t, u in zip(a, b, c):
        assert _same_bytes(s.cpu().numpy(), t.cpu().numpy())
        assert _same_bytes(s.cpu().numpy(), u.cpu().numpy())


def _raw(name, *args):
    rc = getattr(L.lib(), name)(*args)
    return rc, L.lib().mg_last_error().decode()


@pytest.mark.parametrize("what", ["d=6", "d=1028", "n=0", "work", "misaligned"])
def test_rejected_arguments(what):
    n, d = 8, 8
    nwork = d * d + d  # one row segment at 8 rows
    if what == "d=6":
        d = 6
    elif what == "d=1028":
        d = 1028
    elif what == "n=0":
        n = 0
    elif what == "work":
        nwork -= 1  # one double too small
    ld = 1032
    X = torch.ones(8, ld, device=DEV)
    work = torch.full((nwork + 1,), -7.0, device=DEV, dtype=torch.float64)
    s1 = torch.full((1028,), -7.0, device=DEV, dtype=torch.float64)
    s2 = torch.full((1028 * 8,), -7.0, device=DEV, dtype=torch.float64)
    p = L.ptr
    p1 = ctypes.c_void_p(s1.data_ptr() + 4) if what == "misaligned" else p(s1)
    rc, msg = _raw("mg_feature_moments", p(X), ld, n, d, p(work), nwork, p1, p(s2), 0, L.stream())
    assert rc != 0 and "mg_feature_moments" in msg, (rc, msg)
    assert what != "work" or ("work buffer too small" in msg and str(8 * 8 + 8) in msg), msg
    torch.cuda.synchronize()
    assert (work == -7).all() and (s1 == -7).all() and (s2 == -7).all()
