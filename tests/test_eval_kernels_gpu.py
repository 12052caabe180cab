"""The two evaluation kernels (csrc/mg_eval.hip) against fp64 numpy: mg_poly_mmd_sums and mg_retrieval_rank.

Both take their dots on the exact-fp32 MFMA, so data whose every intermediate is exact in fp32 must come back
**equal** to the fp64 sums (the structural check: tiles, masks, fragment maps), and random data must stay inside a
worst-case fp32 bound.  The sums kernel works on 64 x 64 tiles, so the shapes include 63 / 64 / 65 rows beside sizes
of one tile, several tiles and a ragged last tile; d covers one partial k chunk (4, 8), a chunk and a bit (36) and
many chunks (512).  Features are strided views (ld = d + 4) of buffers whose padding columns and rows past the end
hold NaN: anything read out of range poisons the result.

The references and the bound of the random-data tests are in eval_ref.py; gamma is the fp32 value the kernel
receives.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from moegan_mi import _lib as L  # noqa: E402
from moegan_mi import ops  # noqa: E402

from eval_ref import U, margins, ref_rank, ref_sums  # noqa: E402

DEV = "cuda"
SHAPES = [(2, 2, 4), (3, 2, 8), (33, 31, 36), (129, 127, 64), (257, 130, 512), (65, 63, 12), (63, 65, 12),
          (64, 128, 8)]
RANK_CASES = [(1, 1, 4), (5, 2, 8), (10, 3, 36), (100, 100, 512), (257, 128, 512)]


def _padded(a):
    """Device view [n, d] with ld = d + 4 of a NaN-filled [n + 3, d + 4] buffer holding ``a``."""
    n, d = a.shape
    buf = torch.full((n + 3, d + 4), float("nan"), device=DEV, dtype=torch.float32)
    buf[:n, :d] = torch.from_numpy(a).to(DEV)
    v = buf[:n, :d]
    assert v.stride() == (d + 4, 1)
    return v


def _sign_rows(rng, n, d):
    """Rows with 16 entries of +-1 at random positions (every entry when d < 16)."""
    a = np.zeros((n, d), np.float32)
    for i in range(n):
        pos = rng.permutation(d)[:16]
        a[i, pos] = rng.choice([-1.0, 1.0], size=len(pos))
    return a


def _random_pair(n, m, d):
    rng = np.random.default_rng(7 * n + 3 * m + d)
    X = (0.5 * rng.standard_normal((n, d))).astype(np.float32)
    Y = (0.5 * rng.standard_normal((m, d)) + 0.02).astype(np.float32)
    return X, Y


def test_binding():
    for name in ("mg_poly_mmd_sums", "mg_retrieval_rank"):
        assert name in L.exported_symbols()
        assert L.ARGNAMES[name][-1] == "stream"
        assert hasattr(L.lib(), name)


@pytest.mark.parametrize("n,m,d", SHAPES)
def test_sums_exact(n, m, d):
    rng = np.random.default_rng(1000 * n + m + d)
    X, Y = _sign_rows(rng, n, d), _sign_rows(rng, m, d)
    ref, _ = ref_sums(X, Y, 0.25, 1.0)
    got = ops.poly_mmd_sums(_padded(X), _padded(Y), 0.25, 1.0).cpu().numpy()
    print("exact", (n, m, d), got, ref)
    assert got.dtype == np.float64
    assert (got == ref).all(), (got, ref)


@pytest.mark.parametrize("n,m,d", SHAPES)
def test_sums_random(n, m, d):
    X, Y = _random_pair(n, m, d)
    gamma = float(np.float32(1.0 / d))
    ref, bound = ref_sums(X, Y, gamma, 1.0)
    got = ops.poly_mmd_sums(_padded(X), _padded(Y), gamma, 1.0).cpu().numpy()
    print("random", (n, m, d), "err", np.abs(got - ref), "bound", bound)
    assert np.isfinite(got).all()
    assert (np.abs(got - ref) <= bound).all(), (got, ref, bound)


@pytest.mark.parametrize("n,d", [(33, 36), (129, 64), (257, 512)])
def test_sums_diagonal(n, d):
    """Y is X: the cross sum keeps the diagonal the symmetric sum masks."""
    X, _ = _random_pair(n, n, d)
    gamma = float(np.float32(1.0 / d))
    x = _padded(X)
    got = ops.poly_mmd_sums(x, x, gamma, 1.0).cpu().numpy()
    assert got[0] == got[1]
    X64 = X.astype(np.float64)
    t = gamma * (X64 * X64).sum(1) + 1.0
    ref = (t ** 3).sum()
    A = (X64 * X64).sum(1)
    bound = 1.01 * (3 * t * t * gamma * (d + 1) * U * A + 5 * U * np.abs(t) ** 3).sum()
    # the two device sums share every off-diagonal term bit for bit; what is left of them is their fp64 rounding
    bound += 2.0 ** -40 * np.abs((gamma * (X64 @ X64.T) + 1.0) ** 3).sum()
    print("diagonal", (n, d), "err", abs(got[2] - got[0] - ref), "bound", bound)
    assert abs((got[2] - got[0]) - ref) <= bound


def test_sums_repeatable():
    X, Y = _random_pair(257, 130, 512)
    x, y = _padded(X), _padded(Y)
    a = ops.poly_mmd_sums(x, y, 1.0 / 512, 1.0).cpu().numpy()
    b = ops.poly_mmd_sums(x, y, 1.0 / 512, 1.0).cpu().numpy()
    assert a.tobytes() == b.tobytes()


@pytest.mark.parametrize("n,group,d", RANK_CASES)
def test_rank_exact(n, group, d):
    rng = np.random.default_rng(n + 10 * group + d)
    I = rng.integers(-3, 4, (n, d)).astype(np.float32)
    T = rng.integers(-3, 4, (n, d)).astype(np.float32)
    if group >= 2 and n >= 2:
        T[1] = T[0]  # duplicate texts inside a group: the tie goes to the lower index
        if group >= 3 and n >= 3:
            T[2] = T[0]
    if n > group:
        T[group] = T[group - 1]  # and across a group boundary: no tie
    if n > group + 2 and group >= 3:
        T[group + 2] = T[group + 1]
    want_rank, want_diag, _ = ref_rank(I, T, group)
    rank, diag = ops.retrieval_rank(_padded(I), _padded(T), group)
    assert rank.dtype == torch.int32 and diag.dtype == torch.float32
    assert (rank.cpu().numpy() == want_rank).all(), (rank.cpu().numpy(), want_rank)
    assert (diag.cpu().numpy().astype(np.float64) == want_diag).all()


@pytest.mark.parametrize("d", [64, 512])
def test_rank_random(d):
    n, group = 1000, 100
    rng = np.random.default_rng(d)
    G1, G2 = rng.standard_normal((n, d)), rng.standard_normal((n, d))
    norm = lambda a: (a / np.linalg.norm(a, axis=1, keepdims=True)).astype(np.float32)  # noqa: E731
    I, T = norm(G1), norm(0.3 * G1 + G2)
    want_rank, want_diag, S = ref_rank(I, T, group)
    margin = margins(S, group)
    decided = margin > 2 * (d + 1) * U
    print("undecided rows", int((~decided).sum()), "of", n)
    assert (~decided).sum() <= n // 100
    rank, diag = ops.retrieval_rank(_padded(I), _padded(T), group)
    rank, diag = rank.cpu().numpy(), diag.cpu().numpy().astype(np.float64)
    assert (rank[decided] == want_rank[decided]).all()
    print("diag err", np.abs(diag - want_diag).max(), "bound", (d + 1) * U)
    assert (np.abs(diag - want_diag) <= (d + 1) * U).all()


def _raw(name, *args):
    rc = getattr(L.lib(), name)(*args)
    return rc, L.lib().mg_last_error().decode()


@pytest.mark.parametrize("what", ["n=1", "d=6", "d=1028", "group=129"])
def test_rejected_arguments(what):
    n, d, group = 8, 8, 4
    if what == "n=1":
        n = 1
    elif what == "d=6":
        d = 6
    elif what == "d=1028":
        d = 1028
    else:
        group = 129
    ld = 1032
    X = torch.ones(8, ld, device=DEV)
    Y = torch.ones(8, ld, device=DEV)
    part = torch.full((16,), -7.0, device=DEV, dtype=torch.float64)
    sums = torch.full((3,), -7.0, device=DEV, dtype=torch.float64)
    rank = torch.full((8,), -7, device=DEV, dtype=torch.int32)
    diag = torch.full((8,), -7.0, device=DEV)
    p = L.ptr
    if what != "group=129":
        rc, msg = _raw("mg_poly_mmd_sums", p(X), ld, n, p(Y), ld, 8, d, 0.25, 1.0, p(part), 16, p(sums), L.stream())
        assert rc != 0 and "mg_poly_mmd_sums" in msg, (rc, msg)
    if what != "n=1":
        rc, msg = _raw("mg_retrieval_rank", p(X), ld, p(Y), ld, 8, d, group, p(rank), p(diag), L.stream())
        assert rc != 0 and "mg_retrieval_rank" in msg, (rc, msg)
    torch.cuda.synchronize()
    assert (part == -7).all() and (sums == -7).all() and (rank == -7).all() and (diag == -7).all()
