"""Ragged causal self-attention forward (mg_attn_causal.hip: bf16 MFMA path at head dim 64, scalar fp32 / bf16 path)
vs an fp64 causal softmax per sequence on the same (bf16-rounded) qkv.  Bars are the project's existing ones:
bf16 rel < 2e-2 (tests/test_attn_gpu.py), fp32 rel <= 1e-5 (tests/test_xattn_gpu.py), relative to the reference's
max.  Also: no look-ahead (bit-exact), prefix agreement within one output rounding, guard rows, determinism and the
argument checks."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

from moegan_mi import ops  # noqa: E402

DEV = "cuda"
NINE = torch.randint(2, 78, (9,), generator=torch.Generator().manual_seed(9)).tolist()
SHAPES = [(512, 8, (77, 2, 17)),  # full length, minimal length, one past a 16-row tile
          (128, 2, (1, 128)),      # both length limits
          (512, 8, tuple(NINE)),   # B not a multiple of 8
          (512, 8, (3, 20, 1, 16, 31, 8, 64, 5))]  # B a multiple of 8: the XCD-aware unit mapping
DTYPES = [torch.bfloat16, torch.float32]


def rel(a, b):
    return ((a.double() - b.double()).abs().max() / b.double().abs().max().clamp_min(1e-300)).item()


def _row_off(lens):
    off = [0]
    for n in lens:
        off.append(off[-1] + n)
    return torch.tensor(off, device=DEV, dtype=torch.int32)


@functools.lru_cache(maxsize=None)
def _case(C, heads, lens, dtype):
    """(qkv, reference out in fp64), computed once per case and shared; never written to."""
    g = torch.Generator(device=DEV).manual_seed(C + heads + sum(lens))
    R, D = sum(lens), C // heads
    qkv = (torch.randn(R, 3 * C, device=DEV, generator=g) * 1.5).to(dtype)
    x = qkv.double()
    ref = torch.empty(R, C, device=DEV, dtype=torch.float64)
    r0 = 0
    for n in lens:
        q, k, v = (x[r0:r0 + n, i * C:(i + 1) * C].reshape(n, heads, D).transpose(0, 1) for i in range(3))
        s = q @ k.transpose(-1, -2) / D ** 0.5
        s = s.masked_fill(torch.ones(n, n, device=DEV, dtype=torch.bool).triu(1), float("-inf"))
        ref[r0:r0 + n] = (torch.softmax(s, -1) @ v).transpose(0, 1).reshape(n, C)
        r0 += n
    return qkv, ref


def _run(qkv, lens, C, heads, out=None):
    o = ops.attn_causal_fwd(qkv, _row_off(lens), len(lens), max(lens), C, heads=heads, out=out)
    torch.cuda.synchronize()
    return o


def _bar_check(C, heads, lens, dtype):
    qkv, ref = _case(C, heads, lens, dtype)
    got = _run(qkv, lens, C, heads)
    assert got.shape == ref.shape and got.dtype == dtype
    e = rel(got, ref)
    print(f"causal {dtype} C={C} heads={heads} lens={list(lens)}: rel {e:.3e}")
    if dtype == torch.bfloat16:
        assert e < 2e-2
    else:
        assert e <= 1e-5


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("C,heads,lens", SHAPES)
def test_causal_vs_fp64(C, heads, lens, dtype):
    _bar_check(C, heads, lens, dtype)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_causal_head_dim_16_scalar_path(dtype):
    """D = 16 is off the MFMA path in both dtypes (bf16 falls back to the scalar kernel, as mg_attn_fwd does)."""
    _bar_check(128, 8, (5, 33), dtype)


@pytest.mark.parametrize("dtype", DTYPES)
def test_no_look_ahead_exact(dtype):
    """Rows after a cut are overwritten with other finite values: the rows up to the cut do not change by a bit
    (masked scores give probability exactly 0 and the code path is the same)."""
    C, heads, lens = 512, 8, (77,)
    qkv, _ = _case(C, heads, lens, dtype)
    base = _run(qkv, lens, C, heads)
    for n in (1, 15, 16, 17, 32, 33):
        other = qkv.clone()
        g = torch.Generator(device=DEV).manual_seed(n)
        other[n + 1:] = (torch.randn(77 - n - 1, 3 * C, device=DEV, generator=g) * 3 + 1).to(dtype)
        got = _run(other, lens, C, heads)
        assert torch.equal(got[:n + 1], base[:n + 1]), n
        assert not torch.equal(got[n + 1:], base[n + 1:]), n


@pytest.mark.parametrize("dtype", DTYPES)
def test_prefix_is_its_own_sequence(dtype):
    """The sequence truncated to n rows, as its own call, agrees with the first n rows of the long run within one
    output rounding (only the number of masked slots differs: the bar of test_xattn_gpu.py's key_len test)."""
    C, heads, lens = 512, 8, (77,)
    qkv, _ = _case(C, heads, lens, dtype)
    base = _run(qkv, lens, C, heads)
    tol = 2.0 ** -7 if dtype == torch.bfloat16 else 1e-5
    for n in (1, 15, 16, 17, 32, 33):
        got = _run(qkv[:n].contiguous(), (n,), C, heads)
        assert rel(got, base[:n]) <= tol, n


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("C,heads,lens", SHAPES[:2])
def test_guard_rows_and_determinism(C, heads, lens, dtype):
    qkv, _ = _case(C, heads, lens, dtype)
    R = sum(lens)
    out = torch.full((R + 16, C), 7.0, device=DEV, dtype=dtype)
    _run(qkv, lens, C, heads, out=out)
    again = _run(qkv, lens, C, heads)
    assert bool((out[R:].float() == 7.0).all())
    assert torch.equal(out[:R], again)
    assert torch.equal(again, _run(qkv, lens, C, heads))


def test_rejects_unsupported_shapes():
    from moegan_mi._lib import MGError
    off = _row_off((4,))
    with pytest.raises(MGError):  # Lmax 129
        ops.attn_causal_fwd(torch.zeros(4, 3 * 512, device=DEV), off, 1, 129, 512)
    with pytest.raises(MGError):  # head dim 8
        ops.attn_causal_fwd(torch.zeros(4, 3 * 64, device=DEV), off, 1, 4, 64, heads=8)


def test_empty_batch_is_a_noop():
    out = torch.full((16, 512), 7.0, device=DEV)
    ops.attn_causal_fwd(torch.zeros(0, 3 * 512, device=DEV), _row_off(()), 0, 1, 512, out=out)
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
