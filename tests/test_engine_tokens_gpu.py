"""GeneratorEngine with packed per-token text rows (text_rows / row_off / lk_max) against the same engine with the
padded text_tokens / text_len form on the same data: fp32 mode, the reference generator's three attention blocks,
E = 4, B = 2, caption lengths [3, 9].  The two differ only in how many zero rows the text-side sums run over and in
the key-slot count of the cross-attention, so the bar is fp32 rounding of a re-ordered reduction: 1e-4 relative to
the tensor's largest entry, the project's fp32 step tolerance.  Pad rows of the packed token gradient are exact
zeros."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle.recipe import fill_state  # noqa: E402

from moegan_mi.engine_g import GeneratorEngine  # noqa: E402
from moegan_mi.layout import generator_shapes  # noqa: E402
from moegan_mi.params import ParamStore  # noqa: E402
from moegan_mi.tokens import pack_tokens  # noqa: E402

DEV = "cuda"
E, B, LENS, L = 4, 2, [3, 9], 9
REL = 1e-4


def _rel(a, b, what):
    a, b = a.detach().double(), b.detach().double()
    assert a.shape == b.shape, what
    scale = float(b.abs().max())
    err = float((a - b).abs().max())
    assert err <= REL * scale + 1e-30, f"{what}: max abs err {err:.3e} (scale {scale:.3e})"
    return err / max(scale, 1e-30)


def _engine():
    st = ParamStore(generator_shapes(E), DEV, frozen_prefixes=("to_rgb_8.",), shadow_dtype=torch.float32)
    st.load_state_dict({k: torch.from_numpy(v) for k, v in fill_state(generator_shapes(E), 0).items()})
    ge = GeneratorEngine(st, E)
    ge.prep()
    return st, ge


def _run(tok_kw):
    st, ge = _engine()
    g = torch.Generator().manual_seed(71)
    z, text = torch.randn(B, 512, generator=g).to(DEV), torch.randn(B, 512, generator=g).to(DEV)
    eps = [tuple(torch.randn(s, generator=g).to(DEV) for s in ((c, 128), (512, 128), (256, E)))
           for c in (512, 256, 128)]
    img16, img8, kl2s, probs, _, ctx = ge.forward(z, text, eps, 3.0, 0.7, train=True, save=True, want_img8=True,
                                                  **tok_kw)
    g16 = torch.randn(img16.shape, generator=g).to(DEV)
    g16[..., 3:] = 0
    g8 = torch.randn(img8.shape, generator=g).to(DEV)
    g8[..., 3:] = 0
    kl2 = torch.stack(kl2s)
    gz, gtext, gtok = ge.backward(ctx, g16, kl_coef=(0.37 * kl2[:, 1]).contiguous(), want_input_grads=True, g_img8=g8)
    torch.cuda.synchronize()
    return dict(img16=img16, img8=img8, kl2=kl2, probs=probs, gz=gz, gtext=gtext, gtok=gtok, st=st)


def test_engine_packed_vs_padded_tokens():
    rng = np.random.default_rng(5)
    tok = rng.standard_normal((B, L, 512)).astype(np.float16)
    for b, n in enumerate(LENS):
        tok[b, n:] = 0
    rows, off, lk = pack_tokens(tok, LENS)
    assert rows.shape == (16, 512) and off.tolist() == [0, 3, 12] and lk == 32
    pad = _run(dict(text_tokens=torch.from_numpy(tok).float().to(DEV),
                    text_len=torch.tensor(LENS, dtype=torch.int32, device=DEV)))
    pak = _run(dict(text_rows=torch.from_numpy(rows).float().to(DEV), row_off=torch.from_numpy(off).to(DEV),
                    lk_max=lk))
    for k in ("img16", "img8", "kl2", "gz", "gtext"):
        print(k, _rel(pak[k], pad[k], k))
    for i in range(3):
        _rel(pak["probs"][i], pad["probs"][i], f"probs{i}")
    # token gradient: packed [rows, 512] against the live rows of the padded [B, L, 512]; pad rows exact zeros
    gt = pak["gtok"]
    assert gt.shape == (16, 512)
    live = torch.cat([pad["gtok"][b, :n] for b, n in enumerate(LENS)])
    assert float(live.abs().max()) > 0
    print("gtok", _rel(gt[:12], live, "token gradient"))
    assert bool((gt[12:] == 0).all())
    for b, n in enumerate(LENS):  # the padded form's masked slots carry none either
        assert bool((pad["gtok"][b, n:] == 0).all())
    sp, sq = pad["st"], pak["st"]
    n_live = 0
    for n in sp.offsets:
        gp, gq = sp.gview(n), sq.gview(n)
        if float(gp.abs().max()) == 0.0:
            assert float(gq.abs().max()) == 0.0, n
            continue
        _rel(gq, gp, n)
        n_live += 1
    assert n_live > 150
    for n in ("gen_block_4.attn_block.norm2.weight", "gen_block_16.attn_block.cross_attn.in_proj_weight",
              "text_projection.0.weight"):
        assert float(sq.gview(n).abs().max()) > 0, n


def test_engine_packed_excludes_padded():
    st, ge = _engine()
    z = torch.zeros(B, 512, device=DEV)
    rows = torch.zeros(16, 512, device=DEV)
    off = torch.tensor([0, 3, 12], dtype=torch.int32, device=DEV)
    with pytest.raises(AssertionError):
        ge.forward(z, z, None, train=False, save=False, text_rows=rows, row_off=off, lk_max=32,
                   text_tokens=torch.zeros(B, L, 512, device=DEV))
