"""The bf16 engine with attn_res = 32 (R = 32, B = 4, E = 8 top-2, the device's routes and LeakyReLU slopes replayed)
against the fp64 composition of tests/test_attn32_engine_gpu.py: the relative L2 error of every attention block's
output and of its parameter gradients (all ``<block>.attn_block.*`` gradients as one vector).

Bar: gen_block_32's figures stay within 4x gen_block_16's, measured in the same run.  gen_block_16 is existing code
at the same C = 128 on the same kernels except the self-attention; the new block has four times the keys per softmax
row and four times the tokens per per-image sum, so error growing faster than linearly in that count is a defect.

Measured (one MI355X; also in DESIGN.md section 4, "Long-sequence self-attention"), blocks 4 / 8 / 16 / 32:
  block output        6.49e-3  7.84e-3  9.20e-3  9.94e-3    ratio 32 / 16: 1.08
  attn_block grads    1.82e-2  1.61e-2  1.53e-2  1.43e-2    ratio 32 / 16: 0.93"""
import pytest
import torch

from oracle.recipe import fill_state
from steputil import lrelu_slope_replay
from test_attn32_engine_gpu import _nhwc_pad, generator_attn32

pytestmark = pytest.mark.gpu
DEV = "cuda"
torch.set_num_threads(8)


def rel_l2(a, e):
    a, e = a.detach().double().cpu().reshape(-1), e.detach().double().cpu().reshape(-1)
    return float((a - e).norm() / e.norm())


def test_attn32_bf16_error_growth():
    from moegan_mi.engine_g import GeneratorEngine
    from moegan_mi.layout import frozen_rgb_prefixes, generator_shapes
    from moegan_mi.params import ParamStore
    R, B, E, k = 32, 4, 8, 2
    shapes = generator_shapes(E, R, attn_res=32)
    vals = fill_state(shapes, 0)
    st = ParamStore(shapes, DEV, frozen_prefixes=frozen_rgb_prefixes(R), shadow_dtype=torch.bfloat16)
    st.load_state_dict({n: torch.from_numpy(v) for n, v in vals.items()})
    ge = GeneratorEngine(st, E, k, torch.bfloat16)
    ge.prep()
    g = torch.Generator().manual_seed(17)
    z, text = torch.randn(B, 512, generator=g), torch.randn(B, 512, generator=g)
    eps = [tuple(torch.randn(s, generator=g) for s in ((c, 128), (512, 128), (256, E))) for c in (512, 256, 128, 128)]
    epsd = [tuple(t.to(DEV) for t in trip) for trip in eps]
    outs = {}
    orig = ge.attn_fwd

    def spy(pre, x, *a, **kw):
        r = orig(pre, x, *a, **kw)
        outs[pre.split(".")[0]] = r[0]
        return r
    ge.attn_fwd = spy
    with lrelu_slope_replay() as slopes:
        im, ih, kl2s, pr, topis, ctx = ge.forward(z.to(DEV), text.to(DEV), epsd, 3.0, 0.7, train=True, save=True,
                                                  want_img8=True)
    P = {n: torch.from_numpy(v).double().requires_grad_(not n.split(".")[-1].startswith("epsilon_"))
         for n, v in vals.items()}
    feats = {}
    with slopes.oracle():
        img, img_half, kl, probs = generator_attn32(z.double(), text.double(), P,
                                                    [tuple(t.double() for t in e) for e in eps], True, 3.0, 0.7,
                                                    topk=k, routes=[t.long().cpu() for t in topis], feats_out=feats)
    R_img, R_half = torch.randn(img.shape, generator=g), torch.randn(img_half.shape, generator=g)
    ((img * R_img.double()).sum() + (img_half * R_half.double()).sum()).backward()
    ge.backward(ctx, _nhwc_pad(R_img).to(im.dtype), g_img8=_nhwc_pad(R_half).to(im.dtype))
    torch.cuda.synchronize()
    err_out, err_grad = {}, {}
    for res in (4, 8, 16, 32):
        name = f"gen_block_{res}"
        err_out[res] = rel_l2(outs[name].float().permute(0, 3, 1, 2), feats[res])
        names = [n for n, t in P.items() if n.startswith(name + ".attn_block.") and t.grad is not None]
        assert len(names) >= 20 + 4 * E
        err_grad[res] = rel_l2(torch.cat([st.gview(n).reshape(-1).float() for n in names]),
                               torch.cat([P[n].grad.reshape(-1) for n in names]))
    print("bf16 rel L2, block output:  " + "  ".join(f"{r}: {v:.3e}" for r, v in err_out.items()))
    print("bf16 rel L2, attn_block gradients:  " + "  ".join(f"{r}: {v:.3e}" for r, v in err_grad.items()))
    print(f"ratios 32 / 16: output {err_out[32] / err_out[16]:.2f}, gradients {err_grad[32] / err_grad[16]:.2f}")
    assert err_out[32] <= 4 * err_out[16], (err_out[32], err_out[16])
    assert err_grad[32] <= 4 * err_grad[16], (err_grad[32], err_grad[16])
