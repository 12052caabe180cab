"""Wiring of the augmentation into the discriminator engine (fp32 mode, B = 4, reals 64 x 64, fakes 16 x 16): the
existing un-augmented phases are the yardstick.  ``d_phase`` / ``g_phase`` with ``aug_*`` must give what the plain
phases give on images pre-transformed by the fp64 reference (tests/diffaug_ref.py), and the G phase's image gradient
must be the reference's T^T of the plain one; tolerance 1e-4 relative, the project's fp32 step tolerance."""
import pytest
import torch

import diffaug_ref as R
from goldens import close
from oracle.recipe import fill_state

pytestmark = pytest.mark.gpu
DEV = "cuda"
B, MASK = 4, 31


def _engine():
    from moegan_mi.engine_d import DiscriminatorEngine
    from moegan_mi.layout import discriminator_shapes
    from moegan_mi.params import ParamStore
    st = ParamStore(discriminator_shapes(), DEV)
    st.load_state_dict({k: torch.from_numpy(v) for k, v in fill_state(discriminator_shapes(), 50).items()})
    de = DiscriminatorEngine(st)
    de.prep()
    return st, de


def _inputs():
    g = torch.Generator().manual_seed(21)
    real = torch.rand(B, 3, 64, 64, generator=g) * 2 - 1
    fake = torch.rand(B, 3, 16, 16, generator=g) * 2 - 1
    text = torch.randn(B, 512, generator=g)
    perm = torch.tensor([2, 0, 3, 1], dtype=torch.int32)
    aug = torch.rand(3, B, 8, generator=g)
    return real, fake, text, perm, aug


def test_d_phase_matches_plain_phase_on_transformed_images():
    st, de = _engine()
    real, fake, text, perm, aug = _inputs()
    text_d, perm_d, aug_d = text.to(DEV), perm.to(DEV), aug.to(DEV)

    def run(real_nchw, fake_nchw, **kw):
        st.zero_grad()
        res = de.d_phase(real_nchw.float().to(DEV), text_d, R.to_nhwc(fake_nchw.float(), 8), ("nhwc", 8), perm_d, 10.0,
                         **kw)
        torch.cuda.synchronize()
        return {k: v.clone() for k, v in res.items()}, {n: st.gview(n).clone() for n in st.offsets}

    got, got_g = run(real, fake, aug_real=aug_d[0], aug_fake=aug_d[1], aug_mask=MASK)
    want, want_g = run(R.forward(real, aug[0], MASK), R.forward(fake, aug[1], MASK))
    plain, _ = run(real, fake)
    # the augmentation is live: the plain phase on the untransformed images gives another loss
    assert abs(float(plain["losses"][0]) - float(want["losses"][0])) > 1e-3 * abs(float(want["losses"][0]))
    for k in ("losses", "r1", "real_pred", "mism_pred", "fake_pred"):
        close(got[k], want[k].cpu().double(), rtol=1e-4, atol=1e-7, what=k)
    # R1 is taken at the discriminator's input, the augmented real
    close(got["r1_grad"], want["r1_grad"].cpu().double(), rtol=1e-4, atol=1e-9, what="r1_grad")
    for n in st.offsets:
        close(got_g[n], want_g[n].cpu().double(), rtol=1e-4, atol=1e-9, what="grad " + n)


def test_g_phase_loss_and_image_gradient():
    st, de = _engine()
    real, fake, text, perm, aug = _inputs()
    text_d, aug_d = text.to(DEV), aug.to(DEV)
    fake_d = R.to_nhwc(fake, 8)
    loss, pred, g_img = de.g_phase(fake_d, ("nhwc", 8), text_d, aug_fake=aug_d[2], aug_mask=MASK)
    loss_p, pred_p, g_plain = de.g_phase(R.to_nhwc(R.forward(fake, aug[2], MASK).float(), 8), ("nhwc", 8), text_d)
    torch.cuda.synchronize()
    close(loss, loss_p.cpu().double(), rtol=1e-4, atol=1e-7, what="g loss")
    close(pred, pred_p.cpu().double(), rtol=1e-4, atol=1e-7, what="fake_pred")
    assert g_img.shape == fake_d.shape and g_img.dtype == fake_d.dtype
    assert torch.count_nonzero(g_img[..., 3:]) == 0
    want = R.transpose(R.to_nchw(g_plain), aug[2], MASK)
    close(R.to_nchw(g_img), want, rtol=1e-4, atol=1e-12, what="g_img")
    # ... and it is not the plain gradient
    assert float((R.to_nchw(g_img) - R.to_nchw(g_plain)).abs().max()) > 1e-3 * float(want.abs().max())


def test_phases_without_aug_launch_nothing_new():
    """aug_* left out: the phases make no augmentation call (the default step is the step it was)."""
    from moegan_mi import _lib as L
    st, de = _engine()
    real, fake, text, perm, aug = _inputs()
    seen = []

    def hook(name, args, run):
        seen.append(name)
        return run()
    L.HOOK = hook
    try:
        de.d_phase(real.to(DEV), text.to(DEV), R.to_nhwc(fake, 8), ("nhwc", 8), perm.to(DEV), 10.0)
        de.g_phase(R.to_nhwc(fake, 8), ("nhwc", 8), text.to(DEV))
        plain = list(seen)
        del seen[:]
        de.d_phase(real.to(DEV), text.to(DEV), R.to_nhwc(fake, 8), ("nhwc", 8), perm.to(DEV), 10.0,
                   aug_real=aug[0].to(DEV), aug_fake=aug[1].to(DEV), aug_mask=MASK)
        de.g_phase(R.to_nhwc(fake, 8), ("nhwc", 8), text.to(DEV), aug_fake=aug[2].to(DEV), aug_mask=MASK)
    finally:
        L.HOOK = None
    torch.cuda.synchronize()
    assert not [n for n in plain if "diffaug" in n]
    # one launch per direction for the whole batch: real + fake forward in the D phase, forward + transpose in the G
    assert [n for n in seen if "diffaug" in n] == ["mg_diffaug_fwd", "mg_diffaug_fwd", "mg_diffaug_fwd",
                                                  "mg_diffaug_bwd"]
    assert [n for n in seen if "diffaug" not in n] == plain
