"""Differentiable augmentation of the discriminator's inputs (Zhao et al., "Differentiable Augmentation for
Data-Efficient GAN Training"; this build's extension, the reference has none).

The same random transform family T goes on every image the discriminator sees, real and fake, and the generator's
gradient flows back through it.  T is per image and affine, fixed by one row u[0..7] of uniforms in [0, 1):
brightness, saturation and contrast (policy ``color``), an integer shift by up to H / 8 pixels (``translation``) and a
zeroed H / 2 square (``cutout``); include/moegan_hip.h states the formulas.  Both directions are HIP kernels
(csrc/mg_augment.hip): ``ops.diffaug_fwd`` / ``ops.diffaug_bwd``.

The parameters are an explicit input everywhere (``TrainStep.step(aug=...)``), so a step is a function of its
arguments; ``draw`` makes them from a torch generator.
"""
import torch

from . import ops

BRIGHTNESS, SATURATION, CONTRAST, TRANSLATION, CUTOUT = 1, 2, 4, 8, 16
POLICY_BITS = {"color": BRIGHTNESS | SATURATION | CONTRAST, "translation": TRANSLATION, "cutout": CUTOUT}
N_PARAMS = 8  # u0 brightness, u1 saturation, u2 contrast, u3 / u4 shift x / y, u5 / u6 cutout x / y, u7 unused
# rows of a step's ``aug`` [3, B, 8]
ROW_D_REAL, ROW_D_FAKE, ROW_G_FAKE = 0, 1, 2


def parse_policy(policy):
    """Bit mask of a policy string: any comma-separated subset of ``color,translation,cutout`` ('' or None: 0, no
    augmentation).  An unknown name raises ValueError."""
    if policy is None:
        return 0
    if not isinstance(policy, str):
        raise ValueError(f"diffaug policy must be a string such as 'color,translation,cutout', got {policy!r}")
    mask = 0
    for name in (p.strip() for p in policy.split(",")):
        if not name:
            continue
        if name not in POLICY_BITS:
            raise ValueError(f"unknown diffaug policy {name!r}: expected a comma-separated subset of "
                             f"{','.join(POLICY_BITS)}")
        mask |= POLICY_BITS[name]
    return mask


def draw(B, generator=None, device=None):
    """A step's augmentation parameters: fp32 uniforms in [0, 1), [3, B, 8] (row 0: the real batch of the D phase,
    row 1: its fakes, row 2: the fakes of the G phase), on ``generator``'s device (or ``device``)."""
    if device is None:
        device = generator.device if generator is not None else "cpu"
    return torch.rand(3, int(B), N_PARAMS, device=device, dtype=torch.float32, generator=generator)


def _mask_of(policy):
    return int(policy) if isinstance(policy, int) else parse_policy(policy)


class _DiffAugment(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, u, mask):
        B, C, H, W = x.shape
        u = u.to(x.device, torch.float32).contiguous()
        xs = x.detach()
        if xs.dtype not in (torch.float32, torch.bfloat16):
            xs = xs.float()
        sb, sc, sh, sw = xs.stride()
        y = ops.diffaug_fwd(xs, (sb, sh, sw, sc), B, H, u, mask, 4, torch.float32)
        ctx.save_for_backward(u)
        ctx.mask, ctx.in_dtype = mask, x.dtype
        return y[..., :3].permute(0, 3, 1, 2).to(x.dtype)

    @staticmethod
    def backward(ctx, gy):
        (u,) = ctx.saved_tensors
        B, _, H, _ = gy.shape
        g = torch.zeros(B, H, H, 4, device=gy.device, dtype=torch.float32)
        g[..., :3] = gy.detach().float().permute(0, 2, 3, 1)
        gx = ops.diffaug_bwd(g, u, ctx.mask)
        return gx[..., :3].permute(0, 3, 1, 2).to(ctx.in_dtype), None, None


def DiffAugment(x, u, policy):
    """T(x) for images x [B, 3, H, H] (NCHW, any strides, on a HIP device) with parameters u [B, 8] and ``policy`` (a
    policy string or its bit mask), differentiable in x: for use outside the training step.  Returns [B, 3, H, H]
    (a channels-last view) in x's dtype."""
    if x.dim() != 4 or x.shape[1] != 3 or x.shape[2] != x.shape[3]:
        raise ValueError(f"DiffAugment takes square 3-channel NCHW images, got {tuple(x.shape)}")
    if x.device.type != "cuda":
        raise RuntimeError("DiffAugment runs on the HIP device only (there is no CPU path)")
    if tuple(u.shape) != (x.shape[0], N_PARAMS):
        raise ValueError(f"u must be [{x.shape[0]}, {N_PARAMS}], got {tuple(u.shape)}")
    if min(x.stride()) <= 0:
        x = x.contiguous()
    return _DiffAugment.apply(x, u, _mask_of(policy))
