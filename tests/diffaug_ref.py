"""Independent fp64 torch restatement of the augmentation map T and its transpose (include/moegan_hip.h,
moegan_mi/augment.py), written from the formulas, for the tests of csrc/mg_augment.hip and its wiring.

Images are NCHW [B, 3, H, H]; ``u`` is fp32 [B, 8]; ``mask`` the policy bits (1 brightness, 2 saturation, 4 contrast,
8 translation, 16 cutout).  The integers (shift, cutout origin) are derived in fp32 -- one fp32 product, floor -- so
they are the kernel's; everything else is fp64."""
import torch


def geometry(u_row, H, mask):
    """(tx, ty, (r0, r1, c0, c1)): the shift and the clipped cutout rows / columns of one image."""
    u_row = u_row.detach().cpu().float()
    tx = ty = 0
    box = (0, 0, 0, 0)
    if mask & 8:
        r = round(H / 8)  # ties to even
        n = torch.tensor(float(2 * r + 1), dtype=torch.float32)
        tx = int(torch.floor(u_row[3] * n)) - r
        ty = int(torch.floor(u_row[4] * n)) - r
    if mask & 16:
        s = H // 2
        n = torch.tensor(float(H + 1 - s % 2), dtype=torch.float32)
        ox = int(torch.floor(u_row[5] * n))
        oy = int(torch.floor(u_row[6] * n))
        clip = lambda v: min(max(v, 0), H)  # noqa: E731
        box = (clip(oy - s // 2), clip(oy - s // 2 + s), clip(ox - s // 2), clip(ox - s // 2 + s))
    return tx, ty, box


def _shift(y, ty, tx):
    """z[:, i, j] = y[:, i + ty, j + tx], zero where the source is outside."""
    H = y.shape[-1]
    z = torch.zeros_like(y)
    i0, i1 = max(0, -ty), min(H, H - ty)
    j0, j1 = max(0, -tx), min(H, H - tx)
    if i1 > i0 and j1 > j0:
        z[:, i0:i1, j0:j1] = y[:, i0 + ty:i1 + ty, j0 + tx:j1 + tx]
    return z


def forward(x, u, mask):
    """T(x), float64 [B, 3, H, H] on the CPU."""
    x = x.detach().cpu().double()
    u = u.detach().cpu().float()
    ud = u.double()
    B, _, H, _ = x.shape
    out = torch.empty_like(x)
    for b in range(B):
        y = x[b].clone()
        if mask & 1:
            y = y + (ud[b, 0] - 0.5)
        if mask & 2:
            m = y.mean(dim=0, keepdim=True)
            y = (y - m) * (2.0 * ud[b, 1]) + m
        if mask & 4:
            M = y.mean()
            y = (y - M) * (ud[b, 2] + 0.5) + M
        tx, ty, (r0, r1, c0, c1) = geometry(u[b], H, mask)
        if mask & 8:
            y = _shift(y, ty, tx)
        if mask & 16:
            y = y.clone()
            y[:, r0:r1, c0:c1] = 0.0
        out[b] = y
    return out


def transpose(g, u, mask):
    """T^T g (the linear part's transpose), float64 [B, 3, H, H] on the CPU."""
    g = g.detach().cpu().double()
    u = u.detach().cpu().float()
    ud = u.double()
    B, _, H, _ = g.shape
    out = torch.empty_like(g)
    for b in range(B):
        y = g[b].clone()
        tx, ty, (r0, r1, c0, c1) = geometry(u[b], H, mask)
        if mask & 16:
            y[:, r0:r1, c0:c1] = 0.0
        if mask & 8:
            y = _shift(y, -ty, -tx)
        if mask & 4:
            c = ud[b, 2] + 0.5
            y = c * y + (1.0 - c) * y.mean()
        if mask & 2:
            s = 2.0 * ud[b, 1]
            y = s * y + (1.0 - s) * y.mean(dim=0, keepdim=True)
        out[b] = y
    return out


def to_nhwc(x_nchw, ld, dtype=torch.float32, device="cuda"):
    """NCHW [B, 3, H, H] -> NHWC [B, H, H, ld] with zero pad channels."""
    B, _, H, _ = x_nchw.shape
    out = torch.zeros(B, H, H, ld, dtype=dtype, device=device)
    out[..., :3] = x_nchw.permute(0, 2, 3, 1).to(device=device, dtype=dtype)
    return out


def to_nchw(x_nhwc):
    return x_nhwc[..., :3].permute(0, 3, 1, 2).detach().cpu().double()
