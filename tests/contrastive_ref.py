"""fp64 torch restatement of the contrastive CLIP loss (include/moegan_hip.h, mg_clip_contrast), shared by the
clip_contrast tests.

f [B, C] image features, t [N, C] caption features (constants), row i's positive is column pos_off + i:
  s_ij = <f_i / |f_i|, t_j / |t_j|> / tau
  column j live iff |t_j| is finite and non-zero; row i live iff |f_i| is finite and non-zero and its positive is live
  loss = (1 / B) sum_{live i} [ logsumexp_{live j} s_ij - s_{i, pos(i)} ]
The reference gradient is autograd's; ``analytic_grad`` is the closed form the kernel implements."""
import torch


def _masks(f, t, pos_off):
    B = f.shape[0]
    nf, nt = f.norm(dim=1), t.norm(dim=1)
    col = torch.isfinite(nt) & (nt != 0)
    row = torch.isfinite(nf) & (nf != 0) & col[pos_off:pos_off + B]
    return row, col


def _logits(f, t, tau, row, col):
    """s over safe stand-ins for the dead rows / columns (their entries never reach a sum that is kept)."""
    fs = torch.where(row[:, None], f, torch.ones_like(f))
    ts = torch.where(col[:, None], t, torch.ones_like(t))
    fh = fs / fs.norm(dim=1, keepdim=True)
    th = ts / ts.norm(dim=1, keepdim=True)
    return fh @ th.T / tau, fh, th


def loss(f, t, tau, pos_off=0):
    """The loss as a differentiable fp64 scalar (whatever the dtype of f / t)."""
    f, t = f.double(), t.double().detach()
    B = f.shape[0]
    row, col = _masks(f.detach(), t, pos_off)
    s, _, _ = _logits(f, t, tau, row, col)
    s = s.masked_fill(~col[None, :], float("-inf"))
    lse = torch.logsumexp(s, dim=1)
    pos = s[torch.arange(B), pos_off + torch.arange(B, device=f.device)]
    per = torch.where(row, lse - torch.where(row, pos, torch.zeros_like(pos)), torch.zeros_like(lse))
    return per.sum() / B


def loss_and_grad(f, t, tau, scale=1.0, pos_off=0):
    """(loss, scale * d loss / d f) in fp64, the gradient by autograd."""
    x = f.detach().double().clone()
    bad = ~torch.isfinite(x).all(dim=1)
    x[bad] = 0.0  # a non-finite row is dead whatever it holds; autograd must not see inf - inf
    x.requires_grad_(True)
    l = loss(x, t, tau, pos_off)
    if l.requires_grad:
        (g,) = torch.autograd.grad(l, x)
    else:
        g = torch.zeros_like(x)
    return l.detach(), torch.nan_to_num(g) * scale


def analytic_grad(f, t, tau, scale=1.0, pos_off=0):
    """g_f[i] = scale / (B tau) (I - f^ f^T) / |f_i| (sum_{live j} p_ij t^_j - t^_pos(i)); zero rows where dead."""
    f, t = f.double(), t.double()
    B = f.shape[0]
    row, col = _masks(f, t, pos_off)
    s, fh, th = _logits(f, t, tau, row, col)
    p = torch.softmax(s.masked_fill(~col[None, :], float("-inf")), dim=1)
    delta = torch.zeros_like(p)
    delta[torch.arange(B), pos_off + torch.arange(B, device=f.device)] = 1.0
    u = (p - delta) @ torch.where(col[:, None], th, torch.zeros_like(th))
    fn = torch.where(row, f.norm(dim=1), torch.ones(B, dtype=f.dtype, device=f.device))
    g = scale / (B * tau) * (u - fh * (u * fh).sum(dim=1, keepdim=True)) / fn[:, None]
    return torch.where(row[:, None], g, torch.zeros_like(g))
