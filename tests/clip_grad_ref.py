"""Plain PyTorch restatement of the differentiable CLIP loss, shared by the clip_grad tests: clamp, bilinear resize to
the tower's resolution, OpenAI CLIP's VisionTransformer (as tests/test_clip_gpu.py::torch_vit restates it), cosine
loss -- differentiable with respect to the generator-style NHWC image; and the same gradient on the project's
kernels (tower_grads)."""
import torch
import torch.nn.functional as F


def vit(sd, img, heads):
    """OpenAI CLIP VisionTransformer forward on ``img`` [B, 3, res, res], in the dtype of ``sd`` / ``img``."""
    x = F.conv2d(img, sd["conv1.weight"], stride=sd["conv1.weight"].shape[-1])
    B, w = x.shape[:2]
    x = x.reshape(B, w, -1).permute(0, 2, 1)
    x = torch.cat([sd["class_embedding"].expand(B, 1, w), x], dim=1) + sd["positional_embedding"]
    x = F.layer_norm(x, (w,), sd["ln_pre.weight"], sd["ln_pre.bias"])
    i = 0
    while f"transformer.resblocks.{i}.ln_1.weight" in sd:
        p = f"transformer.resblocks.{i}."
        h = F.layer_norm(x, (w,), sd[p + "ln_1.weight"], sd[p + "ln_1.bias"])
        a, _ = F.multi_head_attention_forward(
            h.transpose(0, 1), h.transpose(0, 1), h.transpose(0, 1), w, heads, sd[p + "attn.in_proj_weight"],
            sd[p + "attn.in_proj_bias"], None, None, False, 0.0, sd[p + "attn.out_proj.weight"],
            sd[p + "attn.out_proj.bias"], need_weights=False)
        x = x + a.transpose(0, 1)
        h = F.layer_norm(x, (w,), sd[p + "ln_2.weight"], sd[p + "ln_2.bias"])
        h = F.linear(h, sd[p + "mlp.c_fc.weight"], sd[p + "mlp.c_fc.bias"])
        h = h * torch.sigmoid(1.702 * h)
        x = x + F.linear(h, sd[p + "mlp.c_proj.weight"], sd[p + "mlp.c_proj.bias"])
        i += 1
    return F.layer_norm(x[:, 0], (w,), sd["ln_post.weight"], sd["ln_post.bias"]) @ sd["proj"]


def cos_loss(f, t):
    f = f / f.norm(dim=-1, keepdim=True)
    t = t / t.norm(dim=-1, keepdim=True)
    return 1.0 - torch.nan_to_num((f * t).sum(dim=1)).mean()


def clip_loss_grads(sd, heads, imgs_nhwc, text, weights, res=224, dtype=torch.float32):
    """Gradients of sum_i weights[i] * L_clip(imgs_nhwc[i]) with respect to each NHWC image's channels 0..2
    ([B, R, R, 3] fp32) and the list of loss values; the tower runs in ``dtype`` (its weights and token rows), the
    clamp / resize and the loss in fp32."""
    sdd = {k: v.to(dtype) for k, v in sd.items()}
    leaves = [im[..., :3].detach().float().clone().requires_grad_(True) for im in imgs_nhwc]
    ups = []
    for x in leaves:
        im = torch.clamp(x.permute(0, 3, 1, 2), -1, 1)
        if im.shape[-1] != res:
            im = F.interpolate(im, size=(res, res), mode="bilinear", align_corners=False)
        ups.append(im)
    feats = vit(sdd, torch.cat(ups).to(dtype), heads).float()  # one pass over every image
    losses, r0 = [], 0
    for x in leaves:
        losses.append(cos_loss(feats[r0:r0 + x.shape[0]], text.float()))
        r0 += x.shape[0]
    sum(w * l for w, l in zip(weights, losses)).backward()
    return [x.grad for x in leaves], [l.detach() for l in losses]


def cos_rel(a, b):
    """(cosine, relative L2) of a against b, over all elements."""
    a, b = a.double().reshape(-1), b.double().reshape(-1)
    return float(a @ b / (a.norm() * b.norm())), float((a - b).norm() / b.norm())


def tower_grads(enc, imgs, text, weights):
    """The kernels' path: one 2B-image tower pass, mg_cos_loss per image set, the tower backward."""
    from moegan_mi import ops
    feats, ctx = enc.encode_generated(imgs, save=True)
    g_f = torch.empty_like(feats)
    one = torch.ones(1, device=feats.device)
    losses, r0 = [], 0
    for im in imgs:
        n = im.shape[0]
        loss, _ = ops.cos_loss(feats[r0:r0 + n], text, one, g_f=g_f[r0:r0 + n])
        losses.append(loss)
        r0 += n
    g_imgs = [torch.zeros_like(im) for im in imgs]
    enc.backward(ctx, g_f, g_imgs, alpha=weights, accumulate=[0] * len(imgs))
    return g_imgs, losses, feats
