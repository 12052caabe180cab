"""Checkpoint + prompt -> PNG: the reference's sampling entry point (moegan/generate_images.py) on the MI355X path.

The reference's five flags (``--checkpoint --prompt --num_samples --output_dir --truncation_psi``) and its output:
the samples side by side in one row, saved as ``<prompt with spaces as underscores>.png`` under ``--output_dir``.

This build's extras:
  * ``--ema``: sample the averaged weights (``generator_ema``, written when training ran with ``--ema_kimg``); a
    file without them gives a warning and the live weights;
  * ``--clip_weights`` / ``--bpe``: a local OpenAI CLIP file and its merges file, so the prompt is encoded here
    (t2i_moe_gan.load_clip_weights); ``--prompt_tokens`` also feeds the prompt's token features to the cross-attention;
  * ``--text_embedding FILE.npy``: a pooled [512] or [1, 512] embedding used in place of encoding the prompt (the
    prompt then only names the output file), so no CLIP weights are needed;
  * ``--num_experts --topk --dtype --max_resolution``: the configuration the checkpoint was trained with;
    ``--seed``: the latent draw.

The checkpoint may be a resume file, a model-only file ({'generator', 'discriminator'}) or a bare generator state
dict -- the three shapes checkpoint.load_resume accepts.
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def parse_args(argv=None):
    p = argparse.ArgumentParser(description="Generate images with Aurora GAN-MoE (MI355X)")
    p.add_argument("--checkpoint", type=str, required=True, help="Path to checkpoint file")
    p.add_argument("--prompt", type=str, required=True, help="Text prompt for image generation")
    p.add_argument("--num_samples", type=int, default=4, help="Number of samples to generate")
    p.add_argument("--output_dir", type=str, default="./generated_images", help="Directory to save generated images")
    p.add_argument("--truncation_psi", type=float, default=0.7,
                   help="Truncation psi parameter (lower = better quality, less diversity)")
    # MI355X extras
    p.add_argument("--ema", action="store_true",
                   help="sample the averaged generator ('generator_ema'); falls back to 'generator' with a warning")
    p.add_argument("--clip_weights", type=str, default=None,
                   help="local OpenAI CLIP state_dict / safetensors with the text tower: encodes the prompt")
    p.add_argument("--bpe", type=str, default=None, help="CLIP's merges file (with --clip_weights)")
    p.add_argument("--prompt_tokens", action="store_true",
                   help="feed the prompt's per-token features to the cross-attention too (needs --clip_weights --bpe)")
    p.add_argument("--text_embedding", type=str, default=None,
                   help=".npy with a pooled [512] / [1, 512] text embedding, used instead of encoding the prompt")
    p.add_argument("--num_experts", type=int, default=4)
    p.add_argument("--topk", type=int, default=None, help="sparse top-k routing (default: dense soft combine)")
    p.add_argument("--dtype", choices=["fp32", "bf16"], default="fp32")
    p.add_argument("--max_resolution", type=int, default=16, choices=[16, 32, 64, 128])
    p.add_argument("--attn_resolution", type=int, default=None, choices=[16, 32],
                   help="the attn_resolution the checkpoint was trained with (default: read from its keys)")
    p.add_argument("--seed", type=int, default=None, help="seed of the latent draw (default: unseeded)")
    args = p.parse_args(argv)
    if args.prompt_tokens and args.text_embedding:
        p.error("--prompt_tokens encodes the prompt itself: it cannot be combined with --text_embedding")
    if args.prompt_tokens and not (args.clip_weights and args.bpe):
        p.error("--prompt_tokens needs --clip_weights and --bpe")
    if args.num_samples < 1:
        p.error("--num_samples must be at least 1")
    return args


def generator_state(ck, ema=False):
    """The generator state dict of a loaded checkpoint in any of the three accepted shapes; with ``ema`` the averaged
    weights when the file has them."""
    if "generator" not in ck:  # bare generator state dict
        if ema:
            print("Warning: the checkpoint is a bare state dict without 'generator_ema'; using it as is")
        return ck
    if ema:
        if "generator_ema" in ck:
            return ck["generator_ema"]
        print("Warning: the checkpoint has no 'generator_ema'; using 'generator'")
    return ck["generator"]


def text_features(args, M, device):
    """(pooled [1, 512], tokens or None, text_len or None) for the prompt."""
    if args.text_embedding:
        e = np.load(args.text_embedding)
        if e.shape not in ((512,), (1, 512)):
            raise SystemExit(f"--text_embedding: expected a [512] or [1, 512] array, got {list(e.shape)}")
        return torch.from_numpy(np.asarray(e, dtype=np.float32)).reshape(1, 512), None, None
    if not args.clip_weights:
        raise SystemExit("encoding the prompt needs --clip_weights (and --bpe), or pass --text_embedding FILE.npy")
    M.load_clip_weights(args.clip_weights, device, bpe_path=args.bpe)
    if args.prompt_tokens:
        return M.encode_prompt(args.prompt)
    return M.encode_text_with_clip(args.prompt), None, None


def save_row(images, path):
    """[N, 3, H, W] in [-1, 1] -> one row of N titled panels, 4 x 4 inches each."""
    import matplotlib
    matplotlib.use("Agg")
    import matplotlib.pyplot as plt
    rgb = np.clip((images.detach().float().cpu().numpy().transpose(0, 2, 3, 1) + 1.0) / 2.0, 0.0, 1.0)
    n = rgb.shape[0]
    fig, axes = plt.subplots(1, n, figsize=(4 * n, 4), squeeze=False)
    for i in range(n):
        axes[0][i].imshow(rgb[i])
        axes[0][i].set_title(f"Sample {i + 1}")
        axes[0][i].axis("off")
    fig.tight_layout()
    fig.savefig(path)
    plt.close(fig)


def main(argv=None):
    args = parse_args(argv)
    import t2i_moe_gan as M
    device = M.DEVICE
    os.makedirs(args.output_dir, exist_ok=True)
    ck = torch.load(args.checkpoint, map_location="cpu", weights_only=True)
    if args.attn_resolution is None:  # inferred from the checkpoint's keys (layout.attn_res_of)
        from moegan_mi.layout import attn_res_of
        args.attn_resolution = attn_res_of(generator_state(ck, args.ema))
    generator = M.AuroraGenerator(max_resolution=args.max_resolution, attn_resolution=args.attn_resolution,
                                  num_experts=args.num_experts, topk=args.topk,
                                  dtype=args.dtype).to(device)
    generator.load_state_dict(generator_state(ck, args.ema))
    pooled, tokens, text_len = text_features(args, M, device)
    if args.seed is not None:
        torch.manual_seed(args.seed)
    images = M.sample_aurora_gan(generator, pooled, num_samples=args.num_samples,
                                 truncation_psi=args.truncation_psi, device=device, text_tokens=tokens,
                                 text_len=text_len)
    out = os.path.join(args.output_dir, args.prompt.replace(" ", "_") + ".png")
    save_row(images, out)
    print(f"Generated {args.num_samples} images for prompt: '{args.prompt}'")
    print(f"Saved to {out}")
    return out


if __name__ == "__main__":
    main()
