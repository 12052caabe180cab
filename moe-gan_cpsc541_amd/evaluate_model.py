"""Checkpoint + validation set -> KID / CLIP score / R-precision over CLIP image features, as one JSON object.

This build's extension (the reference has no evaluation entry point).  The metrics are those of
moegan_mi/evaluate.py: the generator draws one image per validation caption in eval mode; real and generated images
go through the image tower of ``--clip_weights``; ``kid_clip`` compares the two feature sets, ``clip_score`` and
``r_precision`` compare each generated image with its caption's pooled embedding.

  python evaluate_model.py --checkpoint CK --val_images IMAGES.npy --val_embeddings TEXT.npy --clip_weights W
                           [--ema] [--num_samples N] [--truncation_psi P] [--seed S] [--group G] [--batch_size B]
                           [--nearest_k K] [--frechet] [--reference_stats FILE] [--save_stats FILE]
                           [--num_experts E --topk K --dtype fp32|bf16 --max_resolution R]

Prints {"kid_clip": ..., "clip_score": ..., "r_precision": ..., "r_precision_n": ..., "n": ...}; r_precision is NaN
when fewer than ``--group`` samples were evaluated.  ``--nearest_k K`` adds "precision", "recall", "density",
"coverage" (improved precision / recall and density / coverage between the two feature sets) and "nearest_k".
``--frechet`` adds "fd_clip", the Fréchet distance between the generated and the validation images' features;
``--reference_stats FILE`` measures it against the mean and covariance of an .npz with 'mu' and 'sigma' (the
reference's reference_stats.npz layout, made with the same tower) instead, and ``--save_stats FILE`` writes the
validation images' 'mu' / 'sigma' / 'n' in that layout; both imply ``--frechet``.  The checkpoint may be any of the shapes generate_images.py takes.
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def parse_args(argv=None):
    p = argparse.ArgumentParser(description="Evaluate an Aurora GAN-MoE checkpoint over CLIP features (MI355X)")
    p.add_argument("--checkpoint", type=str, required=True, help="Path to checkpoint file")
    p.add_argument("--val_images", type=str, required=True, help=".npy of validation images [N, 3, H, W] in [-1, 1]")
    p.add_argument("--val_embeddings", type=str, required=True, help=".npy of their pooled text embeddings [N, 512]")
    p.add_argument("--clip_weights", type=str, required=True,
                   help="local OpenAI CLIP state_dict / safetensors with the image tower")
    p.add_argument("--ema", action="store_true",
                   help="evaluate the averaged generator ('generator_ema'); falls back to 'generator' with a warning")
    p.add_argument("--num_samples", type=int, default=None, help="evaluate at most this many samples (default: all)")
    p.add_argument("--truncation_psi", type=float, default=1.0)
    p.add_argument("--seed", type=int, default=0, help="seed of the latent draws")
    p.add_argument("--group", type=int, default=100, help="R-precision: captions per retrieval group (1 to 128)")
    p.add_argument("--nearest_k", type=int, default=None,
                   help="also improved precision / recall and density / coverage with K nearest neighbours "
                        "(1 to 16, below the number of samples; default: off)")
    p.add_argument("--frechet", action="store_true",
                   help="also the Fréchet distance between the generated and the validation images' features")
    p.add_argument("--reference_stats", type=str, default=None,
                   help="measure the Fréchet distance against this .npz of 'mu' and 'sigma' instead (implies --frechet)")
    p.add_argument("--save_stats", type=str, default=None,
                   help="write the validation images' 'mu' / 'sigma' / 'n' to this .npz (implies --frechet)")
    p.add_argument("--batch_size", type=int, default=64)
    p.add_argument("--num_experts", type=int, default=4)
    p.add_argument("--topk", type=int, default=None, help="sparse top-k routing (default: dense soft combine)")
    p.add_argument("--dtype", choices=["fp32", "bf16"], default="fp32")
    p.add_argument("--max_resolution", type=int, default=16, choices=[16, 32, 64, 128])
    p.add_argument("--attn_resolution", type=int, default=None, choices=[16, 32],
                   help="the attn_resolution the checkpoint was trained with (default: read from its keys)")
    args = p.parse_args(argv)
    if not 1 <= args.group <= 128:
        p.error("--group must be between 1 and 128")
    if args.num_samples is not None and args.num_samples < 2:
        p.error("--num_samples must be at least 2")
    if args.nearest_k is not None and not 1 <= args.nearest_k <= 16:
        p.error("--nearest_k must be between 1 and 16")
    if args.reference_stats or args.save_stats:
        args.frechet = True
    return args


def main(argv=None):
    args = parse_args(argv)
    import t2i_moe_gan as M
    from generate_images import generator_state
    from torch.utils.data import DataLoader
    from train_model import ProcessedMSCOCODataset
    device = M.DEVICE
    ck = torch.load(args.checkpoint, map_location="cpu", weights_only=True)
    if args.attn_resolution is None:  # inferred from the checkpoint's keys (layout.attn_res_of)
        from moegan_mi.layout import attn_res_of
        args.attn_resolution = attn_res_of(generator_state(ck, args.ema))
    generator = M.AuroraGenerator(max_resolution=args.max_resolution, attn_resolution=args.attn_resolution,
                                  num_experts=args.num_experts, topk=args.topk,
                                  dtype=args.dtype).to(device)
    generator.load_state_dict(generator_state(ck, args.ema))
    M.load_clip_weights(args.clip_weights, device)
    loader = DataLoader(ProcessedMSCOCODataset(args.val_images, args.val_embeddings), batch_size=args.batch_size,
                        shuffle=False)
    kw = {}
    if args.frechet:
        kw = dict(frechet=True, reference_stats=args.reference_stats, return_features=bool(args.save_stats))
    m = M.evaluate_aurora_gan(generator, loader, num_samples=args.num_samples, truncation_psi=args.truncation_psi,
                              seed=args.seed, group=args.group, nearest_k=args.nearest_k, **kw)
    if args.save_stats:
        from moegan_mi.evaluate import FeatureMoments
        m, feats = m
        FeatureMoments(feats["real"].shape[1], feats["real"].device).update(feats["real"]).save(args.save_stats)
    print(json.dumps(m))
    return m


if __name__ == "__main__":
    main()
