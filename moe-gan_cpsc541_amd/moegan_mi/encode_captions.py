"""Caption-embedding step of the data pipeline on the project's own CLIP text tower.

    python -m moegan_mi.encode_captions --weights clip.pt --bpe bpe_simple_vocab_16e6.txt.gz \
        --captions captions.txt --out data/train [--batch 256] [--tokens]

Reads one caption per line and writes ``PREFIX_text_embeddings.npy`` (float32 [N, 512], the layout train_model.py's
dataset reads).  With ``--tokens`` also ``PREFIX_text_tokens.npy`` (float16 [N, context_length, 512], zero-padded)
and ``PREFIX_text_len.npy`` (int32 [N]): the per-token features AuroraGenerator.forward takes as ``text_tokens=`` /
``text_len=``.  Captions longer than the context are truncated (the end token kept), as a data pipeline must.
"""
import argparse

import numpy as np
import torch


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--weights", required=True, help="OpenAI CLIP state_dict (.pt) or .safetensors, local")
    ap.add_argument("--bpe", required=True, help="CLIP's BPE merges file (plain or .gz), local")
    ap.add_argument("--captions", required=True, help="text file, one caption per line")
    ap.add_argument("--out", required=True, help="output prefix")
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--tokens", action="store_true", help="also write per-token features and lengths")
    ap.add_argument("--device", default="cuda")
    args = ap.parse_args(argv)

    from .clip_bpe import ClipTokenizer
    from .clip_text import ClipTextEncoder
    tok = ClipTokenizer(args.bpe)
    enc = ClipTextEncoder.from_file(args.weights, device=args.device)
    if tok.vocab_size != enc.vocab_size:
        raise SystemExit(f"--bpe gives {tok.vocab_size} tokens, --weights {enc.vocab_size}")
    with open(args.captions, encoding="utf-8") as f:
        captions = [ln.rstrip("\n") for ln in f]
    if captions and captions[-1] == "":
        captions.pop()
    N, ctx, out = len(captions), enc.context_length, enc.output_dim
    emb = np.zeros((N, out), np.float32)
    toks = np.zeros((N, ctx, out), np.float16) if args.tokens else None
    lens = np.zeros(N, np.int32) if args.tokens else None
    for i in range(0, N, args.batch):
        ids = tok(captions[i:i + args.batch], ctx, truncate=True)
        if args.tokens:
            pooled, t, ln = enc.encode_text(ids, return_tokens=True)
            toks[i:i + len(ids), :t.shape[1]] = t.to(torch.float16).cpu().numpy()
            lens[i:i + len(ids)] = ln.cpu().numpy()
        else:
            pooled = enc.encode_text(ids)
        emb[i:i + len(ids)] = pooled.cpu().numpy()
    np.save(args.out + "_text_embeddings.npy", emb)
    if args.tokens:
        np.save(args.out + "_text_tokens.npy", toks)
        np.save(args.out + "_text_len.npy", lens)
    print(f"{N} captions -> {args.out}_text_embeddings.npy" + (" (+ tokens, len)" if args.tokens else ""))
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
