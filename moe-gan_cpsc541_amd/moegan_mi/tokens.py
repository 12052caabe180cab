"""Per-token text features in packed form: the host side of the generator's ragged text cross-attention.

``encode_captions --tokens`` writes ``PREFIX_text_tokens.npy`` (fp16 [N, 77, 512], rows past a caption's length are
padding) and ``PREFIX_text_len.npy`` (int32 [N]).  Training reads only the live rows: a batch's captions go back to
back into ``text_rows`` [rows, 512], image b at rows ``row_off[b] .. row_off[b+1]-1``.  Two buckets keep the number
of distinct shapes (and so of captured step variants) small:

  rows   = the live row total R rounded up to a multiple of 4*B (pad rows are zero),
  lk_max = the batch's longest caption rounded up to a multiple of 32 (the kernels' key-slot count, at most 128).
"""
import os

import numpy as np
import torch
from torch.utils.data import Dataset

TOKEN_DIM = 512
LK_LIMIT = 128  # mg_xattn_ragged_*: at most 128 keys per image


def bucket_rows(total, batch):
    """The live row total rounded up to a multiple of 4 * batch."""
    q = 4 * int(batch)
    return -(-int(total) // q) * q


def bucket_lk(longest):
    """The longest caption rounded up to a multiple of 32."""
    return -(-int(longest) // 32) * 32


def _clip_lens(lens, L, max_tokens):
    lens = np.asarray(lens).astype(np.int64).reshape(-1)
    if lens.size and int(lens.min()) < 1:
        raise ValueError(f"text length below 1 (min {int(lens.min())}): every caption needs at least one token")
    if lens.size and int(lens.max()) > L:
        raise ValueError(f"text length {int(lens.max())} exceeds the {L} token rows stored per caption")
    if max_tokens is not None:
        if int(max_tokens) < 1:
            raise ValueError("max_tokens must be at least 1")
        lens = np.minimum(lens, int(max_tokens))
    if lens.size and int(lens.max()) > LK_LIMIT:
        raise ValueError(f"captions of up to {int(lens.max())} tokens: the cross-attention takes at most {LK_LIMIT} "
                         f"(pass max_tokens)")
    return lens


def pack_tokens(tokens, lens, max_tokens=None, out=None):
    """Pack a right-padded host batch ``tokens`` [B, L, 512] with lengths ``lens`` [B] (each >= 1) into
    ``(text_rows [rows, 512], row_off int32 [B+1], lk_max)``; ``max_tokens`` keeps each caption's first rows only.
    ``out`` (a [>= rows, 512] array of the tokens' dtype) receives the rows in place of a fresh array."""
    tokens = np.asarray(tokens) if not isinstance(tokens, np.ndarray) else tokens
    B, L = tokens.shape[0], tokens.shape[1]
    lens = _clip_lens(lens, L, max_tokens)
    if lens.shape[0] != B:
        raise ValueError(f"{lens.shape[0]} lengths for {B} captions")
    row_off = np.zeros(B + 1, dtype=np.int32)
    np.cumsum(lens, out=row_off[1:])
    total = int(row_off[B])
    rows = bucket_rows(total, B)
    if out is None:
        out = np.empty((rows, tokens.shape[2]), dtype=tokens.dtype)
    text_rows = out[:rows]
    for b in range(B):  # only the live rows are read (a memory-mapped source touches nothing else)
        text_rows[row_off[b]:row_off[b + 1]] = tokens[b, :lens[b]]
    text_rows[total:] = 0
    return text_rows, row_off, bucket_lk(lens.max() if B else 1)


def token_files(embeddings_file):
    """``X_text_tokens.npy`` / ``X_text_len.npy`` beside ``X_text_embeddings.npy`` (encode_captions --tokens)."""
    suffix = "_text_embeddings.npy"
    base = embeddings_file[:-len(suffix)] if embeddings_file.endswith(suffix) else os.path.splitext(embeddings_file)[0]
    return base + "_text_tokens.npy", base + "_text_len.npy"


class ProcessedTokenDataset(Dataset):
    """(image, pooled text embedding, live token rows) triples, all memory-mapped: item i's token rows are the first
    ``len[i]`` (at most ``max_tokens``) of its [L, 512] block, so padding is never read from disk."""

    def __init__(self, images_file, text_embeddings_file, max_tokens=None):
        tok_f, len_f = token_files(text_embeddings_file)
        missing = [f for f in (tok_f, len_f) if not os.path.exists(f)]
        if missing:
            raise FileNotFoundError(
                f"--text_tokens needs the per-token text files beside {text_embeddings_file}: missing "
                f"{', '.join(missing)} (write them with `python -m moegan_mi.encode_captions --tokens`)")
        self.images = np.load(images_file, mmap_mode="r")
        self.text_embeddings = np.load(text_embeddings_file, mmap_mode="r")
        self.tokens = np.load(tok_f, mmap_mode="r")
        n = len(self.images)
        assert len(self.text_embeddings) == n, "Images and text embeddings count mismatch"
        if self.tokens.ndim != 3 or self.tokens.shape[0] != n or self.tokens.shape[2] != TOKEN_DIM:
            raise ValueError(f"{tok_f}: expected [{n}, L, {TOKEN_DIM}], found {tuple(self.tokens.shape)}")
        lens = np.load(len_f)
        if lens.shape != (n,):
            raise ValueError(f"{len_f}: expected [{n}] lengths, found {tuple(lens.shape)}")
        self.lens = _clip_lens(lens, self.tokens.shape[1], max_tokens)

    def __len__(self):
        return len(self.images)

    def __getitem__(self, idx):
        return (torch.from_numpy(np.array(self.images[idx])), torch.from_numpy(np.array(self.text_embeddings[idx])),
                torch.from_numpy(np.array(self.tokens[idx, :self.lens[idx]])))


def collate_tokens(samples):
    """Batch of ProcessedTokenDataset items -> (images, text, text_rows, row_off, lk_max): the live rows go back to
    back into one packed buffer; the DataLoader (pin_memory=True) pins that buffer alone and DevicePrefetcher moves
    it as it is, so the padding never crosses to the device."""
    images = torch.stack([s[0] for s in samples])
    text = torch.stack([s[1] for s in samples])
    B = len(samples)
    lens = np.array([s[2].shape[0] for s in samples], dtype=np.int64)
    row_off = np.zeros(B + 1, dtype=np.int32)
    np.cumsum(lens, out=row_off[1:])
    total, rows = int(row_off[B]), bucket_rows(int(row_off[B]), B)
    text_rows = torch.empty(rows, samples[0][2].shape[1], dtype=samples[0][2].dtype)
    torch.cat([s[2] for s in samples], out=text_rows[:total])
    text_rows[total:] = 0
    return images, text, text_rows, torch.from_numpy(row_off), bucket_lk(int(lens.max()))


def unpack_tokens(text_rows, row_off, lk_max):
    """Packed rows back to the padded module form: (text_tokens [B, lk_max, 512] with zero pad slots, text_len
    int64 [B] on the host).  For the paths that keep the padded API (validation through the generator module)."""
    off = row_off.detach().cpu().long()
    lens = off[1:] - off[:-1]
    slot = torch.arange(int(lk_max))
    live = (slot[None, :] < lens[:, None]).to(text_rows.device)
    idx = (off[:-1, None] + slot[None, :]).clamp_(max=text_rows.shape[0] - 1).to(text_rows.device)
    return text_rows[idx] * live[..., None].to(text_rows.dtype), lens
