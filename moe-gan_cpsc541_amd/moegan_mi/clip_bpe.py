"""CLIP's byte-level BPE tokenizer, reading a local merges file (``bpe_simple_vocab_16e6.txt`` or its ``.gz``).

Nothing is downloaded: the vocabulary is rebuilt from the merges file alone, in OpenAI CLIP's order -- the 256 byte
symbols, the same 256 with ``</w>`` appended, one entry per merge line (the pair joined), then ``<|startoftext|>``
and ``<|endoftext|>``.  The real file (first line a header, at most 48 894 merges taken) gives 49 408 entries with
start 49406 and end 49407; a short synthetic file gives ``512 + n_merges + 2``.

Text is cleaned as CLIP does (``ftfy.fix_text`` when ftfy is importable, ``html.unescape`` twice, whitespace runs
collapsed, lower-cased), split by CLIP's pattern (the ``regex`` module when importable, else an equivalent ``re``
pattern), and every word's UTF-8 bytes are merged lowest rank first.
"""
import gzip
import html
import os

import torch

MAX_MERGES = 49152 - 256 - 2  # 48 894: the slice of the real file CLIP uses
_PAT = r"<\|startoftext\|>|<\|endoftext\|>|'s|'t|'re|'ve|'m|'ll|'d|[\p{L}]+|[\p{N}]|[^\s\p{L}\p{N}]+"
_PAT_RE = r"<\|startoftext\|>|<\|endoftext\|>|'s|'t|'re|'ve|'m|'ll|'d|[^\W\d_]+|\d|(?:[^\s\w]|_)+"


def bytes_to_unicode():
    """byte -> printable unicode symbol: ``!..~``, ``¡..¬``, ``®..ÿ`` map to themselves, the rest to chr(256 + n)."""
    bs = list(range(ord("!"), ord("~") + 1)) + list(range(ord("¡"), ord("¬") + 1)) + list(range(ord("®"), ord("ÿ") + 1))
    cs = bs[:]
    n = 0
    for b in range(256):
        if b not in bs:
            bs.append(b)
            cs.append(256 + n)
            n += 1
    return dict(zip(bs, (chr(c) for c in cs)))


def _compile_pattern():
    try:
        import regex
        return regex.compile(_PAT, regex.IGNORECASE)
    except ImportError:
        import re
        return re.compile(_PAT_RE, re.IGNORECASE)


def _clean(text):
    try:
        import ftfy
        text = ftfy.fix_text(text)
    except ImportError:
        pass
    text = html.unescape(html.unescape(text)).strip()
    return " ".join(text.split()).lower()


class ClipTokenizer:
    def __init__(self, merges_path):
        if merges_path is None or not os.path.exists(str(merges_path)):
            raise FileNotFoundError(f"ClipTokenizer: merges_path {merges_path!r} does not exist (CLIP's "
                                    "bpe_simple_vocab_16e6.txt or .txt.gz, provided locally)")
        opener = gzip.open if str(merges_path).endswith(".gz") else open
        with opener(str(merges_path), "rt", encoding="utf-8") as f:
            lines = f.read().split("\n")
        merges = [tuple(ln.split()) for ln in lines[1:1 + MAX_MERGES] if len(ln.split()) == 2]
        self.byte_encoder = bytes_to_unicode()
        vocab = list(self.byte_encoder.values())
        vocab = vocab + [v + "</w>" for v in vocab] + ["".join(m) for m in merges]
        vocab += ["<|startoftext|>", "<|endoftext|>"]
        self.encoder = {s: i for i, s in enumerate(vocab)}
        self.ranks = {m: i for i, m in enumerate(merges)}
        self.vocab_size = len(vocab)
        self.sot, self.eot = self.vocab_size - 2, self.vocab_size - 1
        self.cache = {"<|startoftext|>": "<|startoftext|>", "<|endoftext|>": "<|endoftext|>"}
        self.pat = _compile_pattern()

    def bpe(self, token):
        if token in self.cache:
            return self.cache[token]
        word = tuple(token[:-1]) + (token[-1] + "</w>",)
        while len(word) > 1:
            pairs = set(zip(word[:-1], word[1:]))
            best = min(pairs, key=lambda p: self.ranks.get(p, float("inf")))
            if best not in self.ranks:
                break
            a, b = best
            new, i = [], 0
            while i < len(word):
                if i < len(word) - 1 and word[i] == a and word[i + 1] == b:
                    new.append(a + b)
                    i += 2
                else:
                    new.append(word[i])
                    i += 1
            word = tuple(new)
        out = " ".join(word)
        self.cache[token] = out
        return out

    def encode(self, text):
        ids = []
        for tok in self.pat.findall(_clean(text)):
            tok = "".join(self.byte_encoder[b] for b in tok.encode("utf-8"))
            ids.extend(self.encoder[t] for t in self.bpe(tok).split(" "))
        return ids

    def __call__(self, texts, context_length=77, truncate=False):
        """int32 [N, context_length]: ``[start, ..., end, 0, 0, ...]`` per text."""
        if isinstance(texts, str):
            texts = [texts]
        out = torch.zeros(len(texts), context_length, dtype=torch.int32)
        for i, text in enumerate(texts):
            toks = [self.sot] + self.encode(text) + [self.eot]
            if len(toks) > context_length:
                if not truncate:
                    raise RuntimeError(f"Input {text!r} is too long for context length {context_length}")
                toks = toks[:context_length]
                toks[-1] = self.eot
            out[i, :len(toks)] = torch.tensor(toks, dtype=torch.int32)
        return out
