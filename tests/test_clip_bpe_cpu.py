"""CLIP's byte-level BPE (moegan_mi/clip_bpe.py) on a synthetic merges file.  Expected ids are literals derived by
hand from the vocabulary order: the 256 byte symbols (byte b in ``!..~`` -> b - 33, ``¡..¬`` -> 94 + b - 161,
``®..ÿ`` -> 106 + b - 174, the rest after them), the same 256 with ``</w>`` (+ 256), one id per merge line from 512,
then start and end.  Seven merges: vocabulary 521, start 519, end 520."""
import gzip

import pytest
import torch

from moegan_mi.clip_bpe import ClipTokenizer

MERGES = ["t h",         # 512 "th"
          "th e</w>",    # 513 "the</w>"
          "c a",         # 514 "ca"
          "ca t</w>",    # 515 "cat</w>"
          "! !</w>",     # 516 "!!</w>"
          "Ã ©</w>",     # 517: the two UTF-8 bytes of "é" (0xC3 -> "Ã", 0xA9 -> "©"), word-final
          "' s</w>"]     # 518 "'s</w>"
SOT, EOT = 519, 520


@pytest.fixture(scope="module")
def tok(tmp_path_factory):
    p = tmp_path_factory.mktemp("bpe") / "merges.txt"
    p.write_text("#version: synthetic\n" + "\n".join(MERGES) + "\n", encoding="utf-8")
    return ClipTokenizer(str(p))


@pytest.mark.parametrize("text,ids", [
    ("the", [513]),                        # merges fully: t h -> th, th e</w> -> the</w>
    ("cat", [515]),
    ("xyz", [87, 88, 89 + 256]),           # no applicable merge: byte symbols, </w> on the last
    ("123", [16 + 256, 17 + 256, 18 + 256]),  # digits split one by one, each its own word
    ("!!", [516]),                         # punctuation run, merged
    ("!!!", [0, 516]),                     # (!, !, !</w>): only the word-final pair has a rank
    ("?!", [30, 0 + 256]),
    ("THE Cat", [513, 515]),               # upper case folded
    ("  the    cat  ", [513, 515]),        # repeated spaces
    ("é", [517]),                          # a two-byte character, merged
    ("ü", [127, 120 + 256]),               # 0xC3 0xBC, no merge
    ("cat's", [515, 518]),                 # 's split off as its own word
    ("the cat!!", [513, 515, 516]),
    ("&amp;amp;", [5 + 256]),              # html.unescape twice -> "&"
    ("", []),
])
def test_encode_literals(tok, text, ids):
    assert tok.encode(text) == ids


def test_vocabulary_and_layout(tok):
    assert tok.vocab_size == 512 + len(MERGES) + 2
    assert (tok.sot, tok.eot) == (SOT, EOT) == (tok.vocab_size - 2, tok.vocab_size - 1)
    out = tok(["the cat", "xyz", ""])
    assert out.dtype == torch.int32 and tuple(out.shape) == (3, 77)
    assert out[0].tolist() == [SOT, 513, 515, EOT] + [0] * 73
    assert out[1].tolist() == [SOT, 87, 88, 345, EOT] + [0] * 72
    assert out[2].tolist() == [SOT, EOT] + [0] * 75
    assert out.argmax(-1).tolist() == [3, 4, 1]  # CLIP's end-token rule finds the end position
    one = tok("the")  # a single string is a batch of one
    assert tuple(one.shape) == (1, 77) and one[0, :3].tolist() == [SOT, 513, EOT]


def test_too_long(tok):
    text = "the cat the cat"
    with pytest.raises(RuntimeError, match="the cat the cat"):
        tok([text], context_length=5)
    out = tok([text], context_length=5, truncate=True)
    assert out[0].tolist() == [SOT, 513, 515, 513, EOT]
    assert tok([text], context_length=6)[0].tolist() == [SOT, 513, 515, 513, 515, EOT]


def test_gz_file_and_missing_file(tmp_path, tok):
    p = tmp_path / "merges.txt.gz"
    with gzip.open(p, "wt", encoding="utf-8") as f:
        f.write("#version: synthetic\n" + "\n".join(MERGES) + "\n")
    gz = ClipTokenizer(str(p))
    assert gz.vocab_size == tok.vocab_size and gz.encode("the cat's é") == tok.encode("the cat's é")
    with pytest.raises(FileNotFoundError, match="merges_path"):
        ClipTokenizer(str(tmp_path / "nope.txt"))


def test_re_fallback_splits_like_regex():
    """Without the ``regex`` module the pattern is restated for ``re``; both split the same way."""
    import re
    from moegan_mi import clip_bpe
    regex = pytest.importorskip("regex")
    a, b = regex.compile(clip_bpe._PAT, regex.IGNORECASE), re.compile(clip_bpe._PAT_RE, re.IGNORECASE)
    for s in ["a cat's hat, 42 of them!!", "naïve café_x -- y?", "it's we're i'll <|endoftext|> ok", "x_y__z 3.5"]:
        assert a.findall(s) == b.findall(s), s
