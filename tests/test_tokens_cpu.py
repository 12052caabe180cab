"""moegan_mi.tokens on the host: pack_tokens' row placement, row_off, the two buckets, max_tokens, the rejection of a
zero length; and the memory-mapped dataset / collate round trip on synthetic .npy files."""
import numpy as np
import pytest
import torch

from moegan_mi.tokens import ProcessedTokenDataset, collate_tokens, pack_tokens, token_files


def _batch(lens, L=77, seed=0):
    rng = np.random.default_rng(seed)
    tok = rng.standard_normal((len(lens), L, 512)).astype(np.float16)
    for b, n in enumerate(lens):  # what encode_captions leaves past a caption: must never arrive in the packed rows
        tok[b, n:] = 99.0
    return tok


def test_pack_rows_offsets_and_pad():
    lens = [3, 9, 1, 24, 8]
    tok = _batch(lens)
    rows, off, lk = pack_tokens(tok, np.array(lens, dtype=np.int32))
    assert rows.dtype == np.float16 and off.dtype == np.int32 and off.shape == (6,)
    assert off.tolist() == [0] + np.cumsum(lens).tolist()
    for b, n in enumerate(lens):
        assert np.array_equal(rows[off[b]:off[b + 1]], tok[b, :n])
    assert rows.shape == (60, 512)  # 45 live rows -> next multiple of 4 * 5
    assert not rows[off[-1]:].any()
    assert lk == 32


@pytest.mark.parametrize("lens,rows,lk", [([32, 5], 40, 32), ([33, 5], 40, 64), ([4, 4], 8, 32), ([4, 5], 16, 32),
                                          ([64, 1, 1], 72, 64), ([65, 1, 1], 72, 96), ([77], 80, 96)])
def test_pack_buckets(lens, rows, lk):
    r, off, got = pack_tokens(_batch(lens), lens)
    B, total = len(lens), sum(lens)
    assert r.shape[0] == rows and rows % (4 * B) == 0 and 0 <= rows - total < 4 * B
    assert got == lk and got % 32 == 0 and 0 <= got - max(lens) < 32
    assert off[-1] == total


def test_pack_max_tokens_truncates():
    lens = [3, 40, 12]
    tok = _batch(lens)
    rows, off, lk = pack_tokens(tok, lens, max_tokens=10)
    assert off.tolist() == [0, 3, 13, 23] and lk == 32 and rows.shape[0] == 24
    assert np.array_equal(rows[3:13], tok[1, :10]) and np.array_equal(rows[13:23], tok[2, :10])
    assert not rows[23:].any()


def test_pack_rejects_bad_lengths():
    tok = _batch([3, 3])
    with pytest.raises(ValueError):
        pack_tokens(tok, [3, 0])
    with pytest.raises(ValueError):
        pack_tokens(tok, [3, -2])
    with pytest.raises(ValueError):
        pack_tokens(tok, [3, 78])  # more than the rows stored
    with pytest.raises(ValueError):
        pack_tokens(tok, [3])


def test_dataset_collate_round_trip(tmp_path):
    N, lens = 6, [5, 17, 1, 33, 8, 24]
    rng = np.random.default_rng(1)
    img = rng.standard_normal((N, 3, 8, 8)).astype(np.float32)
    emb = rng.standard_normal((N, 512)).astype(np.float32)
    tok = _batch(lens, seed=2)
    emb_f = str(tmp_path / "mscoco_train_text_embeddings.npy")
    tok_f, len_f = token_files(emb_f)
    assert tok_f.endswith("mscoco_train_text_tokens.npy") and len_f.endswith("mscoco_train_text_len.npy")
    np.save(tmp_path / "mscoco_train_images.npy", img)
    np.save(emb_f, emb)
    with pytest.raises(FileNotFoundError, match="text_tokens"):
        ProcessedTokenDataset(str(tmp_path / "mscoco_train_images.npy"), emb_f)
    np.save(tok_f, tok)
    np.save(len_f, np.array(lens, dtype=np.int32))
    ds = ProcessedTokenDataset(str(tmp_path / "mscoco_train_images.npy"), emb_f)
    assert len(ds) == N and ds[3][2].shape == (33, 512)
    dl = torch.utils.data.DataLoader(ds, batch_size=3, shuffle=False, collate_fn=collate_tokens)
    for i, (im, te, rows, off, lk) in enumerate(dl):
        sl = slice(3 * i, 3 * i + 3)
        want_rows, want_off, want_lk = pack_tokens(tok[sl], lens[sl])
        assert torch.equal(im, torch.from_numpy(img[sl])) and torch.equal(te, torch.from_numpy(emb[sl]))
        assert rows.dtype == torch.float16 and off.dtype == torch.int32 and isinstance(lk, int)
        assert np.array_equal(rows.numpy(), want_rows) and np.array_equal(off.numpy(), want_off) and lk == want_lk
    assert i == 1
    ds2 = ProcessedTokenDataset(str(tmp_path / "mscoco_train_images.npy"), emb_f, max_tokens=4)
    assert [ds2[j][2].shape[0] for j in range(N)] == [4, 4, 1, 4, 4, 4]
