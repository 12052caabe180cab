"""Forward-only CLIP text tower (moegan_mi/clip_text.py) vs a plain fp32 PyTorch restatement of OpenAI CLIP's text
side (token + positional embedding, pre-LN residual blocks with a causal nn.MultiheadAttention and a QuickGELU MLP,
ln_final, the end-token row @ text_projection) on the same OpenAI-layout state_dict, and the prompt path built on it
(t2i_moe_gan.load_clip_weights / encode_text_with_clip / encode_prompt / sample_aurora_gan, encode_captions).  The
restatement runs all 77 padded positions, so it also checks that dropping the dead rows changes nothing.  CLIP's
weights are not available (no download): random weights at CLIP's init scales exercise every op; values stay
parity-unpinned against real CLIP.

Bar: the image tower's, for the same op chain and dtype (tests/test_clip_gpu.py): cosine >= 0.999 per row and 2e-2
relative L2 overall, for the pooled features and for the per-token features of the live rows.  Measured on an
MI355X: 2 layers cosine >= 0.99995, rel L2 8.0e-3 (pooled) / 7.6e-3 (tokens); 12 layers cosine >= 0.99991, rel L2
1.11e-2 for both -- inside the bar, so no oracle-side bf16 floor was needed.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda"
LENS = [2, 9, 17, 40, 77]


def torch_text(sd, ids, heads):
    """(pooled [N, out], per-token features [N, ctx, out]) in fp32, every padded position computed."""
    N, ctx = ids.shape
    w = sd["token_embedding.weight"].shape[1]
    x = sd["token_embedding.weight"][ids.long()] + sd["positional_embedding"]
    mask = torch.full((ctx, ctx), float("-inf")).triu(1)
    i = 0
    while f"transformer.resblocks.{i}.ln_1.weight" in sd:
        p = f"transformer.resblocks.{i}."
        h = F.layer_norm(x, (w,), sd[p + "ln_1.weight"], sd[p + "ln_1.bias"])
        a, _ = F.multi_head_attention_forward(
            h.transpose(0, 1), h.transpose(0, 1), h.transpose(0, 1), w, heads, sd[p + "attn.in_proj_weight"],
            sd[p + "attn.in_proj_bias"], None, None, False, 0.0, sd[p + "attn.out_proj.weight"],
            sd[p + "attn.out_proj.bias"], need_weights=False, attn_mask=mask)
        x = x + a.transpose(0, 1)
        h = F.layer_norm(x, (w,), sd[p + "ln_2.weight"], sd[p + "ln_2.bias"])
        h = F.linear(h, sd[p + "mlp.c_fc.weight"], sd[p + "mlp.c_fc.bias"])
        h = h * torch.sigmoid(1.702 * h)
        x = x + F.linear(h, sd[p + "mlp.c_proj.weight"], sd[p + "mlp.c_proj.bias"])
        i += 1
    x = F.layer_norm(x, (w,), sd["ln_final.weight"], sd["ln_final.bias"]) @ sd["text_projection"]
    return x[torch.arange(N), ids.argmax(-1)], x


def make_ids(lens, vocab, ctx=77, seed=0):
    """[start, random ids in [1, vocab - 3], end, 0, ...]: start = vocab - 2, end = vocab - 1."""
    g = torch.Generator().manual_seed(seed)
    ids = torch.zeros(len(lens), ctx, dtype=torch.int32)
    for b, n in enumerate(lens):
        ids[b, 0] = vocab - 2
        ids[b, 1:n - 1] = torch.randint(1, vocab - 2, (n - 2,), generator=g, dtype=torch.int32)
        ids[b, n - 1] = vocab - 1
    return ids


@pytest.mark.parametrize("layers", [2, 12])
def test_clip_text_tower_vs_torch(layers):
    from moegan_mi.clip_text import ClipTextEncoder, random_state_dict
    sd = random_state_dict(512, layers, 77, vocab_size=512, output_dim=512, seed=layers)
    enc = ClipTextEncoder(sd, device=DEV)
    ids = make_ids(LENS, 512, seed=layers)
    ref_pool, ref_tok = torch_text(sd, ids, 8)
    pooled, tokens, text_len = enc.encode_text(ids.to(DEV), return_tokens=True)
    pooled, tokens = pooled.cpu(), tokens.cpu()
    assert pooled.shape == (5, 512) and pooled.dtype == torch.float32
    assert tokens.shape == (5, 77, 512) and tokens.dtype == torch.float32
    assert text_len.dtype == torch.int32 and text_len.tolist() == LENS
    cos = F.cosine_similarity(pooled.double(), ref_pool.double(), dim=1)
    rel = float((pooled - ref_pool).norm() / ref_pool.norm())
    live = torch.arange(77)[None, :] < torch.tensor(LENS)[:, None]
    tcos = F.cosine_similarity(tokens[live].double(), ref_tok[live].double(), dim=1)
    trel = float((tokens[live] - ref_tok[live]).norm() / ref_tok[live].norm())
    print(f"CLIP text tower layers={layers}: pooled cosine {cos.tolist()}, rel L2 {rel:.3e}; "
          f"tokens min cosine {float(tcos.min()):.6f}, rel L2 {trel:.3e}")
    assert float(cos.min()) >= 0.999 and rel <= 2e-2
    assert float(tcos.min()) >= 0.999 and trel <= 2e-2
    assert bool((tokens[~live] == 0).all())
    # the pooled-only call is the same computation
    assert torch.equal(enc.encode_text(ids.to(DEV)).cpu(), pooled)


def test_whole_model_dict_builds_both_towers():
    from moegan_mi import clip_text, clip_vit
    layers = 2
    full = {"visual." + k: v for k, v in clip_vit.random_state_dict(128, 2, 32, 224, 512, seed=1).items()}
    full.update(clip_text.random_state_dict(512, layers, 77, vocab_size=512, output_dim=512, seed=2))
    full["logit_scale"] = torch.tensor(4.6)
    t = clip_text.ClipTextEncoder(full, device=DEV)
    assert (t.width, t.layers, t.heads, t.context_length, t.vocab_size) == (512, layers, 8, 77, 512)
    v = clip_vit.ClipImageEncoder(full, device=DEV)
    assert (v.width, v.layers, v.heads) == (128, 2, 2)
    assert clip_text.has_text_tower(full) and not clip_text.has_text_tower(
        {k: x for k, x in full.items() if k.startswith("visual.")})


MERGES = ["a b", "c d</w>", "e f"]  # vocabulary 512 + 3 + 2 = 517


@pytest.fixture()
def clip_files(tmp_path):
    """(weights path, merges path): random whole-model weights (2-layer towers) whose vocabulary matches a tiny
    synthetic merges file."""
    from moegan_mi import clip_text, clip_vit
    bpe = tmp_path / "merges.txt"
    bpe.write_text("#version: synthetic\n" + "\n".join(MERGES) + "\n", encoding="utf-8")
    full = {"visual." + k: v for k, v in clip_vit.random_state_dict(128, 2, 32, 224, 512, seed=3).items()}
    full.update(clip_text.random_state_dict(128, 2, 77, vocab_size=512 + len(MERGES) + 2, output_dim=512, seed=4))
    full["logit_scale"] = torch.tensor(4.6)
    w = tmp_path / "clip.pt"
    torch.save(full, w)
    return str(w), str(bpe)


def test_dropin_prompt_path(clip_files):
    import t2i_moe_gan as M
    weights, bpe = clip_files
    try:
        model = M.load_clip_weights(weights, device=DEV, bpe_path=bpe)
        assert M.get_clip_model()[0] is model
        for name in ("encode_image", "encode_generated", "encode_text", "tokenize"):
            assert hasattr(model, name), name
        emb = M.encode_text_with_clip(["a b", "c"])  # no ``clip`` package anywhere
        assert emb.shape == (2, 512) and emb.dtype == torch.float32 and bool(torch.isfinite(emb).all())
        pooled, tokens, text_len = M.encode_prompt(["a b", "c"])
        assert pooled.shape == (2, 512) and torch.equal(pooled, emb)
        assert text_len.tolist() == [4, 3]  # start, a, b, end / start, c, end
        assert tokens.shape == (2, 4, 512) and bool((tokens[1, 3] == 0).all())
        ids = model.tokenize(["a b", "c"])
        assert torch.equal(model.encode_text(ids), emb)  # an id tensor is accepted as well
        # CLIPLoss still works with the registered object
        g = torch.Generator().manual_seed(2)
        img16 = (torch.rand(2, 3, 16, 16, generator=g) * 2 - 1).to(DEV)
        loss = M.CLIPLoss(DEV)(img16, emb)
        assert bool(torch.isfinite(loss)) and 0.0 <= float(loss) <= 2.0
        # sampling from a string prompt
        G = M.AuroraGenerator(seed=2).to(DEV)
        torch.manual_seed(5)
        a = M.sample_aurora_gan(G, "a b", num_samples=2, device=DEV, prompt_tokens=True)
        assert a.shape == (2, 3, 16, 16) and bool(torch.isfinite(a).all())
        p1, t1, l1 = M.encode_prompt("a b")
        torch.manual_seed(5)
        z = torch.randn(2, 512, device=DEV, dtype=torch.float32)
        with torch.no_grad():
            b, _ = G.eval()(z, p1.repeat(2, 1), truncation_psi=0.7, text_tokens=t1.repeat(2, 1, 1),
                            text_len=l1.repeat(2))
            c, _ = G(z, p1.repeat(2, 1), truncation_psi=0.7)
        assert torch.equal(a, b.clamp(-1, 1))
        torch.manual_seed(5)
        d = M.sample_aurora_gan(G, "a b", num_samples=2, device=DEV, prompt_tokens=False)
        assert torch.equal(d, c.clamp(-1, 1))
        torch.manual_seed(5)
        assert torch.equal(d, M.sample_aurora_gan(G, "a b", num_samples=2, device=DEV))  # the default
    finally:
        M.set_clip_model(None)


def test_visual_only_file_registers_the_image_tower(tmp_path):
    import t2i_moe_gan as M
    from moegan_mi import clip_vit
    w = tmp_path / "visual.pt"
    torch.save({"visual." + k: v for k, v in clip_vit.random_state_dict(128, 2, 32, 224, 512, seed=3).items()}, w)
    try:
        enc = M.load_clip_weights(str(w), device=DEV)
        assert isinstance(enc, clip_vit.ClipImageEncoder) and not hasattr(enc, "encode_text")
        with pytest.raises(ValueError):
            M.load_clip_weights(str(w), device=DEV, bpe_path=str(tmp_path / "unused.txt"))
    finally:
        M.set_clip_model(None)


def test_encode_captions_main(clip_files, tmp_path):
    from moegan_mi import encode_captions
    from moegan_mi.clip_bpe import ClipTokenizer
    from moegan_mi.clip_text import ClipTextEncoder
    weights, bpe = clip_files
    caps = ["a b", "c d e f", "", "ab cd, ef!"]
    cap = tmp_path / "captions.txt"
    cap.write_text("\n".join(caps) + "\n", encoding="utf-8")
    prefix = str(tmp_path / "train")
    assert encode_captions.main(["--weights", weights, "--bpe", bpe, "--captions", str(cap), "--out", prefix,
                                 "--tokens"]) == 0
    emb, tok, ln = (np.load(prefix + s) for s in ("_text_embeddings.npy", "_text_tokens.npy", "_text_len.npy"))
    assert emb.shape == (4, 512) and emb.dtype == np.float32
    assert tok.shape == (4, 77, 512) and tok.dtype == np.float16
    assert ln.shape == (4,) and ln.dtype == np.int32
    ids = ClipTokenizer(bpe)(caps)
    enc = ClipTextEncoder.from_file(weights, device=DEV)
    pooled, tokens, text_len = enc.encode_text(ids, return_tokens=True)
    assert torch.equal(torch.from_numpy(emb), pooled.cpu())
    assert ln.tolist() == text_len.tolist() == (ids.argmax(-1) + 1).tolist()
    Lk = tokens.shape[1]
    assert torch.equal(torch.from_numpy(tok[:, :Lk]), tokens.to(torch.float16).cpu()) and not tok[:, Lk:].any()
    # without --tokens: the embeddings alone, the same values
    prefix2 = str(tmp_path / "val")
    assert encode_captions.main(["--weights", weights, "--bpe", bpe, "--captions", str(cap), "--out", prefix2]) == 0
    assert np.array_equal(np.load(prefix2 + "_text_embeddings.npy"), emb)
    assert not (tmp_path / "val_text_tokens.npy").exists()
