"""Forward-only CLIP text tower on the HIP kernels: token ids -> pooled text features and per-token text features.

The reference turns prompts into embeddings with the ``clip`` package (``model.encode_text(clip.tokenize(text))``,
t2i_moe_gan.py:211-216, :297-303, :692), which is not available to this build.  This module is the text tower itself,
reading the OpenAI state_dict layout (``token_embedding.weight``, ``positional_embedding``,
``transformer.resblocks.{i}.{ln_1,attn,ln_2,mlp.c_fc,mlp.c_proj}.*``, ``ln_final.*``, ``text_projection``) from a
local file or a whole-model dict (``visual.*`` and ``logit_scale`` are ignored), or random-initialised at CLIP's
init scales (values are then parity-unpinned against real CLIP: its weights cannot be fetched here).

Ragged: the tower's self-attention is causal, so a token's output never depends on later tokens, and the pooled
feature is read at the end token.  Every GEMM, LayerNorm and attention call therefore runs on the live rows only
(start token .. end token of each caption, packed back to back; mg_attn_causal_fwd takes the row offsets) instead of
N * context_length padded rows.

Compute as the image tower (clip_vit.py): every Linear on the MFMA GEMM core with bias / QuickGELU / residual add in
the epilogue, LayerNorm on mg_layernorm_fwd; activations are bf16 token rows, LayerNorm statistics and GEMM
accumulation fp32.
"""
import torch

from . import _lib as L
from . import ops

_TEXT_KEY = "token_embedding.weight"


def has_text_tower(sd):
    """True when a state_dict carries the text side of CLIP."""
    return _TEXT_KEY in sd


class ClipTextEncoder:
    def __init__(self, state_dict=None, device="cuda", **random_kw):
        sd = state_dict if state_dict is not None else random_state_dict(**random_kw)
        if _TEXT_KEY not in sd:
            raise KeyError(f"ClipTextEncoder: no {_TEXT_KEY} in the state_dict (image-tower weights only?)")
        # infer the architecture from the weights
        self.vocab_size, self.width = sd[_TEXT_KEY].shape
        self.context_length = sd["positional_embedding"].shape[0]
        self.layers = 1 + max(int(k.split(".")[2]) for k in sd if k.startswith("transformer.resblocks."))
        self.heads = self.width // 64  # OpenAI CLIP: 64-wide heads
        self.output_dim = sd["text_projection"].shape[1]
        if self.context_length > 128:
            raise ValueError("ClipTextEncoder: context length above 128 (mg_attn_causal_fwd)")
        self.dev = torch.device(device)
        self._load(sd)

    @classmethod
    def from_file(cls, path, device="cuda"):
        """OpenAI CLIP weights saved as a plain state_dict or safetensors; nothing from the file is executed."""
        if str(path).endswith(".safetensors"):
            from safetensors.torch import load_file
            sd = load_file(str(path))
        else:
            sd = torch.load(path, map_location="cpu", weights_only=True)
        return cls(sd, device=device)

    def _load(self, sd):
        dev, bf = self.dev, torch.bfloat16
        mat = lambda t: t.detach().to(dev, bf).contiguous()  # noqa: E731  (MFMA operands)
        vec = lambda t: t.detach().to(dev, torch.float32).contiguous()  # noqa: E731  (bias / LN / embeddings)
        self.tok = vec(sd[_TEXT_KEY])
        self.pos = vec(sd["positional_embedding"])
        self.ln_final = (vec(sd["ln_final.weight"]), vec(sd["ln_final.bias"]))
        self.proj_t = mat(sd["text_projection"].t())  # [out, w]
        self.blocks = []
        for i in range(self.layers):
            p = f"transformer.resblocks.{i}."
            self.blocks.append(dict(
                ln1=(vec(sd[p + "ln_1.weight"]), vec(sd[p + "ln_1.bias"])),
                W_in=mat(sd[p + "attn.in_proj_weight"]), b_in=vec(sd[p + "attn.in_proj_bias"]),
                W_out=mat(sd[p + "attn.out_proj.weight"]), b_out=vec(sd[p + "attn.out_proj.bias"]),
                ln2=(vec(sd[p + "ln_2.weight"]), vec(sd[p + "ln_2.bias"])),
                W_fc=mat(sd[p + "mlp.c_fc.weight"]), b_fc=vec(sd[p + "mlp.c_fc.bias"]),
                W_proj=mat(sd[p + "mlp.c_proj.weight"]), b_proj=vec(sd[p + "mlp.c_proj.bias"])))

    @torch.no_grad()
    def encode_text(self, ids, return_tokens=False):
        """ids: integer [N, context_length], ``[start, ..., end, 0, ...]``; the end position is ``ids.argmax(-1)``
        (CLIP's rule: the end token has the largest id).  Returns the pooled features [N, output_dim] fp32 (the
        end-token row through ln_final and text_projection); with ``return_tokens`` also ``tokens`` [N, Lk,
        output_dim] fp32 (every live row through ln_final and text_projection, Lk = the longest caption, padding
        rows zero) and ``text_len`` int32 [N] -- the generator's ``text_tokens=`` / ``text_len=``."""
        dev, w = self.dev, self.width
        ids = torch.as_tensor(ids).to(dev)
        if ids.dim() != 2 or ids.shape[1] != self.context_length:
            raise ValueError(f"ids: [N, {self.context_length}], got {tuple(ids.shape)}")
        N, ctx = ids.shape
        if N == 0:
            pooled = torch.zeros(0, self.output_dim, device=dev)
            if return_tokens:
                return pooled, torch.zeros(0, 1, self.output_dim, device=dev), torch.zeros(0, device=dev, dtype=torch.int32)
            return pooled
        lens = ids.argmax(-1) + 1  # [N]
        row_off = torch.zeros(N + 1, device=dev, dtype=torch.int32)
        row_off[1:] = lens.cumsum(0)
        Lk = int(lens.max())  # host reads of the lengths: the longest one here, the live-row count below
        live = torch.arange(ctx, device=dev)[None, :] < lens[:, None]  # [N, ctx]
        bt = live.nonzero()  # (caption, position) of every live row, in packed order
        # token + positional embedding of the live rows
        x = ops.gather_rows(self.tok, ids[live].to(torch.int32).contiguous())
        x += ops.gather_rows(self.pos, bt[:, 1].to(torch.int32).contiguous())
        xb = ops.cast(x, torch.bfloat16)  # the residual stream
        for blk in self.blocks:
            n1, _, _ = ops.layernorm_fwd(xb, *blk["ln1"])
            qkv = ops.linear(n1, blk["W_in"], bias=blk["b_in"])
            att = ops.attn_causal_fwd(qkv, row_off, N, Lk, w, heads=self.heads)
            xb = ops.linear(att, blk["W_out"], bias=blk["b_out"], resid=xb, ld_res=w)  # x + attn(ln_1(x))
            n2, _, _ = ops.layernorm_fwd(xb, *blk["ln2"])
            hid = ops.linear(n2, blk["W_fc"], bias=blk["b_fc"], act=L.ACT_QUICK_GELU)
            xb = ops.linear(hid, blk["W_proj"], bias=blk["b_proj"], resid=xb, ld_res=w)  # x + mlp(ln_2(x))
        end_rows = ops.gather_rows(xb, (row_off[1:] - 1).contiguous())
        e, _, _ = ops.layernorm_fwd(end_rows, *self.ln_final)
        pooled = ops.linear(e, self.proj_t, out_dtype=torch.float32)
        if not return_tokens:
            return pooled
        f, _, _ = ops.layernorm_fwd(xb, *self.ln_final)
        rows = ops.linear(f, self.proj_t, out_dtype=torch.float32)
        tokens = torch.zeros(N, Lk, self.output_dim, device=dev, dtype=torch.float32)
        tokens[bt[:, 0], bt[:, 1]] = rows
        return pooled, tokens, lens.to(torch.int32)

    __call__ = encode_text


def random_state_dict(width=512, layers=12, context_length=77, vocab_size=49408, output_dim=512, seed=0):
    """OpenAI CLIP's text-side initialisation scales (CLIP.initialize_parameters): token embedding std 0.02,
    positional embedding 0.01, attention weights width^-0.5, output projections width^-0.5 (2 layers)^-0.5, fc
    (2 width)^-0.5, text_projection width^-0.5; in its state_dict layout."""
    gen = torch.Generator().manual_seed(seed)
    n = lambda *s, std: torch.randn(*s, generator=gen) * std  # noqa: E731
    sc = width ** -0.5
    proj_std, attn_std, fc_std = sc * (2 * layers) ** -0.5, sc, (2 * width) ** -0.5
    sd = {_TEXT_KEY: n(vocab_size, width, std=0.02), "positional_embedding": n(context_length, width, std=0.01),
          "ln_final.weight": torch.ones(width), "ln_final.bias": torch.zeros(width),
          "text_projection": n(width, output_dim, std=sc)}
    for i in range(layers):
        p = f"transformer.resblocks.{i}."
        sd.update({p + "ln_1.weight": torch.ones(width), p + "ln_1.bias": torch.zeros(width),
                   p + "ln_2.weight": torch.ones(width), p + "ln_2.bias": torch.zeros(width),
                   p + "attn.in_proj_weight": n(3 * width, width, std=attn_std),
                   p + "attn.in_proj_bias": torch.zeros(3 * width),
                   p + "attn.out_proj.weight": n(width, width, std=proj_std),
                   p + "attn.out_proj.bias": torch.zeros(width),
                   p + "mlp.c_fc.weight": n(4 * width, width, std=fc_std), p + "mlp.c_fc.bias": torch.zeros(4 * width),
                   p + "mlp.c_proj.weight": n(width, 4 * width, std=proj_std),
                   p + "mlp.c_proj.bias": torch.zeros(width)})
    return sd


ClipTextEncoder.random_state_dict = staticmethod(random_state_dict)


class ClipModel:
    """The CLIP-like object the drop-in module registers (t2i_moe_gan.set_clip_model) when a weights file holds the
    text side: ``encode_image`` / ``encode_generated`` of the image tower (when the file has ``visual.*`` keys),
    ``encode_text`` on ids -- or on strings when a tokenizer is attached -- and ``tokenize``."""

    def __init__(self, text, image=None, tokenizer=None):
        self.text, self.image, self.tokenizer = text, image, tokenizer
        if image is not None:
            self.encode_image = image.encode_image
            self.encode_generated = image.encode_generated
        if tokenizer is not None:
            self.tokenize = self._tokenize

    def _tokenize(self, texts, context_length=None, truncate=False):
        return self.tokenizer(texts, context_length or self.text.context_length, truncate)

    def _ids(self, text):
        if isinstance(text, str) or (isinstance(text, (list, tuple)) and len(text) and isinstance(text[0], str)):
            if self.tokenizer is None:
                raise RuntimeError("encode_text on strings needs a tokenizer: load_clip_weights(path, bpe_path=...)")
            return self._tokenize(text)
        return text

    def encode_text(self, text, return_tokens=False):
        return self.text.encode_text(self._ids(text), return_tokens=return_tokens)
