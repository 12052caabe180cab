"""Drop-in replacement for the reference module ``t2i_moe_gan`` (moegan/t2i_moe_gan.py) on MI355X.

Same public names and signatures -- ``train_aurora_gan``, ``AuroraGenerator``,
``AuroraDiscriminator``, ``AuroraGANLoss``, ``sample_aurora_gan``, the sub-module classes
(``ModulatedConv``, ``ModulatedTransformationModule``, ``SparseExpertFFN``, ``BayesianRouter``,
``SparseMoE``, ``AttentionBlock``, ``ConvolutionBlock``, ``GenerativeBlock``, moegan_mi/modules.py),
``create_optimizer_for_active_blocks``, the module constants -- and
the same ``state_dict`` keys/shapes, so the reference's entry points (train_model.py,
sagemaker_train.py, inference.py, generate_images.py) work by pointing ``sys.path`` here.

Differences by design:
  * the math runs on libmoegan_hip (hand-written gfx950 kernels) through explicit forward/backward
    engines; there is no CPU execution path for the models (the CPU restatement in ``oracle/`` is
    test infrastructure).  Models can be constructed, loaded and saved on the CPU;
  * each model's parameters are ONE flat tensor (``model.flat``); ``state_dict()`` still exposes the
    reference names, so checkpoints interchange with the reference;
  * ``AuroraDiscriminator.forward`` supports first-order autograd; the R1 double backward of the
    training loop is done in closed form inside the fused training step;
  * activation checkpointing and the OOM/memory guards are no-ops (288 GB HBM);
  * the CLIP loss needs a local CLIP image encoder (``set_clip_model``); without one it is
    reported as 0 -- it never contributes a gradient in the reference either (:98-101).
"""
import logging
import math
import os
import sys

import torch
import torch.nn as nn
import torch.nn.functional as F

_HERE = os.path.dirname(os.path.abspath(__file__))
if _HERE not in sys.path:
    sys.path.insert(0, _HERE)

from moegan_mi.engine_d import DiscriminatorEngine  # noqa: E402
from moegan_mi.engine_g import GeneratorEngine  # noqa: E402
from moegan_mi.init import init_discriminator, init_generator, init_vision_head  # noqa: E402
from moegan_mi.layout import (MAX_RESOLUTIONS, discriminator_shapes, frozen_rgb_prefixes,  # noqa: E402
                             generator_shapes, vision_head_shapes)
from moegan_mi.params import ParamStore  # noqa: E402
from moegan_mi.prefetch import DevicePrefetcher  # noqa: E402
from moegan_mi.step import StepConfig, TrainStep  # noqa: E402
from moegan_mi.checkpoint import load_resume, save_resume  # noqa: E402,F401
from moegan_mi.modules import _key_len  # noqa: E402
from moegan_mi.modules import (AttentionBlock, BayesianRouter, ConvolutionBlock, GenerativeBlock,  # noqa: E402,F401
                               ModulatedConv, ModulatedTransformationModule, SparseExpertFFN, SparseMoE,
                               create_optimizer_for_active_blocks)

LATENT_DIM = 512
TEXT_EMBEDDING_DIM = 512
DEVICE = torch.device("cuda:0" if torch.cuda.is_available() else "cpu")
NUM_EXPERTS = 4
CLIP_MODEL_TYPE = "ViT-B/32"

logging.basicConfig(level=logging.INFO)
logger = logging.getLogger(__name__)

_clip_model = None


def set_clip_model(model):
    """Register a CLIP-like model (``encode_image``/``encode_text``) loaded from local weights."""
    global _clip_model
    _clip_model = model


def load_clip_weights(path, device=None, bpe_path=None):
    """Register the forward-only CLIP image tower (moegan_mi/clip_vit.py) built from a local OpenAI CLIP
    state_dict / safetensors file; the CLIP loss terms (:66-119) then use it.  Returns the encoder.

    When the file also holds the text side (``token_embedding.weight`` ...), the registered object is a
    moegan_mi.clip_text.ClipModel: the same ``encode_image`` / ``encode_generated`` plus ``encode_text`` (token ids,
    or strings when ``bpe_path`` names CLIP's merges file, which also gives it ``tokenize``).  A file with only
    ``visual.*`` keys registers the image tower alone, as before."""
    from moegan_mi.clip_vit import ClipImageEncoder
    if str(path).endswith(".safetensors"):
        from safetensors.torch import load_file
        sd = load_file(str(path))
    else:
        sd = torch.load(path, map_location="cpu", weights_only=True)
    from moegan_mi.clip_text import ClipModel, ClipTextEncoder, has_text_tower
    has_image = any(k.startswith("visual.") for k in sd) or "conv1.weight" in sd
    image = ClipImageEncoder(sd, device=device or DEVICE) if has_image else None
    if not has_text_tower(sd):
        if bpe_path is not None:
            raise ValueError("load_clip_weights: bpe_path given but the file holds no text-tower weights")
        enc = image if image is not None else ClipImageEncoder(sd, device=device or DEVICE)
    else:
        tok = None
        if bpe_path is not None:
            from moegan_mi.clip_bpe import ClipTokenizer
            tok = ClipTokenizer(bpe_path)
        text = ClipTextEncoder(sd, device=device or DEVICE)
        if tok is not None and tok.vocab_size != text.vocab_size:
            raise ValueError(f"load_clip_weights: the merges file gives {tok.vocab_size} tokens, the weights "
                             f"{text.vocab_size}")
        enc = ClipModel(text, image, tok)
    set_clip_model(enc)
    return enc


def get_clip_model():
    """Reference :32-47.  CLIP weights cannot be downloaded here; use set_clip_model()."""
    if _clip_model is None:
        raise RuntimeError("no CLIP model registered: call t2i_moe_gan.set_clip_model(model) with local weights")
    return _clip_model, None


def _eps_for(store, generator=None):
    """Fresh router noise for one generator forward (the reference draws normal_() into its epsilon buffers per
    router, :349-351); ``generator`` = a torch.Generator (the rank-shared one under data parallelism)."""
    eps = []
    # one triple per attention (MoE) block, in block order: three, or four with attn_resolution = 32
    for name in sorted({n.split(".")[0] for n in store.buffers if n.endswith(".attn_block.moe.router.epsilon_f")},
                       key=lambda s: int(s.rsplit("_", 1)[1])):
        r = f"{name}.attn_block.moe.router."
        trip = []
        for n in ("epsilon_f", "epsilon_t", "epsilon_c"):
            buf = store.buffers[r + n]
            buf.normal_(generator=generator)
            trip.append(buf)
        eps.append(tuple(trip))
    return eps


class _FlatModule(nn.Module):
    """nn.Module over a ParamStore: one flat parameter, reference-named state_dict."""

    def __init__(self, shapes, frozen=(), dtype="fp32"):
        super().__init__()
        cdt = torch.bfloat16 if dtype == "bf16" else torch.float32
        self._store = ParamStore(shapes, "cpu", frozen_prefixes=frozen, shadow_dtype=cdt)
        self.flat = nn.Parameter(self._store.data)
        self._cdt = cdt

    def _apply(self, fn, recurse=True):
        super()._apply(fn, recurse)
        self._store.rebind(self.flat.data)
        return self

    def state_dict(self, *args, destination=None, prefix="", keep_vars=False):
        sd = self._store.state_dict(cpu=False)
        if destination is not None:
            for k, v in sd.items():
                destination[prefix + k] = v
            return destination
        return sd if not prefix else {prefix + k: v for k, v in sd.items()}

    def load_state_dict(self, state_dict, strict=True, assign=False):
        self._store.load_state_dict(state_dict, strict)
        return nn.modules.module._IncompatibleKeys([], [])

    def _require_gpu(self):
        if not self.flat.is_cuda:
            raise RuntimeError(f"{type(self).__name__}: the MI355X path runs on a HIP device; move the model "
                               "with .to('cuda') (the CPU restatement in oracle/ is test infrastructure)")


class _GenFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, flat, z, text, mod, anneal, psi, train, want8, eps, tokens=None, key_len=None):
        eng = mod._engine()
        eng.prep()
        need = any(ctx.needs_input_grad[:3]) or ctx.needs_input_grad[9]
        if tokens is not None:
            tokens = tokens.float().contiguous()
        img16, img8, kl2s, probs, _, gctx = eng.forward(z.float().contiguous(), text.float().contiguous(), eps,
                                                        anneal, psi, train=train, save=need, want_img8=want8,
                                                        text_tokens=tokens, text_len=key_len)
        out16 = img16[..., :3].permute(0, 3, 1, 2).float().contiguous()
        out8 = img8[..., :3].permute(0, 3, 1, 2).float().contiguous() if img8 is not None else z.new_zeros(0)
        if train:
            kl2 = torch.stack(kl2s)
            kl = kl2[:, 0].sum()
        else:
            kl2 = None
            kl = z.new_zeros(())
        ctx.mod, ctx.gctx, ctx.kl2, ctx.want8 = mod, gctx, kl2, want8
        ctx.mark_non_differentiable(*([] if train else [kl]))
        return (out16, out8, kl) + tuple(probs)

    @staticmethod
    def backward(ctx, g16, g8, gkl, *gprobs):
        mod, eng = ctx.mod, ctx.mod._engine()
        st = mod._store
        st.zero_grad()
        B, dev = ctx.gctx["B"], eng.dev
        R = eng.max_res
        gi16 = torch.zeros(B, R, R, 8, device=dev, dtype=eng.cdt)
        if g16 is not None:
            gi16[..., :3] = g16.permute(0, 2, 3, 1)
        gi8 = None
        if ctx.want8 and g8 is not None and g8.numel():
            gi8 = torch.zeros(B, R // 2, R // 2, 8, device=dev, dtype=eng.cdt)
            gi8[..., :3] = g8.permute(0, 2, 3, 1)
        kl_coef = None
        if ctx.kl2 is not None and gkl is not None:
            kl_coef = (gkl.float() * ctx.kl2[:, 1]).contiguous()
        gp = [None if g is None else g.float().contiguous() for g in gprobs]
        gin = eng.backward(ctx.gctx, gi16, kl_coef=kl_coef, want_input_grads=True, g_probs=gp, g_img8=gi8)
        gz, gtext = gin[0], gin[1]
        gtok = gin[2] if len(gin) > 2 else None  # the token gradient after a forward with text_tokens
        return st.grad.clone(), gz, gtext, None, None, None, None, None, None, gtok, None


class AuroraGenerator(_FlatModule):
    """Reference :668-855.  Extra keyword args: num_experts (default 4, as NUM_EXPERTS), topk (None = dense
    soft combine over all experts, as the reference trains), dtype ("fp32" | "bf16").  ``max_resolution`` 16 is
    the reference; 32 / 64 / 128 select the progressive extension (moegan_mi/layout.py gen_blocks: the output is
    R x R and ``return_intermediate`` gives the R/2 image).  ``attn_resolution`` 16 is the reference's three attention
    blocks; 32 (needs ``max_resolution`` >= 32) gives gen_block_32 the full AttentionBlock as well."""

    def __init__(self, latent_dim=LATENT_DIM, text_embedding_dim=512, max_resolution=16, num_experts=NUM_EXPERTS,
                 topk=None, dtype="fp32", seed=0, clip_grad=False, attn_resolution=16):
        if latent_dim != 512 or text_embedding_dim != 512 or max_resolution not in MAX_RESOLUTIONS:
            raise ValueError("the architecture is fixed at latent 512, text 512 and a 16x16 output (the reference) "
                             f"or one of the progressive resolutions {MAX_RESOLUTIONS[1:]}")
        # clip_grad (train_aurora_gan(clip_grad=True)): the half-resolution to_rgb trains, so it is not frozen
        super().__init__(generator_shapes(num_experts, max_resolution, attn_resolution),
                         frozen=frozen_rgb_prefixes(max_resolution, clip_grad), dtype=dtype)
        self.latent_dim, self.text_embedding_dim, self.max_resolution = latent_dim, text_embedding_dim, max_resolution
        self.attn_resolution = attn_resolution
        self.num_experts, self.topk = num_experts, topk
        self._use_checkpointing = False
        self._eng = None
        self._clip_grad = bool(clip_grad)
        object.__setattr__(self, "_ema_gen", None)
        init_generator(self._store, seed)

    def enable_ema(self):
        """Keep an exponential moving average of the parameters (ParamStore.enable_ema): TrainStep advances it
        inside the optimizer launch when StepConfig.ema_halflife is set.  Idempotent."""
        self._store.enable_ema()
        return self

    def ema_generator(self):
        """An eval-mode AuroraGenerator of the same configuration whose flat parameters ARE the moving average
        (``store.ema``: shared memory, no copy), cached.  Every call re-casts its bf16 shadow -- the optimizer
        kernel's writes to the average do not bump torch's version counter, so the refresh is forced -- and takes
        the buffers from the live store.  It owns its engine and scratch, so sampling through it leaves the training
        state (parameters, gradients, moments, buffers) untouched."""
        st = self._store
        if st.ema is None:
            raise RuntimeError("this generator keeps no moving average: train with ema_kimg / "
                               "StepConfig(ema_halflife=...) or call enable_ema() first")
        g = self._ema_gen
        if g is None or g._store.data.data_ptr() != st.ema.data_ptr() or g._store.device != st.ema.device:
            if g is None:
                g = AuroraGenerator(max_resolution=self.max_resolution, attn_resolution=self.attn_resolution,
                                    num_experts=self.num_experts, topk=self.topk,
                                    dtype="bf16" if self._cdt == torch.bfloat16 else "fp32",
                                    clip_grad=self._clip_grad)
                g.requires_grad_(False)
            g.flat.data = st.ema  # alias, not a copy
            g._store.rebind(g.flat.data)
            object.__setattr__(self, "_ema_gen", g)  # cached, not registered as a sub-module
        else:
            g._store.refresh_shadow(force=True)
        with torch.no_grad():
            for n, b in st.buffers.items():
                if g._store.buffers[n].device != b.device:
                    g._store.buffers[n] = b.detach().clone()
                else:
                    g._store.buffers[n].copy_(b)
        g.eval()
        return g

    def _engine(self):
        if self._eng is None or self._eng.st is not self._store or self._eng.dev != self._store.device:
            self._eng = GeneratorEngine(self._store, self.num_experts, self.topk, self._cdt)
        return self._eng

    def enable_checkpointing(self):
        self._use_checkpointing = True  # no-op: 288 GB HBM; math is unchanged
        return self

    def disable_checkpointing(self):
        self._use_checkpointing = False
        return self

    def encode_text(self, text_or_embeddings):
        if isinstance(text_or_embeddings, str) or (isinstance(text_or_embeddings, list)
                                                     and isinstance(text_or_embeddings[0], str)):
            model, _ = get_clip_model()
            return encode_text_with_clip(text_or_embeddings, model)
        return text_or_embeddings

    def forward(self, z, text_input, truncation_psi=0.7, return_routing=False, return_intermediate=False,
                annealing_factor=1.0, text_tokens=None, text_len=None):
        """``text_tokens`` [B, Lk, 512] (1 <= Lk <= 128; per-token text features, e.g. CLIP's token sequence
        projected to 512): the attention blocks cross-attend over text_projection applied per token instead of the
        one pooled row; ``text_len`` (list or int tensor [B], 1 <= len <= Lk) masks each image's padding tokens.
        The pooled ``text_input`` still feeds the mapping network.  Defaults: the reference's one-token path.
        This is the padded form of the autograd path; the fused TrainStep trains on the same features in packed
        form (TrainStep.step(text_rows=...), train_aurora_gan(text_tokens=True))."""
        self._require_gpu()
        text = self.encode_text(text_input)
        B = z.shape[0]
        if text.shape[0] != B:
            if text.shape[0] == 1:
                text = text.repeat(B, 1)
            else:
                raise ValueError(f"Batch size mismatch: z has batch size {B}, but text_embeddings has batch size "
                                 f"{text.shape[0]}")
        eps = _eps_for(self._store) if self.training else None
        key_len = None
        if text_tokens is not None:
            if text_tokens.dim() != 3 or text_tokens.shape[0] != B or text_tokens.shape[2] != text.shape[1]:
                raise ValueError(f"text_tokens: [{B}, Lk, {text.shape[1]}], got {tuple(text_tokens.shape)}")
            if not 1 <= text_tokens.shape[1] <= 128:
                raise ValueError("text_tokens: 1 to 128 tokens")
            key_len = _key_len(text_len, B, text_tokens.shape[1], z.device)
        elif text_len is not None:
            raise ValueError("text_len needs text_tokens")
        outs = _GenFn.apply(self.flat, z, text, self, float(annealing_factor), float(truncation_psi), self.training,
                            bool(return_intermediate), eps, text_tokens, key_len)
        img16, img8, kl = outs[0], outs[1], outs[2]
        probs = list(outs[3:])
        if return_routing and return_intermediate:
            return img16, img8, kl, probs
        if return_routing:
            return img16, None, kl, probs
        if return_intermediate:
            return img16, img8, kl
        return img16, kl


class _DiscFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, flat, img, text, mod):
        eng = mod._engine()
        eng.prep()
        logits, dctx = eng.logits(img.float(), text.float().contiguous())
        ctx.mod, ctx.dctx = mod, dctx
        return logits.reshape(-1)

    @staticmethod
    def backward(ctx, g):
        mod, eng = ctx.mod, ctx.mod._engine()
        mod._store.zero_grad()
        B = ctx.dctx["f"]["B"]
        gimg = eng.logits_backward(ctx.dctx, g.reshape(B, -1), want_input=ctx.needs_input_grad[1])
        return mod._store.grad.clone(), gimg, None, None


class AuroraDiscriminator(_FlatModule):
    """Reference :858-907 (weight_norm layers stored as weight_g / weight_v)."""

    def __init__(self, text_embedding_dim=512, max_resolution=16, dtype="fp32", seed=1):
        super().__init__(discriminator_shapes(), dtype="fp32")
        self.max_resolution = max_resolution
        self._eng = None
        self._dtype = dtype
        init_discriminator(self._store, seed)

    def _engine(self):
        if self._eng is None or self._eng.st is not self._store or self._eng.dev != self._store.device:
            cdt = torch.bfloat16 if self._dtype == "bf16" else torch.float32
            self._eng = DiscriminatorEngine(self._store, cdt)
        return self._eng

    def forward(self, img, text_embedding):
        self._require_gpu()
        return _DiscFn.apply(self.flat, img, text_embedding, self)


class VisionAidedDiscriminator(_FlatModule):
    """Vision-aided discriminator head (this build's extension, no reference counterpart; Kumari et al., "Ensembling
    off-the-shelf models for GAN training"; GigaGAN's L_vision; StyleGAN-T): a conditional head on the features of a
    frozen image tower.  With x~ / c~ the feature / caption rows scaled to norm sqrt(feature_dim),
        h = LeakyReLU_0.2(fc x~),  logit = out h + <h, text_proj c~> / sqrt(hidden)
    (include/moegan_hip.h: mg_vhead_logits; a row whose norm is zero or not finite gives logit 0).  ``forward`` is
    forward only; training runs inside the fused step (``train_aurora_gan(..., clip_grad=True, vision_d=True)``,
    StepConfig.vision_d), which owns the gradients.  ``hidden`` = 256 and the initialisation (init_vision_head) are
    choices.  state_dict keys: fc.weight, fc.bias, text_proj.weight, text_proj.bias, out.weight, out.bias."""

    def __init__(self, feature_dim=512, hidden=256, seed=2):
        super().__init__(vision_head_shapes(feature_dim, hidden), dtype="fp32")
        self.feature_dim, self.hidden = int(feature_dim), int(hidden)
        init_vision_head(self._store, seed)

    @torch.no_grad()
    def forward(self, features, text_embedding):
        """features [B, feature_dim] (the tower's image features), text_embedding [B, feature_dim] -> logits [B]."""
        self._require_gpu()
        from moegan_mi import ops
        params = {k: self._store.view(k) for k in ops.VHEAD_KEYS}
        return ops.vhead_logits(features.float(), text_embedding.float(), params)


def encode_text_with_clip(text, model=None):
    model = model or get_clip_model()[0]
    if isinstance(text, str):
        text = [text]
    if hasattr(model, "tokenize"):  # the project's own text tower with its tokenizer (load_clip_weights(bpe_path=))
        with torch.no_grad():
            return model.encode_text(model.tokenize(text)).float()
    import clip  # a locally provided CLIP package
    with torch.no_grad():
        return model.encode_text(clip.tokenize(text).to(DEVICE)).float()


def encode_prompt(text, model=None):
    """Prompt(s) -> (pooled [N, 512], tokens [N, Lk, 512], text_len int32 [N]) on the registered text tower
    (moegan_mi/clip_text.py): the pooled row feeds the mapping network, ``tokens`` / ``text_len`` are
    AuroraGenerator.forward's ``text_tokens=`` / ``text_len=``."""
    model = model or get_clip_model()[0]
    if not hasattr(model, "tokenize"):
        raise RuntimeError("encode_prompt needs the text tower and its tokenizer: load_clip_weights(path, bpe_path=...)")
    if isinstance(text, str):
        text = [text]
    with torch.no_grad():
        pooled, tokens, text_len = model.encode_text(model.tokenize(text), return_tokens=True)
    return pooled.float(), tokens.float(), text_len


class _ClipLossFn(torch.autograd.Function):
    """1 - mean cos(CLIP(image), text) with d loss / d image through the build's frozen image tower
    (moegan_mi/clip_vit.py encode_generated(save=True) / backward); images NCHW [B, 3, R, R], text [B, 512]."""

    @staticmethod
    def forward(ctx, images, text, tower, temperature=None):
        from moegan_mi import ops
        B, _, R, _ = images.shape
        nhwc = torch.zeros(B, R, R, 8, device=images.device, dtype=torch.float32)
        nhwc[..., :3] = images.detach().float().permute(0, 2, 3, 1)
        feats, tctx = tower.encode_generated(nhwc, save=True)
        one = torch.ones(1, device=images.device)
        t32 = text.detach().float().contiguous()
        if temperature is None:
            loss, g_f = ops.cos_loss(feats, t32, one)
        else:  # contrastive over the batch's captions, row i's own caption the positive (ops.clip_contrast)
            loss, g_f = ops.clip_contrast(feats, t32, temperature, one)
        ctx.tower, ctx.tctx, ctx.g_f, ctx.nhwc, ctx.in_dtype = tower, tctx, g_f, nhwc, images.dtype
        return loss.reshape(())

    @staticmethod
    def backward(ctx, g):
        g_img = torch.zeros_like(ctx.nhwc)
        ctx.tower.backward(ctx.tctx, ctx.g_f, g_img)
        return (g_img[..., :3].permute(0, 3, 1, 2) * g).to(ctx.in_dtype), None, None, None


class CLIPLoss(nn.Module):
    """Reference :66-119 -- forward-only, no gradient (the image branch runs under no_grad).
    ``differentiable=True`` (this build's extension): ``loss.backward()`` reaches the image through the registered
    image tower's own backward; it needs the build's tower (load_clip_weights), not a foreign CLIP model.
    ``contrastive=True`` (needs ``differentiable=True``): the loss is the softmax cross-entropy of each image against
    the batch's captions at ``temperature`` (its own caption the positive) instead of 1 - mean cos; 0.07 is CLIP's
    initial temperature, a choice and not a measurement (the weight loaders drop the checkpoint's logit_scale)."""

    def __init__(self, device=DEVICE, differentiable=False, contrastive=False, temperature=0.07):
        super().__init__()
        self.device = device
        self.differentiable = bool(differentiable)
        self.contrastive = bool(contrastive)
        if self.contrastive and not self.differentiable:
            raise ValueError("CLIPLoss(contrastive=True) needs differentiable=True")
        if not float(temperature) > 0 or float(temperature) == float("inf"):
            raise ValueError(f"temperature must be positive and finite, got {temperature}")
        self.temperature = float(temperature)

    def forward(self, images, text_embeddings):
        if images is None or _clip_model is None:
            return torch.tensor(0.0, device=self.device)
        if self.differentiable:
            from moegan_mi.step import clip_tower
            tower = clip_tower(_clip_model)
            if tower is None:
                raise RuntimeError("CLIPLoss(differentiable=True) needs the build's image tower "
                                   "(t2i_moe_gan.load_clip_weights); the registered model has no backward")
            return _ClipLossFn.apply(images, text_embeddings, tower, self.temperature if self.contrastive else None)
        with torch.no_grad():
            im = torch.clamp(images, -1, 1)
            if im.shape[-1] != 224 or im.shape[-2] != 224:
                im = F.interpolate(im, size=(224, 224), mode="bilinear", align_corners=False)
            f = _clip_model.encode_image(im).float()
            f = f / f.norm(dim=-1, keepdim=True)
            t = text_embeddings / text_embeddings.norm(dim=-1, keepdim=True)
            sim = torch.nan_to_num((f * t).sum(dim=1))
            return 1.0 - sim.mean()


class AuroraGANLoss:
    """Reference :909-1000 (loss values on logits; the fused step uses the HIP loss kernels)."""

    def __init__(self, device=DEVICE):
        self.device = device
        self.clip_loss_fn = CLIPLoss(device)

    def generator_loss(self, fake_pred, kl_loss=None, kl_weight=0.001):
        g = F.softplus(-fake_pred).mean()
        return g + kl_weight * kl_loss if kl_loss is not None else g

    def compute_clip_loss(self, images, text_input):
        return self.clip_loss_fn(images, text_input.to(images.device))

    def discriminator_loss(self, real_pred, fake_pred, mismatched_pred):
        return F.softplus(-real_pred).mean() + F.softplus(fake_pred).mean() + F.softplus(mismatched_pred).mean()

    def moe_balance_loss(self, routing_probs, balance_weight=0.01):
        if not routing_probs:
            return torch.tensor(0.0, device=self.device)
        p = routing_probs[-1]
        if p is None or p.numel() == 0:
            return torch.tensor(0.0, device=self.device)
        E, T = p.size(1), p.size(0)
        frac = (p.sum(dim=0) + 1e-6) / T
        cv = torch.std(frac) / (torch.mean(frac) + 1e-6)
        return balance_weight * torch.nan_to_num(torch.clamp(E * cv, 0.0, 10.0), nan=0.0)


def _lr_schedule(lr, num_epochs, lr_warmup_epochs):
    """Per-epoch learning rates of the reference (warmup, then CosineAnnealingLR stepped per epoch,
    :1108-1118, :1149-1166, :1514-1516), replayed with torch's own scheduler on a dummy parameter."""
    p = torch.nn.Parameter(torch.zeros(1))
    opt = torch.optim.AdamW([p], lr=lr)
    sch = torch.optim.lr_scheduler.CosineAnnealingLR(opt, T_max=max(1, num_epochs - lr_warmup_epochs),
                                                     eta_min=lr * 0.05)
    out = []
    for epoch in range(num_epochs):
        if epoch < lr_warmup_epochs:
            for g in opt.param_groups:
                g["lr"] = lr * (0.1 + 0.9 * (epoch / lr_warmup_epochs))
        out.append(opt.param_groups[0]["lr"])
        if epoch >= lr_warmup_epochs:
            opt.step()
            sch.step()
    return out


class _StepRunner:
    """Runs the batch body (TrainStep.step) of train_aurora_gan the way bench.py times it: captured once per
    variant as a chain of hipGraphs (moegan_mi/graphs.py) and replayed on fixed input buffers.

    A variant is everything the step bakes into its launches: the batch shape, the epoch's learning rate,
    router temperature factor and effective KL weight, and the accumulation window position (zero_grads /
    step_optim).  The first batch of a new variant runs eagerly on the capture stream -- a real training step
    that also sizes every lazily allocated buffer -- and the variant is captured right after it (a capture
    executes nothing), so every later batch of it is one replay.  Graphs of a finished epoch are released when
    the epoch's scalars change.  A batch whose shape differs from the loader's first batch (a ragged last batch)
    runs eagerly without capture.  ``enabled=False`` (or a non-HIP device) runs every batch eagerly.

    All variants share one capture stream (one library workspace) and one graph memory pool: they replay one at
    a time on the same stream, so the step temporaries of one variant may reuse another's (with
    acc = 8 the loop keeps three variants alive).  A variant's output tensors are private only against variants
    captured BEFORE it: a later capture may place its temporaries in blocks that hold an earlier variant's outputs.
    Invariant: a variant's outputs are read or copied (train_aurora_gan: _stats_to_host, in stream order right after
    the replay) before any other variant replays.  tests/test_loop_gpu.py checks the returned values across the
    variant switches of an acc > 1 window and measures the loop's peak memory.

    A token batch (``text_rows`` / ``row_off`` / ``lk_max``, moegan_mi.tokens) adds its two buckets (rows, lk_max)
    to the variant key, with static buffers for the packed rows and the offsets.  At most ``MAX_TOKEN_VARIANTS``
    token variants are kept per epoch; a batch that would need one more runs eagerly.

    ``aug`` (the augmentation parameters of StepConfig.diffaug, [3, B, 8]) is an input like ``perm``: a static buffer
    per variant, refilled before every replay."""

    MAX_TOKEN_VARIANTS = 8

    def __init__(self, ts, device, enabled=True):
        self.ts = ts
        self.enabled = bool(enabled) and torch.device(device).type == "cuda"
        self.graphs = {}
        self.epoch_key = None
        self.shape = None
        self.stream = self.pool = None

    def __call__(self, real, text, z, eps_d, eps_g, perm, **kw):
        if not self.enabled:
            return self.ts.step(real, text, z, eps_d, eps_g, perm, **kw)
        from moegan_mi.graphs import SegmentedGraph
        if self.shape is None:
            self.shape = tuple(real.shape)
        if tuple(real.shape) != self.shape:
            return self.ts.step(real, text, z, eps_d, eps_g, perm, **kw)
        ekey = (kw["anneal"], kw["lr_g"], kw["lr_d"], kw["eff_kl_weight"], kw.get("acc", 1))
        if ekey != self.epoch_key:
            self.graphs.clear()  # the previous epoch's graphs go, and with the last of them their memory pool
            self.pool = None  # (a released pool cannot be captured into again: the next capture makes a new one)
            self.epoch_key = ekey
        key = (kw.get("zero_grads", True), kw.get("step_optim", True))
        text_rows, row_off, aug = kw.get("text_rows"), kw.get("row_off"), kw.get("aug")
        if text_rows is not None:
            key += (int(text_rows.shape[0]), int(kw["lk_max"]))
        ent = self.graphs.get(key)
        if ent is None:
            if text_rows is not None and sum(len(k) > 2 for k in self.graphs) >= self.MAX_TOKEN_VARIANTS:
                return self.ts.step(real, text, z, eps_d, eps_g, perm, **kw)
            bufs = dict(real=real.clone(), text=text.clone(), z=z.clone(),
                        eps_d=[tuple(t.clone() for t in trip) for trip in eps_d], eps_g=eps_g, perm=perm.clone())
            kws = dict(kw)
            if text_rows is not None:
                bufs.update(text_rows=text_rows.clone(), row_off=row_off.clone())
                kws.update(text_rows=bufs["text_rows"], row_off=bufs["row_off"])
            if aug is not None:
                bufs.update(aug=aug.clone())
                kws.update(aug=bufs["aug"])

            def fn(b=bufs, kw=kws):
                return self.ts.step(b["real"], b["text"], b["z"], b["eps_d"], b["eps_g"], b["perm"], **kw)
            if self.stream is None:
                self.stream = torch.cuda.Stream()
            g = SegmentedGraph(stream=self.stream, pool=self.pool)
            out = g.run_eager(fn)  # this batch, eagerly
            outg = g.capture(fn)
            self.pool = g.pool
            self.graphs[key] = (g, outg, bufs)
            return out
        g, outg, b = ent
        with torch.no_grad():
            b["real"].copy_(real)
            b["text"].copy_(text)
            b["z"].copy_(z)
            b["perm"].copy_(perm)
            if text_rows is not None:
                b["text_rows"].copy_(text_rows)
                b["row_off"].copy_(row_off)
            if aug is not None:
                b["aug"].copy_(aug)
            for dst, src in zip(b["eps_d"], eps_d):
                for x, y in zip(dst, src):
                    x.copy_(y)
            for dst, src in zip(b["eps_g"], eps_g):
                for x, y in zip(dst, src):
                    if x.data_ptr() != y.data_ptr():
                        x.copy_(y)
        g.replay()
        return outg


class _NoEvent:
    def synchronize(self):
        pass


_STAT_KEYS = ("flags", "d_losses", "r1", "g_gan", "balance", "kl", "clip16", "clip8")


def _stats_to_host(out, keys=_STAT_KEYS):
    """The step's guard word and logged losses as one asynchronous copy into pinned host memory (read after the
    NEXT batch is enqueued, so the host never waits for the batch it just launched)."""
    vals = [out["flags"][:1].float()] + [out[k].reshape(-1)[:1].float() if out.get(k) is not None
                                         else torch.zeros(1, device=out["flags"].device) for k in keys[1:]]
    dev_vec = torch.cat(vals)
    host = torch.empty(dev_vec.shape, dtype=torch.float32, pin_memory=True)
    host.copy_(dev_vec, non_blocking=True)
    ev = torch.cuda.Event()
    ev.record()
    return host, ev


def train_aurora_gan(dataloader, val_dataloader=None, num_epochs=50, lr=0.0002, beta1=0.5, beta2=0.999,
                     r1_gamma=10.0, clip_weight_16=0.1, clip_weight_8=0.05, kl_weight=0.001, kl_annealing_epochs=5,
                     lr_warmup_epochs=3, balance_weight=0.01, device=DEVICE, save_dir="./aurora_checkpoints",
                     log_interval=10, save_interval=1000, metric_callback=None, use_amp=True,
                     gradient_accumulation_steps=8, checkpoint_activation=True, batch_memory_limit=20.0,
                     max_resolution=16, *, clip_weight_64=None, clip_weight_32=None, num_experts=NUM_EXPERTS,
                     topk=None, dtype=None, process_group=None, seed=0, resume_from=None, save_every_epoch=False,
                     use_graphs=True, on_batch_done=None, text_tokens=False, max_text_tokens=None, clip_grad=False,
                     ema_kimg=None, ema_rampup=0.05, eval_every=None, eval_samples=None, eval_truncation_psi=1.0,
                     eval_nearest_k=None, eval_frechet=False, diffaug=None, clip_contrastive=False,
                     clip_temperature=0.07, vision_d=False, vision_weight=1.0, attn_resolution=16):
    """Reference :1029-1669.  ``clip_weight_64``/``clip_weight_32`` (the names train_model.py passes,
    SURVEY.md §0) map to the 16x16 / 8x8 CLIP weights.  ``use_amp`` selects bf16 (the MI355X mixed
    precision; the reference's fp16 GradScaler is not needed) unless ``dtype`` is given.

    Data parallel (``process_group``, one process per GPU): z and the mismatch permutation come from a per-rank
    generator, the router noise from a generator seeded identically on every rank (one weight sample per
    forward for the whole global batch); a DistributedSampler is re-seeded every epoch
    (``set_epoch``); validation runs on every rank's shard and its sums are all-reduced, and the early-stop
    decision of ``metric_callback`` (called on rank 0) is broadcast so every rank leaves the loop together.

    Loss guards (:1315-1320, :1367-1376, :1396-1399) run inside the step on the device; the loop reads the
    step's flag word once per batch to print the reference's warnings and to not count a skipped batch.  That
    read (with the logged losses, one pinned copy) is deferred until the next batch has been enqueued.
    ``use_graphs``: every batch body is a replayed hipGraph (``_StepRunner``, bench.py's launch mode).
    ``on_batch_done(epoch, batch_idx, flags)``: called when a batch's results have reached the host (bench.py
    --loop); ``flags`` is the batch's guard word (bit 0: non-finite D loss, bit 1: non-finite G loss).
    ``text_tokens``: the loaders yield (images, text, text_rows, row_off, lk_max) batches (moegan_mi.tokens:
    ProcessedTokenDataset / collate_tokens) and the generator's cross-attention trains on each caption's token
    rows, through the same captured step; validation feeds the same rows to the generator module.
    ``max_text_tokens``: the caption length the loaders were built with (ProcessedTokenDataset truncates); a
    batch whose key bucket exceeds it is an error.
    ``clip_grad``: the two CLIP terms carry their gradient into the generator (StepConfig.clip_grad; this build's
    extension, the reference's terms are gradient-free): needs the build's image tower registered
    (load_clip_weights); to_rgb_8 then trains and its AdamW state is part of the resume checkpoint.
    ``clip_contrastive`` (needs ``clip_grad``; off = the cosine terms): the two CLIP terms become the contrastive
    loss over the global batch's captions at ``clip_temperature`` (StepConfig.clip_loss / clip_temperature; 0.07 is
    CLIP's initial temperature, a choice and not a measurement); validation's CLIP value stays the cosine.
    ``ema_kimg`` (this build's extension; None = off, the reference's loop): keep an exponential moving average of
    the generator with this half-life in thousands of images (StyleGAN's convention), converted to optimizer steps
    with images per step = dataloader.batch_size x gradient_accumulation_steps x world; ``ema_rampup`` caps the
    half-life at that fraction of the optimizer steps taken so far (0 / None: constant).  The average is advanced
    inside the generator's optimizer launch (StepConfig.ema_halflife), sampled with ``generator.ema_generator()``
    / ``sample_aurora_gan(use_ema=True)`` and saved as ``generator_ema``; validation stays on the live generator.
    ``eval_every`` (this build's extension; None / 0 = off, the loop as it was): every that many epochs, after the
    validation pass, ``evaluate_aurora_gan`` runs on the validation loader -- on the moving average when one is kept,
    else on the live generator -- with at most ``eval_samples`` samples at ``eval_truncation_psi``, and
    ``val_kid_clip`` / ``val_clip_score`` / ``val_r_precision`` / ``val_eval_images`` join the dict
    ``metric_callback`` receives.  It needs ``val_dataloader`` and the build's image tower (load_clip_weights).
    ``eval_nearest_k`` (None = off; needs ``eval_every``): that evaluation also measures improved precision / recall
    and density / coverage with this many nearest neighbours (moegan_mi.evaluate.prdc), and ``val_precision`` /
    ``val_recall`` / ``val_density`` / ``val_coverage`` join the dict and the logged line.
    ``eval_frechet`` (off; needs ``eval_every``): that evaluation also measures the Fréchet distance between the
    generated and the validation images' tower features (moegan_mi.evaluate.frechet_distance), and ``val_fd_clip``
    joins the dict and the logged line.
    ``diffaug`` (this build's extension; None = off, the reference's loop): a differentiable-augmentation policy, any
    comma-separated subset of ``color,translation,cutout`` (moegan_mi.augment): every image the discriminator sees in
    a training step, real and fake, goes through a random colour / shift / cutout transform whose parameters are
    drawn per batch from the per-rank generator -- only when the feature is on, so the default random streams and
    resume files are unchanged.  Validation, evaluation, sampling and the CLIP terms see un-augmented images.
    ``vision_d`` (this build's extension; needs ``clip_grad``; off = the loop as it was): a vision-aided
    discriminator head (VisionAidedDiscriminator, StepConfig.vision_d) judges real and generated images in the frozen
    tower's feature space next to the reference's discriminator; its generator-side loss enters with
    ``vision_weight`` (1.0 is a choice, not a measurement).  The logged line and the dict ``metric_callback`` receives
    gain ``d_vision`` / ``g_vision`` (the last logged batch's head losses); resume files gain ``vision_head`` /
    ``optimizer_v``.  Validation is unchanged.
    ``resume_from``: a resume checkpoint (:1484-1491 layout, ours or the reference's) to start from;
    ``save_every_epoch``: write that layout after every epoch (the reference's commented-out :1642-1652).

    Accepted and not applied: ``batch_memory_limit`` (the reference's per-batch ``memory_allocated()`` check that
    skips a batch above the limit and doubles the accumulation after three skips, :1231-1259) and
    ``checkpoint_activation`` (recomputation that changes memory, not math, :734-760).  Here every batch body is
    the same preallocated step (one hipGraph per variant), so its memory is fixed before the first batch: a
    per-batch check would give the same answer for every batch, and with 288 GB of HBM per GPU the C2 step fits
    many times over.  The loop logs the step's allocated memory against the limit once, after the first batch."""
    if diffaug is not None:
        from moegan_mi.augment import parse_policy
        parse_policy(diffaug)  # an unknown name is an error before anything is created or built
    os.makedirs(save_dir, exist_ok=True)
    if clip_weight_64 is not None:
        clip_weight_16 = clip_weight_64
    if clip_weight_32 is not None:
        clip_weight_8 = clip_weight_32
    device = torch.device(device)
    if dtype is None:
        dtype = "bf16" if use_amp else "fp32"
    dist = None
    rank, world = 0, 1
    if process_group is not None:
        import torch.distributed as dist
        rank, world = dist.get_rank(process_group), dist.get_world_size(process_group)
    acc = max(1, int(gradient_accumulation_steps))
    ema_halflife = None
    if ema_kimg is not None:
        ema_kimg = float(ema_kimg)
        bs = getattr(dataloader, "batch_size", None)
        if not bs:
            raise ValueError("ema_kimg converts thousands of images to optimizer steps and needs "
                             "dataloader.batch_size; this loader has none (a batch_sampler?)")
        if not ema_kimg > 0:
            raise ValueError(f"ema_kimg must be positive, got {ema_kimg}")
        ema_halflife = ema_kimg * 1000.0 / (int(bs) * acc * world)
    eval_every = int(eval_every) if eval_every else 0
    if eval_every < 0:
        raise ValueError(f"eval_every must be a positive number of epochs, got {eval_every}")
    if eval_every:
        from moegan_mi.step import clip_tower
        if val_dataloader is None:
            raise ValueError("eval_every needs a val_dataloader: the evaluation runs on the validation set")
        if clip_tower(_clip_model) is None:
            raise ValueError("eval_every needs the build's CLIP image tower: call load_clip_weights(path) first")
    if eval_nearest_k is not None:
        eval_nearest_k = int(eval_nearest_k)
        if not eval_every:
            raise ValueError("eval_nearest_k needs eval_every: it adds to that evaluation")
        if eval_nearest_k < 1:
            raise ValueError(f"eval_nearest_k must be a positive number of neighbours, got {eval_nearest_k}")
    eval_frechet = bool(eval_frechet)
    if eval_frechet and not eval_every:
        raise ValueError("eval_frechet needs eval_every: it adds to that evaluation")
    # max_resolution 16 is the reference generator; 32 / 64 / 128 train the progressive extension (layout.py)
    if clip_contrastive and not clip_grad:
        raise ValueError("clip_contrastive=True needs clip_grad=True (the gradient-free terms stay the cosine)")
    if vision_d and not clip_grad:
        raise ValueError("vision_d=True needs clip_grad=True (the head's generator gradient goes through the "
                         "build's own image-tower backward)")
    if clip_grad and _clip_model is None:
        raise RuntimeError("clip_grad=True needs the CLIP image tower: call load_clip_weights(path) first")
    generator =AuroraGenerator(num_experts=num_experts, topk=topk, dtype=dtype, seed=seed,
                                max_resolution=max_resolution, clip_grad=clip_grad,
                                attn_resolution=attn_resolution).to(device)
    discriminator = AuroraDiscriminator(dtype=dtype, seed=seed + 1).to(device)
    if checkpoint_activation:
        generator.enable_checkpointing()
    cfg = StepConfig(E=num_experts, topk=topk, dtype=dtype, r1_gamma=r1_gamma, clip_weight_16=clip_weight_16,
                     clip_weight_8=clip_weight_8, balance_weight=balance_weight, beta1=beta1, beta2=beta2,
                     max_res=max_resolution, clip_grad=clip_grad, ema_halflife=ema_halflife,
                     ema_rampup=float(ema_rampup) if ema_rampup is not None else None, diffaug=diffaug,
                     clip_loss="contrastive" if clip_contrastive else "cosine", clip_temperature=clip_temperature,
                     vision_d=bool(vision_d), vision_weight=vision_weight, attn_res=attn_resolution)
    vision_head = None
    if vision_d:
        from moegan_mi.step import clip_tower
        tower = clip_tower(_clip_model)
        if tower is None:
            raise ValueError("vision_d=True needs the build's CLIP image tower: call load_clip_weights(path) first")
        vision_head = VisionAidedDiscriminator(int(tower.output_dim), cfg.vision_hidden, seed=seed + 2).to(device)
    # CLIP terms of the generator loss (logging / guard only unless clip_grad: no gradient, :98-101)
    ts = TrainStep(cfg, device, process_group=process_group, gstore=generator._store, dstore=discriminator._store,
                   clip_encoder=_clip_model.encode_image if _clip_model is not None else None,
                   vstore=vision_head._store if vision_head is not None else None)
    stat_keys = _STAT_KEYS + (("vis_d", "vis_g") if vision_d else ())
    last_vision = {}
    if rank == 0:
        print(f"Generator parameters: {generator._store.n_opt + (generator._store.total - generator._store.n_opt):,}")
    lrs = _lr_schedule(lr, num_epochs, lr_warmup_epochs)
    gan_loss = AuroraGANLoss(device)
    # randomness: per-rank z / permutation, rank-shared router noise
    g_local = torch.Generator(device=device).manual_seed(1_000_003 * (seed + 1) + 7919 * rank)
    g_shared = torch.Generator(device=device).manual_seed(1_000_003 * (seed + 1) + 17)
    start_epoch, step = 0, 0
    if resume_from is not None:  # also continues the z / permutation / router-noise streams when the file has them
        start_epoch, step = load_resume(resume_from, generator, discriminator,
                                        generators={f"local{rank}": g_local, "shared": g_shared},
                                        vision_head=vision_head)
        print(f"Resumed from {resume_from}: epoch {start_epoch}, step {step}")
    from tqdm import tqdm
    runner = _StepRunner(ts, device, enabled=use_graphs)
    for epoch in range(start_epoch, num_epochs):
        cur_lr = lrs[epoch]
        kl_warmup = min(1.0, (epoch / kl_annealing_epochs) ** 2)
        eff_kl = kl_weight * (1e-5 + (1.0 - 1e-5) * kl_warmup)
        temperature_factor = max(1.0, 3.0 - epoch * 0.1)
        sampler = getattr(dataloader, "sampler", None)
        if hasattr(sampler, "set_epoch"):
            sampler.set_epoch(epoch)
        if rank == 0:
            print(f"\n{'=' * 20} Epoch {epoch + 1}/{num_epochs} {'=' * 20}")
            print(f"  LR: {cur_lr:.6f}  Temperature factor: {temperature_factor:.2f}  "
                  f"Effective KL weight: {eff_kl:.8f}")
        # batch i+1's host -> HBM copy overlaps batch i's step (moegan_mi/prefetch.py)
        pbar = tqdm(DevicePrefetcher(dataloader, device), desc=f"Epoch {epoch + 1}/{num_epochs}", disable=rank != 0)
        n_batches = len(dataloader)
        pending = None

        def account(rec):
            """The reference's per-batch host work for a finished batch (:1315-1320 warnings, :1441-1471 logging)."""
            nonlocal step
            host, ev, bidx = rec
            ev.synchronize()
            v = host.tolist()
            flags = int(v[0])
            if on_batch_done is not None:
                on_batch_done(epoch, bidx, flags)
            if flags & 1:
                print("⚠️ NaN/Inf detected in discriminator loss! Skipping this batch.")
                return
            if flags & 2:
                print("⚠️ NaN or Inf detected in generator loss! Resetting to zero.")
            if step % log_interval == 0 and rank == 0:
                d_gan, r1, g_gan, bal, kl, c16, c8 = v[1:8]
                g_loss = 0.0 if flags & 2 else g_gan + clip_weight_16 * c16 + clip_weight_8 * c8 + bal
                g_loss += eff_kl * kl
                logger.info(f"\nStep [{step}] Epoch [{epoch + 1}] Batch [{bidx}/{n_batches}] "
                            f"D_loss: {d_gan + r1:.4f} (GAN: {d_gan:.4f}, R1: {r1:.4f}), "
                            f"G_loss: {g_loss:.4f} (GAN: {g_gan:.4f}, Clip16: {c16:.4f}, Clip8: {c8:.4f}, "
                            f"KL: {kl:.4f}, Balance: {bal:.4f})")
                pbar.set_postfix({"D_loss": f"{d_gan:.3f}", "R1": f"{r1:.3f}", "G_loss": f"{g_gan:.3f}",
                                  "KL": f"{kl:.4f}", "Balance": f"{bal:.4f}", "Clip16": f"{c16:.3f}",
                                  "Clip8": f"{c8:.3f}"})
                if vision_d:
                    last_vision.update(d_vision=v[8], g_vision=v[9])
                    logger.info(f"  Vision head: D_vision: {v[8]:.4f}, G_vision: {v[9]:.4f} "
                                f"(weight {float(vision_weight):g})")
            step += 1
        for batch_idx, batch in enumerate(pbar):
            real, text = batch[0], batch[1]
            tok_kw = {}
            if text_tokens:
                if len(batch) != 5:
                    raise ValueError("text_tokens=True needs (images, text, text_rows, row_off, lk_max) batches "
                                     "(moegan_mi.tokens.collate_tokens)")
                tok_kw = dict(text_rows=batch[2].to(device, non_blocking=True).float(),
                              row_off=batch[3].to(device, non_blocking=True).int(), lk_max=int(batch[4]))
                if max_text_tokens is not None and tok_kw["lk_max"] > -(-int(max_text_tokens) // 32) * 32:
                    raise ValueError(f"a batch with captions of up to {tok_kw['lk_max']} tokens: the dataset was "
                                     f"not built with max_tokens={max_text_tokens}")
            real = real.to(device, non_blocking=True).float()
            text = text.to(device, non_blocking=True).float()
            B = real.shape[0]
            z = torch.randn(B, LATENT_DIM, device=device, generator=g_local)
            eps_d = [tuple(t.clone() for t in trip) for trip in _eps_for(generator._store, g_shared)]
            eps_g = _eps_for(generator._store, g_shared)
            perm = torch.randperm(B, device=device, generator=g_local).int()
            aug_kw = {}
            if diffaug is not None:  # (drawn only when on: the default streams stay as they were)
                from moegan_mi.augment import draw
                aug_kw = dict(aug=draw(B, g_local))
            zero = batch_idx % acc == 0
            stp = (batch_idx + 1) % acc == 0 or (batch_idx + 1) == n_batches
            out = runner(real, text, z, eps_d, eps_g, perm, anneal=temperature_factor, lr_g=cur_lr, lr_d=cur_lr,
                         eff_kl_weight=eff_kl, acc=acc, zero_grads=zero, step_optim=stp, **tok_kw, **aug_kw)
            if device.type == "cuda":
                rec = _stats_to_host(out, stat_keys) + (batch_idx,)
            else:
                rec = (torch.stack([out[k].reshape(-1)[0].float() if out.get(k) is not None else torch.zeros(())
                                    for k in stat_keys]), _NoEvent(), batch_idx)
            if pending is not None:
                account(pending)  # the previous batch, now that this one is enqueued
            pending = rec
            if batch_idx == 0 and epoch == start_epoch and rank == 0 and device.type == "cuda" and batch_memory_limit:
                gb = torch.cuda.memory_allocated(device) / 1e9
                logger.info(f"batch_memory_limit={batch_memory_limit}GB is not applied (the step's memory is fixed): "
                            f"{gb:.2f}GB allocated after the first batch")
        if pending is not None:
            account(pending)
        pbar.close()
        if val_dataloader is not None:
            vm = _validate(generator, discriminator, val_dataloader, gan_loss, temperature_factor, eff_kl, device,
                           process_group, g_local)
            if eval_every and (epoch + 1) % eval_every == 0:
                from moegan_mi.evaluate import format_metrics
                em = evaluate_aurora_gan(generator, val_dataloader, num_samples=eval_samples,
                                         truncation_psi=eval_truncation_psi, seed=seed,
                                         use_ema=generator._store.ema is not None, process_group=process_group,
                                         nearest_k=eval_nearest_k, frechet=eval_frechet)
                vm.update(val_kid_clip=em["kid_clip"], val_clip_score=em["clip_score"],
                          val_r_precision=em["r_precision"], val_eval_images=em["n"])
                if eval_nearest_k is not None:
                    vm.update(val_precision=em["precision"], val_recall=em["recall"], val_density=em["density"],
                              val_coverage=em["coverage"])
                if eval_frechet:
                    vm.update(val_fd_clip=em["fd_clip"])
                if rank == 0:
                    print(f"Evaluation ({'EMA' if generator._store.ema is not None else 'live'} generator) - "
                          f"{format_metrics(em)}")
            vm.update(last_vision)
            stop = False
            if rank == 0:
                print(f"Validation Results - D_loss: {vm['val_d_loss']:.4f}, G_loss: {vm['val_g_loss']:.4f}, "
                      f"Clip_Loss_16: {vm['val_clip_loss_16']:.4f}, Clip_Loss_8: {vm['val_clip_loss_8']:.4f}")
                stop = bool(metric_callback and not metric_callback(epoch, vm))
            if dist is not None:  # every rank leaves together (the next all-reduce would otherwise hang)
                flag = torch.tensor([1 if stop else 0], device=device, dtype=torch.int32)
                dist.broadcast(flag, src=dist.get_global_rank(process_group, 0), group=process_group)
                stop = bool(flag.item())
        else:
            stop = False
        if save_every_epoch:  # after validation (which draws from g_local), every rank's local stream
            _save_epoch(save_dir, generator, discriminator, epoch, step, cur_lr, (beta1, beta2), g_local, g_shared,
                        process_group, rank, vision_head=vision_head)
        if stop:
            if rank == 0:
                print("Early stopping triggered by metric callback")
            break
    return generator, discriminator


def _save_epoch(save_dir, generator, discriminator, epoch, step, cur_lr, betas, g_local, g_shared, process_group,
                rank, vision_head=None):
    """End-of-epoch resume file (the reference's commented-out :1642-1652 layout, 'epoch' = epoch + 1), written by
    rank 0 with every rank's local generator state (``rng/local<r>``) gathered over the process group."""
    states = {f"local{rank}": g_local.get_state()}
    if process_group is not None:
        import torch.distributed as dist
        got = [None] * dist.get_world_size(process_group)
        dist.all_gather_object(got, (rank, g_local.get_state()), group=process_group)
        states = {f"local{r}": st for r, st in got}
    if rank == 0:
        states["shared"] = g_shared.get_state()
        save_resume(os.path.join(save_dir, f"aurora_checkpoint_epoch_{epoch + 1}.pt"), generator, discriminator,
                    epoch, step, cur_lr, cur_lr, betas, epoch_complete=True, generators=states,
                    vision_head=vision_head)


def _validate(generator, discriminator, loader, gan_loss, temperature_factor, eff_kl, device, process_group=None,
              gen=None):
    """Reference validation loop :1519-1639 (eval-mode generator: mean router weights, hard top-1).  Under data
    parallelism each rank evaluates its shard and the per-sample sums are all-reduced."""
    generator.eval()
    discriminator.eval()
    keys = ("val_d_loss", "val_g_loss", "val_clip_loss_16", "val_clip_loss_8")
    tot = torch.zeros(len(keys) + 1, dtype=torch.float64)
    with torch.no_grad():
        for batch in loader:
            real, text = batch[0].to(device).float(), batch[1].to(device).float()
            B = real.shape[0]
            z = torch.randn(B, LATENT_DIM, device=device, generator=gen)
            tok_kw = {}
            if len(batch) == 5:  # a token batch (moegan_mi.tokens.collate_tokens): the module takes the padded form
                from moegan_mi.tokens import unpack_tokens
                tok, tlen = unpack_tokens(batch[2].to(device).float(), batch[3].to(device), int(batch[4]))
                tok_kw = dict(text_tokens=tok, text_len=tlen)
            f16, f8, kl = generator(z, text, return_intermediate=True, annealing_factor=temperature_factor, **tok_kw)
            rp = discriminator(real, text)
            fp = discriminator(f16, text)
            mp = discriminator(real, text[torch.randperm(B, device=device, generator=gen)])
            vals = (gan_loss.discriminator_loss(rp, fp, mp), gan_loss.generator_loss(fp, kl, kl_weight=eff_kl),
                    gan_loss.compute_clip_loss(f16, text), gan_loss.compute_clip_loss(f8, text))
            tot += torch.tensor([float(v) * B for v in vals] + [B], dtype=torch.float64)
    if process_group is not None:
        import torch.distributed as dist
        t = tot.to(device)
        dist.all_reduce(t, group=process_group)
        tot = t.cpu()
    generator.train()
    discriminator.train()
    n = max(float(tot[-1]), 1.0)
    vm = {k: float(tot[i]) / n for i, k in enumerate(keys)}
    vm["val_clip_loss"] = vm["val_clip_loss_16"]
    return vm


def evaluate_aurora_gan(generator, dataloader, **kw):
    """KID / CLIP score / R-precision of ``generator`` over the registered image tower's features
    (moegan_mi.evaluate.evaluate_generator; its keywords: num_samples, truncation_psi, seed, use_ema, group,
    process_group, return_features, nearest_k, which adds precision / recall / density / coverage, and frechet /
    reference_stats, which add the Fréchet distance 'fd_clip').  This build's extension; needs load_clip_weights."""
    from moegan_mi.evaluate import evaluate_generator
    from moegan_mi.step import clip_tower
    tower = clip_tower(_clip_model)
    if tower is None:
        raise RuntimeError("evaluate_aurora_gan needs the build's CLIP image tower: call load_clip_weights(path) "
                           "first (a foreign model registered through set_clip_model has no encode_generated)")
    return evaluate_generator(generator, dataloader, tower, **kw)


def sample_aurora_gan(generator, text_prompt, num_samples=1, truncation_psi=0.7, device=DEVICE, text_tokens=None,
                      text_len=None, prompt_tokens=False, use_ema=False):
    """Reference :1672-1709: eval mode (hard top-1 routing), clamp to [-1, 1].  ``text_tokens`` [B or 1, Lk, 512] /
    ``text_len``: per-token text features for the cross-attention (AuroraGenerator.forward).  ``prompt_tokens``
    with a string prompt: the prompt's own token features (encode_prompt) feed the cross-attention too.
    ``use_ema``: sample the generator's moving average (``generator.ema_generator()``) instead of its live weights;
    the live generator then keeps its mode."""
    if use_ema:
        generator = generator.ema_generator()
    generator.eval()
    z = torch.randn(num_samples, LATENT_DIM, device=device, dtype=torch.float32)
    if isinstance(text_prompt, str) or (isinstance(text_prompt, list) and isinstance(text_prompt[0], str)):
        if prompt_tokens and text_tokens is None:
            text_prompt, text_tokens, text_len = encode_prompt(text_prompt)
        else:
            text_prompt = encode_text_with_clip(text_prompt)
    text_prompt = text_prompt.float().to(device)
    if num_samples > 1 and text_prompt.size(0) == 1:
        text_prompt = text_prompt.repeat(num_samples, 1)
    if text_tokens is not None:
        text_tokens = text_tokens.float().to(device)
        if num_samples > 1 and text_tokens.size(0) == 1:
            text_tokens = text_tokens.repeat(num_samples, 1, 1)
            if text_len is not None:
                text_len = torch.as_tensor(text_len).reshape(-1).repeat(num_samples)
    with torch.no_grad():
        fake, _ = generator(z, text_prompt, truncation_psi=truncation_psi, text_tokens=text_tokens,
                            text_len=text_len)
        return torch.clamp(fake, -1, 1)
