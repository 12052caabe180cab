"""One G+D training step of train_aurora_gan (t2i_moe_gan.py:1262-1421) on the HIP engines.

The step keeps the reference's order and semantics:
  D phase: D(real) + R1, G forward under no_grad (fresh router noise), D(fake), D(real, text[perm]),
           D backward, clip_grad_norm_(D, 0.7), AdamW(D)
  G phase: G forward (fresh router noise), KL clamp at 50, D(fake) with the UPDATED D, G adversarial
           loss + CLIP terms (no gradient, :98-101) + balance loss (last layer) + annealed KL,
           G backward, clip_grad_norm_(G, 0.8), AdamW(G)
Parameters with no gradient in the reference (to_rgb_8: only feeds the gradient-free CLIP loss; with the
progressive extension every to_rgb but the final one)
sit in the store's frozen tail and are never updated -- exactly as torch's AdamW skips a
parameter whose .grad is None.

``StepConfig(clip_grad=True)`` (this build's extension, off by default): the two CLIP terms do carry their gradient.
The G phase then runs img16 and img8 through the build's image tower with the data-gradient context saved (one
pass per image, the batches of the gradient-free path, so the logged terms keep its values bit for bit: at a
small batch a 2B-row pass takes other split-K GEMM forms than a B-row one and rounds differently), forms each term
and its feature gradient in one launch (mg_cos_loss), and the tower's backward
(clip_vit.ClipImageEncoder.backward) adds clip_weight_16 * d L_clip / d img16 to the adversarial image gradient and
writes clip_weight_8 * d L_clip / d img8, which the generator backward takes as ``g_img8``: the half-resolution
to_rgb then trains, so the store keeps it inside the optimised range (layout.frozen_rgb_prefixes(clip_grad=True)).
``StepConfig(clip_grad=True, clip_loss="contrastive")`` swaps the term alone: a softmax over the global batch's
captions with the image's own caption as the positive (mg_clip_contrast; under data parallelism the captions are
gathered once per step, the features are not); the tower passes, the weights, the guard and the logged keys stay.

``StepConfig(clip_grad=True, vision_d=True)`` (this build's extension, off by default) adds a vision-aided
discriminator head (Kumari et al., "Ensembling off-the-shelf models for GAN training"; GigaGAN's L_vision; StyleGAN-T's
frozen-feature discriminator): a small conditional head (include/moegan_hip.h, ``mg_vhead_*``) that judges images in the
feature space of the frozen image tower.  It has its own parameter store ``TrainStep.vs`` (layout.vision_head_shapes)
and its own gated AdamW launch with ``lr_d`` / ``d_clip`` and its own step counter.  D phase: one forward-only tower
pass over the real batch and the D-phase fakes together, then ops.vhead_d (real / fake / mismatched-caption softplus
terms, the three of mg_d_loss) into ``vs.grad``; a non-finite head loss skips the batch like a non-finite d_loss.
G phase: ops.vhead_g on the tower features of img16 that the CLIP term already computed, with the head as this step's
D phase updated it; its feature gradient times ``vision_weight`` joins the CLIP term's before the one tower backward
that already runs (img8 gets no vision term).  The head sees un-augmented images (DiffAugment in front of the tower
is out of scope), has no R1 (Kumari et al. use none), and the reference's accumulation "leak" of the G loss into D's
gradients is deliberately not reproduced for it: ``vs.grad`` only ever holds d L_d.

Loss guards (t2i_moe_gan.py:1315-1320, :1367-1376, :1396-1404) run on the device: a flag word per step
(``out["flags"]``) records a non-finite discriminator loss (the whole batch is skipped: no gradient is
kept, no optimizer steps, no step counters advance) or a non-finite generator loss (replaced by 0: only
the routers' KL term keeps a gradient).  A second word per accumulation window records which parameter
groups received a gradient, so the gated optimizer launches skip a group whose gradient the reference
would leave as None.  Everything stays one captured hipGraph; the host reads the flags at most once per
step.

Gradient accumulation (gradient_accumulation_steps > 1): each batch's gradients are formed in
``store.grad`` and added to the window accumulator ``store.acc`` only if the guards keep the batch.

Nothing here synchronises with the host: every loss value stays on the device until the caller reads it,
and all randomness is passed in.  Data parallelism (one process per GPU, RCCL) all-reduces the flat D and
G gradient buffers, the [E] expert-load vector and the guard word.
"""
import os

import torch
import torch.nn.functional as F

from . import graphs, ops
from .engine_d import DiscriminatorEngine
from .engine_g import GeneratorEngine
from .layout import discriminator_shapes, frozen_rgb_prefixes, generator_shapes, vision_head_shapes
from .params import ParamStore

FD, FG = ops.FLAG_D_BAD, ops.FLAG_G_BAD


class StepConfig:
    def __init__(self, E=4, topk=None, dtype="fp32", r1_gamma=10.0, clip_weight_16=0.1, clip_weight_8=0.05,
                 balance_weight=0.01, beta1=0.5, beta2=0.999, weight_decay=0.01, eps=1e-8, d_clip=0.7, g_clip=0.8,
                 psi=0.7, fp8=False, max_res=16, deterministic=None, clip_grad=False, ema_halflife=None,
                 ema_rampup=None, diffaug=None, clip_loss="cosine", clip_temperature=0.07, vision_d=False,
                 vision_weight=1.0, vision_hidden=256, attn_res=16):
        """``attn_res`` (16 or 32; 32 needs ``max_res`` >= 32): the finest block with an AttentionBlock
        (layout.gen_blocks); 16 is the reference's generator.

        ``vision_d`` (needs ``clip_grad=True``: the head's generator gradient goes through the build's own tower
        backward): the vision-aided discriminator head of the module docstring, hidden width ``vision_hidden`` (a
        multiple of 64 in [64, 512]; 256 is a choice); its generator-side loss enters with ``vision_weight`` (finite,
        >= 0).  The default 1.0 -- the adversarial term's own weight -- is a choice, not a measurement.

        ``clip_loss`` (with ``clip_grad=True``): "cosine" = the reference's 1 - mean cos(image, own caption);
        "contrastive" = a softmax over the (global) batch's captions with the image's own caption as the positive
        (ops.clip_contrast), at temperature ``clip_temperature``.  The default 0.07 is CLIP's initial temperature: a
        choice, not a measurement -- it is explicit because the weight loaders drop the checkpoint's logit_scale."""
        self.E, self.topk = E, topk
        # differentiable augmentation of the discriminator's inputs (this build's extension, moegan_mi/augment.py): a
        # policy string, any comma-separated subset of color,translation,cutout; None = off (the reference's step)
        from .augment import parse_policy
        self.diffaug = None if diffaug is None else str(diffaug)
        self.diffaug_mask = None if diffaug is None else parse_policy(diffaug)  # (ValueError for an unknown name)
        # generator output resolution: 16 = the reference; 32 / 64 / 128 = the progressive extension (layout.py)
        self.max_res = max_res
        from .layout import check_attn_res
        self.attn_res = check_attn_res(max_res, attn_res)
        self.dtype = dtype
        self.fp8 = fp8  # MX-fp8 3x3 modulated convs (BASELINE config C5), inside the bf16 mode
        self.r1_gamma = r1_gamma
        self.clip_weight_16, self.clip_weight_8 = clip_weight_16, clip_weight_8
        self.balance_weight = balance_weight
        self.beta1, self.beta2, self.weight_decay, self.eps = beta1, beta2, weight_decay, eps
        self.d_clip, self.g_clip = d_clip, g_clip
        self.psi = psi
        # the CLIP terms train the generator (needs the build's image tower as TrainStep's clip_encoder); False: the
        # reference's gradient-free terms
        self.clip_grad = bool(clip_grad)
        if clip_loss not in ("cosine", "contrastive"):
            raise ValueError(f"clip_loss must be 'cosine' or 'contrastive', got {clip_loss!r}")
        if clip_loss == "contrastive" and not self.clip_grad:
            raise ValueError("clip_loss='contrastive' needs clip_grad=True (the gradient-free terms stay the cosine)")
        if not float(clip_temperature) > 0 or float(clip_temperature) == float("inf"):
            raise ValueError(f"clip_temperature must be positive and finite, got {clip_temperature}")
        self.clip_loss, self.clip_temperature = clip_loss, float(clip_temperature)
        self.vision_d = bool(vision_d)
        if self.vision_d and not self.clip_grad:
            raise ValueError("vision_d=True needs clip_grad=True (the head's generator gradient goes through the "
                             "build's own image-tower backward)")
        vw = float(vision_weight)
        if not (vw >= 0.0 and vw != float("inf")):
            raise ValueError(f"vision_weight must be finite and >= 0, got {vision_weight}")
        if int(vision_hidden) != vision_hidden or int(vision_hidden) % 64 or not 64 <= int(vision_hidden) <= 512:
            raise ValueError(f"vision_hidden must be a multiple of 64 in [64, 512], got {vision_hidden}")
        self.vision_weight, self.vision_hidden = vw, int(vision_hidden)
        # exponential moving average of the generator (this build's extension): half-life in optimizer steps, None =
        # off (the reference's step); ema_rampup caps the half-life at ema_rampup * step early on (None / 0: constant)
        if ema_halflife is not None and not ema_halflife > 0:
            raise ValueError(f"ema_halflife must be positive (optimizer steps), got {ema_halflife}")
        self.ema_halflife = None if ema_halflife is None else float(ema_halflife)
        self.ema_rampup = float(ema_rampup) if ema_rampup else 0.0
        # deterministic mode (ops.set_deterministic): None = the MOEGAN_DETERMINISTIC environment switch
        self.deterministic = (os.environ.get("MOEGAN_DETERMINISTIC", "0") == "1") if deterministic is None \
            else bool(deterministic)


def clip_loss(images_nchw, text, encode_image, images_nhwc=None):
    """CLIPLoss.forward (t2i_moe_gan.py:75-119): 1 - mean cos(CLIP(image), text), forward only (no gradient,
    :98-101).  Logging / validation only; values are parity-unpinned (CLIP weights are not available here).
    With the build's image tower (``encode_image`` a bound ``ClipImageEncoder`` method) and the generator's NHWC
    image, clamp + resize + patchify run as one kernel (``encode_generated``); any other encoder gets the NCHW
    clamp / F.interpolate input of the reference."""
    with torch.no_grad():
        tower = getattr(encode_image, "__self__", None)
        if images_nhwc is not None and hasattr(tower, "encode_generated"):
            f = tower.encode_generated(images_nhwc).float()
        else:
            im = torch.clamp(images_nchw.float(), -1, 1)
            if im.shape[-1] != 224 or im.shape[-2] != 224:
                im = F.interpolate(im, size=(224, 224), mode="bilinear", align_corners=False)
            f = encode_image(im).float()
        f = f / f.norm(dim=-1, keepdim=True)
        t = text.float() / text.float().norm(dim=-1, keepdim=True)
        sim = torch.nan_to_num((f * t).sum(dim=1))
        return (1.0 - sim.mean()).reshape(1)


def clip_tower(encoder):
    """The differentiable image tower behind ``encoder`` (the tower itself or one of its bound methods), or None for
    a foreign encoder (anything without ``encode_generated`` / ``backward``)."""
    for obj in (encoder, getattr(encoder, "__self__", None), getattr(encoder, "image", None)):
        if obj is not None and hasattr(obj, "encode_generated") and hasattr(obj, "backward"):
            return obj
    return None


class TrainStep:
    def __init__(self, cfg, device="cuda", process_group=None, gstore=None, dstore=None, clip_encoder=None,
                 vstore=None):
        self.cfg = cfg
        self.dev = torch.device(device)
        if getattr(cfg, "deterministic", False):
            ops.set_deterministic(True)
        self.cdt = torch.bfloat16 if cfg.dtype == "bf16" else torch.float32
        self.gs = gstore if gstore is not None else ParamStore(
            generator_shapes(cfg.E, getattr(cfg, "max_res", 16), getattr(cfg, "attn_res", 16)), self.dev,
            frozen_prefixes=frozen_rgb_prefixes(getattr(cfg, "max_res", 16), getattr(cfg, "clip_grad", False)),
            shadow_dtype=self.cdt)
        self.ds = dstore if dstore is not None else ParamStore(discriminator_shapes(), self.dev)
        if getattr(cfg, "ema_halflife", None) is not None:
            self.gs.enable_ema()
        self.ge = GeneratorEngine(self.gs, cfg.E, cfg.topk, self.cdt, fp8=getattr(cfg, "fp8", False))
        self.de = DiscriminatorEngine(self.ds, self.cdt)
        self.pg = process_group
        self.world = 1
        if process_group is not None:
            import torch.distributed as dist
            self.world = dist.get_world_size(process_group)
        self.clip_grad = bool(getattr(cfg, "clip_grad", False))
        if self.clip_grad:
            half = self.ge.rgb_half + "weight"
            if self.gs.offsets[half][0] >= self.gs.n_opt:
                raise ValueError(f"clip_grad=True trains {self.ge.rgb_half[:-1]}, which this parameter store keeps "
                                 "frozen: build it with layout.frozen_rgb_prefixes(max_res, clip_grad=True)")
            self._clip_scale = torch.ones(1, device=self.dev)  # device scalar of mg_cos_loss (the weights ride alpha)
        # the vision-aided head (cfg.vision_d): a plain store -- no frozen tail, no shadow, no moving average -- sized
        # by the tower's feature width once one is attached (a given ``vstore`` fixes it)
        self.vision_d = bool(getattr(cfg, "vision_d", False))
        self.vs = vstore
        if self.vision_d:
            self._vis_scale = torch.full((1,), float(cfg.vision_weight), device=self.dev)
        # optional image encoder for the CLIP loss terms (gradient-free unless cfg.clip_grad); images are
        # [B,3,H,W] in [-1, 1]
        self.clip_encoder = clip_encoder
        self.win = torch.zeros(1, device=self.dev, dtype=torch.int32)  # accumulation-window word (mg_flag_window)

    @property
    def clip_encoder(self):
        return self._clip_encoder

    @clip_encoder.setter
    def clip_encoder(self, enc):
        """With cfg.clip_grad only the build's own tower will do: a foreign encoder is refused here, not mid-step."""
        self._clip_tower = clip_tower(enc) if enc is not None else None
        if self.clip_grad and enc is not None and self._clip_tower is None:
            raise ValueError("clip_grad=True needs the build's image tower (moegan_mi.clip_vit.ClipImageEncoder or "
                             f"its encode_image) as clip_encoder; {type(enc).__name__} has no backward")
        self._clip_encoder = enc
        if self.vision_d and self._clip_tower is not None:
            C = int(self._clip_tower.output_dim)
            if self.vs is None:
                from .init import init_vision_head
                self.vs = ParamStore(vision_head_shapes(C, self.cfg.vision_hidden), self.dev)
                init_vision_head(self.vs)
            elif self.vs.shapes["fc.weight"][1] != C:
                raise ValueError(f"the vision head reads {self.vs.shapes['fc.weight'][1]}-wide features, the tower "
                                 f"gives {C}")

    def _vhead(self, buf):
        """The head's six tensors (ops.VHEAD_KEYS) as views into one of ``vs``'s flat buffers."""
        return {k: self.vs._v(buf, k) for k in ops.VHEAD_KEYS}

    # ---- data-parallel reductions ----
    # (collectives stay eager segments when the step is replayed as hipGraphs, graphs.py)
    def _allreduce_mean(self, t):
        if self.pg is None:
            return
        import torch.distributed as dist

        def run():
            dist.all_reduce(t, op=dist.ReduceOp.SUM, group=self.pg)
            t.mul_(1.0 / self.world)
        graphs.eager(run)

    def _allreduce_sum(self, t):
        if self.pg is None:
            return
        import torch.distributed as dist
        graphs.eager(lambda: dist.all_reduce(t, op=dist.ReduceOp.SUM, group=self.pg))

    def _gather_captions(self, t32):
        """(captions of the global batch [world * B, C], this rank's first row): the contrastive CLIP loss's
        negatives.  Each rank writes its rows into a zero buffer and the buffers are summed -- x + 0 is exact, and
        the sum all-reduce is the one collective every backend in use here runs on device tensors.  Captions carry
        no gradient, so nothing comes back.  Once per step; an eager segment of a captured step."""
        if self.pg is None:
            return t32, 0
        import torch.distributed as dist
        B = t32.shape[0]
        pos_off = dist.get_rank(self.pg) * B
        t_all = torch.zeros(self.world * B, t32.shape[1], device=t32.device)
        t_all[pos_off:pos_off + B].copy_(t32)
        self._allreduce_sum(t_all)
        return t_all, pos_off

    def _bucketed_grad_allreduce(self, store, begin):
        """Overlapped data-parallel mean of a flat gradient: ``begin()`` arms the engine so
        every range it reports final during the backward (a block's expert parameters, ~56 % of the generator
        at E=8) starts an asynchronous RCCL all-reduce at once, overlapping the rest of the backward; the
        returned ``finish()`` all-reduces the complement of those ranges in [0, n_opt), waits for every
        bucket and scales by 1 / world.  The reductions are sums of the same per-rank gradients as the single
        collective, just split into disjoint ranges."""
        import torch.distributed as dist
        pending, done = [], []

        def on_final(lo, hi):
            t = store.grad[lo:hi]
            done.append((lo, hi))
            graphs.eager(lambda: pending.append(dist.all_reduce(t, op=dist.ReduceOp.SUM, group=self.pg,
                                                                async_op=True)))
        begin(on_final)

        def finish():
            n = store.n_opt
            rest, cur = [], 0
            for lo, hi in sorted(done):
                if lo > cur:
                    rest.append((cur, lo))
                cur = max(cur, hi)
            if cur < n:
                rest.append((cur, n))
            views = [store.grad[lo:hi] for lo, hi in rest]

            def run():
                for t in views:
                    pending.append(dist.all_reduce(t, op=dist.ReduceOp.SUM, group=self.pg, async_op=True))
                for w in pending:
                    w.wait()
                pending.clear()
                store.grad[:n].mul_(1.0 / self.world)
            graphs.eager(run)
        return finish

    def _allreduce_flags(self, flags):
        """Every rank takes the same guard decision: a bit set on any rank is set on all (MAX per bit)."""
        if self.pg is None:
            return
        import torch.distributed as dist

        def run():
            bits = torch.stack([(flags & FD), (flags & FG)]).view(-1)
            dist.all_reduce(bits, op=dist.ReduceOp.MAX, group=self.pg)
            flags.copy_(bits[0:1] | bits[1:2])
        graphs.eager(run)

    def _guard(self, flags, checks, windows):
        """A phase's loss guards: the finite checks, the data-parallel agreement on the flag word, the window
        updates -- one launch (ops.guard_update) without a process group, check / all-reduce / windows with one."""
        if self.pg is None:
            ops.guard_update(flags, self.win, checks, windows)
            return
        ops.guard_update(flags, None, checks, ())
        self._allreduce_flags(flags)
        ops.guard_update(flags, self.win, (), windows)

    # ---- optimizer ----
    def _adamw(self, store, grad, lr, max_norm, flags, ranges, grad_scale=1.0):
        """clip_grad_norm_ + AdamW over ``grad[:n_opt]`` (torch semantics, :1333-1337 / :1417-1421).  ``ranges``:
        [(lo, hi, step counter, window bit)] -- each range is one gated launch with its own step counter.

        With ``cfg.ema_halflife`` the generator's launches (the store that has ``ema``) also advance its moving
        average, each range with its own counter and gate (ops.adamw_dev(ema=)): no further launch, host read or
        collective.  Under data parallelism every rank holds identical parameters after the all-reduced step and so
        computes identical averages."""
        n = store.n_opt
        if grad_scale != 1.0:  # (loss / accumulation_steps) of the reference == scaling the summed gradient
            grad[:n].mul_(grad_scale)
        ss = torch.empty(1, device=self.dev)
        live = [(lo, hi, step_dev, wbit) for lo, hi, step_dev, wbit in ranges if hi > lo]
        # the norm and every range's device step counter (+1, graph-replayable, gated) in two launches
        ops.grad_norm_steps(grad[:n], ss, [(step_dev, wbit) for _, _, step_dev, wbit in live], flags=flags,
                            skip_mask=FD, win=self.win)
        c = self.cfg
        bf16_shadow = store.shadow is not None and store.shadow.dtype == torch.bfloat16
        halflife = getattr(c, "ema_halflife", None)
        ema = store.ema if halflife is not None and store is self.gs else None
        for lo, hi, step_dev, wbit in live:
            gate = (flags, FD, self.win, wbit)
            if ema is not None:
                ops.adamw_dev(store.data[lo:hi], grad[lo:hi], store.m[lo:hi], store.v[lo:hi], lr, c.beta1, c.beta2,
                              c.eps, c.weight_decay, step_dev, ss, max_norm,
                              shadow=store.shadow[lo:hi] if bf16_shadow else None, gate=gate, ema=ema[lo:hi],
                              ema_halflife=halflife, ema_rampup=c.ema_rampup)
                continue
            ops.adamw_dev(store.data[lo:hi], grad[lo:hi], store.m[lo:hi], store.v[lo:hi], lr, c.beta1, c.beta2,
                          c.eps, c.weight_decay, step_dev, ss, max_norm,
                          shadow=store.shadow[lo:hi] if bf16_shadow else None, gate=gate)
        if bf16_shadow:
            store.mark_shadow_written()
        return ss

    def _check_aug(self, aug, B):
        """``aug`` is given exactly when the configuration names a policy, as fp32 [3, B, 8] on the step's device."""
        policy = getattr(self.cfg, "diffaug", None)
        if policy is None:
            if aug is not None:
                raise ValueError("aug was given but StepConfig(diffaug=None): name a policy to augment")
            return
        if aug is None:
            raise ValueError(f"StepConfig(diffaug={policy!r}) needs the step's aug [3, {B}, 8] "
                             "(moegan_mi.augment.draw)")
        if not torch.is_tensor(aug) or aug.dtype != torch.float32 or tuple(aug.shape) != (3, B, 8):
            got = (tuple(aug.shape), aug.dtype) if torch.is_tensor(aug) else type(aug).__name__
            raise ValueError(f"aug must be a float32 [3, {B}, 8] tensor, got {got}")
        if aug.device.type != self.dev.type or not aug.is_contiguous():
            raise ValueError(f"aug must be contiguous on {self.dev}, got {aug.device}")

    # ---- the step ----
    def step(self, real, text, z, eps_d, eps_g, perm, *, anneal=3.0, lr_g=2e-4, lr_d=2e-4, eff_kl_weight=1e-8,
             prep=True, acc=1, zero_grads=True, step_optim=True, text_rows=None, row_off=None, lk_max=None,
             aug=None):
        """real [B,3,64,64] fp32 NCHW, text [B,512], z [B,512] fp32 (device); eps_d / eps_g: one triple of
        router epsilon tensors per attention block (three; four with attn_res = 32); perm [B] int32.  Returns a dict of device tensors.

        ``text_rows`` [rows, 512] (pad rows zero) / ``row_off`` device int32 [B+1] / ``lk_max``: per-token text
        features in packed form (tokens.pack_tokens).  The generator's attention blocks then attend over each
        image's token rows (the D-phase forward computes the text side with the prefix, the G-phase forward reuses
        it) and norm2.* and the q / k rows of cross_attn.in_proj_* receive gradients; the pooled ``text`` still
        feeds the mapping network and the discriminator, whose phases (and ``perm``) are unchanged.

        Gradient accumulation (t2i_moe_gan.py:1272, :1329, :1353, :1413): ``zero_grads`` at the first batch of
        a window, ``step_optim`` at its last; gradients are summed and scaled by 1/acc before clipping.  As in
        the reference, the generator step's loss also accumulates into the discriminator's gradients, which
        matters only when the D optimizer has not stepped yet in the window (acc > 1).

        ``aug`` fp32 [3,B,8] (device; moegan_mi.augment.draw), required exactly when ``cfg.diffaug`` names a policy:
        the discriminator sees T(image) wherever it sees an image -- row 0 transforms the real batch of the D phase
        (the mismatched-caption branch shares those features), row 1 the fakes of the D phase, row 2 the fakes of the
        G phase, whose image gradient comes back through T^T.  R1 is taken at the discriminator's input (the
        augmented real); the CLIP terms and the returned images stay un-augmented."""
        self._check_aug(aug, real.shape[0])
        if self.clip_grad and self._clip_tower is None:
            raise ValueError("clip_grad=True: attach the image tower first (TrainStep(..., clip_encoder=tower))")
        ops.ARENA.begin(self.dev)
        ops.COLSUMS.active = True  # bias-gradient column sums batched per backward (flushed below)
        # the library's gradient folds too: one batched launch per backward (ops.fold_flush); MOEGAN_FOLD_DEFER=0
        # folds each at its producer (same kernels, bit-identical gradients)
        ops.fold_defer(os.environ.get("MOEGAN_FOLD_DEFER", "1") == "1")
        # bf16 mode: the fp32-operand GEMMs (prefix, demodulation, router / cross-attention vectors) as split-bf16
        # products (ops.set_f32x3); the fp32 parity mode keeps exact-fp32 MFMA
        x3_prev = ops.set_f32x3(self.cdt == torch.bfloat16 and os.environ.get("MOEGAN_F32X3", "1") == "1")
        try:
            return self._step(real, text, z, eps_d, eps_g, perm, anneal, lr_g, lr_d, eff_kl_weight, prep, acc,
                              zero_grads, step_optim, text_rows, row_off, lk_max, aug)
        finally:
            ops.fold_defer(False)
            ops.set_f32x3(x3_prev)
            ops.ARENA.end()
            ops.COLSUMS.active = False
            ops.COLSUMS.items = []
            self.ge.guard_flags = None

    def _step(self, real, text, z, eps_d, eps_g, perm, anneal, lr_g, lr_d, eff_kl_weight, prep, acc, zero_grads,
              step_optim, text_rows=None, row_off=None, lk_max=None, aug=None):
        c = self.cfg
        aug_mask = getattr(c, "diffaug_mask", None) or 0
        aug_d = dict(aug_real=aug[0], aug_fake=aug[1], aug_mask=aug_mask) if aug is not None else {}
        aug_g = dict(aug_fake=aug[2], aug_mask=aug_mask) if aug is not None else {}
        accum = acc > 1
        gs, ds = self.gs, self.ds
        vs = self.vs if self.vision_d else None
        flags = ops.zeros(1, device=self.dev, dtype=torch.int32)  # the step's guard word (zero arena)
        self.ge.guard_flags = flags
        if prep:
            self.ge.prep()
            self.de.prep()
        if accum:
            gs.ensure_acc()
            ds.ensure_acc()
            if zero_grads:
                ds.acc.zero_()
            if vs is not None:
                vs.ensure_acc()
                if zero_grads:
                    vs.acc.zero_()
        # ------------------------- D phase -------------------------
        if zero_grads or accum:
            ds.zero_grad()
            if vs is not None:
                vs.zero_grad()
        # the router-independent prefix of this forward (mapping, styles, gen_block_4's convolution block) is
        # kept with its saved activations and reused by the G-phase forward: same z / text, G not yet updated
        f16, _, _, probs_d, topi_d, _ = self.ge.forward(z, text, eps_d, anneal, c.psi, train=True, save=False,
                                                        want_kl=False, keep_prefix=True, text_rows=text_rows,
                                                        row_off=row_off, lk_max=lk_max)
        prefix, self.ge.last_prefix = self.ge.last_prefix, None
        dres = self.de.d_phase(real, text, f16, ("nhwc", 8), perm, c.r1_gamma, **aug_d)
        ops.fold_flush()
        ops.COLSUMS.flush()
        vis = None
        if vs is not None:
            # the vision-aided head: real batch and D-phase fakes through the frozen tower in one forward-only pass
            # (un-augmented), then the head's three terms and its parameter gradients
            B = real.shape[0]
            real_nhwc = torch.zeros(B, real.shape[2], real.shape[3], 8, device=self.dev, dtype=torch.float32)
            real_nhwc[..., :3] = real.float().permute(0, 2, 3, 1)
            vfeats = self._clip_tower.encode_generated([real_nhwc, f16]).float()
            vis = ops.vhead_d(vfeats[:B], vfeats[B:], text.float().contiguous(), perm, self._vhead(vs.data),
                              self._vhead(vs.grad))
        # guard: NaN / Inf d_loss skips the whole batch (t2i_moe_gan.py:1315-1320)
        self._guard(flags, [(dres["losses"][:1], FD), (dres["r1"], FD)] + ([(vis[0][:1], FD)] if vis else []),
                    [dict(reset_bits=ops.WIN_D if zero_grads else 0, bad_mask=FD, set_bits=ops.WIN_D)])
        if accum:
            ops.gated_axpy(ds.acc, ds.grad, flags, FD)
            if vs is not None:
                ops.gated_axpy(vs.acc, vs.grad, flags, FD)
        dgrad = ds.acc if accum else ds.grad
        d_sumsq = None
        if step_optim:
            self._allreduce_mean(dgrad)
            d_sumsq = self._adamw(ds, dgrad, lr_d, c.d_clip, flags, [(0, ds.n_opt, ds.step_dev, ops.WIN_D)],
                                  grad_scale=1.0 / acc)
            self.de.prep()
            if vs is not None:
                vgrad = vs.acc if accum else vs.grad
                self._allreduce_mean(vgrad)
                self._adamw(vs, vgrad, lr_d, c.d_clip, flags, [(0, vs.n_opt, vs.step_dev, ops.WIN_D)],
                            grad_scale=1.0 / acc)
        # ------------------------- G phase -------------------------
        if accum:
            gs.zero_grad()
            if zero_grads:  # optimizer_g.zero_grad() (:1353) is never reached by a skipped batch
                ops.zero_if(gs.acc, flags, FD, when_set=False)
        elif zero_grads:
            gs.zero_grad()
        want8 = self.clip_encoder is not None
        img16, img8, kl2s, probs, topi_g, ctx = self.ge.forward(z, text, eps_g, anneal, c.psi, train=True,
                                                                save=True, want_img8=want8, prefix=prefix)
        prefix = None
        leak = accum and not step_optim  # the G loss also reaches D's gradients while D has not stepped yet
        if leak:
            ds.zero_grad()
        g_gan, fake_pred, g_img = self.de.g_phase(img16, ("nhwc", 8), text, want_d_params=leak, **aug_g)
        ops.fold_flush()
        ops.COLSUMS.flush()
        # balance loss on the last MoE layer, over the GLOBAL batch (t2i_moe_gan.py:951-1000)
        last = probs[-1]
        load = ops.zeros(c.E, device=self.dev)
        ops.colsum(last, load)
        self._allreduce_sum(load)
        if vs is not None:  # the balance term and the head's L_g side by side: one finite check covers both
            bal_vis = torch.empty(2, device=self.dev)
            bal, vis_g = bal_vis[:1], bal_vis[1:]
        else:
            bal, vis_g = torch.empty(1, device=self.dev), None  # (mg_balance writes it)
        coef = torch.empty(c.E, device=self.dev)
        ops.balance(load, c.E, last.shape[0] * self.world, c.balance_weight, float(self.world), bal, coef)
        # CLIP terms (t2i_moe_gan.py:1385-1387).  Default (the reference): forward only, they enter g_loss's value
        # but no gradient.  cfg.clip_grad: their image gradients join the generator backward below.
        clip16 = clip8 = g_img8 = None
        if self.clip_grad:
            # each image through the tower with its context saved (the gradient-free path's batches: same logged
            # values), the term with its feature gradient, then the tower's backward: + clip_weight_16 * dL/d img16
            # onto the adversarial image gradient, clip_weight_8 * dL/d img8 into the new g_img8
            tower = self._clip_tower
            t32 = text.float().contiguous()
            contrastive = getattr(c, "clip_loss", "cosine") == "contrastive"
            if contrastive:  # the negatives are the global batch's captions; this rank's are rows pos_off ...
                t_all, pos_off = self._gather_captions(t32)
            g_img8 = torch.zeros_like(img8)  # (the pad channels stay 0)
            terms = []
            for img, g_out, w, acc_ in ((img16, g_img, c.clip_weight_16, 1), (img8, g_img8, c.clip_weight_8, 0)):
                feats, cctx = tower.encode_generated(img, save=True)
                if contrastive:
                    term, g_f = ops.clip_contrast(feats, t_all, c.clip_temperature, self._clip_scale, pos_off=pos_off)
                else:
                    term, g_f = ops.cos_loss(feats, t32, self._clip_scale)
                if vs is not None and img is img16:
                    # the head as this step's D phase left it; alpha scales the whole feature gradient and
                    # clip_weight_16 may be 0, so the two gradients are combined in fp32 first
                    _, _, g_vis = ops.vhead_g(feats, t32, self._vhead(vs.data), self._vis_scale, loss=vis_g)
                    g_f = torch.add(g_vis, g_f, alpha=float(w))
                    tower.backward(cctx, g_f, g_out, alpha=1.0, accumulate=acc_)
                else:
                    tower.backward(cctx, g_f, g_out, alpha=w, accumulate=acc_)
                terms.append(term)
                cctx = None
            clip16, clip8 = terms
        elif self.clip_encoder is not None:
            clip16 = clip_loss(img16[..., :3].permute(0, 3, 1, 2), text, self.clip_encoder, images_nhwc=img16)
            clip8 = clip_loss(img8[..., :3].permute(0, 3, 1, 2), text, self.clip_encoder, images_nhwc=img8)
        # KL (t2i_moe_gan.py:846, :1367-1376, :1402-1404)
        kb = self.ge.last_klbuf  # the forward's [blocks, 2] KL buffer, whose rows kl2s are
        kl2 = kb if kb is not None and kb.shape[0] == len(kl2s) else torch.stack(kl2s)
        kl_coef = torch.empty(len(kl2s), device=self.dev)
        kl_total = torch.empty(1, device=self.dev)
        ops.kl_coefs(kl2, len(kl2s), eff_kl_weight, kl_coef, kl_total)
        # guard: NaN / Inf (GAN + CLIP + balance) generator loss -> 0, the KL term stays (:1396-1404)
        self._guard(flags, [(t, FG) for t in (g_gan, bal if vs is None else bal_vis, clip16, clip8) if t is not None],
                    [dict(reset_bits=(ops.WIN_G_MAIN | ops.WIN_G_KL) if zero_grads else 0, keep_mask=FD, bad_mask=FD,
                          set_bits=ops.WIN_G_KL),
                     dict(bad_mask=FD | FG, set_bits=ops.WIN_G_MAIN)])
        # data parallel, one optimizer step per batch: the generator gradient is all-reduced in buckets that
        # start while the backward still runs (expert ranges first); otherwise one collective after it
        g_finish = None
        if self.pg is not None and step_optim and not accum:
            g_finish = self._bucketed_grad_allreduce(gs, lambda cb: setattr(self.ge, "on_grad_final", cb))
        try:
            self.ge.backward(ctx, g_img, coef=coef, kl_coef=kl_coef, g_img8=g_img8)
        finally:
            self.ge.on_grad_final = None
        ops.fold_flush()
        ops.COLSUMS.flush()
        if g_finish is not None:  # every bucket reduced and scaled before the guard below rewrites ranges
            g_finish()
        if accum:
            ops.gated_axpy(gs.acc[:gs.n_main], gs.grad[:gs.n_main], flags, FD | FG)
            ops.gated_axpy(gs.acc[gs.n_main:gs.n_opt], gs.grad[gs.n_main:gs.n_opt], flags, FD)
            if leak:
                ops.gated_axpy(ds.acc, ds.grad, flags, FD | FG)
        else:
            ops.zero_if(gs.grad[:gs.n_main], flags, FG)  # the router KL range kept only its KL term
        ggrad = gs.acc if accum else gs.grad
        g_sumsq = None
        if step_optim:
            if g_finish is None:
                self._allreduce_mean(ggrad)
            g_sumsq = self._adamw(gs, ggrad, lr_g, c.g_clip, flags,
                                  [(0, gs.n_main, gs.step_dev, ops.WIN_G_MAIN),
                                   (gs.n_main, gs.n_opt, gs.step_dev_kl, ops.WIN_G_KL)],
                                  grad_scale=1.0 / acc)
        out = dict(d_losses=dres["losses"], r1=dres["r1"], g_gan=g_gan, balance=bal, kl=kl_total, kl_raw=kl2,
                   d_grad_sumsq=d_sumsq, g_grad_sumsq=g_sumsq, real_pred=dres["real_pred"],
                   fake_pred=dres["fake_pred"], mism_pred=dres["mism_pred"], r1_grad=dres["r1_grad"],
                   img16=img16, img8=img8, probs=probs, topi=topi_g, probs_d=probs_d, topi_d=topi_d,
                   fake_img_d=f16, flags=flags, clip16=clip16, clip8=clip8, d_grad=dgrad, g_grad=ggrad)
        if vs is not None:
            out.update(vis_d=vis[0], vis_real_pred=vis[1], vis_mism_pred=vis[2], vis_fake_pred=vis[3], vis_g=vis_g,
                       fake_d=f16, v_grad=vs.acc if accum else vs.grad)
        return out
