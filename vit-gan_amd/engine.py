"""GanEngine: the alternating G/D step (src/v2/training.py:170-211) as a short list of C calls.

One step on each rank (one process per GPU):
  1. D.grad = 0 ; fake = G(z)                                   (gen forward, saved for step 4)
  2. D([real ; fake.detach()]) -> loss_real + loss_fake -> backward into D.grad
     (the reference runs the two halves as separate passes, training.py:182-194; both accumulate
      into the same .grad before ONE optimizer step and the ViT has no cross-sample op, so running
      them as one 2B batch is the same computation up to fp32 summation order)
  3. all-reduce(D.grad) over ranks ; fused AdamW on D            (training.py:197)
  4. G.grad = 0 ; D(fake) with the UPDATED D -> loss(label = real) -> backward for the input
     gradient only (D's weight gradients of this pass are discarded by the next zero_grad,
     training.py:177, so they are never computed) -> gen backward
  5. all-reduce(G.grad) ; fused AdamW on G                        (training.py:211)
Nothing synchronises with the host; with ``use_graph`` the whole step is replayed as one hipGraph.
"""
from __future__ import annotations

import ctypes as C
import time
import warnings
import weakref
from typing import Optional

import torch
import torch.distributed as dist

from . import _lib, flat, ops
from .dist import GradSync, backward_pieces, world_size
from .generator import SirenGenerator
from .modules import ViTDiscriminator, VisionTransformer
from .spectral import SpectralState, parse_spectral_set, vit_matrix_keys

LOSS_KINDS = {"ns": 0, "hinge": 1, "wasserstein": 2}  # "wasserstein": the critic losses of src/v2/training.py:72,97


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


class GanEngine:
    def __init__(self, discriminator, generator: SirenGenerator, batch: int, loss: str = "ns",
                 lr_d: float = 5e-4, lr_g: float = 5e-4, weight_decay: float = 1e-3, betas=(0.9, 0.999),
                 eps: float = 1e-8, fuse_real_fake: bool = True, use_graph: bool = False,
                 d_dropout: Optional[float] = None, g_dropout: Optional[float] = None, seed: int = 0,
                 concurrent_wgrad: bool = False, clip_d: Optional[float] = None, clip_g: Optional[float] = None,
                 diversity_weight: float = 0.0, instance_noise: float = 0.0,
                 process_group: Optional["dist.ProcessGroup"] = None, external_noise: bool = False,
                 two_stream: bool = False, compress_mapping_grad: bool = False, shard_mapping_update: bool = False, gp_weight: float = 0.0,
                 exchange_single_rank: bool = False, dense_top_block: bool = False, gp_autograd: bool = False, diffaug: str = "",
                 ema_decay: float = 0.0, ema_start: int = 0, spectral_norm: str = "", bcr=(0.0, 0.0), bcr_aug: str = "",
                 aug_p: Optional[float] = None, ada_target: float = 0.0, ada_interval: int = 4, ada_kimg: float = 500.0):
        """concurrent_wgrad: the discriminator's weight gradients on a side stream beside its input gradients.  Off by default
        since the persistent GEMMs (csrc/gemm_wr.hip, gemm_tn.hip: their workgroups hold the CUs for a whole launch) - the
        side stream measured 6.70 against 6.67 ms/step.
        clip_d / clip_g: max gradient norms of ``clip_grad_norm_`` before each optimizer step (the reference's
        Wasserstein step uses 5.0 / 0.5, src/v2/training.py:78,104); None = no clipping (its live loop).
        diversity_weight: weight of ``diversity_loss(fake)`` in the generator loss (0.1 there, training.py:73-74; computed
        over this rank's batch - under data parallelism it is NOT the global-batch quantity).
        instance_noise: sigma of the Gaussian noise added to the discriminator's real and fake inputs in its own step
        (0.1 there, training.py:83-90); the generator's pass through D sees the clean fake.
        two_stream: run the step as two concurrent chains on two HIP streams (single GPU only) - D(real) forward/backward
        beside [G forward, D(fake) forward/backward], which is also the reference's own pass structure (two separate D
        passes, training.py:182-194), then the generator's pass through D as two half-batches side by side.  Kernels of the
        two chains are in different phases (a GEMM main loop next to another GEMM's epilogue, a LayerNorm next to a
        GEMM), which the single-chain step cannot be: every launch of this model covers the chip about once.
        gp_weight: weight of the WGAN-GP gradient penalty in the discriminator loss (``c.lambda_gp`` of training.py:106; the
        field is missing from the reference's Config).  The penalty is ONE C call, ``vg_vit_penalty``: forward, input-gradient
        backward, its double backward and the second backward as kernel sequences with the engine's counter-based dropout masks
        (the discriminator is in train mode there, as in the reference; the input gradients + LayerNorm backwards are fused where
        the full-row kernels take the shape); ``gp_autograd=True`` takes the operator-set path below, the form the C call is
        tested against.  That path runs through torch autograd over the twice-
        differentiable operator set (penalty.py) on the discriminator's real / fake inputs of this step and accumulates
        into the same gradient buffer before the exchange and AdamW.  With ``use_graph`` the autograd passes are captured with
        the rest of the step (every operator is an enqueue-only kernel call; epsilon and the penalty pass's dropout masks come
        from torch's graph-safe generator), so a replay costs no Python dispatch; if the capture fails the step runs eager, loudly.
        compress_mapping_grad (data parallel only, default OFF): exchange the gradient of the generator's mapping Linear - 50 MB of
        the generator's 64 MB, final only when the step's last kernel has run - as bf16 (see GradSync.reduce_range).  The sum is
        then formed in bf16 inside the collective (8 mantissa bits, error growing with the world size), so the default step is
        the exact fp32 all-reduce and a caller that wants the halved link traffic opts in (bench.py does and says so in its line).
        shard_mapping_update (data parallel only, default OFF): the same layer's gradient is reduce-SCATTERED in fp32 (each rank receives
        the exact sum of one 1/world share), every rank runs AdamW on its share alone, the updated fp32 master shares are all-gathered
        (GradSync.reduce_scatter_range / all_gather_range) and every rank casts the layer's bf16 shadow from the gathered master: exact
        sums like the default, 1/world of AdamW's traffic on the layer, and on every rank the master equals the replicated update's and
        the shadow is its round-to-nearest-even - so a later ``refresh_shadow()`` (a module forward, ``sync_from_modules``, the
        load_state_dict hook) recasts current weights.  The links carry the reduce-scatter plus a 4 B/parameter gather: the bytes of
        the all-reduce, not fewer (the cost on more than one real GPU is unmeasured).  AdamW's moments of the shares a rank does not
        own stay unused on that rank.  Not with ``clip_g`` (the clipping norm is taken over the whole gradient) nor together with
        ``compress_mapping_grad``.
        exchange_single_rank: run the staged backward and its all-reduces on a one-rank group as well (tests: the RCCL
        collectives inside a captured step, on a box with one GPU).
        dense_top_block: compute EVERY row of the top encoder block like the reference's operator graph does.  Default off: behind
        its attention that block runs on the B CLS rows only - the classifier reads nothing else (modules.py:195) and the gradient of the
        other rows is exactly zero - with the same logits and gradients (tests/test_engine_gpu.py compares the two); the switch exists
        for A/B measurements (``bench.py --dense-top-block 1``).
        use_graph: replay the step as one hipGraph.  On more than one rank the capture includes the RCCL all-reduces (backend
        "nccl"); when the capture is not possible (gloo process group, a torch build that cannot capture the collective) the
        engine says so loudly (warning + ``graph_fallback_reason``) and runs eager - it never falls back silently.
        external_noise: the latent batch is supplied by the caller (``step(real, z)``) instead of being drawn on the
        device inside the step - what parity tests use to give their CPU checker and the engine the same noise, also under
        hipGraph replay.
        diffaug: differentiable augmentation of what the discriminator sees, a comma-separated subset of ``color,translation,cutout``
        ("" = none: the step is launch for launch the plain one).  In its own step D sees T_1([real ; fake]) - after the instance
        noise when both are on, real and fake rows drawing independently, the gradient penalty taken on the augmented pair; in the
        generator's pass D sees T_2(fake) and ``dfake = T_2^T(dL/d T_2(fake))`` (vg_diffaug_fwd / vg_diffaug_bwd: one launch per
        application, one for the adjoint).  The transforms are keyed on (seed, rank, site, device step counter), so data-parallel ranks
        and every replay of the captured step draw their own; ``aug_params`` holds the last step's parameters of both sites.  Not
        with ``two_stream``.
        ema_decay: decay d of an exponential moving average of the GENERATOR's fp32 master weights, kept in ``ema_g`` by the generator's
        optimizer kernel itself (vg_adamw_ema_step: one pass, 38 B per parameter against AdamW's 30; no extra launch, nothing a
        replayed graph could miss).  With t the device step counter and p_t the weights after step t:  e_t = p_t while
        t <= max(1, ema_start) (the average follows the weights through the warm-up), then e_t = e_{t-1} + (1 - d)(p_t - e_{t-1}).
        0.0 (default) = no average: no buffer, and the step is launch for launch the plain one.  The discriminator is not averaged.
        Under ``shard_mapping_update`` the mapping Linear's average is updated from the gathered master (vg_ema_update), so every
        rank holds the average of a replicated run, bit for bit.  ``sample(z)`` draws from the average, ``ema_state_dict()`` exports
        it under the generator's keys, ``state_dict()`` carries it across a restart.
        spectral_norm: spectral normalisation of the DISCRIMINATOR's weight matrices in ViTGAN's form, W_eff = sigma0 W / sigma with
        sigma0 = sigma_max(W) at construction (so the network is unchanged there) and sigma one power iteration per step behind
        sigma_max(W), as ``torch.nn.utils.spectral_norm`` runs in training.  "qkv": queries / keys / values of every block, each [E, E]
        on its own (the reference's v1 set); "all": also out_projection, fc1, fc2, classifier.fc1 and embedding.conv1 as [E, C P P]
        (not classifier.fc2, which the head kernels read from the fp32 master); "" (default): nothing - no buffer, and the step is
        launch for launch the plain one.  The kernels read only the bf16 shadow, so the normalised network is a scaled cast of the
        master (vg_spectral_update, right after D's AdamW: the generator's pass of the same step sees the new shadow) and the
        optimizer sees the raw-weight gradient after one rank-one correction of the exchanged gradient total (vg_spectral_project,
        before clipping); weight decay acts on the raw weights.  The state (u, v, sigma, sigma0 per matrix) is attached to the
        discriminator's FlatParams, so a module forward, ``sync_from_modules`` and the load_state_dict hook keep the normalised
        shadow; ``state_dict()`` carries it, ``effective_state_dict()`` exports the trained function for a plain ViTDiscriminator.
        ``close()`` detaches it.  Not with ``two_stream``.
        bcr: ``(lambda_real, lambda_fake)``, the weights of balanced consistency regularisation (Zhao et al. 2020; the reference has
        none): L_cr = lambda_real 1/B sum_real |D(x_n) - D(T(x_n))|^2 + lambda_fake 1/B sum_fake |D(x_n) - D(T(x_n))|^2 joins the
        discriminator's loss, both branches carrying gradient.  x is the pair D's own step is given ([real ; fake.detach()], after the
        instance noise).  With ``diffaug`` the partner is the step's own T_1(x) - the adversarial loss and the penalty stay on it, the
        clean x is the consistency partner, no augmentation launch more; without it the adversarial loss and the penalty stay on x
        and T(x) is one vg_diffaug_fwd with policy ``bcr_aug`` at site 2 (``aug_params["c"]``).  D runs ONCE on the 4B images
        [x ; T(x)] - one forward, one backward, one exchange; the dropout masks are those of a 4B pass - and vg_bcr_loss adds the
        consistency gradients to the adversarial rows' and writes the partner rows'.  ``bcr_losses`` holds the two unweighted means.
        (0, 0) (default): nothing - no buffer, and the step is launch for launch the plain one.  The generator's pass is untouched.
        Not with ``two_stream`` nor ``fuse_real_fake=False``.
        bcr_aug: the consistency transform when ``diffaug`` is off, a comma-separated subset of ``color,translation,cutout``.
        aug_p: the probability with which every member of ``diffaug`` is applied to an image (sites 0 and 1; vg_diffaug_p_fwd /
        vg_diffaug_p_bwd: a per-image, per-member gate from the same counter hash, so replays and ranks draw their own).  It lives
        on the device, in ``ada_state[0]``, and the kernels read it there.  None (default) = 1.0 without ADA - and then, with
        ``ada_target=0``, the engine calls the ungated kernels, allocates nothing and the step is launch for launch what it was - and
        0.0 with ADA, where it is the starting value.  ``aug_params[...][:, 7]`` holds every image's effective policy.  With ``bcr``
        the partner T_1(x) is the gated transform: an image whose gates are all off contributes a plain copy, no launch more.
        ada_target: > 0 switches adaptive discriminator augmentation on (Karras et al. 2020): one launch per step of one workgroup,
        vg_ada_update, right behind the discriminator's loss launch, accumulates sign(D(real)) of the adversarial logits' real rows
        and, on every step whose device counter divides by ``ada_interval``, moves p by (images since the last update) /
        (1000 ``ada_kimg``) towards r_t = E[sign(D(real))] = ``ada_target``, clamped to [0, 1].  All of it on the device: a replayed
        hipGraph sees a fresh p with no host round trip.  The generator's pass of a step in which the controller fires ALREADY SEES
        THE NEW p (it runs behind the update); D's own pass of that step saw the old one.  ``ada_p`` / ``ada_rt`` read the state
        (they synchronise: for logging).  ``state_dict()`` carries the state and the four options.  Not with ``loss="wasserstein"``
        (a critic's sign carries no overfitting signal) and not under data parallelism (the statistics are per process; a fixed
        ``aug_p`` is allowed there).
        ada_interval: steps between two updates of p.  ada_kimg: thousands of real images it takes p to go from 0 to 1."""
        self.aug = ops.parse_aug_policy(diffaug)  # ValueError names the three members; argument errors come before any device check
        self.spectral_norm = parse_spectral_set(spectral_norm)  # ValueError names the two sets
        self.bcr_w = ops.parse_bcr_weights(bcr)
        self.bcr_policy = ops.parse_aug_policy(bcr_aug)
        self.bcr = self.bcr_w != (0.0, 0.0)
        if self.bcr_policy and self.aug:
            raise ValueError("bcr_aug: with diffaug on, diffaug's own transform T_1 is the consistency partner; leave bcr_aug empty")
        if self.bcr_policy and not self.bcr:
            raise ValueError("bcr_aug: a consistency transform without consistency weights (bcr=(0, 0)) would do nothing; set bcr")
        if self.bcr and not (self.aug or self.bcr_policy):
            raise ValueError("bcr: the consistency loss needs a transform - switch diffaug on (its T_1 is the partner) or name one in bcr_aug")
        if self.bcr and two_stream:
            raise ValueError("bcr: the consistency step runs the discriminator once on 4B images, on the single-chain schedule; switch two_stream off")
        if self.bcr and not fuse_real_fake:
            raise ValueError("bcr: the consistency step runs the discriminator once on 4B images; it needs fuse_real_fake=True")
        p0, self.ada_target, self.ada_interval, self.ada_kimg = ops.parse_ada_options(aug_p, ada_target, ada_interval, ada_kimg, self.aug, loss)
        self.ada = self.ada_target > 0.0
        self.gated = p0 is not None  # the gated kernels and a device-resident probability
        self.aug_p0 = 1.0 if p0 is None else p0
        if self.ada and (world_size(process_group) > 1 or (exchange_single_rank and dist.is_available() and dist.is_initialized())):
            raise ValueError("ada_target: the controller's statistics are per process and are not exchanged; under data parallelism use a "
                             "fixed aug_p")
        self.ada_step_per_image = 1.0 / (1000.0 * self.ada_kimg)
        self.ema_decay, self.ema_start = float(ema_decay), int(ema_start)
        if not 0.0 <= self.ema_decay < 1.0:
            raise ValueError(f"ema_decay must be in [0, 1), got {ema_decay!r}")
        if self.ema_start < 0 or self.ema_start != ema_start:
            raise ValueError(f"ema_start must be a non-negative integer, got {ema_start!r}")
        if self.aug and two_stream:
            raise ValueError("diffaug: the augmented step is verified on the single-chain schedule only; switch two_stream off")
        if self.spectral_norm and two_stream:
            raise ValueError("spectral_norm: the normalised step is verified on the single-chain schedule only; switch two_stream off")
        vit = discriminator.vit if isinstance(discriminator, ViTDiscriminator) else discriminator
        if not isinstance(vit, VisionTransformer) or not isinstance(generator, SirenGenerator):
            raise TypeError("GanEngine needs a ViTDiscriminator/VisionTransformer and a SirenGenerator")
        if getattr(vit, "precision", "bf16") != "bf16":
            raise ValueError("GanEngine: the fused step is bf16; it does not take a discriminator in precision='fp32'")
        if float(gp_weight) != 0.0:
            vit.require_short_attention("gp_weight > 0 (the gradient penalty)")
        self.vit, self.gen, self._disc = vit, generator, discriminator
        self.dev = vit._flat.flat.device
        if self.dev.type != "cuda" or generator._flat.flat.device != self.dev:
            raise RuntimeError("GanEngine: both networks must be on the same cuda device (no CPU fallback)")
        if loss not in LOSS_KINDS:
            raise ValueError(f"loss must be one of {sorted(LOSS_KINDS)}")
        self.B, self.kind = int(batch), LOSS_KINDS[loss]
        # dropout probabilities: default = what the modules would apply in their current train/eval mode
        self.p_d = float(vit._dropout_p if vit.training else 0.0) if d_dropout is None else float(d_dropout)
        self.p_g = float(generator.dropout_p if generator.training else 0.0) if g_dropout is None else float(g_dropout)
        self.seed = int(seed)
        self.fuse = bool(fuse_real_fake)
        self.hyp = dict(lr_d=lr_d, lr_g=lr_g, wd=weight_decay, b1=betas[0], b2=betas[1], eps=eps)
        self.clip_d, self.clip_g = clip_d, clip_g
        self.dp_chunks = 3  # pieces of the D / G backward whose gradient exchange overlaps the remaining backward
        self.compress_map = bool(compress_mapping_grad)
        self._want_shard_map = bool(shard_mapping_update)
        if self._want_shard_map and (self.compress_map or clip_g is not None):
            raise ValueError("shard_mapping_update excludes compress_mapping_grad and clip_g")
        self.dense_top = int(bool(dense_top_block))
        self.gp_w = float(gp_weight)
        self.gp_loss = torch.zeros(1, dtype=torch.float32, device=self.dev)
        self.gp_epsilon: Optional[torch.Tensor] = None  # tests: a fixed epsilon [B,1,1,1] instead of torch.rand
        if self.gp_w != 0.0 and two_stream:
            raise ValueError("gp_weight: the gradient penalty runs through torch autograd on one stream and cannot be forked")
        if self.gp_w != 0.0 and bool(getattr(vit, "attention_fp8", False)):
            # the penalty path (ops2.py) differentiates the bf16 attention kernels: with fp8 operands in the trained network
            # it would penalise a slightly different function than the one being trained
            raise ValueError("gp_weight: the gradient penalty is built on the bf16 attention kernels; switch attention_fp8 off")
        self.gp_c_call = self.gp_w != 0.0 and not gp_autograd and not bool(getattr(vit, "attention_fp8", False))
        self.div_w = float(diversity_weight)
        self.inst_sigma = float(instance_noise)
        self.external_noise = bool(external_noise)
        self.two_stream = bool(two_stream)
        self.div_loss = torch.zeros(1, dtype=torch.float32, device=self.dev)
        self.clip_scratch = torch.zeros(2, 1 + 1024, dtype=torch.float32, device=self.dev)  # [net][norm, partials]
        self.pg = process_group
        self.sync = GradSync(process_group, self.dev, overlap=True, single_rank=exchange_single_rank)
        self.world = self.sync.world
        g_ = generator._dims
        # (a layer that does not divide over the ranks keeps the all-reduce; a one-rank group - `exchange_single_rank` - runs the same calls)
        self.shard_map = self._want_shard_map and self.sync.active and (g_.T * g_.E * g_.Z) % (4 * self.world) == 0
        # latent noise drawn on the device (vg_step_inputs): one stream per (seed, rank)
        self._noise_seed = (self.seed * 0x9E3779B97F4A7C15 + 0xD1B54A32D192ED03 * (self.sync.rank + 1)) & 0xFFFFFFFFFFFFFFFF
        # differentiable augmentation (vg_diffaug_fwd): its own stream per (seed, rank), apart from the latent noise's
        self._aug_seed = (self._noise_seed ^ 0xA0761D6478BD642F) & 0xFFFFFFFFFFFFFFFF
        d, g = vit._dims, generator._dims
        if g.T * g.CW != d.C * d.IH * d.IH:
            raise ValueError("generator output does not match the discriminator's image shape")
        L = _lib.lib()
        B, dev = self.B, self.dev
        if self.two_stream:
            if self.world > 1:
                raise ValueError("two_stream is a single-GPU schedule (the data-parallel path overlaps the exchange instead)")
            if B % 2:
                raise ValueError("two_stream needs an even batch")
            self.fuse = False
        nD = 4 * B if self.bcr else (2 * B if self.fuse else B)
        self.Kc = d.Kc
        self.ws_d = torch.empty(L.vg_vit_ws_bytes(C.byref(d), nD), dtype=torch.uint8, device=dev)
        if self.two_stream:  # second chain: its own workspace, gradient buffer and stream
            self.ws_d2 = torch.empty(L.vg_vit_ws_bytes(C.byref(d), B), dtype=torch.uint8, device=dev)
            self.grad2 = torch.zeros_like(vit._flat.grad)
            self.side = torch.cuda.Stream(device=dev)
        if self.gp_c_call:  # the penalty's own passes: its forward runs in ws_d (the step's passes come after it), the rest here
            self.ws_gp = torch.empty(L.vg_vit_penalty_ws_bytes(C.byref(d), B), dtype=torch.uint8, device=dev)
            self.gp_eps = torch.empty(B, dtype=torch.float32, device=dev)
        self.ws_g = torch.empty(L.vg_gen_ws_bytes(C.byref(g), B), dtype=torch.uint8, device=dev)
        nL = 4 * B if self.bcr else 2 * B  # logit rows of the discriminator's own pass
        if self.bcr:
            # the 4B images of D's pass, [x ; T(x)], in one buffer: x = the (noisy) pair, T(x) = imgs_aug (diffaug) or imgs_bcr - the
            # step's own buffers are views of it, so no copy launch forms the batch
            self.imgs4 = torch.empty(4 * B, d.C, d.IH, d.IH, dtype=torch.bfloat16, device=dev)
        noisy = self.inst_sigma > 0.0
        # [real ; fake]; the instance noise needs the clean fake behind it (the generator's pass), so then x is imgs_noisy
        self.imgs = self.imgs4[:2 * B] if self.bcr and not noisy else torch.empty(2 * B, d.C, d.IH, d.IH, dtype=torch.bfloat16, device=dev)
        self.dfake = torch.empty(B, d.C, d.IH, d.IH, dtype=torch.bfloat16, device=dev)
        if self.inst_sigma > 0.0:  # noisy copy of [real ; fake] for the D step, and the noise itself (kept for inspection / tests)
            self.inoise = torch.empty(2 * B, d.C, d.IH, d.IH, dtype=torch.float32, device=dev)
            self.imgs_noisy = self.imgs4[:2 * B] if self.bcr else torch.empty_like(self.imgs)
        if self.aug:
            # D step: imgs_aug = T_1(D's input pair).  Generator pass: imgs_aug[:B] = T_2(fake), imgs_aug[B:] = dL/d T_2(fake)
            self.imgs_aug = self.imgs4[2 * B:] if self.bcr else torch.empty_like(self.imgs)
            self.aug_params = {"d": torch.zeros(2 * B, 8, dtype=torch.float32, device=dev),  # (b, s, k, tx, ty, cx, cy, policy) per row
                               "g": torch.zeros(B, 8, dtype=torch.float32, device=dev)}
        if self.bcr_policy:  # T_c(x), site 2
            self.imgs_bcr = self.imgs4[2 * B:]
            self.aug_params = {"c": torch.zeros(2 * B, 8, dtype=torch.float32, device=dev)}
        if self.bcr:
            self.bcr_losses = torch.zeros(2, dtype=torch.float32, device=dev)  # the unweighted means: real, fake
        self.div_scratch = torch.zeros((d.C * d.IH * d.IH + 15) // 16, dtype=torch.float32, device=dev)
        self.logits = torch.empty(nL, d.Kc, dtype=torch.float32, device=dev)
        self.dlogits = torch.empty(nL, d.Kc, dtype=torch.float32, device=dev)
        # (p, acc_sign, acc_count, r_last) of include/vitgan_hip.h, vg_ada_update: element 0 is the gated kernels' prob_dev
        self.ada_state: Optional[torch.Tensor] = None
        if self.gated:
            self.ada_state = torch.tensor([self.aug_p0, 0.0, 0.0, 0.0], dtype=torch.float32, device=dev)
        if self.bcr or self.ada:  # the generator's pass gets rows of its own, so ``logits`` still holds D's whole pass after the step
            self.logits_g, self.dlogits_g = torch.empty(B, d.Kc, dtype=torch.float32, device=dev), torch.empty(B, d.Kc, dtype=torch.float32, device=dev)
        self.z = torch.empty(B, g.Z, dtype=torch.float32, device=dev)
        self.losses = torch.zeros(3, dtype=torch.float32, device=dev)  # d_real, d_fake, g
        self.step_t = torch.zeros(1, dtype=torch.int32, device=dev)
        fd, fg = vit._flat, generator._flat
        self.m_d, self.v_d = torch.zeros_like(fd.flat), torch.zeros_like(fd.flat)
        self.m_g, self.v_g = torch.zeros_like(fg.flat), torch.zeros_like(fg.flat)
        # the generator's averaged weights (a copy of the master until the first step, which copies again: see ema_decay)
        self.ema_g: Optional[torch.Tensor] = fg.flat.detach().clone() if self.ema_decay > 0.0 else None
        self._ema_from = self.ema_start  # the kernels' ema_start (a non-strict load_state_dict without an average moves it)
        self._ema_shadow: Optional[torch.Tensor] = None  # bf16 cast of ema_g for sample(): allocated on first use
        self._ema_cast_key = None                        # (steps, loads) the cast was made at
        self._ema_loads = 0
        self._sample_ws: Optional[torch.Tensor] = None
        self.spec: Optional[SpectralState] = None
        if self.spectral_norm:
            keys = vit_matrix_keys(d.L, self.spectral_norm)
            ent = [(fd.slots[k][0], fd.slots[k][1][0], flat.numel(fd.slots[k][1][1:])) for k in keys]
            self.spec = SpectralState(ent, fd.total, dev, names=keys)
            self.spec.measure(fd.flat)
            fd.spectral = self.spec  # from here on every refresh_shadow() of the discriminator writes the normalised cast
        fd.refresh_shadow()
        fg.refresh_shadow()
        self.ctx = _lib.context() if concurrent_wgrad else None
        # a load_state_dict into either network (directly or through a container such as ViTGAN) copies into the flat
        # master buffers in place: refresh the bf16 shadows the GEMMs read, or the next step runs on stale weights
        # (the hook holds the engine weakly: a strong reference from the module would keep every engine ever built on it -
        # workspaces, optimizer moments - alive, and re-run the refresh of stale engines on every later load_state_dict)
        me = weakref.ref(self)

        def _hook(_mod, _keys):
            eng = me()
            if eng is not None:
                eng.sync_from_modules()
        self._hooks = [m.register_load_state_dict_post_hook(_hook) for m in (vit, generator)]
        self.steps = 0
        self._graph = None
        self._use_graph = bool(use_graph)
        self.graph_fallback_reason: Optional[str] = None
        if self._use_graph and self.sync.active:
            backend = dist.get_backend(process_group)
            if backend != "nccl":
                self._graph_fallback(f"process-group backend '{backend}' cannot be captured in a hipGraph (only nccl = RCCL can)")

    def _graph_fallback(self, reason: str) -> None:
        self._use_graph = False
        self._graph = None
        self.graph_fallback_reason = reason
        warnings.warn(f"GanEngine: hipGraph replay was requested but the step runs EAGER: {reason}", RuntimeWarning, stacklevel=3)

    @property
    def graph_active(self) -> bool:
        """True when step() replays a captured hipGraph (after the first call), False in eager mode."""
        return self._use_graph

    def close(self) -> None:
        """Detach from the modules (load_state_dict hooks) and drop the captured graph and workspaces."""
        for h in self._hooks:
            h.remove()
        self._hooks = []
        self._graph = None
        fd = self.vit._flat
        if getattr(self, "spec", None) is not None and fd.spectral is self.spec:
            fd.spectral = None  # the modules hold the raw weights again: export effective_state_dict() first

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ------------------------------------------------------------------------------------------
    def _nets(self):
        fd, fg = self.vit._flat, self.gen._flat
        # masks: host seed (fixed per pass) mixed on the device with the step counter, so a replayed hipGraph
        # still draws fresh masks; pass A = [real;fake] (or real), B = fake, C = generator pass through D
        step_ptr = self.step_t.data_ptr()
        mk = lambda i, g=None, ctx=True: _lib.VgVitNet(self.vit._dims, fd.flat.data_ptr(), fd.shadow.data_ptr(),  # noqa: E731
                                                       (fd.grad if g is None else g).data_ptr(), self.p_d, self.seed * 8 + i, step_ptr,
                                                       self.ctx if ctx else None, int(self.vit.attention_fp8), self.dense_top)
        if self.two_stream:  # chains run side by side: no third stream inside a pass; the fake chain accumulates into grad2
            return (mk(0, ctx=False), mk(1, self.grad2, ctx=False), mk(2, ctx=False), mk(3, ctx=False)), self._gen_net(step_ptr)
        return (mk(0), mk(1), mk(2)), self._gen_net(step_ptr)

    def _gen_net(self, step_ptr):
        fg, tab = self.gen._flat, self.gen.fourier_table
        return _lib.VgGenNet(self.gen._dims, fg.flat.data_ptr(), fg.shadow.data_ptr(), fg.grad.data_ptr(), self.p_g, self.seed * 8 + 7, step_ptr,
                             None if tab is None else tab.data_ptr())

    def _d_backward(self, nd, n_img: int, dl, want_w: int, dimg, st) -> None:
        """D backward; under data parallelism in ``dp_chunks`` pieces (head + upper blocks first) so that the all-reduce
        of each finished piece - a contiguous tail of the flat gradient buffer - overlaps the backward of the blocks
        below it; only the last piece's exchange is exposed."""
        L = _lib.lib()
        nL = self.vit._dims.L
        if not self.sync.active or not want_w:
            _lib.check(L.vg_vit_backward(C.byref(nd), n_img, _p(self.ws_d), dl, dimg, want_w, st), "vg_vit_backward")
            return
        fd = self.vit._flat
        lay = flat.vit_layout(self.vit._dims)
        for s0, s1, lo, hi in backward_pieces(nL, self.dp_chunks, lay.layer0, lay.layer_stride, fd.total):
            _lib.check(L.vg_vit_backward_stages(C.byref(nd), n_img, _p(self.ws_d), dl, dimg, want_w, s0, s1, st), "vg_vit_backward_stages")
            self.sync.reduce_range(fd.grad, lo, hi)

    def _g_backward(self, ng, st) -> None:
        """G backward; under data parallelism in ``dp_chunks`` pieces like D's: SIREN head + upper blocks first, their
        gradients (a contiguous tail of the flat buffer) are exchanged while the lower blocks still run.  What is left
        exposed is the front of the buffer - learned embedding, mapping Linear, lowest blocks - which only completes
        with the last kernel; its 50 MB mapping-weight part goes over the links as bf16."""
        L = _lib.lib()
        fg = self.gen._flat
        if not self.sync.active:
            _lib.check(L.vg_gen_backward(C.byref(ng), self.B, _p(self.ws_g), _p(self.dfake), st), "vg_gen_backward")
            return
        lay = flat.gen_layout(self.gen._dims)
        d = self.gen._dims
        for s0, s1, lo, hi in backward_pieces(d.L, self.dp_chunks, lay.layer0, lay.layer_stride, fg.total):
            _lib.check(L.vg_gen_backward_stages(C.byref(ng), self.B, _p(self.ws_g), _p(self.dfake), s0, s1, st), "vg_gen_backward_stages")
            if lo == 0 and (self.compress_map or self.shard_map):  # [embedding | mapping weight | mapping bias, lowest blocks]
                w0, w1 = lay.map_w, lay.map_w + d.T * d.E * d.Z
                self.sync.reduce_range(fg.grad, 0, w0)
                if self.shard_map:
                    self.sync.reduce_scatter_range(fg.grad, w0, w1)   # this rank keeps the sum of its share only
                else:
                    self.sync.reduce_range(fg.grad, w0, w1, compress=True)
                self.sync.reduce_range(fg.grad, w1, hi)
            else:
                self.sync.reduce_range(fg.grad, lo, hi)

    def _map_range(self):
        lay, d = flat.gen_layout(self.gen._dims), self.gen._dims
        return lay.map_w, lay.map_w + d.T * d.E * d.Z

    def _adamw_g_sharded(self, st) -> None:
        """The generator's AdamW with the mapping Linear sharded: the whole buffer but that layer as usual, of the layer this rank's
        share only; then the updated fp32 master shares to every rank and the layer's bf16 shadow cast from them there (the GEMMs of
        every rank read the whole shadow; gathering the master, not the shadow, keeps every rank's master current)."""
        fg, h, L = self.gen._flat, self.hyp, _lib.lib()
        w0, w1 = self._map_range()
        a, b = self.sync.share(w0, w1)

        def upd(lo, hi, ema=None):
            if hi <= lo:
                return
            off = lambda t, es: C.c_void_p(t.data_ptr() + es * lo)  # noqa: E731
            if ema is None:
                _lib.check(L.vg_adamw_step(off(fg.flat, 4), off(fg.grad, 4), off(self.m_g, 4), off(self.v_g, 4), off(fg.shadow, 2), hi - lo,
                                           self.hyp["lr_g"], h["b1"], h["b2"], h["eps"], h["wd"], 0, _p(self.step_t), 1.0 / self.world, st), "vg_adamw_step")
            else:
                _lib.check(L.vg_adamw_ema_step(off(fg.flat, 4), off(fg.grad, 4), off(self.m_g, 4), off(self.v_g, 4), off(fg.shadow, 2), off(ema, 4),
                                               hi - lo, self.hyp["lr_g"], h["b1"], h["b2"], h["eps"], h["wd"], 0, _p(self.step_t), 1.0 / self.world,
                                               self.ema_decay, self._ema_from, st), "vg_adamw_ema_step")
        upd(0, w0, self.ema_g)
        upd(a, b)
        upd(w1, fg.total, self.ema_g)
        self.sync.all_gather_range(fg.flat, w0, w1)
        self.sync.wait()
        _lib.check(L.vg_cast_f32_bf16(C.c_void_p(fg.flat.data_ptr() + 4 * w0), C.c_void_p(fg.shadow.data_ptr() + 2 * w0), w1 - w0, st),
                   "vg_cast_f32_bf16")
        if self.ema_g is not None:  # the layer's average from the gathered master: what the fused kernel of a replicated run writes
            _lib.check(L.vg_ema_update(C.c_void_p(self.ema_g.data_ptr() + 4 * w0), C.c_void_p(fg.flat.data_ptr() + 4 * w0), w1 - w0,
                                       self.ema_decay, self._ema_from, 0, _p(self.step_t), st), "vg_ema_update")

    def gather_master(self) -> None:
        """A no-op, kept for callers: the sharded update of the mapping Linear all-gathers its fp32 master inside the step, so every
        rank's master is current after every step.  (It issues no collective, so it is safe on a branch that differs by rank.)"""

    def _adamw(self, fp, m, v, lr, st, clip=None, slot=0, ema=None):
        h = self.hyp
        if clip is not None:  # on the exchanged (global) gradient, like clip_grad_norm_ before optimizer.step()
            _lib.check(_lib.lib().vg_grad_clip(_p(fp.grad), fp.total, 1.0 / self.world, float(clip), _p(self.clip_scratch[slot]), st),
                       "vg_grad_clip")
        if ema is None:
            _lib.check(_lib.lib().vg_adamw_step(_p(fp.flat), _p(fp.grad), _p(m), _p(v), _p(fp.shadow), fp.total, lr, h["b1"], h["b2"],
                                                h["eps"], h["wd"], 0, _p(self.step_t), 1.0 / self.world, st), "vg_adamw_step")
        else:  # the same update and the weights' moving average in one pass
            _lib.check(_lib.lib().vg_adamw_ema_step(_p(fp.flat), _p(fp.grad), _p(m), _p(v), _p(fp.shadow), _p(ema), fp.total, lr, h["b1"],
                                                    h["b2"], h["eps"], h["wd"], 0, _p(self.step_t), 1.0 / self.world, self.ema_decay,
                                                    self._ema_from, st), "vg_adamw_ema_step")

    def _loss(self, lo, n, role, slot, st):
        L = _lib.lib()
        off = 4 * lo * self.Kc
        _lib.check(L.vg_gan_loss(C.c_void_p(self.logits.data_ptr() + off), C.c_void_p(self.dlogits.data_ptr() + off),
                                 C.c_void_p(self.losses.data_ptr() + 4 * slot), n * self.Kc, self.kind, role, 1.0, st), "vg_gan_loss")

    def _augment(self, src, dst, params, n: int, site: int, st) -> None:
        """T(src) -> dst for n images at an augmentation site of the step: the gated kernel with the device-resident probability when
        the engine has one, else the existing call."""
        d_, L = self.vit._dims, _lib.lib()
        if self.gated:
            _lib.check(L.vg_diffaug_p_fwd(src, dst, params, n, d_.C, d_.IH, self.aug, self._aug_seed, site, _p(self.step_t), _p(self.ada_state), st),
                       "vg_diffaug_p_fwd")
        else:
            _lib.check(L.vg_diffaug_fwd(src, dst, params, n, d_.C, d_.IH, self.aug, self._aug_seed, site, _p(self.step_t), st), "vg_diffaug_fwd")

    def _ada_update(self, logits_real, st) -> None:
        """The controller on the real rows of the adversarial logits (the first B rows at ``logits_real``); nothing without ADA."""
        if self.ada:
            _lib.check(_lib.lib().vg_ada_update(logits_real, self.B * self.Kc, _p(self.ada_state), self.ada_target, self.ada_step_per_image,
                                                self.ada_interval, _p(self.step_t), st), "vg_ada_update")

    @property
    def ada_p(self) -> float:
        """The augmentation probability now in force (synchronises: for logging)."""
        return float(self._need_ada("ada_p")[0])

    @property
    def ada_rt(self) -> float:
        """r_t = E[sign(D(real))] over the window of the controller's last update (synchronises: for logging)."""
        return float(self._need_ada("ada_rt")[3])

    def _need_ada(self, what: str) -> torch.Tensor:
        if self.ada_state is None:
            raise RuntimeError(f"{what}: this engine holds no augmentation probability (built without aug_p / ada_target)")
        return self.ada_state

    def _ada_options(self):
        return None if not self.gated else (self.aug_p0, self.ada_target, self.ada_interval, self.ada_kimg)

    def _enqueue_two_stream(self) -> None:
        """The step as two concurrent chains (see ``two_stream``).  Everything is enqueued from this thread; the second chain
        forks from and joins the current stream through events, so the whole step is still one capturable graph."""
        L, B = _lib.lib(), self.B
        s0, s1 = torch.cuda.current_stream(), self.side
        st0, st1 = C.c_void_p(s0.cuda_stream), C.c_void_p(s1.cuda_stream)
        (nd_a, nd_b, nd_c, nd_d), ng = self._nets()
        fd, fg = self.vit._flat, self.gen._flat
        img_bytes = self.imgs[0].numel() * 2
        Kc4 = 4 * self.Kc
        off_img = lambda t, n: C.c_void_p(t.data_ptr() + n * img_bytes)  # noqa: E731
        off_log = lambda t, n: C.c_void_p(t.data_ptr() + n * Kc4)       # noqa: E731
        fake_ptr = off_img(self.imgs, B)
        _lib.check(L.vg_zero_tick(_p(fd.grad), fd.total, _p(self.step_t), st0), "vg_zero_tick")
        self.grad2.zero_()
        d_in = self.imgs
        s1.wait_stream(s0)
        # chain 1 (side stream): G forward, then D on the fake batch (weight gradients into grad2)
        with torch.cuda.stream(s1):
            _lib.check(L.vg_gen_forward(C.byref(ng), B, _p(self.z), _p(self.ws_g), fake_ptr, st1), "vg_gen_forward")
            if self.inst_sigma > 0.0:
                self.inoise[B:].normal_()
                torch.add(self.imgs[B:].float(), self.inoise[B:], alpha=self.inst_sigma, out=self.inoise[B:])
                self.imgs_noisy[B:].copy_(self.inoise[B:])
            src = off_img(self.imgs_noisy if self.inst_sigma > 0.0 else self.imgs, B)
            _lib.check(L.vg_vit_forward(C.byref(nd_b), B, src, 1, _p(self.ws_d2), off_log(self.logits, B), st1), "vg_vit_forward")
            _lib.check(L.vg_gan_loss(off_log(self.logits, B), off_log(self.dlogits, B), C.c_void_p(self.losses.data_ptr() + 4), B * self.Kc,
                                     self.kind, 1, 1.0, st1), "vg_gan_loss")
            _lib.check(L.vg_vit_backward(C.byref(nd_b), B, _p(self.ws_d2), off_log(self.dlogits, B), None, 1, st1), "vg_vit_backward")
        # chain 0 (this stream): D on the real batch
        if self.inst_sigma > 0.0:
            self.inoise[:B].normal_()
            torch.add(self.imgs[:B].float(), self.inoise[:B], alpha=self.inst_sigma, out=self.inoise[:B])
            self.imgs_noisy[:B].copy_(self.inoise[:B])
            d_in = self.imgs_noisy
        _lib.check(L.vg_vit_forward(C.byref(nd_a), B, _p(d_in), 1, _p(self.ws_d), _p(self.logits), st0), "vg_vit_forward")
        self._loss(0, B, 0, 0, st0)
        _lib.check(L.vg_vit_backward(C.byref(nd_a), B, _p(self.ws_d), _p(self.dlogits), None, 1, st0), "vg_vit_backward")
        s0.wait_stream(s1)
        fd.grad.add_(self.grad2)  # the two passes accumulate into one .grad in the reference (training.py:184,194)
        self._adamw(fd, self.m_d, self.v_d, self.hyp["lr_d"], st0, self.clip_d, 0)
        fg.grad.zero_()
        # generator's pass through the updated D: two half-batches side by side (no weight gradients, nothing shared)
        h = B // 2
        s1.wait_stream(s0)
        with torch.cuda.stream(s1):
            _lib.check(L.vg_vit_forward(C.byref(nd_d), h, off_img(self.imgs, B + h), 1, _p(self.ws_d2), off_log(self.logits, h), st1), "vg_vit_forward")
        _lib.check(L.vg_vit_forward(C.byref(nd_c), h, fake_ptr, 1, _p(self.ws_d), _p(self.logits), st0), "vg_vit_forward")
        s0.wait_stream(s1)
        self._loss(0, B, 2, 2, st0)  # one mean over the whole batch
        s1.wait_stream(s0)
        with torch.cuda.stream(s1):
            _lib.check(L.vg_vit_backward(C.byref(nd_d), h, _p(self.ws_d2), off_log(self.dlogits, h), off_img(self.dfake, h), 0, st1), "vg_vit_backward")
        _lib.check(L.vg_vit_backward(C.byref(nd_c), h, _p(self.ws_d), _p(self.dlogits), _p(self.dfake), 0, st0), "vg_vit_backward")
        s0.wait_stream(s1)
        if self.div_w != 0.0:
            Dn = self.dfake[0].numel()
            _lib.check(L.vg_diversity_loss(fake_ptr, _p(self.dfake), _p(self.div_loss), _p(self.div_scratch), B, Dn, self.div_w, st0),
                       "vg_diversity_loss")
        _lib.check(L.vg_gen_backward(C.byref(ng), B, _p(self.ws_g), _p(self.dfake), st0), "vg_gen_backward")
        self._adamw(fg, self.m_g, self.v_g, self.hyp["lr_g"], st0, self.clip_g, 1, self.ema_g)

    def _inputs(self, real: torch.Tensor) -> None:
        """The step's inputs, ONE launch in front of the step proper (and outside its hipGraph, so it reads the caller's tensor
        directly - no staging copy): imgs[:B] = bf16(real), and unless the caller supplies it, the latent batch z ~ N(0, 1)
        (construct_noise(), training.py:35-42 / gan.py:231-232), counter-based on (seed, rank, steps done so far)."""
        B = self.B
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        # the kernel dereferences the caller's pointer with 16-byte loads on THIS engine's device: anything else (another GPU's
        # tensor, an unaligned view) goes through torch's copy, which handles it
        direct = (real.dtype == torch.float32 and real.is_contiguous() and real[0].numel() == self.imgs[0].numel() and real.numel() % 4 == 0
                  and real.device == self.imgs.device and real.data_ptr() % 16 == 0)
        if not direct:
            self.imgs[:B].copy_(real)
        want_z = not self.external_noise
        if direct or want_z:
            _lib.check(_lib.lib().vg_step_inputs(_p(real) if direct else None, _p(self.imgs), real.numel() if direct else 0,
                                                 _p(self.z) if want_z else None, self.z.numel() if want_z else 0, self._noise_seed,
                                                 _p(self.step_t), st), "vg_step_inputs")

    def _enqueue(self, real: torch.Tensor) -> None:
        """Enqueue one full step on the current stream (no host sync)."""
        self._inputs(real)
        self._enqueue_body()

    def _enqueue_body(self) -> None:
        """Everything of a step behind its inputs (``_inputs``): what the hipGraph captures."""
        if self.two_stream:
            return self._enqueue_two_stream()
        L, B = _lib.lib(), self.B
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        (nd, nd_b, nd_c), ng = self._nets()
        fd, fg = self.vit._flat, self.gen._flat
        d_ = self.vit._dims
        img_bytes = self.imgs[0].numel() * 2
        fake_ptr = C.c_void_p(self.imgs.data_ptr() + B * img_bytes)
        # gan.discriminator.zero_grad() (training.py:177) and the device step counter += 1, one launch
        _lib.check(L.vg_zero_tick(_p(fd.grad), fd.total, _p(self.step_t), st), "vg_zero_tick")
        _lib.check(L.vg_gen_forward(C.byref(ng), B, _p(self.z), _p(self.ws_g), fake_ptr, st), "vg_gen_forward")
        d_in = self.imgs
        if self.inst_sigma > 0.0:  # noisy_real / noisy_fake of training.py:83-90 (the clean fake stays in self.imgs for pass C)
            self.inoise.normal_()
            torch.add(self.imgs.float(), self.inoise, alpha=self.inst_sigma, out=self.inoise)
            self.imgs_noisy.copy_(self.inoise)
            d_in = self.imgs_noisy
        if self.aug:  # D sees T_1([real ; fake]) (site 0), and so does the penalty below
            self._augment(_p(d_in), _p(self.imgs_aug), _p(self.aug_params["d"]), 2 * B, 0, st)
            d_in = self.imgs_aug
        if self.bcr_policy:  # the consistency partner T_c(x) (site 2) behind x in the 4B buffer; the losses and the penalty stay on x
            _lib.check(L.vg_diffaug_fwd(_p(d_in), _p(self.imgs_bcr), _p(self.aug_params["c"]), 2 * B, d_.C, d_.IH, self.bcr_policy,
                                        self._aug_seed, 2, _p(self.step_t), st), "vg_diffaug_fwd")
        if self.gp_c_call:  # gradient_penalty(D, noisy_real, noisy_fake) joins the D loss (training.py:101-106): one C call
            if self.gp_epsilon is not None:
                torch.add(self.gp_epsilon.reshape(-1).float(), 0.0, out=self.gp_eps)  # (an elementwise kernel, not a D2D copy: no memcpy / memset nodes in the captured step)
            else:
                self.gp_eps.uniform_()  # epsilon = torch.rand(B, 1, 1, 1), utils.py:129
            pnet = _lib.VgVitNet(self.vit._dims, fd.flat.data_ptr(), fd.shadow.data_ptr(), fd.grad.data_ptr(), self.p_d, self.seed * 8 + 3,
                                 self.step_t.data_ptr(), None, 0, 1)
            _lib.check(L.vg_vit_penalty(C.byref(pnet), B, _p(d_in), C.c_void_p(d_in.data_ptr() + B * img_bytes), _p(self.gp_eps), self.gp_w,
                                        _p(self.ws_d), _p(self.ws_gp), _p(self.gp_loss), st), "vg_vit_penalty")
        elif self.gp_w != 0.0:
            from .penalty import gradient_penalty
            fd.attach_grads()
            disc = self.vit
            from . import ops2
            pen = gradient_penalty(disc, d_in[:B], d_in[B:], epsilon=self.gp_epsilon)
            with ops2.deferred_weight_grads(fd.grad):  # the block Linears' weight gradients: grouped per block, straight into the flat buffer
                (self.gp_w * pen).backward()   # the rest accumulates into the same buffer through the parameters' .grad (views of it)
            self.gp_loss.copy_(pen.detach().reshape(1))
        if self.bcr:
            # ONE pass over [x ; T(x)]: rows [0, 2B) the clean pair, rows [2B, 4B) its transform.  The adversarial rows are T_1(x) with
            # diffaug and x without it; the consistency loss adds to their gradient and writes the partner rows' (every element)
            adv_a = int(bool(self.aug))
            half = 4 * 2 * B * self.Kc  # bytes of 2B logit rows
            lx, la = _p(self.logits), C.c_void_p(self.logits.data_ptr() + half)
            dx, da = _p(self.dlogits), C.c_void_p(self.dlogits.data_ptr() + half)
            _lib.check(L.vg_vit_forward(C.byref(nd), 4 * B, _p(self.imgs4), 1, _p(self.ws_d), lx, st), "vg_vit_forward")
            _lib.check(L.vg_gan_loss_pair(la if adv_a else lx, da if adv_a else dx, _p(self.losses), B * self.Kc, 0, B * self.Kc, 1, self.kind,
                                          1.0, st), "vg_gan_loss_pair")
            self._ada_update(la if adv_a else lx, st)
            _lib.check(L.vg_bcr_loss(lx, la, dx, da, _p(self.bcr_losses), B, B, self.Kc, self.bcr_w[0], self.bcr_w[1], 1 - adv_a, adv_a, 1.0, st),
                       "vg_bcr_loss")
            self._d_backward(nd, 4 * B, dx, 1, None, st)
        elif self.fuse:
            _lib.check(L.vg_vit_forward(C.byref(nd), 2 * B, _p(d_in), 1, _p(self.ws_d), _p(self.logits), st), "vg_vit_forward")
            # D(real) -> slot 0, D(fake) -> slot 1: both halves of the fused pass in one launch
            _lib.check(_lib.lib().vg_gan_loss_pair(_p(self.logits), _p(self.dlogits), _p(self.losses), B * self.Kc, 0, B * self.Kc, 1, self.kind,
                                                   1.0, st), "vg_gan_loss_pair")
            self._ada_update(_p(self.logits), st)
            self._d_backward(nd, 2 * B, _p(self.dlogits), 1, None, st)
        else:
            for half, role in ((0, 0), (1, 1)):
                src = C.c_void_p(d_in.data_ptr() + half * B * img_bytes)
                lg = C.c_void_p(self.logits.data_ptr() + 4 * half * B * self.Kc)
                dl = C.c_void_p(self.dlogits.data_ptr() + 4 * half * B * self.Kc)
                net = nd if half == 0 else nd_b
                _lib.check(L.vg_vit_forward(C.byref(net), B, src, 1, _p(self.ws_d), lg, st), "vg_vit_forward")
                self._loss(half * B, B, role, role, st)
                if half == 0:
                    self._ada_update(lg, st)
                    _lib.check(L.vg_vit_backward(C.byref(net), B, _p(self.ws_d), dl, None, 1, st), "vg_vit_backward")
                else:  # second pass finishes D.grad: exchange it as it completes
                    self._d_backward(net, B, dl, 1, None, st)
        self.sync.wait()
        if self.spec is not None:  # dL/dW_eff -> dL/dW on the exchanged total of both passes and the penalty (the map is linear)
            self.spec.project(fd.grad, fd.flat, st)
        self._adamw(fd, self.m_d, self.v_d, self.hyp["lr_d"], st, self.clip_d, 0)
        if self.spec is not None:  # one power iteration on the updated master; AdamW's plain cast of the normalised ranges is overwritten
            self.spec.update(fd.flat, fd.shadow, True, st)
        fg.grad.zero_()            # gan.generator.zero_grad(), training.py:199
        g_in, g_dimg = fake_ptr, _p(self.dfake)
        if self.aug:  # D sees T_2(fake) (site 1); its input gradient goes back through the adjoint into dfake
            g_in, g_dimg = _p(self.imgs_aug), C.c_void_p(self.imgs_aug.data_ptr() + B * img_bytes)
            self._augment(fake_ptr, g_in, _p(self.aug_params["g"]), B, 1, st)
        if self.bcr or self.ada:
            _lib.check(L.vg_vit_forward(C.byref(nd_c), B, g_in, 1, _p(self.ws_d), _p(self.logits_g), st), "vg_vit_forward")
            _lib.check(L.vg_gan_loss(_p(self.logits_g), _p(self.dlogits_g), C.c_void_p(self.losses.data_ptr() + 8), B * self.Kc, self.kind, 2, 1.0, st),
                       "vg_gan_loss")
            _lib.check(L.vg_vit_backward(C.byref(nd_c), B, _p(self.ws_d), _p(self.dlogits_g), g_dimg, 0, st), "vg_vit_backward")
        else:
            _lib.check(L.vg_vit_forward(C.byref(nd_c), B, g_in, 1, _p(self.ws_d), _p(self.logits), st), "vg_vit_forward")
            self._loss(0, B, 2, 2, st)
            _lib.check(L.vg_vit_backward(C.byref(nd_c), B, _p(self.ws_d), _p(self.dlogits), g_dimg, 0, st), "vg_vit_backward")
        if self.aug and self.gated:
            _lib.check(L.vg_diffaug_p_bwd(g_dimg, _p(self.dfake), 0, B, d_.C, d_.IH, self.aug, self._aug_seed, 1, _p(self.step_t),
                                          _p(self.ada_state), st), "vg_diffaug_p_bwd")
        elif self.aug:
            _lib.check(L.vg_diffaug_bwd(g_dimg, _p(self.dfake), 0, B, d_.C, d_.IH, self.aug, self._aug_seed, 1, _p(self.step_t), st), "vg_diffaug_bwd")
        if self.div_w != 0.0:  # total_gen_loss = loss + w * diversity_loss(fake_images): its gradient joins dL/d fake
            Dn = self.dfake[0].numel()
            _lib.check(L.vg_diversity_loss(fake_ptr, _p(self.dfake), _p(self.div_loss), _p(self.div_scratch), B, Dn, self.div_w, st),
                       "vg_diversity_loss")
        self._g_backward(ng, st)
        self.sync.wait()
        if self.shard_map:
            self._adamw_g_sharded(st)
        else:
            self._adamw(fg, self.m_g, self.v_g, self.hyp["lr_g"], st, self.clip_g, 1, self.ema_g)

    # ------------------------------------------------------------------------------------------
    def _state_tensors(self):
        """Everything a step changes that the next step reads (the training state held on the device)."""
        fd, fg = self.vit._flat, self.gen._flat
        state = [fd.flat, fd.shadow, fg.flat, fg.shadow, self.m_d, self.v_d, self.m_g, self.v_g, self.step_t]
        if self.spec is not None:
            state.append(self.spec.state)
        if self.ada_state is not None:
            state.append(self.ada_state)
        return state if self.ema_g is None else state + [self.ema_g]

    def sync_from_modules(self, reset_optimizer: bool = False) -> None:
        """Call after the modules' parameters were changed behind the engine's back (``load_state_dict``, an in-place
        edit): refreshes the bf16 shadows the GEMMs read; ``reset_optimizer`` also clears AdamW's moments and step count
        (a fresh optimizer, which is what the reference has after a restart: it saves no optimizer state,
        training.py:218-226,262-263).  The generator's moving average needs no code here: a plain refresh leaves it alone, and a
        cleared step counter makes the next step's kernel copy the updated weights into it - the average restarts with the optimizer.
        With ``spectral_norm`` a plain refresh keeps the normalisation (the scaled cast from the stored sigma); ``reset_optimizer``
        measures it again: sigma0 = sigma_max of the current weights, so the network is the plain one at that point."""
        if reset_optimizer and self.spec is not None:
            self.spec.measure(self.vit._flat.flat)
        self.vit._flat.refresh_shadow()
        self.gen._flat.refresh_shadow()
        if reset_optimizer:
            for t in (self.m_d, self.v_d, self.m_g, self.v_g, self.step_t):
                t.zero_()
            # the latent noise is keyed on the device step counter just cleared: move to a fresh stream, keyed on the steps this
            # engine has really done, so a restarted run does not replay the first run's latent sequence
            self._noise_seed = (self._noise_seed * 0x9E3779B97F4A7C15 + 0xD1B54A32D192ED03 * (self.steps + 1)) & 0xFFFFFFFFFFFFFFFF

    # ------------------------------------------------------------------------------------------ averaged generator, sampling
    def _need_ema(self, what: str) -> torch.Tensor:
        if self.ema_g is None:
            raise RuntimeError(f"{what}: this engine keeps no averaged generator (built with ema_decay=0)")
        return self.ema_g

    def sample(self, z: torch.Tensor, ema: bool = True) -> torch.Tensor:
        """Images [n, C, IH, IW] (``generator.out_dtype``) of the latent batch ``z`` [n, Z], n any batch size: one forward-only
        vg_gen_forward without dropout on the current stream, from the averaged weights (``ema=True``: ``ema_g`` and a bf16 cast of
        it, recast only after a step or a load) or from the live master and shadow (``ema=False``: what ``G.eval()(z)`` computes).
        It has its own workspace - the step's belongs to the captured graph - and changes no training state."""
        gen, fg = self.gen, self.gen._flat
        if ema:
            self._need_ema("sample(ema=True)")
        if z.dim() != 2 or z.shape[1] != gen._dims.Z or z.shape[0] < 1 or z.device != self.dev:
            raise ValueError(f"z must be a [n, {gen._dims.Z}] tensor on {self.dev}")
        L, n = _lib.lib(), int(z.shape[0])
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        if ema:
            if self._ema_shadow is None:
                self._ema_shadow = torch.empty(fg.total, dtype=torch.bfloat16, device=self.dev)
            key = (self.steps, self._ema_loads)
            if self._ema_cast_key != key:
                _lib.check(L.vg_cast_f32_bf16(_p(self.ema_g), _p(self._ema_shadow), fg.total, st), "vg_cast_f32_bf16")
                self._ema_cast_key = key
            master, shadow = self.ema_g, self._ema_shadow
        else:
            fg.refresh_shadow()  # like a module forward: the same bits after a step, current weights after an in-place edit
            master, shadow = fg.flat, fg.shadow
        need = gen._ws_bytes(n)
        if self._sample_ws is None or self._sample_ws.numel() < need:
            self._sample_ws = torch.empty(need, dtype=torch.uint8, device=self.dev)
        tab = gen.fourier_table
        net = _lib.VgGenNet(gen._dims, master.data_ptr(), shadow.data_ptr(), fg.grad.data_ptr(), 0.0, 0, None, None if tab is None else tab.data_ptr())
        zin = z.detach().float().contiguous()
        img = torch.empty(n, gen.channels, gen.image_size, gen.image_size, dtype=torch.bfloat16, device=self.dev)
        _lib.check(L.vg_gen_forward(C.byref(net), n, _p(zin), _p(self._sample_ws), _p(img), st), "vg_gen_forward")
        return img.to(gen.out_dtype)

    def ema_state_dict(self) -> dict:
        """The averaged generator under the generator's own keys and shapes (fp32 clones): loads ``strict=True`` into a SirenGenerator."""
        e = self._need_ema("ema_state_dict()")
        return {k: e[off:off + flat.numel(shape)].view(shape).clone() for k, (off, shape) in self.gen._flat.slots.items()}

    def load_ema_state_dict(self, sd) -> None:
        """Copy an ``ema_state_dict()`` into the average in place (a captured graph stays valid)."""
        e, slots = self._need_ema("load_ema_state_dict()"), self.gen._flat.slots
        if set(sd) != set(slots):
            odd = sorted(set(sd) ^ set(slots))
            raise ValueError(f"load_ema_state_dict: keys differ from the generator's, e.g. {odd[:3]}")
        for k, (off, shape) in slots.items():
            if tuple(sd[k].shape) != tuple(shape):
                raise ValueError(f"load_ema_state_dict: {k} has shape {tuple(sd[k].shape)}, the generator's is {tuple(shape)}")
        with torch.no_grad():
            for k, (off, shape) in slots.items():
                e[off:off + flat.numel(shape)].view(shape).copy_(sd[k])
        self._ema_loads += 1

    # ------------------------------------------------------------------------------------------ training state across a restart
    STATE_FORMAT = 1

    def state_dict(self) -> dict:
        """The engine's training state - what ``gan.state_dict()`` (the networks' weights) does not hold: AdamW's moments, the
        device step counter (it keys the bias corrections, the dropout masks, the latent noise and the augmentation), the host's
        step count, the current latent-noise stream and, when they are on, the generator's moving average and the augmentation
        probability with its controller."""
        sd = {"format_version": self.STATE_FORMAT, "steps": int(self.steps), "noise_seed": int(self._noise_seed)}
        for k in ("m_d", "v_d", "m_g", "v_g", "step_t"):
            sd[k] = getattr(self, k).detach().clone()
        if self.ema_g is not None:
            sd["ema_g"] = self.ema_g.detach().clone()
        if self.spec is not None:
            sd["spectral_norm"], sd["spectral_state"] = self.spectral_norm, self.spec.state.detach().clone()
        if self.bcr:  # no training state of its own: the options, so that a resumed run is the same run
            sd["bcr"] = self._bcr_options()
        if self.gated:  # the probability and the controller's accumulators, and the options they were run under
            sd["ada"], sd["ada_state"] = self._ada_options(), self.ada_state.detach().clone()
        return sd

    def _bcr_options(self):
        return None if not self.bcr else (self.bcr_w[0], self.bcr_w[1], self.bcr_policy)

    def effective_state_dict(self) -> dict:
        """The discriminator's ``state_dict()`` (the keys of the module the engine was given) with fp32(s * W), s = sigma0 / sigma, in
        place of every normalised W - the kernel's own expression, so a plain bf16 cast of it is this engine's shadow bit for bit.
        It loads into a plain ViTDiscriminator (or the reference's) and computes the trained function.  Without ``spectral_norm``
        it is the plain state."""
        fd = self.vit._flat
        eff = fd.flat.detach().clone() if self.spec is None else self.spec.effective(fd.flat)
        sd = self._disc.state_dict()
        pre = "vit." if self._disc is not self.vit else ""
        for k, (off, shape) in fd.slots.items():
            sd[pre + k] = eff[off:off + flat.numel(shape)].view(shape).clone()
        return sd

    def load_state_dict(self, sd, strict: bool = True) -> None:
        """Restore ``state_dict()`` in place (a captured graph stays valid) and refresh the shadows from the modules' current
        weights - so: load the ``gan`` state, then this, then go on stepping.  Wrong sizes, a missing entry or another format
        version raise ValueError.  An engine with the moving average on that is given a state without ``ema_g`` raises under
        ``strict``; with ``strict=False`` the average restarts as a copy of the weights at the next step (the step is captured again).  The
        spectral-normalisation state follows the same rule: missing under ``strict`` raises, with ``strict=False`` it is measured
        again from the current weights.  Consistency regularisation has no state; the saved ``bcr`` options must equal this engine's under
        ``strict``.  The augmentation probability and its controller (``aug_p`` / ``ada_target``) follow bCR's rule for the options, and
        their state is restored whenever both sides hold one."""
        if sd.get("format_version") != self.STATE_FORMAT:
            raise ValueError(f"engine state format {sd.get('format_version')!r}, this engine reads format {self.STATE_FORMAT}")
        names = ("m_d", "v_d", "m_g", "v_g", "step_t")
        missing = [k for k in names + ("steps", "noise_seed") if k not in sd]
        if missing:
            raise ValueError(f"engine state lacks {missing}")
        has_spec = sd.get("spectral_state") is not None
        if has_spec and self.spec is not None and sd.get("spectral_norm") != self.spectral_norm:
            raise ValueError(f"engine state was saved with spectral_norm={sd.get('spectral_norm')!r}, this engine has {self.spectral_norm!r}")
        if strict and has_spec != (self.spec is not None):
            raise ValueError("engine state has no spectral_state but this engine normalises its discriminator (strict=False measures it again "
                             "from the current weights)" if not has_spec else "engine state has a spectral_state but this engine has spectral_norm off")
        saved_bcr = None if sd.get("bcr") is None else tuple(sd["bcr"])
        if strict and saved_bcr != self._bcr_options():
            raise ValueError(f"engine state was saved with consistency regularisation (lambda_real, lambda_fake, bcr_aug bits) = {saved_bcr!r}, "
                             f"this engine has {self._bcr_options()!r} (strict=False loads it all the same: bCR holds no training state)")
        saved_ada = None if sd.get("ada") is None else tuple(sd["ada"])
        if strict and saved_ada != self._ada_options():
            raise ValueError(f"engine state was saved with (aug_p, ada_target, ada_interval, ada_kimg) = {saved_ada!r}, this engine has "
                             f"{self._ada_options()!r} (strict=False loads the probability all the same when both sides hold one)")
        has_ada = sd.get("ada_state") is not None and self.ada_state is not None
        has_ema = sd.get("ema_g") is not None
        if strict and has_ema != (self.ema_g is not None):
            raise ValueError("engine state has no ema_g but this engine keeps a moving average (strict=False restarts it)" if not has_ema
                             else "engine state has an ema_g but this engine keeps no moving average")
        pairs = [(getattr(self, k), sd[k], k) for k in names]
        if has_ema and self.ema_g is not None:
            pairs.append((self.ema_g, sd["ema_g"], "ema_g"))
        if has_spec and self.spec is not None:
            pairs.append((self.spec.state, sd["spectral_state"], "spectral_state"))
        if has_ada:
            pairs.append((self.ada_state, sd["ada_state"], "ada_state"))
        for dst, src, k in pairs:
            if not torch.is_tensor(src) or src.numel() != dst.numel():
                raise ValueError(f"engine state {k}: {tuple(getattr(src, 'shape', ()))} does not fit this engine's {tuple(dst.shape)}")
        with torch.no_grad():
            for dst, src, _ in pairs:
                dst.copy_(src.reshape(dst.shape))
        self.steps, self._noise_seed = int(sd["steps"]), int(sd["noise_seed"]) & 0xFFFFFFFFFFFFFFFF
        if self.ema_g is not None:
            self._ema_loads += 1
            # no average in the state: the step after the loaded counter copies.  ema_start is an argument of the captured kernel
            # node, so that (rare) case drops the graph; the next step captures it again
            start = self.ema_start if has_ema else max(self.ema_start, int(sd["step_t"].reshape(-1)[0]) + 1)
            if start != self._ema_from:
                self._ema_from, self._graph = start, None
        if self.spec is not None and not has_spec:  # no state to restore: the current weights become the reference point
            self.spec.measure(self.vit._flat.flat)
        self.sync_from_modules()

    def step(self, real: torch.Tensor, z: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Run one G/D step on ``real`` [B,C,IH,IW] (cuda).  Returns the device tensor
        [loss_d_real, loss_d_fake, loss_g] of this step without synchronising.  ``z`` [B, Z]: the latent batch, required
        iff the engine was built with ``external_noise=True``."""
        if real.shape[0] != self.B or not real.is_cuda:
            raise ValueError("real must be a cuda tensor with the engine's batch size")
        if (z is not None) != self.external_noise:
            raise ValueError("pass z exactly when the engine was built with external_noise=True")
        if not (self.vit._flat.aliased() and self.gen._flat.aliased()):
            raise RuntimeError("module parameters were re-allocated; rebuild the GanEngine")
        if z is not None:
            self.z.copy_(z)
        self.steps += 1
        if not self._use_graph:
            self._enqueue(real)
            return self.losses
        if self._graph is None:
            # Warm-up on a side stream (allocator, lazily loaded code objects), then capture.  The warm-up is a real step:
            # the training state is saved before it and restored after it, so N calls of step() are N steps in graph
            # mode exactly as in eager mode (tests compare the two bit for bit).
            saved = [t.clone() for t in self._state_tensors()]
            s = torch.cuda.Stream()
            self._inputs(real)
            s.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(s):
                self._enqueue_body()
            torch.cuda.current_stream().wait_stream(s)
            for t, keep in zip(self._state_tensors(), saved):
                t.copy_(keep)
            graph = torch.cuda.CUDAGraph()
            # With a process group the RCCL watchdog THREAD polls the events of the collectives the warm-up step enqueued: under the default
            # ("global") capture mode such a hipEventQuery from another thread while this one captures is an error that invalidates the
            # capture and, raised inside the watchdog, ends the process (seen once in ~10 runs of the one-rank RCCL test).  "thread_local"
            # confines the restriction to the capturing thread, which is what a captured step with collectives needs.
            mode = "thread_local" if self.sync.active else "global"
            if self.sync.active:
                # ... and the watchdog gets the time to retire the warm-up's (finished) collectives from its list - it polls every 100 ms,
                # and collectives enqueued DURING a capture are never put on that list - so that it has nothing to query while we capture
                torch.cuda.synchronize()
                time.sleep(0.5)
            try:
                with torch.cuda.graph(graph, capture_error_mode=mode):
                    self._enqueue_body()
            except Exception as exc:  # only reachable with collectives or the autograd-driven penalty in the step: otherwise it is all our own enqueue-only calls
                if not self.sync.active and self.gp_w == 0.0:
                    raise
                torch.cuda.synchronize()
                for t, keep in zip(self._state_tensors(), saved):  # a broken capture must not have advanced the state
                    t.copy_(keep)
                self.sync._pending.clear()
                self._graph_fallback(f"capturing the step ({'collectives' if self.sync.active else 'gradient penalty through torch autograd'}) failed: "
                                     f"{type(exc).__name__}: {exc}")
                self._enqueue(real)
                return self.losses
            self._graph = graph
        self._inputs(real)
        self._graph.replay()
        return self.losses
