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
from .data import DeviceDataset, data_seed
from .dist import GradSync, backward_pieces, world_size
from .generator import SirenGenerator
from .modules import ViTDiscriminator, VisionTransformer
from .spectral import SpectralState, parse_spectral_set, vit_matrix_keys

LOSS_KINDS = {"ns": 0, "hinge": 1, "wasserstein": 2}  # "wasserstein": the critic losses of src/v2/training.py:72,97


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
                 aug_p: Optional[float] = None, ada_target: float = 0.0, ada_interval: int = 4, ada_kimg: float = 500.0,
                 r1_gamma: float = 0.0, r1_interval: int = 1, n_classes: int = 0,
                 lr_schedule: str = "", lr_warmup: int = 0, lr_total: int = 0, lr_final: float = 0.0,
                 dataset: Optional[DeviceDataset] = None, telemetry: int = 0):
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
        optimizer kernel itself (the fused AdamW + EMA call of ``_adamw_range``: one pass, 38 B per parameter against AdamW's 30; no extra launch, nothing a
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
        aug_p: the probability with which every member of ``diffaug`` is applied to an image (sites 0 and 1; the gated kernels of
        ``_augment`` / ``_augment_adjoint``: a per-image, per-member gate from the same counter hash, so replays and ranks draw their own).  It lives
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
        ada_interval: steps between two updates of p.  ada_kimg: thousands of real images it takes p to go from 0 to 1.
        r1_gamma: weight gamma of the zero-centred R1 penalty on real images, gamma / 2 E_real ||grad_x D(x)||^2 (Mescheder et al.
        2018; the reference has none) - the regulariser that goes with ``loss="ns"`` / ``"hinge"``, where WGAN-GP's (||g|| - 1)^2 on
        interpolates is the wrong operator.  ONE C call, ``vg_vit_r1`` (the penalty call's passes with the real images in front and
        u = 2 w / B g as the seed of the second backward), where the gradient penalty runs: behind the augmentations, before D's own
        pass, on the real images as that pass sees them (after instance noise and DiffAugment; bCR's partner is not penalised), with
        the penalty call's dropout key.  ``r1_loss`` holds the last computed unweighted penalty.  0.0 (default): nothing - no buffer,
        no call, and the step is launch for launch the plain one.  Not with ``gp_weight`` (one gradient penalty per step: they share
        the workspaces), ``two_stream`` or fp8 attention.
        r1_interval: lazy regularisation (Karras et al. 2020) - the penalty runs on step 1 and every ``r1_interval``-th step after it
        (``ops.r1_due`` on the host's step count, which ``state_dict()`` carries), weighted ``r1_interval * r1_gamma / 2``; the other
        steps are plain steps and leave ``r1_loss`` alone.  Under ``use_graph`` the two launch lists are two captured graphs, each
        warmed up and captured the first time its kind of step occurs.
        n_classes: K > 0 trains a class-conditional pair (the reference hands labels to a loss that cannot take them); it must equal
        the discriminator's ``classes_count`` and the generator's ``n_classes``.  The discriminator is conditioned by the
        label-selected logit of its K-way head, D(x, y) = D(x)[y] (Mescheder et al. 2018): vg_gan_loss_cond_pair / vg_gan_loss_cond
        take the place of the loss launches - the means are over the B samples, every other logit's gradient is +0 - with the real
        labels on the real rows and the fake labels on the fake rows and in the generator's pass.  The generator adds
        ``class_embedding[y]`` to its modulation vector (the _cond generator calls: one launch more per direction).  ``step(real,
        labels=...)`` takes the real labels; the fake labels are drawn on the device, uniform over the classes, by one
        vg_draw_labels in front of the step, keyed on (seed, rank, device step counter) like the latent batch (augmentation seed,
        site 3) - or supplied as ``step(real, z, labels, fake_labels)`` under ``external_noise``.  ``real_labels`` / ``fake_labels``
        hold the last step's, ``selected`` the 2B selected logits of D's own pass.  ADA reads the B selected real logits.  bCR stays on
        ALL Kc logits of both partners: consistency under augmentation is asked of the whole head, not of one class's logit.
        ``sample(z, labels)`` draws from the average; ``state_dict()`` records the class count.  0 (default): no buffer, and the
        step is launch for launch the plain one - a Kc-way head is then B Kc independent samples, as before.  Not with ``gp_weight``
        / ``r1_gamma`` (the penalty call seeds its first backward with ones over all Kc logits and folds that into its second-order
        head: a label-selected seed is a follow-up), ``two_stream``, or a process group of more than one rank (the staged exchange of
        the generator's gradient treats the tail of the flat buffer as final after stage 1; the table is final after stage L+1).
        lr_schedule / lr_warmup / lr_total / lr_final: a learning-rate schedule evaluated ON THE DEVICE (the reference imports
        ReduceLROnPlateau and never steps it, training.py:15,215-216): "constant", "linear" or "cosine", one shape for both networks,
        each on its own base rate ``lr_d`` / ``lr_g``.  With t the device step counter (1 on the first step) the rate of step t is
        base * f(t) * multiplier: f rises as t / lr_warmup over the first ``lr_warmup`` steps, is 1 at t = lr_warmup, then falls -
        linearly, or along half a cosine - to ``lr_final`` at t = ``lr_total`` and stays there ("constant": stays 1; ``lr_warmup > 0``
        with ``lr_schedule=""`` means "constant" with warm-up).  ONE launch of two threads, vg_lr_schedule, right behind vg_zero_tick,
        writes both rates into ``lr_now`` in fp64 rounded once; every AdamW call of the step is then the _dlr form
        (vg_adamw_step_dlr / vg_adamw_ema_step_dlr, the sharded pieces included), which reads its network's rate there - so a captured
        step replays with a fresh rate and a resumed run continues its schedule from the restored counter.  ``lr`` reads the pair in
        force; ``set_lr_scale(d=, g=)`` writes the multipliers (1 at construction; what a plateau rule drives), ``state_dict()`` carries
        them and the four options.  Default ("" and no warm-up): no buffer, the host floats ``hyp["lr_d"]`` / ``hyp["lr_g"]`` as kernel
        arguments, and the step is launch for launch and bit for bit the plain one.  With a schedule on, ``hyp["lr_*"]`` are the base
        rates, read when a step is enqueued (captured).  Goes with every other option and both schedules of the step.
        dataset: a ``DeviceDataset`` (data.py) - the step fetches its own real batch.  ONE vg_dataset_fetch at the HEAD of the step, in
        front of vg_zero_tick and inside the captured graph, writes ``imgs[:B]``, the real labels and ``batch_indices`` from the device
        step counter (the image at position p of epoch e is ``perm_e(p)``, a keyed bijection: include/vitgan_hip.h), followed there by
        the launches that draw z and the fake labels - they read the counter as before.  ``step()`` then takes no ``real`` / ``labels``
        (passing them raises; ``z`` / ``fake_labels`` stay the caller's under ``external_noise``), a replay needs no launch from the host,
        and ``run(n)`` replays n steps.  The data seed is derived from ``seed`` WITHOUT the rank: all ranks walk one permutation and
        rank r of a world of w reads batch ``j w + r`` of it (``rank`` / ``world`` from the process group).  The position is a function of
        the counter ``state_dict()`` carries, so a resumed run continues the epoch where it stopped; the state records (N, B, world,
        shuffle, flip, data seed) and ``load_state_dict`` refuses another.  The set must match the discriminator's geometry, carry
        labels iff ``n_classes > 0`` (their values are not read on the host; the kernels clamp) and hold one global batch.  None
        (default): no buffer, no call, and the step is launch for launch and bit for bit the host-fed one.
        telemetry: an integer ``cap >= 1`` makes the step RECORD itself (the reference's per-step series - losses, D's real / fake
        accuracies, the gradient norms of both networks, src/v2/training.py:80-84,112-123 - which a run of bare hipGraph replays hides
        from the host): at most seven launches more, all inside the captured step - vg_logit_stats behind D's loss launch (on the rows
        ADA reads: the selected logits when class-conditional, all B Kc otherwise), vg_grad_stats (two launches) on D's gradient between
        the clipping and AdamW (the gradient AdamW consumes: exchanged, projected, clipped), the same pair for the generator, and
        vg_telemetry_commit last, which writes row ``(t - 1) % cap`` of the rings from the device step counter t.  ``history()`` reads
        what has been recorded since its last call, ``first_nonfinite_step`` the first recorded step with a NaN / Inf gradient element.
        The rings are a log, not training state: ``state_dict()`` does not carry them, and the warm-up of a captured step and its first
        replay write the same row with the same values.  Not with ``two_stream`` nor a process group of more than one rank (the
        statistics are per process, like ADA's).  0 (default): no buffer, no launch, the same bits."""
        self._check_options(discriminator, generator, dict(locals()))
        self._carve()
        self._attach()

    def _check_options(self, discriminator, generator, o) -> None:
        """Constructor, part 1: every argument error, in a fixed order, from host code alone - no device is touched, so a bad argument
        is reported as such on any machine - and the parsed options on ``self``.  ``o``: the constructor's arguments by name."""
        two_stream, loss, pg = bool(o["two_stream"]), o["loss"], o["process_group"]
        self.aug = ops.parse_aug_policy(o["diffaug"])  # ValueError names the three members
        self.spectral_norm = parse_spectral_set(o["spectral_norm"])  # ValueError names the two sets
        self.bcr_w = ops.parse_bcr_weights(o["bcr"])
        self.bcr_policy = ops.parse_aug_policy(o["bcr_aug"])
        self.bcr = self.bcr_w != (0.0, 0.0)
        self.r1_gamma, self.r1_interval = ops.parse_r1_options(o["r1_gamma"], o["r1_interval"], o["gp_weight"])
        self.r1 = self.r1_gamma > 0.0
        self.lr_opts = ops.parse_lr_schedule(o["lr_schedule"], o["lr_warmup"], o["lr_total"], o["lr_final"])  # None = host floats
        if self.lr_opts is not None:
            for name in ("lr_d", "lr_g"):  # (what vg_lr_schedule refuses as a base rate)
                try:
                    ok = 0.0 < float(o[name]) < float("inf")
                except (TypeError, ValueError):
                    ok = False
                if not ok:
                    raise ValueError(f"lr_schedule: the base rate {name} must be positive and finite, got {o[name]!r}")
        if self.bcr_policy and self.aug:
            raise ValueError("bcr_aug: with diffaug on, diffaug's own transform T_1 is the consistency partner; leave bcr_aug empty")
        if self.bcr_policy and not self.bcr:
            raise ValueError("bcr_aug: a consistency transform without consistency weights (bcr=(0, 0)) would do nothing; set bcr")
        if self.bcr and not (self.aug or self.bcr_policy):
            raise ValueError("bcr: the consistency loss needs a transform - switch diffaug on (its T_1 is the partner) or name one in bcr_aug")
        if self.bcr and two_stream:
            raise ValueError("bcr: the consistency step runs the discriminator once on 4B images, on the single-chain schedule; switch two_stream off")
        if self.bcr and not o["fuse_real_fake"]:
            raise ValueError("bcr: the consistency step runs the discriminator once on 4B images; it needs fuse_real_fake=True")
        p0, self.ada_target, self.ada_interval, self.ada_kimg = ops.parse_ada_options(o["aug_p"], o["ada_target"], o["ada_interval"], o["ada_kimg"],
                                                                                      self.aug, loss)
        self.ada, self.aug_p0 = self.ada_target > 0.0, 1.0 if p0 is None else p0
        self.gated = p0 is not None  # the gated kernels and a device-resident probability
        world = world_size(pg)
        self.tel_cap = ops.parse_telemetry(o["telemetry"])  # 0 = off
        if self.tel_cap and two_stream:
            raise ValueError("telemetry: the recording launches are placed in the single-chain schedule; switch two_stream off")
        if self.tel_cap and world > 1:
            raise ValueError("telemetry: the statistics are per process and are not exchanged; a process group of more than one rank is not built")
        if self.ada and (world > 1 or (o["exchange_single_rank"] and dist.is_available() and dist.is_initialized())):
            raise ValueError("ada_target: the controller's statistics are per process and are not exchanged; under data parallelism use a "
                             "fixed aug_p")
        self.ada_step_per_image = 1.0 / (1000.0 * self.ada_kimg)
        self.ema_decay, self.ema_start = float(o["ema_decay"]), int(o["ema_start"])
        if not 0.0 <= self.ema_decay < 1.0:
            raise ValueError(f"ema_decay must be in [0, 1), got {o['ema_decay']!r}")
        if self.ema_start < 0 or self.ema_start != o["ema_start"]:
            raise ValueError(f"ema_start must be a non-negative integer, got {o['ema_start']!r}")
        if self.aug and two_stream:
            raise ValueError("diffaug: the augmented step is verified on the single-chain schedule only; switch two_stream off")
        if self.spectral_norm and two_stream:
            raise ValueError("spectral_norm: the normalised step is verified on the single-chain schedule only; switch two_stream off")
        vit = discriminator.vit if isinstance(discriminator, ViTDiscriminator) else discriminator
        if not isinstance(vit, VisionTransformer) or not isinstance(generator, SirenGenerator):
            raise TypeError("GanEngine needs a ViTDiscriminator/VisionTransformer and a SirenGenerator")
        if getattr(vit, "precision", "bf16") != "bf16":
            raise ValueError("GanEngine: the fused step is bf16; it does not take a discriminator in precision='fp32'")
        if getattr(generator, "precision", "bf16") != "bf16":
            raise ValueError("GanEngine: the fused step is bf16; it does not take a generator in precision='fp32'")
        self.gp_w = float(o["gp_weight"])
        if self.gp_w != 0.0:
            vit.require_short_attention("gp_weight > 0 (the gradient penalty)")
        if self.r1:
            if two_stream:
                raise ValueError("r1_gamma: the R1 penalty runs on the single-chain schedule only; switch two_stream off")
            if bool(getattr(vit, "attention_fp8", False)):
                raise ValueError("r1_gamma: the R1 penalty is built on the bf16 attention kernels; switch attention_fp8 off")
            vit.require_short_attention("r1_gamma > 0 (the R1 penalty)")
        self.n_classes = K = o["n_classes"]
        if isinstance(K, bool) or not isinstance(K, int) or not 0 <= K <= 16:
            raise ValueError(f"n_classes must be an integer in [0, 16] (0 = unconditional), got {K!r}")
        if K or generator.n_classes:
            if not (vit._dims.Kc == generator.n_classes == K):
                raise ValueError(f"n_classes: the discriminator's head, the generator's table and the engine must agree - classes_count="
                                 f"{vit._dims.Kc}, generator.n_classes={generator.n_classes}, n_classes={K}")
            if self.gp_w != 0.0 or self.r1:
                raise ValueError("n_classes: the gradient penalties (gp_weight, r1_gamma) seed their first backward with ones over all Kc "
                                 "logits; a label-selected penalty is not built - switch the penalty off")
            if two_stream:
                raise ValueError("n_classes: the conditional step is verified on the single-chain schedule only; switch two_stream off")
            if world > 1:
                raise ValueError("n_classes: the staged gradient exchange treats the tail of the generator's flat buffer as final after "
                                 "stage 1, the class table is final after stage L+1; data parallelism over more than one rank is not built")
        self.cond = K > 0
        self.vit, self.gen, self._disc = vit, generator, discriminator
        if loss not in LOSS_KINDS:
            raise ValueError(f"loss must be one of {sorted(LOSS_KINDS)}")
        self.B, self.kind = int(o["batch"]), LOSS_KINDS[loss]
        self.clip_d, self.clip_g = o["clip_d"], o["clip_g"]
        self.compress_map, self._want_shard_map = bool(o["compress_mapping_grad"]), bool(o["shard_mapping_update"])
        if self._want_shard_map and (self.compress_map or self.clip_g is not None):
            raise ValueError("shard_mapping_update excludes compress_mapping_grad and clip_g")
        fp8 = bool(getattr(vit, "attention_fp8", False))
        if self.gp_w != 0.0 and two_stream:
            raise ValueError("gp_weight: the gradient penalty runs through torch autograd on one stream and cannot be forked")
        if self.gp_w != 0.0 and fp8:
            # the penalty path (ops2.py) differentiates the bf16 attention kernels: with fp8 operands in the trained network
            # it would penalise a slightly different function than the one being trained
            raise ValueError("gp_weight: the gradient penalty is built on the bf16 attention kernels; switch attention_fp8 off")
        d, g = vit._dims, generator._dims
        if g.T * g.CW != d.C * d.IH * d.IH:
            raise ValueError("generator output does not match the discriminator's image shape")
        if two_stream and world > 1:
            raise ValueError("two_stream is a single-GPU schedule (the data-parallel path overlaps the exchange instead)")
        if two_stream and self.B % 2:
            raise ValueError("two_stream needs an even batch")
        self.two_stream = two_stream
        self.fuse = bool(o["fuse_real_fake"]) and not two_stream
        self.gp_c_call = self.gp_w != 0.0 and not o["gp_autograd"] and not fp8
        # dropout probabilities: default = what the modules would apply in their current train/eval mode
        self.p_d = float(vit._dropout_p if vit.training else 0.0) if o["d_dropout"] is None else float(o["d_dropout"])
        self.p_g = float(generator.dropout_p if generator.training else 0.0) if o["g_dropout"] is None else float(o["g_dropout"])
        self.hyp = dict(lr_d=o["lr_d"], lr_g=o["lr_g"], wd=o["weight_decay"], b1=o["betas"][0], b2=o["betas"][1], eps=o["eps"])
        self.dp_chunks = 3  # pieces of the D / G backward whose gradient exchange overlaps the remaining backward
        self.seed, self.dense_top, self.external_noise = int(o["seed"]), int(bool(o["dense_top_block"])), bool(o["external_noise"])
        self.div_w, self.inst_sigma = float(o["diversity_weight"]), float(o["instance_noise"])
        self.pg, self._single_rank = pg, o["exchange_single_rank"]
        self._want_ctx, self._use_graph = bool(o["concurrent_wgrad"]), bool(o["use_graph"])
        self.dataset = ds = o["dataset"]
        if ds is not None:
            if not isinstance(ds, DeviceDataset):
                raise TypeError(f"dataset must be a DeviceDataset, got {type(ds).__name__}")
            if (ds.C, ds.IH) != (d.C, d.IH):
                raise ValueError(f"dataset: its images are {ds.C} x {ds.IH} x {ds.IH}, the discriminator takes {d.C} x {d.IH} x {d.IH}")
            if (ds.labels is not None) != self.cond:
                raise ValueError(f"dataset: labels go with a class-conditional engine and only with one - the dataset "
                                 f"{'has' if ds.labels is not None else 'has no'} labels, n_classes={K}")
            if len(ds) < self.B * world:
                raise ValueError(f"dataset: {len(ds)} images are fewer than one global batch of {self.B} x {world} rank(s)")
            self.data_seed, self._data_world = data_seed(self.seed), world

    def _carve(self) -> None:
        """Constructor, part 2: the device check, the exchange, every buffer the step owns - and every SUB-RANGE the step addresses as a
        view of its buffer, made here once: the step itself slices nothing and computes no pointer."""
        vit, generator = self.vit, self.gen
        self.dev = dev = vit._flat.flat.device
        if dev.type != "cuda" or generator._flat.flat.device != dev:
            raise RuntimeError("GanEngine: both networks must be on the same cuda device (no CPU fallback)")
        self.sync = GradSync(self.pg, dev, overlap=True, single_rank=self._single_rank)
        self.world = self.sync.world
        d, g, B = vit._dims, generator._dims, self.B
        # (a layer that does not divide over the ranks keeps the all-reduce; a one-rank group - `exchange_single_rank` - runs the same calls)
        self.shard_map = self._want_shard_map and self.sync.active and (g.T * g.E * g.Z) % (4 * self.world) == 0
        # latent noise drawn on the device (vg_step_inputs): one stream per (seed, rank)
        self._noise_seed = (self.seed * 0x9E3779B97F4A7C15 + 0xD1B54A32D192ED03 * (self.sync.rank + 1)) & 0xFFFFFFFFFFFFFFFF
        # differentiable augmentation (vg_diffaug_fwd): its own stream per (seed, rank), apart from the latent noise's
        self._aug_seed = (self._noise_seed ^ 0xA0761D6478BD642F) & 0xFFFFFFFFFFFFFFFF
        L = _lib.lib()
        f32 = lambda *shape: torch.zeros(*shape, dtype=torch.float32, device=dev)  # noqa: E731
        images = lambda n: torch.empty(n, d.C, d.IH, d.IH, dtype=torch.bfloat16, device=dev)  # noqa: E731
        self.gp_loss, self.div_loss = f32(1), f32(1)
        self.gp_epsilon: Optional[torch.Tensor] = None  # tests: a fixed epsilon [B,1,1,1] instead of torch.rand
        self.clip_scratch = f32(2, 1 + 1024)  # [net][norm, partials]
        self.clip_slot = tuple(self.clip_scratch)
        nD = 4 * B if self.bcr else (2 * B if self.fuse else B)
        self.ws_d = torch.empty(L.vg_vit_ws_bytes(C.byref(d), nD), dtype=torch.uint8, device=dev)
        if self.two_stream:  # second chain: its own workspace, gradient buffer and stream
            self.ws_d2 = torch.empty(L.vg_vit_ws_bytes(C.byref(d), B), dtype=torch.uint8, device=dev)
            self.grad2 = torch.zeros_like(vit._flat.grad)
            self.side = torch.cuda.Stream(device=dev)
        if self.gp_c_call or self.r1:  # the penalty's own passes: its forward runs in ws_d (the step's passes come after it), the rest here
            self.ws_gp = torch.empty(L.vg_vit_penalty_ws_bytes(C.byref(d), B), dtype=torch.uint8, device=dev)
        if self.gp_c_call:
            self.gp_eps = torch.empty(B, dtype=torch.float32, device=dev)
        self.r1_loss: Optional[torch.Tensor] = f32(1) if self.r1 else None  # the last computed unweighted penalty
        self.ws_g = torch.empty(L.vg_gen_ws_bytes(C.byref(g), B), dtype=torch.uint8, device=dev)
        nL, self.Kc = 4 * B if self.bcr else 2 * B, d.Kc  # logit rows of the discriminator's own pass
        if self.bcr:
            # the 4B images of D's pass, [x ; T(x)], in one buffer: x = the (noisy) pair, T(x) = imgs_aug (diffaug) or imgs_bcr - the
            # step's own buffers are views of it, so no copy launch forms the batch
            self.imgs4 = images(4 * B)
        noisy = self.inst_sigma > 0.0
        # [real ; fake]; the instance noise needs the clean fake behind it (the generator's pass), so then x is imgs_noisy
        self.imgs = self.imgs4[:2 * B] if self.bcr and not noisy else images(2 * B)
        self.dfake = images(B)
        self.img_numel = self.dfake[0].numel()
        self.x = self.imgs  # the pair D's own step is given
        if noisy:  # noisy copy of [real ; fake] for the D step, and the noise itself (kept for inspection / tests)
            self.inoise = torch.empty(2 * B, d.C, d.IH, d.IH, dtype=torch.float32, device=dev)
            self.x = self.imgs_noisy = self.imgs4[:2 * B] if self.bcr else torch.empty_like(self.imgs)
            whole = (self.imgs, self.inoise, self.imgs_noisy)  # (clean, noise, noisy): the step's one part, or the two chains' halves
            self.noise_parts = [tuple(t[:B] for t in whole), tuple(t[B:] for t in whole)] if self.two_stream else [whole]
        if self.aug:
            # D step: imgs_aug = T_1(D's input pair).  Generator pass: imgs_aug[:B] = T_2(fake), imgs_aug[B:] = dL/d T_2(fake)
            self.imgs_aug = self.imgs4[2 * B:] if self.bcr else torch.empty_like(self.imgs)
            self.aug_params = {"d": f32(2 * B, 8), "g": f32(B, 8)}  # (b, s, k, tx, ty, cx, cy, policy) per row
        if self.bcr_policy:  # T_c(x), site 2
            self.imgs_bcr = self.imgs4[2 * B:]
            self.aug_params = {"c": f32(2 * B, 8)}
        if self.bcr:
            self.bcr_losses = f32(2)  # the unweighted means: real, fake
        self.div_scratch = f32((d.C * d.IH * d.IH + 15) // 16)
        rows = lambda n: torch.empty(n, d.Kc, dtype=torch.float32, device=dev)  # noqa: E731
        self.logits, self.dlogits = rows(nL), rows(nL)
        # (p, acc_sign, acc_count, r_last) of include/vitgan_hip.h, vg_ada_update: element 0 is the gated kernels' prob_dev
        self.ada_state: Optional[torch.Tensor] = torch.tensor([self.aug_p0, 0.0, 0.0, 0.0], dtype=torch.float32, device=dev) if self.gated else None
        if self.bcr or self.ada:  # the generator's pass gets rows of its own, so ``logits`` still holds D's whole pass after the step
            self.logits_g, self.dlogits_g = rows(B), rows(B)
        self.z = torch.empty(B, g.Z, dtype=torch.float32, device=dev)
        # class conditioning: the labels of D's pair [real ; fake] in one buffer (the pair launch reads it whole) and the selected logits
        self.real_labels = self.fake_labels = self.selected = None
        if self.cond:
            self.labels_d = torch.zeros(2 * B, dtype=torch.int32, device=dev)
            self.real_labels, self.fake_labels = self.labels_d[:B], self.labels_d[B:]
            self.selected = f32(2 * B)
            self.sel_half = (self.selected[:B], self.selected[B:])
        self.losses = f32(3)  # d_real, d_fake, g
        self.batch_indices: Optional[torch.Tensor] = None
        if self.dataset is not None:  # the set moves to this device once and stays uint8; the last fetch's indices for inspection
            self.dataset.to(dev)
            self.batch_indices = torch.zeros(B, dtype=torch.int32, device=dev)
            self.real_dst = self.imgs[:B]
        self.step_t = torch.zeros(1, dtype=torch.int32, device=dev)
        fd, fg = vit._flat, generator._flat
        self.m_d, self.v_d = torch.zeros_like(fd.flat), torch.zeros_like(fd.flat)
        self.m_g, self.v_g = torch.zeros_like(fg.flat), torch.zeros_like(fg.flat)
        # the generator's averaged weights (a copy of the master until the first step, which copies again: see ema_decay)
        self.ema_g: Optional[torch.Tensor] = fg.flat.detach().clone() if self.ema_decay > 0.0 else None
        # the scheduled rates: the multipliers (training state, written by set_lr_scale) and what vg_lr_schedule writes each step
        self.lr_scale: Optional[torch.Tensor] = None
        self.lr_now: Optional[torch.Tensor] = None
        if self.lr_opts is not None:
            self.lr_scale, self.lr_now = torch.ones(2, dtype=torch.float32, device=dev), f32(2)
            self.lr_slot = (self.lr_now[0:1], self.lr_now[1:2])  # slot 0 = D, 1 = G: the _dlr calls' lr_dev
        if self.tel_cap:  # the per-step record: one plan per gradient buffer, the logit statistics, the three rings (a log, not state)
            cap = self.tel_cap
            self.tel_d, self.tel_g = ops.GradStatsPlan(fd.slots, fd.total, dev), ops.GradStatsPlan(fg.slots, fg.total, dev)
            self.tel_logit = torch.full((3, 4), float("nan"), dtype=torch.float32, device=dev)  # slots: D on real, D on fake, G's pass
            self.tel_sel_g = f32(B) if self.cond else None  # the generator pass's selected logits
            self.tel_ring_step = torch.zeros(cap, dtype=torch.int32, device=dev)
            self.tel_ring = torch.full((cap, _lib.TEL_NF), float("nan"), dtype=torch.float32, device=dev)
            self.tel_ring_seg = (f32(cap, self.tel_d.n_seg), f32(cap, self.tel_g.n_seg))
        # ---- the views: what each pass reads and writes, chosen here once
        halves = lambda t: (t[:B], t[B:2 * B])  # noqa: E731
        self.fake = self.imgs[B:]
        self.loss_slot = tuple(self.losses[i:i + 1] for i in range(3))
        self.d_in = self.imgs_aug if self.aug else self.x  # what D's own pass, and the penalty, see
        self.d_in_half, self.lg_half, self.dlg_half = halves(self.d_in), halves(self.logits), halves(self.dlogits)
        if self.bcr:
            # ONE pass over [x ; T(x)]: rows [0, 2B) the clean pair, rows [2B, 4B) its transform.  The adversarial rows are T_1(x) with
            # diffaug and x without it; the consistency loss adds to their gradient and writes the partner rows' (every element)
            self.cr_rows = (self.logits[:2 * B], self.logits[2 * B:], self.dlogits[:2 * B], self.dlogits[2 * B:])  # D(x), D(T(x)), and their gradients
            self.d_pass = (4 * B, self.imgs4) + (self.cr_rows[1::2] if self.aug else self.cr_rows[0::2])
        else:
            self.d_pass = (2 * B, self.d_in, self.logits, self.dlogits)  # (images, input, adversarial logits, their gradient)
        self.tel_adv = (self.d_pass[2][:B], self.d_pass[2][B:2 * B])  # the adversarial rows' halves: what the logit statistics read
        # the generator's pass through D: D sees T_2(fake) (site 1) under diffaug, its input gradient goes back through the adjoint
        self.g_in, self.g_dimg = (self.imgs_aug[:B], self.imgs_aug[B:]) if self.aug else (self.fake, self.dfake)
        self.g_rows = (self.logits_g, self.dlogits_g) if self.bcr or self.ada else (self.lg_half[0], self.dlg_half[0])
        if self.two_stream:  # the generator's pass as two half-batches: (fake rows, logits, their gradient, dfake rows) of each chain
            h = B // 2
            self.g_half = [tuple(t[i * h:(i + 1) * h] for t in (self.fake, self.logits, self.dlogits, self.dfake)) for i in (0, 1)]
        # AdamW's ranges: a whole network, or with the mapping Linear sharded the three pieces of the generator and the layer itself
        cut = lambda lo, hi, ema=self.ema_g: self._range(fg, self.m_g, self.v_g, ema, lo, hi)  # noqa: E731
        self.r_d, self.r_g = self._range(fd, self.m_d, self.v_d, None, 0, fd.total), cut(0, fg.total)
        if self.shard_map:
            w0, w1 = self._map_range()
            a, b = self.sync.share(w0, w1)
            self.r_g_pieces, self.r_g_map = (cut(0, w0), cut(a, b, None), cut(w1, fg.total)), cut(w0, w1)

    def _attach(self) -> None:
        """Constructor, part 3: what ties the engine to its modules and to the run - the spectral state, the shadows, the
        load_state_dict hooks, the graph flags."""
        vit, fd, fg = self.vit, self.vit._flat, self.gen._flat
        self._ema_from = self.ema_start  # the kernels' ema_start (a non-strict load_state_dict without an average moves it)
        self._ema_shadow: Optional[torch.Tensor] = None  # bf16 cast of ema_g for sample(): allocated on first use
        self._ema_cast_key, self._ema_loads = None, 0    # (steps, loads) the cast was made at
        self._sample_ws: Optional[torch.Tensor] = None
        self.spec: Optional[SpectralState] = None
        if self.spectral_norm:
            keys = vit_matrix_keys(vit._dims.L, self.spectral_norm)
            ent = [(fd.slots[k][0], fd.slots[k][1][0], flat.numel(fd.slots[k][1][1:])) for k in keys]
            self.spec = SpectralState(ent, fd.total, self.dev, names=keys)
            self.spec.measure(fd.flat)
            fd.spectral = self.spec  # from here on every refresh_shadow() of the discriminator writes the normalised cast
        fd.refresh_shadow()
        fg.refresh_shadow()
        self.ctx = _lib.context() if self._want_ctx else None
        # a load_state_dict into either network (directly or through a container such as ViTGAN) copies into the flat
        # master buffers in place: refresh the bf16 shadows the GEMMs read, or the next step runs on stale weights
        # (the hook holds the engine weakly: a strong reference from the module would keep every engine ever built on it -
        # workspaces, optimizer moments - alive, and re-run the refresh of stale engines on every later load_state_dict)
        me = weakref.ref(self)

        def _hook(_mod, _keys):
            eng = me()
            if eng is not None:
                eng.sync_from_modules()
        self._hooks = [m.register_load_state_dict_post_hook(_hook) for m in (vit, self.gen)]
        self._tel_cursor = 0  # the last step history() has returned
        self.first_nonfinite_step: Optional[int] = None  # the first recorded step with a NaN / Inf gradient element (history() sets it)
        self.steps, self._graphs = 0, {}  # the captured step(s), by kind: False = the plain launch list, True = with the R1 call
        self.graph_fallback_reason: Optional[str] = None
        if self._use_graph and self.sync.active:
            backend = dist.get_backend(self.pg)
            if backend != "nccl":
                self._graph_fallback(f"process-group backend '{backend}' cannot be captured in a hipGraph (only nccl = RCCL can)", stacklevel=4)

    def _graph_fallback(self, reason: str, stacklevel: int = 3) -> None:
        self._use_graph, self._graphs = False, {}
        self.graph_fallback_reason = reason
        warnings.warn(f"GanEngine: hipGraph replay was requested but the step runs EAGER: {reason}", RuntimeWarning, stacklevel=stacklevel)

    @property
    def graph_active(self) -> bool:
        """True when step() replays a captured hipGraph, False in eager mode (as before, it is already True between construction and the
        first call, which captures).  With lazy R1 there are two kinds of step; ``step()`` captures a kind inside the call in which it
        first occurs, or falls back to eager for good, so after any ``step()`` every kind that has occurred is captured."""
        return self._use_graph

    def close(self) -> None:
        """Detach from the modules (load_state_dict hooks) and drop the captured graph and workspaces."""
        for h in self._hooks:
            h.remove()
        self._hooks, self._graphs = [], {}
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
        tab = self.gen.fourier_table
        ng = _lib.VgGenNet(self.gen._dims, fg.flat.data_ptr(), fg.shadow.data_ptr(), fg.grad.data_ptr(), self.p_g, self.seed * 8 + 7, step_ptr,
                           None if tab is None else tab.data_ptr())
        if self.cond:  # the generator's passes take the fake labels and the table's shadow and gradient (the _cond calls)
            self._gcond = self.gen._cond(self.fake_labels)
        if self.two_stream:  # chains run side by side: no third stream inside a pass; the fake chain accumulates into grad2
            return (mk(0, ctx=False), mk(1, self.grad2, ctx=False), mk(2, ctx=False), mk(3, ctx=False)), ng
        return (mk(0), mk(1), mk(2)), ng

    # ---- the helpers every schedule is written in: one call site per job
    def _d_forward(self, net, n: int, src, ws, logits, st) -> None:
        _lib.call("vg_vit_forward", C.byref(net), n, _lib.ptr(src), 1, _lib.ptr(ws), _lib.ptr(logits), st)

    def _loss(self, logits, dlogits, n: int, role: int, st) -> None:
        """The loss of n logit rows in ``role`` (0 = D on real, 1 = D on fake, 2 = the generator's) into the role's slot of ``losses``."""
        if self.cond:  # the label-selected logit of each row: real labels for D on real, the fake labels for D on fake and for G
            _lib.call("vg_gan_loss_cond", _lib.ptr(logits), _lib.ptr(self.fake_labels if role else self.real_labels), _lib.ptr(dlogits),
                      _lib.ptr(self.sel_half[role] if role < 2 else (self.tel_sel_g if self.tel_cap else None)), _lib.ptr(self.loss_slot[role]), n, self.Kc,
                      self.kind, role, 1.0, st)
            return
        _lib.call("vg_gan_loss", _lib.ptr(logits), _lib.ptr(dlogits), _lib.ptr(self.loss_slot[role]), n * self.Kc, self.kind, role, 1.0, st)

    def _g_forward(self, ng, st) -> None:
        """fake = G(z), conditioned on the fake labels when the engine is class-conditional"""
        if self.cond:
            _lib.call("vg_gen_forward_cond", C.byref(ng), self.B, _lib.ptr(self.z), _lib.ptr(self.ws_g), _lib.ptr(self.fake), C.byref(self._gcond), st)
        else:
            _lib.call("vg_gen_forward", C.byref(ng), self.B, _lib.ptr(self.z), _lib.ptr(self.ws_g), _lib.ptr(self.fake), st)

    def _d_backward(self, nd, n_img: int, ws, dl, want_w: int, dimg, st, exchange: bool = True) -> None:
        """D backward; under data parallelism, when the pass completes D.grad (``exchange``), in ``dp_chunks`` pieces (head + upper
        blocks first) so that the all-reduce of each finished piece - a contiguous tail of the flat gradient buffer - overlaps the
        backward of the blocks below it; only the last piece's exchange is exposed."""
        if not (self.sync.active and want_w and exchange):
            _lib.call("vg_vit_backward", C.byref(nd), n_img, _lib.ptr(ws), _lib.ptr(dl), _lib.ptr(dimg), want_w, st)
            return
        fd = self.vit._flat
        lay = flat.vit_layout(self.vit._dims)
        for s0, s1, lo, hi in backward_pieces(self.vit._dims.L, self.dp_chunks, lay.layer0, lay.layer_stride, fd.total):
            _lib.call("vg_vit_backward_stages", C.byref(nd), n_img, _lib.ptr(ws), _lib.ptr(dl), _lib.ptr(dimg), want_w, s0, s1, st)
            self.sync.reduce_range(fd.grad, lo, hi)

    def _instance_noise(self, part) -> None:
        """noisy_real / noisy_fake of training.py:83-90 for one part of the pair (the clean fake stays in ``imgs`` for the generator's pass)"""
        clean, noise, noisy = part
        noise.normal_()
        torch.add(clean.float(), noise, alpha=self.inst_sigma, out=noise)
        noisy.copy_(noise)

    def _augment(self, src, dst, params, n: int, policy: int, site: int, st) -> None:
        """T(src) -> dst for n images at an augmentation site of the step: the gated kernel with the device-resident probability when
        the engine has one (sites 0 and 1: an engine with a probability has no site 2), else the plain call."""
        _lib.call("vg_diffaug_p_fwd" if self.gated else "vg_diffaug_fwd", _lib.ptr(src), _lib.ptr(dst), _lib.ptr(params), *self._aug_site(n, policy, site, st))

    def _augment_adjoint(self, dy, dx, n: int, policy: int, site: int, st) -> None:
        """dx = T^T(dy), the transform of ``_augment`` at the same site and step, gated like it."""
        _lib.call("vg_diffaug_p_bwd" if self.gated else "vg_diffaug_bwd", _lib.ptr(dy), _lib.ptr(dx), 0, *self._aug_site(n, policy, site, st))

    def _aug_site(self, n: int, policy: int, site: int, st):
        """what the four augmentation calls share: geometry, policy, the draw's key, and for the gated ones the probability"""
        d_ = self.vit._dims
        return (n, d_.C, d_.IH, policy, self._aug_seed, site, _lib.ptr(self.step_t)) + ((_lib.ptr(self.ada_state), st) if self.gated else (st,))

    def _ada_update(self, logits_real, st) -> None:
        """The controller on the real rows of the adversarial logits (the first B rows of ``logits_real``); nothing without ADA."""
        if self.ada and self.cond:  # the B selected real logits D(x, y): what the conditional loss was taken on
            _lib.call("vg_ada_update", _lib.ptr(self.sel_half[0]), self.B, _lib.ptr(self.ada_state), self.ada_target, self.ada_step_per_image,
                      self.ada_interval, _lib.ptr(self.step_t), st)
        elif self.ada:
            _lib.call("vg_ada_update", _lib.ptr(logits_real), self.B * self.Kc, _lib.ptr(self.ada_state), self.ada_target, self.ada_step_per_image,
                      self.ada_interval, _lib.ptr(self.step_t), st)

    def _diversity(self, st) -> None:
        """total_gen_loss = loss + w * diversity_loss(fake_images): its gradient joins dL/d fake; nothing at weight 0."""
        if self.div_w != 0.0:
            _lib.call("vg_diversity_loss", _lib.ptr(self.fake), _lib.ptr(self.dfake), _lib.ptr(self.div_loss), _lib.ptr(self.div_scratch), self.B,
                      self.img_numel, self.div_w, st)

    def _map_range(self):
        lay, d = flat.gen_layout(self.gen._dims), self.gen._dims
        return lay.map_w, lay.map_w + d.T * d.E * d.Z

    def _range(self, fp, m, v, ema, lo: int, hi: int):
        """(master, gradient, m, v, shadow, average or None, elements) of [lo, hi) of a network's flat buffers: AdamW's operands"""
        return tuple(None if t is None else t[lo:hi] for t in (fp.flat, fp.grad, m, v, fp.shadow, ema)) + (hi - lo,)

    def _lr_tick(self, st) -> None:
        """Both networks' rates of this step from the counter vg_zero_tick has just advanced (one launch); nothing without a schedule."""
        if self.lr_opts is not None:
            d, g = (ops.lr_sched_struct(self.hyp[k], *self.lr_opts) for k in ("lr_d", "lr_g"))
            _lib.call("vg_lr_schedule", C.byref(d), C.byref(g), _lib.ptr(self.step_t), _lib.ptr(self.lr_scale), _lib.ptr(self.lr_now), st)

    def _adamw_range(self, r, slot: int, st) -> None:
        """AdamW on one range (``_range``) of network ``slot`` (0 = D, 1 = G) - with the weights' moving average in the same pass when
        the range carries one; the rate is the host float, or with a schedule on the slot's float on the device (the _dlr calls)."""
        *bufs, ema, n = r
        if n <= 0:
            return
        h = self.hyp
        dlr = "" if self.lr_opts is None else "_dlr"
        lr = _lib.ptr(self.lr_slot[slot]) if dlr else h["lr_g" if slot else "lr_d"]
        tail = (n, lr, h["b1"], h["b2"], h["eps"], h["wd"], 0, _lib.ptr(self.step_t), 1.0 / self.world)
        if ema is None:
            _lib.call("vg_adamw_step" + dlr, *map(_lib.ptr, bufs), *tail, st)
        else:
            _lib.call("vg_adamw_ema_step" + dlr, *map(_lib.ptr, bufs), _lib.ptr(ema), *tail, self.ema_decay, self._ema_from, st)

    def _adamw(self, r, slot: int, st, clip=None) -> None:
        """A whole network's optimizer step (``slot``: 0 = D, 1 = G): the clipping (on the exchanged, global gradient, like
        clip_grad_norm_ before optimizer.step()), then AdamW on the whole range."""
        if clip is not None:
            _lib.call("vg_grad_clip", _lib.ptr(r[1]), r[-1], 1.0 / self.world, float(clip), _lib.ptr(self.clip_slot[slot]), st)
        self._tel_grad(slot, st)
        self._adamw_range(r, slot, st)

    # ---- telemetry: every launch the option adds; nothing without it
    def _tel_grad(self, slot: int, st) -> None:
        """The per-tensor norms of network ``slot``'s gradient as its AdamW is about to read it (two launches)."""
        if self.tel_cap:
            plan, fp = ((self.tel_d, self.vit._flat), (self.tel_g, self.gen._flat))[slot]
            plan.enqueue(fp.grad, 1.0 / self.world, st)

    def _tel_logits(self, x0, x1, n: int, role: int, st) -> None:
        """mean and the fractions > 0 / < 0 of n logits per row pointer into slot ``role`` (and ``role + 1``) of ``tel_logit``."""
        if self.tel_cap:
            _lib.call("vg_logit_stats", _lib.ptr(x0), _lib.ptr(x1), n, role, _lib.ptr(self.tel_logit), st)

    def _tel_d_logits(self, real, fake, st) -> None:
        """D's own pass: the rows ADA reads - the B selected logits of each half when class-conditional, all B Kc otherwise."""
        if self.tel_cap and self.cond:
            self._tel_logits(self.sel_half[0], self.sel_half[1], self.B, 0, st)
        elif self.tel_cap:
            self._tel_logits(real, fake, self.B * self.Kc, 0, st)

    def _tel_g_logits(self, lg, st) -> None:
        """The generator's pass: the B logits selected by the fake labels when class-conditional, all B Kc otherwise."""
        if self.tel_cap and self.cond:
            self._tel_logits(self.tel_sel_g, None, self.B, 2, st)
        elif self.tel_cap:
            self._tel_logits(lg, None, self.B * self.Kc, 2, st)

    def _tel_commit(self, r1_due: bool, st) -> None:
        """The step's last launch: this step's row of the rings, gathered from where the step left each value."""
        if not self.tel_cap:
            return
        pen = self.gp_loss if self.gp_w != 0.0 else self.r1_loss
        ptr = _lib.ptr
        src = _lib.VgTelemetrySrc(ptr(self.losses), ptr(self.tel_logit), ptr(self.tel_d.totals), ptr(self.tel_g.totals), ptr(pen),
                                  ptr(self.bcr_losses if self.bcr else None), ptr(self.ada_state if self.ada else None), ptr(self.lr_now),
                                  ptr(self.div_loss if self.div_w != 0.0 else None), ptr(self.tel_d.norm_seg), ptr(self.tel_g.norm_seg),
                                  self.tel_d.n_seg, self.tel_g.n_seg, int(self.gp_w != 0.0 or bool(r1_due)))
        _lib.call("vg_telemetry_commit", C.byref(src), _lib.ptr(self.step_t), self.tel_cap, _lib.ptr(self.tel_ring_step), _lib.ptr(self.tel_ring),
                  _lib.ptr(self.tel_ring_seg[0]), _lib.ptr(self.tel_ring_seg[1]), st)

    def _adamw_g_sharded(self, st) -> None:
        """The generator's AdamW with the mapping Linear sharded: the whole buffer but that layer as usual, of the layer this rank's
        share only; then the updated fp32 master shares to every rank and the layer's bf16 shadow cast from them there (the GEMMs of
        every rank read the whole shadow; gathering the master, not the shadow, keeps every rank's master current)."""
        self._tel_grad(1, st)
        for r in self.r_g_pieces:  # below the layer, this rank's share of it (its average comes from the gathered master), above it
            self._adamw_range(r, 1, st)
        w0, w1 = self._map_range()
        self.sync.all_gather_range(self.gen._flat.flat, w0, w1)
        self.sync.wait()
        master, _, _, _, shadow, ema, n = self.r_g_map
        _lib.call("vg_cast_f32_bf16", _lib.ptr(master), _lib.ptr(shadow), n, st)
        if ema is not None:  # the layer's average from the gathered master: what the fused kernel of a replicated run writes
            _lib.call("vg_ema_update", _lib.ptr(ema), _lib.ptr(master), n, self.ema_decay, self._ema_from, 0, _lib.ptr(self.step_t), st)

    def gather_master(self) -> None:
        """A no-op, kept for callers: the sharded update of the mapping Linear all-gathers its fp32 master inside the step, so every
        rank's master is current after every step.  (It issues no collective, so it is safe on a branch that differs by rank.)"""

    def _g_backward(self, ng, st) -> None:
        """G backward; under data parallelism in ``dp_chunks`` pieces like D's: SIREN head + upper blocks first, their
        gradients (a contiguous tail of the flat buffer) are exchanged while the lower blocks still run.  What is left
        exposed is the front of the buffer - learned embedding, mapping Linear, lowest blocks - which only completes
        with the last kernel; its 50 MB mapping-weight part goes over the links as bf16."""
        fg = self.gen._flat
        if not self.sync.active:
            if self.cond:
                _lib.call("vg_gen_backward_cond", C.byref(ng), self.B, _lib.ptr(self.ws_g), _lib.ptr(self.dfake), C.byref(self._gcond), st)
            else:
                _lib.call("vg_gen_backward", C.byref(ng), self.B, _lib.ptr(self.ws_g), _lib.ptr(self.dfake), st)
            return
        lay = flat.gen_layout(self.gen._dims)
        # (a class table sits behind the C layout and is final with the LAST stage: the pieces tile the C layout, the table follows them)
        for s0, s1, lo, hi in backward_pieces(self.gen._dims.L, self.dp_chunks, lay.layer0, lay.layer_stride, lay.total if self.cond else fg.total):
            if self.cond:
                _lib.call("vg_gen_backward_stages_cond", C.byref(ng), self.B, _lib.ptr(self.ws_g), _lib.ptr(self.dfake), s0, s1, C.byref(self._gcond), st)
            else:
                _lib.call("vg_gen_backward_stages", C.byref(ng), self.B, _lib.ptr(self.ws_g), _lib.ptr(self.dfake), s0, s1, st)
            if lo == 0 and (self.compress_map or self.shard_map):  # [embedding | mapping weight | mapping bias, lowest blocks]
                w0, w1 = self._map_range()
                self.sync.reduce_range(fg.grad, 0, w0)
                if self.shard_map:
                    self.sync.reduce_scatter_range(fg.grad, w0, w1)   # this rank keeps the sum of its share only
                else:
                    self.sync.reduce_range(fg.grad, w0, w1, compress=True)
                self.sync.reduce_range(fg.grad, w1, hi)
            else:
                self.sync.reduce_range(fg.grad, lo, hi)
        if self.cond:
            self.sync.reduce_range(fg.grad, lay.total, fg.total)

    @property
    def ada_p(self) -> float:
        """The augmentation probability now in force (synchronises: for logging)."""
        return float(self._need_ada("ada_p")[0])

    @property
    def ada_rt(self) -> float:
        """r_t = E[sign(D(real))] over the window of the controller's last update (synchronises: for logging)."""
        return float(self._need_ada("ada_rt")[3])

    @property
    def lr(self):
        """``(lr_d, lr_g)`` now in force (synchronises: for logging): with a schedule on, what the last step's AdamW read
        ((0, 0) until this engine has run a step); without one, the host floats."""
        if self.lr_opts is None:
            return float(self.hyp["lr_d"]), float(self.hyp["lr_g"])
        d, g = self.lr_now.tolist()
        return d, g

    @property
    def lr_scales(self):
        """The two device multipliers ``(d, g)`` (synchronises: for logging)."""
        d, g = self._need(self.lr_scale, "lr_scales: this engine runs no learning-rate schedule (built without lr_schedule / lr_warmup)").tolist()
        return d, g

    def set_lr_scale(self, d: Optional[float] = None, g: Optional[float] = None) -> None:
        """Write the device multipliers of the scheduled rates (None leaves one alone): the step after the call runs at
        base * f(t) * multiplier.  The write goes to a buffer the step reads, outside the hipGraph like the step's inputs, so a
        captured step needs no new capture.  Under data parallelism the caller sets the SAME value on every rank (nothing exchanges
        the multipliers; the schedule itself is a function of the counter and needs no exchange)."""
        scale = self._need(self.lr_scale, "set_lr_scale: this engine runs no learning-rate schedule (built without lr_schedule / lr_warmup)")
        for i, v in ((0, d), (1, g)):
            if v is None:
                continue
            try:
                ok = 0.0 <= float(v) < float("inf")
            except (TypeError, ValueError):
                ok = False
            if not ok:
                raise ValueError(f"set_lr_scale: a multiplier is a finite, non-negative number, got {v!r}")
            scale[i:i + 1].fill_(float(v))

    def _need_ada(self, what: str) -> torch.Tensor:
        return self._need(self.ada_state, f"{what}: this engine holds no augmentation probability (built without aug_p / ada_target)")

    @staticmethod
    def _need(t, complaint: str) -> torch.Tensor:
        if t is None:
            raise RuntimeError(complaint)
        return t

    def _ada_options(self):
        return None if not self.gated else (self.aug_p0, self.ada_target, self.ada_interval, self.ada_kimg)

    def _r1_options(self):
        return None if not self.r1 else (self.r1_gamma, self.r1_interval)

    def _dataset_options(self):
        ds = self.dataset
        return None if ds is None else (ds.N, self.B, self._data_world, ds.shuffle, ds.flip, self.data_seed)

    def _bcr_options(self):
        return None if not self.bcr else (self.bcr_w[0], self.bcr_w[1], self.bcr_policy)

    # ---- the schedules
    def _enqueue_two_stream(self) -> None:
        """The step as two concurrent chains (see ``two_stream``).  Everything is enqueued from this thread; the second chain
        forks from and joins the current stream through events, so the whole step is still one capturable graph."""
        B = self.B
        s0, s1 = torch.cuda.current_stream(), self.side
        st0, st1 = C.c_void_p(s0.cuda_stream), C.c_void_p(s1.cuda_stream)
        (nd_a, nd_b, nd_c, nd_d), ng = self._nets()
        fd, fg = self.vit._flat, self.gen._flat
        noisy = self.inst_sigma > 0.0
        self._fetch(st0)
        _lib.call("vg_zero_tick", _lib.ptr(fd.grad), fd.total, _lib.ptr(self.step_t), st0)
        self._lr_tick(st0)
        self.grad2.zero_()
        s1.wait_stream(s0)
        # chain 1 (side stream): G forward, then D on the fake batch (weight gradients into grad2)
        with torch.cuda.stream(s1):
            _lib.call("vg_gen_forward", C.byref(ng), B, _lib.ptr(self.z), _lib.ptr(self.ws_g), _lib.ptr(self.fake), st1)
            if noisy:
                self._instance_noise(self.noise_parts[1])
            self._d_forward(nd_b, B, self.d_in_half[1], self.ws_d2, self.lg_half[1], st1)
            self._loss(self.lg_half[1], self.dlg_half[1], B, 1, st1)
            self._d_backward(nd_b, B, self.ws_d2, self.dlg_half[1], 1, None, st1, exchange=False)
        # chain 0 (this stream): D on the real batch
        if noisy:
            self._instance_noise(self.noise_parts[0])
        self._d_forward(nd_a, B, self.d_in_half[0], self.ws_d, self.lg_half[0], st0)
        self._loss(self.lg_half[0], self.dlg_half[0], B, 0, st0)
        self._d_backward(nd_a, B, self.ws_d, self.dlg_half[0], 1, None, st0, exchange=False)
        s0.wait_stream(s1)
        fd.grad.add_(self.grad2)  # the two passes accumulate into one .grad in the reference (training.py:184,194)
        self._adamw(self.r_d, 0, st0, self.clip_d)
        fg.grad.zero_()
        # generator's pass through the updated D: two half-batches side by side (no weight gradients, nothing shared)
        h = B // 2
        (img0, lg0, dlg0, df0), (img1, lg1, dlg1, df1) = self.g_half
        s1.wait_stream(s0)
        with torch.cuda.stream(s1):
            self._d_forward(nd_d, h, img1, self.ws_d2, lg1, st1)
        self._d_forward(nd_c, h, img0, self.ws_d, lg0, st0)
        s0.wait_stream(s1)
        self._loss(*self.g_rows, B, 2, st0)  # one mean over the whole batch
        s1.wait_stream(s0)
        with torch.cuda.stream(s1):
            self._d_backward(nd_d, h, self.ws_d2, dlg1, 0, df1, st1)
        self._d_backward(nd_c, h, self.ws_d, dlg0, 0, df0, st0)
        s0.wait_stream(s1)
        self._diversity(st0)
        _lib.call("vg_gen_backward", C.byref(ng), B, _lib.ptr(self.ws_g), _lib.ptr(self.dfake), st0)
        self._adamw(self.r_g, 1, st0, self.clip_g)

    def _inputs(self, real: Optional[torch.Tensor], labels=None, fake_labels=None) -> None:
        """The step's inputs, ONE launch in front of the step proper (and outside its hipGraph, so it reads the caller's tensor
        directly - no staging copy): imgs[:B] = bf16(real), and unless the caller supplies it, the latent batch z ~ N(0, 1)
        (construct_noise(), training.py:35-42 / gan.py:231-232), counter-based on (seed, rank, steps done so far).  With a dataset
        the step fetches its own batch and draws z itself (``_fetch``): only the caller's fake labels are copied here."""
        if self.dataset is not None:
            if fake_labels is not None:
                self.fake_labels.copy_(fake_labels)
            return
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        # the kernel dereferences the caller's pointer with 16-byte loads on THIS engine's device: anything else (another GPU's
        # tensor, an unaligned view) goes through torch's copy, which handles it
        direct = (real.dtype == torch.float32 and real.is_contiguous() and real[0].numel() == self.imgs[0].numel() and real.numel() % 4 == 0
                  and real.device == self.imgs.device and real.data_ptr() % 16 == 0)
        if not direct:
            self.imgs[:self.B].copy_(real)
        want_z = not self.external_noise
        if direct or want_z:
            _lib.call("vg_step_inputs", _lib.ptr(real) if direct else None, _lib.ptr(self.imgs), real.numel() if direct else 0,
                      _lib.ptr(self.z) if want_z else None, self.z.numel() if want_z else 0, self._noise_seed, _lib.ptr(self.step_t), st)
        if self.cond:  # the real labels into their static buffer; the fake ones supplied with z, or drawn like z: one launch, keyed on the counter
            self.real_labels.copy_(labels)
            if fake_labels is not None:
                self.fake_labels.copy_(fake_labels)
            else:
                _lib.call("vg_draw_labels", _lib.ptr(self.fake_labels), self.B, self.n_classes, self._aug_seed, 3, _lib.ptr(self.step_t), st)

    def _fetch(self, st) -> None:
        """The head of a step with a dataset, inside what the hipGraph captures: the real batch (images, labels, indices) from the device
        step counter, then z and the fake labels as ``_inputs`` draws them - the counter is still the one ``_inputs`` would read."""
        ds = self.dataset
        if ds is None:
            return
        _lib.call("vg_dataset_fetch", _lib.ptr(ds.images), _lib.ptr(ds.labels), ds.N, ds.C, ds.IH, ds.layout, _lib.ptr(ds.lut_bf16), _lib.ptr(self.real_dst),
                  _lib.ptr(self.real_labels), _lib.ptr(self.batch_indices), self.B, self.sync.rank, self.world, ds.flags, self.data_seed, _lib.ptr(self.step_t),
                  st)
        if not self.external_noise:
            _lib.call("vg_step_inputs", None, None, 0, _lib.ptr(self.z), self.z.numel(), self._noise_seed, _lib.ptr(self.step_t), st)
            if self.cond:
                _lib.call("vg_draw_labels", _lib.ptr(self.fake_labels), self.B, self.n_classes, self._aug_seed, 3, _lib.ptr(self.step_t), st)

    def _penalty(self, st) -> None:
        """gradient_penalty(D, noisy_real, noisy_fake) joins the D loss (training.py:101-106), on what D's own pass sees."""
        fd = self.vit._flat
        real, fake = self.d_in_half
        if self.gp_c_call:  # one C call
            if self.gp_epsilon is not None:
                torch.add(self.gp_epsilon.reshape(-1).float(), 0.0, out=self.gp_eps)  # (an elementwise kernel, not a D2D copy: no memcpy / memset nodes in the captured step)
            else:
                self.gp_eps.uniform_()  # epsilon = torch.rand(B, 1, 1, 1), utils.py:129
            pnet = _lib.VgVitNet(self.vit._dims, fd.flat.data_ptr(), fd.shadow.data_ptr(), fd.grad.data_ptr(), self.p_d, self.seed * 8 + 3,
                                 self.step_t.data_ptr(), None, 0, 1)
            _lib.call("vg_vit_penalty", C.byref(pnet), self.B, _lib.ptr(real), _lib.ptr(fake), _lib.ptr(self.gp_eps), self.gp_w, _lib.ptr(self.ws_d),
                      _lib.ptr(self.ws_gp), _lib.ptr(self.gp_loss), st)
        else:
            from . import ops2
            from .penalty import gradient_penalty
            fd.attach_grads()
            pen = gradient_penalty(self.vit, real, fake, epsilon=self.gp_epsilon)
            with ops2.deferred_weight_grads(fd.grad):  # the block Linears' weight gradients: grouped per block, straight into the flat buffer
                (self.gp_w * pen).backward()   # the rest accumulates into the same buffer through the parameters' .grad (views of it)
            self.gp_loss.copy_(pen.detach().reshape(1))

    def _r1(self, st) -> None:
        """gamma / 2 E ||grad_x D(x)||^2 on the real images D's own pass sees joins the D loss: one C call, the lazy interval in its weight."""
        fd = self.vit._flat
        pnet = _lib.VgVitNet(self.vit._dims, fd.flat.data_ptr(), fd.shadow.data_ptr(), fd.grad.data_ptr(), self.p_d, self.seed * 8 + 3,
                             self.step_t.data_ptr(), None, 0, 1)
        _lib.call("vg_vit_r1", C.byref(pnet), self.B, _lib.ptr(self.d_in_half[0]), 0.5 * self.r1_gamma * self.r1_interval, _lib.ptr(self.ws_d),
                  _lib.ptr(self.ws_gp), _lib.ptr(self.r1_loss), st)

    def _enqueue_body(self, r1_due: bool = False) -> None:
        """Everything of a step behind its inputs (``_inputs``): what the hipGraph captures.  ``r1_due``: the kind of step - with the
        R1 call (lazy regularisation: step 1 and every ``r1_interval``-th after it) or the plain launch list."""
        if self.two_stream:
            return self._enqueue_two_stream()
        B = self.B
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        (nd, nd_b, nd_c), ng = self._nets()
        fd, fg = self.vit._flat, self.gen._flat
        self._fetch(st)
        # gan.discriminator.zero_grad() (training.py:177) and the device step counter += 1, one launch
        _lib.call("vg_zero_tick", _lib.ptr(fd.grad), fd.total, _lib.ptr(self.step_t), st)
        self._lr_tick(st)
        self._g_forward(ng, st)
        if self.inst_sigma > 0.0:
            self._instance_noise(self.noise_parts[0])
        if self.aug:  # D sees T_1([real ; fake]) (site 0), and so does the penalty below
            self._augment(self.x, self.imgs_aug, self.aug_params["d"], 2 * B, self.aug, 0, st)
        if self.bcr_policy:  # the consistency partner T_c(x) (site 2) behind x in the 4B buffer; the losses and the penalty stay on x
            self._augment(self.d_in, self.imgs_bcr, self.aug_params["c"], 2 * B, self.bcr_policy, 2, st)
        if self.gp_w != 0.0:
            self._penalty(st)
        if r1_due:
            self._r1(st)
        if self.fuse:  # D's own pass, real and fake rows in one batch (with bCR: the pair and its transform, 4B images)
            n, src, adv, dadv = self.d_pass
            self._d_forward(nd, n, src, self.ws_d, self.logits, st)
            # D(real) -> slot 0, D(fake) -> slot 1: both halves of the adversarial rows in one launch
            if self.cond:  # ... on the label-selected logit of each row: the means are over B samples, the other logits get +0
                _lib.call("vg_gan_loss_cond_pair", _lib.ptr(adv), _lib.ptr(self.labels_d), _lib.ptr(dadv), _lib.ptr(self.selected), _lib.ptr(self.losses), B, 0,
                          B, 1, self.Kc, self.kind, 1.0, st)
            else:
                _lib.call("vg_gan_loss_pair", _lib.ptr(adv), _lib.ptr(dadv), _lib.ptr(self.losses), B * self.Kc, 0, B * self.Kc, 1, self.kind, 1.0, st)
            self._ada_update(adv, st)
            self._tel_d_logits(*self.tel_adv, st)
            if self.bcr:
                _lib.call("vg_bcr_loss", *map(_lib.ptr, self.cr_rows), _lib.ptr(self.bcr_losses), B, B, self.Kc, self.bcr_w[0], self.bcr_w[1],
                          int(not self.aug), int(bool(self.aug)), 1.0, st)
            self._d_backward(nd, n, self.ws_d, self.dlogits, 1, None, st)
        else:  # the reference's two passes; the second one finishes D.grad: exchange it as it completes
            for half, net in ((0, nd), (1, nd_b)):
                self._d_forward(net, B, self.d_in_half[half], self.ws_d, self.lg_half[half], st)
                self._loss(self.lg_half[half], self.dlg_half[half], B, half, st)
                if half == 0:
                    self._ada_update(self.lg_half[0], st)
                else:  # both halves' logits are in place behind the second loss launch: one launch for the two
                    self._tel_d_logits(self.lg_half[0], self.lg_half[1], st)
                self._d_backward(net, B, self.ws_d, self.dlg_half[half], 1, None, st, exchange=half == 1)
        self.sync.wait()
        if self.spec is not None:  # dL/dW_eff -> dL/dW on the exchanged total of both passes and the penalty (the map is linear)
            self.spec.project(fd.grad, fd.flat, st)
        self._adamw(self.r_d, 0, st, self.clip_d)
        if self.spec is not None:  # one power iteration on the updated master; AdamW's plain cast of the normalised ranges is overwritten
            self.spec.update(fd.flat, fd.shadow, True, st)
        fg.grad.zero_()            # gan.generator.zero_grad(), training.py:199
        if self.aug:  # D sees T_2(fake) (site 1); its input gradient goes back through the adjoint into dfake
            self._augment(self.fake, self.g_in, self.aug_params["g"], B, self.aug, 1, st)
        lg, dlg = self.g_rows
        self._d_forward(nd_c, B, self.g_in, self.ws_d, lg, st)
        self._loss(lg, dlg, B, 2, st)
        self._tel_g_logits(lg, st)
        self._d_backward(nd_c, B, self.ws_d, dlg, 0, self.g_dimg, st)
        if self.aug:
            self._augment_adjoint(self.g_dimg, self.dfake, B, self.aug, 1, st)
        self._diversity(st)
        self._g_backward(ng, st)
        self.sync.wait()
        if self.shard_map:
            self._adamw_g_sharded(st)
        else:
            self._adamw(self.r_g, 1, st, self.clip_g)
        self._tel_commit(r1_due, st)

    # ------------------------------------------------------------------------------------------ the per-step record
    def history(self) -> dict:
        """The records of the steps since the previous call, oldest first (synchronises once): ``step`` int64 [n]; one float32 [n]
        array per field of ``_lib.TEL_FIELDS`` (the three losses, D's real / fake logit mean and accuracy, the generator pass's logit
        mean and fraction > 0, ``gnorm_{d,g}_{sum,l2}``, ``nonfinite_{d,g}``, ``penalty``, ``bcr_real`` / ``bcr_fake``, ``ada_p`` /
        ``ada_rt``, ``lr_d`` / ``lr_g``, ``diversity`` - NaN where the option is off, and ``penalty`` NaN on a step where lazy R1 was
        not due); ``grad_norms_d`` / ``grad_norms_g`` [n, n_seg] with ``keys_d`` / ``keys_g``, the state_dict keys of the tensors; and
        ``dropped``, the steps that fell out of a ring shorter than the gap between two calls."""
        if not self.tel_cap:
            raise RuntimeError("history(): this engine records nothing (built with telemetry=0)")
        import numpy as np
        torch.cuda.synchronize(self.dev)
        t = int(self.step_t.item())
        steps_dev, ring = self.tel_ring_step.cpu().numpy(), self.tel_ring.cpu().numpy()
        seg_d, seg_g = (r.cpu().numpy() for r in self.tel_ring_seg)
        cap, last = self.tel_cap, min(self._tel_cursor, t)
        want = list(range(max(last + 1, t - cap + 1), t + 1))
        rows = [(s - 1) % cap for s in want]
        stale = [s for s, r in zip(want, rows) if steps_dev[r] != s]
        if stale:
            raise RuntimeError(f"history(): the rings do not hold step(s) {stale[:4]} the counter says were run")
        idx = np.asarray(rows, dtype=np.int64)
        pre = "vit." if self._disc is not self.vit else ""
        out = {"step": np.asarray(want, dtype=np.int64), "dropped": (t - last) - len(want),
               "grad_norms_d": seg_d[idx].copy(), "grad_norms_g": seg_g[idx].copy(),
               "keys_d": [pre + k for k in self.tel_d.keys], "keys_g": list(self.tel_g.keys)}
        for f, name in enumerate(_lib.TEL_FIELDS):
            out[name] = ring[idx, f].astype(np.float32)
        bad = [int(s) for s, a, b in zip(want, out["nonfinite_d"], out["nonfinite_g"]) if a != 0 or b != 0]
        if bad and self.first_nonfinite_step is None:
            self.first_nonfinite_step = bad[0]
        self._tel_cursor = t
        return out

    # ------------------------------------------------------------------------------------------
    def _optional_state(self):
        """THE table of training state an option adds: (key, tensor or None when the option is off, options key, options getter).  It
        drives ``_state_tensors`` (what the graph warm-up must put back), ``state_dict`` and ``load_state_dict``: an option's state is
        one entry here.  (bCR and R1 hold no state, only options; the average is saved without options; the learning-rate schedule's
        state is its two multipliers - the rates themselves are rewritten by every step.)"""
        spec = self.spec is not None
        return (("spectral_state", self.spec.state if spec else None, "spectral_norm", lambda: self.spectral_norm if spec else None),
                (None, None, "bcr", self._bcr_options),
                (None, None, "r1", self._r1_options),
                (None, None, "n_classes", lambda: self.n_classes or None),
                (None, None, "dataset", self._dataset_options),
                ("ada_state", self.ada_state, "ada", self._ada_options),
                ("lr_scale", self.lr_scale, "lr", lambda: self.lr_opts),
                ("ema_g", self.ema_g, None, None))

    def _state_tensors(self):
        """Everything a step changes that the next step reads (the training state held on the device)."""
        fd, fg = self.vit._flat, self.gen._flat
        return ([fd.flat, fd.shadow, fg.flat, fg.shadow, self.m_d, self.v_d, self.m_g, self.v_g, self.step_t]
                + [t for _, t, _, _ in self._optional_state() if t is not None])

    def sync_from_modules(self, reset_optimizer: bool = False) -> None:
        """Call after the modules' parameters were changed behind the engine's back (``load_state_dict``, an in-place
        edit): refreshes the bf16 shadows the GEMMs read; ``reset_optimizer`` also clears AdamW's moments and step count
        (a fresh optimizer, which is what the reference has after a restart: it saves no optimizer state,
        training.py:218-226,262-263).  The generator's moving average needs no code here: a plain refresh leaves it alone, and a
        cleared step counter makes the next step's kernel copy the updated weights into it - the average restarts with the optimizer.
        A learning-rate schedule restarts with the counter as well (its warm-up runs again); the multipliers stay as they are.
        With ``spectral_norm`` a plain refresh keeps the normalisation (the scaled cast from the stored sigma); ``reset_optimizer``
        measures it again: sigma0 = sigma_max of the current weights, so the network is the plain one at that point."""
        if reset_optimizer and self.spec is not None:
            self.spec.measure(self.vit._flat.flat)
        self.vit._flat.refresh_shadow()
        self.gen._flat.refresh_shadow()
        if reset_optimizer:
            for t in (self.m_d, self.v_d, self.m_g, self.v_g, self.step_t):
                t.zero_()
            self._tel_cursor = 0  # the record follows the device counter
            # the latent noise is keyed on the device step counter just cleared: move to a fresh stream, keyed on the steps this
            # engine has really done, so a restarted run does not replay the first run's latent sequence
            self._noise_seed = (self._noise_seed * 0x9E3779B97F4A7C15 + 0xD1B54A32D192ED03 * (self.steps + 1)) & 0xFFFFFFFFFFFFFFFF
            if self.dataset is not None:  # the seed is an argument of a captured node there (``_fetch``): capture again.  The cleared
                self._graphs = {}         # counter also puts the dataset back to position 0 of epoch 0

    # ------------------------------------------------------------------------------------------ averaged generator, sampling
    def _need_ema(self, what: str) -> torch.Tensor:
        return self._need(self.ema_g, f"{what}: this engine keeps no averaged generator (built with ema_decay=0)")

    def sample(self, z: torch.Tensor, labels=None, ema: bool = True) -> torch.Tensor:
        """Images [n, C, IH, IW] (``generator.out_dtype``) of the latent batch ``z`` [n, Z], n any batch size - of the classes ``labels``
        (an integer tensor [n] on the device, required iff the engine is class-conditional; checked on the host): one forward-only
        vg_gen_forward without dropout on the current stream, from the averaged weights (``ema=True``: ``ema_g`` and a bf16 cast of
        it, recast only after a step or a load) or from the live master and shadow (``ema=False``: what ``G.eval()(z)`` computes).
        It has its own workspace - the step's belongs to the captured graph - and changes no training state."""
        gen, fg = self.gen, self.gen._flat
        if isinstance(labels, bool):  # sample(z, False): the flag in its old position
            labels, ema = None, labels
        if ema:
            self._need_ema("sample(ema=True)")
        if z.dim() != 2 or z.shape[1] != gen._dims.Z or z.shape[0] < 1 or z.device != self.dev:
            raise ValueError(f"z must be a [n, {gen._dims.Z}] tensor on {self.dev}")
        n = int(z.shape[0])
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        if ema:
            if self._ema_shadow is None:
                self._ema_shadow = torch.empty(fg.total, dtype=torch.bfloat16, device=self.dev)
            key = (self.steps, self._ema_loads)
            if self._ema_cast_key != key:
                _lib.call("vg_cast_f32_bf16", _lib.ptr(self.ema_g), _lib.ptr(self._ema_shadow), fg.total, st)
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
        y = gen._labels(labels, int(z.shape[0]), self.dev)
        if y is None:
            _lib.call("vg_gen_forward", C.byref(net), n, _lib.ptr(zin), _lib.ptr(self._sample_ws), _lib.ptr(img), st)
        else:
            cond = _lib.VgGenCond(y.data_ptr(), shadow.data_ptr() + 2 * gen._class_off, None, self.n_classes)
            _lib.call("vg_gen_forward_cond", C.byref(net), n, _lib.ptr(zin), _lib.ptr(self._sample_ws), _lib.ptr(img), C.byref(cond), st)
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
        for key, t, okey, options in self._optional_state():
            if okey is not None and options() is not None:  # the options the state was run under, so that a resumed run is the same run
                sd[okey] = options()
            if t is not None:
                sd[key] = t.detach().clone()
        return sd

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
        ``strict``, and so must the saved ``r1`` options (the lazy schedule continues from the restored ``steps``).  The augmentation probability and its controller (``aug_p`` / ``ada_target``) follow bCR's rule for the options, and
        their state is restored whenever both sides hold one.  The learning-rate schedule's options (``"lr"``) are compared under ``strict``
        in the same way; its multipliers are restored whenever both sides hold them, so a resumed run continues its schedule from the
        restored counter at the restored multipliers.  A dataset holds no state of its own - the position in the epoch is a function
        of the counter - but the saved ``dataset`` options (N, B, world, shuffle, flip, data seed) must equal this engine's, strict or
        not: with others the restored counter would point into another epoch."""
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
        if int(sd.get("n_classes") or 0) != self.n_classes:  # (strict or not: the generator's buffers differ in size)
            raise ValueError(f"engine state was saved with n_classes={int(sd.get('n_classes') or 0)}, this engine has n_classes={self.n_classes}")
        saved_ds = None if sd.get("dataset") is None else tuple(sd["dataset"])
        if saved_ds != self._dataset_options():  # (strict or not: the position in the epoch is a function of these and the counter)
            raise ValueError(f"engine state was saved with the dataset (N, B, world, shuffle, flip, data seed) = {saved_ds!r}, this engine has "
                             f"{self._dataset_options()!r}: the restored counter would not continue the same epoch")
        saved_r1 = None if sd.get("r1") is None else tuple(sd["r1"])
        if strict and saved_r1 != self._r1_options():
            raise ValueError(f"engine state was saved with the R1 penalty (r1_gamma, r1_interval) = {saved_r1!r}, this engine has "
                             f"{self._r1_options()!r} (strict=False loads it all the same: R1 holds no training state)")
        saved_lr = None if sd.get("lr") is None else tuple(sd["lr"])
        if strict and saved_lr != self.lr_opts:
            raise ValueError(f"engine state was saved with the learning-rate schedule (kind, warmup, total, final) = {saved_lr!r}, this engine "
                             f"has {self.lr_opts!r} (strict=False loads the multipliers all the same when both sides hold them)")
        has_ema = sd.get("ema_g") is not None
        if strict and has_ema != (self.ema_g is not None):
            raise ValueError("engine state has no ema_g but this engine keeps a moving average (strict=False restarts it)" if not has_ema
                             else "engine state has an ema_g but this engine keeps no moving average")
        # restored: the fixed state, and every optional state that both sides hold; first every size check, then the copies
        pairs = [(getattr(self, k), sd[k], k) for k in names]
        pairs += [(t, sd[k], k) for k, t, _, _ in self._optional_state() if t is not None and sd.get(k) is not None]
        for dst, src, k in pairs:
            if not torch.is_tensor(src) or src.numel() != dst.numel():
                raise ValueError(f"engine state {k}: {tuple(getattr(src, 'shape', ()))} does not fit this engine's {tuple(dst.shape)}")
        with torch.no_grad():
            for dst, src, _ in pairs:
                dst.copy_(src.reshape(dst.shape))
        if self.dataset is not None and int(sd["noise_seed"]) & 0xFFFFFFFFFFFFFFFF != self._noise_seed:
            self._graphs = {}  # the latent stream's seed is an argument of a captured node there (``_fetch``): capture again
        self.steps, self._noise_seed = int(sd["steps"]), int(sd["noise_seed"]) & 0xFFFFFFFFFFFFFFFF
        self._tel_cursor = int(sd["step_t"].reshape(-1)[0])  # the record continues behind the restored counter
        if self.ema_g is not None:
            self._ema_loads += 1
            # no average in the state: the step after the loaded counter copies.  ema_start is an argument of the captured kernel
            # node, so that (rare) case drops the graph; the next step captures it again
            start = self.ema_start if has_ema else max(self.ema_start, int(sd["step_t"].reshape(-1)[0]) + 1)
            if start != self._ema_from:
                self._ema_from, self._graphs = start, {}
        if self.spec is not None and not has_spec:  # no state to restore: the current weights become the reference point
            self.spec.measure(self.vit._flat.flat)
        self.sync_from_modules()

    def step(self, real: Optional[torch.Tensor] = None, z: Optional[torch.Tensor] = None, labels: Optional[torch.Tensor] = None,
             fake_labels: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Run one G/D step on ``real`` [B,C,IH,IW] (cuda).  Returns the device tensor
        [loss_d_real, loss_d_fake, loss_g] of this step without synchronising.  ``z`` [B, Z]: the latent batch, required
        iff the engine was built with ``external_noise=True``.  ``labels`` [B]: the classes of ``real``, an integer cuda tensor,
        required iff the engine is class-conditional; ``fake_labels`` [B]: the classes the generator is asked for, required together
        with ``z`` and drawn on the device otherwise.  The values are not read on the host (no synchronisation): the kernels clamp
        a label into [0, n_classes) before they use it.  An engine built with ``dataset`` fetches ``real`` and ``labels`` itself:
        passing either raises."""
        if self.dataset is not None:
            if real is not None or labels is not None:
                raise ValueError("this engine fetches its real batch from its dataset: call step() without real and labels")
        elif real is None or real.shape[0] != self.B or not real.is_cuda:
            raise ValueError("real must be a cuda tensor with the engine's batch size")
        if (z is not None) != self.external_noise:
            raise ValueError("pass z exactly when the engine was built with external_noise=True")
        if not (self.vit._flat.aliased() and self.gen._flat.aliased()):
            raise RuntimeError("module parameters were re-allocated; rebuild the GanEngine")
        if self.dataset is None and (labels is not None) != self.cond:
            raise ValueError(f"pass labels exactly when the engine is class-conditional (n_classes={self.n_classes})")
        if (fake_labels is not None) != (self.cond and self.external_noise):
            raise ValueError("pass fake_labels exactly when a class-conditional engine was built with external_noise=True")
        for name, t in (("labels", labels), ("fake_labels", fake_labels)):
            if t is not None and (not torch.is_tensor(t) or t.is_floating_point() or t.dtype == torch.bool or tuple(t.shape) != (self.B,) or not t.is_cuda):
                raise ValueError(f"{name} must be an integer cuda tensor of shape [{self.B}]")
        if z is not None:
            self.z.copy_(z)
        self.steps += 1
        due = self.r1 and ops.r1_due(self.steps, self.r1_interval)  # the kind of step: a launch list, and a captured graph, of its own
        if not self._use_graph:
            self._inputs(real, labels, fake_labels)
            self._enqueue_body(due)  # the whole step on the current stream, no host sync
            return self.losses
        if due not in self._graphs:
            # Warm-up on a side stream (allocator, lazily loaded code objects), then capture.  The warm-up is a real step:
            # the training state is saved before it and restored after it, so N calls of step() are N steps in graph
            # mode exactly as in eager mode (tests compare the two bit for bit).
            saved = [t.clone() for t in self._state_tensors()]
            s = torch.cuda.Stream()
            self._inputs(real, labels, fake_labels)
            s.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(s):
                self._enqueue_body(due)
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
                    self._enqueue_body(due)
            except Exception as exc:  # only reachable with collectives or the autograd-driven penalty in the step: otherwise it is all our own enqueue-only calls
                if not self.sync.active and self.gp_w == 0.0:
                    raise
                torch.cuda.synchronize()
                for t, keep in zip(self._state_tensors(), saved):  # a broken capture must not have advanced the state
                    t.copy_(keep)
                self.sync._pending.clear()
                self._graph_fallback(f"capturing the step ({'collectives' if self.sync.active else 'gradient penalty through torch autograd'}) failed: "
                                     f"{type(exc).__name__}: {exc}")
                self._inputs(real, labels, fake_labels)
                self._enqueue_body(due)
                return self.losses
            self._graphs[due] = graph
        self._inputs(real, labels, fake_labels)
        self._graphs[due].replay()
        return self.losses

    # ------------------------------------------------------------------------------------------ the device-resident dataset
    def _need_dataset(self, what: str) -> DeviceDataset:
        if self.dataset is None:
            raise RuntimeError(f"{what}: this engine has no dataset (built without dataset=)")
        return self.dataset

    def run(self, n: int) -> torch.Tensor:
        """``n`` steps of an engine with a dataset, nothing synchronised; returns ``losses`` (the last step's).  Every step is the R1-due
        or the plain launch list as in ``step()``; once a kind is captured its steps are bare replays.  Not with ``external_noise``
        (every step would need the caller's z)."""
        self._need_dataset("run()")
        if self.external_noise:
            raise ValueError("run(): an engine built with external_noise=True takes z with every step; call step(z=...)")
        if isinstance(n, bool) or not isinstance(n, int) or n < 0:
            raise ValueError(f"run(): n must be a non-negative integer, got {n!r}")
        if not (self.vit._flat.aliased() and self.gen._flat.aliased()):
            raise RuntimeError("module parameters were re-allocated; rebuild the GanEngine")
        for _ in range(n):
            due = self.r1 and ops.r1_due(self.steps + 1, self.r1_interval)
            if self._use_graph and due in self._graphs:
                self.steps += 1
                self._graphs[due].replay()
            else:
                self.step()
        return self.losses

    @property
    def steps_per_epoch(self) -> int:
        """Whole global batches per epoch of the dataset."""
        return self._need_dataset("steps_per_epoch").steps_per_epoch(self.B, self._data_world)

    @property
    def epoch(self) -> int:
        """The epoch the NEXT step fetches from, from the device step counter (synchronises: for logging)."""
        return int(self.step_t.item()) // self.steps_per_epoch
