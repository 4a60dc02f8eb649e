"""Shared step of the two DCGAN scripts (MODE 'wgan-CT'): TF/CT_gan_cifar.py:102-154,190-204 and
TF/CT_gan_mnist.py:110-179,232-249.  Loss = WGAN + consistency term (two dropout passes over the
real batch) + LAMBDA * gradient penalty; Adam(1e-4, beta1=.5, beta2=.9), no LR decay.

Exact restructurings: the three live critic calls of the reference (real with masks A, real with masks
B, fake with masks C) are evaluated as ONE batch of 3B rows (dropout is elementwise, the critic has no
batch-coupled op); where the module exposes `DiscriminatorTrunk` / `DiscriminatorTail` (the layer-normalised
ResNet critics, whose first dropout sits after the 16x16 blocks) the deterministic trunk runs once on [real ; fake]
and the two dropout passes over the real batch share it; the WGAN difference, the consistency term and the sum with the
gradient penalty are one fused loss-heads launch each way (rows ordered real, fake, real); the dead 4th call `disc_fake_2` and the extra
generators are not executed.  Without injected draws (`rnd=None`) the dropout masks are regenerated from the
Philox streams inside the kernels.

The scripts' other MODE branches - 'wgan' (weight-clipped WGAN, RMSProp), 'dcgan' (sigmoid cross-entropy, Adam) and 'lsgan' (least
squares, RMSProp) - run on the same trainer from the module's MODES table (GanMode): only D(real) and D(fake) reach their losses (TF
prunes the other critic calls of the graph), evaluated as one batch of 2B rows [real ; fake] whose batch-normalised layers keep one
statistic group per reference call.
"""
from typing import NamedTuple

import torch

from . import functional as F
from . import kernels as K
from . import tflib as lib
from .optim import FlatAdam, FlatRMSProp, LossScaler, SpectralNorm
from .optim import averaged as averaged_weights
from .rng import AUG_FAKE, AUG_GEN, AUG_REAL, DeviceRNG


import os as _os
# A/B switch: the two dropout passes over the real batch share the critic's layers before the first dropout (modules that expose
# DiscriminatorTrunk / DiscriminatorTail: the layer-normalised ResNet critics, whose dropouts sit after the 16x16 blocks)
TRUNK_SHARE = _os.environ.get('CTGAN_UNCOND_TRUNK_SHARE', '1') != '0'


# The fake batches of an iteration's critic steps from one generator forward (A/B switch; the ResNet trainer's BATCH_FAKES)
BATCH_FAKES = _os.environ.get('CTGAN_DCGAN_BATCH_FAKES', '1') != '0'


class GanMode(NamedTuple):
    """One MODE branch of a script: its objective, optimizer and loop literals (TF/CT_gan_mnist.py:122-206,238-249;
    TF/CT_gan_64x64.py:490-579,634-646)."""
    loss: str                    # 'ct' (WGAN + consistency term + gradient penalty), 'wgan', 'bce' (MODE 'dcgan'), 'ls' (MODE 'lsgan');
                                 # 'hinge' (DCGANTrainer(objective='hinge'): in no MODES table, the scripts have no such branch)
    optimizer: str               # 'adam' | 'rmsprop' (the same for critic and generator)
    lr: float = None             # None: the module's CT learning rate (cfg.LR, or its lr(iteration))
    betas: tuple = None          # Adam (beta1, beta2); None: the module's ADAM_BETAS
    clip: float = None           # critic weights clipped to [-clip, clip] after every critic update
    critic_iters: int = None     # critic steps per iteration; None: cfg.CRITIC_ITERS


CT_MODE = GanMode('ct', 'adam')
HINGE_MODE = GanMode('hinge', 'adam')       # objective='hinge': the CT default's learning rate, ADAM_BETAS and cfg.CRITIC_ITERS


def validate_mode(module_name, modes, mode):
    """Config(MODE=...) of the modules with a MODES table: a value no branch of the script codes raises."""
    if mode not in modes:
        raise NotImplementedError('%s: MODE %r is not supported (supported: %s)' % (module_name, mode, ', '.join(sorted(modes))))


def image_shape_of(module):
    """(channels, height, width) of the flat NCHW images `module` trains on: SCHEDULED_CRITIC of the two DCGAN scripts, image_shape() of
    the others."""
    spec = getattr(module, 'SCHEDULED_CRITIC', None)
    if spec is not None:
        return (spec['channels'], spec['size'], spec['size'])
    return tuple(module.image_shape())


def mode_of(module):
    modes = getattr(module, 'MODES', None)
    if modes is None:                # the ResNet / LSUN scripts have no MODE switch: their CT objective
        return CT_MODE
    validate_mode(module.__name__, modes, module.cfg.MODE)
    return modes[module.cfg.MODE]


class DCGANTrainer:
    def __init__(self, module, seed=2024, rank=0, world_size=1, allreduce=None, g_average=0.0, augment=None, loss_scale=None,
                 spectral_norm=False, objective=None):
        """`module` = ctgan_amd.gan_cifar or ctgan_amd.gan_mnist (provides cfg, Generator, Discriminator,
        real_prep, feat_shapes).  g_average > 0 (NOT in the reference): keep an exponential moving average of the GENERATOR's weights,
        moved inside its update launch (optim.FlatAdam / FlatRMSProp avg_rate), whatever the mode's optimizer.  It is the RATE, 1 - decay:
        g_average=1e-4 is a decay of 0.9999.  `averaged()` samples from it; the critic is never averaged.  0 (default): nothing differs
        from a trainer built without the argument.  augment (NOT in the reference): a Differentiable Augmentation policy (Zhao et al.
        2020), a comma-separated subset of 'color,translation,cutout'; None / '': off, nothing differs.  The random transformation T
        (kernels.diffaug) is applied to the reals and the fakes in front of the critic in the critic step - before the interpolation, so
        the penalty is taken at the augmented x_hat - and to the samples in the generator step, whose gradient flows back through T.  Its
        draws come from three reserved streams (rng.AUG_REAL / AUG_FAKE / AUG_GEN) at the trainer's own counter: no other draw of a step
        moves, there is no state to checkpoint.  loss_scale (NOT in the reference; for kernels.set_mma_dtype('f16')): None - the
        module's LOSS_SCALE, or 1, as before; a float - that fixed power-of-two scale; 'dynamic' or an optim.LossScaler - a dynamic scale
        kept on the device (`scaler`; both optimizers share it): the backward is seeded with it, an update whose gradients hold a NaN /
        inf is dropped as a whole and halves it, growth_interval applied updates in a row double it.  spectral_norm (NOT in
        the reference; Miyato et al. 2018): the critic reads every conv filter and Linear weight divided by its spectral norm,
        one power iteration per critic update (optim.SpectralNorm: `spectral`); the registry, the optimizer and the checkpoints keep the
        raw weights, `d_params` and a step's out['grads'] are the normalised weights and the gradients with respect to them (the raw
        weights' are in d_opt.grad).  ValueError under MODE 'wgan', whose weight clip answers the same question.  False: nothing differs.
        objective (NOT in the reference; Lim & Ye 2017, Miyato et al. 2018): None - the module's MODE; 'hinge' - the critic
        minimises mean max(0, 1 - D(x)) + mean max(0, 1 + D(G(z))), the generator -mean D(G(z)): `mode` becomes GanMode('hinge', 'adam'),
        i.e. the module's CT learning rate, its ADAM_BETAS and cfg.CRITIC_ITERS, one dropout pass over [real ; fake], no penalty.  Valid
        only while the module's MODE is its CT default (the unnormalised critic with dropout and one statistic group): ValueError under
        'wgan', 'dcgan' or 'lsgan', and for any other value.  The step runs on the autograd path (no hand schedule for this family).
        None (default): nothing differs."""
        if objective not in (None, 'hinge'):
            raise ValueError("objective: None or 'hinge' (got %r)" % (objective,))
        self.objective = objective
        self.mod = module
        self.aug_policy = K.diffaug_policy(augment)
        self.aug_shape = image_shape_of(module) if self.aug_policy else None
        self.dev = lib._dev()
        self.rank, self.world, self.allreduce = rank, world_size, allreduce
        self.rng = DeviceRNG(seed, rank, self.dev)
        self.d_named = lib.named_params_with_name('Discriminator', trainable_only=True)
        self.g_named = lib.named_params_with_name('Generator', trainable_only=True)
        self.mode = mode_of(module)
        if objective == 'hinge':
            if self.mode.loss != 'ct':
                raise ValueError("objective='hinge' replaces the CT objective only: not under MODE %r" % (module.cfg.MODE,))
            self.mode = HINGE_MODE
        self.disc_iters = self.mode.critic_iters or module.cfg.CRITIC_ITERS     # critic steps per iteration
        if spectral_norm and self.mode.clip:
            raise ValueError('spectral_norm: not with the weight clip of MODE %r (two answers to one question: use one)' % (module.cfg.MODE,))
        # Power-of-two loss scale for the fp16 matrix-core mode (kernels.set_mma_dtype('f16')): the backward passes are linear in the
        # seed, so the cost gradient is seeded with S instead of 1 - every first-order gradient TENSOR the fp16 kernels round is S
        # times larger, away from fp16's subnormals (per-pixel gradients shrink with 1 / (B H W)) - and Adam divides it out again
        # (grad_scale); exact in fp32 (a power of two), a no-op for S = 1.  Dynamic: S lives in `scaler.state`, the static factor stays 1.
        if isinstance(loss_scale, str) and loss_scale != 'dynamic':
            raise ValueError("loss_scale: None, a number, 'dynamic' or an optim.LossScaler (got %r)" % (loss_scale,))
        self.scaler = LossScaler(device=self.dev) if isinstance(loss_scale, str) else loss_scale if isinstance(loss_scale, LossScaler) else None
        if self.scaler is not None and self.scaler.state.device.type != torch.device(self.dev).type:
            raise ValueError('loss_scale: the LossScaler lives on %s, the trainer on %s' % (self.scaler.state.device, self.dev))
        kw = {'scaler': self.scaler} if self.scaler is not None else {}
        if self.mode.optimizer == 'rmsprop':
            self.d_opt = FlatRMSProp(self.d_named, clip=self.mode.clip, **kw)
            self.g_opt = FlatRMSProp(self.g_named, avg_rate=g_average, **kw)
        else:
            b1, b2 = self.mode.betas or getattr(module, 'ADAM_BETAS', (0.5, 0.9))
            self.d_opt = FlatAdam(self.d_named, b1, b2, **kw)
            self.g_opt = FlatAdam(self.g_named, b1, b2, avg_rate=g_average, **kw)
        # the clip op also covers the critic's non-trainable BatchNorm moving statistics; nothing else writes them (training-mode
        # statistics only), so clamping them once, at the first critic update, is exact
        self._stats_to_clip = [p for n, p in lib.named_params_with_name('Discriminator') if n in lib._non_trainable] if self.mode.clip else []
        self.towers = getattr(module, 'GEN_TOWERS', 1)                    # generator calls per batch, each with its own BN statistics
        self.piecewise = getattr(module, 'PIECEWISE_LINEAR_CRITIC', True)
        self.iteration = 0
        self.d_params = [p for _, p in self.d_named]
        self.g_params = [p for _, p in self.g_named]
        self.spectral = None
        if spectral_norm:
            self.spectral = SpectralNorm(self.d_named, self.d_opt)
            self.spectral.install()            # (until detach_spectral() or lib.delete_all_params(): the registry reads theta_bar)
            self.d_params = [v for _, v in self.spectral.views()]
        if self.scaler is not None:
            self._loss_scale = 1.0
        else:
            self._loss_scale = float(getattr(module, 'LOSS_SCALE', 1.0) if loss_scale is None else loss_scale)
        self._seed = None

    @property
    def loss_scale(self):
        """The STATIC loss scale, the factor the host folds into grad_scale: the fixed scale, or 1.0 under a dynamic one (whose value is
        on the device: scaler.scale())."""
        return self._loss_scale

    @loss_scale.setter
    def loss_scale(self, value):
        if self.scaler is not None:
            raise AttributeError('loss_scale cannot be assigned on a trainer with a dynamic loss scale (it lives in trainer.scaler)')
        self._loss_scale = float(value)

    def detach_spectral(self):
        """Give the registry back (a trainer built with spectral_norm=True owns its alias table until this or lib.delete_all_params()):
        the critic reads the raw weights again, d_params are the raw parameters, d_opt steps without the normalisation.  Not under graph
        replay: captured graphs keep reading the normalised copy."""
        if self.spectral is not None:
            self.spectral.remove()
            self.spectral = None
            self.d_params = [p for _, p in self.d_named]

    def averaged(self):
        """Context manager: inside it the generator's parameters hold their weight average (optim.averaged; ValueError when the
        trainer was built with g_average = 0).  Sample and score inside; do not train inside."""
        return averaged_weights(self.g_opt)

    def cost_seed(self):
        """grad_outputs of the final backward: a cached 0-dim tensor holding the loss scale (no fill kernel per step); under a dynamic
        scale the device view of it (LossScaler.seed)."""
        if self.scaler is not None:
            return self.scaler.seed()
        if self._seed is None or float(self._seed_val) != self.loss_scale:
            self._seed = torch.full((), self.loss_scale, dtype=torch.float32, device=self.dev)
            self._seed_val = self.loss_scale
        return self._seed

    def lr(self):
        """The learning rate of this iteration's updates: the mode's literal, or the module's CT rate."""
        if self.mode.lr is not None:
            return self.mode.lr
        return self.mod.lr(self.iteration) if hasattr(self.mod, 'lr') else self.mod.cfg.LR

    def clip_stats(self):
        """The clip op on the critic's moving statistics (see __init__): run once, after the first critic update."""
        if self._stats_to_clip:
            with torch.no_grad():
                for p in self._stats_to_clip:
                    p.clamp_(-self.mode.clip, self.mode.clip)
            self._stats_to_clip = []

    def aug_real(self, real_in):
        """The critic step's reals: real_prep, then T on the stream AUG_REAL when augmenting (integer pixels: both in one launch)."""
        m = self.mod
        if not self.aug_policy:
            return m.real_prep(real_in)
        spec = self.rng.aug_spec(AUG_REAL)
        denom = getattr(m, 'REAL_DENOM', None)
        if denom is not None and real_in.dtype == torch.int32 and real_in.is_contiguous():
            return K.diffaug(real_in, self.aug_shape, self.aug_policy, spec, denom=denom)       # bit-equal to the two launches below
        return K.diffaug(m.real_prep(real_in).contiguous(), self.aug_shape, self.aug_policy, spec)

    def aug_fake(self, fake):
        """The critic step's (detached) fakes under T on the stream AUG_FAKE when augmenting."""
        if not self.aug_policy:
            return fake
        return K.diffaug(fake.contiguous(), self.aug_shape, self.aug_policy, self.rng.aug_spec(AUG_FAKE))

    def _critic(self, x, u, groups):
        """The critic on rows made of `groups` reference calls (each its own BatchNorm statistics) - the non-CT objectives."""
        m = self.mod
        if self.mode.loss == 'hinge':       # the CT default's critic: no batch norm, one statistic group (gan_cifar's takes no `groups`)
            return m.Discriminator(x, u=u) if u is not None else m.Discriminator(x, rng=self.rng)
        return m.Discriminator(x, u=u, groups=groups) if u is not None else m.Discriminator(x, rng=self.rng, groups=groups)

    def _d_losses_plain(self, real_in, rnd, fake):
        """Critic cost of the 'wgan' / 'dcgan' / 'lsgan' objectives (and of objective='hinge') over D(real) (masks u_real) and D(fake) (masks
        u_fake) - one batch of 2B rows, two statistic groups per generator tower."""
        m, B = self.mod, self.mod.cfg.BATCH_SIZE
        with torch.no_grad():
            if fake is None:
                fake = self._gen(B, rnd['z'] if rnd is not None else None)
            real = self.aug_real(real_in)
            fake_in = self.aug_fake(fake)
        u = [torch.cat([a, c], 0) for a, c in zip(rnd['u_real'], rnd['u_fake'])] if rnd is not None else None
        d, _ = self._critic(torch.cat([real, fake_in], 0), u, 2 * self.towers)
        if self.mode.loss == 'wgan':
            cost = F.mean_diff(d, B, B, -1.0, 1.0)             # mean(D(fake)) - mean(D(real))
        else:
            cost = F.gan_loss(d, B, self.mode.loss, 'd')
        return {'cost': cost, 'fake': fake, 'd_real': d[:B].detach(), 'd_fake': d[B:].detach()}

    def d_losses(self, real_in, rnd=None, fake=None):
        if self.mode.loss != 'ct':
            return self._d_losses_plain(real_in, rnd, fake)
        m, cfg = self.mod, self.mod.cfg
        B = cfg.BATCH_SIZE
        with torch.no_grad():
            if fake is None:        # `fake`: a batch drawn earlier from the same generator weights (generate_fakes)
                fake = self._gen(B, rnd['z'] if rnd is not None else None)
            real = self.aug_real(real_in)
            fake_in = self.aug_fake(fake)       # (the samples themselves stay in out['fake'])
            alpha = rnd['alpha'] if rnd is not None else self.rng.uniform(B, 1)
            interp = K.interpolate(real, fake_in, alpha)
        # rows of the batched passes: real (masks A), fake (masks C), real (masks B) - the order the fused loss heads read
        u = [torch.cat([a, c, b], 0) for a, b, c in zip(rnd['u_real'], rnd['u_real_'], rnd['u_fake'])] if rnd is not None else None
        if TRUNK_SHARE and hasattr(m, 'DiscriminatorTrunk') and getattr(m, 'critic_is_per_sample', lambda: True)():
            # the critic's layers before its first dropout are deterministic and per-sample: the two dropout passes over the real
            # batch share ONE evaluation of them - rows [real ; fake] through the trunk, rows [real, fake, real] through the tail
            h = m.DiscriminatorTrunk(torch.cat([real, fake_in], 0))
            h3 = F.rows_select(h, [(0, B), (B, 2 * B), (0, B)])
            d, f = m.DiscriminatorTail(h3, u=u, rng=None if rnd is not None else self.rng)
        else:
            x3 = torch.cat([real, fake_in, real], 0)
            # masks regenerated from the Philox stream inside the dropout kernels when none are injected: no uniform tensors
            d, f = m.Discriminator(x3, u=u) if rnd is not None else m.Discriminator(x3, rng=self.rng)
        interp.requires_grad_(True)
        with F.weight_grads(not self.piecewise):     # a LeakyReLU + dropout critic is piecewise linear; a layer-normalised one is not
            d_gp = (m.Discriminator(interp, u=rnd['u_gp']) if rnd is not None else m.Discriminator(interp, rng=self.rng))[0]
        (grads,) = torch.autograd.grad(d_gp, interp, grad_outputs=torch.ones_like(d_gp), create_graph=True)
        gp, slopes = F.gradient_penalty(grads, cfg.LAMBDA)
        # mean(fake) - mean(real), the consistency term over the two real passes and the sum with gp: one launch each way
        cost, wgan, ct, _, _ = F.critic_heads(d, f, None, None, B, cfg.LAMBDA_2, cfg.Factor_M, 0.0, gp)
        return {'cost': cost, 'wgan_only': wgan, 'ct': ct, 'gp': gp, 'fake': fake, 'slopes': slopes, 'gp_grads': grads}

    def d_grads(self, real_in, rnd=None, fake=None):
        """Losses and parameter gradients of one critic step -> (out, grads aligned with self.d_params; scaled by the loss scale).  The
        DCGAN scripts' piecewise-linear critic runs the hand-scheduled step (dcgan_schedule.py: one forward and one backward chain over
        [real, fake, real | x_hat], the penalty's double backward on its own rows); everything else - injected draws, the layer-normalised
        ResNet critics - the autograd form."""
        from . import dcgan_schedule as DS
        if fake is None and rnd is None:
            with torch.no_grad():
                fake = self._gen(self.mod.cfg.BATCH_SIZE, None)
        if DS.usable(self, rnd, fake, real_in):
            with torch.no_grad(), F.deferred_wgrads():
                if not self.aug_policy:
                    return DS.critic_step(self, real_in, fake)
                out, grads = DS.critic_step(self, real_in, self.aug_fake(fake), real=self.aug_real(real_in))
                out['fake'] = fake
                return out, grads
        out = self.d_losses(real_in, rnd, fake=fake)
        with F.deferred_wgrads():       # the queued weight gradients of the step: one grouped launch (functional._flush_groups)
            grads = torch.autograd.grad(out['cost'], self.d_params, grad_outputs=self.cost_seed().reshape(out['cost'].shape), allow_unused=True)
        return out, grads

    def _gen(self, n, z, groups=1):
        g = self.towers * groups
        if g > 1:
            return self.mod.Generator(n, noise=z, rng=self.rng, groups=g)
        return self.mod.Generator(n, noise=z, rng=self.rng)

    def generate_fakes(self, n_steps):
        """The fake batches of the next `n_steps` critic steps in ONE generator forward: the generator does not change between the critic
        updates of an iteration (TF/CT_gan_cifar.py:190-204), each step's batch keeps its own BatchNorm statistic group(s).  A step of its
        own in the Philox numbering (as gan_cifar_resnet.Trainer.generate_fakes)."""
        B = self.mod.cfg.BATCH_SIZE
        self.rng.begin_step()
        with torch.no_grad():
            fake = self._gen(n_steps * B, None, groups=n_steps)
        self.rng.end_step()
        return fake.reshape(n_steps, B, -1)

    def g_losses(self, rnd=None):
        m, B = self.mod, self.mod.cfg.BATCH_SIZE
        x = self._gen(B, rnd['z'] if rnd is not None else None)
        # the critic sees T(x) on the stream AUG_GEN when augmenting; the generator's gradient flows back through T (its adjoint launch)
        xa = F.diffaug(x, self.aug_shape, self.aug_policy, self.rng.aug_spec(AUG_GEN)) if self.aug_policy else x
        with F.weight_grads(False):
            u = rnd['u_fake'] if rnd is not None else None
            if self.mode.loss == 'ct':
                d, _ = m.Discriminator(xa, u=u) if rnd is not None else m.Discriminator(xa, rng=self.rng)
            else:
                d, _ = self._critic(xa, u, self.towers)
        if self.mode.loss in ('ct', 'wgan'):
            cost = F.mean_diff(d, B, 0, -1.0, 0.0)                # -mean(D(fake))
        else:
            cost = F.gan_loss(d, B, self.mode.loss, 'g')
        return {'cost': cost, 'samples': x}

    def _apply(self, opt, grads):
        opt.set_lr(self.lr())
        scale = 1.0 / (self.world * self.loss_scale)
        if self.allreduce is None or self.world <= 1:
            opt.update(grads, scale, rng=self.rng)          # bucket + Adam: one launch; end of the step (beta powers, Philox counter): one launch
            return
        flat = opt.gather_grads(grads)
        self.allreduce(flat)
        if hasattr(self.allreduce, 'wait'):
            self.allreduce.wait()
        opt.step(grad_scale=scale, rng=self.rng)

    def _unscaled(self, grads, seed=None):
        """`seed`: under a dynamic scale, a COPY of the scale the gradients were taken at (the end of the step may have changed it)."""
        if seed is not None:
            return [None if g is None else g / seed for g in grads]
        if self.loss_scale == 1.0:
            return grads
        return [None if g is None else g / self.loss_scale for g in grads]

    def d_step(self, real_in, rnd=None, fake=None):
        self.rng.begin_step()
        out, grads = self.d_grads(real_in, rnd, fake=fake)
        seed = self.scaler.seed().clone() if self.scaler is not None else None
        self._apply(self.d_opt, grads)          # (the weight clip of MODE 'wgan' is fused into the update, on every rank)
        self.clip_stats()
        out['grads'] = dict(zip([n for n, _ in self.d_named], self._unscaled(grads, seed)))
        return out

    def g_step(self, rnd=None):
        self.rng.begin_step()
        out = self.g_losses(rnd)
        with F.deferred_wgrads():
            grads = torch.autograd.grad(out['cost'], self.g_params, grad_outputs=self.cost_seed().reshape(out['cost'].shape), allow_unused=True)
        seed = self.scaler.seed().clone() if self.scaler is not None else None
        self._apply(self.g_opt, grads)
        out['grads'] = dict(zip([n for n, _ in self.g_named], self._unscaled(grads, seed)))
        return out

    def train_iteration(self, iteration, next_batch):
        self.iteration = iteration
        if iteration > 0:
            self.g_step()
        out = None
        n = self.disc_iters
        fakes = self.generate_fakes(n) if BATCH_FAKES else None
        for i in range(n):
            out = self.d_step(next_batch(), fake=None if fakes is None else fakes[i])
        return out


def build_params(module, device=None):
    """Instantiate every parameter of `module` once (the reference does this while building its graph)."""
    if hasattr(module, 'build_params'):
        module.build_params(device)
        return
    if device is not None:
        lib.set_device(device)
    dev = lib._dev()
    with torch.no_grad():
        x = module.Generator(2, noise=torch.zeros(2, 128, device=dev))
        module.Discriminator(x, u=[torch.full((2,) + tuple(s), 0.9, device=dev) for s in module.feat_shapes()])


def sample_grid(module, noise, trainer=None, averaged=False):
    """generate_image of the scripts (TF/CT_gan_cifar.py:162-165, TF/CT_gan_mnist.py:211-216, TF/CT_gan_64x64.py:588-592): the fixed-noise
    samples as the array tflib.save_images takes - [n, 28, 28] floats in [0, 1] (MNIST) or [n, 3, H, W] integer pixels.  averaged (with the
    `trainer` that keeps it): from the generator's weight average (DCGANTrainer.averaged)."""
    import contextlib
    import math
    if averaged and trainer is None:
        raise ValueError('sample_grid: averaged=True needs the trainer that keeps the average')
    with trainer.averaged() if averaged else contextlib.nullcontext():
        F.prepare_filters()
        with torch.no_grad():
            s = module.Generator(noise.shape[0], noise=noise)
    n, d = s.shape
    if d % 3:
        side = int(round(math.sqrt(d)))
        return s.reshape(n, side, side).cpu().numpy()
    from .evaluate import SCORE_SCALE
    side = int(round(math.sqrt(d // 3)))
    scale = SCORE_SCALE.get(module.__name__.rsplit('.', 1)[-1], 255.99 / 2)
    return ((s + 1.) * scale).to(torch.int32).reshape(n, 3, side, side).cpu().numpy()


def train(module, next_batch, dev_batches=None, iters=None, out_dir='.', seed=2024, use_graphs=True, sample_every=100, dev_every=100,
          checkpoint_every=1000, score_every=None, classifier=None, resume=None, log=print, g_average=0.0, augment=None, loss_scale=None,
          spectral_norm=False, objective=None):
    """The loop body the DCGAN-family scripts share (TF/CT_gan_cifar.py:190-236, TF/CT_gan_mnist.py:232-270, TF/CT_gan_64x64.py:628-669):
    `next_batch()` -> one real batch on the device; `dev_batches()` -> an iterable over the held-out batches (None: no dev pass).  Series
    (train_log.Series, log.jsonl in `out_dir`): `train disc cost` and `time` per iteration; every `dev_every` iterations `dev disc cost`
    (+ `slope_real` for gan_cifar); with a `classifier`, every `score_every` iterations the script's score series (and `frechet`
    when it is a score_cifar.ClassifierScore with a reference, `precision` / `recall` / `nn_dist` when it has a manifold); the fixed-noise sample grid every `sample_every`; checkpoints every `checkpoint_every`.  Flushed as the scripts do: the first five iterations and every
    `dev_every`-th.  `g_average` > 0 (NOT in the reference; DCGANTrainer): the generator's weight average is kept, scored after the live
    generator under the same series names + `_avg`, and sampled into `samples_%d_avg.png`.  `augment` (NOT in the reference; DCGANTrainer):
    a Differentiable Augmentation policy such as 'color,translation,cutout' for the critic's inputs in both steps; the dev cost, the sample
    grids and the scores stay un-augmented.  `loss_scale` (NOT in the reference; DCGANTrainer): None, a fixed scale, or 'dynamic' / an
    optim.LossScaler - then the series `loss_scale` and `skipped_steps` are added at every flush.  `spectral_norm` (NOT in the reference;
    DCGANTrainer): the critic's weights are spectrally normalised - then the series `sn_sigma_max` and `sn_sigma_min` are added at every
    flush.  `objective` (NOT in the reference; DCGANTrainer): None or 'hinge' - the hinge critic and generator costs in place of the CT
    objective; the series keep their names.  Returns the trainer."""
    import os
    import time

    from . import checkpoint, evaluate
    from .engine import GraphedDCGANTrainer
    from .tflib import save_images
    from .train_log import Series
    cfg = module.cfg
    iters = cfg.ITERS if iters is None else iters
    build_params(module)
    trainer = DCGANTrainer(module, seed=seed, g_average=g_average, augment=augment, loss_scale=loss_scale, spectral_norm=spectral_norm,
                           objective=objective)
    start = checkpoint.load(resume, trainer) if resume else 0
    first = next_batch()
    eng = GraphedDCGANTrainer(trainer, tuple(first.shape), first.dtype, use_graphs=use_graphs)
    pending = [first]
    feed = lambda: pending.pop() if pending else next_batch()          # noqa: E731
    ev = evaluate.Evaluator(trainer)
    n_fixed = {'gan_cifar': 128, 'gan_mnist': 128, 'gan_lsun128': 64}.get(ev.name, cfg.BATCH_SIZE)
    fixed_noise = torch.randn(n_fixed, 128, generator=torch.Generator().manual_seed(seed)).to(trainer.dev)
    series = Series(os.path.join(out_dir, 'log.jsonl'), echo=log)
    series.iteration = start
    for iteration in range(start, iters):
        t0 = time.time()
        out = eng.train_iteration(iteration, feed)
        series.add('train disc cost', out['cost'].item())
        series.add('time', time.time() - t0)
        if classifier is not None and score_every and iteration % score_every == score_every - 1:
            evaluate.record_score(ev, series, classifier)
            if g_average:
                evaluate.record_score(ev, series, classifier, averaged=True)
        if dev_batches is not None and dev_every and iteration % dev_every == dev_every - 1:
            dev = ev.dev_cost(dev_batches())
            if 'slope_real' in dev:
                series.add('slope_real', dev['slope_real'])
            series.add('dev disc cost', dev['dev_cost'])
        if sample_every and iteration % sample_every == sample_every - 1:
            save_images.save_images(sample_grid(module, fixed_noise), os.path.join(out_dir, 'samples_%d.png' % iteration))
            if g_average:
                save_images.save_images(sample_grid(module, fixed_noise, trainer, averaged=True),
                                        os.path.join(out_dir, 'samples_%d_avg.png' % iteration))
        if checkpoint_every and iteration % checkpoint_every == checkpoint_every - 1:
            checkpoint.save(os.path.join(out_dir, 'checkpoint.pt'), trainer, iteration + 1)
        if iteration < 5 or (dev_every and iteration % dev_every == dev_every - 1):
            if trainer.scaler is not None:
                series.add('loss_scale', trainer.scaler.scale())
                series.add('skipped_steps', trainer.scaler.skipped_steps())
            if trainer.spectral is not None:
                sig = trainer.spectral.sigmas().values()
                series.add('sn_sigma_max', max(sig))
                series.add('sn_sigma_min', min(sig))
            series.flush()
        series.tick()
    return trainer
