"""Evaluation between training iterations: the held-out critic cost and the score samples of the scripts' loops
(TF/CT_gan_cifar_resnet.py:350-360,414-427; TF/CT_gan_cifar.py:167-176,210-229; TF/CT_gan_mnist.py:254-263; TF/CT_gan_64x64.py:600-608,
652-663).

`Evaluator.dev_cost` averages the script's `disc_cost` over the dev batches without updating anything: `session.run(disc_cost)` draws a
fresh fake batch, fresh dropout masks and a fresh x_hat per dev batch and touches no optimizer.  Exact restructurings:

  * an evaluation pass is not bound to the training batch.  The CT critics are per-sample and the generators' (and the other modes'
    critics') BatchNorms take `groups`, so `width` = G dev batches share ONE pass of G*B rows, laid out as the loss heads read them - real
    (masks A) of all G batches, the fakes of all G, real (masks B) of all G; x_hat beside them - with `groups` multiplied by G.  All
    batches have B rows, so the heads' mean over G*B rows IS the mean of the G batch costs.  G = 1 is the same code;
  * nothing of a training step that an evaluation does not need runs: the dropout passes are no_grad, weight gradients are off
    (F.weight_grads(False)), and the penalty's dD/dx_hat is one first-order data gradient (no double-backward graph);
  * the running sum stays on the device, weighted by each pass's batch count; the host synchronises once per call.

Evaluation draws from a Philox stream of its own (`eval_stream`): the trainer's seed plus EVAL_SEED_OFFSET, with its own device step
counter, advanced by one per pass.  The training stream is never read, so a run with evaluation interleaved is bit-identical in weights
and optimizer state to one without."""
import math

import numpy as np
import torch

from . import functional as F
from . import kernels as K
from . import tflib as lib
from .rng import DeviceRNG

# seed of the evaluation stream = (training seed + EVAL_SEED_OFFSET) mod 2^64 (the golden-ratio increment: far from every small seed)
EVAL_SEED_OFFSET = 0x9E3779B97F4A7C15

# Dev batches per pass (`width=None`), by module.  The 32x32 / 28x28 modules: the smallest measured width (1, 2, 4, 8) whose time lies within
# the spread of the best - 8 for all three; a pass then holds 4 G B = 2048 critic rows (real, fake, real, x_hat) of 32x32.
# gan_64x64 / gan_lsun128: bounded by the rows in flight, not measured - 4 B = 256 critic rows of 64x64 / 128x128 per pass at G = 1, the
# penalty pass's activations kept for its backward.
DEFAULT_WIDTH = {'gan_cifar_resnet': 8, 'gan_cifar': 8, 'gan_mnist': 8, 'gan_64x64': 1, 'gan_lsun128': 1}
# Score samples per generator call (statistic groups of 100 each): rows in flight of one call
DEFAULT_SCORE_CHUNK = {'gan_cifar_resnet': 1000, 'gan_cifar': 1000, 'gan_64x64': 200}
# (samples + 1) * scale -> integer pixels: 255.99 / 2 (TF/CT_gan_cifar_resnet.py:356, TF/CT_gan_64x64.py:604); TF/CT_gan_cifar.py:174 has 255 / 2
SCORE_SCALE = {'gan_cifar_resnet': 255.99 / 2, 'gan_cifar': 255. / 2, 'gan_64x64': 255.99 / 2}
# score samples per evaluation and the series they are logged under (:414-418; TF/CT_gan_64x64.py:652-655; TF/CT_gan_cifar.py:171,210-212)
SCORE_SAMPLES = {'gan_cifar_resnet': 50000, 'gan_cifar': 1000, 'gan_64x64': 50000}
SCORE_SERIES = {'gan_cifar_resnet': ('inception_50k', 'inception_50k_std'), 'gan_cifar': ('inception score',),
                'gan_64x64': ('inception_50k', 'inception_50k_std')}
SCORE_GROUP = 100          # samples_100 = Generator(100, ...): one BatchNorm statistic group per 100 samples


def eval_stream(trainer):
    """The evaluation stream of `trainer` (created on first use; checkpoint.py saves and restores its counter through here)."""
    rng = getattr(trainer, 'eval_rng', None)
    if rng is None or rng.seed != ((trainer.rng.seed + EVAL_SEED_OFFSET) & (2 ** 64 - 1)):
        ctr = None if rng is None else rng.ctr
        rng = DeviceRNG((trainer.rng.seed + EVAL_SEED_OFFSET) & (2 ** 64 - 1), trainer.rng.rank, trainer.dev)
        if ctr is not None:          # (the seed was replaced by a checkpoint load: the position stays)
            rng.ctr.copy_(ctr)
        trainer.eval_rng = rng
    return rng


def _short_name(module):
    return module.__name__.rsplit('.', 1)[-1]


def _cat(ts):
    return ts[0] if len(ts) == 1 else torch.cat(ts, 0)


def _cat_masks(rnds, key, rows=None):
    """Per dropout site: the uniforms `key` of every batch, one after the other (rows: a slice of each batch's tensor)."""
    n_sites = len(rnds[0][key])
    return [_cat([r[key][i] if rows is None else r[key][i][rows] for r in rnds]) for i in range(n_sites)]


class Evaluator:
    def __init__(self, trainer, width=None):
        """`trainer`: a gan_cifar_resnet.Trainer or a dcgan_step.DCGANTrainer (every module, every GanMode).  `width`: dev batches per
        pass (None: DEFAULT_WIDTH of the module)."""
        self.t = trainer
        self.resnet = not hasattr(trainer, 'mod')
        if self.resnet:
            from . import gan_cifar_resnet
            self.mod = gan_cifar_resnet
        else:
            self.mod = trainer.mod
        self.name = _short_name(self.mod)
        self.width = int(width) if width is not None else DEFAULT_WIDTH.get(self.name, 1)
        if self.width < 1:
            raise ValueError('Evaluator: width must be >= 1')
        self.with_slope = self.name == 'gan_cifar'          # TF/CT_gan_cifar.py:145,149,225-228

    @property
    def rng(self):
        return eval_stream(self.t)

    # ------------------------------------------------------------------ inputs
    def _to_dev(self, a):
        if not torch.is_tensor(a):
            a = torch.from_numpy(np.ascontiguousarray(a))
        dtype = torch.float32 if a.dtype.is_floating_point else torch.int32
        return a.to(device=self.t.dev, dtype=dtype).contiguous()

    def _unpack(self, batch):
        """One dev batch as the loaders yield it -> (data, labels or None) on the device."""
        if isinstance(batch, (tuple, list)):
            data, labels = batch[0], (batch[1] if len(batch) > 1 else None)
        else:
            data, labels = batch, None
        if not self.resnet:
            return self._to_dev(data), None
        if labels is None:
            raise ValueError('Evaluator: the conditional ResNet takes (images, labels) dev batches')
        return self._to_dev(data), self._to_dev(labels)

    # ------------------------------------------------------------------ dev cost
    def dev_cost(self, batches, rnd=None):
        """Mean of the script's disc_cost over `batches` (an iterable of dev batches as the loaders yield them; (images, labels) for the
        ResNet) -> {'dev_cost': float, 'n_batches': int} (+ 'slope_real' for gan_cifar).  `rnd` (parity mode): one dict of injected
        draws per dev batch, with the keys Trainer.d_losses / DCGANTrainer.d_losses take (+ 'u_slope' for gan_cifar's last batch)."""
        vals, n = self.dev_cost_device(batches, rnd)
        keys = list(vals)
        host = torch.stack([vals[k].reshape(()) for k in keys]).tolist()           # the call's one host synchronisation
        out = dict(zip(keys, host))
        out['n_batches'] = n
        return out

    def dev_cost_device(self, batches, rnd=None):
        """dev_cost without its host synchronisation -> ({'dev_cost': 0-dim device tensor [, 'slope_real': ...]}, number of batches)."""
        F.prepare_filters()
        total, n, group, last = None, 0, [], None
        with F.weight_grads(False):
            for batch in batches:
                group.append(self._unpack(batch))
                if len(group) == self.width:
                    total, n, last = self._add_pass(total, n, group, rnd), n + len(group), group[-1]
                    group = []
            if group:                    # the ragged last pass: fewer than `width` batches, same code
                total, n, last = self._add_pass(total, n, group, rnd), n + len(group), group[-1]
            if n == 0:
                raise ValueError('Evaluator.dev_cost: no dev batch')
            if rnd is not None and len(rnd) != n:
                raise ValueError('Evaluator.dev_cost: %d injected draws for %d dev batches' % (len(rnd), n))
            vals = {'dev_cost': total / n}
            if self.with_slope:
                vals['slope_real'] = self._slope_real(last[0], rnd[-1] if rnd is not None else None)
        return vals, n

    def _add_pass(self, total, n_done, group, rnd):
        """total + (number of batches) * (mean cost of one pass over `group`), on the device."""
        rnds = None
        if rnd is not None:
            rnds = rnd[n_done:n_done + len(group)]
            if len(rnds) != len(group):
                raise ValueError('Evaluator.dev_cost: fewer injected draws than dev batches')
        rng = self.rng
        rng.begin_step()
        cost = (self._pass_resnet if self.resnet else self._pass_dcgan)(group, rnds, rng)
        rng.end_step()
        part = cost.detach() * float(len(group))
        return part if total is None else total + part

    def _pass_resnet(self, group, rnds, rng):
        """disc_cost of TF/CT_gan_cifar_resnet.py:194-305 over G batches at once: WGAN + CT + GP_LAMBDA GP + ACGAN_SCALE ACGAN, fakes from
        the batches' own labels (two towers per batch: groups = 2 G)."""
        R, cfg = self.mod, self.mod.cfg
        G, B = len(group), cfg.BATCH_SIZE
        n = G * B
        real_int = _cat([d for d, _ in group])
        labels = _cat([lab for _, lab in group])
        assert real_int.shape[0] == n and labels.shape[0] == n, 'every dev batch has BATCH_SIZE rows'
        fuse_heads = R._heads_fusable(rnds, rng)
        if getattr(self.t, 'objective', None) == 'hinge':
            return self._pass_resnet_hinge(real_int, labels, rnds, rng, G, fuse_heads)
        with torch.no_grad():
            z = _cat([torch.cat(r['z'], 0) for r in rnds]) if rnds is not None else None
            fake = R.Generator(n, labels, noise=z, groups=2 * G, rng=rng)
            if R.PREP_FUSION and rnds is None and cfg.OUTPUT_DIM % 4 == 0 and fake.is_contiguous():
                rf, interp, _ = K.critic_prep(real_int, fake, rng.seed, rng._sid(), rng._sid(), rng.ctr, 0.0, 1. / 128, 256.0)
            else:
                deq = _cat([r['dequant'] for r in rnds]) if rnds is not None else rng.uniform(n, cfg.OUTPUT_DIM, lo=0.0, hi=1. / 128)
                real = K.real_prep(real_int, deq, 256.0)
                alpha = _cat([r['alpha'] for r in rnds]) if rnds is not None else rng.uniform(n, 1)
                interp = K.interpolate(real, fake, alpha)
                rf = torch.cat([real, fake], 0)
        # gradient penalty :277-286: dD/dx_hat, first order only
        interp = interp.detach().requires_grad_(True)
        with torch.enable_grad():
            if fuse_heads:        # D(x_hat) itself is never used: the backward starts at the last block with dD/dz (F.gp_head_grad)
                y_gp = R.DiscriminatorTailBody(R.DiscriminatorTrunk(interp), 0.8, 0.5, 0.5, rng=rng, mask_done=True)
                with torch.no_grad():     # (projection head: x_hat row i of the stacked batches carries labels[i], its own batch's)
                    emb = R.projection_table() if cfg.PROJECTION else None
                    gz = F.gp_head_grad(y_gp, lib.param('Discriminator.Output.W'), 1.0 / 0.5, emb=emb, labels=labels if emb is not None else None)
                (grads,) = torch.autograd.grad(y_gp, interp, grad_outputs=gz, create_graph=False)
            else:
                u_gp = _cat_masks(rnds, 'u_gp') if rnds is not None else None
                d_gp = R.Discriminator(interp, labels, 0.8, 0.5, 0.5, u=u_gp, rng=rng, heads=('wgan',))[0]
                (grads,) = torch.autograd.grad(d_gp, interp, grad_outputs=torch.ones_like(d_gp), create_graph=False)
        use_ac = cfg.CONDITIONAL and cfg.ACGAN
        P = lib.param
        with torch.no_grad():
            gp, _ = F.gradient_penalty(grads.detach(), cfg.GP_LAMBDA)
            # dropout passes 1 and 2 share the trunk; pass 2 is needed on the real rows only
            lab_c = R.critic_labels(labels)          # the label-conditioned Layernorm critic: one label per row of every stacked pass
            h = R.DiscriminatorTrunk(rf, torch.cat([lab_c, lab_c], 0) if lab_c is not None else None)
            if fuse_heads:
                y = R.DiscriminatorTailBody(h, 0.8, 0.5, 0.5, rng=rng, mask_done=True, cat_extra=n)
                return F.critic_tail_heads(y, P('Discriminator.Output.W'), P('Discriminator.Output.b'),
                                           P('Discriminator.ACGANOutput.W') if use_ac else None, P('Discriminator.ACGANOutput.b') if use_ac else None,
                                           labels, n, cfg.LAMBDA_2, cfg.Factor_M, cfg.ACGAN_SCALE if use_ac else 0.0, 1.0 / 0.5, gp,
                                           emb=R.projection_table() if cfg.PROJECTION else None)[0]
            u = None
            if rnds is not None:       # rows: real (pass 1) of all batches, fake (pass 1) of all batches, real (pass 2) of all batches
                p1r, p1f, p2r = (_cat_masks(rnds, 'u_pass1', slice(0, B)), _cat_masks(rnds, 'u_pass1', slice(B, 2 * B)),
                                 _cat_masks(rnds, 'u_pass2', slice(0, B)))
                u = [torch.cat([a, b, c], 0) for a, b, c in zip(p1r, p1f, p2r)]
            d_all, f_all, a_all = R.DiscriminatorTail(torch.cat([h, h[:n]], 0), 0.8, 0.5, 0.5, u=u, rng=rng,
                                                      labels=torch.cat([lab_c, lab_c, lab_c], 0) if lab_c is not None else None,
                                                      proj_labels=torch.cat([labels, labels, labels], 0) if cfg.PROJECTION else None)
            return F.critic_heads(d_all, f_all, a_all if use_ac else None, labels, n, cfg.LAMBDA_2, cfg.Factor_M,
                                  cfg.ACGAN_SCALE if use_ac else 0.0, gp)[0]

    def _pass_resnet_hinge(self, real_int, labels, rnds, rng, G, fuse_heads):
        """The hinge critic cost (Trainer(objective='hinge'); NOT in the reference) over G batches at once: mean max(0, 1 - D(x)) + mean
        max(0, 1 + D(G(z))) + ACGAN_SCALE ACGAN, one dropout pass over [real ; fake] - the call sites of Trainer.d_losses_hinge."""
        R, cfg = self.mod, self.mod.cfg
        n = real_int.shape[0]
        use_ac = cfg.CONDITIONAL and cfg.ACGAN
        P = lib.param
        with torch.no_grad():
            z = _cat([torch.cat(r['z'], 0) for r in rnds]) if rnds is not None else None
            fake = R.Generator(n, labels, noise=z, groups=2 * G, rng=rng)
            rf = R.real_fake_inputs(real_int, fake, rng, _cat([r['dequant'] for r in rnds]) if rnds is not None else None)
            lab2 = torch.cat([labels, labels], 0)
            if fuse_heads:
                y = R.DiscriminatorTailBody(R.DiscriminatorTrunk(rf), 0.8, 0.5, 0.5, rng=rng, mask_done=True)
                if not y.permute(0, 2, 3, 1).is_contiguous():
                    y = F.to_channels_last(y)
                return K.tail_hinge_heads_fwd(y, n, P('Discriminator.Output.W'), P('Discriminator.Output.b'), labels=labels,
                                              emb=R.projection_table() if cfg.PROJECTION else None,
                                              w_ac=P('Discriminator.ACGANOutput.W') if use_ac else None,
                                              b_ac=P('Discriminator.ACGANOutput.b') if use_ac else None,
                                              scale=cfg.ACGAN_SCALE if use_ac else 0.0)[0][0]
            u = None
            if rnds is not None:       # rows: real of all batches, fake of all batches
                u = [torch.cat([a, b], 0) for a, b in zip(_cat_masks(rnds, 'u_pass1', slice(0, cfg.BATCH_SIZE)),
                                                          _cat_masks(rnds, 'u_pass1', slice(cfg.BATCH_SIZE, 2 * cfg.BATCH_SIZE)))]
            d, _, a = R.Discriminator(rf, lab2, 0.8, 0.5, 0.5, u=u, rng=rng)
            cost = F.gan_loss(d, n, 'hinge', 'd')
            if use_ac:
                cost = cost + cfg.ACGAN_SCALE * F.softmax_cross_entropy(a[:n], labels)[0]
            return cost

    def _gen(self, n, z, groups, rng):
        g = self.t.towers * groups
        if g > 1:
            return self.mod.Generator(n, noise=z, rng=rng, groups=g)
        return self.mod.Generator(n, noise=z, rng=rng)

    def _pass_dcgan(self, group, rnds, rng):
        """disc_cost of the shared step (dcgan_step.DCGANTrainer.d_losses) over G batches at once.  'ct': WGAN + CT + LAMBDA GP; the other
        modes: the mode's critic loss on D(real) and D(fake), `towers` statistic groups per critic call."""
        t, m, cfg = self.t, self.mod, self.mod.cfg
        G, B = len(group), cfg.BATCH_SIZE
        n = G * B
        real_in = _cat([d for d, _ in group])
        assert real_in.shape[0] == n, 'every dev batch has BATCH_SIZE rows'
        with torch.no_grad():
            fake = self._gen(n, _cat([r['z'] for r in rnds]) if rnds is not None else None, G, rng)
            real = m.real_prep(real_in)
            if t.mode.loss != 'ct':
                x = torch.cat([real, fake], 0)
                # (objective='hinge' keeps the CT default's critic: no batch norm, no `groups`)
                kw = {} if t.mode.loss == 'hinge' else {'groups': 2 * t.towers * G}
                if rnds is not None:
                    u = [torch.cat([a, c], 0) for a, c in zip(_cat_masks(rnds, 'u_real'), _cat_masks(rnds, 'u_fake'))]
                    d, _ = m.Discriminator(x, u=u, **kw)
                else:
                    d, _ = m.Discriminator(x, rng=rng, **kw)
                if t.mode.loss == 'wgan':
                    return F.mean_diff(d, n, n, -1.0, 1.0)
                return F.gan_loss(d, n, t.mode.loss, 'd')
            alpha = _cat([r['alpha'] for r in rnds]) if rnds is not None else rng.uniform(n, 1)
            interp = K.interpolate(real, fake, alpha)
            # rows of the batched passes: real (masks A), fake (masks C), real (masks B) - the order the fused loss heads read
            u = None
            if rnds is not None:
                u = [torch.cat([a, c, b], 0) for a, b, c in zip(_cat_masks(rnds, 'u_real'), _cat_masks(rnds, 'u_real_'), _cat_masks(rnds, 'u_fake'))]
            from . import dcgan_step
            if dcgan_step.TRUNK_SHARE and hasattr(m, 'DiscriminatorTrunk') and getattr(m, 'critic_is_per_sample', lambda: True)():
                h = m.DiscriminatorTrunk(torch.cat([real, fake], 0))
                h3 = F.rows_select(h, [(0, n), (n, 2 * n), (0, n)])
                d, f = m.DiscriminatorTail(h3, u=u, rng=None if rnds is not None else rng)
            else:
                x3 = torch.cat([real, fake, real], 0)
                d, f = m.Discriminator(x3, u=u) if rnds is not None else m.Discriminator(x3, rng=rng)
        interp = interp.detach().requires_grad_(True)
        with torch.enable_grad():
            d_gp = (m.Discriminator(interp, u=_cat_masks(rnds, 'u_gp')) if rnds is not None else m.Discriminator(interp, rng=rng))[0]
            (grads,) = torch.autograd.grad(d_gp, interp, grad_outputs=torch.ones_like(d_gp), create_graph=False)
        with torch.no_grad():
            gp, _ = F.gradient_penalty(grads.detach(), cfg.LAMBDA)
            return F.critic_heads(d, f, None, None, n, cfg.LAMBDA_2, cfg.Factor_M, 0.0, gp)[0]

    def _slope_real(self, real_in, rnd):
        """max_b ||dD(real_b)/dreal_b||_2 over one batch, under a dropout pass with masks of its own (TF/CT_gan_cifar.py:145,149,225-228:
        the scripts report the LAST dev batch's)."""
        m, rng = self.mod, self.rng
        rng.begin_step()
        with torch.no_grad():
            real = m.real_prep(real_in)
        real = real.detach().requires_grad_(True)
        with torch.enable_grad():
            d = (m.Discriminator(real, u=rnd['u_slope']) if rnd is not None else m.Discriminator(real, rng=rng))[0]
            (g,) = torch.autograd.grad(d, real, grad_outputs=torch.ones_like(d), create_graph=False)
        rng.end_step()
        with torch.no_grad():
            _, slopes = F.gradient_penalty(g.detach(), 1.0)
            return slopes.max()

    # ------------------------------------------------------------------ score samples
    def score_draws(self, n, labels=None, chunk=None, averaged=False):
        """Yields (samples fp32 [m, OUTPUT_DIM] as the generator returns them, their labels int32 [m] - None for an unconditional
        generator) until `n` samples are out.  Samples are drawn on the evaluation stream in statistic groups of 100
        (samples_100 = Generator(100, ...)); `chunk` samples (a multiple of 100; None: DEFAULT_SCORE_CHUNK) share one generator call.
        ResNet: `labels` [n] int32, or drawn uniformly in [0, 10) on the evaluation stream (:351).  averaged (NOT in the reference): the
        samples come from the generator's weight average - the whole iteration runs inside `trainer.averaged()`, which is left when
        the iterator is exhausted or closed, so consume it to its end (or close it) before training on."""
        if self.name not in SCORE_SCALE:
            raise NotImplementedError('%s: the script scores no samples (no three-channel output)' % self.mod.__name__)
        chunk = DEFAULT_SCORE_CHUNK[self.name] if chunk is None else int(chunk)
        if chunk < SCORE_GROUP or chunk % SCORE_GROUP:
            raise ValueError('score samples: chunk must be a positive multiple of %d' % SCORE_GROUP)
        if averaged:
            with self.t.averaged():
                yield from self.score_draws(n, labels, chunk)
            return
        rng = self.rng
        F.prepare_filters()
        done = 0
        while done < n:
            m = min(chunk, n - done)
            groups = (m + SCORE_GROUP - 1) // SCORE_GROUP
            drawn = groups * SCORE_GROUP            # whole statistic groups; a trailing partial group is cut after the draw
            lab = None
            rng.begin_step()
            with torch.no_grad():
                if self.resnet:
                    lab = rng.labels(drawn, 10)
                    if labels is not None:
                        lab[:m] = labels[done:done + m].to(device=lab.device, dtype=torch.int32)
                    x = self.mod.Generator(drawn, lab, groups=groups, rng=rng)
                elif groups > 1:
                    x = self.mod.Generator(drawn, rng=rng, groups=groups)
                else:
                    x = self.mod.Generator(drawn, rng=rng)
            rng.end_step()
            yield x.contiguous()[:m], (lab[:m] if lab is not None else None)
            done += m

    def score_samples(self, n, labels=None, scale=255.99 / 2, chunk=None, averaged=False):
        """Yields uint8 [m, H, W, 3] pixel tensors, trunc((sample + 1) * scale), of the samples of score_draws(n, labels, chunk, averaged)."""
        side = int(round(math.sqrt(self.mod.cfg.OUTPUT_DIM // 3)))
        for x, _ in self.score_draws(n, labels, chunk, averaged):
            yield K.pixels_u8(x, 3, scale).reshape(x.shape[0], side, side, 3)

    def get_inception_score(self, n, classifier, splits=10, scale=None, averaged=False):
        """(mean, std) of the score over `n` samples: `classifier` (a host callable) gets float32 [m, H, W, 3] arrays in [0, 255] and
        returns class probabilities [m, n_classes] (tflib.inception_score).  `scale`: None = the script's literal (SCORE_SCALE).
        averaged: the samples come from the generator's weight average (score_draws)."""
        from .tflib.inception_score import score_from_probabilities
        if classifier is None:
            raise ValueError('get_inception_score needs a classifier: none ships with this library')
        scale = SCORE_SCALE[self.name] if scale is None else scale
        preds = [np.asarray(classifier(px.cpu().numpy().astype(np.float32))) for px in self.score_samples(n, scale=scale, averaged=averaged)]
        return score_from_probabilities(np.concatenate(preds, 0), splits)

    def get_classifier_score(self, n, scorer, splits=10, averaged=False):
        """The score of `n` samples under `scorer` (a score_cifar.ClassifierScore), everything on the device: samples -> classifier
        input (kernels.score_input) -> logits -> streaming statistic -> {'mean', 'std', 'splits', 'hist', 'acc'}, one host copy; a scorer
        with a reference adds 'frechet' from the same classifier passes.  averaged: the samples come from the generator's weight average."""
        if averaged:
            return scorer.score_generator(self.t, n, splits=splits, averaged=True)
        return scorer.score_generator(self.t, n, splits=splits)


def record_score(ev, series, classifier, averaged=False):
    """One scoring of the loops: the script's sample count through `classifier`, recorded under the script's series names.  A
    score_cifar.ClassifierScore takes the device path (get_classifier_score) and also records `score_acc` where the samples have labels
    and, when the scorer has a reference (ClassifierScore.set_reference), `frechet`: the classifier Frechet distance to it; when it has
    a manifold (ClassifierScore.set_manifold), `precision`, `recall` and `nn_dist`: the k-nearest-neighbour manifold estimate against it; when it has a class reference
    (ClassifierScore.set_class_reference), `intra_frechet`: the mean per-class Frechet distance to it; when it has a kernel reference
    (ClassifierScore.set_kernel_reference), `kid`: the unbiased kernel distance to it; when it has a class manifold or a class kernel
    reference (set_class_manifold, set_class_kernel_reference), `intra_precision` and `intra_recall`, or `intra_kid`.  averaged (NOT in the reference): the samples come
    from the generator's weight average (trainer.averaged) and every series name gets the suffix `_avg` (`inception_50k_avg`,
    `frechet_avg`, `kid_avg`, ...); the loops call it after the live scoring, on the next steps of the evaluation stream."""
    if ev.name not in SCORE_SERIES:
        return
    from .score_cifar import ClassifierScore
    kw = {'averaged': True} if averaged else {}
    sfx = '_avg' if averaged else ''
    if isinstance(classifier, ClassifierScore):
        res = ev.get_classifier_score(SCORE_SAMPLES[ev.name], classifier, **kw)
        for name, value in zip(SCORE_SERIES[ev.name], (res['mean'], res['std'])):
            series.add(name + sfx, value)
        if res['acc'] is not None:
            series.add('score_acc' + sfx, res['acc'])
        if 'frechet' in res:
            series.add('frechet' + sfx, res['frechet'])
        for name in ('precision', 'recall', 'nn_dist', 'intra_frechet', 'kid', 'intra_precision', 'intra_recall', 'intra_kid'):
            if name in res:
                series.add(name + sfx, res[name])
        return
    score = ev.get_inception_score(SCORE_SAMPLES[ev.name], classifier, **kw)
    for name, value in zip(SCORE_SERIES[ev.name], score):
        series.add(name + sfx, value)
