"""The score of CIFAR-10 samples under the project's own CT classifier (ct_cifar.py / ct_cifar_te.py), kept on the device.

The CIFAR scripts' headline number is the score of generator samples (`inception_50k` of TF/CT_gan_cifar_resnet.py:350-360,414-418,
`inception score` of TF/CT_gan_cifar.py:167-176,210-212) under the 2015 Inception graph, which the reference downloads at import and
which cannot ship here.  `ClassifierScore` puts the self-trained CT classifier - evaluated on its averaged parameters, as
`predict(averaged=True)` - in its place, the move score_mnist.py makes for MNIST.  It is a CLASSIFIER score: the Inception-score
formula (TF/tflib/inception_score.py:60-69, tflib.inception_score.score_from_probabilities) over that classifier's 10 CIFAR classes.
Its values are not comparable to published Inception scores (1000 ImageNet classes, another network).

    samples -> classifier input    kernels.score_input   one launch: quantise as the saved pixels (kernels.pixels_u8's bytes), byte table,
                                                         channels-last, rotated by 180 degrees - the classifier's internal form
    classifier input -> logits     ct_cifar._classifier  the deterministic pass on the averaged parameters
    logits -> statistic            kernels.score_accum   per chunk, fp64, into caller-owned device state; kernels.score_finish at the end
No [n, K] prediction array exists; one device -> host copy per scoring (the scores and the class counts).

The normalised filters W g / sqrt(1e-6 + |W|^2) of the ten layers do not change within a scoring: they are made by the layers' own
normalisation launches in the first chunk (tflib.ops.wn_conv.constant_filters) and reused by every later chunk - the logits stay
bit-equal to `predict(averaged=True)` - and made again when the registry's parameter version moves (a classifier that trains on, or
any registry-wide bump: a GAN training between two scorings makes each scoring normalise once).  They are plain tensors owned by the
scorer: no cache outside it holds their addresses, so the conv wrappers pack them per call as they do for `predict`.
"""
import os

import numpy as np
import torch

from . import ct_cifar
from . import kernels as K
from . import tflib as lib
from .tflib.ops import wn_conv as _wn

MAX_CLASSES = 32            # kernels.score_accum keeps a row's class accumulators in registers
DEFAULT_CHUNK = 1000        # rows per classifier pass


def _module(te):
    if te:
        from . import ct_cifar_te
        return ct_cifar_te
    return ct_cifar


class ClassifierScore:
    """ClassifierScore(trainer): scores through a live ct_cifar.CifarSSLTrainer / ct_cifar_te.CifarTETrainer's averaged parameters.
    ClassifierScore(weights=PATH): from a checkpoint ct_cifar.train / ct_cifar_te.train wrote (under the module's current Config): only the
    `Classifier.*` entries are loaded, with the averaged values written into the parameters themselves; no generator parameter is
    created (ct_cifar's `Generator.*` names would be picked up by the GAN modules' params_with_name('Generator')).  When PATH does not
    exist and `data_dir` (or `arrays`) is given, the classifier is trained first - ct_cifar.train (te=True: ct_cifar_te.train) for `epochs`
    epochs, which EMPTIES the registry, so construct the scorer before the GAN's parameters - saved to PATH, and the run's
    `Generator.*` entries are removed."""

    def __init__(self, trainer=None, weights=None, data_dir=None, epochs=None, te=False, **train_kw):
        if (trainer is None) == (weights is None):
            raise ValueError('ClassifierScore: pass a trainer or weights=PATH')
        self.trainer = trainer
        if trainer is None:
            if os.path.isfile(weights):
                self._load(weights)
            else:
                if data_dir is None and train_kw.get('arrays') is None:
                    raise ValueError('ClassifierScore: no checkpoint at %s - pass data_dir= (the CIFAR-10 python batches) to train' % weights)
                self._train(weights, data_dir, epochs, te, train_kw)
        self.cfg = ct_cifar.cfg
        if self.cfg.N_CLASSES > MAX_CLASSES:
            raise ValueError('ClassifierScore: %d classes (the score kernels take at most %d)' % (self.cfg.N_CLASSES, MAX_CLASSES))
        self.dev = lib._dev()
        self.lut = torch.from_numpy(ct_cifar.byte_table()).to(self.dev)
        self._filters, self._version = {}, None

    # ---- construction
    @staticmethod
    def _build_classifier():
        cfg = ct_cifar.cfg
        with torch.no_grad():
            ct_cifar._classifier(K.empty_cl(2, cfg.CHANNELS, cfg.IMG, cfg.IMG, lib._dev()).zero_(), deterministic=True)

    def _load(self, path):
        if [n for n, _ in lib.named_params_with_name('Classifier.') if n.startswith('Classifier.')]:
            raise ValueError('ClassifierScore: the registry already holds Classifier.* parameters')
        ck = torch.load(path, map_location='cpu', weights_only=False)
        sd = {n: v for n, v in ck['params'].items() if n.startswith('Classifier.')}
        avg = ck['d_opt'].get('avg')
        if not sd or avg is None:
            raise ValueError('ClassifierScore: %s holds no CT classifier with parameter averages' % path)
        self._build_classifier()
        named = lib.named_params_with_name('Classifier.')
        trained = lib.named_params_with_name('Classifier.', trainable_only=True)
        bad = [n for n, p in named if n not in sd or tuple(sd[n].shape) != tuple(p.shape)]
        if bad or len(named) != len(sd) or sum(p.numel() for _, p in trained) != avg.numel():
            lib.delete_params_with_name('Classifier.')
            raise ValueError("ClassifierScore: %s does not fit the classifier of ct_cifar's current Config (%s)" % (path, bad[:3]))
        lib.load_state_dict(sd, strict=False)
        off = 0
        with torch.no_grad():
            for _, p in trained:              # the optimizer's flat layout: the trained parameters in registry order
                p.copy_(avg[off:off + p.numel()].view(p.shape))
                off += p.numel()
        lib.bump_epoch('Classifier')

    def _train(self, path, data_dir, epochs, te, train_kw):
        from . import checkpoint
        mod = _module(te)
        tr = mod.train(data_dir, epochs=epochs, **train_kw)
        done = (mod.cfg.EPOCHS if epochs is None else epochs)
        checkpoint.save(path, tr, done, extra=tr.checkpoint_extra())
        with torch.no_grad():
            for p, (_, a) in zip(tr.d_opt.params, tr.d_opt.avg_views()):
                p.copy_(a)
        lib.delete_params_with_name('Generator.')
        lib.bump_epoch('Classifier')

    # ---- samples in internal form -> logits
    def _logits(self, x):
        version = lib.epoch('Classifier')
        if version != self._version:        # (the version also counts registry-wide bumps: a GAN that trains makes every scoring renormalise once)
            self._filters.clear()
            self._version = version

        def run():
            with _wn.constant_filters(self._filters):
                return ct_cifar._classifier(x, deterministic=True)

        if self.trainer is not None:
            logits = self.trainer._averaged(run, True)
        else:
            with torch.no_grad():
                logits = run()
        return logits.contiguous()

    # ---- the statistic
    def _begin(self, n, splits):
        nc = self.cfg.N_CLASSES
        if n < splits or splits < 1:
            raise ValueError('ClassifierScore: %d samples for %d splits' % (n, splits))
        return (torch.zeros(splits, nc + 1, dtype=torch.float64, device=self.dev), torch.zeros(2 * nc, dtype=torch.int64, device=self.dev))

    def _finish(self, acc, cnt, n, splits, with_labels):
        nc = self.cfg.N_CLASSES
        out = K.score_finish(acc, n, splits)
        host = torch.cat([out, cnt.to(torch.float64)]).cpu().numpy()          # the scoring's one device -> host copy (counts < 2^53: exact)
        counts = host[2 + splits:].astype(np.int64)
        return {'mean': float(host[0]), 'std': float(host[1]), 'splits': host[2:2 + splits].copy(), 'hist': counts[:nc].copy(),
                'acc': float(counts[nc:].sum()) / n if with_labels else None}

    def _labels(self, labels, n):
        if labels is None:
            return None
        t = torch.as_tensor(labels).reshape(-1)
        if t.numel() != n:
            raise ValueError('ClassifierScore: %d labels for %d samples' % (t.numel(), n))
        return t.to(device=self.dev, dtype=torch.int32).contiguous()

    def score(self, images_u8, labels=None, splits=10, chunk=None):
        """The score of a uint8 set [N, CHANNELS, IMG, IMG] (the reference's orientation, as CifarSSLData holds it), read through
        kernels.aug_gather's fixed mode in chunks of `chunk` rows (None: min(1000, N)); labels [N]: also the accuracy.
        -> {'mean', 'std', 'splits' [splits], 'hist' [K] predicted-class counts, 'acc' (None without labels)}."""
        cfg = self.cfg
        data = torch.as_tensor(images_u8)
        if data.dtype != torch.uint8 or data.dim() != 4 or tuple(data.shape[1:]) != (cfg.CHANNELS, cfg.IMG, cfg.IMG):
            raise ValueError('ClassifierScore.score: uint8 [N, %d, %d, %d] images expected (got %s %s)'
                             % (cfg.CHANNELS, cfg.IMG, cfg.IMG, data.dtype, tuple(data.shape)))
        n = data.shape[0]
        acc, cnt = self._begin(n, splits)
        data = data.to(self.dev).contiguous()
        labels = self._labels(labels, n)
        chunk = min(DEFAULT_CHUNK, n) if chunk is None else int(chunk)
        if chunk < 1:
            raise ValueError('ClassifierScore.score: chunk must be positive')
        for r0 in range(0, n, chunk):
            m = min(chunk, n - r0)
            idx = torch.arange(r0, r0 + m, dtype=torch.int32, device=self.dev)
            logits = self._logits(K.aug_gather(data, idx, self.lut, cfg.IMG, cfg.PAD))
            K.score_accum(logits, r0, n, splits, acc, cnt, None if labels is None else labels[r0:r0 + m])
        return self._finish(acc, cnt, n, splits, labels is not None)

    def score_generator(self, gan_trainer, n, labels=None, splits=10, chunk=None):
        """The score of `n` samples of a gan_cifar / gan_cifar_resnet trainer's generator, drawn exactly as evaluate.Evaluator.score_samples
        draws them - on the trainer's EVALUATION stream, in statistic groups of 100, `chunk` (a multiple of 100; None: 1000) per
        generator call, the ResNet's labels drawn there unless given - and quantised with the script's SCORE_SCALE as the saved pixels
        are: the training stream, the weights and the optimizers stay untouched.  The ResNet's labels feed the accuracy count."""
        from . import evaluate
        ev = evaluate.Evaluator(gan_trainer)
        cfg = self.cfg
        if ev.name not in evaluate.SCORE_SCALE or ev.mod.cfg.OUTPUT_DIM != cfg.CHANNELS * cfg.IMG * cfg.IMG:
            raise ValueError('ClassifierScore.score_generator: %s samples are not %dx%dx%d images' % (ev.name, cfg.CHANNELS, cfg.IMG, cfg.IMG))
        acc, cnt = self._begin(n, splits)
        labels = self._labels(labels, n)
        scale, r0, with_labels = evaluate.SCORE_SCALE[ev.name], 0, False
        for x, lab in ev.score_draws(n, labels, chunk):
            logits = self._logits(K.score_input(x, cfg.CHANNELS, scale, self.lut))
            K.score_accum(logits, r0, n, splits, acc, cnt, None if lab is None else lab.contiguous())
            with_labels = lab is not None
            r0 += x.shape[0]
        return self._finish(acc, cnt, n, splits, with_labels)
