"""What the three semi-supervised CT classifiers (ct_mnist, ct_cifar, ct_cifar_te; TH/ = CT-GANs/Theano_classifier of the reference)
share on the host: the `Config` base, the trainer's step plumbing (`SSLTrainerBase`) and the scripts' epoch loop (`train_loop`).  The
networks, the losses, the data classes and the literals stay in the three modules."""
import os
import time

import torch

from . import tflib as lib
from .optim import FlatAdamTheano
from .rng import DeviceRNG


class Config:
    """Hyper-parameters as class attributes (a module's Config holds its script's literals); keywords override known ones."""

    def __init__(self, **kw):
        for k, v in kw.items():
            if not hasattr(type(self), k):
                raise AttributeError('unknown hyper-parameter %s' % k)
            setattr(self, k, v)


class SSLTrainerBase:
    """The two Theano functions train_batch_disc / train_batch_gen as steps.  A trainer class supplies `cfg` (its module's current
    Config), `d_losses(*batch)` and `g_losses(x_unl)`, and states as data
        d_cotangents()   {output vector of d_losses: its cotangent} - the classifier's cost is the sum of the products
        D_KEYS           the entries of d_losses' result that d_body returns, detached
        REPORT           the epoch line of train_loop: (first word, ((label, output averaged over the epoch), ..),
                         ((label, output summed over the epoch), ..))
    A classifier batch is whatever d_losses takes; `train_iteration` takes it followed by the generator's unlabelled batch."""
    D_KEYS = ()
    REPORT = None

    def __init__(self, build_params, seed=None):
        cfg = self.cfg
        self.dev = lib._dev()
        self.rng = DeviceRNG(cfg.SEED if seed is None else seed, 0, self.dev)
        build_params()
        self.d_named = lib.named_params_with_name('Classifier', trainable_only=True)
        self.g_named = lib.named_params_with_name('Generator', trainable_only=True)
        self.d_params = [p for _, p in self.d_named]
        self.g_params = [p for _, p in self.g_named]
        self.d_opt = FlatAdamTheano(self.d_named, cfg.BETA1, cfg.BETA2, avg_rate=cfg.AVG_RATE)
        self.g_opt = FlatAdamTheano(self.g_named, cfg.BETA1, cfg.BETA2, avg_rate=0.0)
        self.d_heads = [(k, torch.tensor(v, dtype=torch.float32, device=self.dev)) for k, v in self.d_cotangents().items()]
        self.iteration = 0

    def lr(self):
        return self.cfg.LR

    # ---- classifier step
    def d_grads(self, *batch):
        out = self.d_losses(*batch)
        grads = torch.autograd.grad([out[k] for k, _ in self.d_heads], self.d_params, grad_outputs=[c for _, c in self.d_heads],
                                    allow_unused=True)
        return out, grads

    def d_body(self, *batch):
        """Losses, gradients, Adam + average, end of step - everything a replayed graph holds (the learning rate is device state)."""
        out, grads = self.d_grads(*batch)
        self.d_opt.update(grads, rng=self.rng)
        return {k: out[k].detach() for k in self.D_KEYS}

    def d_step(self, *batch):
        self.d_opt.set_lr(self.lr())
        return self.d_body(*batch)

    # ---- generator step
    def g_grads(self, x_unl):
        out = self.g_losses(x_unl)
        grads = torch.autograd.grad(out['loss_gen'], self.g_params, allow_unused=True)
        return out, grads

    def g_body(self, x_unl):
        out, grads = self.g_grads(x_unl)
        self.g_opt.update(grads, rng=self.rng)
        return {'loss_gen': out['loss_gen'].detach()}

    def g_step(self, x_unl):
        self.g_opt.set_lr(self.lr())
        return self.g_body(x_unl)

    def train_iteration(self, *batch):
        """One classifier step on batch[:-1] and one generator step on batch[-1]."""
        out = self.d_step(*batch[:-1])
        out.update(self.g_step(batch[-1]))
        self.iteration += 1
        return out

    # ---- evaluation on the averaged parameters
    def _averaged(self, fn, averaged):
        """fn() without gradients; averaged: with every trained classifier parameter replaced by its average (`givens`) - a
        parameter that is not trained has no average and stays live."""
        if averaged:
            own = {p: a for p, (_, a) in zip(self.d_opt.params, self.d_opt.avg_views())}
            lib.alias_params(own)
        try:
            with torch.no_grad():
                return fn()
        finally:
            if averaged:
                lib.delete_param_aliases(own)        # its own entries only: another owner's aliases stay installed

    # ---- what train_loop asks of a trainer beside the steps: nothing, except with temporal ensembling
    def end_epoch(self):
        pass

    def checkpoint_extra(self):
        """State a checkpoint carries beside checkpoint.save's own."""
        return {}

    def restore_extra(self, path, epoch):
        """Restores checkpoint_extra() from the checkpoint at `path`, written after `epoch` epochs."""


def train_loop(trainer, data, engine_cls, init, epochs=None, use_graphs=True, out_dir=None, resume=None, checkpoint_every=1, log=print,
               max_batches=None):
    """The scripts' epoch loop.  `data`: begin_epoch() -> number of batches, batch(t) -> the arrays of one train_iteration,
    test_set() -> (x, y).  `init(trainer, data)`: the data-dependent init, run after the first begin_epoch() of a run that does not
    resume.  `engine_cls`: the graphed engine (graph replay unless use_graphs=False).  Per epoch: one train_iteration per batch,
    trainer.end_epoch(), the test error on the averaged parameters, the report line trainer.REPORT describes (also one record of
    train_log.Series in `out_dir`/log.jsonl); every `checkpoint_every` epochs a checkpoint (checkpoint.py, with
    trainer.checkpoint_extra()) in `out_dir`; `resume` continues from one at the epoch it was written.  max_batches: shorten the
    epochs.  Returns the trainer."""
    from . import checkpoint
    from .train_log import Series
    word, means, sums = trainer.REPORT
    start = 0
    if resume:
        start = checkpoint.load(resume, trainer)
        trainer.restore_extra(resume, start)
    for _ in range(start):             # the host streams of the epochs already run
        data.begin_epoch()
    eng = None
    series = Series(os.path.join(out_dir, 'log.jsonl') if out_dir else None, echo=None)
    series.iteration = start
    for epoch in range(start, trainer.cfg.EPOCHS if epochs is None else epochs):
        begin = time.time()
        n = data.begin_epoch()
        n = n if max_batches is None else min(n, max_batches)
        if eng is None:
            if not resume:
                init(trainer, data)
            eng = engine_cls(trainer, use_graphs=use_graphs)
        outs, totals = [], [[] for _ in sums]
        for t in range(n):
            out = eng.train_iteration(*[torch.from_numpy(a) for a in data.batch(t)])
            outs.append(torch.stack([out[k] for _, k in means]))
            for tot, (_, k) in zip(totals, sums):
                tot.append(out[k].clone())
        trainer.end_epoch()
        m = torch.stack(outs).cpu().numpy().mean(0)
        row = [(label, m[i]) for i, (label, _) in enumerate(means)]
        row += [(label, float(torch.stack(tot).sum().item())) for tot, (label, _) in zip(totals, sums)]      # never divided, as the scripts
        test_err = trainer.test_error(*data.test_set())
        # the scripts' own spacing: `, ` between the averaged entries, a bare `,` around the summed ones
        log('%s %d, time = %ds' % (word, epoch, time.time() - begin) + ''.join(', %s = %.4f' % kv for kv in row[:len(means)])
            + ''.join(',%s = %.4f' % kv for kv in row[len(means):]) + (',' if sums else ', ') + 'test err = %.4f' % test_err)
        for k, v in row + [('test err', test_err), ('time', time.time() - begin)]:
            series.add(k, v)
        series.tick()
        series.flush()
        if out_dir and checkpoint_every and (epoch + 1) % checkpoint_every == 0:
            checkpoint.save(os.path.join(out_dir, 'checkpoint.pt'), trainer, epoch + 1, extra=trainer.checkpoint_extra())
    return trainer
