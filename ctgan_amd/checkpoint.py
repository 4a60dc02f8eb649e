"""Checkpoint / resume of a training run.

The reference has no resume for its CIFAR/MNIST scripts (`np.save("param.pyn", ...)` of the critic only,
TF/CT_gan_cifar.py:216-222; a `tf.train.Saver` in the LSUN script).  Here the registry's names make it
trivial: one file holds every parameter by its reference name and layout, both optimizers' slots (Adam m, v and
beta-power state, or RMSProp ms - tagged with the optimizer kind, so a resume under another MODE fails clearly -, step count), the Philox step counter and the loop iteration - enough for a bit-exact
continuation (tests/test_gpu_checkpoint.py).  The `rng` entry also holds the step counter of the evaluation stream (evaluate.eval_stream:
`eval_ctr`), so that a resumed run logs the dev costs of the uninterrupted one; a file written before that entry existed loads with the
counter at 0.  A trainer with a dynamic loss scale (DCGANTrainer(loss_scale='dynamic')) adds the entry `loss_scaler` - the scale and its
two counts; a run without one writes the keys it always wrote.  A file without the entry starts a dynamic trainer at its init_scale; a
file with it loads into a trainer with a fixed scale, which ignores it.  A trainer with spectral normalisation (`spectral_norm=True`) keeps
`u`, `v`, `sigma` in the entry `spectral` of its critic optimizer's state; `params` hold the RAW weights under their usual names, and
`d_opt.load_state_dict` - which runs after the parameters are restored - recomputes the normalised weights from the saved sigma without
iterating.  A file without the entry starts such a trainer from its constructor's `u` with one iteration; a plain trainer ignores the entry."""
import torch

from . import tflib as lib
from .evaluate import eval_stream


def save(path, trainer, iteration, extra=None):
    scaler = getattr(trainer, 'scaler', None)
    torch.save({
        **({'loss_scaler': scaler.state_dict()} if scaler is not None else {}),
        'format': 1,
        'iteration': int(iteration),
        'params': lib.state_dict(),
        'd_opt': trainer.d_opt.state_dict(),
        'g_opt': trainer.g_opt.state_dict() if trainer.g_opt is not None else None,        # (score_mnist: one optimizer, no stream)
        'rng': {'seed': trainer.rng.seed, 'rank': trainer.rng.rank, 'ctr': int(trainer.rng.ctr.item()),
                'eval_ctr': int(eval_stream(trainer).ctr.item())} if trainer.rng is not None else None,
        'extra': extra or {},
    }, path)


def load(path, trainer):
    """Restores weights, optimizer slots and random-stream position into `trainer`; returns the iteration
    to continue from."""
    ck = torch.load(path, map_location='cpu', weights_only=False)
    if ck.get('format') != 1:
        raise ValueError('unknown checkpoint format')
    lib.load_state_dict(ck['params'], strict=True)
    trainer.d_opt.load_state_dict(ck['d_opt'])
    if trainer.g_opt is not None:
        trainer.g_opt.load_state_dict(ck['g_opt'])
    if trainer.rng is not None:
        trainer.rng.seed = ck['rng']['seed']
        trainer.rng.ctr.fill_(ck['rng']['ctr'])
        eval_stream(trainer).ctr.fill_(ck['rng'].get('eval_ctr', 0))
    if getattr(trainer, 'scaler', None) is not None:
        trainer.scaler.load_state_dict(ck.get('loss_scaler'))
    return ck['iteration']


def load_extra(path):
    """The `extra` dict a checkpoint was saved with (empty if none): state that belongs to one trainer class, restored by its caller."""
    return torch.load(path, map_location='cpu', weights_only=False).get('extra') or {}
