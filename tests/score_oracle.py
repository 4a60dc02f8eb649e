"""Torch restatement (fp64 by default, autograd; any dtype - fp32 gives the twin) of the reference's self-trained MNIST score
classifier: LS/inception_score.py with the parts of LS/tflib/ops/batchnorm.py and LS/tflib/train_loop_2.py it uses (LS/ =
tensorflow_generative_model/LSUN_bedrooms of the reference).  TEST INFRASTRUCTURE ONLY.  Written from the scripts' mathematics, cited
by line; nothing of their text is reused.  Parameters are a name -> tensor dict under the product's registry names and layouts
(`.Filters` HWIO, `.W` [in,out]).

One thing is TensorFlow's and not visible in the reference tree: in training tf.nn.fused_batch_norm returns as batch variance the
biased variance times n/(n-1) (Bessel), n = N*H*W - that is what batchnorm.py:65 blends into moving_variance.  The divisor is
max(n-1, 1) so that a single element leaves the variance 0 instead of 0/0.
"""
import collections
import math

import numpy as np
import torch

from oracle import tf_ops

EPS = 1e-5                      # LS/tflib/ops/batchnorm.py:31,38


def elu(x):
    """tf.nn.elu (inception_score.py:38-39)"""
    return torch.where(x > 0, x, torch.expm1(torch.clamp(x, max=0)))


def bn_training(x, scale, offset):
    """batchnorm.py:30-31: tf.nn.fused_batch_norm in training -> (y, batch_mean, batch_var); batch_var carries the n/(n-1) factor."""
    n = x.shape[0] * x.shape[2] * x.shape[3]
    mean, var = tf_ops.moments(x, [0, 2, 3])
    y = tf_ops.batch_normalization(x, mean, var, offset[None, :, None, None], scale[None, :, None, None], EPS)
    return y, mean.reshape(-1), var.reshape(-1) * (n / max(n - 1, 1))


def moving_update(moving, batch, it):
    """batchnorm.py:62-65 - no special case at it = 0: the old value gets weight 0."""
    it = float(it)
    return (it / (it + 1)) * moving + (1 / (it + 1)) * batch


def bn_blend(x, scale, offset, moving_mean, moving_var):
    """batchnorm.py:32-38: per-sample moments over (h, w), blended with the moving statistics by the row count of the call."""
    B = float(x.shape[0])
    mean, var = tf_ops.moments(x, [2, 3])
    mean = (1. / B) * mean + ((B - 1.) / B) * moving_mean[None, :, None, None]
    var = (1. / B) * var + ((B - 1.) / B) * moving_var[None, :, None, None]
    return tf_ops.batch_normalization(x, mean, var, offset[None, :, None, None], scale[None, :, None, None], EPS)


def batchnorm(P, name, x, is_training, stats_iter, moved):
    """Batchnorm(name, [0,2,3], x, is_training, stats_iter, update_moving_stats=True); `moved` receives the new moving statistics."""
    scale, offset = P[name + '.scale'], P[name + '.offset']
    if is_training:
        y, bm, bv = bn_training(x, scale, offset)
        moved[name + '.moving_mean'] = moving_update(P[name + '.moving_mean'], bm.detach(), stats_iter)
        moved[name + '.moving_variance'] = moving_update(P[name + '.moving_variance'], bv.detach(), stats_iter)
        return y
    return bn_blend(x, scale, offset, P[name + '.moving_mean'], P[name + '.moving_variance'])


def conv(P, name, x, stride=1):
    return tf_ops.bias_add_nchw(tf_ops.conv2d_same(x, P[name + '.Filters'], stride), P[name + '.Biases'])


def residual_block(P, name, x, resample, is_training, stats_iter, moved, res_scale):
    """inception_score.py:52-93 (mask_type None)"""
    if name + '.Shortcut.Filters' in P:
        shortcut = conv(P, name + '.Shortcut', x, 2 if resample == 'down' else 1)       # :77
    else:
        shortcut = x                                                                     # :75
    out = elu(x)                                                                         # :81
    out = conv(P, name + '.Conv1', out)                                                  # :82
    out = elu(out)                                                                       # :83
    out = conv(P, name + '.Conv2', out, 2 if resample == 'down' else 1)                  # :84
    out = batchnorm(P, name + '.BN', out, is_training, stats_iter, moved)                # :85
    return shortcut + res_scale * out                                                    # :93


def classifier(P, x, is_training, stats_iter=0, moved=None, res_scale=.3):
    """build_model (:101-108): x [N,784] -> logits [N,10]"""
    moved = {} if moved is None else moved
    out = x.reshape(-1, 1, 28, 28)
    out = conv(P, 'InceptionScore.Conv1', out)
    for k, resample in ((1, 'down'), (2, None), (3, 'down'), (4, None)):
        out = residual_block(P, 'InceptionScore.Res%d' % k, out, resample, is_training, stats_iter, moved, res_scale)
    out = out.mean(dim=(2, 3))                                                           # :107
    return out @ P['InceptionScore.Linear.W'] + P['InceptionScore.Linear.b']             # :108


def cost_acc(logits, y):
    """:118-130"""
    cost = tf_ops.sparse_softmax_ce(logits, y).mean()
    acc = (logits.argmax(dim=1) == y.long()).to(logits.dtype).mean()
    return cost, acc


def inception(logits):
    """:132-135, in fp64"""
    p = torch.softmax(logits.double(), dim=1)
    kl = p * (torch.log(p) - torch.log(p.mean(dim=0, keepdim=True)))
    return math.exp(kl.sum(dim=1).mean().item())


def top2_gap(logits):
    t = logits.topk(2, dim=1).values
    return (t[:, 0] - t[:, 1]).min().item()


def param_names(widths=(32, 32, 32, 64, 64)):
    """Registry names in creation order -> shape; the trainable ones are those that are not moving statistics."""
    W = widths
    names = collections.OrderedDict()

    def conv_(name, k, cin, cout):
        names[name + '.Filters'] = (k, k, cin, cout)
        names[name + '.Biases'] = (cout,)
    conv_('InceptionScore.Conv1', 3, 1, W[0])
    for k, resample in ((1, 'down'), (2, None), (3, 'down'), (4, None)):
        name, cin, cout = 'InceptionScore.Res%d' % k, W[k - 1], W[k]
        if resample == 'down' or cin != cout:
            conv_(name + '.Shortcut', 1, cin, cout)
        conv_(name + '.Conv1', 3, cin, cin if resample == 'down' else cout)
        conv_(name + '.Conv2', 3, cin if resample == 'down' else cout, cout)
        for s in ('offset', 'scale', 'moving_mean', 'moving_variance'):
            names['%s.BN.%s' % (name, s)] = (cout,)
    names['InceptionScore.Linear.W'] = (W[4], 10)
    names['InceptionScore.Linear.b'] = (10,)
    return names


def is_moving(n):
    return n.endswith(('.moving_mean', '.moving_variance'))


def make_params(widths=(32, 32, 32, 64, 64), seed=0, dtype=torch.float64, head_gain=4.0):
    """Random parameters away from the initial values (non-trivial scale / offset / moving statistics); values are fp32-representable.
    head_gain spreads the logits so that the top-two gap is far above fp32 noise."""
    g = torch.Generator().manual_seed(seed)
    P = collections.OrderedDict()
    for n, shape in param_names(widths).items():
        if n.endswith('.Filters'):
            v = torch.randn(shape, generator=g) / math.sqrt(shape[0] * shape[1] * shape[2])
        elif n.endswith('.W'):
            v = head_gain * torch.randn(shape, generator=g) / math.sqrt(shape[0])
        elif n.endswith(('.scale', '.moving_variance')):
            v = torch.rand(shape, generator=g) + 0.5
        else:
            v = 0.1 * torch.randn(shape, generator=g)
        P[n] = v.float().to(dtype)
    return P


def train_step(P, slots, t, x, y, lr=1e-3, betas=(.9, .999), eps=1e-8, clip=5., res_scale=.3):
    """train_fn (train_loop_2.py:76-92) with bn_vars = (True, 0): cost, acc, the global norm of the gradients, the gradients clipped by
    it at `clip`, TF-form Adam (t counts from 1), the moving statistics replaced by this batch's.  slots: name -> (m, v).
    -> dict(cost, acc, gradnorm, grads (before the clip), P (new), slots (new))"""
    dtype = next(iter(P.values())).dtype
    names = [n for n in P if not is_moving(n)]
    leaves = collections.OrderedDict((n, P[n].detach().clone().requires_grad_(True)) for n in names)
    Q = collections.OrderedDict((n, leaves.get(n, P[n])) for n in P)
    moved = {}
    logits = classifier(Q, x.to(dtype), True, 0, moved, res_scale)
    cost, acc = cost_acc(logits, y)
    grads = dict(zip(names, torch.autograd.grad(cost, list(leaves.values()))))
    gradnorm = math.sqrt(sum((g.double() ** 2).sum().item() for g in grads.values()))        # tf.global_norm (:76)
    factor = clip / max(gradnorm, clip)                                                       # tf.clip_by_global_norm (:79)
    newP, new_slots = collections.OrderedDict(), {}
    for n in P:
        if n in moved:
            newP[n] = moved[n]
        else:
            m, v = slots[n]
            newP[n], m, v = tf_ops.tf_adam_step(P[n], grads[n] * factor, m, v, t, lr, betas[0], betas[1], eps)
            new_slots[n] = (m, v)
    return {'cost': cost.detach(), 'acc': acc, 'gradnorm': gradnorm, 'grads': grads, 'P': newP, 'slots': new_slots, 'logits': logits.detach()}


def zero_slots(P):
    return {n: (torch.zeros_like(v), torch.zeros_like(v)) for n, v in P.items() if not is_moving(n)}


def stats_pass(P, x, i, res_scale=.3):
    """bn_stats_fn (train_loop_2.py:94-101): a training-mode forward with stats_iter = i -> P with the moved statistics."""
    moved = {}
    with torch.no_grad():
        classifier(P, x, True, i, moved, res_scale)
    return collections.OrderedDict((n, moved.get(n, v)) for n, v in P.items())


def evaluate(P, x, y, res_scale=.3):
    """eval_fn (:103-111): inference mode -> cost, acc, inception (floats)"""
    with torch.no_grad():
        logits = classifier(P, x, False, 0, None, res_scale)
        cost, acc = cost_acc(logits, y)
    return cost.item(), acc.item(), inception(logits), logits


def rel_l2(a, b):
    return ((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-30)).item()


def step_inputs(B, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(B, 784, generator=g), torch.randint(0, 10, (B,), generator=g, dtype=torch.int32)


def as_numpy(P):
    return collections.OrderedDict((n, np.asarray(v.detach().float())) for n, v in P.items())
