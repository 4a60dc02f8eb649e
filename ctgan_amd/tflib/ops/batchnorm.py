"""tflib.ops.batchnorm - same signature as TF/tflib/ops/batchnorm.py:6-87 (= LS/tflib/ops/batchnorm.py:7-87).

is_training=None (every CT script): training-mode batch statistics; the moving statistics are registered and never written.
is_training=True / False (LS/inception_score.py through LS/tflib/train_loop_2.py's `bn_vars`): the `tf.cond` of :52-69, decided on the
host - a Python bool, not a tensor.  True: batch statistics and, with update_moving_stats, the update of :62-65 with `stats_iter` an int
or a device scalar tensor (read on the device, so a captured step replays with the current value).  False: the blend of :32-38, forward
only, no update.
Build-only kwargs: `groups` (independent statistic groups = the reference's per-tower batches; is_training=None only),
`relu` (fuse the ReLU that always follows in the generators), `act` = 'lrelu' | 'tanh' | 'gate' with `alpha` (is_training=None, axes
[0,2,3] only: the LeakyReLU / tanh / gated nonlinearity that follows in the DCGAN-style 64x64 nets, functional.batch_norm_act), `resid` / `resid_scale` / `want_elu` (is_training True / False only):
the result is resid + resid_scale * Batchnorm(inputs) and, with want_elu, the pair (result, elu(result)) - the epilogue of
LS/inception_score.py's residual block in the normalisation's own apply pass.
"""
import numpy as np
import torch

from ... import functional as F
from ... import kernels as K
from .. import param as _param


def Batchnorm(name, axes, inputs, is_training=None, stats_iter=None, update_moving_stats=True, fused=True,
              groups=1, relu=False, resid=None, resid_scale=1.0, want_elu=False, act=None, alpha=0.2):
    if act is not None and (is_training is not None or axes != [0, 2, 3] or not fused or relu or resid is not None or want_elu):
        raise ValueError('Batchnorm: act needs is_training=None on the fused [0,2,3] path, without relu / resid / want_elu')
    fuse = dict(shortcut=resid, alpha=resid_scale, want_elu=want_elu)
    if (resid is not None or resid_scale != 1.0 or want_elu) and (is_training is None or axes != [0, 2, 3] or not fused or relu):
        raise ValueError('Batchnorm: resid / resid_scale / want_elu need is_training True or False on the fused [0,2,3] path, without relu')
    if ((axes == [0, 2, 3]) or (axes == [0, 2])) and fused:
        if is_training is not None:
            if torch.is_tensor(is_training) or not isinstance(is_training, (bool, np.bool_)):
                raise TypeError('Batchnorm: is_training is a Python bool or None (there is no tf.cond here)')
            if groups != 1:
                raise ValueError('Batchnorm: groups > 1 needs is_training=None')
            if is_training and update_moving_stats and stats_iter is None:
                raise ValueError('Batchnorm: update_moving_stats needs stats_iter (:62)')
        x = inputs.unsqueeze(3) if axes == [0, 2] else inputs
        C = x.shape[1]
        offset = _param(name + '.offset', lambda rng: np.zeros(C, dtype='float32'))
        scale = _param(name + '.scale', lambda rng: np.ones(C, dtype='float32'))
        moving_mean = _param(name + '.moving_mean', lambda rng: np.zeros(C, dtype='float32'), trainable=False)
        moving_variance = _param(name + '.moving_variance', lambda rng: np.ones(C, dtype='float32'), trainable=False)
        if act is not None:
            return F.batch_norm_act(x, scale, offset, act, alpha, groups)
        if is_training is None:
            out = F.batch_norm(x, scale.view(1, C), offset.view(1, C), None, groups, relu)
        elif is_training:
            moving = (moving_mean.data, moving_variance.data, K.device_scalar(stats_iter, x.device)) if update_moving_stats else None
            out = F.batch_norm_moving(x, scale, offset, moving, relu=relu, **fuse)
        else:
            out = F.batch_norm_blend(x, scale, offset, moving_mean.data, moving_variance.data, relu=relu, **fuse)
        if want_elu:
            return out
        return out[:, :, :, 0] if axes == [0, 2] else out
    if axes == [0] and inputs.dim() == 2:
        C = inputs.shape[1]
        offset = _param(name + '.offset', lambda rng: np.zeros([1, C], dtype='float32'))   # moments' shape (:78-83)
        scale = _param(name + '.scale', lambda rng: np.ones([1, C], dtype='float32'))
        return F.batch_norm(inputs, scale, offset, None, groups, relu)        # (the reference's else branch ignores is_training, :75-87)
    raise NotImplementedError('Batchnorm axes %s: only [0,2,3], [0,2] and [0] (2-D input) are used' % (axes,))
