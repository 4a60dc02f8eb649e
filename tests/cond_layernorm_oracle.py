"""TEST-ONLY fp64 restatement of the label-conditioned Layernorm (LS/tflib/ops/layernorm.py:6-34) on the oracle's registry, and the
critic-side Normalize of TF/CT_gan_cifar_resnet.py:70-87 that calls it.  oracle/nets.py already hands `labels` / `[labels ; labels]`
to the critic's blocks; its Normalize drops them at the Layernorm (the main-tree operator takes none), so the tests that need the
"vanilla" conditional critic monkeypatch oracle.nets.Normalize with `normalize` below."""
import numpy as np
import torch

from oracle import nets as onets
from oracle import tf_ops
from oracle import tflib_ref as oref


def Layernorm(reg, name, norm_axes, inputs, labels=None, n_labels=None):
    """Per-sample moments over norm_axes; without labels `name.scale` / `name.offset` of size C, with labels [n_labels, C] tables looked
    up per sample (:21-25) and broadcast over H and W (:29-30); any norm_axes but [1, 2, 3] with labels is 'unsupported' (:27-28)."""
    norm_axes = list(norm_axes)
    if labels is None:
        return oref.Layernorm(reg, name, norm_axes, inputs)
    mean, var = tf_ops.moments(inputs, norm_axes)
    C = inputs.shape[norm_axes[0]]
    offset_m = reg.param(name + '.offset', lambda rng: np.zeros([n_labels, C], dtype='float32'))
    scale_m = reg.param(name + '.scale', lambda rng: np.ones([n_labels, C], dtype='float32'))
    offset, scale = offset_m[labels.long()], scale_m[labels.long()]
    if norm_axes != [1, 2, 3]:
        raise Exception('unsupported')
    return tf_ops.batch_normalization(inputs, mean, var, offset[:, :, None, None], scale[:, :, None, None], 1e-5)


def layer_norm(x, scale, offset, labels=None, eps=1e-5):
    """The bare operator on explicit tensors (any rank >= 2, moments over all non-batch axes): scale / offset [C], or [n_labels, C]
    tables with `labels`."""
    dims = tuple(range(1, x.dim()))
    mean = x.mean(dim=dims, keepdim=True)
    var = ((x - mean) ** 2).mean(dim=dims, keepdim=True)
    if labels is None:
        shp = [1, -1] + [1] * (x.dim() - 2)
        s, o = scale.reshape(shp), offset.reshape(shp)
    else:
        shp = [x.shape[0], -1] + [1] * (x.dim() - 2)
        s, o = scale[labels.long()].reshape(shp), offset[labels.long()].reshape(shp)
    return (x - mean) / torch.sqrt(var + eps) * s + o


_plain_normalize = onets.Normalize


def normalize(reg, cfg, name, inputs, labels=None):
    """oracle.nets.Normalize with the script's critic branch (:76-77): Layernorm(name, [1,2,3], inputs, labels=labels, n_labels=10),
    the labels having passed the two filters of :71-74."""
    if not cfg.CONDITIONAL:
        labels = None
    if cfg.CONDITIONAL and cfg.ACGAN and ('Discriminator' in name):
        labels = None
    if ('Discriminator' in name) and cfg.NORMALIZATION_D:
        return Layernorm(reg, name, [1, 2, 3], inputs, labels=labels, n_labels=10)
    return _plain_normalize(reg, cfg, name, inputs, labels=labels)
