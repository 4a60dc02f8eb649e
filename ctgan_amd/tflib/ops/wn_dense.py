"""tflib.ops.wn_dense - the weight-normalised dense layer and the Gaussian noise layer of the reference's Theano classifier
(TH/nn.py:398-430 `DenseLayer`, :232-244 `GaussianNoiseLayer`; TH/ = CT-GANs/Theano_classifier).  A separate operator: the
`weightnorm=` argument of Conv2D / Deconv2D / Linear (never enabled by the TF scripts) keeps raising.

`WNDense` computes  nonlinearity(inputs @ W + b)  with  W = theta * weight_scale / sqrt(column sums of theta^2)  (no epsilon, :407)
and, with `sigma` > 0, the GaussianNoiseLayer that follows it in the network - `+ sigma N(0,1)` - in the same launch
(functional.dense_noise).  Parameters: `name.theta` [in, out] ~ N(0, 0.1^2), `name.weight_scale` [out] = 1 (trainable only with
train_scale, :406), `name.b` [out] = 0.
"""
import numpy as np
import torch

from ... import functional as F
from ... import kernels as K
from .. import param as _param


def GaussianNoise(inputs, sigma, deterministic=False, rng=None, row_offset=0):
    """inputs + sigma N(0,1) (:238-244); the identity when deterministic or sigma == 0.  One random call site of `rng`; row_offset:
    the first row's position in that site's stream (a pass that is a row block of a larger stacked batch)."""
    if deterministic or sigma == 0:
        return inputs
    return F.dense_noise(inputs, None, False, sigma, F.noise_spec(rng), row_offset)


def WNDense(name, input_dim, output_dim, inputs, sigma=0.0, nonlinearity='relu', train_scale=False, init=False, deterministic=False, rng=None,
            row_offset=0, want_pre_noise=False, frozen=False):
    """nonlinearity: 'relu' | None.  init: the data-dependent initialisation pass (:421-426) - the pre-activation is centred and divided by
    its per-column root mean square over the batch before the nonlinearity, and weight_scale <- weight_scale / stdv, b <- -mean / stdv are
    written in place.  deterministic: no noise (and no random call site).  want_pre_noise: return (h, a) with a the activation before the
    noise.  frozen: the parameters enter as constants (a pass that only needs data gradients)."""
    if nonlinearity not in ('relu', None):
        raise Exception('WNDense: unsupported nonlinearity %r' % (nonlinearity,))
    relu = nonlinearity == 'relu'
    theta = _param(name + '.theta', lambda r: r.normal(0.0, 0.1, (input_dim, output_dim)).astype('float32'))
    scale = _param(name + '.weight_scale', lambda r: np.ones((output_dim,), dtype='float32'), trainable=bool(train_scale))
    b = _param(name + '.b', lambda r: np.zeros((output_dim,), dtype='float32'))
    noisy = sigma != 0 and not deterministic
    spec = F.noise_spec(rng) if noisy else None
    sig = sigma if noisy else 0.0
    if init:
        with torch.no_grad():
            y = F.linear(inputs, F.weight_norm(theta, scale, 0.0))
            K.wn_init(y, scale, b, relu)
            h = F.dense_noise(y, None, False, sig, spec, row_offset) if noisy else y
        return (h, y) if want_pre_noise else h
    if frozen:
        theta, scale, b = theta.detach(), scale.detach(), b.detach()
    w = F.weight_norm(theta, scale, 0.0)
    if not relu and not noisy and not want_pre_noise:
        return F.linear(inputs, w, b)
    return F.dense_noise(F.linear(inputs, w), b, relu, sig, spec, row_offset, want_pre_noise)
