"""tflib.ops.wn_conv - the weight-normalised conv, transposed-conv, NIN and dense layers of the reference's convolutional Theano
classifier (TH/nn.py:49-104 `WeightNormLayer` / `weight_norm` around dnn.Conv2DDNNLayer, nn.Deconv2DLayer, ll.NINLayer and
ll.DenseLayer; TH/ = CT-GANs/Theano_classifier).  Separate operators: the `weightnorm=` argument of Conv2D / Deconv2D / Linear (never
enabled by the TF scripts) keeps raising.

Every layer computes  nonlinearity(op(inputs, W) + b)  with  W = W_param * g / sqrt(1e-6 + sum of W_param^2 per OUTPUT channel)
(:81).  Parameters: `name.W` ~ N(0, 0.05^2) in this project's filter layouts (HWIO for a conv, [k, k, out, in] for a transposed conv,
[in, out] for NIN / dense), `name.g` [out] = 1 (trainable only with train_g, :59), `name.b` [out] = 0.  The convs are this project's
TF-SAME kernels: ct_cifar.py runs the Theano network in coordinates rotated by 180 degrees, in which its `pad=1` strided convs and
`border_mode='half'` transposed convs ARE the SAME ones (see its docstring), and states the relabelling of the parameters.

Common arguments - init: the data-dependent initialisation pass (:85-91): the pre-activation WITHOUT b is centred per channel over
(n, h, w), multiplied by init_stdv / its root mean square, and  g <- g inv_stdv,  b <- -mean inv_stdv  are written in place (one
launch, kernels.wn_init_map).  deterministic: no dropout (and no random call site).  frozen: the parameters enter as constants (a
pass that only needs data gradients).  rng: the DeviceRNG the dropout site is numbered from.
"""
import numpy as np
import torch

from ... import functional as F
from ... import kernels as K
from .. import param as _param

W_STD = 0.05            # lasagne.init.Normal(0.05) on every layer of TH/CT_CIFAR.py:72-93
WN_EPS = 1e-6           # TH/nn.py:81
LRELU_SLOPE = 0.2       # TH/nn.py lrelu


_CONST = None            # inside constant_filters(store): the store


class constant_filters:
    """with constant_filters(store): every WNConv2D / WNNIN / WNLinear layer outside its init pass takes its normalised filter from
    the dict `store` (layer name -> tensor), made by the layer's own normalisation launch the first time and kept there - the same
    values a pass outside the context computes, so its results are bit-equal.  For passes whose W and g do not change between calls
    (score_cifar.ClassifierScore, which owns the store and empties it when the classifier's parameters move); no gradients."""

    def __init__(self, store):
        self.store = store

    def __enter__(self):
        global _CONST
        self.old, _CONST = _CONST, self.store

    def __exit__(self, *a):
        global _CONST
        _CONST = self.old
        return False


def _normalised(name, make):
    if _CONST is None:
        return make()
    if torch.is_grad_enabled():
        raise RuntimeError('wn_conv.constant_filters: %s is being built with gradients enabled - the stored filters are constants' % name)
    if name not in _CONST:
        with torch.no_grad():
            _CONST[name] = make().detach()
    return _CONST[name]


def _normal(shape):
    return lambda r: r.normal(0.0, W_STD, shape).astype('float32')


def _gb(name, output_dim, train_g):
    g = _param(name + '.g', lambda r: np.ones((output_dim,), dtype='float32'), trainable=bool(train_g))
    b = _param(name + '.b', lambda r: np.zeros((output_dim,), dtype='float32'))
    return g, b


def _act(y, nonlinearity, drop_keep, deterministic, rng):
    """nonlinearity (+ the DropoutLayer that follows the layer in the network, in the same launch)."""
    keep = 1.0 if deterministic else float(drop_keep)
    if nonlinearity == 'lrelu':
        return F.lrelu_dropout(y, LRELU_SLOPE, keep, rng)
    if nonlinearity == 'tanh':
        y = F.tanh(y)
    return F.dropout(y, keep, rng=rng)


def _check(nonlinearity):
    if nonlinearity not in ('lrelu', 'tanh', None):
        raise Exception('unsupported nonlinearity %r' % (nonlinearity,))


def _init_map(y, g, b, nonlinearity, init_stdv):
    if not y.permute(0, 2, 3, 1).is_contiguous():
        y = K.to_channels_last(y)
    return K.wn_init_map(y, g, b, nonlinearity, LRELU_SLOPE, init_stdv)


def WNConv2D(name, input_dim, output_dim, filter_size, inputs, stride=1, pad='same', nonlinearity='lrelu', drop_keep=1.0, train_g=False,
             init_stdv=1.0, init=False, deterministic=False, frozen=False, rng=None):
    """inputs [n, input_dim, H, W] -> [n, output_dim, ceil(H / stride), ceil(W / stride)]; pad=0 (stride 1, odd filter): the valid conv,
    [n, output_dim, H - k + 1, W - k + 1] - the centre of the SAME result.  drop_keep < 1: dropout(keep) after the nonlinearity."""
    _check(nonlinearity)
    if pad not in ('same', 0) or (pad == 0 and (stride != 1 or filter_size % 2 != 1)):
        raise Exception('WNConv2D: pad is "same", or 0 with stride 1 and an odd filter')
    W = _param(name + '.W', _normal((filter_size, filter_size, input_dim, output_dim)))
    g, b = _gb(name, output_dim, train_g)

    def valid(y):
        if pad == 'same':
            return y
        m = filter_size // 2
        return F.crop(y, y.shape[2] - 2 * m, y.shape[3] - 2 * m, m, m)

    if init:
        with torch.no_grad():
            y = valid(F.conv2d(inputs, F.weight_norm_filter(W, g, WN_EPS), None, stride=stride))
            y = _init_map(y, g, b, nonlinearity, init_stdv)
            return F.dropout(y, 1.0 if deterministic else float(drop_keep), rng=rng)
    if frozen:
        W, g, b = W.detach(), g.detach(), b.detach()
    y = valid(F.conv2d(inputs, _normalised(name, lambda: F.weight_norm_filter(W, g, WN_EPS)), b, stride=stride))
    return _act(y, nonlinearity, drop_keep, deterministic, rng)


def WNNIN(name, input_dim, output_dim, inputs, nonlinearity='lrelu', drop_keep=1.0, train_g=False, init_stdv=1.0, init=False,
          deterministic=False, frozen=False, rng=None):
    """ll.NINLayer: a 1x1 conv on [n, input_dim, H, W]."""
    _check(nonlinearity)
    W = _param(name + '.W', _normal((input_dim, output_dim)))
    g, b = _gb(name, output_dim, train_g)
    if init:
        with torch.no_grad():
            y = F.conv2d(inputs, F.weight_norm(W, g, WN_EPS).view(1, 1, input_dim, output_dim))
            y = _init_map(y, g, b, nonlinearity, init_stdv)
            return F.dropout(y, 1.0 if deterministic else float(drop_keep), rng=rng)
    if frozen:
        W, g, b = W.detach(), g.detach(), b.detach()
    y = F.conv2d(inputs, _normalised(name, lambda: F.weight_norm(W, g, WN_EPS).view(1, 1, input_dim, output_dim)), b)
    return _act(y, nonlinearity, drop_keep, deterministic, rng)


def WNLinear(name, input_dim, output_dim, inputs, nonlinearity=None, train_g=False, init_stdv=1.0, init=False, deterministic=False,
             frozen=False, rng=None):
    """ll.DenseLayer under weight_norm on [n, input_dim]: the pattern of wn_dense.WNDense with the epsilon of TH/nn.py:81 and init_stdv."""
    _check(nonlinearity)
    W = _param(name + '.W', _normal((input_dim, output_dim)))
    g, b = _gb(name, output_dim, train_g)
    if init:
        with torch.no_grad():
            y = F.linear(inputs, F.weight_norm(W, g, WN_EPS)).contiguous()
            return K.wn_init_map(y, g, b, nonlinearity, LRELU_SLOPE, init_stdv)
    if frozen:
        W, g, b = W.detach(), g.detach(), b.detach()
    y = F.linear(inputs, _normalised(name, lambda: F.weight_norm(W, g, WN_EPS)), b)
    return _act(y, nonlinearity, 1.0, deterministic, rng)


def WNDeconv2D(name, input_dim, output_dim, filter_size, inputs, nonlinearity='tanh', train_g=False, init_stdv=1.0, init=False,
               deterministic=False, frozen=False, rng=None):
    """nn.Deconv2DLayer under weight_norm: [n, input_dim, H, W] -> [n, output_dim, 2H, 2W], stride 2; the norm of the [k, k, out, in]
    filter runs over (k, k, in) per output channel (TH/nn.py:71-73: axes (0, 2, 3) of W [in, out, k, k])."""
    _check(nonlinearity)
    W = _param(name + '.W', _normal((filter_size, filter_size, output_dim, input_dim)))
    g, b = _gb(name, output_dim, train_g)
    if init:
        with torch.no_grad():
            y = F.conv2d_transpose(inputs, F.weight_norm_mid(W, g, WN_EPS), None, stride=2)
            return _init_map(y, g, b, nonlinearity, init_stdv)
    if frozen:
        W, g, b = W.detach(), g.detach(), b.detach()
    y = F.conv2d_transpose(inputs, F.weight_norm_mid(W, g, WN_EPS), b, stride=2)
    return _act(y, nonlinearity, 1.0, deterministic, rng)
