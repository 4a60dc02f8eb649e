"""Self-attention block of SAGAN / BigGAN (Zhang et al., ICML 2019; NOT in the reference) on the fused fp32 kernel of csrc/attention.hip.

    SelfAttention(name, dim, x) = x + gamma * Out(attention(Query(x), Key(x), Value(x)))

over the N = H W positions of a channels-last [n, dim, H, W] tensor - the BigGAN form without the pooling, no 1 / sqrt(dk) scale.  The
four 1x1 projections are ordinary Conv2D operators (they follow kernels.MMA_DTYPE like every conv); the core softmax(q k^T) v is ONE
launch forward and two backward that never write the [n, N, N] scores, always on the exact-fp32 MFMA.

AttentionFn and AttnResidualFn are first order only: their backwards call kernels directly, so a second differentiation raises
(functional._once).  Attention2Fn and AttnResidual2Fn (attention2, attn_residual2, SelfAttention(..., second_order=True)) are the same
launches with a first backward that is itself a Function (AttentionBwdFn, AttnResidualBwdFn) on the second-derivative kernels
(kernels.attention_bwd2 / attn_residual_bwd2): the gradient penalty of the CT objective can stand behind those
(gan_cifar_resnet.Config.ATTENTION_SECOND_ORDER).  They all live here, not in functional.py, whose Function classes
tests/autograd_orders_cases.py enumerates.
"""
import numpy as np
import torch
from torch.autograd import Function

from . import functional as F
from . import kernels as K
from . import tflib as lib
from .tflib.ops import conv2d as _conv2d


def _rows(t):
    return t if t.is_contiguous() else t.contiguous()


class AttentionFn(Function):
    """out [n, N, dv] = softmax(q k^T) v per image over dense rows q, k [n, N, dk], v [n, N, dv] (kernels.attention_fwd / attention_bwd)."""

    @staticmethod
    def forward(ctx, q, k, v):
        q, k, v = _rows(q), _rows(k), _rows(v)
        need = any(ctx.needs_input_grad)
        out, lse = K.attention_fwd(q, k, v, want_lse=need)
        if need:
            ctx.save_for_backward(q, k, v, out, lse)
        return out

    @staticmethod
    @F._once
    def backward(ctx, gout):
        q, k, v, out, lse = ctx.saved_tensors
        gq, gk, gv = K.attention_bwd(q, k, v, out, lse, _rows(gout))
        return gq, gk, gv


class AttnResidualFn(Function):
    """y = x + gamma * o with the one-element gate read on the device (kernels.attn_residual_fwd / attn_residual_bwd)."""

    @staticmethod
    def forward(ctx, x, o, gamma):
        ctx.save_for_backward(o, gamma)
        return K.attn_residual_fwd(x, o, gamma)

    @staticmethod
    @F._once
    def backward(ctx, gy):
        o, gamma = ctx.saved_tensors
        go, ggamma = K.attn_residual_bwd(gy, o, gamma)
        return gy, go, ggamma.reshape(gamma.shape)


def attention(q, k, v):
    """softmax(q k^T) v over dense rows [n, N, d]; under no_grad the row statistics are not written."""
    return AttentionFn.apply(q, k, v)


def attn_residual(x, o, gamma):
    return AttnResidualFn.apply(x, o, gamma)


# ---- the twice-differentiable operators: the same forward launches; the first backward is itself a Function ------------------
def _or_zeros(g, like):
    return torch.zeros_like(like) if g is None else _rows(g)


class Attention2Fn(Function):
    """AttentionFn whose backward is AttentionBwdFn: the gradient penalty of the CT objective may stand behind it."""

    @staticmethod
    def forward(ctx, q, k, v):
        q, k, v = _rows(q), _rows(k), _rows(v)
        need = any(ctx.needs_input_grad)
        out, lse = K.attention_fwd(q, k, v, want_lse=need)
        if need:
            ctx.save_for_backward(q, k, v, out, lse)
        return out

    @staticmethod
    def backward(ctx, gout):
        q, k, v, out, lse = ctx.saved_tensors
        return AttentionBwdFn.apply(q, k, v, gout, out.detach(), lse.detach())


class AttentionBwdFn(Function):
    """(q, k, v, gout) -> (gq, gk, gv): the launches of kernels.attention_bwd.  out, lse and delta ride along detached - they are functions
    of q, k, v, and the backward (kernels.attention_bwd2) is the TOTAL derivative, so their slots get None.  A third differentiation is
    refused (functional._once)."""

    @staticmethod
    def forward(ctx, q, k, v, gout, out, lse):
        gout = _rows(gout)
        gq, gk, gv, delta = K.attention_bwd_delta(q, k, v, out, lse, gout)
        ctx.save_for_backward(q, k, v, gout, lse, delta)
        ctx.set_materialize_grads(False)
        return gq, gk, gv

    @staticmethod
    @F._once
    def backward(ctx, a, b, c):
        if a is None and b is None and c is None:
            return None, None, None, None, None, None
        q, k, v, gout, lse, delta = ctx.saved_tensors
        dq, dk, dv, dgout = K.attention_bwd2(q, k, v, lse, delta, gout, _or_zeros(a, q), _or_zeros(b, k), _or_zeros(c, v))
        return dq, dk, dv, dgout, None, None


class AttnResidual2Fn(Function):
    """AttnResidualFn whose backward is AttnResidualBwdFn (the gradient of x is gy itself: autograd's own identity)."""

    @staticmethod
    def forward(ctx, x, o, gamma):
        ctx.save_for_backward(o, gamma)
        return K.attn_residual_fwd(x, o, gamma)

    @staticmethod
    def backward(ctx, gy):
        o, gamma = ctx.saved_tensors
        go, ggamma = AttnResidualBwdFn.apply(gy, o, gamma)
        return gy, go, ggamma.reshape(gamma.shape)


class AttnResidualBwdFn(Function):
    """(gy, o, gamma) -> (go = gamma gy, ggamma [1] = sum gy o): the launches of kernels.attn_residual_bwd; its backward is
    kernels.attn_residual_bwd2.  A third differentiation is refused (functional._once)."""

    @staticmethod
    def forward(ctx, gy, o, gamma):
        go, ggamma = K.attn_residual_bwd(gy, o, gamma)
        ctx.save_for_backward(gy, o, gamma)
        ctx.set_materialize_grads(False)
        return go, ggamma

    @staticmethod
    @F._once
    def backward(ctx, cgo, cgg):
        if cgo is None and cgg is None:
            return None, None, None
        gy, o, gamma = ctx.saved_tensors
        dgy, d_o, dgamma = K.attn_residual_bwd2(gy, o, gamma, torch.zeros_like(o) if cgo is None else cgo, cgg)
        return dgy, d_o, dgamma.reshape(gamma.shape)


def attention2(q, k, v):
    """attention(q, k, v), the same launches and bits, differentiable twice (the second time on kernels.attention_bwd2)."""
    return Attention2Fn.apply(q, k, v)


def attn_residual2(x, o, gamma):
    """attn_residual(x, o, gamma), the same launches and bits, differentiable twice (kernels.attn_residual_bwd2)."""
    return AttnResidual2Fn.apply(x, o, gamma)


PARAMS = ('Query.Filters', 'Key.Filters', 'Value.Filters', 'Out.Filters', 'gamma')     # of one block, in creation order


def _tokens(t):
    """Logical [n, c, H, W] (channels-last) -> its rows [n, H W, c]: a view of a channels-last tensor."""
    n, c, h, w = t.shape
    return t.permute(0, 2, 3, 1).reshape(n, h * w, c)


def SelfAttention(name, dim, x, second_order=False):
    """x [n, dim, H, W] -> x + gamma * Out(softmax(Query(x) Key(x)^T) Value(x)).  Parameters, created at first use in this order:
    name.Query.Filters, name.Key.Filters (1x1, dim -> dim // 8), name.Value.Filters (dim -> dim // 2), name.Out.Filters (dim // 2 -> dim) -
    no biases, he_init=False - and name.gamma [1] = 0: a fresh block is the identity.  second_order: the core and the residual are
    attention2 / attn_residual2 - the same parameters, launches and bits, differentiable twice."""
    n, c, h, w = x.shape
    assert c == dim, 'SelfAttention: %d channels, dim = %d' % (c, dim)
    dk, dv = dim // 8, dim // 2
    q = _conv2d.Conv2D(name + '.Query', dim, dk, 1, x, he_init=False, biases=False)
    k = _conv2d.Conv2D(name + '.Key', dim, dk, 1, x, he_init=False, biases=False)
    v = _conv2d.Conv2D(name + '.Value', dim, dv, 1, x, he_init=False, biases=False)
    o = (attention2 if second_order else attention)(_tokens(q), _tokens(k), _tokens(v))
    o = o.reshape(n, h, w, dv).permute(0, 3, 1, 2)
    o = _conv2d.Conv2D(name + '.Out', dv, dim, 1, o, he_init=False, biases=False)
    gamma = lib.param(name + '.gamma', lambda rng: np.zeros(1, dtype='float32'))
    return (attn_residual2 if second_order else attn_residual)(x, o, gamma)
