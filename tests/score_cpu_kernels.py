"""TEST-ONLY torch-CPU stand-ins (fp32 results, as the device gives) for the wrappers ctgan_amd.kernels gained with the score classifier
(csrc/score.hip and the moving-statistics / blend / fused-apply entry points of csrc/bn.hip).  Layered on tests/cpu_kernels.py by the
fixture of tests/test_score_mnist_host.py; nothing under ctgan_amd/ imports this file."""
import torch

from tests import cpu_kernels as C

__all__ = ['bn_stats_moving', 'bn_blend_stats', 'bn_apply_ex', 'bn_bwd_scaled', 'elu_fwd', 'elu_bwd', 'global_norm', 'clip_by_norm_', 'conv_wgrad']


def _x4(x):
    return C.to_channels_last(x if x.dim() == 4 else x.reshape(x.shape[0], x.shape[1], 1, 1))


def bn_stats_moving(x, eps=1e-5, moving_mean=None, moving_var=None, it=None):
    x4 = _x4(x)
    N, Cc, H, W = x4.shape
    xd = x4.double()
    mean = xd.mean(dim=(0, 2, 3))
    var = ((xd * xd).mean(dim=(0, 2, 3)) - mean * mean).clamp_min(0)
    rstd = (1.0 / torch.sqrt(var + eps)).float()
    if moving_mean is not None:
        cnt = N * H * W
        bm, bv = mean.float(), (var * (cnt / max(cnt - 1, 1))).float()
        fi = it.reshape(()).float()
        wa, wb = fi / (fi + 1.), 1. / (fi + 1.)
        moving_mean.copy_(wa * moving_mean + wb * bm)
        moving_var.copy_(wa * moving_var + wb * bv)
    return mean.float().view(1, Cc), rstd.view(1, Cc), x4


def bn_blend_stats(x, moving_mean, moving_var, eps=1e-5):
    x4 = _x4(x)
    N = x4.shape[0]
    xd = x4.double()
    m = xd.mean(dim=(2, 3))
    v = ((xd * xd).mean(dim=(2, 3)) - m * m).clamp_min(0)
    B = torch.tensor(float(N))
    wa, wb = 1. / B, (B - 1.) / B
    mean = wa * m.float() + wb * moving_mean[None, :]
    var = wa * v.float() + wb * moving_var[None, :]
    return mean, (1.0 / torch.sqrt(var.double() + eps)).float(), x4


def bn_apply_ex(x4, mean, rstd, scale, offset, shortcut=None, alpha=1.0, relu=False, want_elu=False):
    y = (x4 - mean[:, :, None, None]) * rstd[:, :, None, None] * scale.reshape(1, -1, 1, 1) + offset.reshape(1, -1, 1, 1)
    if relu:
        y = torch.relu(y)
    y = alpha * y if shortcut is None else shortcut + alpha * y
    y = C._cl(y)
    return y, (elu_fwd(y) if want_elu else None)


def bn_bwd_scaled(gy, x4, mean, rstd, scale, offset, gy_scale):
    return C.bn_bwd(gy * gy_scale, x4, mean, rstd, scale.reshape(1, -1), offset.reshape(1, -1), None, 1, False)


def elu_fwd(x):
    return torch.where(x > 0, x, torch.expm1(torch.clamp(x, max=0)))


def elu_bwd(gy, y, add=None):
    gx = torch.where(y > 0, gy, gy * (y + 1.))
    return gx if add is None else add + gx


def global_norm(flat, out=None):
    n = torch.sqrt((flat.double() ** 2).sum()).float().reshape(1)
    if out is not None:
        out.copy_(n)
        return out
    return n


def clip_by_norm_(flat, norm, clip):
    return flat.mul_(torch.tensor(float(clip), dtype=torch.float32) / torch.clamp(norm.reshape(()), min=float(clip)))


def conv_wgrad(x, gy, g, with_bias=False, relu_x=False, out=None):
    """tests/cpu_kernels.conv_wgrad, except for strided 1x1 convs (the network's 'down' shortcuts): torch's CPU convolution backward
    crashes on that shape with channels-last operands here, so the weight gradient is taken as the plain contraction it is."""
    if not (g.R == 1 and g.S == 1 and g.stride > 1 and not g.x_up):
        return C.conv_wgrad(x, gy, g, with_bias, relu_x, out)
    xs = (torch.relu(x) if relu_x else x)[:, :, ::g.stride, ::g.stride]
    gw = torch.einsum('ncpq,nkpq->ck', xs, gy).reshape(1, 1, g.C, g.K).contiguous()
    gb = gy.sum(dim=(0, 2, 3)) if with_bias else None
    if out is not None:
        out[0].copy_(gw)
        if with_bias:
            out[1].copy_(gb)
        gw, gb = out[0], out[1]
    return (gw, gb) if with_bias else gw
