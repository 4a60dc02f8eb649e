"""TEST-ONLY torch-CPU stand-ins (fp32 results, as the device gives) for the wrappers ctgan_amd.kernels gained with the 64x64 script's
architecture selector (csrc/bn_act.hip: ctgan_bn_act_{apply,bwd}, ctgan_gate_{fwd,bwd}).  Layered on tests/cpu_kernels.py by the fixture
`arch_cpu_kernels` below; nothing under ctgan_amd/ imports this file."""
import pytest
import torch

from tests import cpu_kernels as C

__all__ = ['bn_act_fwd', 'bn_act_bwd', 'gate_fwd', 'gate_bwd']


def _act(z, act, alpha):
    if act == 'lrelu':
        return torch.where(z > 0, z, alpha * z)
    if act == 'tanh':
        return torch.tanh(z)
    assert act == 'gate' and z.shape[1] % 2 == 0
    return torch.sigmoid(z[:, ::2]) * torch.tanh(z[:, 1::2])


def _dact(z, gy, act, alpha):
    """g = act'(z) gy, in z's shape (the gate's gy has half the channels)."""
    if act == 'lrelu':
        return torch.where(z > 0, gy, alpha * gy)
    if act == 'tanh':
        return gy * (1 - torch.tanh(z) ** 2)
    s, t = torch.sigmoid(z[:, ::2]), torch.tanh(z[:, 1::2])
    g = torch.empty_like(z)
    g[:, ::2] = gy * s * (1 - s) * t
    g[:, 1::2] = gy * s * (1 - t * t)
    return g


def _cl(t):
    return C._cl(t) if t.dim() == 4 else t.contiguous()


def bn_act_fwd(x, scale, offset, act, alpha, groups, eps=1e-5):
    z, mean, rstd, x4 = C.bn_fwd(x, scale.reshape(1, -1), offset.reshape(1, -1), None, groups, False, eps)
    return _cl(_act(z, act, alpha)), mean, rstd, x4


def bn_act_bwd(gy, x4, mean, rstd, scale, offset, act, alpha, groups):
    N, Cn, H, W = x4.shape
    per = N // groups
    mu = mean.repeat_interleave(per, 0)[:, :, None, None]
    rs = rstd.repeat_interleave(per, 0)[:, :, None, None]
    z = (x4 - mu) * rs * scale.reshape(1, -1, 1, 1) + offset.reshape(1, -1, 1, 1)
    g = _dact(z, gy.reshape(N, -1, H, W), act, alpha)
    gx, gs, go = C.bn_bwd(g, x4, mean, rstd, scale.reshape(1, -1), offset.reshape(1, -1), None, groups, False)
    return gx, gs.reshape(-1), go.reshape(-1)


def gate_fwd(x):
    return _cl(_act(x, 'gate', 0.0))


def gate_bwd(gy, x):
    return _cl(_dact(x, gy, 'gate', 0.0))


@pytest.fixture
def arch_cpu_kernels(cpu_kernels, monkeypatch):
    """cpu_kernels (tests/conftest.py) plus the stand-ins of this file and of the non-CT objectives (tests/test_gan_modes_host.py)."""
    import sys
    import ctgan_amd.kernels as K
    from tests import test_gan_modes_host as H
    mod = sys.modules[__name__]
    for name in __all__:
        monkeypatch.setattr(K, name, getattr(mod, name))
    for name, fn in (('rmsprop_step', H._rmsprop_step), ('rmsprop_step_packed', H._rmsprop_step_packed), ('gan_loss_fwd', H._gan_loss_fwd),
                     ('gan_loss_bwd', H._gan_loss_bwd)):
        monkeypatch.setattr(K, name, fn)
    yield mod
