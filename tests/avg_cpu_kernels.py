"""TEST-ONLY torch-CPU stand-ins for what ctgan_amd.kernels gained with the generator's weight average (csrc/optim_rng.hip: the `_avg`
forms of the four update launches, ctgan_exchange).  Layered on the stand-ins that are installed when the fixture `avg_kernels` below runs
(tests/cpu_kernels.py through `cpu_kernels`, the RMSProp ones of tests/test_gan_modes_host.py through `mode_kernels`): each update
stand-in here calls the one it replaces with that one's own argument list, then moves the average as the device does - avg <- avg +
rate * (theta - avg) in fp32, one rounding per operation (separate torch ops: no fused multiply-add).  Nothing under ctgan_amd/ imports
this file."""
import pytest
import torch

from tests.test_gan_modes_host import mode_kernels        # noqa: F401  (fixture)

__all__ = ['adam_step', 'adam_step_packed', 'rmsprop_step', 'rmsprop_step_packed', 'exchange_']

_BASE = {}          # name -> the stand-in this file's wrapper replaced (set by the fixture)


def move_average(avg, theta, rate):
    """The averaging line of the update kernels on whole tensors, in place."""
    assert avg.dtype == theta.dtype == torch.float32 and avg.shape == theta.shape and 0.0 < rate <= 1.0
    rate = torch.tensor(rate, dtype=torch.float32)
    avg.copy_(avg + rate * (theta - avg))


def _with_average(name):
    def step(*args, avg=None, avg_rate=0.0, **kw):
        _BASE[name](*args, **kw)
        if avg is not None:
            theta = args[4] if name.endswith('_packed') else args[0]
            move_average(avg, theta, float(avg_rate))
    step.__name__ = name
    return step


adam_step = _with_average('adam_step')
adam_step_packed = _with_average('adam_step_packed')
rmsprop_step = _with_average('rmsprop_step')
rmsprop_step_packed = _with_average('rmsprop_step_packed')


def exchange_(a, b):
    assert a.dtype == b.dtype == torch.float32 and a.is_contiguous() and b.is_contiguous() and a.numel() == b.numel()
    t = a.clone()
    a.copy_(b)
    b.copy_(t)


@pytest.fixture
def avg_kernels(mode_kernels, monkeypatch):        # noqa: F811
    """mode_kernels (cpu_kernels + the RMSProp / GAN-loss stand-ins) plus the stand-ins of this file."""
    import sys
    import ctgan_amd.kernels as K
    mod = sys.modules[__name__]
    for name in __all__:
        if name != 'exchange_':
            monkeypatch.setitem(_BASE, name, getattr(K, name, None))
        monkeypatch.setattr(K, name, getattr(mod, name))
    yield mode_kernels
