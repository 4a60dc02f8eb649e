"""TEST-ONLY torch-CPU stand-in for kernels.diffaug (csrc/diffaug.hip), layered on the stand-ins the fixture `mode_kernels` installs
(tests/cpu_kernels.py, the RMSProp / GAN-loss ones of tests/test_gan_modes_host.py).  The draws are the device's (oracle/philox.py restates
the Philox streams in numpy, tests/diffaug_oracle.params the kernel's float32 expressions); the arithmetic is tests/diffaug_oracle's in
float32, so two calls on the same inputs and the same (seed, stream, step) agree bit for bit - which is what the host tests compare.
Nothing under ctgan_amd/ imports this file."""
import pytest
import torch

from tests import diffaug_oracle as O
from tests.test_gan_modes_host import mode_kernels        # noqa: F401  (fixture)

__all__ = ['diffaug']

CALLS = []          # (stream id, policy mask, adjoint) of every stand-in launch since the fixture started


def _step_of(ctr):
    return 0 if ctr is None else int(ctr.reshape(-1)[0].item())


def diffaug(x, shape, policy, spec, adjoint=False, denom=None, params=None, out=None):
    import ctgan_amd.kernels as K
    c, h, w = (int(v) for v in shape)
    n = x.shape[0]
    assert x.is_contiguous() and x.numel() == n * c * h * w
    policy = int(policy)
    nobright = bool(policy & K.DIFFAUG_NO_BRIGHTNESS)
    policy &= ~K.DIFFAUG_NO_BRIGHTNESS
    assert 0 <= policy <= 7
    if x.dtype == torch.int32:
        assert denom is not None and not adjoint
        x = 2. * ((x.to(torch.float32) / denom) - .5)          # tests/cpu_kernels.real_prep's line
    else:
        assert x.dtype == torch.float32 and denom is None
    seed, sid, ctr = spec
    assert 0 <= int(sid) <= 0xffffffff
    CALLS.append((int(sid), policy, bool(adjoint)))
    p = O.params(seed, sid, _step_of(ctr), n, h, w, policy)
    flat = x.reshape(n, c * h * w)
    if adjoint:
        y = O.adjoint(flat, (c, h, w), p, dtype=torch.float32)
    else:
        y = O.forward(flat, (c, h, w), p, brightness=not nobright, dtype=torch.float32)
    y = y.reshape(x.shape)
    if params is not None:
        params.copy_(torch.from_numpy(O.params_table(p, policy)))
    if out is not None:
        out.copy_(y)
        return out
    return y


@pytest.fixture
def diffaug_kernels(mode_kernels, monkeypatch):        # noqa: F811
    """mode_kernels (cpu_kernels + the RMSProp / GAN-loss stand-ins) plus the stand-in of this file."""
    import sys
    import ctgan_amd.kernels as K
    mod = sys.modules[__name__]
    for name in __all__:
        monkeypatch.setattr(K, name, getattr(mod, name))
    del CALLS[:]
    yield mode_kernels
    del CALLS[:]
