"""TEST-ONLY fp32 torch-CPU stand-ins for the second-derivative attention wrappers of ctgan_amd.kernels (csrc/attention.hip: attention_bwd2,
attn_residual_bwd2, and attention_bwd_delta - attention_bwd that also hands out its row scratch), layered on tests/attention_cpu_kernels.py.
The arithmetic is DESIGN 33's formulas in float32, tile-free, with the [n, N, N] quantities materialised; two calls on the same inputs agree bit
for bit.  Nothing under ctgan_amd/ imports this file."""
import pytest
import torch

from tests import attention_cpu_kernels as AK
from tests.attention_cpu_kernels import attention_kernels        # noqa: F401  (fixture)

__all__ = ['attention_bwd_delta', 'attention_bwd2', 'attn_residual_bwd2']

CALLS = AK.CALLS          # one list with the first-order stand-ins: (name, shapes, flag) of every launch since the fixture started


def attention_bwd_delta(q, k, v, out, lse, gout):
    with torch.no_grad():
        return tuple(AK.attention_bwd(q, k, v, out, lse, gout)) + ((gout * out).sum(dim=2),)


def attention_bwd2(q, k, v, lse, delta, gout, a, b, c):
    with torch.no_grad():
        CALLS.append(('attention_bwd2', AK._check(q, k, v), True))
        for t, like in ((gout, v), (a, q), (b, k), (c, v)):
            assert t.is_contiguous() and t.shape == like.shape and t.dtype == torch.float32
        assert tuple(lse.shape) == tuple(delta.shape) == tuple(q.shape[:2])
        kt, vt = k.transpose(1, 2), v.transpose(1, 2)
        P = torch.exp(q @ kt - lse.unsqueeze(2))
        dP = gout @ vt
        dl = delta.unsqueeze(2)
        T = a @ kt + q @ b.transpose(1, 2)
        tau = (P * T).sum(dim=2, keepdim=True)
        Pc = P @ c
        rho = (P * T * dP).sum(dim=2, keepdim=True) - 2 * tau * dl + (gout * Pc).sum(dim=2, keepdim=True)
        W = P * (T - tau)
        Sbar = P * (T * dP - dP * tau - T * dl + gout @ c.transpose(1, 2) - rho)
        dS = P * (dP - dl)
        return Sbar @ k + dS @ b, Sbar.transpose(1, 2) @ q + dS.transpose(1, 2) @ a, W.transpose(1, 2) @ gout, W @ v + Pc


def attn_residual_bwd2(gy, o, gamma, cgo, cgg=None):
    with torch.no_grad():
        assert gamma.numel() == 1 and gy.shape == o.shape == cgo.shape and (cgg is None or cgg.numel() == 1)
        CALLS.append(('attn_residual_bwd2', tuple(o.shape), cgg is not None))
        g = gamma.reshape(())
        dgamma = (cgo.double() * gy.double()).sum().to(torch.float32).reshape(1)
        if cgg is None:
            return g * cgo, None, dgamma
        s = cgg.reshape(())
        return g * cgo + s * o, s * gy, dgamma


@pytest.fixture
def attention2_kernels(attention_kernels, monkeypatch):        # noqa: F811
    """attention_kernels (cpu_kernels, the RMSProp / GAN-loss and the first-order attention stand-ins) plus the stand-ins of this file."""
    import sys
    import ctgan_amd.kernels as K
    mod = sys.modules[__name__]
    for name in __all__:
        monkeypatch.setattr(K, name, getattr(mod, name))
    yield attention_kernels
