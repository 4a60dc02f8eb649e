"""TEST-ONLY fp32 torch-CPU stand-ins for the attention wrappers of ctgan_amd.kernels (csrc/attention.hip), layered on the stand-ins the
fixture `mode_kernels` installs (tests/cpu_kernels.py, the RMSProp / GAN-loss ones of tests/test_gan_modes_host.py).  The arithmetic is the
kernel's formulas in float32 with the scores materialised; two calls on the same inputs agree bit for bit.  Nothing under ctgan_amd/ imports
this file."""
import pytest
import torch

from tests.test_gan_modes_host import mode_kernels        # noqa: F401  (fixture)

__all__ = ['attention_fwd', 'attention_bwd', 'attn_residual_fwd', 'attn_residual_bwd']

CALLS = []          # (name, shapes, want_lse) of every stand-in launch since the fixture started


def _check(q, k, v):
    n, N, dk = q.shape
    dv = v.shape[2]
    assert q.is_contiguous() and k.is_contiguous() and v.is_contiguous() and q.dtype == torch.float32
    assert tuple(k.shape) == (n, N, dk) and tuple(v.shape) == (n, N, dv)
    if N % 16 or N < 16:
        raise ValueError('attention: N = %d tokens' % N)
    if dk % 4 or not 4 <= dk <= 64:
        raise ValueError('attention: dk = %d' % dk)
    if dv % 16 or not 16 <= dv <= 128:
        raise ValueError('attention: dv = %d' % dv)
    return n, N, dk, dv


def attention_fwd(q, k, v, want_lse=True):
    with torch.no_grad():
        CALLS.append(('attention_fwd', _check(q, k, v), bool(want_lse)))
        s = q @ k.transpose(1, 2)
        m = s.max(dim=2, keepdim=True).values
        p = torch.exp(s - m)
        l = p.sum(dim=2, keepdim=True)
        out = (p @ v) / l
        return out, ((m + torch.log(l)).squeeze(2) if want_lse else None)


def attention_bwd(q, k, v, out, lse, gout):
    with torch.no_grad():
        CALLS.append(('attention_bwd', _check(q, k, v), True))
        assert gout.is_contiguous() and gout.shape == out.shape == v.shape and tuple(lse.shape) == tuple(q.shape[:2])
        p = torch.exp(q @ k.transpose(1, 2) - lse.unsqueeze(2))
        delta = (gout * out).sum(dim=2, keepdim=True)
        ds = p * (gout @ v.transpose(1, 2) - delta)
        return ds @ k, ds.transpose(1, 2) @ q, p.transpose(1, 2) @ gout


def attn_residual_fwd(x, o, gamma):
    with torch.no_grad():
        assert gamma.numel() == 1 and x.shape == o.shape
        CALLS.append(('attn_residual_fwd', tuple(x.shape), False))
        return x + gamma.reshape(()) * o


def attn_residual_bwd(gy, o, gamma):
    with torch.no_grad():
        assert gamma.numel() == 1 and gy.shape == o.shape
        CALLS.append(('attn_residual_bwd', tuple(o.shape), False))
        return gamma.reshape(()) * gy, (gy.double() * o.double()).sum().to(torch.float32).reshape(1)


@pytest.fixture
def attention_kernels(mode_kernels, monkeypatch):        # noqa: F811
    """mode_kernels (cpu_kernels + the RMSProp / GAN-loss stand-ins) plus the stand-ins of this file."""
    import sys
    import ctgan_amd.kernels as K
    mod = sys.modules[__name__]
    for name in __all__:
        monkeypatch.setattr(K, name, getattr(mod, name))
    del CALLS[:]
    yield mode_kernels
    del CALLS[:]
