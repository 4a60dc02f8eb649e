"""TEST-ONLY torch-CPU stand-ins (fp32 results, as the device gives) for the wrappers ctgan_amd.kernels gained with the hinge objective
(csrc/loss.hip: ctgan_gan_loss_* kinds 4 and 5, ctgan_tail_hinge_heads_fwd/bwd; csrc/optim_rng.hip: ctgan_real_fake_prep).  Layered on
tests/cpu_kernels.py, the projection / conditional-Layernorm / spectral-normalisation stand-ins and the DiffAugment one by the fixture `hinge_cpu_kernels` below; nothing
under ctgan_amd/ imports this file.

The hinge is t >= 0 ? t : 0 (the project's tie rule, tests/loss_heads_cases.py): its derivative at t == 0 is 1.  With a table of zeros the
projected head has the plain head's bits (w + 0.0 is exact)."""
import pytest
import torch

from tests import cpu_kernels as C
from tests.spectral_cpu_kernels import (avg_kernels, cond_cpu_kernels, mode_kernels, projection_cpu_kernels, scale_kernels,  # noqa: F401
                                        spectral_cpu_kernels)                                                         # (fixtures the one below builds on)

__all__ = ['gan_loss_fwd', 'gan_loss_bwd', 'real_fake_prep', 'tail_hinge_heads_fwd', 'tail_hinge_heads_bwd']


def _hinge(t):
    return torch.where(t >= 0, t, torch.zeros_like(t))


def _on(t):
    return (t >= 0).to(t.dtype)


def gan_loss_fwd(d, B, kind):
    if kind < 4:
        from tests import test_gan_modes_host as M
        return M._gan_loss_fwd(d, B, kind)
    d = d.detach()
    assert kind in (4, 5) and d.numel() == (2 * B if kind == 4 else B)
    if kind == 4:
        return _hinge(1.0 - d[:B]).mean() + _hinge(1.0 + d[B:]).mean()
    return -d.mean()


def gan_loss_bwd(d, gout, B, kind):
    if kind < 4:
        from tests import test_gan_modes_host as M
        return M._gan_loss_bwd(d, gout, B, kind)
    d = d.detach()
    g = gout.reshape(()) / B
    if kind == 4:
        return torch.cat([-g * _on(1.0 - d[:B]), g * _on(1.0 + d[B:])])
    return (-g).expand(B).contiguous()


def real_fake_prep(x_int, fake, seed, sid_deq, ctr, lo, hi, denom):
    B, d = x_int.shape
    assert d % 4 == 0 and x_int.dtype == torch.int32 and tuple(fake.shape) == (B, d)
    deq = C.rng_uniform(torch.empty(B, d), seed, sid_deq, ctr, lo, hi)
    return torch.cat([C.real_prep(x_int, deq, denom), fake], 0)


def _check(y, B, emb, w_ac):
    n, nf = y.shape[0], y.shape[1]
    assert n == 2 * B and B > 0 and nf % 4 == 0 and nf <= 1024 and not (emb is not None and w_ac is not None)


def tail_hinge_heads_fwd(y, B, w_out, b_out, labels=None, emb=None, w_ac=None, b_ac=None, scale=0.0):
    _check(y, B, emb, w_ac)
    f, d, a = C.tail_heads_fwd(y, w_out, b_out, w_ac, b_ac)
    if emb is not None:
        d = d + (f * emb[labels.long().repeat(2)]).sum(dim=1)            # tests/projection_cpu_kernels._projected: a zero table adds 0.0
    hr, hf = _hinge(1.0 - d[:B]).mean(), _hinge(1.0 + d[B:]).mean()
    probs = acc = None
    ac = torch.zeros(())
    if w_ac is not None:
        ac, probs, _ = C.softmax_ce_fwd(a[:B], labels)
        acc = C.accuracy2(a, labels, B)
    out = torch.stack([(hr + hf) + scale * ac, hr + hf, hr, hf, ac]).float()
    return out, f, d, a, probs, acc


def tail_hinge_heads_bwd(y, d, f, probs, labels, gout, B, scale, mask_scale, w_out, emb=None, w_ac=None, out=None):
    _check(y, B, emb, w_ac)
    g = gout.reshape(()) / B
    gd = torch.cat([-g * _on(1.0 - d[:B]), g * _on(1.0 + d[B:])])
    w_rows = w_out.reshape(1, -1).expand(2 * B, -1)
    lab2 = labels.long().repeat(2) if labels is not None else None
    if emb is not None:
        w_rows = w_rows + emb[lab2]
    t = gd[:, None] * w_rows
    gw_ac = gb_ac = g_emb = None
    if w_ac is not None:
        oh = torch.nn.functional.one_hot(labels.long(), probs.shape[1]).to(probs.dtype)
        ga = gout.reshape(()) * scale / B * (probs - oh)
        t = torch.cat([t[:B] + ga @ w_ac.t(), t[B:]], 0)
        gw_ac = f[:B].t() @ ga
        gb_ac = ga.sum(dim=0)
    hw = y.shape[2] * y.shape[3]
    gy = (t / hw)[:, :, None, None] * (y > 0).to(y.dtype) * mask_scale
    gw_out = (f.t() @ gd).reshape(w_out.shape); gb_out = gd.sum().reshape(1)
    if emb is not None:
        acc = torch.zeros(emb.shape, dtype=torch.float64)
        acc.index_add_(0, lab2, (f * gd[:, None]).double())
        g_emb = acc.float()
    if out is not None:
        out.copy_(gy)
        gy = out
    else:
        gy = gy.contiguous(memory_format=torch.channels_last)
    return gy, gw_out, gb_out, g_emb, gw_ac, gb_ac


@pytest.fixture
def hinge_cpu_kernels(spectral_cpu_kernels, monkeypatch):  # noqa: F811
    """spectral_cpu_kernels (which layers cpu_kernels, the projection, Layernorm, GAN-mode, averaging and loss-scale stand-ins), the DiffAugment
    stand-in and the stand-ins of this file."""
    import sys
    import ctgan_amd.kernels as K
    from tests import diffaug_cpu_kernels as DA
    for name in DA.__all__:
        monkeypatch.setattr(K, name, getattr(DA, name))
    mod = sys.modules[__name__]
    for name in __all__:
        monkeypatch.setattr(K, name, getattr(mod, name))
    yield mod
