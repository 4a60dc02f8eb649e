"""TEST-ONLY torch-CPU stand-ins (fp32 results, as the device gives) for the two wrappers ctgan_amd.kernels gained with spectral normalisation
(csrc/spectral.hip): spectral_normalize and spectral_grad.  kernels.SpectralTable needs no stand-in - it is filled on the host by the library
and only copied to the trainer's device.  Layered on tests/cpu_kernels.py,
tests/projection_cpu_kernels.py and tests/loss_scale_cpu_kernels.py by the fixture `spectral_cpu_kernels` below; nothing under ctgan_amd/
imports this file.  The sums run in fp64 and are rounded once: within the bounds of tests/spectral_oracle.py, not the device's bits."""
import pytest
import torch

from tests.loss_scale_cpu_kernels import avg_kernels, mode_kernels, scale_kernels  # noqa: F401  (fixtures the one below builds on)
from tests.projection_cpu_kernels import cond_cpu_kernels, projection_cpu_kernels  # noqa: F401

__all__ = ['spectral_normalize', 'spectral_grad']

EPS = 1e-12


def _jobs(table):
    return [(o, k, n, uo, vo) for (o, k, n), uo, vo in zip(table.jobs, table.u_offs, table.v_offs)]


def spectral_normalize(theta, theta_bar, table, u, v, sigma, scratch, iterate=True, hold=None):
    if hold is not None and float(hold[0]) != 0.0:
        iterate = False                       # the update since spectral_grad(..., scaler=, hold=) was dropped: no new weight version
    assert theta.numel() == theta_bar.numel() == table.total
    theta_bar.copy_(theta)
    for j, (o, k, n, uo, vo) in enumerate(_jobs(table)):
        M = theta[o:o + k * n].view(k, n)
        if iterate:
            t = (M.double() @ u[uo:uo + n].double()).float()
            nt = t.double().pow(2).sum().sqrt().float().clamp_min(EPS)
            vj = t / nt
            s = (M.double().t() @ t.double()).float() / nt
            sg = s.double().pow(2).sum().sqrt().float()
            v[vo:vo + k].copy_(vj); sigma[j] = sg; u[uo:uo + n].copy_(s / sg.clamp_min(EPS))
        theta_bar[o:o + k * n].copy_((M / sigma[j].clamp_min(EPS)).reshape(-1))


def spectral_grad(gbar, theta_bar, table, u, v, sigma, scratch, scaler=None, hold=None):
    assert (scaler is None) == (hold is None)
    if hold is not None:
        hold[0] = scaler[1]
    assert gbar.numel() == theta_bar.numel() == table.total
    for j, (o, k, n, uo, vo) in enumerate(_jobs(table)):
        G = gbar[o:o + k * n].view(k, n)
        dot = (G.double() * theta_bar[o:o + k * n].view(k, n).double()).sum().float()
        G.copy_((G - (dot * v[vo:vo + k])[:, None] * u[uo:uo + n][None, :]) / sigma[j].clamp_min(EPS))


@pytest.fixture
def spectral_cpu_kernels(projection_cpu_kernels, scale_kernels, monkeypatch):  # noqa: F811
    """cpu_kernels (tests/conftest.py), the conditional-Layernorm and projection-head stand-ins, the RMSProp / GAN-loss / weight-average /
    loss-scale stand-ins, plus the stand-ins of this file."""
    import sys
    import ctgan_amd.kernels as K
    mod = sys.modules[__name__]
    for name in __all__:
        monkeypatch.setattr(K, name, getattr(mod, name))
    yield mod
