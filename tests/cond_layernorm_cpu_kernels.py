"""TEST-ONLY torch-CPU stand-ins (fp32 results, as the device gives) for the wrappers ctgan_amd.kernels gained with the label-conditioned
Layernorm (csrc/layernorm.hip: ctgan_layernorm_cond_{fwd,bwd,bwd2} and the row gather / by-label sum of the composed operator).  Layered
on tests/cpu_kernels.py by the fixture `cond_cpu_kernels` below; nothing under ctgan_amd/ imports this file."""
import pytest
import torch

from tests import cpu_kernels as C

__all__ = ['layernorm_cond_fwd', 'layernorm_cond_bwd', 'layernorm_cond_bwd2', 'rows_gather', 'rows_sum_by_label']


def _rows(table, labels):
    return table[labels.long().clamp(0, table.shape[0] - 1)]


def _by_label(rows, labels, n_labels):
    out = torch.zeros(n_labels, rows.shape[1], dtype=torch.float64)
    out.index_add_(0, labels.long().clamp(0, n_labels - 1), rows.double())
    return out.float()


def rows_gather(table, labels):
    return _rows(table, labels).contiguous()


def rows_sum_by_label(rows, labels, n_labels):
    return _by_label(rows, labels, n_labels)


def _parts(x, scale, labels, mean, rstd):
    shp = [-1] + [1] * (x.dim() - 1)
    nshp = [x.shape[0], -1] + [1] * (x.dim() - 2)
    xh = (x.double() - mean.double().reshape(shp)) * rstd.double().reshape(shp)
    return xh, _rows(scale, labels).double().reshape(nshp), shp, nshp, tuple(range(1, x.dim())), tuple(range(2, x.dim()))


def layernorm_cond_fwd(x, scale, offset, labels, eps, relu=False):
    dims = tuple(range(1, x.dim()))
    xd = x.double()
    mean = xd.mean(dim=dims)
    rstd = 1.0 / torch.sqrt(xd.var(dim=dims, unbiased=False) + eps)
    xh, s, shp, nshp, _, _ = _parts(x, scale, labels, mean, rstd)
    y = xh * s + _rows(offset, labels).double().reshape(nshp)
    if relu:
        y = torch.relu(y)
    return C._like(y.float(), x), mean.float(), rstd.float()


def layernorm_cond_bwd(gy, x, scale, labels, mean, rstd, want_params, ymask=None):
    xh, s, shp, nshp, sd, hw = _parts(x, scale, labels, mean, rstd)
    if ymask is not None:
        gy = gy * (ymask > 0).to(gy.dtype)
    g = gy.double() * s
    a = g.mean(dim=sd, keepdim=True); b = (g * xh).mean(dim=sd, keepdim=True)
    gx = C._like((rstd.double().reshape(shp) * (g - a - xh * b)).float(), x)
    if not want_params:
        return gx, None, None
    L = scale.shape[0]
    gs, go = gy.double() * xh, gy.double()
    if hw:
        gs, go = gs.sum(dim=hw), go.sum(dim=hw)
    return gx, _by_label(gs, labels, L), _by_label(go, labels, L)


def layernorm_cond_bwd2(u, gy, x, scale, labels, mean, rstd, want_gy=True, want_x=True, want_scale=True, ymask=None):
    # autograd through the double-precision restatement of layernorm_cond_bwd as a function of (gy, x, scale table)
    dims = tuple(range(1, x.dim()))
    nshp = [x.shape[0], -1] + [1] * (x.dim() - 2)
    # per sample, so that var + eps is 1 / rstd^2 of that sample whatever the other samples' variances are (a constant one among them)
    eps = (1.0 / rstd.double() ** 2 - x.double().var(dim=dims, unbiased=False)).reshape([-1] + [1] * (x.dim() - 1))
    with torch.enable_grad():
        gy_, x_, s_ = (t.detach().double().requires_grad_(True) for t in (gy, x, scale))
        m = x_.mean(dim=dims, keepdim=True)
        r = 1.0 / torch.sqrt(x_.var(dim=dims, unbiased=False, keepdim=True) + eps)
        xh = (x_ - m) * r
        g = gy_ * _rows(s_, labels).reshape(nshp)
        if ymask is not None:
            g = g * (ymask > 0).double()
        gx = r * (g - g.mean(dim=dims, keepdim=True) - xh * (g * xh).mean(dim=dims, keepdim=True))
        cg, cx, cs = torch.autograd.grad(gx, [gy_, x_, s_], u.double())
    return (C._like(cg.float(), x) if want_gy else None, C._like(cx.float(), x) if want_x else None, cs.float() if want_scale else None)


@pytest.fixture
def cond_cpu_kernels(cpu_kernels, monkeypatch):
    """cpu_kernels (tests/conftest.py) plus the stand-ins of this file."""
    import sys
    import ctgan_amd.kernels as K
    mod = sys.modules[__name__]
    for name in __all__:
        monkeypatch.setattr(K, name, getattr(mod, name))
    yield mod
