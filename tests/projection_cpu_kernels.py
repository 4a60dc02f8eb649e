"""TEST-ONLY torch-CPU stand-ins (fp32 results, as the device gives) for the six wrappers ctgan_amd.kernels gained with the projection head
(csrc/loss.hip: ctgan_*_proj).  Layered on tests/cpu_kernels.py and tests/cond_layernorm_cpu_kernels.py (the op-by-op head gathers table rows
with rows_gather) by the fixture `projection_cpu_kernels` below; nothing under ctgan_amd/ imports this file.

Each stand-in is its twin's stand-in with the per-row weight w_out + emb[label] written where the twin has w_out, in the twin's order of
operations: with a table of zeros every output has the twin's bits (w + 0.0 is exact), which tests/test_projection_host.py relies on."""
import pytest
import torch

from tests import cpu_kernels as C
from tests.cond_layernorm_cpu_kernels import cond_cpu_kernels  # noqa: F401  (fixture the one below builds on)

__all__ = ['tail_critic_heads_fwd_proj', 'tail_heads_bwd_proj', 'gen_heads_fwd_proj', 'gen_heads_bwd_proj', 'gp_head_grad_proj',
           'gp_head_wgrad_proj']


def _rows(emb, labels):
    return emb[labels.long()]


def _by_label(rows, labels, like):
    out = torch.zeros(like.shape, dtype=torch.float64)
    out.index_add_(0, labels.long(), rows.double())
    return out.float()


def _projected(f, d, emb, row_labels):
    return d + (f * _rows(emb, row_labels)).sum(dim=1)


def tail_critic_heads_fwd_proj(y, B, w_out, b_out, emb, labels, gp, lam2, M, slopes=None, gp_lambda=0.0):
    f, d, _ = C.tail_heads_fwd(y, w_out, b_out, None, None)
    d = _projected(f, d, emb, labels.repeat(3))
    if slopes is not None:
        gp.copy_((gp_lambda * ((slopes - 1) ** 2).mean()).reshape(gp.shape))
    out, ct_i, _ = C.critic_heads_fwd(d, f, None, labels, B, lam2, M, 0.0, gp)
    return out, f, d, ct_i


def tail_heads_bwd_proj(y, d, f, labels, ct_i, gout, B, lam2, M, mask_scale, w_out, emb, out=None, y_gp=None, out_gp=None):
    if y_gp is not None:
        gp_head_grad_proj(y_gp, w_out, mask_scale, emb, labels[:y_gp.shape[0]], out=out_gp)
    gd, gf, _ = C.critic_heads_bwd(d, f, None, labels, ct_i, gout, B, lam2, M, 0.0)
    lab3 = labels.repeat(3)
    t = gf + gd[:, None] * (w_out.reshape(1, -1) + _rows(emb, lab3))
    hw = y.shape[2] * y.shape[3]
    gy = (t / hw)[:, :, None, None] * (y > 0).to(y.dtype) * mask_scale
    gw_out = (f.t() @ gd).reshape(w_out.shape); gb_out = gd.sum().reshape(1)
    g_emb = _by_label(f * gd[:, None], lab3, emb)
    if out is not None:
        out.copy_(gy)
        return out, gw_out, gb_out, g_emb
    return gy.contiguous(memory_format=torch.channels_last), gw_out, gb_out, g_emb


def gen_heads_fwd_proj(y, w_out, b_out, emb, labels):
    f, d, _ = C.tail_heads_fwd(y, w_out, b_out, None, None)
    d = _projected(f, d, emb, labels)
    return (-d.mean()).reshape(1).float(), d


def gen_heads_bwd_proj(y, labels, gout, mask_scale, w_out, emb):
    n = y.shape[0]; hw = y.shape[2] * y.shape[3]
    g0 = gout.reshape(()) / n
    t = (-g0 * (w_out.reshape(1, -1) + _rows(emb, labels))).expand(n, -1)
    gy = (t / hw)[:, :, None, None] * (y > 0).to(y.dtype) * mask_scale
    return gy.contiguous(memory_format=torch.channels_last)


def gp_head_grad_proj(y, w_out, mask_scale, emb, labels, out=None):
    hw = y.shape[2] * y.shape[3]
    gz = (y > 0).to(y.dtype) * ((w_out.reshape(1, -1) + _rows(emb, labels))[:, :, None, None] / hw * mask_scale)
    if out is not None:
        out.copy_(gz)
        return out
    return gz.contiguous(memory_format=torch.channels_last)


def gp_head_wgrad_proj(gg, y, mask_scale, like, emb, labels, add_to=None, add_to_emb=None):
    hw = y.shape[2] * y.shape[3]
    gw = C.gp_head_wgrad(gg, y, mask_scale, like, add_to=add_to)                  # the twin's own sum: the same bits for gw_out
    per_row = (gg * (y > 0).to(y.dtype)).sum(dim=(2, 3)) * (mask_scale / hw)
    g_emb = _by_label(per_row, labels, emb)
    if add_to_emb is not None:
        add_to_emb += g_emb
        return gw, add_to_emb
    return gw, g_emb


@pytest.fixture
def projection_cpu_kernels(cond_cpu_kernels, monkeypatch):  # noqa: F811
    """cpu_kernels (tests/conftest.py) and cond_cpu_kernels plus the stand-ins of this file."""
    import sys
    import ctgan_amd.kernels as K
    mod = sys.modules[__name__]
    for name in __all__:
        monkeypatch.setattr(K, name, getattr(mod, name))
    yield mod
