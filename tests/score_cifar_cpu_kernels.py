"""TEST-ONLY torch-CPU stand-ins for the wrappers ctgan_amd.kernels gained with the classifier score of CIFAR-10 samples
(csrc/score_cifar.hip: ctgan_score_{input,accum,finish}).  Layered on tests/cpu_kernels.py, on tests/ssl_cifar_oracle.py's stand-ins
(the CT classifiers) and on the evaluation tests' (the GAN modes, pixels_u8) by the fixture `score_cifar_kernels` below; nothing under
ctgan_amd/ imports this file."""
import pytest
import torch

from tests import eval_helpers as H

__all__ = ['score_input', 'score_accum', 'score_finish']


def score_input(x, channels, scale, lut):
    n, hw = x.shape[0], x.shape[1] // channels
    side = int(round(hw ** 0.5))
    assert side * side == hw
    px = H.pixels_u8_cpu(x, channels, scale).reshape(n, side, side, channels)          # NHWC bytes
    out = lut[torch.flip(px, (1, 2)).long()]                                           # rotated by 180 degrees, still NHWC
    return out.permute(0, 3, 1, 2)                                                     # logical NCHW over channels-last memory


def score_accum(logits, r0, n, splits, acc, cnt, labels=None):
    m, K = logits.shape
    if K > 32:
        raise NotImplementedError('score_accum: %d classes (at most 32)' % K)
    if n < splits or r0 < 0 or r0 + m > n:
        raise ValueError('score_accum: bad shape')
    assert acc.dtype == torch.float64 and tuple(acc.shape) == (splits, K + 1) and cnt.dtype == torch.int64 and cnt.numel() == 2 * K
    z = logits.double()
    lp = torch.log_softmax(z, dim=1)
    p = lp.exp()
    term = torch.where((p == 0) & torch.isfinite(lp), torch.zeros_like(p), p * lp).sum(dim=1)
    arg = torch.from_numpy(logits.numpy().argmax(axis=1))
    for k in range(splits):
        a, b = max(k * n // splits, r0) - r0, min((k + 1) * n // splits, r0 + m) - r0
        if a < b:
            acc[k, :K] += p[a:b].sum(dim=0)
            acc[k, K] += term[a:b].sum()
    cnt[:K] += torch.bincount(arg, minlength=K)
    if labels is not None:
        cnt[K:] += torch.bincount(arg[arg == labels.long()], minlength=K)


def score_finish(acc, n, splits):
    K = acc.shape[1] - 1
    nk = torch.tensor([(k + 1) * n // splits - k * n // splits for k in range(splits)], dtype=torch.float64)
    m = acc[:, :K] / nk[:, None]
    h = torch.where(m == 0, torch.zeros_like(m), m * m.log()).sum(dim=1)
    s = (acc[:, K] / nk - h).exp()
    return torch.cat([s.mean().reshape(1), s.std(unbiased=False).reshape(1), s])


@pytest.fixture
def score_cifar_kernels(cpu_kernels, monkeypatch):
    """cpu_kernels (tests/conftest.py) plus every stand-in a CT classifier, a CIFAR GAN of any mode and the score path between them need."""
    import sys
    import ctgan_amd.ct_cifar as M
    import ctgan_amd.kernels as K
    import ctgan_amd.tflib as lib
    import ctgan_amd.ct_cifar_te as T
    from tests import ssl_cifar_te_oracle as O
    from tests import test_gan_modes_host as G
    O.install_stand_ins(monkeypatch)                  # (ssl_cifar_oracle's stand-ins plus the temporal-ensembling head's)
    for name, fn in (('rmsprop_step', G._rmsprop_step), ('rmsprop_step_packed', G._rmsprop_step_packed), ('gan_loss_fwd', G._gan_loss_fwd),
                     ('gan_loss_bwd', G._gan_loss_bwd), ('pixels_u8', H.pixels_u8_cpu)):
        monkeypatch.setattr(K, name, fn)
    mod = sys.modules[__name__]
    for name in __all__:
        monkeypatch.setattr(K, name, getattr(mod, name))
    yield mod
    T.configure(); M.configure(); lib.delete_all_params(); lib.delete_param_aliases()
