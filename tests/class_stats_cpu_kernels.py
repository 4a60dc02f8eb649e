"""TEST-ONLY torch-CPU stand-ins for the wrappers ctgan_amd.kernels gained with the per-class Frechet distance and the confusion matrix
(csrc/moments.hip: ctgan_class_moments_accum, ctgan_confusion_accum).  Layered on tests/frechet_cpu_kernels.py by the fixture
`class_stats_kernels` below; nothing under ctgan_amd/ imports this file."""
import pytest
import torch

from tests.frechet_cpu_kernels import frechet_kernels, moments_accum, score_cifar_kernels        # noqa: F401  (fixtures)

__all__ = ['class_moments_accum', 'confusion_accum']


def class_moments_accum(feat, labels, cnt, s1, s2):
    m, d = feat.shape
    k = cnt.numel()
    if k > 32:
        raise NotImplementedError('class_moments_accum: %d classes (at most 32)' % k)
    assert labels.dtype == torch.int32 and tuple(labels.shape) == (m,)
    assert cnt.dtype == torch.int64 and tuple(s1.shape) == (k, d) and tuple(s2.shape) == (k, d, d)
    for c in range(k):
        rows = feat[labels == c].contiguous()          # the gathered rows, in ascending row order
        cnt[c] += rows.shape[0]
        if rows.shape[0]:
            moments_accum(rows, s1[c], s2[c])


def confusion_accum(logits, labels, conf):
    m, k = logits.shape
    if k > 32:
        raise NotImplementedError('confusion_accum: %d classes (at most 32)' % k)
    assert labels.dtype == torch.int32 and tuple(labels.shape) == (m,) and conf.dtype == torch.int64 and tuple(conf.shape) == (k, k)
    arg = torch.from_numpy(logits.numpy().argmax(axis=1))
    lab = labels.long()
    ok = (lab >= 0) & (lab < k)
    conf += torch.bincount(lab[ok] * k + arg[ok], minlength=k * k).view(k, k)


@pytest.fixture
def class_stats_kernels(frechet_kernels, monkeypatch):        # noqa: F811
    """frechet_kernels plus the stand-ins of this file."""
    import sys
    import ctgan_amd.kernels as K
    mod = sys.modules[__name__]
    for name in __all__:
        monkeypatch.setattr(K, name, getattr(mod, name))
    yield mod
