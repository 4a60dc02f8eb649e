"""TEST-ONLY torch-CPU stand-in for the wrapper ctgan_amd.kernels gained with the classifier Frechet distance (csrc/moments.hip:
ctgan_moments_accum).  Layered on tests/score_cifar_cpu_kernels.py by the fixture `frechet_kernels` below; nothing under ctgan_amd/
imports this file."""
import pytest
import torch

from tests.score_cifar_cpu_kernels import score_cifar_kernels        # noqa: F401  (fixture)

__all__ = ['moments_accum']


def moments_accum(feat, s1, s2):
    m, d = feat.shape
    if d > 1024:
        raise NotImplementedError('moments_accum: %d features (at most 1024)' % d)
    assert feat.dtype == torch.float32 and feat.is_contiguous()
    assert s1.dtype == s2.dtype == torch.float64 and tuple(s1.shape) == (d,) and tuple(s2.shape) == (d, d)
    f = feat.double()
    s1 += f.sum(dim=0)
    s2 += f.t() @ f


@pytest.fixture
def frechet_kernels(score_cifar_kernels, monkeypatch):        # noqa: F811
    """score_cifar_kernels plus the stand-in of this file."""
    import sys
    import ctgan_amd.kernels as K
    mod = sys.modules[__name__]
    for name in __all__:
        monkeypatch.setattr(K, name, getattr(mod, name))
    yield mod
