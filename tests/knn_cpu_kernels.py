"""TEST-ONLY torch-CPU stand-ins for the wrappers ctgan_amd.kernels gained with precision and recall (csrc/knn.hip: ctgan_knn_radii,
ctgan_knn_cover).  Layered on tests/frechet_cpu_kernels.py by the fixture `knn_kernels` below; nothing under ctgan_amd/ imports this
file.  The distances are the oracle's direct form sum (a - b)^2 in fp64 (tests/knn_oracle.py): bit-identical rows are at exactly 0, as
on the device."""
import pytest
import torch

from tests import knn_oracle as KO
from tests.frechet_cpu_kernels import frechet_kernels, score_cifar_kernels        # noqa: F401  (fixtures)

__all__ = ['knn_radii', 'knn_cover']

KNN_MAX_K = 8


def _d2(a, b):
    return torch.from_numpy(KO.d2_direct(a.numpy(), b.numpy()))          # the oracle's distances; the selections below are torch's own


def _out(out, rows, dtype):
    if out is None:
        return torch.empty(rows, dtype=dtype)
    assert out.dtype == dtype and out.dim() == 1 and out.is_contiguous() and out.numel() >= rows
    return out


def knn_radii(feat, k, out=None):
    n, d = feat.shape
    assert feat.dtype == torch.float32 and feat.is_contiguous()
    if d > 1024:
        raise NotImplementedError('knn_radii: %d features (at most 1024)' % d)
    if k > KNN_MAX_K:
        raise NotImplementedError('knn_radii: k = %d (at most %d)' % (k, KNN_MAX_K))
    if k < 1 or n < k + 1:
        raise ValueError('knn_radii: %d rows have no %d-th other neighbour' % (n, k))
    out = _out(out, n, torch.float64)
    dist = _d2(feat, feat)
    dist.fill_diagonal_(float('inf'))
    out[:n] = torch.sort(dist, dim=1, stable=True).values[:, k - 1]
    return out


def knn_cover(a, b, r2_b=None, covered=None, nn_d2=None, nn_idx=None):
    (m, d), (n, db) = a.shape, b.shape
    assert a.dtype == b.dtype == torch.float32 and a.is_contiguous() and b.is_contiguous() and d == db
    assert r2_b is None or (r2_b.dtype == torch.float64 and r2_b.numel() == n)
    if d > 1024:
        raise NotImplementedError('knn_cover: %d features (at most 1024)' % d)
    if n < 1:
        raise ValueError('knn_cover: bad argument')
    covered = None if r2_b is None else _out(covered, m, torch.int32)
    nn_d2, nn_idx = _out(nn_d2, m, torch.float64), _out(nn_idx, m, torch.int32)
    if m == 0:
        return covered, nn_d2, nn_idx
    dist = _d2(a, b)
    low = dist.min(dim=1).values
    nn_d2[:m] = low
    nn_idx[:m] = (dist == low[:, None]).int().argmax(dim=1).int()          # the lowest index attaining the minimum
    if r2_b is not None:
        covered[:m] = (dist <= r2_b[None, :]).any(dim=1).int()
    return covered, nn_d2, nn_idx


@pytest.fixture
def knn_kernels(frechet_kernels, monkeypatch):        # noqa: F811
    """frechet_kernels plus the stand-ins of this file."""
    import sys
    import ctgan_amd.kernels as K
    mod = sys.modules[__name__]
    for name in __all__:
        monkeypatch.setattr(K, name, getattr(mod, name))
    yield mod
