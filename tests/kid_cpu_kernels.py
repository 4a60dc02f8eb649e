"""TEST-ONLY torch-CPU stand-in for the wrapper ctgan_amd.kernels gained with the kernel distance (csrc/kid.hip: ctgan_kernel_tile_sums).
Layered on tests/knn_cpu_kernels.py and tests/class_stats_cpu_kernels.py by the fixture `kid_kernels` below; nothing under ctgan_amd/
imports this file.  The kernel values are fp64 throughout, (gamma a . b + coef0)^3 with torch's own product for the dots - within the
oracle's bound of the direct form (tests/kid_oracle.py) - and padded rows and the excluded diagonal are masked by index, as on the
device."""
import pytest
import torch

from tests.class_stats_cpu_kernels import class_stats_kernels        # noqa: F401  (fixture)
from tests.knn_cpu_kernels import frechet_kernels, knn_kernels, score_cifar_kernels        # noqa: F401  (fixtures)

__all__ = ['kernel_tile_sums']

KERNEL_TILE = 64
ROWS = 1024          # rows of `a` per product: the [rows, n] kernel values stay small


def kernel_tile_sums(a, b, gamma=None, coef0=1.0, exclude_diag=False, out=None):
    (m, d), (n, db) = a.shape, b.shape
    assert a.dtype == b.dtype == torch.float32 and a.is_contiguous() and b.is_contiguous() and d == db
    if d > 1024:
        raise NotImplementedError('kernel_tile_sums: %d features (at most 1024)' % d)
    if m < 1 or n < 1 or (exclude_diag and m != n):
        raise ValueError('kernel_tile_sums: bad argument (m %d n %d)' % (m, n))
    t = KERNEL_TILE
    mt, nt = -(-m // t), -(-n // t)
    if out is None:
        out = torch.empty(mt, nt, dtype=torch.float64)
    assert out.dtype == torch.float64 and out.is_contiguous() and tuple(out.shape) == (mt, nt)
    gamma = 1.0 / d if gamma is None else float(gamma)
    b64 = b.double()
    for r0 in range(0, m, ROWS):
        rows = min(ROWS, m - r0)
        v = gamma * (a[r0:r0 + rows].double() @ b64.T) + float(coef0)
        k = torch.zeros(-(-rows // t) * t, nt * t, dtype=torch.float64)          # the padding holds 0, not coef0^3
        k[:rows, :n] = (v * v) * v
        if exclude_diag:
            i = torch.arange(r0, r0 + rows)
            k[i - r0, i] = 0.0
        out[r0 // t:r0 // t + k.shape[0] // t] = k.view(-1, t, nt, t).sum(dim=(1, 3))
    return out


@pytest.fixture
def kid_kernels(knn_kernels, class_stats_kernels, monkeypatch):        # noqa: F811
    """knn_kernels and class_stats_kernels plus the stand-in of this file."""
    import sys
    import ctgan_amd.kernels as K
    mod = sys.modules[__name__]
    for name in __all__:
        monkeypatch.setattr(K, name, getattr(mod, name))
    yield mod
