"""TEST-ONLY torch-CPU stand-ins for the wrappers ctgan_amd.kernels gained with the per-class precision, recall and kernel distance
(csrc/knn.hip: ctgan_knn_radii_seg, ctgan_knn_cover_seg; csrc/kid.hip: ctgan_kernel_tile_sums_seg, ctgan_segment_sums).  Layered on
tests/kid_cpu_kernels.py by the fixture `class_manifold_kernels` below; nothing under ctgan_amd/ imports this file.  Each is the pooled
stand-in of tests/knn_cpu_kernels.py / tests/kid_cpu_kernels.py applied to one segment at a time - what the device's contract says of the
grouped kernels - with the counts read on the host, which a test may do.  kernels.class_segments is torch alone and runs as it is."""
import math

import pytest
import torch

from tests import kid_cpu_kernels as KC
from tests import knn_cpu_kernels as NC
from tests.kid_cpu_kernels import class_stats_kernels, frechet_kernels, kid_kernels, knn_kernels, score_cifar_kernels        # noqa: F401  (fixtures)

__all__ = ['knn_radii_seg', 'knn_cover_seg', 'kernel_tile_sums_seg', 'segment_sums']

SEG_MAX_CLASSES = 32
KERNEL_TILE = 64


def _segments(seg, rows):
    assert seg.dtype == torch.int32 and seg.dim() == 1 and 2 <= seg.numel() <= SEG_MAX_CLASSES + 1
    s = [min(max(int(v), 0), rows) for v in seg.tolist()]
    return [(s[c], max(s[c + 1], s[c])) for c in range(len(s) - 1)]


def knn_radii_seg(feat, seg, k, out=None):
    n, d = feat.shape
    assert feat.dtype == torch.float32 and feat.is_contiguous()
    if d > 1024:
        raise NotImplementedError('knn_radii_seg: %d features (at most 1024)' % d)
    if k > NC.KNN_MAX_K:
        raise NotImplementedError('knn_radii_seg: k = %d (at most %d)' % (k, NC.KNN_MAX_K))
    if k < 1:
        raise ValueError('knn_radii_seg: bad argument')
    out = NC._out(out, n, torch.float64)
    for s0, s1 in _segments(seg, n):
        if s1 - s0 >= k + 1:
            out[s0:s1] = NC.knn_radii(feat[s0:s1].contiguous(), k)
        else:
            out[s0:s1] = float('inf')
    return out


def knn_cover_seg(a, seg_a, b, seg_b, r2_b=None, covered=None, nn_d2=None, nn_idx=None):
    (m, d), (n, db) = a.shape, b.shape
    assert a.dtype == b.dtype == torch.float32 and a.is_contiguous() and b.is_contiguous() and d == db
    assert seg_a.numel() == seg_b.numel()
    assert r2_b is None or (r2_b.dtype == torch.float64 and r2_b.numel() == n)
    if d > 1024:
        raise NotImplementedError('knn_cover_seg: %d features (at most 1024)' % d)
    covered = None if r2_b is None else NC._out(covered, m, torch.int32)
    nn_d2, nn_idx = NC._out(nn_d2, m, torch.float64), NC._out(nn_idx, m, torch.int32)
    for (a0, a1), (b0, b1) in zip(_segments(seg_a, m), _segments(seg_b, n)):
        if a1 == a0:
            continue
        if b1 == b0:
            nn_d2[a0:a1], nn_idx[a0:a1] = float('inf'), -1
            if covered is not None:
                covered[a0:a1] = 0
            continue
        cov, d2, idx = NC.knn_cover(a[a0:a1].contiguous(), b[b0:b1].contiguous(), None if r2_b is None else r2_b[b0:b1].contiguous())
        nn_d2[a0:a1], nn_idx[a0:a1] = d2, idx
        if covered is not None:
            covered[a0:a1] = cov
    return covered, nn_d2, nn_idx


def kernel_tile_sums_seg(a, seg_a, b, seg_b, gamma=None, coef0=1.0, exclude_diag=False, out=None):
    (m, d), (n, db) = a.shape, b.shape
    assert a.dtype == b.dtype == torch.float32 and a.is_contiguous() and b.is_contiguous() and d == db
    assert seg_a.numel() == seg_b.numel()
    assert not exclude_diag or (a.data_ptr() == b.data_ptr() and seg_a.data_ptr() == seg_b.data_ptr())
    if d > 1024:
        raise NotImplementedError('kernel_tile_sums_seg: %d features (at most 1024)' % d)
    if m < 1 or n < 1:
        raise ValueError('kernel_tile_sums_seg: bad argument (m %d n %d)' % (m, n))
    t, classes = KERNEL_TILE, seg_a.numel() - 1
    size = (-(-m // t) + classes) * (-(-n // t) + 1)
    if out is None:
        out = torch.zeros(size, dtype=torch.float64)
    assert out.dtype == torch.float64 and tuple(out.shape) == (size,)
    out.zero_()
    toff = [0]
    for (a0, a1), (b0, b1) in zip(_segments(seg_a, m), _segments(seg_b, n)):
        cnt = -(-(a1 - a0) // t) * -(-(b1 - b0) // t)
        if cnt:
            out[toff[-1]:toff[-1] + cnt] = KC.kernel_tile_sums(a[a0:a1].contiguous(), b[b0:b1].contiguous(), gamma, coef0, exclude_diag).reshape(-1)
        toff.append(toff[-1] + cnt)
    return out, torch.tensor(toff, dtype=torch.int64)


def segment_sums(vals, off, out=None):
    assert vals.dtype == torch.float64 and vals.dim() == 1 and off.dtype == torch.int64 and off.dim() == 1 and off.numel() >= 1
    s = off.numel() - 1
    out = NC._out(out, s, torch.float64)
    o = off.tolist()
    for i in range(s):
        out[i] = math.fsum(vals[o[i]:o[i + 1]].tolist())
    return out


@pytest.fixture
def class_manifold_kernels(kid_kernels, monkeypatch):        # noqa: F811
    """kid_kernels (and all it is layered on) plus the stand-ins of this file."""
    import sys
    import ctgan_amd.kernels as K
    mod = sys.modules[__name__]
    for name in __all__:
        monkeypatch.setattr(K, name, getattr(mod, name))
    yield mod
