"""The per-class raw moments and the confusion matrix on the MI355X (`-m gpu`): csrc/moments.hip - ctgan_class_moments_accum against fp64
numpy on each class's rows and, bit for bit, against ctgan_moments_accum on those rows gathered in order; ctgan_confusion_accum against
numpy and against ctgan_score_accum's counts on the same logits.

Every bound is tests/frechet_oracle.py's, none is tuned: a class's raw moments within the order-independent summation bound
n_c 2^-52 |F_c|^T |F_c| of its own rows; the per-class distance within `distance_tolerance` of the two-pass distance of that class's
rows.  The counts and the matrix are integers: exact.  The largest observed error / bound ratios go to class_moments_err.json in the
run-output directory (tests/score_cifar_oracle.py `report_dir`)."""
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import frechet_oracle as FO  # noqa: E402
from tests import score_cifar_oracle as O  # noqa: E402
from tests.test_gpu_score_cifar import K  # noqa: E402,F401  (fixture)

_RATIOS = {}


def _report(key, ratio):
    _RATIOS[key] = max(float(ratio), _RATIOS.get(key, 0.0))
    with open(os.path.join(O.report_dir(), 'class_moments_err.json'), 'w') as f:
        json.dump({'largest_error_over_bound': _RATIOS}, f, indent=1, sort_keys=True)


def _ratio(err, bound):
    """max err / bound over the elements (an element with a zero bound must have a zero error)."""
    err, bound = np.asarray(err, dtype=np.float64), np.asarray(bound, dtype=np.float64)
    assert (err[bound == 0] == 0).all()
    return float((err[bound > 0] / bound[bound > 0]).max()) if (bound > 0).any() else 0.0


def _max_rows():
    import ctgan_amd.kernels as K
    return K.CLASS_MOMENTS_MAX_ROWS


def _labels(kind, m, classes, seed):
    r = np.random.RandomState(seed)
    if kind == 'random':
        lab = r.randint(0, classes, m)
    elif kind == 'zero':
        lab = np.zeros(m)
    elif kind == 'one_class':                                # all rows in one class, not the first
        lab = np.full(m, classes - 2)
    elif kind == 'absent_and_single':                        # class 3 absent altogether, class 7 with exactly 1 row
        lab = r.choice([c for c in range(classes) if c not in (3, 7)], m)
        lab[m // 2] = 7
    elif kind == 'ascending':
        lab = np.sort(r.randint(0, classes, m))
    elif kind == 'descending':
        lab = np.sort(r.randint(0, classes, m))[::-1]
    return np.ascontiguousarray(lab, dtype=np.int32)


# (m, d, classes, chunk, labels); m = chunk = None: CLASS_MOMENTS_MAX_ROWS + 5, the wrapper's split
CASES = [(1, 1, 1, 1, 'zero'),
         (57, 10, 3, 7, 'random'),                           # chunks with an absent class, a column tail
         (64, 17, 10, 64, 'absent_and_single'),
         (130, 16, 32, 130, 'random'),                       # the class limit; about 4 rows per class: three of the four waves get no rows
         (130, 33, 4, 50, 'one_class'),
         (301, 33, 10, 97, 'random'), (301, 33, 10, 97, 'ascending'), (301, 33, 10, 97, 'descending'),
         (1000, 192, 10, 1000, 'random'),
         (3000, 192, 10, 1000, 'random'),
         (None, 16, 3, None, 'random')]


def _pieces(m, chunk):
    """The (r0, r1) row ranges of the kernel calls: chunks of `chunk` rows, each cut by the wrapper at CLASS_MOMENTS_MAX_ROWS."""
    top = _max_rows()
    for c0 in range(0, m, chunk):
        c1 = min(c0 + chunk, m)
        for r0 in range(c0, c1, top):
            yield r0, min(r0 + top, c1)


def _device_class_moments(K, fd, ld, classes, chunk):
    m, d = fd.shape
    cnt = torch.zeros(classes, dtype=torch.int64, device='cuda')
    s1 = torch.zeros(classes, d, dtype=torch.float64, device='cuda')
    s2 = torch.zeros(classes, d, d, dtype=torch.float64, device='cuda')
    for r0 in range(0, m, chunk):
        K.class_moments_accum(fd[r0:r0 + chunk], ld[r0:r0 + chunk], cnt, s1, s2)
    return cnt, s1, s2


@pytest.mark.parametrize('offset', [0.0, 5.0])
@pytest.mark.parametrize('m,d,classes,chunk,kind', CASES)
def test_class_moments_match_fp64_and_the_gathered_rows_bit_for_bit(K, m, d, classes, chunk, kind, offset):
    if m is None:
        m = chunk = _max_rows() + 5
    f = FO.gaussian_features(m, d, seed=m + d, offset=offset)
    lab = _labels(kind, m, classes, seed=m + classes)
    if kind == 'absent_and_single':
        assert (lab == 3).sum() == 0 and (lab == 7).sum() == 1
    fd, ld = torch.from_numpy(f).cuda(), torch.from_numpy(lab).cuda()
    cnt, s1, s2 = _device_class_moments(K, fd, ld, classes, chunk)
    assert cnt.cpu().numpy().tolist() == np.bincount(lab, minlength=classes).tolist()
    g1, g2 = s1.cpu().numpy(), s2.cpu().numpy()
    worst = 0.0
    for c in range(classes):
        rows = f[lab == c]
        r1, r2 = FO.reference_moments(rows)
        b1, b2 = FO.moment_bound(rows)
        worst = max(worst, _ratio(np.abs(g1[c] - r1), b1), _ratio(np.abs(g2[c] - r2), b2))
        assert np.array_equal(g2[c], g2[c].T), c                                # exactly symmetric
    print('m %d d %d classes %d chunk %d %s offset %g: largest |moment - ref| / bound %.3e' % (m, d, classes, chunk, kind, offset, worst))
    _report('m%d_d%d_K%d_chunk%d_%s_offset%g' % (m, d, classes, chunk, kind, offset), worst)
    assert worst <= 1.0
    # the contract: the bits moments_accum leaves from each class's rows of each call, gathered in order
    t1 = torch.zeros(classes, d, dtype=torch.float64, device='cuda')
    t2 = torch.zeros(classes, d, d, dtype=torch.float64, device='cuda')
    for r0, r1 in _pieces(m, chunk):
        for c in range(classes):
            K.moments_accum(fd[r0:r1][ld[r0:r1] == c].contiguous(), t1[c], t2[c])
    assert torch.equal(s1, t1) and torch.equal(s2, t2)
    again = _device_class_moments(K, fd, ld, classes, chunk)                    # the same chunking: the same bits
    assert torch.equal(cnt, again[0]) and torch.equal(s1, again[1]) and torch.equal(s2, again[2])


def _filled(classes, d):
    return (torch.full((classes,), 3, dtype=torch.int64, device='cuda'), torch.full((classes, d), 3.0, dtype=torch.float64, device='cuda'),
            torch.full((classes, d, d), 3.0, dtype=torch.float64, device='cuda'))


def _untouched(*state):
    torch.cuda.synchronize()
    return all((t == 3).all().item() for t in state)


def test_absent_classes_and_labels_out_of_range_add_to_nothing(K):
    f = torch.from_numpy(FO.gaussian_features(40, 17, seed=1)).cuda()
    cnt, s1, s2 = _filled(4, 17)
    lab = torch.from_numpy(np.array([0, 2] * 20, dtype=np.int32)).cuda()       # classes 1 and 3 absent
    K.class_moments_accum(f, lab, cnt, s1, s2)
    assert cnt.cpu().tolist() == [23, 3, 23, 3]
    for c in (1, 3):
        assert (s1[c] == 3).all().item() and (s2[c] == 3).all().item()
    for c in (0, 2):
        assert not (s1[c] == 3).any().item() and not (s2[c] == 3).any().item()
    for value in (-1, 4):                                                       # every label outside [0, classes)
        cnt, s1, s2 = _filled(4, 17)
        K.class_moments_accum(f, torch.full((40,), value, dtype=torch.int32, device='cuda'), cnt, s1, s2)
        assert _untouched(cnt, s1, s2)
    K.class_moments_accum(f[:0], lab[:0], cnt, s1, s2)                           # no rows: a successful no-op
    assert _untouched(cnt, s1, s2)


def test_unsupported_and_bad_arguments_leave_the_state_untouched(K):
    f, lab = torch.ones(4, 16, device='cuda'), torch.zeros(4, dtype=torch.int32, device='cuda')
    cnt, s1, s2 = _filled(33, 16)
    with pytest.raises(NotImplementedError, match='33 classes'):
        K.class_moments_accum(f, lab, cnt, s1, s2)
    assert _untouched(cnt, s1, s2)
    cnt, s1, s2 = _filled(2, 1025)
    with pytest.raises(NotImplementedError, match='1025 features'):
        K.class_moments_accum(torch.ones(4, 1025, device='cuda'), lab, cnt, s1, s2)
    assert _untouched(cnt, s1, s2)
    cnt, s1, s2 = _filled(3, 16)
    with pytest.raises(AssertionError):
        K.class_moments_accum(f, lab, cnt, s1, s2[:, :, :8])
    with pytest.raises(AssertionError):
        K.class_moments_accum(f, lab, cnt, s1[:2], s2)
    with pytest.raises(AssertionError):
        K.class_moments_accum(f, lab, cnt, s1.float(), s2)
    with pytest.raises(AssertionError):
        K.class_moments_accum(f, lab, cnt.int(), s1, s2)
    with pytest.raises(AssertionError):
        K.class_moments_accum(f, lab[:3], cnt, s1, s2)
    with pytest.raises(TypeError):
        K.class_moments_accum(f, lab.long(), cnt, s1, s2)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        K.class_moments_accum(f.cpu(), lab, cnt, s1, s2)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        K.class_moments_accum(f, lab.cpu(), cnt, s1, s2)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        K.class_moments_accum(f, lab, cnt, s1.cpu(), s2)
    assert _untouched(cnt, s1, s2)
    conf = torch.full((33, 33), 3, dtype=torch.int64, device='cuda')
    with pytest.raises(NotImplementedError, match='33 classes'):
        K.confusion_accum(torch.ones(4, 33, device='cuda'), lab, conf)
    with pytest.raises(AssertionError):
        K.confusion_accum(torch.ones(4, 10, device='cuda'), lab, conf)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        K.confusion_accum(torch.ones(4, 33, device='cuda'), lab, conf.cpu())
    assert _untouched(conf)


@pytest.mark.parametrize('n,nc,chunk', [(1, 1, 1), (103, 10, 40), (3000, 10, 1000), (20000, 32, 20000)])
def test_confusion_matrix_is_exact_and_agrees_with_the_score_counts(K, n, nc, chunk):
    """Random logits with planted ties (the first maximum wins) and planted labels out of range; 20,000 rows: every workgroup takes
    more than one stride."""
    r = np.random.RandomState(n + nc)
    z = r.randn(n, nc).astype(np.float32)
    lab = r.randint(0, nc, n).astype(np.int32)
    if n > 1:
        for row in range(0, n, 7):                           # a tie of two or three maxima
            cols = r.choice(nc, min(nc, 2 + row % 2), replace=False)
            z[row, cols] = 9.0
        lab[1::11] = -1
        lab[5::13] = nc
        lab[6 % n] = 1 << 20
    valid = (lab >= 0) & (lab < nc)
    arg = z.argmax(axis=1)
    want = np.zeros((nc, nc), np.int64)
    np.add.at(want, (lab[valid], arg[valid]), 1)
    zd, ld = torch.from_numpy(z).cuda(), torch.from_numpy(lab).cuda()
    conf = torch.zeros(nc, nc, dtype=torch.int64, device='cuda')
    for r0 in range(0, n, chunk):
        K.confusion_accum(zd[r0:r0 + chunk], ld[r0:r0 + chunk], conf)
    got = conf.cpu().numpy()
    assert np.array_equal(got, want) and got.sum() == valid.sum()
    # score_accum on the same logits: its predicted-class counts over the valid rows, its label hits over all rows
    nv = int(valid.sum())
    zv, lv = torch.from_numpy(z[valid]).cuda(), torch.from_numpy(lab[valid]).cuda()
    acc, cnt = torch.zeros(1, nc + 1, dtype=torch.float64, device='cuda'), torch.zeros(2 * nc, dtype=torch.int64, device='cuda')
    K.score_accum(zv, 0, nv, 1, acc, cnt, lv)
    assert np.array_equal(got.sum(axis=0), cnt[:nc].cpu().numpy()) and np.array_equal(np.diag(got), cnt[nc:].cpu().numpy())
    acc, cnt = torch.zeros(1, nc + 1, dtype=torch.float64, device='cuda'), torch.zeros(2 * nc, dtype=torch.int64, device='cuda')
    K.score_accum(zd, 0, n, 1, acc, cnt, ld)
    assert np.array_equal(np.diag(got), cnt[nc:].cpu().numpy())


@pytest.mark.parametrize('offset', [0.0, 5.0])
@pytest.mark.parametrize('d', [16, 33])
def test_per_class_distance_of_synthetic_features_matches_the_two_pass_oracle(K, d, offset):
    """3 classes, 8 D + c rows of class c on each side, interleaved: per-class raw moments on the device -> ClassStatistics ->
    intra_frechet, against the two-pass distance of each class's rows."""
    from ctgan_amd.score_cifar import ClassStatistics, intra_frechet
    lab = np.repeat(np.arange(3), [8 * d + c for c in range(3)]).astype(np.int32)
    sides = []
    for side in range(2):
        l = lab.copy()
        np.random.RandomState(d + side).shuffle(l)
        f = FO.gaussian_features(len(l), d, seed=d + side, offset=offset + 0.3 * side)
        f += (0.5 * l[:, None]).astype(np.float32)
        cnt, s1, s2 = _device_class_moments(K, torch.from_numpy(f).cuda(), torch.from_numpy(l).cuda(), 3, 100)
        sides.append((f, l, ClassStatistics.from_moments(cnt.cpu().numpy(), s1.cpu().numpy(), s2.cpu().numpy())))
    (fa, la, a), (fb, lb, b) = sides
    got = intra_frechet(a, b)
    for c in range(3):
        ra, rb = fa[la == c], fb[lb == c]
        want = FO.features_distance(ra, rb)
        tol, info = FO.distance_tolerance(ra, rb)
        diff = abs(got['frechet_class'][c] - want)
        print('D %d offset %g class %d: distance %.17g, oracle %.17g, |diff| %.3e, tolerance %.3e' % (d, offset, c, got['frechet_class'][c], want, diff, tol))
        _report('synthetic_distance_D%d_offset%g_class%d' % (d, offset, c), diff / tol)
        assert info['lambda_min_product'] > 0.01 and tol < 1e-6 * want          # a well-conditioned case: the tolerance is a tight one
        assert diff <= tol
    assert got['intra_frechet'] == float(np.mean(got['frechet_class']))
