"""The per-class Frechet distance and the confusion matrix of conditional samples (ctgan_amd.score_cifar: ClassStatistics, intra_frechet,
the class reference of ClassifierScore) without a GPU: the host arithmetic against the fp64 restatement (tests/frechet_oracle.py), and
the host logic on CPU stand-ins (tests/class_stats_cpu_kernels.py).  Every bound is frechet_oracle's; none is tuned."""
import numpy as np
import pytest
import torch

from tests import eval_helpers as H
from tests import frechet_oracle as FO
from tests import score_cifar_oracle as O
from tests.class_stats_cpu_kernels import class_stats_kernels, frechet_kernels, score_cifar_kernels        # noqa: F401  (fixtures)
from tests.test_score_cifar_host import _Series, _checkpoint_scorer

SCORE_KEYS = ('mean', 'std', 'splits', 'hist', 'acc')
CLASS_KEYS = ('frechet_class', 'intra_frechet', 'n_class', 'confusion', 'acc_class')


def _labelled(counts, d, seed, offset=0.0):
    """fp32 features [sum counts, d] and a shuffled int32 label column with counts[c] rows of class c."""
    lab = np.repeat(np.arange(len(counts)), counts).astype(np.int32)
    np.random.RandomState(seed).shuffle(lab)
    f = FO.gaussian_features(len(lab), d, seed=seed, offset=offset)
    f += (0.25 * lab[:, None]).astype(np.float32)          # the classes differ in their means
    return f, lab


def _raw(f, lab, classes):
    d = f.shape[1]
    cnt, s1, s2 = np.zeros(classes, np.int64), np.zeros((classes, d)), np.zeros((classes, d, d))
    for c in range(classes):
        cnt[c] = (lab == c).sum()
        s1[c], s2[c] = FO.reference_moments(f[lab == c])
    return cnt, s1, s2


# ----------------------------------------------------------------------------------------------------- ClassStatistics
def test_class_statistics_per_class_pooled_and_the_nan_rules(tmp_path):
    from ctgan_amd.score_cifar import ClassStatistics, FeatureStatistics
    f, lab = _labelled([40, 0, 1, 25], 6, seed=1, offset=2.0)
    st = ClassStatistics.from_moments(*_raw(f, lab, 4), classifier='abc')
    assert st.classes == 4 and st.width == 6 and st.n.dtype == np.int64 and st.n.tolist() == [40, 0, 1, 25]
    for c in (0, 3):
        n, mean, cov = FO.two_pass_statistics(f[lab == c])
        dmean, dcov = FO.statistics_bound(f[lab == c])
        one = st.of(c)
        assert isinstance(one, FeatureStatistics) and one.n == n and one.classifier == 'abc'
        assert (np.abs(one.mean - mean) <= dmean).all() and (np.abs(one.cov - cov) <= dcov).all()
    assert np.isnan(st.mean[1]).all() and np.isnan(st.cov[1]).all()                         # no rows: no mean, no covariance
    assert np.array_equal(st.mean[2], f[lab == 2][0].astype(np.float64)) and np.isnan(st.cov[2]).all()          # one row: no covariance
    assert st.of(2).n == 1
    with pytest.raises(ValueError, match='no rows'):
        st.of(1)
    # all counted rows together: the one-row class and the empty one included
    pooled = st.pooled()
    n, mean, cov = FO.two_pass_statistics(f)
    dmean, dcov = FO.statistics_bound(f)
    assert pooled.n == n == 66 and pooled.classifier == 'abc'
    assert (np.abs(pooled.mean - mean) <= dmean).all() and (np.abs(pooled.cov - cov) <= dcov).all()
    for tag in ('abc', None):
        path = str(tmp_path / ('cls_%s.npz' % tag))
        ClassStatistics(st.n, st.mean, st.cov, tag).save(path)
        back = ClassStatistics.load(path)
        assert back.classifier == tag and np.array_equal(back.n, st.n) and back.n.dtype == np.int64
        assert np.array_equal(back.mean, st.mean, equal_nan=True) and np.array_equal(back.cov, st.cov, equal_nan=True)
    with np.load(str(tmp_path / 'cls_abc.npz'), allow_pickle=False) as z:
        assert sorted(z.files) == ['classifier', 'cov', 'mean', 'n']
    with pytest.raises(ValueError):
        ClassStatistics(st.n, st.mean[:3], st.cov)
    with pytest.raises(ValueError):
        ClassStatistics.from_moments(np.zeros(2, np.int64), np.zeros((2, 3)), np.zeros((2, 3, 3))).pooled()


def test_intra_frechet_is_the_mean_of_the_per_class_distances():
    from ctgan_amd.score_cifar import ClassStatistics, intra_frechet
    d = 6
    fa, la = _labelled([50, 48, 1, 0, 52], d, seed=2)
    fb, lb = _labelled([49, 51, 50, 47, 1], d, seed=3, offset=0.3)
    a = ClassStatistics.from_moments(*_raw(fa, la, 5))
    b = ClassStatistics.from_moments(*_raw(fb, lb, 5))
    got = intra_frechet(a, b)
    assert set(got) == {'frechet_class', 'intra_frechet'} and got['frechet_class'].shape == (5,) and got['frechet_class'].dtype == np.float64
    assert np.isnan(got['frechet_class'][2:]).all()          # 1 row on side a; none on side a; 1 row on side b
    for c in (0, 1):
        want = FO.features_distance(fa[la == c], fb[lb == c])
        tol, _ = FO.distance_tolerance(fa[la == c], fb[lb == c])
        assert want > 0.01 and abs(got['frechet_class'][c] - want) <= tol
    assert got['intra_frechet'] == float(np.mean(got['frechet_class'][:2]))
    # the three refusals, and the pair with nothing to compare
    with pytest.raises(ValueError, match='classes'):
        intra_frechet(a, ClassStatistics(b.n[:4], b.mean[:4], b.cov[:4]))
    with pytest.raises(ValueError, match='features'):
        intra_frechet(a, ClassStatistics(b.n, b.mean[:, :4], b.cov[:, :4, :4]))
    with pytest.raises(ValueError, match='different classifiers'):
        intra_frechet(ClassStatistics(a.n, a.mean, a.cov, 'x'), ClassStatistics(b.n, b.mean, b.cov, 'y'))
    intra_frechet(ClassStatistics(a.n, a.mean, a.cov, 'x'), b)          # one side synthetic: fine
    fc, lc = _labelled([0, 0, 60, 55, 0], d, seed=4)
    with pytest.raises(ValueError, match='no class has 2 rows'):
        intra_frechet(a, ClassStatistics.from_moments(*_raw(fc, lc, 5)))          # a: classes 0, 1, 4; the other side: 2, 3


# ----------------------------------------------------------------------------------------------------- the stand-ins
def test_stand_ins_segment_by_label_and_count_first_maxima():
    from tests import class_stats_cpu_kernels as C
    f, lab = _labelled([20, 0, 17, 20], 5, seed=5, offset=1.0)
    lab[[3, 30]] = [-1, 4]                                   # out of range: belong to no class
    cnt = torch.zeros(4, dtype=torch.int64)
    s1, s2 = torch.zeros(4, 5, dtype=torch.float64), torch.zeros(4, 5, 5, dtype=torch.float64)
    for r0 in range(0, 57, 9):
        C.class_moments_accum(torch.from_numpy(f[r0:r0 + 9]), torch.from_numpy(lab[r0:r0 + 9]), cnt, s1, s2)
    assert cnt.tolist() == [int((lab == c).sum()) for c in range(4)] and cnt.sum().item() == 55
    for c in range(4):
        r1, r2 = FO.reference_moments(f[lab == c])
        b1, b2 = FO.moment_bound(f[lab == c])
        assert (np.abs(s1[c].numpy() - r1) <= b1).all() and (np.abs(s2[c].numpy() - r2) <= b2).all()
    z = np.random.RandomState(6).randn(57, 4).astype(np.float32)
    z[5, [1, 3]] = 9.0                                       # a tie: the first maximum
    conf = torch.zeros(4, 4, dtype=torch.int64)
    C.confusion_accum(torch.from_numpy(z), torch.from_numpy(lab), conf)
    want = np.zeros((4, 4), np.int64)
    ok = (lab >= 0) & (lab < 4)
    np.add.at(want, (lab[ok], z.argmax(axis=1)[ok]), 1)
    assert np.array_equal(conf.numpy(), want) and conf.sum().item() == 55 and z[5].argmax() == 1
    with pytest.raises(NotImplementedError):
        C.confusion_accum(torch.zeros(2, 33), torch.zeros(2, dtype=torch.int32), torch.zeros(33, 33, dtype=torch.int64))


# ----------------------------------------------------------------------------------------------------- ClassifierScore
def _features(tr, images, chunk):
    import ctgan_amd.ct_cifar as M
    data = torch.from_numpy(images)
    out = []
    for r0 in range(0, len(images), chunk):
        idx = torch.arange(r0, min(r0 + chunk, len(images)), dtype=torch.int32)
        x = tr.gather_fixed(idx, data=data)
        out.append(tr._averaged(lambda: M._classifier(x, deterministic=True, features=True), True))
    return torch.cat(out).numpy()


def test_scoring_a_labelled_set_with_a_class_reference(class_stats_kernels, tmp_path):
    import ctgan_amd.ct_cifar as M
    from ctgan_amd.score_cifar import ClassifierScore, ClassStatistics, intra_frechet
    M.configure(**O.SMALL)
    tr = O.classifier_trainer()
    scorer = ClassifierScore(tr)
    images, other = O.random_images(90, seed=9), O.random_images(70, seed=10)
    lab_ref = (np.arange(90) % 10).astype(np.int32)
    lab = np.random.RandomState(1).randint(0, 9, 70).astype(np.int32)          # class 9 absent from the scored set
    ref = scorer.class_statistics(images, lab_ref, chunk=40)
    f = _features(tr, images, 40)
    assert ref.classes == 10 and ref.width == 8 and ref.n.tolist() == [9] * 10 and ref.classifier == scorer.fingerprint()
    for c in range(10):
        _, mean, cov = FO.two_pass_statistics(f[lab_ref == c])
        dmean, dcov = FO.statistics_bound(f[lab_ref == c])
        assert (np.abs(ref.mean[c] - mean) <= dmean).all() and (np.abs(ref.cov[c] - cov) <= dcov).all()
    plain = scorer.score(other, labels=lab, splits=4, chunk=25)
    assert set(plain) == set(SCORE_KEYS)                                        # without the option: exactly today's five
    path = str(tmp_path / 'cls.npz')
    ref.save(path)
    scorer.set_class_reference(path)
    got = scorer.score(other, labels=lab, splits=4, chunk=25)
    assert set(got) == set(SCORE_KEYS) | set(CLASS_KEYS)
    for k in SCORE_KEYS:
        assert np.array_equal(np.asarray(got[k]), np.asarray(plain[k])), k
    assert got['n_class'].dtype == np.int64 and np.array_equal(got['n_class'], np.bincount(lab, minlength=10)) and got['n_class'].sum() == 70
    conf = got['confusion']
    assert conf.dtype == np.int64 and conf.shape == (10, 10) and conf.sum() == 70
    assert np.array_equal(conf.sum(axis=0), got['hist']) and np.array_equal(conf.sum(axis=1), got['n_class'])
    assert np.trace(conf) / 70 == got['acc']
    assert np.isnan(got['acc_class'][9]) and np.array_equal(got['acc_class'][:9], np.diag(conf)[:9] / got['n_class'][:9])
    fo = _features(tr, other, 25)
    assert np.isnan(got['frechet_class'][9])
    seen = [c for c in range(9) if got['n_class'][c] >= 2]
    for c in seen:
        want = FO.features_distance(fo[lab == c], f[lab_ref == c])
        tol, _ = FO.distance_tolerance(fo[lab == c], f[lab_ref == c])
        assert abs(got['frechet_class'][c] - want) <= tol, c
    assert got['intra_frechet'] == float(np.mean(got['frechet_class'][seen]))
    assert got['intra_frechet'] == intra_frechet(scorer.class_statistics(other, lab, chunk=25), ref)['intra_frechet']
    # beside a pooled reference: 'frechet' by its own path, unchanged
    pooled = scorer.statistics(images, chunk=40)
    scorer.set_class_reference(None)
    scorer.set_reference(pooled)
    only = scorer.score(other, labels=lab, splits=4, chunk=25)
    scorer.set_class_reference(ref)
    both = scorer.score(other, labels=lab, splits=4, chunk=25)
    assert set(both) == set(SCORE_KEYS) | set(CLASS_KEYS) | {'frechet'} and both['frechet'] == only['frechet']
    assert np.array_equal(both['frechet_class'], got['frechet_class'], equal_nan=True) and np.array_equal(both['confusion'], conf)
    scorer.set_reference(None)
    # no labels: refused; a label out of range: refused after the copy
    with pytest.raises(ValueError, match='no labels'):
        scorer.score(other, splits=4)
    bad = lab.copy()
    bad[3] = 10
    with pytest.raises(ValueError, match='69 of 70 rows'):
        scorer.score(other, labels=bad, splits=4)
    with pytest.raises(ValueError, match='69 of 70 rows'):
        scorer.class_statistics(other, bad)
    # a reference of another classifier, of none, of another width or class count is refused
    scorer.set_class_reference(None)
    with pytest.raises(ValueError, match='another classifier'):
        scorer.set_class_reference(ClassStatistics(ref.n, ref.mean, ref.cov, 'f' * 64))
    with pytest.raises(ValueError, match='do not record'):
        scorer.set_class_reference(ClassStatistics(ref.n, ref.mean, ref.cov))
    with pytest.raises(ValueError, match='class reference features'):
        scorer.set_class_reference(ClassStatistics(ref.n, ref.mean[:, :4], ref.cov[:, :4, :4], ref.classifier))
    with pytest.raises(ValueError, match='reference classes'):
        scorer.set_class_reference(ClassStatistics(ref.n[:5], ref.mean[:5], ref.cov[:5], ref.classifier))
    assert scorer.class_reference is None and set(scorer.score(other, labels=lab, splits=4)) == set(SCORE_KEYS)
    scorer.set_class_reference(ref)
    idx4 = lambda *v: torch.tensor(v, dtype=torch.int32)          # noqa: E731
    tr.d_opt.set_lr(0.05)
    tr.d_body_idx(idx4(0, 5, 7, 2), idx4(1, 2, 3, 4), idx4(7, 6, 3, 1))          # one classifier step: the averaged parameters move
    with pytest.raises(ValueError, match='another classifier'):
        scorer.score(other, labels=lab, splits=4)
    with pytest.raises(ValueError, match='another classifier'):
        ClassifierScore(tr, class_reference=ref)


@pytest.mark.parametrize('name', ['resnet', 'cifar'])
def test_generator_scoring_with_a_class_reference(class_stats_kernels, tmp_path, monkeypatch, name):
    import ctgan_amd.ct_cifar as M
    import ctgan_amd.kernels as K
    import ctgan_amd.tflib as lib
    from ctgan_amd import evaluate
    from ctgan_amd.score_cifar import intra_frechet
    M.configure(**O.SMALL)
    scorer, _, _, _ = _checkpoint_scorer(tmp_path)
    ref = scorer.class_statistics(O.random_images(80, seed=3), (np.arange(80) % 10).astype(np.int32), chunk=30)
    long_name = 'gan_cifar_resnet' if name == 'resnet' else 'gan_cifar'
    case = H.Case(lib, name, 16 if name == 'resnet' else 8, 4, 'cpu')
    try:
        gan = case.trainer()
        stream = evaluate.eval_stream(gan)
        c0 = int(stream.ctr.item())
        before = H.snapshot(lib, gan)
        plain = scorer.score_generator(gan, 300, chunk=200)
        scorer.set_class_reference(ref)
        stream.ctr.fill_(c0)
        if name == 'cifar':                                                     # an unconditional generator: refused before any launch
            launched = []
            for fn in ('score_input', 'score_accum', 'class_moments_accum', 'confusion_accum'):
                monkeypatch.setattr(K, fn, lambda *a, _fn=fn, **kw: launched.append(_fn))
            for call in (lambda: scorer.score_generator(gan, 300, chunk=200), lambda: scorer.class_statistics_generator(gan, 300)):
                with pytest.raises(ValueError, match='no labels'):
                    call()
            assert not launched and int(stream.ctr.item()) == c0
            return
        got = scorer.score_generator(gan, 300, chunk=200)
        assert int(stream.ctr.item()) == c0 + 2
        H.assert_same(before, H.snapshot(lib, gan))                             # training stream, weights, optimizer state
        assert set(got) == set(SCORE_KEYS) | set(CLASS_KEYS)
        for k in SCORE_KEYS:
            assert np.array_equal(np.asarray(got[k]), np.asarray(plain[k])), k
        conf = got['confusion']
        assert conf.sum() == 300 and np.array_equal(conf.sum(axis=0), got['hist']) and np.trace(conf) / 300 == got['acc']
        assert np.array_equal(conf.sum(axis=1), got['n_class']) and got['n_class'].sum() == 300
        stream.ctr.fill_(c0)
        stats = scorer.class_statistics_generator(gan, 300, chunk=200)
        H.assert_same(before, H.snapshot(lib, gan))
        assert np.array_equal(stats.n, got['n_class']) and stats.classifier == ref.classifier
        want = intra_frechet(stats, ref)
        assert got['intra_frechet'] == want['intra_frechet'] and np.array_equal(got['frechet_class'], want['frechet_class'], equal_nan=True)
        stream.ctr.fill_(c0)
        scorer.set_class_reference(None)
        pooled = scorer.statistics_generator(gan, 300, chunk=200)               # the same draws, pooled
        assert stats.pooled().n == pooled.n == 300
        # the loops' hook writes `intra_frechet` only when a class reference is set
        monkeypatch.setitem(evaluate.SCORE_SAMPLES, long_name, 200)
        ev = evaluate.Evaluator(gan)
        rows = {}
        for with_ref in (True, False):
            scorer.set_class_reference(ref if with_ref else None)
            stream.ctr.fill_(c0)
            s = _Series()
            evaluate.record_score(ev, s, scorer)
            rows[with_ref] = s.rows
        stream.ctr.fill_(c0)
        scorer.set_class_reference(ref)
        res = scorer.score_generator(gan, 200)
        assert rows[True] == rows[False] + [('intra_frechet', res['intra_frechet'])] and 'intra_frechet' not in dict(rows[False])
        lab = ((np.arange(100) * 7) % 10).astype(np.int32)                      # given labels are the conditioned labels
        stream.ctr.fill_(c0)
        given = scorer.score_generator(gan, 100, labels=lab)
        assert np.array_equal(given['n_class'], np.bincount(lab, minlength=10))
    finally:
        case.close()


# ----------------------------------------------------------------------------------------------------- the ABI
def test_entry_points_validate_before_any_launch():
    """Argument validation happens before a launch, so it is observable without a GPU."""
    import ctypes
    import ctgan_amd.kernels as K
    from ctgan_amd import _lib
    lib = _lib.lib
    rows = lib.ctgan_class_moments_max_rows()
    assert K.CLASS_MOMENTS_MAX_ROWS == rows >= 8192
    one = ctypes.c_void_p(8)                                 # a non-null, 8-byte aligned address; never dereferenced on these paths
    odd = ctypes.c_void_p(12)
    cm = lib.ctgan_class_moments_accum
    assert cm(one, one, rows + 1, 16, 3, one, one, one, None) == -2 and b'rows in one call' in lib.ctgan_last_error()
    assert cm(one, one, 8, 16, 33, one, one, one, None) == -2 and b'33 classes' in lib.ctgan_last_error()
    assert cm(one, one, 8, 1025, 3, one, one, one, None) == -2 and b'1025 features' in lib.ctgan_last_error()
    assert cm(one, one, 8, 0, 3, one, one, one, None) == -1 and b'class_moments_accum' in lib.ctgan_last_error()
    assert cm(one, one, 8, 16, 0, one, one, one, None) == -1
    assert cm(one, one, -1, 16, 3, one, one, one, None) == -1
    for null in range(5):                                    # a null pointer with rows to read
        args = [one] * 5
        args[null] = None
        assert cm(args[0], args[1], 8, 16, 3, args[2], args[3], args[4], None) == -1, null
    for at in range(3):
        args = [one] * 3
        args[at] = odd
        assert cm(one, one, 8, 16, 3, args[0], args[1], args[2], None) == -1 and b'aligned' in lib.ctgan_last_error()
    assert cm(None, None, 0, 16, 3, None, None, None, None) == 0
    assert cm(None, None, 0, 1024, 32, None, None, None, None) == 0
    cf = lib.ctgan_confusion_accum
    assert cf(one, one, 8, 33, one, None) == -2 and b'33 classes' in lib.ctgan_last_error()
    assert cf(one, one, 8, 0, one, None) == -1 and cf(one, one, -1, 10, one, None) == -1
    assert cf(None, one, 8, 10, one, None) == -1 and cf(one, None, 8, 10, one, None) == -1 and cf(one, one, 8, 10, None, None) == -1
    assert cf(one, one, 8, 10, odd, None) == -1 and b'aligned' in lib.ctgan_last_error()
    assert cf(None, None, 0, 10, None, None) == 0
