"""Per-class precision, recall and kernel distance of conditional samples (ctgan_amd.score_cifar: labelled FeatureSets,
class_precision_recall, class_kernel_distance, the class manifold and class kernel reference of ClassifierScore) without a GPU: the
oracle's own checks (tests/class_manifold_oracle.py), and the host logic on CPU stand-ins (tests/class_manifold_cpu_kernels.py)."""
import ctypes
import math

import numpy as np
import pytest
import torch

from tests import class_manifold_oracle as CO
from tests import eval_helpers as H
from tests import score_cifar_oracle as O
from tests.class_manifold_cpu_kernels import (class_manifold_kernels, class_stats_kernels, frechet_kernels, kid_kernels,  # noqa: F401  (fixtures)
                                              knn_kernels, score_cifar_kernels)
from tests.test_score_cifar_host import _Series, _checkpoint_scorer

SCORE_KEYS = ('mean', 'std', 'splits', 'hist', 'acc')
CLASS_MANIFOLD_KEYS = ('precision_class', 'recall_class', 'nn_dist_class', 'nn_zero_class', 'n_class', 'n_class_reference', 'intra_precision',
                       'intra_recall')
CLASS_KERNEL_KEYS = ('kid_class', 'intra_kid', 'n_class', 'n_class_reference')


def _same(a, b):
    if a is None or b is None:
        return a is b
    return np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True)


def _sets(c):
    from ctgan_amd.score_cifar import FeatureSet
    return FeatureSet(c.a, labels=c.la, classes=c.classes), FeatureSet(c.b, labels=c.lb, classes=c.classes)


# ----------------------------------------------------------------------------------------------------- the oracle
@pytest.mark.parametrize('name', CO.NAMES)
def test_oracle_decides_every_row_of_every_class(name):
    """The GPU test leaves undecidable rows and ambiguous neighbours out of its comparisons: on these inputs there are none, so nothing
    hides there; the NaN rules hold; and the sizes are the ones the case states."""
    c = CO.case(name)
    base = CO.VARIANTS.get(name, (name,))[0]
    d, k, _, sa, sb = CO.CASES[base]
    outside = name == 'L4_outside'
    if not outside:
        assert [o.m for o in c.of] == sa and [o.n for o in c.of] == sb
    else:
        assert sum(o.m for o in c.of) == sum(sa) - len(CO.OUTSIDE['samples']) and sum(o.n for o in c.of) == sum(sb) - len(CO.OUTSIDE['reference'])
    left, rows = CO.undecidable(c.of)
    assert left == 0 and rows > 0
    assert all(o.nn_sure.all() for o in c.of if o.nn_sure is not None)
    r, kr = c.result, c.kernel
    for i, o in enumerate(c.of):
        assert np.isnan(r['precision_class'][i]) == (o.m == 0 or o.n < k + 1)
        assert np.isnan(r['recall_class'][i]) == (o.n == 0 or o.m < k + 1)
        assert np.isnan(r['nn_dist_class'][i]) == (o.m == 0 or o.n == 0)
        assert np.isnan(kr['kid_class'][i]) == (o.m < 2 or o.n < 2)
    print('%s: precision %s recall %s' % (name, np.round(r['precision_class'], 2), np.round(r['recall_class'], 2)))
    if name == 'L5_planted':
        assert (c.of[0].nn_d2 == 0).sum() == 6 and (c.of[0].r2_b == 0).sum() == k + 1 and (c.of[0].e_r2_b[10:11 + k] == 0).all()
    if name == 'L2':
        assert 0.3 < r['precision_class'].min() and r['precision_class'].max() < 0.6
        assert 0.7 < r['recall_class'].min() and r['recall_class'].max() < 0.85


def test_stand_ins_equal_the_oracle_class_by_class():
    import ctgan_amd.kernels as K
    from tests import class_manifold_cpu_kernels as C
    for name in ('L1', 'L3', 'L4_outside'):
        c = CO.case(name)
        a, b = torch.from_numpy(c.a), torch.from_numpy(c.b)
        (pa, sa), (pb, sb) = K.class_segments(torch.from_numpy(c.la), c.classes), K.class_segments(torch.from_numpy(c.lb), c.classes)
        fa, fb = a[pa].contiguous(), b[pb].contiguous()
        assert sa.dtype == torch.int32 and sa.tolist() == [int((c.la[(c.la >= 0)] < i).sum()) for i in range(c.classes + 1)]
        for i in range(c.classes):                                        # a stable sort: the class's rows in their original order
            assert torch.equal(fa[sa[i]:sa[i + 1]], a[torch.from_numpy(c.la == i)])
        r2 = C.knn_radii_seg(fb, sb, c.k)
        cov, d2, idx = C.knn_cover_seg(fa, sa, fb, sb, r2)
        for i, o in enumerate(c.of):
            rows, ref = slice(int(sa[i]), int(sa[i + 1])), slice(int(sb[i]), int(sb[i + 1]))
            assert np.array_equal(r2[ref].numpy(), o.r2_b) if o.r2_b is not None else bool(torch.isinf(r2[ref]).all())
            if o.m and o.n:
                assert np.array_equal(d2[rows].numpy(), o.nn_d2) and np.array_equal(idx[rows].numpy(), o.nn_idx)
                if o.covered is not None:
                    assert np.array_equal(cov[rows].numpy().astype(bool), o.covered)
            elif o.m:
                assert bool(torch.isinf(d2[rows]).all()) and bool((idx[rows] == -1).all()) and bool((cov[rows] == 0).all())
    vals = torch.arange(10, dtype=torch.float64)
    assert C.segment_sums(vals, torch.tensor([0, 0, 3, 10], dtype=torch.int64)).tolist() == [0.0, 3.0, 42.0]


# ----------------------------------------------------------------------------------------------------- FeatureSet
def test_feature_set_round_trip_with_labels_and_the_class_caches(class_manifold_kernels, tmp_path, monkeypatch):
    import ctgan_amd.kernels as K
    from ctgan_amd.score_cifar import FeatureSet
    c = CO.case('L1')
    fs = FeatureSet(c.b, 'abc123', labels=c.lb, classes=4)
    assert fs.classes == 4 and fs.labels.dtype == torch.int32
    calls = []
    for fn in ('knn_radii_seg', 'kernel_tile_sums_seg'):
        monkeypatch.setattr(K, fn, lambda *a, _f=getattr(K, fn), _n=fn, **kw: calls.append(_n) or _f(*a, **kw))
    feat, perm, seg = fs.by_class()
    assert fs.by_class()[0] is feat and seg.tolist() == [0, 5, 9, 74, 75] and torch.equal(feat, fs.features[perm])
    r3 = fs.class_radii(3)
    assert fs.class_radii(3) is r3 and calls == ['knn_radii_seg']                       # computed once
    assert np.array_equal(r3[:5].numpy(), c.of[0].r2_b) and np.array_equal(r3[9:74].numpy(), c.of[2].r2_b) and bool(torch.isinf(r3[74:]).all())
    tot = fs.class_kernel_totals()
    assert fs.class_kernel_totals() is tot and calls == ['knn_radii_seg', 'kernel_tile_sums_seg'] and tot.shape == (4,) and tot[3] == 0
    path = str(tmp_path / 'labelled.npz')
    fs.save(path)
    with np.load(path, allow_pickle=False) as z:
        assert sorted(z.files) == ['class_kernel_totals', 'class_radii_3', 'class_radii_k', 'classes', 'classifier', 'features', 'labels', 'radii_k']
    back = FeatureSet.load(path)
    del calls[:]
    assert back.classes == 4 and torch.equal(back.labels, fs.labels) and torch.equal(back.class_radii(3), r3)
    assert torch.equal(back.class_kernel_totals(), tot) and calls == []                  # the saved ones are used
    assert back.class_radii(1).shape == (75,) and calls == ['knn_radii_seg']
    # a set without labels writes exactly the keys it wrote before labels existed, and has no class view
    plain = FeatureSet(c.b, 'abc123')
    plain.radii(3)
    plain.save(path)
    with np.load(path, allow_pickle=False) as z:
        assert sorted(z.files) == ['classifier', 'features', 'radii_3', 'radii_k']
    assert FeatureSet.load(path).labels is None
    for call in (plain.by_class, lambda: plain.class_radii(3), plain.class_kernel_totals):
        with pytest.raises(ValueError, match='no labels'):
            call()
    with pytest.raises(ValueError, match='classes='):
        FeatureSet(c.b, labels=c.lb)
    with pytest.raises(ValueError, match='classes='):
        FeatureSet(c.b, labels=c.lb, classes=33)
    with pytest.raises(ValueError, match='int labels'):
        FeatureSet(c.b, labels=c.lb[:5], classes=4)
    with pytest.raises(ValueError, match='without labels'):
        FeatureSet(c.b, classes=4)
    with pytest.raises(ValueError, match='class radii'):
        FeatureSet(c.b, labels=c.lb, classes=4, class_radii={3: np.zeros(5)})


# ----------------------------------------------------------------------------------------------------- the two functions
@pytest.mark.parametrize('name', CO.NAMES)
def test_class_precision_recall_and_kernel_distance_match_the_oracle(class_manifold_kernels, name):
    from ctgan_amd.score_cifar import class_kernel_distance, class_precision_recall
    c = CO.case(name)
    sa, sb = _sets(c)
    got, want = class_precision_recall(sa, sb, k=c.k), c.result
    assert set(got) == set(CLASS_MANIFOLD_KEYS) | {'k'} and got['k'] == c.k
    for key in ('precision_class', 'recall_class', 'nn_dist_class', 'nn_zero_class', 'n_class', 'n_class_reference'):
        assert _same(got[key], want[key]), key                                         # the stand-ins' distances are the oracle's
    assert got['precision_class'].dtype == np.float64 and got['nn_zero_class'].dtype == np.int64 and got['n_class'].dtype == np.int64
    for key, per in (('intra_precision', 'precision_class'), ('intra_recall', 'recall_class')):
        assert got[key] == float(np.nanmean(got[per])) == want[key]
    kd, kw = class_kernel_distance(sa, sb), c.kernel
    assert set(kd) == set(CLASS_KERNEL_KEYS)
    assert np.array_equal(np.isnan(kd['kid_class']), np.isnan(kw['kid_class']))
    ok = ~np.isnan(kw['kid_class'])
    assert (np.abs(kd['kid_class'][ok] - kw['kid_class'][ok]) <= kw['e_kid_class'][ok]).all()
    assert kd['intra_kid'] == float(np.nanmean(kd['kid_class'])) and _same(kd['n_class'], kw['n_class'])
    assert _same(kd['n_class_reference'], kw['n_class_reference'])


def test_refusals_of_the_two_functions(class_manifold_kernels):
    from ctgan_amd.score_cifar import FeatureSet, class_kernel_distance, class_precision_recall
    c = CO.case('L1')
    sa, sb = _sets(c)
    for fn in (class_precision_recall, class_kernel_distance):
        with pytest.raises(ValueError, match='need labels'):
            fn(FeatureSet(c.a), sb)
        with pytest.raises(ValueError, match='need labels'):
            fn(sa, FeatureSet(c.b))
        with pytest.raises(ValueError, match='10 and 8 features'):
            fn(sa, FeatureSet(c.b[:, :8], labels=c.lb, classes=4))
        with pytest.raises(ValueError, match='4 and 5 classes'):
            fn(sa, FeatureSet(c.b, labels=c.lb, classes=5))
        with pytest.raises(ValueError, match='different classifiers'):
            fn(FeatureSet(c.a, 'a' * 64, labels=c.la, classes=4), FeatureSet(c.b, 'b' * 64, labels=c.lb, classes=4))
    with pytest.raises(ValueError, match='k = 9'):
        class_precision_recall(sa, sb, k=9)
    none = class_kernel_distance(FeatureSet(c.a[:4], labels=np.arange(4), classes=4), FeatureSet(c.b[:4], labels=np.arange(4), classes=4))
    assert np.isnan(none['kid_class']).all() and math.isnan(none['intra_kid'])          # no class with 2 rows on both sides


# ----------------------------------------------------------------------------------------------------- ClassifierScore
def test_scoring_a_labelled_set_with_the_class_references(class_manifold_kernels, tmp_path, monkeypatch):
    import ctgan_amd.ct_cifar as M
    from ctgan_amd.score_cifar import ClassifierScore, FeatureSet, class_kernel_distance, class_precision_recall
    M.configure(**O.SMALL)
    tr = O.classifier_trainer()
    scorer = ClassifierScore(tr)
    images, other = O.random_images(90, seed=9), O.random_images(70, seed=10)
    lab_ref = (np.arange(90) % 10).astype(np.int32)
    lab = np.random.RandomState(1).randint(0, 9, 70).astype(np.int32)          # class 9 absent from the scored set
    ref = scorer.features(images, chunk=40, labels=lab_ref)
    assert ref.classes == 10 and ref.labels.tolist() == lab_ref.tolist() and ref.classifier == scorer.fingerprint()
    assert scorer.features(images, chunk=40).labels is None
    plain = scorer.score(other, labels=lab, splits=4, chunk=25)
    assert set(plain) == set(SCORE_KEYS)
    path = str(tmp_path / 'class_manifold.npz')
    ref.class_radii(3)
    ref.save(path)
    scorer.set_class_manifold(path)
    assert scorer.class_manifold.classes == 10 and 3 in scorer.class_manifold._class_radii
    got = scorer.score(other, labels=lab, splits=4, chunk=25)
    assert set(got) == set(SCORE_KEYS) | set(CLASS_MANIFOLD_KEYS)
    for k in SCORE_KEYS:
        assert np.array_equal(np.asarray(got[k]), np.asarray(plain[k])), k
    samples = scorer.features(other, chunk=25, labels=lab)
    want = class_precision_recall(samples, ref, k=3)
    oracle = CO.class_precision_recall(samples.features.numpy(), lab, ref.features.numpy(), lab_ref, 10, 3)
    for k in CLASS_MANIFOLD_KEYS:
        assert _same(got[k], want[k]) and _same(got[k], oracle[k]), k
    assert np.isnan(got['precision_class'][9]) and got['n_class'][9] == 0 and np.array_equal(got['n_class'], np.bincount(lab, minlength=10))
    # the kernel reference alone, then both beside the pooled ones: every key by its own path, one device -> host copy
    scorer.set_class_manifold(None)
    scorer.set_class_kernel_reference(ref)
    only = scorer.score(other, labels=lab, splits=4, chunk=25)
    assert set(only) == set(SCORE_KEYS) | set(CLASS_KERNEL_KEYS)
    wk = class_kernel_distance(samples, ref)
    for k in CLASS_KERNEL_KEYS:
        assert _same(only[k], wk[k]), k
    scorer.set_class_manifold(ref, k=2)
    scorer.set_manifold(FeatureSet(ref.features, ref.classifier))
    scorer.set_kernel_reference(FeatureSet(ref.features, ref.classifier))
    copies = []
    cpu = torch.Tensor.cpu
    monkeypatch.setattr(torch.Tensor, 'cpu', lambda t, *a, **kw: copies.append(tuple(t.shape)) or cpu(t, *a, **kw))
    both = scorer.score(other, labels=lab, splits=4, chunk=25)
    monkeypatch.setattr(torch.Tensor, 'cpu', cpu)
    assert len(copies) == 1, copies                                                 # the scoring's one device -> host copy
    pooled = ('precision', 'recall', 'nn_dist', 'nn_zero', 'kid', 'kid_std', 'kid_blocks')
    assert set(both) == set(SCORE_KEYS) | set(CLASS_MANIFOLD_KEYS) | set(CLASS_KERNEL_KEYS) | set(pooled)
    scorer.set_class_manifold(None)
    scorer.set_class_kernel_reference(None)
    without = scorer.score(other, labels=lab, splits=4, chunk=25)
    for k in SCORE_KEYS + pooled:
        assert _same(both[k], without[k]), k
    assert _same(both['kid_class'], only['kid_class']) and _same(both['precision_class'], class_precision_recall(samples, ref, k=2)['precision_class'])
    scorer.set_manifold(None)
    scorer.set_kernel_reference(None)
    # no labels: refused; a label out of range: refused after the copy
    scorer.set_class_manifold(ref)
    with pytest.raises(ValueError, match='no labels'):
        scorer.score(other, splits=4)
    bad = lab.copy()
    bad[3] = 10
    with pytest.raises(ValueError, match='69 of 70 rows'):
        scorer.score(other, labels=bad, splits=4)
    scorer.set_class_manifold(None)
    scorer.set_class_kernel_reference(ref)
    with pytest.raises(ValueError, match='no labels'):
        scorer.score(other, splits=4)
    scorer.set_class_kernel_reference(None)
    # a set without labels, of another classifier, of none, of another width or class count is refused
    for setter, what in ((scorer.set_class_manifold, 'class manifold'), (scorer.set_class_kernel_reference, 'class kernel reference')):
        with pytest.raises(ValueError, match='no labels'):
            setter(FeatureSet(ref.features, ref.classifier))
        with pytest.raises(ValueError, match='another classifier'):
            setter(FeatureSet(ref.features, 'f' * 64, labels=lab_ref, classes=10))
        with pytest.raises(ValueError, match='do not record'):
            setter(FeatureSet(ref.features, labels=lab_ref, classes=10))
        with pytest.raises(ValueError, match='%s features' % what):
            setter(FeatureSet(ref.features[:, :4], ref.classifier, labels=lab_ref, classes=10))
        with pytest.raises(ValueError, match='%s classes' % what):
            setter(FeatureSet(ref.features, ref.classifier, labels=lab_ref, classes=11))
    with pytest.raises(ValueError, match='class_manifold_k'):
        scorer.set_class_manifold(ref, k=9)
    assert scorer.class_manifold is None and scorer.class_kernel_reference is None
    assert set(scorer.score(other, labels=lab, splits=4)) == set(SCORE_KEYS)
    scorer.set_class_manifold(ref)
    idx4 = lambda *v: torch.tensor(v, dtype=torch.int32)          # noqa: E731
    tr.d_opt.set_lr(0.05)
    tr.d_body_idx(idx4(0, 5, 7, 2), idx4(1, 2, 3, 4), idx4(7, 6, 3, 1))          # one classifier step: the averaged parameters move
    with pytest.raises(ValueError, match='another classifier'):
        scorer.score(other, labels=lab, splits=4)
    with pytest.raises(ValueError, match='another classifier'):
        ClassifierScore(tr, class_kernel_reference=ref)


@pytest.mark.parametrize('name', ['resnet', 'cifar'])
def test_generator_scoring_with_the_class_references(class_manifold_kernels, tmp_path, monkeypatch, name):
    import ctgan_amd.ct_cifar as M
    import ctgan_amd.kernels as K
    import ctgan_amd.tflib as lib
    from ctgan_amd import evaluate
    from ctgan_amd.score_cifar import class_kernel_distance, class_precision_recall
    M.configure(**O.SMALL)
    scorer, _, _, _ = _checkpoint_scorer(tmp_path)
    ref = scorer.features(O.random_images(80, seed=3), chunk=30, labels=(np.arange(80) % 10).astype(np.int32))
    long_name = 'gan_cifar_resnet' if name == 'resnet' else 'gan_cifar'
    case = H.Case(lib, name, 16 if name == 'resnet' else 8, 4, 'cpu')
    try:
        gan = case.trainer()
        stream = evaluate.eval_stream(gan)
        c0 = int(stream.ctr.item())
        before = H.snapshot(lib, gan)
        plain = scorer.score_generator(gan, 300, chunk=200)
        stream.ctr.fill_(c0)
        feats = scorer.features_generator(gan, 300, chunk=200)
        assert (feats.labels is not None) == (name == 'resnet')
        scorer.set_class_manifold(ref)
        scorer.set_class_kernel_reference(ref)
        stream.ctr.fill_(c0)
        if name == 'cifar':                                                     # an unconditional generator: refused before any launch
            launched = []
            for fn in ('score_input', 'score_accum', 'knn_cover_seg', 'kernel_tile_sums_seg'):
                monkeypatch.setattr(K, fn, lambda *a, _fn=fn, **kw: launched.append(_fn))
            with pytest.raises(ValueError, match='no labels'):
                scorer.score_generator(gan, 300, chunk=200)
            assert not launched and int(stream.ctr.item()) == c0
            return
        got = scorer.score_generator(gan, 300, chunk=200)
        assert int(stream.ctr.item()) == c0 + 2
        H.assert_same(before, H.snapshot(lib, gan))                             # training stream, weights, optimizer state
        assert set(got) == set(SCORE_KEYS) | set(CLASS_MANIFOLD_KEYS) | set(CLASS_KERNEL_KEYS)
        for k in SCORE_KEYS:
            assert np.array_equal(np.asarray(got[k]), np.asarray(plain[k])), k
        assert feats.classes == 10 and got['n_class'].sum() == 300 and np.array_equal(got['n_class'], np.bincount(feats.labels.numpy(), minlength=10))
        want = dict(class_precision_recall(feats, ref, k=3), **class_kernel_distance(feats, ref))
        for k in CLASS_MANIFOLD_KEYS + CLASS_KERNEL_KEYS:
            assert _same(got[k], want[k]), k
        # the loops' hook writes the three series only when the class references are set
        monkeypatch.setitem(evaluate.SCORE_SAMPLES, long_name, 200)
        ev = evaluate.Evaluator(gan)
        rows = {}
        for with_ref in (True, False):
            scorer.set_class_manifold(ref if with_ref else None)
            scorer.set_class_kernel_reference(ref if with_ref else None)
            stream.ctr.fill_(c0)
            s = _Series()
            evaluate.record_score(ev, s, scorer)
            rows[with_ref] = s.rows
        stream.ctr.fill_(c0)
        scorer.set_class_manifold(ref)
        scorer.set_class_kernel_reference(ref)
        res = scorer.score_generator(gan, 200)
        assert rows[True] == rows[False] + [(k, res[k]) for k in ('intra_precision', 'intra_recall', 'intra_kid')]
        assert not {'intra_precision', 'intra_recall', 'intra_kid'} & set(dict(rows[False]))
    finally:
        case.close()


# ----------------------------------------------------------------------------------------------------- the ABI
def test_grouped_entry_points_validate_before_any_launch():
    """Argument validation happens before a launch, so it is observable without a GPU."""
    import ctgan_amd.kernels as K
    from ctgan_amd import _lib
    lib = _lib.lib
    one, two, odd = ctypes.c_void_p(64), ctypes.c_void_p(128), ctypes.c_void_p(12)          # never dereferenced on these paths
    assert K.SEG_MAX_CLASSES == 32
    rs = lib.ctgan_knn_radii_seg
    assert rs(one, one, 33, 100, 16, 3, one, None) == -2 and b'33 classes' in lib.ctgan_last_error()
    assert rs(one, one, 0, 100, 16, 3, one, None) == -1 and b'knn_radii_seg' in lib.ctgan_last_error()
    assert rs(one, one, 10, 100, 1025, 3, one, None) == -2 and b'1025 features' in lib.ctgan_last_error()
    assert rs(one, one, 10, 100, 16, 9, one, None) == -2 and b'k = 9' in lib.ctgan_last_error()
    assert rs(one, one, 10, 100, 16, 0, one, None) == -1
    assert rs(None, one, 10, 100, 16, 3, one, None) == -1 and rs(one, None, 10, 100, 16, 3, one, None) == -1
    assert rs(one, one, 10, 100, 16, 3, None, None) == -1 and rs(one, one, 10, 100, 16, 3, odd, None) == -1
    assert rs(None, None, 10, 0, 16, 3, None, None) == 0                                                    # no rows: a no-op
    cs = lib.ctgan_knn_cover_seg
    assert cs(one, one, 5, one, one, 5, 33, 16, one, one, one, one, None) == -2 and b'33 classes' in lib.ctgan_last_error()
    assert cs(one, one, 5, one, one, 5, 0, 16, one, one, one, one, None) == -1
    assert cs(one, one, 5, one, one, 5, 10, 1025, one, one, one, one, None) == -2
    assert cs(None, one, 5, one, one, 5, 10, 16, one, one, one, one, None) == -1 and b'null pointer' in lib.ctgan_last_error()
    assert cs(one, None, 5, one, one, 5, 10, 16, one, one, one, one, None) == -1 and cs(one, one, 5, one, None, 5, 10, 16, one, one, one, one, None) == -1
    assert cs(one, one, 5, None, one, 5, 10, 16, one, one, one, one, None) == -1 and cs(one, one, 5, one, one, 5, 10, 16, one, None, one, one, None) == -1
    assert cs(one, one, 5, one, one, 5, 10, 16, odd, one, one, one, None) == -1 and b'aligned' in lib.ctgan_last_error()
    assert cs(one, one, 5, one, one, 5, 10, 16, one, one, odd, one, None) == -1
    assert cs(None, None, 0, None, None, 5, 10, 16, None, None, None, None, None) == 0                      # no rows: a no-op
    ts = lib.ctgan_kernel_tile_sums_seg
    assert ts(one, one, 5, two, one, 5, 33, 16, 1.0, 1.0, 0, one, one, None) == -2 and b'33 classes' in lib.ctgan_last_error()
    assert ts(one, one, 5, two, one, 5, 0, 16, 1.0, 1.0, 0, one, one, None) == -1
    assert ts(one, one, 5, two, one, 5, 10, 1025, 1.0, 1.0, 0, one, one, None) == -2 and b'1025 features' in lib.ctgan_last_error()
    assert ts(one, one, 0, two, one, 5, 10, 16, 1.0, 1.0, 0, one, one, None) == -1
    assert ts(one, one, 5, two, one, 5, 10, 16, 1.0, 1.0, 1, one, one, None) == -1 and b'exclude_diag' in lib.ctgan_last_error()      # a != b
    assert ts(one, one, 5, one, two, 5, 10, 16, 1.0, 1.0, 1, one, one, None) == -1 and b'exclude_diag' in lib.ctgan_last_error()      # seg_a != seg_b
    assert ts(None, one, 5, two, one, 5, 10, 16, 1.0, 1.0, 0, one, one, None) == -1 and b'null pointer' in lib.ctgan_last_error()
    assert ts(one, one, 5, two, one, 5, 10, 16, 1.0, 1.0, 0, None, one, None) == -1 and ts(one, one, 5, two, one, 5, 10, 16, 1.0, 1.0, 0, one, None, None) == -1
    assert ts(one, one, 5, two, one, 5, 10, 16, 1.0, 1.0, 0, one, odd, None) == -1 and b'aligned' in lib.ctgan_last_error()
    ss = lib.ctgan_segment_sums
    assert ss(one, one, -1, one, None) == -1 and ss(None, one, 3, one, None) == -1 and ss(one, None, 3, one, None) == -1
    assert ss(one, one, 3, None, None) == -1 and ss(odd, one, 3, one, None) == -1 and ss(None, None, 0, None, None) == 0
