"""Precision and recall of CIFAR-10 samples (ctgan_amd.score_cifar: FeatureSet, precision_recall, the manifold of ClassifierScore)
without a GPU: the fp64 oracle's own checks (tests/knn_oracle.py), and the host logic on CPU stand-ins (tests/knn_cpu_kernels.py)."""
import numpy as np
import pytest
import torch

from tests import eval_helpers as H
from tests import knn_oracle as KO
from tests import score_cifar_oracle as O
from tests.knn_cpu_kernels import frechet_kernels, knn_kernels, score_cifar_kernels        # noqa: F401  (fixtures)
from tests.test_score_cifar_host import _Series, _checkpoint_scorer

SCORE_KEYS = ('mean', 'std', 'splits', 'hist', 'acc')
MANIFOLD_KEYS = ('precision', 'recall', 'nn_dist', 'nn_zero')


def _same_score(a, b):
    for k in SCORE_KEYS:
        assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])), k


# ----------------------------------------------------------------------------------------------------- the oracle
@pytest.mark.parametrize('seed', [7, 11])
@pytest.mark.parametrize('shape', KO.CASES)
def test_oracle_decides_every_row_of_every_case(shape, seed):
    """The GPU test leaves undecidable rows and ambiguous neighbours out of its comparisons: on these inputs there are none, so nothing
    hides there.  The device's expression in numpy's order stays within a tenth of the derived bound."""
    c = KO.case(*shape, seed=seed)
    m, n, d, k, _ = shape
    assert c.decidable.all() and c.nn_sure.all()
    assert c.back is None or c.back_decidable.all()
    ratio = np.abs(KO.gemm_form(c.a, c.b) - c.dist)
    live = c.e_dist > 0                                        # (numpy's form need not give the exact 0 of identical rows: the device's does)
    q = float((ratio[live] / c.e_dist[live]).max()) if live.any() else 0.0
    print('%s seed %d: precision %.3f recall %s, gemm form / bound %.3f' % (shape, seed, c.precision, c.recall, q))
    assert q <= 0.10
    if shape in KO.MULTI_ROW:
        assert 0.05 < c.precision < 0.999 and 0.05 < c.recall < 0.999
    if c.planted:
        assert (c.r2_b == 0).sum() == k + 1 and (c.r2_b[10:11 + k] == 0).all() and (c.e_r2_b[10:11 + k] == 0).all()
        zero = [0, 1, 2, 3, 4, KO.COPY_OF_B10]
        assert (c.nn_d2[zero] == 0).all() and (c.nn_d2 == 0).sum() == 6 and c.covered[zero].all()
        assert c.nn_idx[KO.COPY_OF_B10] == 10 and list(c.nn_idx[:5]) == [0, 1, 2, 3, 4]


def test_oracle_radii_exclude_self_by_index_not_by_distance():
    f = np.array([[0.], [0.], [3.], [7.]], dtype=np.float32)          # rows 0 and 1 identical: each is the other's neighbour at 0
    r1, e1 = KO.radii(f, 1)
    assert list(r1) == [0., 0., 9., 16.] and e1[0] == e1[1] == 0 and e1[2] > 0
    assert list(KO.radii(f, 2)[0]) == [9., 9., 9., 49.]
    dist = KO.d2_direct(np.array([[-1.]], dtype=np.float32), f)      # 1, 1, 16, 64
    assert list(KO.nearest(dist)[1]) == [0]                           # the lowest index among equal distances
    assert list(KO.cover(dist, np.array([1., 0., 0., 0.]))) == [True] and list(KO.cover(dist, np.array([0.9, 0., -1., 0.]))) == [False]


def test_stand_ins_equal_the_oracle():
    from tests import knn_cpu_kernels as C
    for shape in KO.CASES[:6]:
        c = KO.case(*shape)
        a, b = torch.from_numpy(c.a), torch.from_numpy(c.b)
        r2 = C.knn_radii(b, c.k)
        assert np.array_equal(r2.numpy(), c.r2_b)
        covered, nn_d2, nn_idx = C.knn_cover(a, b, r2)
        assert np.array_equal(covered.numpy().astype(bool), c.covered) and np.array_equal(nn_d2.numpy(), c.nn_d2)
        assert np.array_equal(nn_idx.numpy(), c.nn_idx)
        none, d2, idx = C.knn_cover(a, b)
        assert none is None and torch.equal(d2, nn_d2) and torch.equal(idx, nn_idx)
    with pytest.raises(NotImplementedError):
        C.knn_radii(torch.zeros(20, 4), 9)
    with pytest.raises(ValueError):
        C.knn_radii(torch.zeros(3, 4), 3)


# ----------------------------------------------------------------------------------------------------- FeatureSet, precision_recall
def test_feature_set_round_trip_keeps_the_radii(knn_kernels, tmp_path, monkeypatch):
    import ctgan_amd.kernels as K
    from ctgan_amd.score_cifar import FeatureSet
    c = KO.case(57, 70, 10, 3, 0.0)
    fs = FeatureSet(c.b, 'abc123')
    assert fs.n == 70 and fs.width == 10
    calls = []
    radii = K.knn_radii
    monkeypatch.setattr(K, 'knn_radii', lambda f, k, out=None: calls.append(k) or radii(f, k, out))
    r3 = fs.radii(3)
    assert fs.radii(3) is r3 and calls == [3]                        # computed once
    assert np.array_equal(r3.numpy(), c.r2_b) and np.array_equal(fs.radii(1).numpy(), KO.radii(c.b, 1)[0])
    for tag in ('abc123', None):
        path = str(tmp_path / ('set_%s.npz' % tag))
        FeatureSet(fs.features, tag, fs._radii).save(path)
        with np.load(path, allow_pickle=False) as z:
            assert sorted(z.files) == ['classifier', 'features', 'radii_1', 'radii_3', 'radii_k']
        back = FeatureSet.load(path)
        assert back.classifier == tag and back.features.dtype == torch.float32 and torch.equal(back.features, fs.features)
        del calls[:]
        assert torch.equal(back.radii(3), r3) and torch.equal(back.radii(1), fs.radii(1)) and calls == []          # the saved radii are used
        assert back.radii(2).shape == (70,) and calls == [2]
    with pytest.raises(ValueError, match='no 70-th'):
        fs.radii(70)
    with pytest.raises(ValueError):
        FeatureSet(np.zeros(5, dtype=np.float32))
    with pytest.raises(ValueError, match='radii'):
        FeatureSet(c.b, None, {3: np.zeros(5)})


def test_precision_recall_matches_the_oracle_and_refuses_mixed_sets(knn_kernels):
    from ctgan_amd.score_cifar import FeatureSet, precision_recall
    for shape in [(57, 70, 10, 3, 0.0), (65, 129, 17, 8, 5.0)]:
        c = KO.case(*shape)
        got = precision_recall(FeatureSet(c.a), FeatureSet(c.b), k=c.k)
        want = KO.precision_recall(c.a, c.b, c.k)
        assert set(got) == {'precision', 'recall', 'k', 'nn_dist', 'nn_zero'} and got == want
        assert got['precision'] == c.precision and got['recall'] == c.recall and got['nn_zero'] == 0
    c = KO.case(57, 70, 10, 3, 0.0)
    same = precision_recall(FeatureSet(c.b), FeatureSet(c.b.copy()), k=3)                   # a set against itself
    assert same == {'precision': 1.0, 'recall': 1.0, 'k': 3, 'nn_dist': 0.0, 'nn_zero': 70}
    even = precision_recall(FeatureSet(c.a[:56]), FeatureSet(c.b))                          # an even count: the mean of the two middle ones
    assert even['k'] == 3 and even['nn_dist'] == float(np.median(np.sqrt(c.nn_d2[:56])))
    with pytest.raises(ValueError, match='different classifiers'):
        precision_recall(FeatureSet(c.a, 'a' * 64), FeatureSet(c.b, 'b' * 64))
    assert precision_recall(FeatureSet(c.a, 'a' * 64), FeatureSet(c.b))['k'] == 3          # a synthetic set goes with any
    with pytest.raises(ValueError, match='10 and 8 features'):
        precision_recall(FeatureSet(c.a), FeatureSet(c.b[:, :8]))
    with pytest.raises(ValueError, match='neighbour'):
        precision_recall(FeatureSet(c.a[:3]), FeatureSet(c.b), k=3)
    with pytest.raises(ValueError, match='k = 9'):
        precision_recall(FeatureSet(c.a), FeatureSet(c.b), k=9)


# ----------------------------------------------------------------------------------------------------- ClassifierScore
def test_manifold_of_a_uint8_set_and_the_fingerprint_rules(knn_kernels, tmp_path):
    import ctgan_amd.ct_cifar as M
    from ctgan_amd.score_cifar import ClassifierScore, FeatureSet
    from tests.test_frechet_host import _features
    M.configure(**O.SMALL)
    tr = O.classifier_trainer()
    scorer = ClassifierScore(tr)
    images, other = O.random_images(57, seed=9), O.random_images(40, seed=10)
    fs = scorer.features(images, chunk=20)
    f = _features(scorer, tr, images, 20)
    assert fs.n == 57 and fs.width == 8 and np.array_equal(fs.features.numpy(), f)          # the rows `statistics` reads, bit for bit
    assert fs.classifier == scorer.fingerprint()
    plain = scorer.score(other, splits=4, chunk=15)
    assert set(plain) == set(SCORE_KEYS)
    path = str(tmp_path / 'manifold.npz')
    fs.radii(3)
    fs.save(path)
    scorer.set_manifold(path)
    assert scorer.manifold.n == 57 and scorer.manifold_k == 3 and 3 in scorer.manifold._radii
    got = scorer.score(other, splits=4, chunk=15)
    assert set(got) == set(SCORE_KEYS) | set(MANIFOLD_KEYS)
    _same_score(got, plain)
    want = KO.precision_recall(_features(scorer, tr, other, 15), f, 3)
    assert {k: got[k] for k in MANIFOLD_KEYS} == {k: want[k] for k in MANIFOLD_KEYS}
    own = scorer.score(images, splits=4, chunk=20)                       # the manifold's own images: every sample is a reference row
    assert own['precision'] == 1.0 and own['recall'] == 1.0 and own['nn_zero'] == 57 and own['nn_dist'] == 0.0
    # with a reference too: the Frechet distance of a scorer without a manifold, and both sets of keys
    scorer.set_manifold(None)
    scorer.set_reference(scorer.statistics(images, chunk=20))
    only_ref = scorer.score(other, splits=4, chunk=15)
    assert set(only_ref) == set(SCORE_KEYS) | {'frechet'}
    scorer.set_manifold(fs, k=2)
    both = scorer.score(other, splits=4, chunk=15)
    assert set(both) == set(SCORE_KEYS) | {'frechet'} | set(MANIFOLD_KEYS) and both['frechet'] == only_ref['frechet']
    assert both['precision'] == KO.precision_recall(_features(scorer, tr, other, 15), f, 2)['precision']
    scorer.set_reference(None)
    scorer.set_manifold(None)
    assert set(scorer.score(other, splits=4)) == set(SCORE_KEYS)
    # refusals: at set_manifold and, when the classifier moves later, at the scoring
    with pytest.raises(ValueError, match='another classifier'):
        scorer.set_manifold(FeatureSet(fs.features, 'f' * 64))
    with pytest.raises(ValueError, match='do not record'):
        scorer.set_manifold(FeatureSet(fs.features))
    with pytest.raises(ValueError, match='manifold features'):
        scorer.set_manifold(FeatureSet(fs.features[:, :4], fs.classifier))
    with pytest.raises(ValueError, match='manifold_k'):
        scorer.set_manifold(fs, k=9)
    with pytest.raises(ValueError, match='neighbour'):
        scorer.set_manifold(FeatureSet(fs.features[:3], fs.classifier), k=3)
    assert scorer.manifold is None
    scorer.set_manifold(fs, k=3)
    with pytest.raises(ValueError, match='neighbour'):
        scorer.score(other[:3], splits=1)                                # three samples have no third other neighbour
    idx4 = lambda *v: torch.tensor(v, dtype=torch.int32)          # noqa: E731
    tr.d_opt.set_lr(0.05)
    tr.d_body_idx(idx4(0, 5, 7, 2), idx4(1, 2, 3, 4), idx4(7, 6, 3, 1))          # one classifier step: the averaged parameters move
    with pytest.raises(ValueError, match='another classifier'):
        scorer.score(other, splits=4)
    with pytest.raises(ValueError, match='another classifier'):
        ClassifierScore(tr, manifold=fs)
    with pytest.raises(ValueError):
        scorer.features(other[:, :, :16, :16])


@pytest.mark.parametrize('name', ['resnet', 'cifar'])
def test_generator_scoring_with_a_manifold_changes_nothing_else(knn_kernels, tmp_path, name):
    import ctgan_amd.ct_cifar as M
    import ctgan_amd.tflib as lib
    from ctgan_amd import evaluate
    from ctgan_amd.score_cifar import precision_recall
    M.configure(**O.SMALL)
    scorer, _, _, _ = _checkpoint_scorer(tmp_path)
    ref = scorer.features(O.random_images(60, seed=3), chunk=25)
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
        assert int(stream.ctr.item()) == c0 + 2                                 # one step of the EVALUATION stream per generator call
        H.assert_same(before, H.snapshot(lib, gan))                             # training stream, weights, optimizer state
        assert feats.n == 300 and feats.classifier == ref.classifier
        scorer.set_manifold(ref)
        stream.ctr.fill_(c0)
        got = scorer.score_generator(gan, 300, chunk=200)
        H.assert_same(before, H.snapshot(lib, gan))
        assert set(got) == set(SCORE_KEYS) | set(MANIFOLD_KEYS)
        _same_score(got, plain)
        want = precision_recall(feats, ref, k=3)
        assert {k: got[k] for k in MANIFOLD_KEYS} == {k: want[k] for k in MANIFOLD_KEYS}
        assert want == KO.precision_recall(feats.features.numpy(), ref.features.numpy(), 3)
        # the loops' hook writes the three series only when a manifold is set
        evaluate.SCORE_SAMPLES[long_name], kept = 200, evaluate.SCORE_SAMPLES[long_name]
        try:
            ev = evaluate.Evaluator(gan)
            rows = {}
            for with_manifold in (True, False):
                scorer.set_manifold(ref if with_manifold else None)
                stream.ctr.fill_(c0)
                s = _Series()
                evaluate.record_score(ev, s, scorer)
                rows[with_manifold] = s.rows
            stream.ctr.fill_(c0)
            scorer.set_manifold(ref)
            res = scorer.score_generator(gan, 200)
        finally:
            evaluate.SCORE_SAMPLES[long_name] = kept
        assert rows[True] == rows[False] + [(k, res[k]) for k in ('precision', 'recall', 'nn_dist')]
        assert not set(MANIFOLD_KEYS) & set(dict(rows[False])) and len(rows[False]) == (3 if name == 'resnet' else 1)
        if name == 'resnet':
            lab = ((np.arange(100) * 7) % 10).astype(np.int32)
            with pytest.raises(ValueError, match='labels'):
                scorer.features_generator(gan, 100, labels=lab[:50])
    finally:
        case.close()


# ----------------------------------------------------------------------------------------------------- the ABI
def test_knn_entry_points_validate_before_any_launch():
    """Argument validation happens before a launch, so it is observable without a GPU."""
    import ctgan_amd.kernels as K
    from ctgan_amd import _lib
    lib = _lib.lib
    assert K.KNN_MAX_K == lib.ctgan_knn_max_k() == KO.KNN_MAX_K >= 8
    assert lib.ctgan_knn_radii(None, 100, 16, 9, None, None) == -2 and b'k = 9' in lib.ctgan_last_error()
    assert lib.ctgan_knn_radii(None, 100, 1025, 3, None, None) == -2 and b'1025 features' in lib.ctgan_last_error()
    assert lib.ctgan_knn_radii(None, 3, 16, 3, None, None) == -1 and b'knn_radii' in lib.ctgan_last_error()          # n < k + 1
    assert lib.ctgan_knn_radii(None, 100, 16, 0, None, None) == -1
    assert lib.ctgan_knn_radii(None, 100, 16, 3, None, None) == -1                                                    # null pointers
    assert lib.ctgan_knn_cover(None, 5, None, 5, 1025, None, None, None, None, None) == -2
    assert lib.ctgan_knn_cover(None, 5, None, 0, 16, None, None, None, None, None) == -1
    assert lib.ctgan_knn_cover(None, 5, None, 5, 16, None, None, None, None, None) == -1                              # null pointers
    assert lib.ctgan_knn_cover(None, 0, None, 5, 16, None, None, None, None, None) == 0                               # no rows: a no-op
