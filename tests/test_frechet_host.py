"""The classifier Frechet distance of CIFAR-10 samples (ctgan_amd.score_cifar: FeatureStatistics, frechet_distance, the reference of
ClassifierScore) without a GPU: the distance against a closed form and the fp64 restatement (tests/frechet_oracle.py), and the host
logic on CPU stand-ins (tests/frechet_cpu_kernels.py)."""
import numpy as np
import pytest
import torch

from tests import eval_helpers as H
from tests import frechet_oracle as FO
from tests import score_cifar_oracle as O
from tests.frechet_cpu_kernels import frechet_kernels, score_cifar_kernels        # noqa: F401  (fixtures)
from tests.test_score_cifar_host import _Series, _checkpoint_scorer

SCORE_KEYS = ('mean', 'std', 'splits', 'hist', 'acc')


def _same_score(a, b):
    for k in SCORE_KEYS:
        assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])), k


# ----------------------------------------------------------------------------------------------------- the distance
def _commuting(D=16, seed=0):
    """Two fits whose covariances share an orthogonal eigenbasis -> (a, b, the closed form |d mu|^2 + sum (sqrt a_i - sqrt b_i)^2)."""
    from ctgan_amd.score_cifar import FeatureStatistics
    r = np.random.RandomState(seed)
    q, _ = np.linalg.qr(r.randn(D, D))
    ea, eb = r.uniform(0.1, 4.0, D), r.uniform(0.1, 4.0, D)
    ma, mb = r.randn(D), r.randn(D)
    a = FeatureStatistics(100, ma, (q * ea) @ q.T)
    b = FeatureStatistics(200, mb, (q * eb) @ q.T)
    return a, b, float(((ma - mb) ** 2).sum() + ((np.sqrt(ea) - np.sqrt(eb)) ** 2).sum())


def test_distance_equals_the_closed_form_for_commuting_covariances():
    """Both sides are exact expressions of the same number: they differ by the roundings of three D = 16 eigensolves and a few
    matrix products, each a small multiple of D 2^-53 relative to the traces (about 70 here): 1e-12 absolute leaves two orders."""
    from ctgan_amd.score_cifar import frechet_distance
    a, b, want = _commuting()
    got = frechet_distance(a, b)
    print('distance %.17g, closed form %.17g, d(a, a) %.3e' % (got, want, frechet_distance(a, a)))
    assert want > 5 and abs(got - want) <= 1e-12
    assert abs(frechet_distance(a, a)) <= 1e-12
    assert abs(got - FO.distance(a.mean, a.cov, b.mean, b.cov)) <= 1e-12          # ... and the independent restatement


def test_distance_is_symmetric_and_needs_two_rows():
    from ctgan_amd.score_cifar import FeatureStatistics, frechet_distance
    fa, fb = FO.gaussian_features(200, 16, seed=1), FO.gaussian_features(150, 16, seed=2, offset=0.5)
    a, b = (FeatureStatistics(*FO.two_pass_statistics(f)) for f in (fa, fb))
    ab, ba = frechet_distance(a, b), frechet_distance(b, a)
    assert ab > 0.1 and abs(ab - ba) <= 1e-12 * max(1.0, ab)
    one = FeatureStatistics.from_moments(1, fa[0].astype(np.float64), np.outer(fa[0], fa[0]).astype(np.float64))
    assert one.n == 1
    for pair in ((one, b), (a, one)):
        with pytest.raises(ValueError, match='at least 2 rows'):
            frechet_distance(*pair)
    with pytest.raises(ValueError, match='features'):
        frechet_distance(a, FeatureStatistics(*FO.two_pass_statistics(fa[:, :8])))


def test_singular_covariances_give_a_finite_distance():
    from ctgan_amd.score_cifar import FeatureStatistics, frechet_distance
    fa, fb = FO.gaussian_features(5, 16, seed=3), FO.gaussian_features(7, 16, seed=4)          # n < D: rank n - 1
    a, b = (FeatureStatistics(*FO.two_pass_statistics(f)) for f in (fa, fb))
    assert np.linalg.matrix_rank(a.cov) == 4
    d = frechet_distance(a, b)
    assert np.isfinite(d) and d > 0 and abs(d - FO.features_distance(fa, fb)) <= 1e-9 * d
    assert abs(frechet_distance(a, a)) <= 1e-6          # (sqrt of eigenvalues that are 0 up to 1e-16: 1e-8 each)


def test_statistics_from_raw_moments_equal_the_two_pass_ones():
    from ctgan_amd.score_cifar import FeatureStatistics
    f = FO.gaussian_features(300, 12, seed=5, offset=5.0)
    s1, s2 = FO.reference_moments(f)
    got = FeatureStatistics.from_moments(300, s1, s2)
    n, mean, cov = FO.two_pass_statistics(f)
    dmean, dcov = FO.statistics_bound(f)
    assert got.n == n and (np.abs(got.mean - mean) <= dmean).all() and (np.abs(got.cov - cov) <= dcov).all()
    assert dcov.max() < 1e-10


def test_save_load_round_trip(tmp_path):
    from ctgan_amd.score_cifar import FeatureStatistics
    n, mean, cov = FO.two_pass_statistics(FO.gaussian_features(40, 6))
    for tag in ('abc123', None):
        path = str(tmp_path / ('ref_%s.npz' % tag))
        FeatureStatistics(n, mean, cov, tag).save(path)
        back = FeatureStatistics.load(path)
        assert back.n == n and back.classifier == tag and np.array_equal(back.mean, mean) and np.array_equal(back.cov, cov)
        assert back.mean.dtype == back.cov.dtype == np.float64
    with pytest.raises(ValueError):
        FeatureStatistics(3, mean, cov[:3])


# ----------------------------------------------------------------------------------------------------- the stand-in
def test_stand_in_accumulates_the_raw_moments():
    from tests import frechet_cpu_kernels as C
    f = FO.gaussian_features(57, 10, seed=6, offset=5.0)
    s1, s2 = torch.zeros(10, dtype=torch.float64), torch.zeros(10, 10, dtype=torch.float64)
    for r0 in range(0, 57, 7):
        C.moments_accum(torch.from_numpy(f[r0:r0 + 7]), s1, s2)
    r1, r2 = FO.reference_moments(f)
    b1, b2 = FO.moment_bound(f)
    assert (np.abs(s1.numpy() - r1) <= b1).all() and (np.abs(s2.numpy() - r2) <= b2).all()
    with pytest.raises(NotImplementedError):
        C.moments_accum(torch.zeros(2, 1025), torch.zeros(1025, dtype=torch.float64), torch.zeros(1025, 1025, dtype=torch.float64))


# ----------------------------------------------------------------------------------------------------- ClassifierScore
def _features(scorer, tr, images, chunk):
    """The pooled features of the averaged classifier on a uint8 set, by the plain pass (no constant filters), in chunks."""
    import ctgan_amd.ct_cifar as M
    data = torch.from_numpy(images)
    out = []
    for r0 in range(0, len(images), chunk):
        idx = torch.arange(r0, min(r0 + chunk, len(images)), dtype=torch.int32)
        x = tr.gather_fixed(idx, data=data)
        out.append(tr._averaged(lambda: M._classifier(x, deterministic=True, features=True), True))
    return torch.cat(out).numpy()


def test_statistics_of_a_uint8_set_and_the_reference_rules(frechet_kernels, tmp_path):
    import ctgan_amd.ct_cifar as M
    from ctgan_amd.score_cifar import ClassifierScore, FeatureStatistics, frechet_distance
    M.configure(**O.SMALL)
    tr = O.classifier_trainer()
    scorer = ClassifierScore(tr)
    images, other = O.random_images(57, seed=9), O.random_images(40, seed=10)
    stats = scorer.statistics(images, chunk=20)
    f = _features(scorer, tr, images, 20)
    assert f.shape == (57, 8) and f.dtype == np.float32
    n, mean, cov = FO.two_pass_statistics(f)
    dmean, dcov = FO.statistics_bound(f)
    assert stats.n == n and (np.abs(stats.mean - mean) <= dmean).all() and (np.abs(stats.cov - cov) <= dcov).all()
    assert stats.classifier == scorer.fingerprint() and len(stats.classifier) == 64
    # without a reference: today's dict; with one: the same score keys, bit for bit, plus the distance
    labels = np.random.RandomState(1).randint(0, 10, 40).astype(np.int32)
    plain = scorer.score(other, labels=labels, splits=4, chunk=15)
    assert set(plain) == set(SCORE_KEYS)
    path = str(tmp_path / 'ref.npz')
    stats.save(path)
    scorer.set_reference(path)
    assert scorer.reference.n == 57
    got = scorer.score(other, labels=labels, splits=4, chunk=15)
    assert set(got) == set(SCORE_KEYS) | {'frechet'}
    _same_score(got, plain)
    want = FO.features_distance(_features(scorer, tr, other, 15), f)
    tol, _ = FO.distance_tolerance(_features(scorer, tr, other, 15), f)
    print('frechet %.17g, oracle %.17g, tolerance %.3e' % (got['frechet'], want, tol))
    assert abs(got['frechet'] - want) <= tol
    assert got['frechet'] == frechet_distance(scorer.statistics(other, chunk=15), stats)
    assert abs(scorer.score(images, splits=4, chunk=20)['frechet']) <= 2 * FO.distance_tolerance(f, f)[0] + 1e-12
    scorer.set_reference(None)
    assert set(scorer.score(other, splits=4)) == set(SCORE_KEYS)
    # a reference of another classifier, or of none, is refused: at set_reference and, when the classifier moves later, at the scoring
    with pytest.raises(ValueError, match='another classifier'):
        scorer.set_reference(FeatureStatistics(stats.n, stats.mean, stats.cov, 'f' * 64))
    with pytest.raises(ValueError, match='do not record'):
        scorer.set_reference(FeatureStatistics(stats.n, stats.mean, stats.cov))
    with pytest.raises(ValueError, match='reference features'):
        scorer.set_reference(FeatureStatistics(stats.n, stats.mean[:4], stats.cov[:4, :4], stats.classifier))
    assert scorer.reference is None
    scorer.set_reference(stats)
    idx4 = lambda *v: torch.tensor(v, dtype=torch.int32)          # noqa: E731
    tr.d_opt.set_lr(0.05)
    tr.d_body_idx(idx4(0, 5, 7, 2), idx4(1, 2, 3, 4), idx4(7, 6, 3, 1))          # one classifier step: the averaged parameters move
    with pytest.raises(ValueError, match='another classifier'):
        scorer.score(other, splits=4)
    with pytest.raises(ValueError, match='another classifier'):
        ClassifierScore(tr, reference=stats)
    with pytest.raises(ValueError):
        scorer.statistics(other[:, :, :16, :16])


@pytest.mark.parametrize('name', ['resnet', 'cifar'])
def test_generator_scoring_with_a_reference_changes_nothing_else(frechet_kernels, tmp_path, name):
    import ctgan_amd.ct_cifar as M
    import ctgan_amd.tflib as lib
    from ctgan_amd import evaluate
    from ctgan_amd.score_cifar import frechet_distance
    M.configure(**O.SMALL)
    scorer, _, _, _ = _checkpoint_scorer(tmp_path)
    ref = scorer.statistics(O.random_images(60, seed=3), chunk=25)
    long_name = 'gan_cifar_resnet' if name == 'resnet' else 'gan_cifar'
    case = H.Case(lib, name, 16 if name == 'resnet' else 8, 4, 'cpu')
    try:
        gan = case.trainer()
        stream = evaluate.eval_stream(gan)
        c0 = int(stream.ctr.item())
        before = H.snapshot(lib, gan)
        plain = scorer.score_generator(gan, 300, chunk=200)
        stream.ctr.fill_(c0)
        stats = scorer.statistics_generator(gan, 300, chunk=200)
        assert int(stream.ctr.item()) == c0 + 2                                 # one step of the EVALUATION stream per generator call
        H.assert_same(before, H.snapshot(lib, gan))                             # training stream, weights, optimizer state
        assert stats.n == 300 and stats.classifier == ref.classifier
        scorer.set_reference(ref)
        stream.ctr.fill_(c0)
        got = scorer.score_generator(gan, 300, chunk=200)
        H.assert_same(before, H.snapshot(lib, gan))
        assert set(got) == set(SCORE_KEYS) | {'frechet'}
        _same_score(got, plain)
        assert np.isfinite(got['frechet']) and got['frechet'] == frechet_distance(stats, ref)
        # the loops' hook writes `frechet` only when a reference is set
        evaluate.SCORE_SAMPLES[long_name], kept = 200, evaluate.SCORE_SAMPLES[long_name]
        try:
            ev = evaluate.Evaluator(gan)
            rows = {}
            for with_ref in (True, False):
                scorer.set_reference(ref if with_ref else None)
                stream.ctr.fill_(c0)
                s = _Series()
                evaluate.record_score(ev, s, scorer)
                rows[with_ref] = s.rows
            stream.ctr.fill_(c0)
            scorer.set_reference(ref)
            res = scorer.score_generator(gan, 200)
        finally:
            evaluate.SCORE_SAMPLES[long_name] = kept
        assert rows[True] == rows[False] + [('frechet', res['frechet'])]
        assert 'frechet' not in dict(rows[False]) and len(rows[False]) == (3 if name == 'resnet' else 1)
        if name == 'resnet':                                                    # given labels are used as score_generator uses them
            lab = ((np.arange(100) * 7) % 10).astype(np.int32)
            stream.ctr.fill_(c0)
            a = scorer.statistics_generator(gan, 100, labels=lab)
            stream.ctr.fill_(c0)
            assert scorer.score_generator(gan, 100, labels=lab)['frechet'] == frechet_distance(a, ref)
            with pytest.raises(ValueError, match='labels'):
                scorer.statistics_generator(gan, 100, labels=lab[:50])
        with pytest.raises(ValueError):
            scorer.score_generator(gan, 1, splits=1)                            # one sample has no covariance
    finally:
        case.close()


def test_other_image_sizes_are_refused_by_the_statistics_too(frechet_kernels, tmp_path):
    import ctgan_amd.ct_cifar as M
    import ctgan_amd.tflib as lib
    M.configure(**O.SMALL)
    scorer, _, _, _ = _checkpoint_scorer(tmp_path)
    case = H.Case(lib, 'mnist', 4, 4, 'cpu')
    try:
        with pytest.raises(ValueError, match='are not 3x32x32 images'):
            scorer.statistics_generator(case.trainer(), 100)
    finally:
        case.M.configure()
        lib.delete_params_with_name('Generator')
        lib.delete_params_with_name('Discriminator')


# ----------------------------------------------------------------------------------------------------- the ABI
def test_moments_entry_point_validates_before_any_launch():
    """Argument validation happens before a launch, so it is observable without a GPU."""
    from ctgan_amd import _lib
    lib = _lib.lib
    assert lib.ctgan_moments_accum(None, 8, 0, None, None, None) == -1 and b'moments_accum' in lib.ctgan_last_error()
    assert lib.ctgan_moments_accum(None, -1, 192, None, None, None) == -1
    assert lib.ctgan_moments_accum(None, 8, 192, None, None, None) == -1             # null pointers with rows to read
    assert lib.ctgan_moments_accum(None, 8, 1025, None, None, None) == -2 and b'1025 features' in lib.ctgan_last_error()
    assert lib.ctgan_moments_accum(None, 0, 192, None, None, None) == 0
    assert lib.ctgan_moments_accum(None, 0, 1024, None, None, None) == 0
