"""The per-class Frechet distance and the confusion matrix of conditional samples on the MI355X, end to end (`-m gpu`):
ctgan_amd.score_cifar's ClassStatistics / class reference path on a full-width CT classifier and a small gan_cifar_resnet, against the
two-pass restatement (tests/frechet_oracle.py) of the plain-pass features per class.  Every bound is derived there; the largest
observed error / bound ratios go to class_stats_err.json in the run-output directory (tests/score_cifar_oracle.py `report_dir`).

The file is named to be collected after tests/test_gpu_kernels.py, as tests/test_gpu_score_cifar_frechet.py is and for its reason."""
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import eval_helpers as H  # noqa: E402
from tests import frechet_oracle as FO  # noqa: E402
from tests import score_cifar_oracle as O  # noqa: E402
from tests.test_gpu_score_cifar import K, _full_width_trainer, clean  # noqa: E402,F401  (fixtures and helpers)
from tests.test_gpu_score_cifar_frechet import _ratio, _set_features  # noqa: E402

SCORE_KEYS = ('mean', 'std', 'splits', 'hist', 'acc')
CLASS_KEYS = ('frechet_class', 'intra_frechet', 'n_class', 'confusion', 'acc_class')
_RATIOS = {}


def _report(key, ratio):
    _RATIOS[key] = max(float(ratio), _RATIOS.get(key, 0.0))
    with open(os.path.join(O.report_dir(), 'class_stats_err.json'), 'w') as f:
        json.dump({'largest_error_over_bound': _RATIOS}, f, indent=1, sort_keys=True)


def test_class_statistics_of_a_labelled_uint8_set_on_the_full_width_classifier(K, clean):
    from ctgan_amd.score_cifar import ClassifierScore
    M = clean
    tr = _full_width_trainer(M)
    images = O.random_images(230, seed=5)
    labels = np.random.RandomState(2).randint(0, 10, 230).astype(np.int32)
    scorer = ClassifierScore(tr)
    stats = scorer.class_statistics(images, labels, chunk=100)
    f = _set_features(M, tr, images, 100)
    assert f.shape == (230, 128) and stats.classes == 10 and stats.width == 128 and stats.classifier == scorer.fingerprint()
    assert np.array_equal(stats.n, np.bincount(labels, minlength=10)) and stats.n.min() >= 2
    worst = 0.0
    for c in range(10):
        n, mean, cov = FO.two_pass_statistics(f[labels == c])
        dmean, dcov = FO.statistics_bound(f[labels == c])
        worst = max(worst, _ratio(np.abs(stats.mean[c] - mean), dmean), _ratio(np.abs(stats.cov[c] - cov), dcov))
        assert np.array_equal(stats.cov[c], stats.cov[c].T)
    print('full width, per class: largest |statistic - ref| / bound %.3e' % worst)
    _report('full_width_class_statistics_230', worst)
    assert worst <= 1.0
    # all classes together against the pooled path over the same set
    pooled, whole = stats.pooled(), scorer.statistics(images, chunk=100)
    n, mean, cov = FO.two_pass_statistics(f)
    dmean, dcov = FO.statistics_bound(f)
    q = max(_ratio(np.abs(pooled.mean - mean), dmean), _ratio(np.abs(pooled.cov - cov), dcov))
    qs = max(_ratio(np.abs(pooled.mean - whole.mean), dmean), _ratio(np.abs(pooled.cov - whole.cov), dcov))
    print('full width, pooled: |statistic - ref| / bound %.3e, |pooled - statistics()| / bound %.3e' % (q, qs))
    _report('full_width_pooled_230', max(q, qs))
    assert pooled.n == whole.n == n == 230 and q <= 1.0 and qs <= 1.0


def test_score_generator_with_a_class_reference_on_a_resnet_gan(K, clean):
    import ctgan_amd.tflib as lib
    from ctgan_amd import evaluate
    from ctgan_amd.score_cifar import ClassifierScore, intra_frechet
    M = clean
    tr = _full_width_trainer(M)
    lib.delete_params_with_name('Generator.')          # the classifier trainer's own generator: its names are the GAN's
    scorer = ClassifierScore(tr)
    images = O.random_images(230, seed=5)
    labels = np.random.RandomState(2).randint(0, 10, 230).astype(np.int32)
    ref = scorer.class_statistics(images, labels, chunk=100)
    case = H.Case(lib, 'resnet', 16, 4, 'cuda')
    try:
        gan = case.trainer()
        stream = evaluate.eval_stream(gan)
        c0 = int(stream.ctr.item())
        before = H.snapshot(lib, gan)
        plain = scorer.score_generator(gan, 300)
        assert set(plain) == set(SCORE_KEYS)
        scorer.set_class_reference(ref)
        stream.ctr.fill_(c0)
        got = scorer.score_generator(gan, 300)
        H.assert_same(before, H.snapshot(lib, gan))                             # training stream, weights, optimizer state
        assert set(got) == set(SCORE_KEYS) | set(CLASS_KEYS)
        for k in SCORE_KEYS:                                                    # the score does not move by a bit
            assert np.array_equal(np.asarray(got[k]), np.asarray(plain[k])), k
        conf = got['confusion']
        assert conf.dtype == np.int64 and conf.shape == (10, 10) and conf.sum() == 300
        assert np.array_equal(conf.sum(axis=0), got['hist']) and np.trace(conf) / 300 == got['acc']
        stream.ctr.fill_(c0)
        drawn = torch.cat([lab for _, lab in evaluate.Evaluator(gan).score_draws(300)]).cpu().numpy()
        assert got['n_class'].dtype == np.int64 and np.array_equal(got['n_class'], np.bincount(drawn, minlength=10))
        assert np.array_equal(conf.sum(axis=1), got['n_class'])
        rows = conf.sum(axis=1)
        assert np.array_equal(got['acc_class'][rows > 0], (np.diag(conf) / np.maximum(rows, 1))[rows > 0]) and np.isnan(got['acc_class'][rows == 0]).all()
        stream.ctr.fill_(c0)
        stats = scorer.class_statistics_generator(gan, 300)
        H.assert_same(before, H.snapshot(lib, gan))
        want = intra_frechet(stats, ref)
        assert np.array_equal(got['frechet_class'], want['frechet_class'], equal_nan=True) and got['intra_frechet'] == want['intra_frechet']
        assert np.isfinite(got['intra_frechet']) and got['intra_frechet'] > 0
    finally:
        case.close()


def test_an_unconditional_generator_is_refused_before_any_launch(K, clean):
    import ctgan_amd.tflib as lib
    from ctgan_amd import evaluate
    from ctgan_amd.score_cifar import ClassifierScore
    M = clean
    tr = _full_width_trainer(M)
    lib.delete_params_with_name('Generator.')
    scorer = ClassifierScore(tr)
    scorer.set_class_reference(scorer.class_statistics(O.random_images(40, seed=6), (np.arange(40) % 10).astype(np.int32), chunk=40))
    with pytest.raises(ValueError, match='no labels'):
        scorer.score(O.random_images(40, seed=7), splits=4)
    case = H.Case(lib, 'cifar', 8, 4, 'cuda')
    try:
        gan = case.trainer()
        c0 = int(evaluate.eval_stream(gan).ctr.item())
        launched = []
        kept = {fn: getattr(K, fn) for fn in ('score_input', 'score_accum', 'class_moments_accum', 'confusion_accum')}
        try:
            for fn in kept:
                setattr(K, fn, lambda *a, _fn=fn, **kw: launched.append(_fn))
            with pytest.raises(ValueError, match='no labels'):
                scorer.score_generator(gan, 300)
            with pytest.raises(ValueError, match='no labels'):
                scorer.class_statistics_generator(gan, 300)
        finally:
            for fn, value in kept.items():
                setattr(K, fn, value)
        assert not launched and int(evaluate.eval_stream(gan).ctr.item()) == c0
    finally:
        case.close()
