"""The classifier Frechet distance of CIFAR-10 samples on the MI355X (`-m gpu`): csrc/moments.hip - ctgan_moments_accum against fp64
numpy on the same fp32 features - and ctgan_amd.score_cifar's FeatureStatistics / frechet_distance / reference path end to end against
the two-pass restatement (tests/frechet_oracle.py).

Every bound is derived there, none is tuned: the raw moments within the order-independent summation bound n 2^-52 |F|^T |F| (the
products are exact in fp64), mean and covariance within that bound propagated through (s2 - n mu mu^T) / (n - 1), the distance within
those propagated through the trace of the matrix square root with the oracle's own eigenvalues.  The largest observed error / bound
ratios go to frechet_err.json in the run-output directory (tests/score_cifar_oracle.py `report_dir`).

The file is named to be collected after tests/test_gpu_kernels.py: the graph-capture test below makes a GraphedTrainer, which creates a
capture stream, and the clock-probe test there depends on which hardware queue the next stream created in the process is given."""
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import eval_helpers as H  # noqa: E402
from tests import frechet_oracle as FO  # noqa: E402
from tests import score_cifar_oracle as O  # noqa: E402
from tests.test_gpu_score_cifar import K, _full_width_trainer, _gan_loop, clean  # noqa: E402,F401  (fixtures and helpers)

# (m, d, chunk): one element; one full tile with a row tail; a column tail inside one tile; three tiles with row, column and chunk tails;
# two tiles, the second one column wide; 192 features (12 tiles, 78 tile pairs) in one chunk, in three, and in one-row chunks
CASES = [(1, 1, 1), (3, 16, 3), (57, 10, 7), (301, 33, 97), (64, 17, 64), (1000, 192, 1000), (3000, 192, 1000), (130, 192, 1)]
SCORE_KEYS = ('mean', 'std', 'splits', 'hist', 'acc')
_RATIOS = {}


def _report(key, ratio):
    _RATIOS[key] = max(float(ratio), _RATIOS.get(key, 0.0))
    with open(os.path.join(O.report_dir(), 'frechet_err.json'), 'w') as f:
        json.dump({'largest_error_over_bound': _RATIOS}, f, indent=1, sort_keys=True)


def _ratio(err, bound):
    """max err / bound over the elements (an element with a zero bound must have a zero error)."""
    err, bound = np.asarray(err, dtype=np.float64), np.asarray(bound, dtype=np.float64)
    assert (err[bound == 0] == 0).all()
    return float((err[bound > 0] / bound[bound > 0]).max()) if (bound > 0).any() else 0.0


def _device_moments(K, f, chunk):
    m, d = f.shape
    fd = torch.from_numpy(f).cuda()
    s1 = torch.zeros(d, dtype=torch.float64, device='cuda')
    s2 = torch.zeros(d, d, dtype=torch.float64, device='cuda')
    for r0 in range(0, m, chunk):
        K.moments_accum(fd[r0:r0 + chunk], s1, s2)
    return s1, s2


# ----------------------------------------------------------------------------------------------------- the kernel
@pytest.mark.parametrize('offset', [0.0, 5.0])
@pytest.mark.parametrize('m,d,chunk', CASES)
def test_moments_match_fp64_within_the_summation_bound(K, m, d, chunk, offset):
    f = FO.gaussian_features(m, d, seed=m + d, offset=offset)
    s1, s2 = _device_moments(K, f, chunk)
    r1, r2 = FO.reference_moments(f)
    b1, b2 = FO.moment_bound(f)
    g1, g2 = s1.cpu().numpy(), s2.cpu().numpy()
    q1, q2 = _ratio(np.abs(g1 - r1), b1), _ratio(np.abs(g2 - r2), b2)
    print('m %d d %d chunk %d offset %g: |s1 - ref| / bound %.3e, |s2 - ref| / bound %.3e' % (m, d, chunk, offset, q1, q2))
    _report('moments_m%d_d%d_chunk%d_offset%g' % (m, d, chunk, offset), max(q1, q2))
    assert q1 <= 1.0 and q2 <= 1.0
    assert np.array_equal(g2, g2.T)                                             # exactly symmetric
    t1, t2 = _device_moments(K, f, chunk)                                       # the same chunking: the same bits
    assert torch.equal(s1, t1) and torch.equal(s2, t2)


def test_unsupported_and_bad_arguments_leave_the_state_untouched(K):
    s1 = torch.zeros(1025, dtype=torch.float64, device='cuda')
    s2 = torch.zeros(1025, 1025, dtype=torch.float64, device='cuda')
    with pytest.raises(NotImplementedError, match='1025 features'):
        K.moments_accum(torch.ones(4, 1025, device='cuda'), s1, s2)
    torch.cuda.synchronize()
    assert not s1.any().item() and not s2.any().item()
    s1, s2 = torch.full((16,), 3.0, dtype=torch.float64, device='cuda'), torch.full((16, 16), 3.0, dtype=torch.float64, device='cuda')
    K.moments_accum(torch.ones(0, 16, device='cuda'), s1, s2)                   # no rows: a successful no-op
    assert (s1 == 3).all().item() and (s2 == 3).all().item()
    with pytest.raises(AssertionError):
        K.moments_accum(torch.ones(4, 16, device='cuda'), s1, s2[:, :8])
    with pytest.raises(AssertionError):
        K.moments_accum(torch.ones(4, 16, device='cuda'), s1.float(), s2)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        K.moments_accum(torch.ones(4, 16), s1, s2)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        K.moments_accum(torch.ones(4, 16, device='cuda'), s1.cpu(), s2)
    torch.cuda.synchronize()
    assert (s1 == 3).all().item() and (s2 == 3).all().item()


@pytest.mark.parametrize('offset', [0.0, 5.0])
@pytest.mark.parametrize('d', [16, 33])
def test_distance_of_synthetic_features_matches_the_two_pass_oracle(K, d, offset):
    """n = 8 D Gaussian rows through a well-conditioned mixing matrix on both sides: raw moments on the device -> FeatureStatistics ->
    frechet_distance, against the two-pass distance of the same features."""
    from ctgan_amd.score_cifar import FeatureStatistics, frechet_distance
    fa = FO.gaussian_features(8 * d, d, seed=d, offset=offset)
    fb = FO.gaussian_features(8 * d + 5, d, seed=d + 1, offset=offset + 0.3)
    stats = []
    for f in (fa, fb):
        s1, s2 = _device_moments(K, f, 100)
        stats.append(FeatureStatistics.from_moments(f.shape[0], s1.cpu().numpy(), s2.cpu().numpy()))
        _, mean, cov = FO.two_pass_statistics(f)
        dmean, dcov = FO.statistics_bound(f)
        assert (np.abs(stats[-1].mean - mean) <= dmean).all() and (np.abs(stats[-1].cov - cov) <= dcov).all()
    got, want = frechet_distance(*stats), FO.features_distance(fa, fb)
    tol, info = FO.distance_tolerance(fa, fb)
    print('D %d offset %g: distance %.17g, oracle %.17g, |diff| %.3e, tolerance %.3e, %s' % (d, offset, got, want, abs(got - want), tol, info))
    _report('synthetic_distance_D%d_offset%g' % (d, offset), abs(got - want) / tol)
    assert info['lambda_min_product'] > 0.01 and tol < 1e-6 * want          # a well-conditioned case: the tolerance is a tight one
    assert abs(got - want) <= tol


# ----------------------------------------------------------------------------------------------------- end to end
def _plain_features(M, tr, x):
    """The pooled features of the averaged classifier by its plain deterministic pass (predict's, no constant filters)."""
    return tr._averaged(lambda: M._classifier(x, deterministic=True, features=True), True)


def _set_features(M, tr, images, chunk):
    data = torch.from_numpy(images).cuda()
    out = []
    for r0 in range(0, len(images), chunk):
        idx = torch.arange(r0, min(r0 + chunk, len(images)), dtype=torch.int32, device='cuda')
        out.append(_plain_features(M, tr, tr.gather_fixed(idx, data=data)))
    return torch.cat(out).cpu().numpy()


def test_statistics_of_a_uint8_set_on_the_full_width_classifier(K, clean):
    from ctgan_amd.score_cifar import ClassifierScore
    M = clean
    tr = _full_width_trainer(M)
    images = O.random_images(230, seed=5)
    scorer = ClassifierScore(tr)
    stats = scorer.statistics(images, chunk=100)
    f = _set_features(M, tr, images, 100)
    assert f.shape == (230, M.cfg.D_WIDTHS[-1]) and f.shape[1] == 128 and f.dtype == np.float32          # (the script's width: eight tiles)
    idx = torch.arange(100, dtype=torch.int32, device='cuda')                   # the constant-filter pass gives the same feature bits
    logits, feat = scorer._forward(tr.gather_fixed(idx, data=torch.from_numpy(images).cuda()), True)
    assert torch.equal(feat.cpu(), torch.from_numpy(f[:100])) and torch.equal(logits.cpu(), torch.from_numpy(O.predict_chunks(tr, images[:100], 100)))
    n, mean, cov = FO.two_pass_statistics(f)
    dmean, dcov = FO.statistics_bound(f)
    q1, q2 = _ratio(np.abs(stats.mean - mean), dmean), _ratio(np.abs(stats.cov - cov), dcov)
    var = np.diag(cov)
    print('full width: |mean - ref| / bound %.3e, |cov - ref| / bound %.3e; features mean^2 / var: median %.3g, max %.3g'
          % (q1, q2, np.median(mean ** 2 / var), (mean ** 2 / var).max()))
    _report('full_width_statistics_230', max(q1, q2))
    assert stats.n == n == 230 and q1 <= 1.0 and q2 <= 1.0
    assert np.array_equal(stats.cov, stats.cov.T) and stats.classifier == scorer.fingerprint()


def test_score_generator_with_a_reference_on_a_resnet_gan(K, clean):
    import ctgan_amd.tflib as lib
    from ctgan_amd import evaluate
    from ctgan_amd.score_cifar import ClassifierScore
    M = clean
    tr = _full_width_trainer(M)
    lib.delete_params_with_name('Generator.')          # the classifier trainer's own generator: its names are the GAN's
    scorer = ClassifierScore(tr)
    images = O.random_images(230, seed=5)
    ref = scorer.statistics(images, chunk=100)
    fb = _set_features(M, tr, images, 100)
    case = H.Case(lib, 'resnet', 16, 4, 'cuda')
    try:
        gan = case.trainer()
        stream = evaluate.eval_stream(gan)
        c0 = int(stream.ctr.item())
        before = H.snapshot(lib, gan)
        plain = scorer.score_generator(gan, 300)
        assert set(plain) == set(SCORE_KEYS)
        scorer.set_reference(ref)
        stream.ctr.fill_(c0)
        got = scorer.score_generator(gan, 300)
        H.assert_same(before, H.snapshot(lib, gan))
        assert set(got) == set(SCORE_KEYS) | {'frechet'}
        for k in SCORE_KEYS:                                                    # the score does not move by a bit
            assert np.array_equal(np.asarray(got[k]), np.asarray(plain[k])), k
        # the same samples -> kernels.score_input -> the averaged classifier's plain pass -> the two-pass oracle
        ev = evaluate.Evaluator(gan)
        stream.ctr.fill_(c0)
        scale = evaluate.SCORE_SCALE['gan_cifar_resnet']
        fa = torch.cat([_plain_features(M, tr, K.score_input(x, 3, scale, scorer.lut)) for x, _ in ev.score_draws(300)]).cpu().numpy()
        assert fa.shape == (300, M.cfg.D_WIDTHS[-1])
        want = FO.features_distance(fa, fb)
        tol, info = FO.distance_tolerance(fa, fb)
        print('resnet generator: frechet %.17g, oracle %.17g, |diff| %.3e, tolerance %.3e, %s' % (got['frechet'], want, abs(got['frechet'] - want), tol, info))
        _report('resnet_generator_300_distance', abs(got['frechet'] - want) / tol)
        assert np.isfinite(got['frechet']) and got['frechet'] > 0 and abs(got['frechet'] - want) <= tol
        stream.ctr.fill_(c0)
        stats = scorer.statistics_generator(gan, 300)
        H.assert_same(before, H.snapshot(lib, gan))
        dmean, dcov = FO.statistics_bound(fa)
        _, mean, cov = FO.two_pass_statistics(fa)
        assert (np.abs(stats.mean - mean) <= dmean).all() and (np.abs(stats.cov - cov) <= dcov).all()
    finally:
        case.close()


def test_scoring_with_a_reference_around_captured_graphs_leaves_the_training_run_bit_identical(K, clean):
    """tests/test_gpu_score_cifar.py's graph-capture check with a reference set: the moment launches and the scorer's state sit between
    the replays of the GAN's captured graphs, and the graphed run's weights still equal, bit for bit, those of an eager run that never
    scores; every scoring returns a finite distance, and the distance moves as the generator does."""
    import ctgan_amd.tflib as lib
    from ctgan_amd.score_cifar import ClassifierScore
    M = clean
    tr = _full_width_trainer(M)
    lib.delete_params_with_name('Generator.')
    scorer = ClassifierScore(tr)
    stable, packs = set(K._STABLE_PTRS), len(K._pack16)
    images = O.random_images(100, seed=8)
    scorer.set_reference(scorer.statistics(images, chunk=50))
    first = scorer.score(images, splits=4, chunk=50)
    assert set(K._STABLE_PTRS) == stable and len(K._pack16) == packs
    results, score_generator = [], scorer.score_generator

    def recording(*a, **kw):
        results.append(score_generator(*a, **kw))
        return results[-1]
    scorer.score_generator = recording
    with_scoring, scores = _gan_loop(scorer, True)
    without, _ = _gan_loop(None, False)
    for a, b in zip(with_scoring, without):
        assert torch.equal(a, b)
    dist = [r['frechet'] for r in results]
    assert len(scores) == len(dist) == 3 and all(np.isfinite(v) and v > 0 for v in dist) and len(set(dist)) == 3
    again = scorer.score(images, splits=4, chunk=50)
    assert again['mean'] == first['mean'] and again['frechet'] == first['frechet']          # the classifier did not move
    assert abs(first['frechet']) <= 2 * FO.distance_tolerance(*[_set_features(M, tr, images, 50)] * 2)[0]          # d(a, a)
