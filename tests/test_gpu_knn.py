"""Precision and recall of CIFAR-10 samples on the MI355X (`-m gpu`): csrc/knn.hip - ctgan_knn_radii and ctgan_knn_cover against the
fp64 direct-form oracle (tests/knn_oracle.py) on the same fp32 features - and ctgan_amd.score_cifar's FeatureSet / precision_recall /
manifold path end to end.

Every bound is derived in the oracle, none is tuned: a device distance within E(i, j) = (d + 4) 2^-52 (|a_i| + |b_j|)^2 of the direct
form, exactly 0 between bit-identical rows; a radius within the bound of its own pair; coverage equal on every row the oracle can
decide (on these inputs: every row, tests/test_knn_host.py); the nearest index equal wherever the runner-up is more than 2 E away.  The
largest observed error / bound ratios go to knn_err.json in the run-output directory (tests/score_cifar_oracle.py `report_dir`).

Named to be collected after tests/test_gpu_kernels.py, as tests/test_gpu_score_cifar_frechet.py explains."""
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import eval_helpers as H  # noqa: E402
from tests import knn_oracle as KO  # noqa: E402
from tests import score_cifar_oracle as O  # noqa: E402
from tests.test_gpu_score_cifar import K, _full_width_trainer, clean  # noqa: E402,F401  (fixtures and helpers)

SCORE_KEYS = ('mean', 'std', 'splits', 'hist', 'acc')
MANIFOLD_KEYS = ('precision', 'recall', 'nn_dist', 'nn_zero')
UNDECIDABLE_CAP = 0.01
_RATIOS = {}


def _report(key, ratio):
    _RATIOS[key] = max(float(ratio), _RATIOS.get(key, 0.0))
    with open(os.path.join(O.report_dir(), 'knn_err.json'), 'w') as f:
        json.dump({'largest_error_over_bound': _RATIOS}, f, indent=1, sort_keys=True)


def _ratio(err, bound):
    """max err / bound over the elements (an element with a zero bound must have a zero error)."""
    err, bound = np.asarray(err, dtype=np.float64), np.asarray(bound, dtype=np.float64)
    assert (err[bound == 0] == 0).all()
    return float((err[bound > 0] / bound[bound > 0]).max()) if (bound > 0).any() else 0.0


def _sentinel(rows, dtype, value, tail=5):
    return torch.full((rows + tail,), value, dtype=dtype, device='cuda')


# ----------------------------------------------------------------------------------------------------- the kernels
@pytest.mark.parametrize('shape', KO.CASES)
def test_radii_match_the_oracle_within_the_bound(K, shape):
    c = KO.case(*shape)
    n, k = shape[1], c.k
    f = torch.from_numpy(c.b).cuda()
    out = _sentinel(n, torch.float64, -7.0)
    assert K.knn_radii(f, k, out=out) is out
    got = out.cpu().numpy()
    assert (got[n:] == -7.0).all()                                              # nothing past n is written
    q = _ratio(np.abs(got[:n] - c.r2_b), c.e_r2_b)
    print('%s: |r2 - ref| / bound %.3e, %d radii exactly 0' % (shape, q, (got[:n] == 0).sum()))
    _report('radii_%s' % '_'.join('%g' % v for v in shape), q)
    assert q <= 1.0
    if c.planted:
        assert (got[10:11 + k] == 0.0).all() and (got[:n] == 0.0).sum() == k + 1          # the k + 1 copies: self excluded by index only
    assert torch.equal(K.knn_radii(f, k), out[:n])                              # a second run: the same bits


@pytest.mark.parametrize('shape', KO.CASES)
def test_cover_and_nearest_match_the_oracle(K, shape):
    c = KO.case(*shape)
    m, n, d, k, _ = shape
    a, b, r2 = torch.from_numpy(c.a).cuda(), torch.from_numpy(c.b).cuda(), torch.from_numpy(c.r2_b).cuda()
    bufs = _sentinel(m, torch.int32, -3), _sentinel(m, torch.float64, -7.0), _sentinel(m, torch.int32, -5)
    covered, nn_d2, nn_idx = K.knn_cover(a, b, r2, *bufs)
    assert covered is bufs[0] and nn_d2 is bufs[1] and nn_idx is bufs[2]
    cov, d2, idx = (t.cpu().numpy() for t in bufs)
    assert (cov[m:] == -3).all() and (d2[m:] == -7.0).all() and (idx[m:] == -5).all()          # nothing past m is written
    cov, d2, idx = cov[:m], d2[:m], idx[:m]
    assert set(np.unique(cov)) <= {0, 1} and ((idx >= 0) & (idx < n)).all()                    # a padded row of b is never a neighbour
    left_out = 1.0 - c.decidable.mean()
    assert left_out <= UNDECIDABLE_CAP
    assert np.array_equal(cov[c.decidable].astype(bool), c.covered[c.decidable])
    q = _ratio(np.abs(d2 - c.nn_d2), c.e_nn)
    print('%s: |nn_d2 - ref| / bound %.3e, %d of %d rows covered (oracle %d), %.2f%% undecidable, %d ambiguous neighbours'
          % (shape, q, cov.sum(), m, c.covered.sum(), 100 * left_out, (~c.nn_sure).sum()))
    _report('nearest_%s' % '_'.join('%g' % v for v in shape), q)
    assert q <= 1.0
    assert np.array_equal(idx[c.nn_sure], c.nn_idx[c.nn_sure])
    if c.planted:
        zero = [0, 1, 2, 3, 4, KO.COPY_OF_B10]
        assert (d2[zero] == 0.0).all() and (d2 == 0.0).sum() == len(zero) and (cov[zero] == 1).all()
        assert idx[KO.COPY_OF_B10] == 10 and list(idx[:5]) == [0, 1, 2, 3, 4]          # the lowest of the k + 1 identical rows
        only_zero = torch.full_like(r2, -1.0)                                     # every ball empty but those of radius exactly 0
        only_zero[r2 == 0] = 0.0
        through = K.knn_cover(a, b, only_zero)[0].cpu().numpy()
        assert through[KO.COPY_OF_B10] == 1 and through.sum() == 1                # ... which hold the copy of b[10] and nothing else
    # a second run: the same bits; without radii: the same nearest neighbours, no coverage
    again = K.knn_cover(a, b, r2)
    assert all(torch.equal(x, y[:m]) for x, y in zip(again, bufs))
    none, d2_only, idx_only = K.knn_cover(a, b)
    assert none is None and torch.equal(d2_only, nn_d2[:m]) and torch.equal(idx_only, nn_idx[:m])
    if c.back is not None:                                                        # the other direction: recall, with the device's own radii
        back = K.knn_cover(b, a, K.knn_radii(a, k))[0].cpu().numpy().astype(bool)
        assert 1.0 - c.back_decidable.mean() <= UNDECIDABLE_CAP
        assert np.array_equal(back[c.back_decidable], c.back[c.back_decidable])


def test_unsupported_and_bad_arguments_launch_nothing(K):
    f = torch.ones(20, 16, device='cuda')
    out = torch.full((20,), -7.0, dtype=torch.float64, device='cuda')
    with pytest.raises(NotImplementedError, match='k = 9'):
        K.knn_radii(f, K.KNN_MAX_K + 1, out=out)
    with pytest.raises(NotImplementedError, match='1025 features'):
        K.knn_radii(torch.ones(20, 1025, device='cuda'), 3, out=out)
    with pytest.raises(ValueError, match='neighbour'):
        K.knn_radii(f[:3], 3, out=out)                                          # n < k + 1
    with pytest.raises(ValueError):
        K.knn_radii(f, 0, out=out)
    bufs = (torch.full((20,), -3, dtype=torch.int32, device='cuda'), torch.full((20,), -7.0, dtype=torch.float64, device='cuda'),
            torch.full((20,), -5, dtype=torch.int32, device='cuda'))
    r2 = torch.ones(20, dtype=torch.float64, device='cuda')
    with pytest.raises(NotImplementedError, match='1025 features'):
        K.knn_cover(torch.ones(20, 1025, device='cuda'), torch.ones(20, 1025, device='cuda'), r2, *bufs)
    K.knn_cover(f[:0], f, r2, *bufs)                                            # no rows: a successful no-op
    with pytest.raises(AssertionError):
        K.knn_cover(f, f[:, :8].contiguous(), r2, *bufs)
    with pytest.raises(AssertionError):
        K.knn_cover(f, f, r2.float(), *bufs)
    with pytest.raises(AssertionError):
        K.knn_cover(f, f, r2, bufs[0][:10], bufs[1], bufs[2])                   # an output shorter than m
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        K.knn_cover(f.cpu(), f, r2, *bufs)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        K.knn_radii(f.cpu(), 3)
    torch.cuda.synchronize()
    assert (out == -7.0).all().item() and (bufs[0] == -3).all().item() and (bufs[1] == -7.0).all().item() and (bufs[2] == -5).all().item()


# ----------------------------------------------------------------------------------------------------- end to end
def test_features_of_a_uint8_set_on_the_full_width_classifier(K, clean):
    from ctgan_amd.score_cifar import ClassifierScore, precision_recall
    M = clean
    tr = _full_width_trainer(M)
    images = O.random_images(230, seed=5)
    scorer = ClassifierScore(tr)
    fs = scorer.features(images, chunk=100)
    data = torch.from_numpy(images).cuda()
    want = torch.cat([scorer._forward(tr.gather_fixed(torch.arange(r0, min(r0 + 100, 230), dtype=torch.int32, device='cuda'), data=data), True)[1]
                      for r0 in range(0, 230, 100)])
    assert fs.n == 230 and fs.width == M.cfg.D_WIDTHS[-1] == 128 and torch.equal(fs.features, want)          # the pass's features, bit for bit
    assert fs.classifier == scorer.fingerprint()
    # scoring the manifold's own images: every sample is a reference row
    scorer.set_manifold(fs)
    own = scorer.score(images, splits=10, chunk=100)
    assert set(own) == set(SCORE_KEYS) | set(MANIFOLD_KEYS)
    assert own['nn_zero'] == 230 and own['precision'] == 1.0 and own['recall'] == 1.0 and own['nn_dist'] == 0.0
    assert precision_recall(fs, fs) == {'precision': 1.0, 'recall': 1.0, 'k': 3, 'nn_dist': 0.0, 'nn_zero': 230}


def test_score_generator_with_a_manifold_on_a_resnet_gan(K, clean):
    import ctgan_amd.tflib as lib
    from ctgan_amd import evaluate
    from ctgan_amd.score_cifar import ClassifierScore
    M = clean
    tr = _full_width_trainer(M)
    lib.delete_params_with_name('Generator.')          # the classifier trainer's own generator: its names are the GAN's
    scorer = ClassifierScore(tr)
    ref = scorer.features(O.random_images(230, seed=5), chunk=100)
    case = H.Case(lib, 'resnet', 16, 4, 'cuda')
    try:
        gan = case.trainer()
        stream = evaluate.eval_stream(gan)
        c0 = int(stream.ctr.item())
        before = H.snapshot(lib, gan)
        plain = scorer.score_generator(gan, 300)
        assert set(plain) == set(SCORE_KEYS)
        scorer.set_manifold(ref)
        stream.ctr.fill_(c0)
        got = scorer.score_generator(gan, 300)
        H.assert_same(before, H.snapshot(lib, gan))
        assert set(got) == set(SCORE_KEYS) | set(MANIFOLD_KEYS)
        for k in SCORE_KEYS:                                                    # the score does not move by a bit
            assert np.array_equal(np.asarray(got[k]), np.asarray(plain[k])), k
        stream.ctr.fill_(c0)
        feats = scorer.features_generator(gan, 300)
        H.assert_same(before, H.snapshot(lib, gan))
        fa, fb = feats.features.cpu().numpy(), ref.features.cpu().numpy()
        assert fa.shape == (300, 128)
        want = KO.precision_recall(fa, fb, 3)
        # the counts are the oracle's wherever it can decide them: here every row
        dist, e = KO.d2_direct(fa, fb), KO.bound(fa, fb)
        (r2b, eb), (r2a, ea) = KO.radii(fb, 3), KO.radii(fa, 3)
        sure = KO.decidable(dist, r2b, e, eb).all() and KO.decidable(dist.T, r2a, e.T, ea).all()
        nn = dist.min(axis=1)
        print('resnet generator: %s, oracle %s, every row decidable: %s' % ({k: got[k] for k in MANIFOLD_KEYS}, want, sure))
        assert sure
        assert got['precision'] == want['precision'] and got['recall'] == want['recall'] and got['nn_zero'] == want['nn_zero']
        e_nn = e[np.arange(300), dist.argmin(axis=1)]                           # sqrt: |sqrt x - sqrt y| <= |x - y| / (sqrt x + sqrt y)
        assert abs(got['nn_dist'] - want['nn_dist']) <= (e_nn / np.sqrt(nn)).max() if nn.min() > 0 else got['nn_dist'] >= 0
    finally:
        case.close()
