"""The unbiased kernel distance of CIFAR-10 samples on the MI355X (`-m gpu`): csrc/kid.hip - ctgan_kernel_tile_sums against the long
double direct-form oracle (tests/kid_oracle.py) on the same fp32 features - and ctgan_amd.score_cifar's FeatureSet.kernel_tiles /
kernel_distance / kernel-reference path end to end.

Every bound is derived in the oracle, none is tuned: a tile sum within the sum of its pairs' E_k plus 4096 2^-52 sum |k|, the estimate and
its blocks within the same bounds pushed through the formula.  A padded row or the diagonal counted by mistake is an error of
coef0^3 = 1 per pair against bounds near 1e-9, so the edge shapes need not be large.  The largest observed error / bound ratios go to
kid_err.json in the run-output directory (tests/score_cifar_oracle.py `report_dir`).

Named to be collected after tests/test_gpu_kernels.py, as tests/test_gpu_score_cifar_frechet.py explains."""
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import eval_helpers as H  # noqa: E402
from tests import kid_oracle as KO  # noqa: E402
from tests import score_cifar_oracle as O  # noqa: E402
from tests.test_gpu_score_cifar import K, _full_width_trainer, clean  # noqa: E402,F401  (fixtures and helpers)

SCORE_KEYS = ('mean', 'std', 'splits', 'hist', 'acc')
MANIFOLD_KEYS = ('precision', 'recall', 'nn_dist', 'nn_zero')
KID_KEYS = ('kid', 'kid_std', 'kid_blocks')
_RATIOS = {}


def _report(key, ratio):
    _RATIOS[key] = max(float(ratio), _RATIOS.get(key, 0.0))
    with open(os.path.join(O.report_dir(), 'kid_err.json'), 'w') as f:
        json.dump({'largest_error_over_bound': _RATIOS}, f, indent=1, sort_keys=True)


def _ratio(got, want, bound):
    """max |got - want| / bound over the elements (an element with a zero bound must have a zero error)."""
    err = np.abs(np.asarray(got, dtype=np.longdouble) - np.asarray(want, dtype=np.longdouble)).astype(np.float64)
    bound = np.asarray(bound, dtype=np.float64)
    assert (err[bound == 0] == 0).all()
    return float((err[bound > 0] / bound[bound > 0]).max()) if (bound > 0).any() else 0.0


def _close(got, want, key):
    """A kernel_distance dict (or the kid keys of a scoring) against the oracle's, within the oracle's bounds."""
    q = max(_ratio(got['kid'], want['kid'], want['e_kid']), _ratio(got['kid_blocks'], want['kid_blocks'], want['e_blocks']))
    print('%s: kid %.6e (oracle %.6e, bound %.1e), %d blocks, error / bound %.3e' % (key, got['kid'], want['kid'], want['e_kid'],
                                                                                      len(want['kid_blocks']), q))
    _report(key, q)
    assert got['kid_blocks'].dtype == np.float64 and got['kid_blocks'].shape == want['kid_blocks'].shape
    assert q <= 1.0
    if want['kid_std'] is None:
        assert got['kid_std'] is None
    else:
        assert abs(got['kid_std'] - want['kid_std']) <= KO.std_bound(want['kid_blocks'], want['e_blocks'])


# ----------------------------------------------------------------------------------------------------- the kernel
@pytest.mark.parametrize('shape', KO.CASES)
def test_tile_sums_match_the_oracle_within_the_bound(K, shape):
    m, n, d, exclude = shape
    a, b, sums, bound = KO.case(*shape)
    ta = torch.from_numpy(a).cuda()
    tb = ta if exclude else torch.from_numpy(b).cuda()
    out = torch.full(tuple(sums.shape), -7.0, dtype=torch.float64, device='cuda')
    assert K.kernel_tile_sums(ta, tb, exclude_diag=exclude, out=out) is out
    got = out.cpu().numpy()
    q = _ratio(got, sums, bound)
    print('%s: %d x %d tiles, |sum - ref| / bound %.3e, largest bound %.2e' % (shape, sums.shape[0], sums.shape[1], q, bound.max()))
    _report('tiles_%s' % '_'.join('%d' % v for v in shape), q)
    assert q <= 1.0
    assert torch.equal(K.kernel_tile_sums(ta, tb, exclude_diag=exclude), out)          # a second run, a new buffer: the same bits
    if not exclude and m == n:                                                           # the diagonal is there unless it is asked away
        assert not torch.equal(K.kernel_tile_sums(ta, ta, exclude_diag=True), K.kernel_tile_sums(ta, ta))


def test_tile_sums_where_the_kernel_changes_sign(K):
    a, b = KO.signed_inputs()
    sums, bound = KO.tile_sums(a, b, 1.0, -0.5)
    k, _ = KO.kernel_direct(a, b, 1.0, -0.5)
    assert (k < 0).mean() > 0.2 and (k > 0).mean() > 0.2
    got = K.kernel_tile_sums(torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda(), gamma=1.0, coef0=-0.5).cpu().numpy()
    q = _ratio(got, sums, bound)
    print('%s gamma 1 coef0 -0.5: |sum - ref| / bound %.3e' % (KO.SIGNED[:3], q))
    _report('tiles_signed', q)
    assert q <= 1.0


def test_bits_do_not_depend_on_the_grid_shape(K):
    """(1000, 2100): 16 tiles of a, 33 of b; the host asks for ceil(512 / 16) = 32 slabs per tile of a: slabs of 2 tiles, a 16 x 17 grid.
    (64, 2100): one tile of a; 512 slabs wanted, 33 tiles there: slabs of 1 tile, a 1 x 33 grid.  Row 0 is the same bits in both."""
    a, b, _, _ = KO.case(1000, 2100, 128, False)
    ta, tb = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
    whole = K.kernel_tile_sums(ta, tb)
    first = K.kernel_tile_sums(ta[:64].contiguous(), tb)
    assert tuple(whole.shape) == (16, 33) and tuple(first.shape) == (1, 33) and torch.equal(first[0], whole[0])
    last = K.kernel_tile_sums(ta[960:].contiguous(), tb)                                # the partial last tile of a, on its own
    assert torch.equal(last[0], whole[15])
    assert torch.equal(K.kernel_tile_sums(ta, tb[:128].contiguous()), whole[:, :2].contiguous())      # 16 x 2: slabs of 1


def test_unsupported_and_bad_arguments_launch_nothing(K):
    f = torch.ones(20, 16, device='cuda')
    out = torch.full((1, 1), -7.0, dtype=torch.float64, device='cuda')
    wide = torch.ones(20, 1025, device='cuda')
    with pytest.raises(NotImplementedError, match='1025 features'):
        K.kernel_tile_sums(wide, wide, out=out)
    with pytest.raises(ValueError, match='exclude_diag'):
        K.kernel_tile_sums(f, f[:19].contiguous(), exclude_diag=True, out=out)
    with pytest.raises(ValueError):
        K.kernel_tile_sums(f[:0], f, out=torch.empty(0, 1, dtype=torch.float64, device='cuda'))
    with pytest.raises(AssertionError):
        K.kernel_tile_sums(f, f[:, :8].contiguous(), out=out)
    with pytest.raises(AssertionError):
        K.kernel_tile_sums(f, f, out=out.float())
    with pytest.raises(AssertionError):
        K.kernel_tile_sums(f, f, out=torch.empty(2, 1, dtype=torch.float64, device='cuda'))
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        K.kernel_tile_sums(f.cpu(), f, out=out)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        K.kernel_tile_sums(f, f, out=out.cpu())
    torch.cuda.synchronize()
    assert (out == -7.0).all().item()
    assert K.KERNEL_TILE == 64


# ----------------------------------------------------------------------------------------------------- end to end
@pytest.mark.parametrize('shape', [(130, 200, 10), (300, 257, 128)])
def test_kernel_distance_on_device_sets(K, shape):
    from ctgan_amd.score_cifar import FeatureSet, kernel_distance
    m, n, d = shape
    fa, fb = KO.relu_rows(m, d, 3), KO.relu_rows(n, d, 4, shift=0.1)
    sa, sb = FeatureSet(torch.from_numpy(fa).cuda()), FeatureSet(torch.from_numpy(fb).cuda())
    got = kernel_distance(sa, sb)
    assert set(got) == set(KID_KEYS) | {'subset'} and got['subset'] == KO.default_subset(m, n)
    _close(got, KO.kernel_distance(fa, fb), 'kernel_distance_%d_%d_%d' % shape)
    tiles = sb.kernel_tiles()
    assert sb.kernel_tiles() is tiles and tiles.is_cuda and tuple(tiles.shape) == (-(-n // 64),) * 2
    again = kernel_distance(sa, sb, subset=128)
    assert again['kid'] == got['kid'] and again['subset'] == 128 and len(again['kid_blocks']) == min(m, n) // 128


def test_kernel_reference_of_a_uint8_set_on_the_full_width_classifier(K, clean):
    from ctgan_amd.score_cifar import ClassifierScore, kernel_distance
    M = clean
    tr = _full_width_trainer(M)
    images = O.random_images(230, seed=5)
    scorer = ClassifierScore(tr)
    fs = scorer.features(images, chunk=100)
    plain = scorer.score(images, splits=10, chunk=100)
    scorer.set_kernel_reference(fs)
    own = scorer.score(images, splits=10, chunk=100)          # the reference's own images: the estimate of two identical sets
    assert set(own) == set(SCORE_KEYS) | set(KID_KEYS)
    for k in SCORE_KEYS:
        assert np.array_equal(np.asarray(own[k]), np.asarray(plain[k])), k
    f = fs.features.cpu().numpy()
    want = KO.kernel_distance(f, f)
    assert want['kid'] < 0 and want['subset'] == 64 and len(want['kid_blocks']) == 3
    _close(own, want, 'score_own_images_230')
    assert own['kid'] < 0
    same = kernel_distance(fs, fs)
    assert same['kid'] == own['kid'] and np.array_equal(same['kid_blocks'], own['kid_blocks'])


def test_score_generator_with_a_kernel_reference_on_a_resnet_gan(K, clean):
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
        scorer.set_kernel_reference(ref)
        stream.ctr.fill_(c0)
        got = scorer.score_generator(gan, 300)
        H.assert_same(before, H.snapshot(lib, gan))
        assert set(got) == set(SCORE_KEYS) | set(KID_KEYS)
        for k in SCORE_KEYS:                                                    # the score does not move by a bit
            assert np.array_equal(np.asarray(got[k]), np.asarray(plain[k])), k
        stream.ctr.fill_(c0)
        feats = scorer.features_generator(gan, 300)
        H.assert_same(before, H.snapshot(lib, gan))
        fa, fb = feats.features.cpu().numpy(), ref.features.cpu().numpy()
        assert fa.shape == (300, 128)
        _close(got, KO.kernel_distance(fa, fb), 'score_generator_resnet_300')
        # with a manifold too: one buffer serves both, and the manifold keys are those of the manifold alone
        scorer.set_kernel_reference(None)
        scorer.set_manifold(ref)
        stream.ctr.fill_(c0)
        only = scorer.score_generator(gan, 300)
        assert set(only) == set(SCORE_KEYS) | set(MANIFOLD_KEYS)
        scorer.set_kernel_reference(ref)
        stream.ctr.fill_(c0)
        both = scorer.score_generator(gan, 300)
        assert set(both) == set(SCORE_KEYS) | set(MANIFOLD_KEYS) | set(KID_KEYS)
        for k in SCORE_KEYS + MANIFOLD_KEYS:
            assert np.array_equal(np.asarray(both[k]), np.asarray(only[k])), k
        for k in KID_KEYS:
            assert np.array_equal(np.asarray(both[k]), np.asarray(got[k])), k
    finally:
        case.close()
