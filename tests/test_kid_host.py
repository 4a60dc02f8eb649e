"""The unbiased kernel distance of CIFAR-10 samples (ctgan_amd.score_cifar: FeatureSet.kernel_tiles, kernel_distance, the kernel
reference of ClassifierScore) without a GPU: the fp64 oracle's own checks (tests/kid_oracle.py), and the host logic on CPU stand-ins
(tests/kid_cpu_kernels.py)."""
import numpy as np
import pytest
import torch

from tests import eval_helpers as H
from tests import kid_oracle as KO
from tests import score_cifar_oracle as O
from tests.kid_cpu_kernels import (class_stats_kernels, frechet_kernels, kid_kernels, knn_kernels,        # noqa: F401  (fixtures)
                                   score_cifar_kernels)
from tests.test_score_cifar_host import _Series, _checkpoint_scorer

SCORE_KEYS = ('mean', 'std', 'splits', 'hist', 'acc')
MANIFOLD_KEYS = ('precision', 'recall', 'nn_dist', 'nn_zero')
KID_KEYS = ('kid', 'kid_std', 'kid_blocks')


def _same(a, b, keys):
    for k in keys:
        assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])), k


def _close(got, want):
    """A kernel_distance dict against the oracle's, within the oracle's bounds."""
    assert set(got) == {'kid', 'kid_std', 'kid_blocks', 'subset'} and got['subset'] == want['subset']
    assert abs(got['kid'] - want['kid']) <= want['e_kid'], (got['kid'], want['kid'], want['e_kid'])
    assert got['kid_blocks'].dtype == np.float64 and got['kid_blocks'].shape == want['kid_blocks'].shape
    assert (np.abs(got['kid_blocks'] - want['kid_blocks']) <= want['e_blocks']).all()
    if want['kid_std'] is None:
        assert got['kid_std'] is None
    else:
        assert abs(got['kid_std'] - want['kid_std']) <= KO.std_bound(want['kid_blocks'], want['e_blocks'])


# ----------------------------------------------------------------------------------------------------- the oracle
def test_oracle_gemm_form_stays_within_the_pair_bound_and_fsum_agrees():
    a, b = KO.inputs(65, 129, 128, False)
    k, e = KO.kernel_direct(a, b)
    q = float((np.abs(KO.gemm_form(a, b) - k) / e).max())
    print('gemm form / E_k at d = 128: %.4f' % q)
    assert q <= 0.06
    sa, sb = KO.signed_inputs()
    k, e = KO.kernel_direct(sa, sb, 1.0, -0.5)
    assert (k < 0).any() and (k > 0).any()
    assert float((np.abs(KO.gemm_form(sa, sb, 1.0, -0.5) - k) / e).max()) <= 0.5
    for shape in [(17, 70, 10, False), (57, 57, 10, True), (65, 129, 128, False)]:
        a, b, sums, bound = KO.case(*shape)
        exact = KO.tile_sums_fsum(a, b, exclude_diag=shape[3])
        assert sums.shape == bound.shape == exact.shape and (np.abs(np.asarray(sums, dtype=np.float64) - exact) <= 1e-3 * bound).all()
    # a padded pair is worth coef0^3 = 1: the bounds are many orders below it
    assert max(float(KO.case(*shape)[3].max()) for shape in KO.CASES) < 1e-6


def test_oracle_masks_by_index():
    a = np.array([[2.0], [0.0], [3.0]], dtype=np.float32)
    sums, _ = KO.tile_sums(a, a, gamma=1.0, coef0=0.0, exclude_diag=True)          # 2 (2 * 3)^3 and nothing of the zero row but 0
    assert sums.shape == (1, 1) and float(sums[0, 0]) == 432.0
    full, _ = KO.tile_sums(a, a, gamma=1.0, coef0=1.0)
    assert float(full[0, 0]) == 5.0 ** 3 + 10.0 ** 3 + 2 * 7.0 ** 3 + 5 * 1.0


def test_stand_in_equals_the_oracle_within_the_bound():
    from tests import kid_cpu_kernels as C
    for shape in KO.CASES[:9]:
        a, b, sums, bound = KO.case(*shape)
        got = C.kernel_tile_sums(torch.from_numpy(a), torch.from_numpy(b), exclude_diag=shape[3]).numpy()
        assert got.shape == sums.shape and (np.abs(got - np.asarray(sums, dtype=np.float64)) <= bound).all(), shape
    sa, sb = KO.signed_inputs()
    sums, bound = KO.tile_sums(sa, sb, 1.0, -0.5)
    got = C.kernel_tile_sums(torch.from_numpy(sa), torch.from_numpy(sb), gamma=1.0, coef0=-0.5).numpy()
    assert (np.abs(got - np.asarray(sums, dtype=np.float64)) <= bound).all()
    with pytest.raises(NotImplementedError):
        C.kernel_tile_sums(torch.zeros(3, 1025), torch.zeros(3, 1025))
    with pytest.raises(ValueError):
        C.kernel_tile_sums(torch.zeros(3, 4), torch.zeros(4, 4), exclude_diag=True)


# ----------------------------------------------------------------------------------------------------- kernel_distance
@pytest.mark.parametrize('shape', [(130, 200, 10), (300, 257, 128)])
def test_kernel_distance_matches_the_oracle(kid_kernels, shape):
    from ctgan_amd.score_cifar import FeatureSet, kernel_distance
    m, n, d = shape
    fa, fb = KO.relu_rows(m, d, 3), KO.relu_rows(n, d, 4, shift=0.1)
    _close(kernel_distance(FeatureSet(fa), FeatureSet(fb)), KO.kernel_distance(fa, fb))
    got = kernel_distance(FeatureSet(fa), FeatureSet(fb), subset=128)
    want = KO.kernel_distance(fa, fb, subset=128)
    assert got['subset'] == 128 and len(got['kid_blocks']) == min(m, n) // 128
    _close(got, want)


def test_subset_rule_and_refusals(kid_kernels):
    from ctgan_amd.score_cifar import FeatureSet, kernel_distance, kernel_subset
    assert kernel_subset(1000, 50000) == 192 and kernel_subset(50000, 50000) == 1024 and kernel_subset(100, 90) == 64
    assert kernel_subset(1000, 50000, 256) == 256
    assert KO.default_subset(1000, 50000) == 192 and KO.default_subset(50000, 50000) == 1024
    fa, fb = KO.relu_rows(100, 10, 3), KO.relu_rows(90, 10, 4)
    got = kernel_distance(FeatureSet(fa), FeatureSet(fb))
    assert got['subset'] == 64 and got['kid_blocks'].shape == (1,) and got['kid_std'] is None
    _close(got, KO.kernel_distance(fa, fb))
    tiny = kernel_distance(FeatureSet(fa[:40]), FeatureSet(fb))          # fewer rows than a block: the estimate, no blocks
    assert tiny['subset'] == 64 and tiny['kid_blocks'].shape == (0,) and tiny['kid_std'] is None
    for bad in (100, 0, -64, 96.5):
        with pytest.raises(ValueError, match='subset'):
            kernel_distance(FeatureSet(fa), FeatureSet(fb), subset=bad)
    with pytest.raises(ValueError, match='10 and 8 features'):
        kernel_distance(FeatureSet(fa), FeatureSet(fb[:, :8]))
    with pytest.raises(ValueError, match='different classifiers'):
        kernel_distance(FeatureSet(fa, 'a' * 64), FeatureSet(fb, 'b' * 64))
    assert kernel_distance(FeatureSet(fa, 'a' * 64), FeatureSet(fb))['subset'] == 64          # a synthetic set goes with any
    with pytest.raises(ValueError, match='at least 2'):
        kernel_distance(FeatureSet(fa[:1]), FeatureSet(fb))
    with pytest.raises(ValueError, match='at least 2'):
        kernel_distance(FeatureSet(fa), FeatureSet(fb[:1]))


def test_feature_set_round_trip_with_and_without_kernel_tiles(kid_kernels, tmp_path, monkeypatch):
    import ctgan_amd.kernels as K
    from ctgan_amd.score_cifar import FeatureSet
    f = KO.relu_rows(70, 10, 5)
    fs = FeatureSet(f, 'abc123')
    fs.radii(1), fs.radii(3)
    calls = []
    sums = K.kernel_tile_sums
    monkeypatch.setattr(K, 'kernel_tile_sums', lambda *a, **kw: calls.append(kw) or sums(*a, **kw))
    without = str(tmp_path / 'without.npz')
    fs.save(without)
    with np.load(without, allow_pickle=False) as z:
        assert sorted(z.files) == ['classifier', 'features', 'radii_1', 'radii_3', 'radii_k']          # exactly the files of a set without
    assert calls == []
    tiles = fs.kernel_tiles()
    assert fs.kernel_tiles() is tiles and calls == [{'exclude_diag': True}]                          # computed once
    want, bound = KO.tile_sums(f, f, exclude_diag=True)
    assert tiles.dtype == torch.float64 and tuple(tiles.shape) == (2, 2)
    assert (np.abs(tiles.numpy() - np.asarray(want, dtype=np.float64)) <= bound).all()
    with_tiles = str(tmp_path / 'with.npz')
    fs.save(with_tiles)
    with np.load(with_tiles, allow_pickle=False) as z:
        assert sorted(z.files) == ['classifier', 'features', 'kernel_tiles', 'radii_1', 'radii_3', 'radii_k']
    del calls[:]
    back = FeatureSet.load(with_tiles)
    assert back.classifier == 'abc123' and torch.equal(back.features, fs.features) and torch.equal(back.radii(3), fs.radii(3))
    assert torch.equal(back.kernel_tiles(), tiles) and calls == []                                   # the saved sums are used
    bare = FeatureSet.load(without)
    assert bare._kernel_tiles is None and torch.equal(bare.features, fs.features) and torch.equal(bare.radii(1), fs.radii(1))
    assert torch.equal(bare.kernel_tiles(), tiles) and len(calls) == 1
    with pytest.raises(ValueError, match='kernel tile sums'):
        FeatureSet(f, None, None, np.zeros((3, 3)))


def test_same_distribution_sets_are_at_zero_within_their_own_error_bar(kid_kernels):
    """1,000 samples against 5,000 reference rows of one generator (128-wide ReLU-Gaussian rows): |kid| is below three standard errors of
    its own blocks, where the Frechet distance of such sets is 1.6; a set shifted by 0.25 before the ReLU is far outside: beyond five
    standard errors of its own blocks and ten times the range of the unshifted set."""
    from ctgan_amd.score_cifar import FeatureSet, kernel_distance
    ref = FeatureSet(KO.relu_rows(5000, 128, 11))
    same = kernel_distance(FeatureSet(KO.relu_rows(1000, 128, 12)), ref)
    p = len(same['kid_blocks'])
    assert same['subset'] == 192 and p == 5
    bar = 3.0 * same['kid_std'] / np.sqrt(p)
    print('same distribution: kid %.3e, 3 std / sqrt(P) %.3e' % (same['kid'], bar))
    assert abs(same['kid']) < bar
    shifted = kernel_distance(FeatureSet(KO.relu_rows(1000, 128, 13, shift=0.25)), ref)
    far = 3.0 * shifted['kid_std'] / np.sqrt(len(shifted['kid_blocks']))
    print('shifted by 0.25: kid %.3e, 3 std / sqrt(P) %.3e' % (shifted['kid'], far))
    assert shifted['kid'] > 5.0 / 3.0 * far and shifted['kid'] > 10 * bar          # beyond 5 standard errors of its own, 30 of the same set's


# ----------------------------------------------------------------------------------------------------- ClassifierScore
def test_kernel_reference_of_a_uint8_set_and_the_fingerprint_rules(kid_kernels, tmp_path):
    import ctgan_amd.ct_cifar as M
    from ctgan_amd.score_cifar import ClassifierScore, FeatureSet
    from tests.test_frechet_host import _features
    M.configure(**O.SMALL)
    tr = O.classifier_trainer()
    scorer = ClassifierScore(tr)
    assert scorer.kernel_reference is None and scorer.kernel_subset is None
    images, other = O.random_images(150, seed=9), O.random_images(140, seed=10)
    fs = scorer.features(images, chunk=60)
    f = _features(scorer, tr, images, 60)
    plain = scorer.score(other, splits=4, chunk=50)
    assert set(plain) == set(SCORE_KEYS)
    path = str(tmp_path / 'kernel_reference.npz')
    fs.kernel_tiles()
    fs.save(path)
    scorer.set_kernel_reference(path)
    assert scorer.kernel_reference.n == 150 and scorer.kernel_reference._kernel_tiles is not None
    got = scorer.score(other, splits=4, chunk=50)
    assert set(got) == set(SCORE_KEYS) | set(KID_KEYS)
    _same(got, plain, SCORE_KEYS)
    want = KO.kernel_distance(_features(scorer, tr, other, 50), f)
    assert want['subset'] == 64 and len(want['kid_blocks']) == 2
    _close(dict({k: got[k] for k in KID_KEYS}, subset=64), want)
    own = scorer.score(images, splits=4, chunk=60)                       # the reference's own images: the estimate of identical sets
    same = KO.kernel_distance(f, f)
    assert same['kid'] < 0 and abs(own['kid'] - same['kid']) <= same['e_kid']
    scorer.set_kernel_reference(fs, subset=128)
    assert len(scorer.score(other, splits=4, chunk=50)['kid_blocks']) == 1 and scorer.kernel_subset == 128
    # with a reference and a manifold too: the union of the keys, every other key as without a kernel reference
    scorer.set_kernel_reference(None)
    scorer.set_reference(scorer.statistics(images, chunk=60))
    scorer.set_manifold(fs, k=2)
    others = scorer.score(other, splits=4, chunk=50)
    assert set(others) == set(SCORE_KEYS) | {'frechet'} | set(MANIFOLD_KEYS)
    scorer.set_kernel_reference(fs)
    every = scorer.score(other, splits=4, chunk=50)
    assert set(every) == set(SCORE_KEYS) | {'frechet'} | set(MANIFOLD_KEYS) | set(KID_KEYS)
    _same(every, others, SCORE_KEYS + ('frechet',) + MANIFOLD_KEYS)
    _same(every, got, KID_KEYS)                                          # and the kernel distance of the run with nothing else
    scorer.set_reference(None)
    scorer.set_manifold(None)
    scorer.set_kernel_reference(None)
    assert set(scorer.score(other, splits=4)) == set(SCORE_KEYS)
    # refusals: at set_kernel_reference and, when the classifier moves later, at the scoring
    with pytest.raises(ValueError, match='another classifier'):
        scorer.set_kernel_reference(FeatureSet(fs.features, 'f' * 64))
    with pytest.raises(ValueError, match='do not record'):
        scorer.set_kernel_reference(FeatureSet(fs.features))
    with pytest.raises(ValueError, match='kernel reference features'):
        scorer.set_kernel_reference(FeatureSet(fs.features[:, :4], fs.classifier))
    with pytest.raises(ValueError, match='subset'):
        scorer.set_kernel_reference(fs, subset=100)
    with pytest.raises(ValueError, match='at least 2'):
        scorer.set_kernel_reference(FeatureSet(fs.features[:1], fs.classifier))
    assert scorer.kernel_reference is None
    scorer.set_kernel_reference(fs)
    with pytest.raises(ValueError, match='at least 2 samples'):
        scorer.score(other[:1], splits=1)
    idx4 = lambda *v: torch.tensor(v, dtype=torch.int32)          # noqa: E731
    tr.d_opt.set_lr(0.05)
    tr.d_body_idx(idx4(0, 5, 7, 2), idx4(1, 2, 3, 4), idx4(7, 6, 3, 1))          # one classifier step: the averaged parameters move
    with pytest.raises(ValueError, match='another classifier'):
        scorer.score(other, splits=4)
    with pytest.raises(ValueError, match='another classifier'):
        ClassifierScore(tr, kernel_reference=fs)


@pytest.mark.parametrize('name', ['resnet', 'cifar'])
def test_generator_scoring_with_a_kernel_reference_changes_nothing_else(kid_kernels, tmp_path, name):
    import ctgan_amd.ct_cifar as M
    import ctgan_amd.tflib as lib
    from ctgan_amd import evaluate
    from ctgan_amd.score_cifar import kernel_distance
    M.configure(**O.SMALL)
    scorer, _, _, _ = _checkpoint_scorer(tmp_path)
    ref = scorer.features(O.random_images(160, seed=3), chunk=50)
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
        scorer.set_kernel_reference(ref)
        stream.ctr.fill_(c0)
        got = scorer.score_generator(gan, 300, chunk=200)
        H.assert_same(before, H.snapshot(lib, gan))
        assert set(got) == set(SCORE_KEYS) | set(KID_KEYS)
        _same(got, plain, SCORE_KEYS)
        want = kernel_distance(feats, ref)
        _same(got, want, KID_KEYS)
        _close(want, KO.kernel_distance(feats.features.numpy(), ref.features.numpy()))
        # the loops' hook writes the series only when a kernel reference is set
        evaluate.SCORE_SAMPLES[long_name], kept = 200, evaluate.SCORE_SAMPLES[long_name]
        try:
            ev = evaluate.Evaluator(gan)
            rows = {}
            for with_reference in (True, False):
                scorer.set_kernel_reference(ref if with_reference else None)
                stream.ctr.fill_(c0)
                s = _Series()
                evaluate.record_score(ev, s, scorer)
                rows[with_reference] = s.rows
            stream.ctr.fill_(c0)
            scorer.set_kernel_reference(ref)
            res = scorer.score_generator(gan, 200)
        finally:
            evaluate.SCORE_SAMPLES[long_name] = kept
        assert rows[True] == rows[False] + [('kid', res['kid'])]
        assert 'kid' not in dict(rows[False]) and len(rows[False]) == (3 if name == 'resnet' else 1)
    finally:
        case.close()


# ----------------------------------------------------------------------------------------------------- the ABI
def test_kernel_tile_sums_validates_before_any_launch():
    """Argument validation happens before a launch, so it is observable without a GPU."""
    import ctypes
    import ctgan_amd.kernels as K
    from ctgan_amd import _lib
    lib = _lib.lib
    assert K.KERNEL_TILE == lib.ctgan_kernel_tile() == KO.TILE == 64
    some = ctypes.c_void_p(4096)          # never dereferenced: every call below is refused before the launch
    assert lib.ctgan_kernel_tile_sums(some, 5, some, 5, 1025, 1.0, 1.0, 0, some, None) == -2 and b'1025 features' in lib.ctgan_last_error()
    assert lib.ctgan_kernel_tile_sums(some, 5, some, 6, 16, 1.0, 1.0, 1, some, None) == -1 and b'exclude_diag' in lib.ctgan_last_error()
    for m, n, d in [(0, 5, 16), (5, 0, 16), (5, 5, 0), (-1, 5, 16)]:
        assert lib.ctgan_kernel_tile_sums(some, m, some, n, d, 1.0, 1.0, 0, some, None) == -1
    for args in [(None, some, some), (some, None, some), (some, some, None)]:
        assert lib.ctgan_kernel_tile_sums(args[0], 5, args[1], 5, 16, 1.0, 1.0, 0, args[2], None) == -1          # null pointers
