"""The classifier score of CIFAR-10 samples on the MI355X (`-m gpu`): csrc/score_cifar.hip - ctgan_score_input bit for bit against the
three launches it replaces, ctgan_score_accum + ctgan_score_finish against the fp64 restatement (tests/score_cifar_oracle.py) on the
same logits - and ctgan_amd.score_cifar.ClassifierScore end to end on a full-width CT classifier.

Tolerance on the mean, the std and every per-split score: 1e-10 max(1, mean).  At most 1,500 rows x 32 classes go through a handful of
fp64 libm calls and adds, each a few ulp (2.2e-16): the accumulated difference is bounded near 1e-11; 10x is the margin for the device
libm.  The class counts and the accuracy are exact.  The largest observed relative difference per case goes to
score_cifar_err.json in the run-output directory (tests/score_cifar_oracle.py `report_dir`)."""
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import eval_helpers as H  # noqa: E402
from tests import score_cifar_oracle as O  # noqa: E402

TOL = 1e-10
# (n, splits, chunk, K): a ragged last chunk; chunks smaller than a split and chunks that straddle splits; one row per split; 1,500 rows
# per workgroup (more than one stride of its 256 threads); the smallest and the largest class count
CASES = [(103, 10, 100, 10), (37, 3, 7, 10), (10, 10, 100, 10), (3000, 2, 3000, 10), (103, 10, 40, 2), (103, 10, 40, 32)]
_ERRS = {}


def _report(key, err):
    _ERRS[key] = max(err, _ERRS.get(key, 0.0))
    with open(os.path.join(O.report_dir(), 'score_cifar_err.json'), 'w') as f:
        json.dump({'tolerance': TOL, 'largest_relative_difference': _ERRS}, f, indent=1, sort_keys=True)


@pytest.fixture
def K():
    import ctgan_amd.kernels as K
    return K


@pytest.fixture
def clean():
    import ctgan_amd.ct_cifar as M
    import ctgan_amd.tflib as lib
    lib.delete_all_params()
    yield M
    M.configure(); lib.delete_all_params(); lib.delete_param_aliases()


def _lut():
    import ctgan_amd.ct_cifar as M
    return torch.from_numpy(M.byte_table()).cuda()


def _device_score(K, z, splits, chunk, labels=None):
    """The three kernels over the logits in chunks -> (the dict ClassifierScore returns, acc, cnt)."""
    n, nc = z.shape
    zd = torch.from_numpy(z).cuda()
    ld = None if labels is None else torch.from_numpy(labels).cuda()
    acc = torch.zeros(splits, nc + 1, dtype=torch.float64, device='cuda')
    cnt = torch.zeros(2 * nc, dtype=torch.int64, device='cuda')
    for r0 in range(0, n, chunk):
        K.score_accum(zd[r0:r0 + chunk], r0, n, splits, acc, cnt, None if ld is None else ld[r0:r0 + chunk])
    out = K.score_finish(acc, n, splits).cpu().numpy()
    c = cnt.cpu().numpy()
    return {'mean': float(out[0]), 'std': float(out[1]), 'splits': out[2:], 'hist': c[:nc],
            'acc': float(c[nc:].sum()) / n if labels is not None else None}, acc, cnt


# ----------------------------------------------------------------------------------------------------- score_input
@pytest.mark.parametrize('scale', [255. / 2, 255.99 / 2])
@pytest.mark.parametrize('n,channels,side', [(1, 3, 32), (3, 3, 32), (100, 3, 32), (2, 1, 5)])
def test_score_input_is_bit_equal_to_the_three_launches(K, n, channels, side, scale):
    x = torch.from_numpy(O.edge_samples(n, channels * side * side, seed=n)).cuda()
    assert not torch.isfinite(x).all() and (x == 1).any() and (x == -1).any() and (x > 1).any() and (x < -1).any()
    lut = _lut()
    got = K.score_input(x, channels, scale, lut)
    want = O.compose_input(K, x, channels, scale, lut, 2)
    assert got.shape == want.shape == (n, channels, side, side) and got.stride() == want.stride()
    assert torch.equal(got, want)
    # ... which is the byte table of the rotated saved pixels; a non-finite sample is byte 0
    px = H.pixels_reference(torch.nan_to_num(x, nan=-1.0, posinf=-1.0, neginf=-1.0).clamp(-4, 4), channels, scale).reshape(n, side, side, channels)
    assert torch.equal(got.permute(0, 2, 3, 1), lut[torch.flip(px, (1, 2)).long()])


def test_score_input_refuses_bad_arguments(K):
    lut = _lut()
    with pytest.raises(ValueError):
        K.score_input(torch.zeros(2, 48, device='cuda'), 3, 0.0, lut)
    with pytest.raises(AssertionError):
        K.score_input(torch.zeros(2, 3 * 15, device='cuda'), 3, 127.5, lut)          # not square
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        K.score_input(torch.zeros(2, 48), 3, 127.5, lut)
    assert K.score_input(torch.zeros(0, 48, device='cuda'), 3, 127.5, lut).shape == (0, 3, 4, 4)


# ----------------------------------------------------------------------------------------------------- score_accum + score_finish
@pytest.mark.parametrize('scale', [0.01, 3.0, 30.0])
@pytest.mark.parametrize('with_labels', [False, True])
@pytest.mark.parametrize('n,splits,chunk,nc', CASES)
def test_accum_and_finish_match_the_restatement(K, n, splits, chunk, nc, with_labels, scale):
    z, labels = O.logits_for(n, K=nc, scale=scale, seed=n + nc)
    labels = labels if with_labels else None
    got, acc, cnt = _device_score(K, z, splits, chunk, labels)
    ref = O.streaming_score(z, splits, chunk, labels)
    err = O.check_result(got, ref, TOL)
    _report('n%d_splits%d_chunk%d_K%d_scale%g' % (n, splits, chunk, nc, scale), err)
    if not with_labels:
        assert cnt[nc:].sum().item() == 0
    # two runs with the same chunking: the same bits
    got2, acc2, cnt2 = _device_score(K, z, splits, chunk, labels)
    assert torch.equal(acc, acc2) and torch.equal(cnt, cnt2) and got['mean'] == got2['mean'] and np.array_equal(got['splits'], got2['splits'])


def test_saturated_rows_score_one_and_non_finite_logits_give_nan(K):
    z = np.full((40, 10), -400.0, dtype=np.float32)
    z[np.arange(40), np.arange(40) % 3] = 400.0
    got, _, _ = _device_score(K, z, 4, 7)
    ref = O.streaming_score(z, 4, 7)
    assert np.isfinite(got['mean']) and np.isfinite(got['std'])
    _report('saturated', O.check_result(got, ref, TOL))
    z1 = np.full((40, 10), -400.0, dtype=np.float32)
    z1[:, 3] = 400.0                                        # one class only: the score is exactly that of a point mass, 1
    one, _, _ = _device_score(K, z1, 4, 7)
    assert abs(one['mean'] - 1.0) <= TOL and abs(one['std']) <= TOL and np.array_equal(one['hist'], np.bincount([3] * 40, minlength=10))
    for bad in (np.nan, np.inf, -np.inf):
        z2, _ = O.logits_for(40)
        z2[5, 2] = bad
        assert np.isnan(_device_score(K, z2, 4, 7)[0]['mean']), bad
    z3, lab3 = O.logits_for(40)
    z3[7, 4] = np.nan                                       # numpy.argmax takes the first NaN
    got3, _, _ = _device_score(K, z3, 4, 7, lab3)
    assert np.array_equal(got3['hist'], np.bincount(z3.argmax(axis=1), minlength=10))
    assert got3['acc'] == float((z3.argmax(axis=1) == lab3).sum()) / 40


def test_first_maximum_wins_and_labels_outside_the_classes_never_match(K):
    z = np.zeros((6, 10), dtype=np.float32)
    z[1, [4, 7]] = 2.0
    z[2, 9] = 1.0
    labels = np.array([0, 4, 9, -1, 10, 1 << 20], dtype=np.int32)
    got, _, cnt = _device_score(K, z, 2, 6, labels)
    assert np.array_equal(got['hist'], [4, 0, 0, 0, 1, 0, 0, 0, 0, 1]) and got['acc'] == 3.0 / 6
    assert cnt.cpu().tolist()[10:] == [1, 0, 0, 0, 1, 0, 0, 0, 0, 1]


def test_more_than_32_classes_is_unsupported_and_launches_nothing(K):
    z = torch.randn(8, 33, device='cuda')
    acc = torch.zeros(2, 34, dtype=torch.float64, device='cuda')
    cnt = torch.zeros(66, dtype=torch.int64, device='cuda')
    with pytest.raises(NotImplementedError, match='33 classes'):
        K.score_accum(z, 0, 8, 2, acc, cnt)
    with pytest.raises(NotImplementedError, match='33 classes'):
        K.score_finish(acc, 8, 2)
    torch.cuda.synchronize()
    assert not acc.any().item() and not cnt.any().item()
    acc, cnt = torch.zeros(2, 11, dtype=torch.float64, device='cuda'), torch.zeros(20, dtype=torch.int64, device='cuda')
    z = torch.randn(8, 10, device='cuda')
    for args in [(0, 1, 2), (4, 8, 2), (-1, 8, 2)]:                          # n < splits; rows past n; negative offset
        with pytest.raises(ValueError):
            K.score_accum(z, args[0], args[1], args[2], acc, cnt)
    torch.cuda.synchronize()
    assert not acc.any().item() and not cnt.any().item()


# ----------------------------------------------------------------------------------------------------- end to end
def _full_width_trainer(M):
    M.configure(INIT_ROWS=100)                         # the script's widths and image size; a shorter init batch
    return O.classifier_trainer()


def test_score_of_a_uint8_set_on_the_full_width_classifier(K, clean):
    from ctgan_amd.score_cifar import ClassifierScore
    import ctgan_amd.tflib as lib
    M = clean
    tr = _full_width_trainer(M)
    images = O.random_images(230, seed=5)
    labels = np.random.RandomState(2).randint(0, 10, 230).astype(np.int32)
    scorer = ClassifierScore(tr)
    got = scorer.score(images, labels=labels, splits=10, chunk=100)
    z = O.predict_chunks(tr, images, 100)
    _report('full_width_score_230', O.check_result(got, O.streaming_score(z, 10, 100, labels), TOL))
    # the normalised filters are made once, and the logits stay bit-equal to predict(averaged=True) on the same rows at the same chunk size
    assert len(scorer._filters) == 10
    kept = dict(scorer._filters)
    data = torch.from_numpy(images).cuda()
    for r0, m in ((0, 100), (200, 30)):
        idx = torch.arange(r0, r0 + m, dtype=torch.int32, device='cuda')
        assert torch.equal(scorer._logits(tr.gather_fixed(idx, data=data)).cpu(), torch.from_numpy(z[r0:r0 + m]))
    assert all(scorer._filters[k] is v for k, v in kept.items()) and not lib._param_aliases


def test_score_generator_on_a_resnet_gan(K, clean):
    import ctgan_amd.tflib as lib
    from ctgan_amd import evaluate
    from ctgan_amd.score_cifar import ClassifierScore
    M = clean
    tr = _full_width_trainer(M)
    lib.delete_params_with_name('Generator.')          # the classifier trainer's own generator: its names are the GAN's
    scorer = ClassifierScore(tr)
    case = H.Case(lib, 'resnet', 16, 4, 'cuda')
    try:
        gan = case.trainer()
        c0 = int(evaluate.eval_stream(gan).ctr.item())
        before = H.snapshot(lib, gan)
        got = scorer.score_generator(gan, 300)
        H.assert_same(before, H.snapshot(lib, gan))
        # the same samples: score_samples -> the three-launch composition -> the averaged classifier -> restatement
        ev = evaluate.Evaluator(gan)
        evaluate.eval_stream(gan).ctr.fill_(c0)
        labels = torch.cat([lab for _, lab in ev.score_draws(300)]).cpu().numpy()
        evaluate.eval_stream(gan).ctr.fill_(c0)
        logits = []
        for px in ev.score_samples(300, scale=evaluate.SCORE_SCALE['gan_cifar_resnet']):
            data = px.permute(0, 3, 1, 2).contiguous()
            x = K.aug_gather(data, torch.arange(data.shape[0], dtype=torch.int32, device='cuda'), scorer.lut, 32, M.cfg.PAD)
            z = tr._averaged(lambda: M._classifier(x, deterministic=True), True)
            assert torch.equal(z, tr.predict(scorer.lut[data.long()], averaged=True))
            logits.append(z)
        ref = O.streaming_score(torch.cat(logits).cpu().numpy(), 10, 1000, labels)
        _report('resnet_generator_300', O.check_result(got, ref, TOL))
        assert got['acc'] is not None and got['hist'].sum() == 300
    finally:
        case.close()


def _gan_loop(scorer, graphs, iters=5, dim=32, B=8):
    """A short gan_cifar_resnet training loop (graph replay or eager), with a scoring before the graphs are captured and after
    every second iteration when `scorer` is given -> ((critic theta, generator theta, training-stream counter), [score means])."""
    import ctgan_amd.gan_cifar_resnet as R
    import ctgan_amd.tflib as lib
    from ctgan_amd.engine import GraphedTrainer
    nrng = np.random.default_rng(77)
    batches = [(torch.from_numpy(nrng.integers(0, 256, (B, 3072), dtype=np.int32)).cuda(),
                torch.from_numpy(nrng.integers(0, 10, (B,), dtype=np.int32)).cuda()) for _ in range(8)]
    feed = iter(batches * iters)
    lib.set_seed(5)
    R.configure(DIM_G=dim, DIM_D=dim, BATCH_SIZE=B)
    try:
        R.build_params()
        tr = R.Trainer(seed=2024)
        scores = []
        if scorer is not None:
            scores.append(scorer.score_generator(tr, 200, chunk=100)['mean'])
        eng = GraphedTrainer(tr, use_graphs=graphs)
        assert eng.graphed == graphs, eng.graph_error
        for it in range(iters):
            eng.train_iteration(it, lambda: next(feed))
            if scorer is not None and it % 2 == 1:
                scores.append(scorer.score_generator(tr, 200, chunk=100)['mean'])
        torch.cuda.synchronize()
        return (tr.d_opt.theta.clone(), tr.g_opt.theta.clone(), tr.rng.ctr.clone()), scores
    finally:
        lib.delete_params_with_name('Generator.'); lib.delete_params_with_name('Discriminator.')
        R.configure()


def test_scoring_around_captured_graphs_leaves_the_training_run_bit_identical(K, clean):
    """A scoring before the GAN's graphs are captured and scorings between their replays: the graphed run's weights equal, bit for
    bit, those of an eager run that never scores, and every scoring still equals the classifier's own averaged pass - the scorer's
    constant filters are its own tensors, and nothing a captured graph holds points at them."""
    import ctgan_amd.tflib as lib
    from ctgan_amd.score_cifar import ClassifierScore
    M = clean
    tr = _full_width_trainer(M)
    lib.delete_params_with_name('Generator.')
    scorer = ClassifierScore(tr)
    stable, packs = set(K._STABLE_PTRS), len(K._pack16)
    images = O.random_images(100, seed=8)
    first = scorer.score(images, splits=4, chunk=50)
    assert set(K._STABLE_PTRS) == stable and len(K._pack16) == packs          # no cache outside the scorer holds the filters' addresses
    with_scoring, scores = _gan_loop(scorer, True)
    without, _ = _gan_loop(None, False)
    for a, b in zip(with_scoring, without):
        assert torch.equal(a, b)
    assert len(scores) == 3 and all(np.isfinite(s) for s in scores) and len(set(scores)) == 3          # the generator moved between them
    again = scorer.score(images, splits=4, chunk=50)
    assert again['mean'] == first['mean'] and np.array_equal(again['splits'], first['splits'])          # the classifier did not
    z = O.predict_chunks(tr, images, 50)
    O.check_result(again, O.streaming_score(z, 4, 50), TOL)
