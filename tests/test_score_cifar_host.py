"""The classifier score of CIFAR-10 samples (ctgan_amd.score_cifar) without a GPU: the fp64 streaming restatement
(tests/score_cifar_oracle.py) against tflib.inception_score.score_from_probabilities, and the host logic of ClassifierScore, of
Evaluator.get_classifier_score and of record_score on CPU stand-ins (tests/score_cifar_cpu_kernels.py) against that restatement."""
import numpy as np
import pytest
import torch

from tests import eval_helpers as H
from tests import score_cifar_oracle as O
from tests.score_cifar_cpu_kernels import score_cifar_kernels        # noqa: F401  (fixture)

TOL = 1e-10


# ----------------------------------------------------------------------------------------------------- the restatement
@pytest.mark.parametrize('n,splits,chunk,scale', O.CASES)
def test_streaming_restatement_equals_score_from_probabilities(n, splits, chunk, scale):
    """The two sides differ by summation order only: 1e-12 relative (measured 4e-16)."""
    z, labels = O.logits_for(n, scale=scale, seed=n)
    got = O.streaming_score(z, splits, chunk, labels)
    mean, std = O.reference_score(z, splits)
    print('n %d: %.17g +- %.17g vs %.17g +- %.17g' % (n, got['mean'], got['std'], mean, std))
    assert abs(got['mean'] - mean) <= 1e-12 * abs(mean) and abs(got['std'] - std) <= 1e-12 * abs(mean)
    arg = z.argmax(axis=1)
    assert np.array_equal(got['hist'], np.bincount(arg, minlength=10)) and got['acc'] == float((arg == labels).sum()) / n
    assert O.streaming_score(z, splits, chunk)['acc'] is None


def test_underflowed_probabilities_add_zero_and_non_finite_logits_propagate():
    z = np.full((40, 10), -400.0, dtype=np.float32)
    z[:, 3] = 400.0
    got = O.streaming_score(z, 4, 7)
    assert (got['mean'], got['std']) == (1.0, 0.0)
    with np.errstate(all='ignore'):
        assert np.isnan(O.reference_score(z, 4)[0])               # 0 log 0 in the formula as written
    for bad in (np.nan, np.inf, -np.inf):
        z2, _ = O.logits_for(40)
        z2[5, 2] = bad
        assert np.isnan(O.streaming_score(z2, 4, 7)['mean'])


def test_stand_ins_equal_the_restatement():
    from tests import score_cifar_cpu_kernels as C
    z, labels = O.logits_for(37, K=7, scale=30.0)
    acc, cnt = torch.zeros(3, 8, dtype=torch.float64), torch.zeros(14, dtype=torch.int64)
    for r0 in range(0, 37, 7):
        C.score_accum(torch.from_numpy(z[r0:r0 + 7]), r0, 37, 3, acc, cnt, torch.from_numpy(labels[r0:r0 + 7]))
    out = C.score_finish(acc, 37, 3).numpy()
    ref = O.streaming_score(z, 3, 7, labels)
    assert np.allclose(out[2:], ref['splits'], rtol=1e-13, atol=0) and abs(out[0] - ref['mean']) < 1e-13 and abs(out[1] - ref['std']) < 1e-13
    assert np.array_equal(cnt[:7].numpy(), ref['hist']) and cnt[7:].sum().item() == round(ref['acc'] * 37)
    with pytest.raises(NotImplementedError):
        C.score_accum(torch.zeros(4, 33), 0, 4, 2, torch.zeros(2, 34, dtype=torch.float64), torch.zeros(66, dtype=torch.int64))
    # score_input against the composition it replaces, on the stand-ins of both
    import ctgan_amd.ct_cifar as M
    from tests import ssl_cifar_oracle as S

    class Kc:
        pixels_u8 = staticmethod(H.pixels_u8_cpu)
        aug_gather = staticmethod(S._aug_gather)
    lut = torch.from_numpy(M.byte_table())
    for scale in (255. / 2, 255.99 / 2):
        x = torch.from_numpy(O.edge_samples(3, 3 * 8 * 8))
        got = C.score_input(x, 3, scale, lut)
        want = O.compose_input(Kc, x, 3, scale, lut, 2)
        assert got.shape == want.shape and got.stride() == want.stride() and torch.equal(got, want)


# ----------------------------------------------------------------------------------------------------- ClassifierScore
def test_score_equals_the_restatement_on_predict_logits(score_cifar_kernels):
    import ctgan_amd.ct_cifar as M
    from ctgan_amd.score_cifar import ClassifierScore
    M.configure(**O.SMALL)
    tr = O.classifier_trainer()
    images = O.random_images(57, seed=9)
    labels = np.random.RandomState(1).randint(0, 10, 57).astype(np.int32)
    scorer = ClassifierScore(tr)
    got = scorer.score(images, labels=labels, splits=5, chunk=20)
    z = O.predict_chunks(tr, images, 20)
    assert len(set(z.argmax(axis=1))) > 1
    O.check_result(got, O.streaming_score(z, 5, 20, labels), TOL)
    assert set(got) == {'mean', 'std', 'splits', 'hist', 'acc'} and got['splits'].shape == (5,) and got['hist'].sum() == 57
    assert scorer.score(images, splits=5, chunk=20)['acc'] is None
    # the constant normalised filters: made once per parameter version, logits bit-equal to predict(averaged=True)
    idx = torch.arange(20, dtype=torch.int32)
    filters = dict(scorer._filters)
    assert len(filters) == 10
    logits = scorer._logits(tr.gather_fixed(idx, data=torch.from_numpy(images)))
    assert torch.equal(logits, torch.from_numpy(z[:20]))
    assert all(scorer._filters[k] is v for k, v in filters.items())
    import ctgan_amd.tflib as lib
    assert not lib._param_aliases
    version = lib.epoch('Classifier')                       # one real classifier step moves the version: the filters are made again
    idx4 = lambda *v: torch.tensor(v, dtype=torch.int32)          # noqa: E731
    tr.d_opt.set_lr(0.05)
    tr.d_body_idx(idx4(0, 5, 7, 2), idx4(1, 2, 3, 4), idx4(7, 6, 3, 1))
    assert lib.epoch('Classifier') != version
    with torch.no_grad():                                   # (the average moves by 1e-4 of the step: bring it to the live values)
        tr.d_opt.avg.copy_(tr.d_opt.theta)
    again = scorer.score(images, labels=labels, splits=5, chunk=20)
    O.check_result(again, O.streaming_score(O.predict_chunks(tr, images, 20), 5, 20, labels), TOL)
    assert again['mean'] != got['mean'] and all(scorer._filters[k] is not v for k, v in filters.items())
    with pytest.raises(ValueError):
        scorer.score(images[:4], splits=5)                       # n < splits
    with pytest.raises(ValueError):
        scorer.score(images[:, :, :16, :16])                     # not the classifier's IMG


def _checkpoint_scorer(tmp_path):
    """A checkpoint of a classifier trainer -> (ClassifierScore(weights=...), the averaged values by name, the trainer's live values)."""
    import ctgan_amd.tflib as lib
    from ctgan_amd import checkpoint
    from ctgan_amd.score_cifar import ClassifierScore
    tr = O.classifier_trainer()
    path = str(tmp_path / 'ct.pt')
    checkpoint.save(path, tr, 1)
    avg = {n: a.detach().clone() for n, a in tr.d_opt.avg_views()}
    live = {n: p.detach().clone() for n, p in lib._params.items()}
    lib.delete_all_params()
    return ClassifierScore(weights=path), avg, live, path


def test_checkpoint_round_trip_loads_only_the_classifier(score_cifar_kernels, tmp_path):
    import ctgan_amd.ct_cifar as M
    import ctgan_amd.tflib as lib
    from ctgan_amd.score_cifar import ClassifierScore
    M.configure(**O.SMALL)
    scorer, avg, live, path = _checkpoint_scorer(tmp_path)
    names = list(lib._params)
    assert names and all(n.startswith('Classifier.') for n in names) and not [n for n in names if 'Generator' in n]
    assert names == [n for n in live if n.startswith('Classifier.')]
    for n, p in lib._params.items():
        assert torch.equal(p.detach(), avg[n] if n in avg else live[n]), n
    assert 'Classifier.3.g' not in avg and 'Classifier.10.g' in avg
    with pytest.raises(ValueError, match='already holds'):
        ClassifierScore(weights=path)
    with pytest.raises(ValueError):
        ClassifierScore()
    with pytest.raises(ValueError, match='data_dir'):
        ClassifierScore(weights=str(tmp_path / 'none.pt'))
    lib.delete_all_params()
    M.configure(**dict(O.SMALL, D_WIDTHS=(8, 8, 8, 16, 16, 16, 16, 16, 4)))
    with pytest.raises(ValueError, match='does not fit'):
        ClassifierScore(weights=path)
    assert not lib._params
    M.configure(**dict(O.SMALL, N_CLASSES=33))
    with pytest.raises(ValueError, match='33 classes'):
        ClassifierScore(O.classifier_trainer())


@pytest.mark.parametrize('te', [False, True])
def test_missing_checkpoint_trains_saves_and_drops_the_generator(score_cifar_kernels, tmp_path, te):
    import ctgan_amd.ct_cifar as M
    import ctgan_amd.ct_cifar_te as T
    import ctgan_amd.tflib as lib
    from ctgan_amd.score_cifar import ClassifierScore
    (T if te else M).configure(**dict(O.SMALL, IMG=16))
    arrays = {'x_train': O.random_images(40, 16), 'y_train': np.arange(40) % 10, 'x_test': O.random_images(8, 16, seed=1), 'y_test': np.arange(8) % 10}
    path = str(tmp_path / 'trained.pt')
    scorer = ClassifierScore(weights=path, arrays=arrays, epochs=1, te=te, use_graphs=False, max_batches=2, log=lambda *a: None)
    assert not [n for n in lib._params if 'Generator' in n] and len(lib._params) == 30
    got = scorer.score(arrays['x_test'], splits=2)
    assert np.isfinite(got['mean']) and got['hist'].sum() == 8
    kept = {n: p.detach().clone() for n, p in lib._params.items()}
    lib.delete_all_params()
    again = ClassifierScore(weights=path)                        # what was saved is a checkpoint the loader takes: the same averaged values
    for n, p in lib._params.items():
        assert torch.equal(p.detach(), kept[n]), n
    assert again.score(arrays['x_test'], splits=2)['mean'] == got['mean']


# ----------------------------------------------------------------------------------------------------- generators
def _reference_generator_score(scorer, gan, name, n, chunk, splits, c0, given=None):
    """The same samples through score_samples -> the three-launch composition -> the classifier's plain deterministic pass -> restatement."""
    import ctgan_amd.ct_cifar as M
    import ctgan_amd.kernels as K
    from ctgan_amd import evaluate
    ev = evaluate.Evaluator(gan)
    evaluate.eval_stream(gan).ctr.fill_(c0)
    labs = [lab for _, lab in ev.score_draws(n, given, chunk=chunk)]
    evaluate.eval_stream(gan).ctr.fill_(c0)
    logits = []
    for px in ev.score_samples(n, given, scale=evaluate.SCORE_SCALE[name], chunk=chunk):
        data = px.permute(0, 3, 1, 2).contiguous()
        x = K.aug_gather(data, torch.arange(data.shape[0], dtype=torch.int32, device=data.device), scorer.lut, M.cfg.IMG, M.cfg.PAD)
        with torch.no_grad():
            logits.append(M._classifier(x, deterministic=True))
    labels = None if labs[0] is None else torch.cat(labs).cpu().numpy()
    return O.streaming_score(torch.cat(logits).cpu().numpy(), splits, chunk, labels)


@pytest.mark.parametrize('name', ['resnet', 'cifar'])
def test_score_generator_equals_the_restatement_and_leaves_the_trainer_alone(score_cifar_kernels, tmp_path, name):
    import ctgan_amd.ct_cifar as M
    import ctgan_amd.tflib as lib
    from ctgan_amd import evaluate
    M.configure(**O.SMALL)
    scorer, _, _, _ = _checkpoint_scorer(tmp_path)
    case = H.Case(lib, name, 16 if name == 'resnet' else 8, 4, 'cpu')
    try:
        gan = case.trainer()
        long_name = 'gan_cifar_resnet' if name == 'resnet' else 'gan_cifar'
        c0 = int(evaluate.eval_stream(gan).ctr.item())
        before = H.snapshot(lib, gan)
        got = scorer.score_generator(gan, 300, chunk=200)
        assert int(evaluate.eval_stream(gan).ctr.item()) == c0 + 2          # one step of the EVALUATION stream per generator call
        H.assert_same(before, H.snapshot(lib, gan))                         # training stream, weights (the classifier's too), Adam state
        ref = _reference_generator_score(scorer, gan, long_name, 300, 200, 10, c0)
        O.check_result(got, ref, TOL)
        assert (got['acc'] is not None) == (name == 'resnet') and got['hist'].sum() == 300
        ev = evaluate.Evaluator(gan)
        evaluate.eval_stream(gan).ctr.fill_(c0)
        assert ev.get_classifier_score(300, scorer)['hist'].sum() == 300
        with pytest.raises(ValueError):
            scorer.score_generator(gan, 5)
        if name == 'resnet':                                  # given labels replace the drawn ones
            evaluate.eval_stream(gan).ctr.fill_(c0)
            lab = ((np.arange(100) * 7) % 10).astype(np.int32)
            a = scorer.score_generator(gan, 100, labels=lab)
            ref_given = _reference_generator_score(scorer, gan, long_name, 100, 1000, 10, c0, given=torch.from_numpy(lab))
            ref_drawn = _reference_generator_score(scorer, gan, long_name, 100, 1000, 10, c0)
            O.check_result(a, ref_given, TOL)                      # acc counts argmax == the GIVEN label, on samples generated from them
            assert (ref_given['mean'], ref_given['acc']) != (ref_drawn['mean'], ref_drawn['acc'])
    finally:
        case.close()


def test_other_image_sizes_are_refused(score_cifar_kernels, tmp_path):
    import ctgan_amd.ct_cifar as M
    import ctgan_amd.tflib as lib
    M.configure(**O.SMALL)
    scorer, _, _, _ = _checkpoint_scorer(tmp_path)
    for name in ('64x64', 'mnist'):
        case = H.Case(lib, name, 4, 4, 'cpu')
        try:
            with pytest.raises(ValueError, match='are not 3x32x32 images'):
                scorer.score_generator(case.trainer(), 100)
        finally:
            case.M.configure()
            lib.delete_params_with_name('Generator')
            lib.delete_params_with_name('Discriminator')


# ----------------------------------------------------------------------------------------------------- the loops' hook
class _Series:
    def __init__(self):
        self.rows = []

    def add(self, name, value):
        self.rows.append((name, value))


@pytest.mark.parametrize('name', ['resnet', 'cifar'])
def test_record_score_takes_the_device_path_for_a_classifier_score(score_cifar_kernels, tmp_path, monkeypatch, name):
    import ctgan_amd.ct_cifar as M
    import ctgan_amd.tflib as lib
    from ctgan_amd import evaluate
    M.configure(**O.SMALL)
    scorer, _, _, _ = _checkpoint_scorer(tmp_path)
    long_name = 'gan_cifar_resnet' if name == 'resnet' else 'gan_cifar'
    monkeypatch.setitem(evaluate.SCORE_SAMPLES, long_name, 200)
    case = H.Case(lib, name, 16 if name == 'resnet' else 8, 4, 'cpu')
    try:
        gan = case.trainer()
        ev = evaluate.Evaluator(gan)
        c0 = int(evaluate.eval_stream(gan).ctr.item())

        def stub(x):                       # a host callable: today's path, unchanged
            assert isinstance(x, np.ndarray) and x.dtype == np.float32 and x.shape[1:] == (32, 32, 3)
            z = x.reshape(x.shape[0], -1)[:, :3070].reshape(x.shape[0], 10, -1).mean(axis=2) / 16.
            p = np.exp(z - z.max(axis=1, keepdims=True))
            return p / p.sum(axis=1, keepdims=True)
        s = _Series()
        evaluate.record_score(ev, s, stub)
        evaluate.eval_stream(gan).ctr.fill_(c0)
        want = ev.get_inception_score(200, stub)
        assert s.rows == list(zip(evaluate.SCORE_SERIES[long_name], want))
        evaluate.eval_stream(gan).ctr.fill_(c0)
        d = _Series()
        evaluate.record_score(ev, d, scorer)
        evaluate.eval_stream(gan).ctr.fill_(c0)
        res = scorer.score_generator(gan, 200)
        if name == 'resnet':
            assert d.rows == [('inception_50k', res['mean']), ('inception_50k_std', res['std']), ('score_acc', res['acc'])]
        else:
            assert d.rows == [('inception score', res['mean'])]
    finally:
        case.close()


def test_score_entry_points_validate_before_any_launch():
    """Argument validation happens before a launch, so it is observable without a GPU: the unsupported class count, n < splits, rows past n."""
    from ctgan_amd import _lib
    lib = _lib.lib
    assert lib.ctgan_score_accum(None, 8, 33, 0, 8, 2, None, None, None, None) == -2 and b'33 classes' in lib.ctgan_last_error()
    assert lib.ctgan_score_finish(None, 8, 2, 33, None, None) == -2
    assert lib.ctgan_score_accum(None, 1, 10, 0, 1, 2, None, None, None, None) == -1             # n < splits
    assert lib.ctgan_score_accum(None, 8, 10, 4, 8, 2, None, None, None, None) == -1             # rows [4, 12) of 8
    assert lib.ctgan_score_accum(None, 8, 10, 0, 8, 2, None, None, None, None) == -1             # null state
    assert lib.ctgan_score_finish(None, 8, 2, 10, None, None) == -1
    assert lib.ctgan_score_input(None, 2, 3, 32, 0.0, None, None, None) == -1
    assert lib.ctgan_score_input(None, 2, 17, 32, 127.5, None, None, None) == -1
