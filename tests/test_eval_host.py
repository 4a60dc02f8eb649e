"""Host logic of ctgan_amd.evaluate - the held-out critic cost in wide passes, its stream separation, the score path - and of the
training loops that call it, with the HIP wrappers swapped for CPU stand-ins (tests/cpu_kernels.py; the stand-ins of the wrappers that
table lacks come from tests/test_gan_modes_host.py and tests/eval_helpers.py).  No GPU."""
import gzip
import json
import os
import pickle

import numpy as np
import pytest
import torch

from tests import eval_helpers as H
from tests.test_gan_modes_host import mode_kernels        # noqa: F401  (fixture: cpu_kernels + the MODE work's stand-ins)

N_DEV = 5          # dev batches per case: at width 2 the last pass is ragged


@pytest.fixture
def eval_kernels(mode_kernels, monkeypatch):       # noqa: F811
    import ctgan_amd.kernels as K
    monkeypatch.setattr(K, 'pixels_u8', H.pixels_u8_cpu)
    return mode_kernels


def _case(name):
    import ctgan_amd.tflib as lib
    dim = 4 if name.startswith('64x64') else 8
    return H.Case(lib, name, dim, 4, 'cpu')


def _dev_set(case, n=N_DEV):
    pairs = [case.batch() for _ in range(n)]
    rnds = [case.draws() for _ in range(n)]
    return [p[0] for p in pairs], [p[1] for p in pairs], rnds


# ----------------------------------------------------------------------------- 1, 2: parity with the fp64 oracle, width invariance
@pytest.mark.parametrize('name', H.CASES)
def test_dev_cost_matches_the_oracle_and_does_not_depend_on_width(eval_kernels, name):
    from ctgan_amd.evaluate import Evaluator
    case = _case(name)
    try:
        tr = case.trainer()
        batches, batches_o, rnds = _dev_set(case)
        costs, reg = case.oracle_costs(tr, batches_o, rnds)
        want = sum(costs) / len(costs)
        rnd32 = [H.f32_rnd(r, 'cpu') for r in rnds]
        got = {}
        for width in (2, 1, 5):
            out = Evaluator(tr, width=width).dev_cost(iter(batches), rnd=rnd32)
            assert out['n_batches'] == N_DEV and isinstance(out['dev_cost'], float)
            print('%s width %d: dev_cost %.9g, oracle %.9g' % (name, width, out['dev_cost'], want))
            H.close(out['dev_cost'], want, '%s width %d vs oracle' % (name, width))
            got[width] = out
        for width in (1, 5):
            H.close(got[width]['dev_cost'], got[2]['dev_cost'], '%s width %d vs width 2' % (name, width))
        if name == 'cifar':
            ref = H.slope_real_ref(reg, case.D, batches_o[-1], rnds[-1]['u_slope'])
            for width in (2, 1, 5):
                print('cifar width %d: slope_real %.9g, fp64 %.9g' % (width, got[width]['slope_real'], ref))
                H.close(got[width]['slope_real'], ref, 'slope_real width %d' % width)
        else:
            assert 'slope_real' not in got[2]
    finally:
        case.close()


def test_default_widths_and_bad_arguments(eval_kernels):
    from ctgan_amd import evaluate
    from ctgan_amd.evaluate import Evaluator
    assert set(evaluate.DEFAULT_WIDTH) == {'gan_cifar_resnet', 'gan_cifar', 'gan_mnist', 'gan_64x64', 'gan_lsun128'}
    assert evaluate.DEFAULT_WIDTH['gan_lsun128'] == 1
    case = _case('mnist')
    try:
        tr = case.trainer()
        ev = Evaluator(tr)
        assert ev.width == evaluate.DEFAULT_WIDTH['gan_mnist'] and not ev.with_slope
        with pytest.raises(ValueError):
            Evaluator(tr, width=0)
        with pytest.raises(ValueError):
            ev.dev_cost(iter([]))
        with pytest.raises(NotImplementedError):
            next(ev.score_samples(100))              # one-channel output: the MNIST script scores nothing
        batches, _, rnds = _dev_set(case, 2)
        with pytest.raises(ValueError):
            ev.dev_cost(iter(batches), rnd=[H.f32_rnd(rnds[0], 'cpu')])
    finally:
        case.close()


# ----------------------------------------------------------------------------- 3: no training work, no side effects
@pytest.mark.parametrize('name', ['resnet', 'cifar', 'mnist-wgan', '64x64'])
def test_dev_cost_does_no_training_work_and_leaves_the_trainer_alone(eval_kernels, monkeypatch, name):
    import ctgan_amd.kernels as K
    import ctgan_amd.tflib as lib
    from ctgan_amd.evaluate import Evaluator
    case = _case(name)
    try:
        tr = case.trainer()
        batches, _, _ = _dev_set(case, 3)
        feed = iter(batches * 8)
        tr.train_iteration(0, lambda: next(feed))              # optimizer slots, counters and weights away from their initial values
        tr.train_iteration(1, lambda: next(feed))
        calls = []
        for nm in [n for n in dir(K) if n.startswith('conv_wgrad') and callable(getattr(K, n))]:
            monkeypatch.setattr(K, nm, (lambda f, nm=nm: lambda *a, **kw: (calls.append(nm), f(*a, **kw))[1])(getattr(K, nm)))
        before = H.snapshot(lib, tr)
        epochs = (lib.epoch(), lib.epoch('Discriminator'), lib.epoch('Generator'))
        ev = Evaluator(tr, width=2)
        vals, n = ev.dev_cost_device(iter(batches))
        assert n == 3 and all(torch.isfinite(v).item() for v in vals.values())
        assert not calls, calls
        assert all(v.grad_fn is None and not v.requires_grad for v in vals.values())
        assert set(vals) == ({'dev_cost', 'slope_real'} if name == 'cifar' else {'dev_cost'})
        H.assert_same(before, H.snapshot(lib, tr))
        assert epochs == (lib.epoch(), lib.epoch('Discriminator'), lib.epoch('Generator'))
        assert int(ev.rng.ctr.item()) == 2 + (1 if name == 'cifar' else 0)                  # one step per pass (+ the slope pass)
    finally:
        case.close()


# ----------------------------------------------------------------------------- 4: stream separation
@pytest.mark.parametrize('name', ['resnet', 'cifar'])
def test_training_with_dev_passes_equals_training_without(eval_kernels, name):
    from ctgan_amd.evaluate import Evaluator, eval_stream
    res = {}
    for with_dev in (False, True):
        case = _case(name)
        try:
            tr = case.trainer(seed=5)
            batches, _, _ = _dev_set(case, 3)
            feed = iter(batches * 8)
            ev = Evaluator(tr, width=2)
            for it in range(3):
                tr.train_iteration(it, lambda: next(feed))
                if with_dev:
                    ev.dev_cost(iter(batches))
            res[with_dev] = (tr.d_opt.theta.clone(), tr.g_opt.theta.clone(), tr.d_opt.m.clone(), tr.g_opt.m.clone(), tr.rng.ctr.clone())
            if with_dev:
                c0 = int(eval_stream(tr).ctr.item())
                a = ev.dev_cost(iter(batches))
                b = ev.dev_cost(iter(batches))
                assert a['dev_cost'] != b['dev_cost']                      # consecutive passes: fresh draws
                eval_stream(tr).ctr.fill_(c0)
                c = Evaluator(tr, width=2).dev_cost(iter(batches))         # another evaluator at the same counter: the same draws
                assert c == a
        finally:
            case.close()
    for x, y in zip(res[False], res[True]):
        assert torch.equal(x, y)


# ----------------------------------------------------------------------------- 5: the loops
def _read_log(path):
    return [json.loads(line) for line in open(path)]


def _write_mnist(path, n_train, n_dev):
    g = np.random.default_rng(3)
    splits = [(g.random((n, 784), dtype=np.float32), g.integers(0, 10, n)) for n in (n_train, n_dev, n_dev)]
    with gzip.open(path, 'wb') as f:
        pickle.dump(tuple(splits), f, protocol=2)


def test_mnist_loop_logs_dev_cost_and_resumes(eval_kernels, monkeypatch, tmp_path):
    """gan_mnist.train on a synthetic mnist.pkl.gz: `dev disc cost` at exactly the dev_every iterations, sample grid, checkpoint; a run
    resumed from the checkpoint logs the dev cost of the uninterrupted run (the feeds are made order-preserving, and an epoch is one
    iteration's worth of batches, so both runs see the same batches)."""
    import ctgan_amd.gan_mnist as M
    import ctgan_amd.tflib as lib
    from ctgan_amd import checkpoint
    from ctgan_amd.evaluate import eval_stream
    monkeypatch.setattr(np.random, 'shuffle', lambda a: None)
    data = str(tmp_path / 'mnist.pkl.gz')
    _write_mnist(data, 20, 12)
    kw = dict(use_graphs=False, sample_every=3, dev_every=3, checkpoint_every=3, seed=9, log=None)

    def run(out, **more):
        lib.delete_all_params(); lib.set_device('cpu'); lib.set_seed(2)
        M.configure(DIM=8, BATCH_SIZE=4)
        os.makedirs(out, exist_ok=True)
        try:
            return M.train(data, n_examples=20, out_dir=out, **dict(kw, **more))
        finally:
            M.configure()

    a, b = str(tmp_path / 'a'), str(tmp_path / 'b')
    tr = run(a, iters=6)
    assert tr.d_opt.t == 30 and tr.g_opt.t == 5
    log = _read_log(os.path.join(a, 'log.jsonl'))
    assert [r['iter'] for r in log] == [0, 1, 2, 3, 4, 5]
    assert [r['iter'] for r in log if 'dev disc cost' in r] == [2, 5]
    assert all('train disc cost' in r and 'time' in r and 'slope_real' not in r for r in log)
    assert all(os.path.exists(os.path.join(a, f)) for f in ('samples_2.png', 'samples_5.png', 'checkpoint.pt'))
    assert int(eval_stream(tr).ctr.item()) == 2                  # 3 dev batches at the default width: one pass per dev evaluation
    run(b, iters=3)
    run(b, iters=6, resume=os.path.join(b, 'checkpoint.pt'))
    log_b = _read_log(os.path.join(b, 'log.jsonl'))
    assert [r['iter'] for r in log_b] == [0, 1, 2, 3, 4, 5]
    for ra, rb in zip(log, log_b):
        assert ra['train disc cost'] == rb['train disc cost']
        assert ra.get('dev disc cost') == rb.get('dev disc cost')
    # a checkpoint written before the evaluation counter existed still loads, with the counter at 0
    path = os.path.join(a, 'checkpoint.pt')
    ck = torch.load(path, map_location='cpu', weights_only=False)
    assert ck['format'] == 1 and ck['rng']['eval_ctr'] == 2
    del ck['rng']['eval_ctr']
    torch.save(ck, path)
    lib.delete_all_params(); lib.set_device('cpu')
    M.configure(DIM=8, BATCH_SIZE=4)
    try:
        from ctgan_amd import dcgan_step
        dcgan_step.build_params(M)
        tr2 = dcgan_step.DCGANTrainer(M, seed=1)
        eval_stream(tr2).ctr.fill_(7)
        assert checkpoint.load(path, tr2) == 6
        assert int(eval_stream(tr2).ctr.item()) == 0 and tr2.rng.seed == 9
        assert eval_stream(tr2).seed == (9 + 0x9E3779B97F4A7C15) % 2 ** 64
    finally:
        M.configure()


def test_cifar_loop_logs_dev_cost_and_slope_real(eval_kernels, monkeypatch, tmp_path):
    import ctgan_amd.gan_cifar as M
    import ctgan_amd.tflib as lib
    g = np.random.default_rng(0)
    for name, rows in [('data_batch_%d' % k, 4) for k in range(1, 6)] + [('test_batch', 12)]:
        with open(os.path.join(str(tmp_path), name), 'wb') as f:
            pickle.dump({'data': g.integers(0, 256, (rows, 3072), dtype=np.uint8), 'labels': [int(v) for v in g.integers(0, 10, rows)]}, f, protocol=2)
    lib.delete_all_params(); lib.set_device('cpu'); lib.set_seed(2)
    M.configure(DIM=8, BATCH_SIZE=4)
    scored = []

    def classifier(x):
        scored.append(x.shape[0])
        return np.full((x.shape[0], 10), 0.1)
    try:
        tr = M.train(str(tmp_path), n_examples=20, iters=4, out_dir=str(tmp_path), use_graphs=False, sample_every=2, dev_every=2,
                     checkpoint_every=4, score_every=4, classifier=classifier, log=None)
        assert tr.d_opt.t == 20 and tr.g_opt.t == 3
        log = _read_log(os.path.join(str(tmp_path), 'log.jsonl'))
        assert [r['iter'] for r in log] == [0, 1, 2, 3]
        assert [r['iter'] for r in log if 'dev disc cost' in r] == [1, 3] == [r['iter'] for r in log if 'slope_real' in r]
        assert all(np.isfinite(r['dev disc cost']) and r['slope_real'] > 0 for r in log if 'slope_real' in r)
        assert [r['iter'] for r in log if 'inception score' in r] == [3] and abs(log[3]['inception score'] - 1.0) < 1e-12
        assert sum(scored) == 1000                          # the script scores 1000 samples (TF/CT_gan_cifar.py:171)
        assert all(os.path.exists(os.path.join(str(tmp_path), f)) for f in ('samples_1.png', 'samples_3.png', 'checkpoint.pt'))
    finally:
        M.configure(); lib.delete_all_params()


# ----------------------------------------------------------------------------- 6: the score path
def test_inception_score_feeds_the_classifier_nhwc_floats(eval_kernels):
    from ctgan_amd.evaluate import Evaluator
    from ctgan_amd.tflib.inception_score import score_from_probabilities
    case = _case('resnet')
    try:
        tr = case.trainer()
        before = tr.rng.ctr.clone()
        seen, outs = [], []

        def stub(x):
            assert isinstance(x, np.ndarray) and x.dtype == np.float32 and x.shape[1:] == (32, 32, 3)
            assert x.min() >= 0 and x.max() <= 255 and np.all(x == np.floor(x))
            seen.append(x)
            z = x.reshape(x.shape[0], -1)[:, :3070].reshape(x.shape[0], 10, -1).mean(axis=2) / 16.
            p = np.exp(z - z.max(axis=1, keepdims=True))
            outs.append(p / p.sum(axis=1, keepdims=True))
            return outs[-1]
        ev = Evaluator(tr)
        score = ev.get_inception_score(300, stub)
        assert sum(x.shape[0] for x in seen) == 300
        assert score == score_from_probabilities(np.concatenate(outs, 0), 10)
        assert torch.equal(before, tr.rng.ctr)
        # chunks: statistic groups of 100, several per generator call; a trailing partial group is cut
        chunks = [c for c in ev.score_samples(250, chunk=200)]
        assert [tuple(c.shape) for c in chunks] == [(200, 32, 32, 3), (50, 32, 32, 3)] and all(c.dtype == torch.uint8 for c in chunks)
        lab = torch.arange(100, dtype=torch.int32) % 10
        a = next(ev.score_samples(100, labels=lab))
        assert a.shape == (100, 32, 32, 3)
        with pytest.raises(ValueError):
            next(ev.score_samples(100, chunk=150))
    finally:
        case.close()
