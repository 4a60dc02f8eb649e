"""The semi-supervised CT classifier (ctgan_amd.ct_mnist) without a GPU: self-checks of its fp64 oracle (tests/ssl_oracle.py) against
closed forms, the host logic of the trainer on CPU stand-ins of the new kernel wrappers against that oracle, the Config literals,
the host data class, a checkpoint round trip, and the oracle pinned to the committed fixture tests/golden/ssl_step.npz."""
import math
import os

import numpy as np
import pytest
import torch

from tests import ssl_oracle as O

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'ssl_step.npz')


@pytest.fixture
def ssl_kernels(cpu_kernels, monkeypatch):
    import ctgan_amd.ct_mnist as M
    import ctgan_amd.tflib as lib
    O.install_stand_ins(monkeypatch)
    yield cpu_kernels
    M.configure(); lib.delete_all_params(); lib.delete_param_aliases()


def _small():
    import ctgan_amd.ct_mnist as M
    return M.Config(IN_DIM=20, HIDDEN=(24, 16, 12, 12, 12), N_CLASSES=10, Z_DIM=8, G_HIDDEN=(16, 16), BATCH_SIZE=8, INIT_ROWS=40)


# ----------------------------------------------------------------------------------------------------- oracle self-checks
def test_oracle_weight_norm_columns_have_norm_s():
    g = torch.Generator().manual_seed(0)
    theta = torch.randn(37, 11, generator=g, dtype=torch.float64)
    s = torch.rand(11, generator=g, dtype=torch.float64) + 0.5
    W = O.wn_weight(theta, s)
    assert torch.allclose(W.norm(dim=0), s, rtol=1e-13, atol=0)


def test_oracle_init_normalises_every_pre_activation():
    cfg = _small()
    P = O.make_params(cfg, seed=1)
    x = torch.rand(cfg.INIT_ROWS, cfg.IN_DIM, generator=torch.Generator().manual_seed(2), dtype=torch.float64)
    pre = []
    O.init_pass(P, cfg, x, seed=3, step=0, pre=pre)
    assert len(pre) == len(cfg.HIDDEN) + 1
    for a in pre:
        assert a.mean(dim=0).abs().max().item() < 1e-12 and ((a * a).mean(dim=0) - 1).abs().max().item() < 1e-12
    # ... and the stored (s, b) reproduce them: the same noisy pass without init gives the normalised pre-activations + 0
    noise = O._site_noise(cfg, 3, 0, cfg.INIT_ROWS, 0, len(cfg.HIDDEN), torch.float64)
    logits = O.classifier(P, cfg, x, noise)
    assert (logits - pre[-1]).abs().max().item() < 1e-10


def test_oracle_weight_norm_gradient_equals_the_formula():
    g = torch.Generator().manual_seed(4)
    theta = torch.randn(13, 5, generator=g, dtype=torch.float64, requires_grad=True)
    s = (torch.rand(5, generator=g, dtype=torch.float64) + 0.5).requires_grad_(True)
    gW = torch.randn(13, 5, generator=g, dtype=torch.float64)
    for eps in (0.0, 1e-6):
        gt, gs = torch.autograd.grad(O.wn_weight(theta, s, eps), [theta, s], gW)
        ft, fs = O.wn_grad_formula(gW, theta.detach(), s.detach(), eps)
        assert torch.allclose(gt, ft, rtol=1e-12, atol=1e-14) and torch.allclose(gs, fs, rtol=1e-12, atol=1e-14)


def test_oracle_adam_first_step():
    g = torch.tensor([1e-3, -0.5, 2.0, 30.0, -1e-6], dtype=torch.float64)
    p0 = torch.tensor([0.1, -0.2, 0.3, 0.4, -0.5], dtype=torch.float64)
    p, m, v = O.adam_theano(p0, g, torch.zeros_like(g), torch.zeros_like(g), 1, 0.003)
    assert torch.allclose(p0 - p, 0.003 * g / torch.sqrt(g * g + 1e-8), rtol=1e-12, atol=0)
    assert torch.allclose(m, 0.5 * g) and torch.allclose(v, 0.001 * g * g)


def test_oracle_loss_unl_at_zero_logits():
    cfg = _small()
    B = 4
    logits = torch.zeros(4 * B, 10, dtype=torch.float64)
    out4, ct_i = O._head_terms(logits, torch.zeros(B, dtype=torch.int32), B, cfg.LAMBDA_2, cfg.Factor_M)
    sp = math.log(10) + math.log1p(1 / 10.)          # softplus(log 10) = log(1 + 10)
    assert abs(out4[1].item() - 0.5 * (-math.log(10) + 2 * sp)) < 1e-14
    assert abs(out4[0].item() - math.log(10)) < 1e-14 and out4[2].item() == 0 and ct_i.abs().max().item() == 0


def test_oracle_head_is_stable_at_large_logits():
    B = 3
    g = torch.Generator().manual_seed(5)
    logits = torch.where(torch.rand(4 * B, 10, generator=g) < 0.5, -80.0, 80.0).double()
    out4, ct_i = O._head_terms(logits, torch.tensor([0, 3, 9], dtype=torch.int32), B, 0.1, 0.0)
    assert torch.isfinite(out4).all() and torch.isfinite(ct_i).all()


# ----------------------------------------------------------------------------------------------------- config, data
def test_config_literals():
    import ctgan_amd.ct_mnist as M
    c = M.Config()
    assert (c.BATCH_SIZE, c.COUNT, c.UNLABELED_WEIGHT, c.LAMBDA_2, c.Factor_M, c.LR) == (100, 10, 1., .1, 0., .003)
    assert (c.SEED, c.SEED_DATA, c.BETA1, c.BETA2, c.AVG_RATE, c.EPOCHS, c.INIT_ROWS) == (2, 2, 0.5, 0.999, 1e-4, 300, 500)
    assert (c.IN_DIM, c.HIDDEN, c.N_CLASSES, c.Z_DIM, c.G_HIDDEN) == (784, (1000, 500, 250, 250, 250), 10, 100, (500, 500))
    assert (c.SIGMA_IN, c.SIGMA_HIDDEN) == (0.3, 0.5)
    with pytest.raises(AttributeError):
        M.Config(NOPE=1)
    assert M.configure(BATCH_SIZE=7).BATCH_SIZE == 7 and M.configure().BATCH_SIZE == 100


def _fake_mnist(n_train=300, n_valid=100, n_test=60, seed=0):
    r = np.random.RandomState(seed)
    mk = lambda n: (r.rand(n, 784).astype(np.float32), (np.arange(n) % 10).astype(np.int64))      # noqa: E731
    (xt, yt), (xv, yv), (xs, ys) = mk(n_train), mk(n_valid), mk(n_test)
    return {'x_train': xt, 'y_train': yt, 'x_valid': xv, 'y_valid': yv, 'x_test': xs, 'y_test': ys}


def test_ssl_data_pick_and_streams(tmp_path):
    import ctgan_amd.ct_mnist as M
    arrays = _fake_mnist()
    path = str(tmp_path / 'mnist.npz')
    np.savez(path, **arrays)
    d = M.SSLData(path, count=3, batch_size=20)
    assert d.txs.shape == (30, 784) and sorted(np.bincount(d.tys, minlength=10)) == [3] * 10
    assert d.tys.dtype == np.int32 and d.unl.shape == (400, 784) and d.init_batch.shape == (400, 784)      # fewer than INIT_ROWS rows exist
    allx = np.concatenate([arrays['x_train'], arrays['x_valid']])
    inds = np.random.RandomState(2).permutation(400)
    ally = np.concatenate([arrays['y_train'], arrays['y_valid']])[inds]
    assert np.array_equal(d.txs[:3], allx[inds][ally == 0][:3])          # the first COUNT of each class after the seed_data permutation
    n = d.begin_epoch()
    assert n == 20 and d.lab_x.shape == (390, 784) and d.lab_y.shape == (390,)      # 400 // 30 = 13 permutations of the labelled set
    for k in range(13):
        assert sorted(d.lab_y[30 * k:30 * (k + 1)].tolist()) == sorted(d.tys.tolist())
    srt = lambda a: a[np.lexsort(a.T[::-1])]                                              # noqa: E731
    assert np.array_equal(srt(d.unl), srt(allx)) and np.array_equal(srt(d.unl2), srt(allx))
    assert not np.array_equal(d.unl, d.unl2) and not np.array_equal(d.unl, allx)      # two independent shuffles
    x_lab, y, x_unl, x_unl2 = d.batch(2)
    assert x_lab.shape == (20, 784) and y.shape == (20,) and np.array_equal(x_unl, d.unl[40:60]) and np.array_equal(x_unl2, d.unl2[40:60])
    first = d.unl.copy()
    d.begin_epoch()
    assert not np.array_equal(first, d.unl)
    # same seeds, same streams; dict input equals file input
    e = M.SSLData(arrays=arrays, count=3, batch_size=20)
    e.begin_epoch(); e.begin_epoch()
    assert np.array_equal(e.unl, d.unl) and np.array_equal(e.lab_y, d.lab_y)
    with pytest.raises(IOError, match='not downloaded'):
        M.SSLData(str(tmp_path / 'missing.npz'))


# ----------------------------------------------------------------------------------------------------- host logic on stand-ins
def test_registry_and_trainable_set(ssl_kernels):
    import ctgan_amd.ct_mnist as M
    import ctgan_amd.tflib as lib
    cfg = O.small_cfg()
    tr = M.SSLTrainer(seed=1)
    names, trainable = O.d_names(cfg)
    assert [n for n in lib._params if n.startswith('Classifier')] == names
    assert [n for n, _ in tr.d_named] == trainable and [n for n, _ in tr.g_named] == O.g_names(cfg)
    assert lib._non_trainable == {'Classifier.%d.weight_scale' % l for l in range(1, 6)}
    assert tuple(lib._params['Classifier.1.theta'].shape) == (20, 24) and tuple(lib._params['Classifier.6.theta'].shape) == (12, 10)
    th = lib._params['Classifier.3.theta'].detach()
    assert abs(th.std().item() - 0.1) < 0.02 and lib._params['Classifier.3.weight_scale'].eq(1).all() and lib._params['Classifier.3.b'].eq(0).all()
    assert tr.d_opt.kind == 'adam_theano' and tr.d_opt.avg is not None and tr.g_opt.avg is None and tr.d_opt.avg.eq(0).all()


def test_weightnorm_argument_of_the_tf_operators_still_raises(ssl_kernels):
    from ctgan_amd.tflib.ops import linear
    with pytest.raises(NotImplementedError):
        linear.Linear('l', 4, 4, torch.zeros(1, 4), weightnorm=True)


def test_trainer_steps_match_oracle_host_logic(ssl_kernels):
    """Init, one classifier step, one generator step at reduced widths: the project's host-logic bounds (cost 1e-5, gradient relative L2
    1e-4), only the trainable set moves, s_1..s_5 unchanged by training, the generator step leaves D untouched, averages from zero."""
    O.small_cfg()
    assert O.run_steps('cpu', cost_tol=1e-5, grad_tol=1e-4) == 13 + 7


def test_averages_follow_the_rule_from_zero(ssl_kernels):
    import ctgan_amd.ct_mnist as M
    cfg = O.small_cfg()
    tr = M.SSLTrainer(seed=3)
    g = torch.Generator().manual_seed(0)
    B = cfg.BATCH_SIZE
    tr.init_params(torch.rand(cfg.INIT_ROWS, cfg.IN_DIM, generator=g))
    avg = torch.zeros_like(tr.d_opt.theta)
    scales = {l: tr_p.detach().clone() for l, tr_p in ((l, M.lib._params['Classifier.%d.weight_scale' % l]) for l in range(1, 6))}
    for it in range(3):
        x = [torch.rand(B, cfg.IN_DIM, generator=g) for _ in range(3)]
        y = torch.randint(0, 10, (B,), generator=g, dtype=torch.int32)
        d_before = tr.d_opt.theta.clone()
        tr.d_step(x[0], y, x[1])
        avg = avg + 1e-4 * (tr.d_opt.theta - avg)
        assert torch.allclose(tr.d_opt.avg, avg, rtol=1e-6, atol=1e-12) and not torch.equal(tr.d_opt.theta, d_before)
        d_after, a_after = tr.d_opt.theta.clone(), tr.d_opt.avg.clone()
        tr.g_step(x[2])
        assert torch.equal(tr.d_opt.theta, d_after) and torch.equal(tr.d_opt.avg, a_after)
    for l, s in scales.items():
        assert torch.equal(M.lib._params['Classifier.%d.weight_scale' % l].detach(), s)
    assert tr.d_opt.t == 3 and tr.g_opt.t == 3 and int(tr.rng.ctr.item()) == 7
    assert abs(tr.d_opt.state[1].item() - 0.5 ** 4) < 1e-7


def test_predict_uses_averages_and_live_scales(ssl_kernels):
    import ctgan_amd.ct_mnist as M
    import ctgan_amd.tflib as lib
    cfg = O.small_cfg()
    tr = M.SSLTrainer(seed=3)
    g = torch.Generator().manual_seed(1)
    x = torch.rand(cfg.BATCH_SIZE, cfg.IN_DIM, generator=g)
    tr.init_params(torch.rand(cfg.INIT_ROWS, cfg.IN_DIM, generator=g))
    tr.d_opt.avg.copy_(torch.randn(tr.d_opt.avg.shape, generator=g) * 0.1)
    P = {n: p.detach().double() for n, p in lib._params.items()}
    live = O.classifier(P, cfg, x.double())
    P.update({n: a.detach().double() for n, a in tr.d_opt.avg_views()})
    avg = O.classifier(P, cfg, x.double())
    assert (tr.predict(x, averaged=False).double() - live).abs().max().item() < 1e-4
    assert (tr.predict(x).double() - avg).abs().max().item() < 1e-4 * max(1.0, avg.abs().max().item())
    assert not lib._param_aliases
    y = avg.argmax(1).numpy()
    assert tr.test_error(x.numpy(), y) == 0.0 and tr.test_error(x.numpy(), (y + 1) % 10) == 1.0


def test_checkpoint_round_trip(ssl_kernels, tmp_path):
    import ctgan_amd.ct_mnist as M
    import ctgan_amd.tflib as lib
    from ctgan_amd import checkpoint
    cfg = O.small_cfg()
    g = torch.Generator().manual_seed(2)
    B = cfg.BATCH_SIZE
    batches = [([torch.rand(B, cfg.IN_DIM, generator=g) for _ in range(3)], torch.randint(0, 10, (B,), generator=g, dtype=torch.int32))
               for _ in range(4)]
    x0 = torch.rand(cfg.INIT_ROWS, cfg.IN_DIM, generator=g)

    def run(tr, lo, hi):
        for x, y in batches[lo:hi]:
            tr.train_iteration(x[0], y, x[1], x[2])

    def snap(tr):
        return ({n: p.detach().clone() for n, p in lib._params.items()},
                [t.clone() for o in (tr.d_opt, tr.g_opt) for t in o.slots()], int(tr.rng.ctr.item()), tr.d_opt.t, tr.g_opt.t)
    lib.set_seed(5)
    tr = M.SSLTrainer(seed=9)
    tr.init_params(x0)
    run(tr, 0, 2)
    path = str(tmp_path / 'ck.pt')
    checkpoint.save(path, tr, 2)
    run(tr, 2, 4)
    want = snap(tr)
    lib.delete_all_params(); lib.set_seed(77)
    tr2 = M.SSLTrainer(seed=1)
    assert checkpoint.load(path, tr2) == 2
    run(tr2, 2, 4)
    got = snap(tr2)
    assert all(torch.equal(got[0][n], want[0][n]) for n in want[0]) and all(torch.equal(a, b) for a, b in zip(got[1], want[1]))
    assert got[2:] == want[2:]
    # another optimizer's state is refused
    ck = torch.load(path, weights_only=False)
    ck['d_opt']['kind'] = 'adam'
    torch.save(ck, path)
    with pytest.raises(ValueError, match='cannot be loaded'):
        checkpoint.load(path, tr2)


def test_train_runs_the_scripts_loop(ssl_kernels, tmp_path, monkeypatch):
    """train() on an mnist.npz-format file (eager: no graphs without a GPU) prints the script's per-epoch line and resumes."""
    import ctgan_amd.ct_mnist as M
    M.configure(HIDDEN=(16, 12, 8, 8, 8), G_HIDDEN=(12, 12), Z_DIM=6, BATCH_SIZE=20, COUNT=2, EPOCHS=2, INIT_ROWS=50)
    path = str(tmp_path / 'mnist.npz')
    np.savez(path, **_fake_mnist(80, 20, 40))
    lines = []
    tr = M.train(path, use_graphs=False, out_dir=str(tmp_path), log=lines.append)
    assert len(lines) == 2 and lines[1].startswith('Iteration 1, time = ')
    for key in ('loss_lab = ', 'loss_unl = ', 'train err = ', 'test err = '):
        assert key in lines[0]
    assert tr.iteration == 10 and os.path.exists(str(tmp_path / 'checkpoint.pt')) and os.path.exists(str(tmp_path / 'log.jsonl'))
    want = tr.d_opt.theta.clone()
    # one epoch, then a resumed second epoch: the same weights and the same report line as the uninterrupted run
    os.makedirs(str(tmp_path / 'b'))
    M.train(path, epochs=1, use_graphs=False, out_dir=str(tmp_path / 'b'), log=lambda s: None)
    lines2 = []
    tr2 = M.train(path, epochs=2, use_graphs=False, resume=str(tmp_path / 'b' / 'checkpoint.pt'), out_dir=str(tmp_path / 'b'), log=lines2.append)
    assert torch.equal(tr2.d_opt.theta, want) and torch.equal(tr2.d_opt.avg, tr.d_opt.avg)
    assert len(lines2) == 1 and lines2[0].split('loss_lab')[1] == lines[1].split('loss_lab')[1]
    with pytest.raises(IOError):
        M.train(str(tmp_path / 'nope.npz'), use_graphs=False)


# ----------------------------------------------------------------------------------------------------- fixture
def test_oracle_is_pinned_to_the_committed_fixture():
    """tests/golden/ssl_step.npz (written by tests/golden/make_ssl_golden.py) holds the oracle's outputs for the init, one classifier and
    one generator step at reduced widths; the GPU suite pins the product to the same file."""
    O.small_cfg()
    try:
        import ctgan_amd.ct_mnist as M
        assert O.golden_matches(O.oracle_golden(M.cfg), np.load(GOLDEN)) > 30
    finally:
        M.configure()
