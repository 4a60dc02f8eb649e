"""Host logic of the self-trained MNIST score classifier (ctgan_amd.score_mnist, tflib.ops.batchnorm with is_training, the
global-norm clip of optim.FlatAdam, engine.GraphedScoreTrainer's eager path, checkpoints) against the fp64 restatement of the script
(tests/score_oracle.py), with the HIP wrappers swapped for CPU stand-ins (tests/cpu_kernels.py + tests/score_cpu_kernels.py).  No GPU.

Bounds: those of the other step-parity tests (tests/ssl_cifar_oracle.run_steps): scalars within 2e-4 max(1, |ref|), gradients within
relative L2 max(3e-3, 3 x the oracle's own fp32 twin), updates by ssl_oracle.update_ok; moving statistics within 1e-6 max(1, |ref|)."""
import collections
import os

import numpy as np
import pytest
import torch

from tests import score_cpu_kernels as SK
from tests import score_oracle as O
from tests.ssl_oracle import update_ok

COST_TOL, GRAD_TOL, MOVING_TOL = 2e-4, 3e-3, 1e-6
WIDTHS = (8, 8, 8, 16, 16)


@pytest.fixture
def score_kernels(cpu_kernels, monkeypatch):
    import ctgan_amd.kernels as K
    import ctgan_amd.score_mnist as M
    for name in SK.__all__:
        monkeypatch.setattr(K, name, getattr(SK, name))
    yield M
    M.configure()


def _bn(name, x, **kw):
    from ctgan_amd.tflib.ops import batchnorm
    return batchnorm.Batchnorm(name, [0, 2, 3], x, **kw)


def _moving(lib, name):
    return lib._params[name + '.moving_mean'], lib._params[name + '.moving_variance']


def _close(a, b, tol, what):
    a, b = a.detach().double(), b.detach().double()
    e = (a - b).abs().max().item()
    print('%s: max abs err %.3g (ref max %.3g)' % (what, e, b.abs().max().item()))
    assert e <= tol * max(1.0, b.abs().max().item()), (what, e)


# ----------------------------------------------------------------------------- the operator API
def test_batchnorm_is_training_no_longer_raises(score_kernels):
    x = torch.randn(4, 6, 5, 5, generator=torch.Generator().manual_seed(0))
    y = _bn('A.BN', x, is_training=True, stats_iter=0)
    assert tuple(y.shape) == tuple(x.shape) and torch.isfinite(y).all()
    with torch.no_grad():
        z = _bn('A.BN', x, is_training=False)
    assert tuple(z.shape) == tuple(x.shape) and torch.isfinite(z).all()


def test_batchnorm_argument_rules(score_kernels):
    import ctgan_amd.tflib as lib
    from ctgan_amd.tflib.ops import batchnorm
    x = torch.randn(4, 6, 5, 5, generator=torch.Generator().manual_seed(1))
    with pytest.raises(ValueError):
        _bn('A.BN', x, is_training=True)                                   # update requested, no stats_iter
    _bn('A.BN', x, is_training=True, update_moving_stats=False)            # no update: no stats_iter needed
    mm, mv = _moving(lib, 'A.BN')
    assert torch.equal(mm, torch.zeros(6)) and torch.equal(mv, torch.ones(6))
    with pytest.raises(TypeError):
        _bn('A.BN', x, is_training=torch.tensor(True), stats_iter=0)
    with pytest.raises(ValueError):
        _bn('A.BN', x, is_training=True, stats_iter=0, groups=2)
    with pytest.raises(ValueError):
        _bn('A.BN', x, is_training=False, groups=2)
    with pytest.raises(RuntimeError):
        _bn('A.BN', x.clone().requires_grad_(True), is_training=False)     # the blend is forward only
    # relu= keeps working in both modes
    y = _bn('A.BN', x, is_training=True, stats_iter=3, relu=True)
    ref = torch.relu(O.bn_training(x.double(), torch.ones(6, dtype=torch.float64), torch.zeros(6, dtype=torch.float64))[0])
    _close(y, ref, 2e-5, 'training relu')
    with torch.no_grad():
        z = _bn('A.BN', x, is_training=False, relu=True)
    assert (z >= 0).all() and (z == 0).any()
    # the non-fused branch ignores is_training, as the reference's else branch
    x2 = torch.randn(5, 7, generator=torch.Generator().manual_seed(2))
    a = batchnorm.Batchnorm('B.BN', [0], x2, is_training=True)
    b = batchnorm.Batchnorm('B.BN', [0], x2)
    assert torch.equal(a, b)
    # stats_iter as a tensor: int32 or float32 scalar
    for it in (torch.tensor(2, dtype=torch.int32), torch.tensor([2.0])):
        lib._params['A.BN.moving_mean'].data.fill_(1.0)
        _bn('A.BN', x, is_training=True, stats_iter=it)
        want = O.moving_update(torch.ones(6, dtype=torch.float64), x.double().mean(dim=(0, 2, 3)), 2)
        _close(lib._params['A.BN.moving_mean'], want, MOVING_TOL, 'tensor stats_iter')


def test_is_training_none_leaves_the_moving_statistics_alone(score_kernels):
    import ctgan_amd.tflib as lib
    g = torch.Generator().manual_seed(3)
    x = torch.randn(4, 6, 5, 5, generator=g) + 3
    _bn('A.BN', x)                                                      # registers
    mm, mv = _moving(lib, 'A.BN')
    mm.data.copy_(torch.randn(6, generator=g)); mv.data.copy_(torch.rand(6, generator=g))
    before = (mm.detach().clone(), mv.detach().clone())
    y = _bn('A.BN', x.clone().requires_grad_(True))
    y.sum().backward()
    assert torch.equal(mm, before[0]) and torch.equal(mv, before[1])


@pytest.mark.parametrize('shape', [(4, 5, 3), (1, 3, 1), (1, 4, 5), (3, 6, 1)], ids=lambda s: 'n%d_c%d_h%d' % s)
@pytest.mark.parametrize('it', [0, 1, 999])
def test_moving_update_and_blend_match_the_oracle(score_kernels, shape, it):
    """(1, 3, 1): one element per channel - the divisor max(n-1, 1); (1, 4, 5): B = 1, the blend is the sample's own moments."""
    import ctgan_amd.tflib as lib
    n, c, h = shape
    g = torch.Generator().manual_seed(10 * n + c + it)
    x = torch.randn(n, c, h, h, generator=g) * 2 + 3
    scale, offset = torch.rand(c, generator=g) + .5, torch.randn(c, generator=g)
    mm0, mv0 = torch.randn(c, generator=g), torch.rand(c, generator=g) + .5
    lib.load_state_dict({'A.BN.offset': offset.clone(), 'A.BN.scale': scale.clone(), 'A.BN.moving_mean': mm0.clone(),
                         'A.BN.moving_variance': mv0.clone()}, strict=False)          # (a new parameter may share the tensor's storage)
    d = lambda t: t.double()          # noqa: E731
    y = _bn('A.BN', x, is_training=True, stats_iter=it)
    ref, bm, bv = O.bn_training(d(x), d(scale), d(offset))
    _close(y, ref, 2e-5, 'training forward')
    mm, mv = _moving(lib, 'A.BN')
    _close(mm, O.moving_update(d(mm0), bm, it), MOVING_TOL, 'moving_mean')
    _close(mv, O.moving_update(d(mv0), bv, it), MOVING_TOL, 'moving_variance')
    assert torch.isfinite(mv).all()
    if n * h * h == 1:
        assert torch.equal(bv, torch.zeros(c, dtype=torch.float64))
    if it == 0:                        # the formula as written replaces the old value
        _close(mm, bm, MOVING_TOL, 'it = 0 replaces')
    with torch.no_grad():
        z = _bn('A.BN', x, is_training=False)
    _close(z, O.bn_blend(d(x), d(scale), d(offset), d(mm.detach()), d(mv.detach())), 2e-5, 'blend forward')
    assert torch.equal(mm, _moving(lib, 'A.BN')[0]) and torch.equal(mv, _moving(lib, 'A.BN')[1])


def test_k_stats_passes_give_the_plain_mean(score_kernels):
    import ctgan_amd.tflib as lib
    g = torch.Generator().manual_seed(5)
    xs = [torch.randn(3, 4, 5, 5, generator=g) * (k + 1) + k for k in range(6)]
    for i, x in enumerate(xs):
        _bn('A.BN', x, is_training=True, stats_iter=i)
    stats = [O.bn_training(x.double(), torch.ones(4, dtype=torch.float64), torch.zeros(4, dtype=torch.float64))[1:] for x in xs]
    mm, mv = _moving(lib, 'A.BN')
    _close(mm, torch.stack([s[0] for s in stats]).mean(0), 1e-5, 'mean of batch means')
    _close(mv, torch.stack([s[1] for s in stats]).mean(0), 1e-5, 'mean of batch variances')


# ----------------------------------------------------------------------------- one step against the oracle
def _trainer_from(M, P):
    import ctgan_amd.tflib as lib
    lib.delete_all_params(); lib.set_seed(4)
    tr = M.ScoreTrainer()
    lib.load_state_dict(collections.OrderedDict((n, v.float()) for n, v in P.items()), strict=True)
    assert [n for n in lib._params] == list(P)
    return tr


def _one_step(M, clip, seed=0):
    import ctgan_amd.tflib as lib
    B = 6
    M.configure(WIDTHS=WIDTHS, BATCH_SIZE=B, CLIP_NORM=clip)
    P = O.make_params(WIDTHS, seed=seed)
    x, y = O.step_inputs(B, seed + 1)
    ref = O.train_step(P, O.zero_slots(P), 1, x.double(), y, clip=clip)
    P32 = collections.OrderedDict((n, v.float()) for n, v in P.items())
    twin = O.train_step(P32, O.zero_slots(P32), 1, x, y, clip=clip)
    tr = _trainer_from(M, P)
    tr.opt.set_lr(M.cfg.LR)
    tr.stats_iter.fill_(0)
    out = tr.losses(x, y)
    grads = torch.autograd.grad(out['cost'], tr.params, allow_unused=True)
    gradnorm = tr.opt.update_clipped(grads, M.cfg.CLIP_NORM)
    got = {'cost': out['cost'].item(), 'acc': out['acc'].item(), 'gradnorm': gradnorm.item(),
           'grads': {n: g for (n, _), g in zip(tr.named, grads)}, 'P': {n: p.detach().clone() for n, p in lib._params.items()}}
    return P, ref, twin, got, tr


def _check_step(P, ref, twin, got):
    assert O.top2_gap(ref['logits']) > 1e-3               # every row: the argmax cannot flip under fp32 noise
    for k in ('cost', 'acc', 'gradnorm'):
        a, b = got[k], float(ref[k])
        print(k, a, b)
        assert abs(a - b) <= COST_TOL * max(1.0, abs(b)), (k, a, b)
    names = [n for n in P if not O.is_moving(n)]
    assert list(got['grads']) == names
    for n in names:
        assert got['grads'][n] is not None, ('no gradient', n)
        tol = max(GRAD_TOL, 3 * O.rel_l2(twin['grads'][n], ref['grads'][n]))
        e = O.rel_l2(got['grads'][n], ref['grads'][n])
        print('grad', n, 'rel L2 %.3g' % e, 'bound %.3g' % tol)
        assert (got['grads'][n].double() - ref['grads'][n]).norm().item() <= tol * ref['grads'][n].norm().item() + 2e-6, (n, e, tol)
    factor = 5. / max(ref['gradnorm'], 5.)
    for n in P:
        if O.is_moving(n):
            _close(got['P'][n], ref['P'][n], MOVING_TOL, n)             # stats_iter 0: the batch's own statistics
        else:
            ok, how = update_ok(got['P'][n].double(), P[n], ref['P'][n], ref['grads'][n] * factor, got['grads'][n] * factor)
            assert ok, ('update', n, how)


@pytest.mark.parametrize('fused', [True, False])
def test_one_step_matches_the_oracle(score_kernels, monkeypatch, fused):
    """The fused epilogue and the unfused composition (CTGAN_SCORE_FUSED=0) both."""
    import ctgan_amd.functional as F
    monkeypatch.setattr(F, 'SCORE_FUSED', fused)
    P, ref, twin, got, _ = _one_step(score_kernels, 5.)
    _check_step(P, ref, twin, got)


@pytest.mark.parametrize('taken', [True, False])
def test_clip_branch_taken_and_not_taken(score_kernels, taken):
    """CLIP_NORM at half / ten times the ORACLE's gradient norm of this batch; the reported norm is the one before the clip."""
    M = score_kernels
    P0 = O.make_params(WIDTHS, seed=0)
    x, y = O.step_inputs(6, 1)
    g0 = O.train_step(P0, O.zero_slots(P0), 1, x.double(), y)['gradnorm']
    clip = (0.5 if taken else 10.) * g0
    P, ref, twin, got, tr = _one_step(M, clip)
    assert abs(ref['gradnorm'] - g0) < 1e-12 * g0
    assert abs(got['gradnorm'] - g0) <= COST_TOL * max(1.0, g0)
    flat_ref = torch.cat([ref['grads'][n].reshape(-1) for n in ref['grads']]) * (clip / max(g0, clip))
    e = O.rel_l2(tr.opt.grad, flat_ref)
    print('clipped bucket rel L2 %.3g, norm %.6g, clip %.6g' % (e, tr.opt.grad.double().norm().item(), clip))
    assert e < GRAD_TOL
    if taken:
        assert abs(tr.opt.grad.double().norm().item() - clip) <= 1e-5 * clip
    else:
        assert torch.equal(tr.opt.grad, torch.cat([got['grads'][n].reshape(-1) for n in got['grads']]))      # factor exactly 1


def test_stats_passes_then_evaluate_match_the_oracle(score_kernels):
    M = score_kernels
    M.configure(WIDTHS=WIDTHS, BATCH_SIZE=6)
    P = O.make_params(WIDTHS, seed=2)
    tr = _trainer_from(M, P)
    import ctgan_amd.tflib as lib
    before = {n: p.detach().clone() for n, p in lib._params.items() if not O.is_moving(n)}
    for i in range(3):
        x, _ = O.step_inputs(6, 20 + i)
        tr.bn_stats_pass(x, i)
        P = O.stats_pass(P, x.double(), i)
    for n, p in lib._params.items():
        if O.is_moving(n):
            _close(p, P[n], 1e-5, n)
        else:
            assert torch.equal(p, before[n]), ('a statistics pass moved a weight', n)
    x, y = O.step_inputs(5, 30)
    c, a, inc, logits = O.evaluate(P, x.double(), y)
    assert O.top2_gap(logits) > 1e-3
    got = tr.evaluate(x, y)
    print(got, (c, a, inc))
    assert abs(got[0] - c) <= COST_TOL * max(1, abs(c)) and got[1] == a and abs(got[2] - inc) <= COST_TOL * inc
    _close(tr.logits(x), logits, 2e-4, 'logits')


# ----------------------------------------------------------------------------- the loop
class _Epochs:
    """Deterministic epoch factory over fixed batches (counts the epochs it started)."""

    def __init__(self, batches):
        self.batches, self.started = batches, 0

    def __call__(self):
        self.started += 1
        for b in self.batches:
            yield b


def _data(B, n_train=3, n_dev=2, seed=0):
    g = torch.Generator().manual_seed(seed)
    mk = lambda: (torch.rand(B, 784, generator=g).numpy(), torch.randint(0, 10, (B,), generator=g).numpy())      # noqa: E731
    return _Epochs([mk() for _ in range(n_train)]), _Epochs([mk() for _ in range(n_dev)]), _Epochs([mk()])


def _small(M, **kw):
    M.configure(**dict(dict(WIDTHS=(4, 4, 4, 8, 8), BATCH_SIZE=4, TEST_EVERY=3, BN_STATS_ITERS=5, STOP_AFTER=7, SAVE_EVERY=3), **kw))


def test_loop_protocol(score_kernels, monkeypatch):
    """Test pass after 2 and 5 completed steps (iteration % TEST_EVERY == TEST_EVERY - 1), BN_STATS_ITERS statistics passes with
    i = 0, 1, .. over a FRESH training epoch stream before each, the logged test figures are the mean over the dev batches, train steps
    run with stats_iter 0, and the loop drops the second batch of every epoch after the first (train_loop_2.py:215-217)."""
    M = score_kernels
    _small(M)
    train_data, dev_data, test_data = _data(4)
    calls = []
    step0, stats0, eval0 = M.ScoreTrainer.step, M.ScoreTrainer.bn_stats_pass, M.ScoreTrainer.evaluate

    def which(x, batches):
        x = np.asarray(x)
        return [i for i, b in enumerate(batches) if np.array_equal(b[0], x)][0]

    def step(self, x, y):
        out = step0(self, x, y)
        calls.append(('train', which(x, train_data.batches), float(self.stats_iter.item())))
        return out

    def stats(self, x, i):
        calls.append(('stats', which(x, train_data.batches), i))
        return stats0(self, x, i)

    def evaluate(self, x, y):
        out = eval0(self, x, y)
        calls.append(('dev', which(x, dev_data.batches), out))
        return out
    monkeypatch.setattr(M.ScoreTrainer, 'step', step)
    monkeypatch.setattr(M.ScoreTrainer, 'bn_stats_pass', stats)
    monkeypatch.setattr(M.ScoreTrainer, 'evaluate', evaluate)
    lines = []
    tr = M.train((train_data, dev_data, test_data), use_graphs=False, log=lines.append)
    assert tr.iteration == 7 and tr.opt.t == 7
    kinds = [c[0] for c in calls]
    block = ['stats'] * 5 + ['dev'] * 2
    assert kinds == ['train'] * 2 + block + ['train'] * 3 + block + ['train'] * 2
    trains = [c for c in calls if c[0] == 'train']
    assert [c[1] for c in trains] == [0, 1, 2, 0, 2, 0, 2] and all(c[2] == 0.0 for c in trains)
    for first in (2, 12):
        assert [(c[1], c[2]) for c in calls[first:first + 5]] == [(0, 0), (1, 1), (2, 2), (0, 3), (1, 4)]
    tests = [ln for ln in lines if 'test cost' in ln]
    assert len(tests) == 2 and '\titeration:2\t' in tests[0] and '\titeration:5\t' in tests[1]
    devs = [c[2] for c in calls[7:9]]
    want = np.array(devs).mean(axis=0)
    assert tests[0].endswith('test cost:%.4f\ttest acc:%.4f\ttest inception:%.4f' % tuple(want))
    assert len([ln for ln in lines if 'train cost' in ln]) == 7
    assert dev_data.started == 2 and test_data.started == 0


def _state(tr):
    import ctgan_amd.tflib as lib
    s = {'p/' + n: p.detach().clone() for n, p in lib._params.items()}
    for i, b in enumerate(tr.opt.slots()):
        s['slot%d' % i] = b.clone()
    s['t'] = torch.tensor(tr.opt.t)
    return s


def test_checkpoint_round_trip_and_bit_exact_resume(score_kernels, tmp_path):
    M = score_kernels
    from ctgan_amd import checkpoint
    _small(M)
    full = _state(M.train(_data(4), use_graphs=False, log=lambda *_: None))
    a = tmp_path / 'a'; a.mkdir()
    tr = M.train(_data(4), iters=5, use_graphs=False, out_dir=str(a), log=lambda *_: None)
    saved = _state(tr)
    ck = torch.load(str(a / 'checkpoint.pt'), map_location='cpu', weights_only=False)
    assert ck['iteration'] == 5 and ck['g_opt'] is None and ck['rng'] is None
    assert any(n.endswith('.moving_variance') for n in ck['params']) and ck['d_opt']['t'] == 5
    # round trip into a fresh trainer
    import ctgan_amd.tflib as lib
    lib.delete_all_params()
    tr2 = M.ScoreTrainer()
    assert checkpoint.load(str(a / 'checkpoint.pt'), tr2) == 5
    back = _state(tr2)
    assert sorted(back) == sorted(saved) and all(torch.equal(back[n], saved[n]) for n in saved)
    # resume: the remaining two steps reproduce the uninterrupted run bit for bit, moving statistics and Adam state included
    lines = []
    resumed = _state(M.train(_data(4), use_graphs=False, resume=str(a / 'checkpoint.pt'), log=lines.append))
    assert len([ln for ln in lines if 'train cost' in ln]) == 2 and not [ln for ln in lines if 'test cost' in ln]
    assert sorted(resumed) == sorted(full)
    for n in full:
        assert torch.equal(resumed[n], full[n]), n
    assert int(full['t']) == 7 and os.path.isfile(str(a / 'log.jsonl'))


# ----------------------------------------------------------------------------- scoring
def test_inception_score_class(score_kernels, tmp_path):
    from ctgan_amd.tflib.inception_score import score_from_probabilities
    import ctgan_amd.tflib as lib
    M = score_kernels
    _small(M, STOP_AFTER=2)
    path = str(tmp_path / 'w.pt')
    with pytest.raises(ValueError):
        M.InceptionScore(weights=path)                    # no file, no data: nothing is downloaded or invented
    s1 = M.InceptionScore(weights=path, retrain=True, data=_data(4), use_graphs=False, log=lambda *_: None)
    assert os.path.isfile(path)
    x = torch.rand(7, 784, generator=torch.Generator().manual_seed(9)).numpy()
    a = s1.score(x)
    trained = {n: p.detach().clone() for n, p in lib.named_params_with_name('InceptionScore')}
    s2 = M.InceptionScore(weights=path)                   # loads: same weights (moving statistics included), same score
    for n, p in lib.named_params_with_name('InceptionScore'):
        assert torch.equal(p, trained[n]), n
    assert s2.score(x) == a
    probs = torch.softmax(s2.trainer.logits(x).double(), dim=1).numpy()
    want = score_from_probabilities(probs, splits=1)[0]
    print(a, want)
    assert abs(a - want) <= 1e-12 * want and 1.0 <= a <= 10.0
    # chunks of min(1000, len): 1500 rows -> 1000 + 500, and the blend makes the chunking visible
    big = np.concatenate([x] * 215)[:1500]
    z = np.concatenate([s2.trainer.logits(big[:1000]).double().numpy(), s2.trainer.logits(big[1000:]).double().numpy()])
    assert s2.score(big) == M.inception_from_logits(z)


def test_score_generator_leaves_the_gan_alone(score_kernels, tmp_path):
    from tests import eval_helpers as H
    import ctgan_amd.tflib as lib
    M = score_kernels
    _small(M, STOP_AFTER=1)
    case = H.Case(lib, 'mnist', 8, 4, 'cpu')
    try:
        gan = case.trainer()
        feed = iter([case.batch()[0] for _ in range(12)])
        gan.train_iteration(0, lambda: next(feed))
        path = str(tmp_path / 'w.pt')
        scorer = M.InceptionScore(weights=path, retrain=True, data=_data(4), use_graphs=False, log=lambda *_: None)
        before = H.snapshot(lib, gan)
        from ctgan_amd.evaluate import eval_stream
        ctr0 = int(eval_stream(gan).ctr.item())
        s = scorer.score_generator(gan, 10)
        assert 1.0 <= s <= 10.0
        H.assert_same(before, H.snapshot(lib, gan))        # weights (the classifier's too), optimizer slots, the training stream's counter
        assert int(eval_stream(gan).ctr.item()) == ctr0 + 1
        assert scorer.score_generator(gan, 10) != s        # the evaluation stream moved on: fresh samples
    finally:
        case.close()
