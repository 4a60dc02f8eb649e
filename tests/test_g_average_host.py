"""The generator's weight average (optim.FlatAdam / FlatRMSProp `avg_rate`, the trainers' `g_average` and `averaged()`, the `averaged`
flag of the evaluation) without a GPU, on the CPU stand-ins of tests/avg_cpu_kernels.py.  Not in the reference: the checks are the
feature's own contract - the fp32 recurrence bit for bit, nothing changed when the rate is 0, a pure exchange, exact resume."""
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from tests import eval_helpers as H
from tests.avg_cpu_kernels import avg_kernels, mode_kernels        # noqa: F401  (fixtures)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RATE = 0.125          # large enough that every step moves the average by many ulps


def _params(g, head='Generator'):
    return [(head + '.W', torch.nn.Parameter(torch.randn(3, 5, generator=g))), (head + '.b', torch.nn.Parameter(torch.randn(7, generator=g)))]


def _make(kind, g, rate, **kw):
    from ctgan_amd.optim import FlatAdam, FlatRMSProp
    if kind == 'adam':
        return FlatAdam(_params(g), 0.5, 0.9, avg_rate=rate, **kw)
    return FlatRMSProp(_params(g), clip=0.05 if kind == 'rmsprop-clip' else None, avg_rate=rate, **kw)


def recurrence(avg, theta, rate):
    """avg + rate * (theta - avg) in IEEE fp32, one rounding per operation."""
    a, t = avg.numpy().astype(np.float32), theta.numpy().astype(np.float32)
    return torch.from_numpy((a + np.float32(rate) * (t - a)).astype(np.float32))


@pytest.mark.parametrize('kind', ['adam', 'rmsprop', 'rmsprop-clip'])
def test_average_starts_at_the_weights_and_follows_the_fp32_recurrence(avg_kernels, kind):
    g = torch.Generator().manual_seed(3)
    opt = _make(kind, g, RATE)
    assert opt.avg is not opt.theta and torch.equal(opt.avg, opt.theta) and opt.avg.data_ptr() != opt.theta.data_ptr()
    assert [tuple(v.shape) for _, v in opt.avg_views()] == [(3, 5), (7,)] and [n for n, _ in opt.avg_views()] == opt.names
    opt.set_lr(0.01)
    want = opt.avg.clone()
    for k in range(5):
        grads = [torch.randn(3, 5, generator=g), None if k == 2 else torch.randn(7, generator=g)]
        if k == 1:
            grads[0][1, 2] = float('inf')          # a skipped element: its weight stays, its average still follows it
        if k % 2:
            opt.update(grads, 0.5)
        else:
            opt.gather_grads(grads)
            opt.step(0.5)
        want = recurrence(want, opt.theta, RATE)
        assert torch.equal(opt.avg, want), (kind, k)
    assert not torch.equal(opt.avg, opt.theta) and opt.skipped() == 1
    if kind == 'rmsprop-clip':
        assert float(opt.theta.abs().max()) <= 0.05 + 1e-9


@pytest.mark.parametrize('kind', ['adam', 'rmsprop', 'rmsprop-clip'])
def test_rate_zero_changes_nothing_and_the_average_moves_no_other_state(avg_kernels, kind):
    runs = {}
    for rate in (0.0, RATE):
        g = torch.Generator().manual_seed(5)
        opt = _make(kind, g, rate)
        opt.set_lr(0.01)
        for k in range(3):
            opt.update([torch.randn(3, 5, generator=g), torch.randn(7, generator=g)])
        runs[rate] = opt
    off, on = runs[0.0], runs[RATE]
    assert off.avg is None
    with pytest.raises(ValueError):
        from ctgan_amd.optim import averaged
        with averaged(off):
            pass
    if kind == 'adam':
        assert [a is b for a, b in zip(off.slots(), (off.m, off.v, off.state))] == [True] * 3 and len(off.slots()) == 3
        assert sorted(off.state_dict()) == ['kind', 'm', 'state', 't', 'v']
    else:
        assert len(off.slots()) == (3 if off.clip > 0 else 2) and off.slots()[0] is off.ms and off.slots()[1] is off.state
        assert sorted(off.state_dict()) == ['kind', 'ms', 'state', 't']
    assert len(on.slots()) == len(off.slots()) + 1 and on.slots()[-1] is on.avg
    assert sorted(on.state_dict()) == sorted(list(off.state_dict()) + ['avg'])
    assert torch.equal(on.theta, off.theta) and torch.equal(on.state, off.state)
    for a, b in zip(on.slots()[:-1], off.slots()):
        assert torch.equal(a, b)


def test_avg_rate_is_validated():
    g = torch.Generator().manual_seed(1)
    for bad in (-0.1, 1.5):
        with pytest.raises(ValueError):
            _make('adam', g, bad)


def test_theano_adam_keeps_its_own_average_from_zeros():
    from ctgan_amd.optim import FlatAdamTheano
    g = torch.Generator().manual_seed(1)
    th = FlatAdamTheano(_params(g, 'Classifier'), 0.9, 0.999, avg_rate=0.01)
    assert torch.equal(th.avg, torch.zeros_like(th.theta)) and not th._avg_own
    assert [a is b for a, b in zip(th.slots(), (th.m, th.v, th.state, th.avg))] == [True] * 4 and len(th.slots()) == 4
    assert sorted(th.state_dict()) == ['avg', 'kind', 'm', 'state', 't', 'v'] and th.state_dict()['kind'] == 'adam_theano'
    plain = FlatAdamTheano(_params(g, 'Classifier'), 0.9, 0.999)
    assert plain.avg is None and len(plain.slots()) == 3 and 'avg' not in plain.state_dict()
    sd = th.state_dict(); del sd['avg']
    with pytest.raises(KeyError):
        th.load_state_dict(sd)          # as before: its average is part of its state


@pytest.mark.parametrize('kind', ['adam', 'rmsprop'])
def test_state_dict_round_trip_and_loading_states_without_an_average(avg_kernels, kind):
    g = torch.Generator().manual_seed(9)
    a = _make(kind, g, RATE)
    a.set_lr(0.01)
    a.update([torch.randn(3, 5, generator=g), torch.randn(7, generator=g)])
    sd = a.state_dict()
    assert torch.equal(sd['avg'], a.avg) and sd['avg'].data_ptr() != a.avg.data_ptr()
    b = _make(kind, torch.Generator().manual_seed(10), RATE)
    b.theta.copy_(a.theta)          # (checkpoint.load: parameters first)
    b.load_state_dict(sd)
    assert torch.equal(b.avg, a.avg) and not torch.equal(b.avg, b.theta) and b.t == a.t
    old = {k: v for k, v in sd.items() if k != 'avg'}          # a checkpoint of a run that kept no average
    b.load_state_dict(old)
    assert torch.equal(b.avg, b.theta) and b.avg.data_ptr() != b.theta.data_ptr()
    c = _make(kind, torch.Generator().manual_seed(11), 0.0)
    c.load_state_dict(sd)           # an average in the file, none kept: ignored
    assert c.avg is None and 'avg' not in c.state_dict()


# ----------------------------------------------------------------------------- trainers
def _dcgan_trainer(lib, name, g_average, seed=3):
    from ctgan_amd.dcgan_step import DCGANTrainer
    case = H.Case(lib, name, 8, 4, 'cpu')
    return case, DCGANTrainer(case.M, seed=seed, g_average=g_average)


@pytest.mark.parametrize('name', ['mnist-dcgan', 'mnist-wgan'])          # an Adam mode and an RMSProp mode
def test_averaged_context_is_a_pure_exchange(avg_kernels, name):
    import ctgan_amd.tflib as lib
    case, tr = _dcgan_trainer(lib, name, RATE)
    try:
        assert tr.d_opt.avg is None and tr.g_opt.avg is not None          # the critic is never averaged
        real = case.batch()[0]
        for it in range(3):
            tr.train_iteration(it, lambda: real)
        theta, avg = tr.g_opt.theta.clone(), tr.g_opt.avg.clone()
        assert not torch.equal(theta, avg)
        want = [(n, v.clone()) for n, v in tr.g_opt.avg_views()]
        e0 = lib.epoch('Generator')
        with tr.averaged():
            assert lib.epoch('Generator') != e0
            e1 = lib.epoch('Generator')
            for (n, p), (m, v) in zip(tr.g_named, want):
                assert n == m and torch.equal(lib.param(n).detach(), v) and p.data_ptr() == lib.param(n).data_ptr()
            assert torch.equal(tr.g_opt.avg, theta)
        assert lib.epoch('Generator') != e1
        assert torch.equal(tr.g_opt.theta, theta) and torch.equal(tr.g_opt.avg, avg)
        with pytest.raises(KeyError):
            with tr.averaged():
                raise KeyError('body')
        assert torch.equal(tr.g_opt.theta, theta) and torch.equal(tr.g_opt.avg, avg)
        from ctgan_amd.dcgan_step import DCGANTrainer, sample_grid
        noise = torch.randn(4, 128, generator=torch.Generator().manual_seed(0))
        live, mean = sample_grid(case.M, noise), sample_grid(case.M, noise, tr, averaged=True)
        assert live.shape == mean.shape and not np.array_equal(live, mean) and np.array_equal(sample_grid(case.M, noise), live)
        with pytest.raises(ValueError):
            sample_grid(case.M, noise, averaged=True)
        plain = DCGANTrainer(case.M, seed=3)
        assert plain.g_opt.avg is None
        with pytest.raises(ValueError):
            with plain.averaged():
                pass
    finally:
        case.close()


def test_resnet_trainer_averages_the_generator_only(avg_kernels):
    import ctgan_amd.tflib as lib
    case = H.Case(lib, 'resnet', 8, 4, 'cpu')
    try:
        tr = case.M.Trainer(seed=2, g_average=RATE)
        assert tr.d_opt.avg is None and torch.equal(tr.g_opt.avg, tr.g_opt.theta) and len(tr.g_opt.slots()) == 4 and len(tr.d_opt.slots()) == 3
        (real, labels), _ = case.batch()
        for it in range(2):
            tr.train_iteration(it, lambda: (real, labels))
        assert not torch.equal(tr.g_opt.avg, tr.g_opt.theta)
        noise = torch.randn(4, 128, generator=torch.Generator().manual_seed(0))
        lab = torch.arange(4, dtype=torch.int32)
        s_live, _ = tr.generate_samples(noise, lab)
        s_avg, px = tr.generate_samples(noise, lab, averaged=True)
        with tr.averaged():
            s_in, _ = tr.generate_samples(noise, lab)
        assert torch.equal(s_avg, s_in) and not torch.equal(s_avg, s_live) and px.dtype == torch.int32
        assert torch.equal(tr.generate_samples(noise, lab)[0], s_live)
        with pytest.raises(ValueError):
            with case.M.Trainer(seed=2).averaged():
                pass
    finally:
        case.close()


def test_checkpoint_resume_equals_the_uninterrupted_run(avg_kernels, tmp_path):
    import ctgan_amd.tflib as lib
    from ctgan_amd import checkpoint
    path = str(tmp_path / 'ck.pt')
    ends = {}
    for run in ('whole', 'resumed'):
        case, tr = _dcgan_trainer(lib, 'mnist-dcgan', RATE)
        try:
            g = torch.Generator().manual_seed(4)
            feed = [torch.rand(4, 784, generator=g) for _ in range(4)]
            start = 0
            if run == 'resumed':
                start = checkpoint.load(path, tr)
                assert start == 2 and not torch.equal(tr.g_opt.avg, tr.g_opt.theta)
            for it in range(start, 4):
                tr.train_iteration(it, lambda: feed[it])
                if run == 'whole' and it == 1:
                    checkpoint.save(path, tr, it + 1)
            ends[run] = {'theta': tr.g_opt.theta.clone(), 'avg': tr.g_opt.avg.clone(), 'm': tr.g_opt.m.clone(), 'd': tr.d_opt.theta.clone()}
        finally:
            case.close()
    for k in ends['whole']:
        assert torch.equal(ends['whole'][k], ends['resumed'][k]), k
    ck = torch.load(path, map_location='cpu', weights_only=False)
    assert 'avg' in ck['g_opt'] and 'avg' not in ck['d_opt']
    # averaging switched on at the resume of a checkpoint written without it
    del ck['g_opt']['avg']
    torch.save(ck, path)
    case, tr = _dcgan_trainer(lib, 'mnist-dcgan', RATE)
    try:
        assert checkpoint.load(path, tr) == 2
        assert torch.equal(tr.g_opt.avg, tr.g_opt.theta) and torch.equal(tr.g_opt.theta, torch.cat([ck['params'][n].reshape(-1) for n in tr.g_opt.names]))
    finally:
        case.close()


class _Series:
    def __init__(self):
        self.rows = []

    def add(self, name, value):
        self.rows.append((name, value))


def test_record_score_averaged_writes_the_avg_series_only(avg_kernels, monkeypatch):
    import ctgan_amd.tflib as lib
    from ctgan_amd import evaluate
    from ctgan_amd.dcgan_step import DCGANTrainer
    monkeypatch.setattr(evaluate.K, 'pixels_u8', H.pixels_u8_cpu)
    monkeypatch.setitem(evaluate.SCORE_SAMPLES, 'gan_cifar', 200)
    case = H.Case(lib, 'cifar', 8, 4, 'cpu')
    try:
        tr = DCGANTrainer(case.M, seed=1, g_average=RATE)
        real = case.batch()[0]
        for it in range(2):
            tr.train_iteration(it, lambda: real)
        ev = evaluate.Evaluator(tr)
        stream = evaluate.eval_stream(tr)
        c0 = int(stream.ctr.item())

        def stub(x):
            z = x.reshape(x.shape[0], -1)[:, :3070].reshape(x.shape[0], 10, -1).mean(axis=2) / 16.
            p = np.exp(z - z.max(axis=1, keepdims=True))
            return p / p.sum(axis=1, keepdims=True)
        theta, avg = tr.g_opt.theta.clone(), tr.g_opt.avg.clone()
        live, mean = _Series(), _Series()
        evaluate.record_score(ev, live, stub)
        c1 = int(stream.ctr.item())
        evaluate.record_score(ev, mean, stub, averaged=True)          # the loops' order: live, then the average on the next steps
        assert int(stream.ctr.item()) - c1 == c1 - c0 > 0
        assert torch.equal(tr.g_opt.theta, theta) and torch.equal(tr.g_opt.avg, avg)
        names = evaluate.SCORE_SERIES['gan_cifar']
        assert [n for n, _ in live.rows] == list(names) and [n for n, _ in mean.rows] == [n + '_avg' for n in names]
        stream.ctr.fill_(c1)
        with tr.averaged():
            want = ev.get_inception_score(200, stub)
        assert [v for _, v in mean.rows] == list(want)[:len(names)]
        stream.ctr.fill_(c1)
        assert [v for _, v in mean.rows] == list(ev.get_inception_score(200, stub, averaged=True))[:len(names)]
        stream.ctr.fill_(c0)
        assert [v for _, v in live.rows] == list(ev.get_inception_score(200, stub))[:len(names)]
        assert [v for _, v in live.rows] != [v for _, v in mean.rows]
        # a scoring that is abandoned half way still puts the live weights back
        it = ev.score_draws(200, chunk=100, averaged=True)
        next(it)
        assert torch.equal(tr.g_opt.theta, avg)
        it.close()
        assert torch.equal(tr.g_opt.theta, theta) and torch.equal(tr.g_opt.avg, avg)
    finally:
        case.close()


# ----------------------------------------------------------------------------- two ranks
def _worker(rank, world, port, out_dir):
    sys.path.insert(0, ROOT)
    torch.set_num_threads(2)
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank), MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port))
    import ctgan_amd.kernels as K
    from tests import avg_cpu_kernels as A
    from tests.test_ddp_gloo import _patch_cpu
    lib = _patch_cpu()
    for name in A.__all__:
        if name != 'exchange_':
            A._BASE[name] = getattr(K, name)
        setattr(K, name, getattr(A, name))
    import ctgan_amd.gan_cifar_resnet as R
    from ctgan_amd import ddp
    from ctgan_amd.engine import GraphedTrainer
    ddp.init_from_env(backend='gloo')
    lib.set_seed(7 + rank)                        # different inits: the broadcast makes the weights - and the average - the same
    R.configure(DIM_G=8, DIM_D=8, BATCH_SIZE=4)
    R.build_params('cpu')
    tr = R.Trainer(seed=1, rank=rank, world_size=world, allreduce=ddp.FlatAllReduce(), g_average=RATE)
    ddp.broadcast_params([tr.d_opt.theta, tr.g_opt.theta, tr.g_opt.avg])
    eng = GraphedTrainer(tr, use_graphs=False)
    g = torch.Generator().manual_seed(500 + rank)          # per-rank shards
    for it in range(3):
        eng.train_iteration(it, lambda: (torch.randint(0, 256, (4, 3072), generator=g, dtype=torch.int32),
                                         torch.randint(0, 10, (4,), generator=g, dtype=torch.int32)))
    torch.save({'theta': tr.g_opt.theta.clone(), 'avg': tr.g_opt.avg.clone(), 't': tr.g_opt.t}, os.path.join(out_dir, 'avg_rank%d.pt' % rank))
    ddp.barrier()
    torch.distributed.destroy_process_group()
    R.configure()


def test_two_ranks_end_with_the_same_average(tmp_path):
    """No collective of its own: every rank applies the same reduced gradient to the same weights, so the averages agree bit for bit."""
    world = 2
    s = socket.socket(); s.bind(('127.0.0.1', 0)); port = s.getsockname()[1]; s.close()
    mp.spawn(_worker, args=(world, port, str(tmp_path)), nprocs=world, join=True)
    res = [torch.load(os.path.join(str(tmp_path), 'avg_rank%d.pt' % r)) for r in range(world)]
    assert res[0]['t'] == res[1]['t'] == 2
    assert torch.equal(res[0]['theta'], res[1]['theta']) and torch.equal(res[0]['avg'], res[1]['avg'])
    assert not torch.equal(res[0]['avg'], res[0]['theta'])
