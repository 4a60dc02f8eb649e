"""The dynamic loss scale (optim.LossScaler, the `scaler=` path of FlatAdam / FlatRMSProp, DCGANTrainer(loss_scale=), the checkpoint
entry) without a GPU, on the stand-ins of tests/loss_scale_cpu_kernels.py.  Not in the reference: the checks are the feature's own
contract - the state machine against a few lines of plain Python, a good step equal to the static path bit for bit, a dropped step that
changes nothing, exact round trips, two ranks that take the same decision."""
import os
import socket
import sys

import pytest
import torch
import torch.multiprocessing as mp

from tests import eval_helpers as H
from tests.loss_scale_cpu_kernels import avg_kernels, mode_kernels, scale_kernels        # noqa: F401  (fixtures)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _params(g, head='Generator'):
    return [(head + '.W', torch.nn.Parameter(torch.randn(3, 5, generator=g))), (head + '.b', torch.nn.Parameter(torch.randn(7, generator=g)))]


def _make(kind, g, scaler, rate=0.0):
    from ctgan_amd.optim import FlatAdam, FlatRMSProp
    kw = {'scaler': scaler} if scaler is not None else {}
    if kind == 'adam':
        return FlatAdam(_params(g), 0.5, 0.9, avg_rate=rate, **kw)
    return FlatRMSProp(_params(g), clip=0.05 if kind == 'rmsprop-clip' else None, avg_rate=rate, **kw)


def _scaler(**kw):
    from ctgan_amd.optim import LossScaler
    return LossScaler(device='cpu', **kw)


class PlainScaler:
    """The scheme in plain Python."""

    def __init__(self, init, growth, lo, hi):
        self.S, self.good, self.skipped, self.growth, self.lo, self.hi = init, 0, 0, growth, lo, hi

    def end(self, found):
        if found:
            self.S, self.good, self.skipped = max(self.S / 2, self.lo), 0, self.skipped + 1
        else:
            self.good += 1
            if self.good == self.growth:
                self.S, self.good = min(2 * self.S, self.hi), 0


# ----------------------------------------------------------------------------- the state machine
def test_state_machine_against_plain_python(scale_kernels):
    from ctgan_amd.rng import DeviceRNG
    sc = _scaler(init_scale=8.0, growth_interval=3, min_scale=2.0, max_scale=32.0)
    ref = PlainScaler(8.0, 3, 2.0, 32.0)
    g = torch.Generator().manual_seed(2)
    opt = _make('adam', g, sc)
    opt.set_lr(0.01)
    rng = DeviceRNG(5, 0, 'cpu')
    assert sc.seed().data_ptr() == sc.state.data_ptr() and sc.seed().dim() == 0 and sc.scale() == 8.0
    # overflow pattern: growth at exactly 3 good updates (twice, to the upper clamp and held there), then five backoffs to the lower clamp
    pattern = [0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 0, 0, 1, 1, 1, 1, 1, 0, 0, 0, 1]
    seen = []
    for k, bad in enumerate(pattern):
        grads = [torch.randn(3, 5, generator=g) * sc.scale(), torch.randn(7, generator=g) * sc.scale()]
        if bad:
            grads[k % 2].view(-1)[k % 7] = [float('inf'), float('-inf'), float('nan')][k % 3]
        before = (opt.theta.clone(), opt.m.clone(), opt.v.clone(), opt.state.clone(), int(rng.ctr.item()))
        if k % 2:
            opt.update(grads, 1.0, rng=rng)
        else:
            opt.gather_grads(grads)
            opt.step(1.0, rng=rng)
        ref.end(bool(bad))
        assert (sc.scale(), sc.good_steps(), sc.skipped_steps()) == (ref.S, ref.good, ref.skipped), k
        assert float(sc.state[1]) == 0.0, 'found is cleared at the end of the step'
        assert int(rng.ctr.item()) == before[4] + 1, 'the Philox counter advances on a skipped step too'
        if bad:
            assert torch.equal(opt.theta, before[0]) and torch.equal(opt.m, before[1]) and torch.equal(opt.v, before[2])
            assert torch.equal(opt.state, before[3]), 'the beta powers are frozen on a skipped step'
        else:
            assert not torch.equal(opt.theta, before[0])
            assert torch.equal(opt.state[1:3], before[3][1:3] * torch.tensor([0.5, 0.9]))
        seen.append(sc.scale())
    assert seen[2] == 16.0 and seen[1] == 8.0 and seen[5] == 32.0 and seen[8] == 32.0          # growth at exactly 3, clamp at max
    assert min(seen) == 2.0 and seen.count(2.0) >= 2                                            # clamp at min
    assert opt.t == len(pattern) and opt.skipped() == 0          # t counts attempts; a dropped update does not count elements


def test_scaler_validation():
    from ctgan_amd.optim import FlatAdamTheano, LossScaler
    for kw in ({'init_scale': 3.0}, {'min_scale': 0.75}, {'max_scale': 1000.0}, {'init_scale': 0.0}, {'init_scale': -2.0},
               {'init_scale': float('inf')}, {'init_scale': 2.0, 'min_scale': 4.0}, {'init_scale': 2.0 ** 25}, {'growth_interval': 0},
               {'growth_interval': 1.5}):
        with pytest.raises(ValueError):
            LossScaler(device='cpu', **kw)
    sc = LossScaler(device='cpu')
    assert (sc.init_scale, sc.growth_interval, sc.min_scale, sc.max_scale) == (2.0 ** 16, 2000, 1.0, 2.0 ** 24)
    assert sc.state.tolist() == [65536.0, 0.0, 0.0, 0.0]
    assert LossScaler(init_scale=0.5, min_scale=2.0 ** -10, device='cpu').scale() == 0.5
    with pytest.raises(ValueError):
        FlatAdamTheano(_params(torch.Generator().manual_seed(0), 'Classifier'), 0.9, 0.999, scaler=sc)


@pytest.mark.parametrize('kind', ['adam', 'rmsprop', 'rmsprop-clip'])
def test_no_scaler_changes_nothing_at_the_optimizer(scale_kernels, kind, monkeypatch):
    """Without a scaler the launches carry no `scaler` keyword and slots() / state_dict() are what they were."""
    import ctgan_amd.kernels as K
    seen = []
    for name in ('adam_step', 'adam_step_packed', 'rmsprop_step', 'rmsprop_step_packed', 'step_advance', 'grads_nonfinite'):
        def spy(*a, _f=getattr(K, name), _n=name, **kw):
            seen.append((_n, sorted(kw)))
            return _f(*a, **kw)
        monkeypatch.setattr(K, name, spy)
    g = torch.Generator().manual_seed(5)
    opt = _make(kind, g, None)
    opt.set_lr(0.01)
    opt.update([torch.randn(3, 5, generator=g), torch.randn(7, generator=g)], 0.5)
    assert [kw for _, kw in seen] == [[], []] and [n for n, _ in seen][1] == 'step_advance'
    assert len(opt.slots()) == {'adam': 3, 'rmsprop': 2, 'rmsprop-clip': 3}[kind]
    assert sorted(opt.state_dict()) == (['kind', 'm', 'state', 't', 'v'] if kind == 'adam' else ['kind', 'ms', 'state', 't'])
    del seen[:]
    sc = _scaler()
    on = _make(kind, g, sc, rate=0.125)
    on.set_lr(0.01)
    on.update([torch.randn(3, 5, generator=g), torch.randn(7, generator=g)], 0.5)
    assert [n for n, _ in seen][0] == 'grads_nonfinite' and [n for n, _ in seen][2] == 'step_advance' and len(seen) == 3
    assert seen[1][1] == ['avg', 'avg_rate', 'scaler'] and seen[2][1] == ['scaler', 'scaler_consts']
    assert on.slots()[-1] is sc.state and on.slots()[-2] is on.avg
    with pytest.raises(NotImplementedError):
        on.update_clipped([torch.randn(3, 5, generator=g), torch.randn(7, generator=g)], 1.0)


# ----------------------------------------------------------------------------- optimizers: good step, skip
@pytest.mark.parametrize('kind,rate', [('adam', 0.0), ('rmsprop-clip', 0.0), ('adam', 0.125), ('rmsprop', 0.125), ('rmsprop-clip', 0.125)])
def test_optimizer_good_step_equals_static_and_skip_changes_nothing(scale_kernels, kind, rate):
    sc = _scaler(init_scale=1024.0, growth_interval=10 ** 9)
    dyn = _make(kind, torch.Generator().manual_seed(7), sc, rate)
    sta = _make(kind, torch.Generator().manual_seed(7), None, rate)
    g = torch.Generator().manual_seed(8)
    for o in (dyn, sta):
        o.set_lr(0.01)
    for k in range(4):
        grads = [torch.randn(3, 5, generator=g) * 1024.0, None if k == 1 else torch.randn(7, generator=g) * 1024.0]
        if k == 2:
            grads[0][0, 3] = float('inf')          # under a FIXED scale the element is skipped and the rest applied ...
        for o in (dyn, sta):
            if k % 2:
                o.update(grads, 0.5 if o is dyn else 0.5 / 1024.0)
            else:
                o.gather_grads(grads)
                o.step(0.5 if o is dyn else 0.5 / 1024.0)
        if k < 2:
            for a, b in zip([dyn.theta] + dyn.slots()[:-1], [sta.theta] + sta.slots()):
                assert torch.equal(a, b), (kind, k)
        if k == 1:
            keep = [t.clone() for t in [dyn.theta] + dyn.slots()[:-1]]
    # ... under the dynamic one step 2 was dropped as a whole (the next test looks at every slot) and step 3 was applied at S / 2
    assert sc.scale() == 512.0 and sc.skipped_steps() == 1 and sc.good_steps() == 1 and dyn.skipped() == 0 and sta.skipped() == 1
    assert not torch.equal(dyn.theta, keep[0])


@pytest.mark.parametrize('kind', ['adam', 'rmsprop', 'rmsprop-clip'])
@pytest.mark.parametrize('packed', [False, True])
def test_one_inf_leaves_every_slot_untouched_to_the_bit(scale_kernels, kind, packed):
    sc = _scaler(init_scale=64.0)
    g = torch.Generator().manual_seed(11)
    opt = _make(kind, g, sc, rate=0.25)
    opt.set_lr(0.01)
    opt.update([torch.randn(3, 5, generator=g) * 64, torch.randn(7, generator=g) * 64])
    before = {k: v.clone() for k, v in (('theta', opt.theta), ('state', opt.state), ('avg', opt.avg))}
    before.update({k: getattr(opt, k).clone() for k in (('m', 'v') if kind == 'adam' else ('ms',))})
    grads = [torch.randn(3, 5, generator=g) * 64, torch.randn(7, generator=g) * 64]
    grads[1][6] = float('inf')
    if packed:
        opt.update(grads)
    else:
        opt.gather_grads(grads)
        opt.step()
    for k in before:
        if k != 'avg':
            assert torch.equal(getattr(opt, k), before[k]), k
    a = before['avg']
    assert torch.equal(opt.avg, a + torch.tensor(0.25) * (opt.theta - a)), 'the average still moves towards the weights as they are'
    assert torch.equal(opt.grad, torch.cat([x.reshape(-1) for x in grads])), 'the bucket still holds the step\'s gradients'
    assert sc.scale() == 32.0 and sc.skipped_steps() == 1 and sc.good_steps() == 0 and opt.skipped() == 0


def test_dropped_rmsprop_update_still_clips(scale_kernels):
    sc = _scaler(init_scale=4.0)
    g = torch.Generator().manual_seed(12)
    opt = _make('rmsprop-clip', g, sc)
    opt.set_lr(0.01)
    assert float(opt.theta.abs().max()) > 0.05
    ms = opt.ms.clone()
    opt.update([torch.full((3, 5), float('nan')), torch.zeros(7)])
    assert float(opt.theta.abs().max()) == float(torch.tensor(0.05)) and torch.equal(opt.ms, ms) and sc.skipped_steps() == 1


# ----------------------------------------------------------------------------- trainers
def _trainer(lib, name, **kw):
    from ctgan_amd.dcgan_step import DCGANTrainer
    case = H.Case(lib, name, 8, 4, 'cpu')
    return case, DCGANTrainer(case.M, seed=3, **kw)


@pytest.mark.parametrize('name,g_average', [('mnist', 0.0), ('mnist-dcgan', 0.0), ('mnist-wgan', 0.0), ('mnist-dcgan', 0.125), ('mnist-wgan', 0.125)])
def test_dynamic_trainer_held_at_1024_equals_static_trainer_at_1024(scale_kernels, name, g_average):
    """Adam (the CT objective and MODE 'dcgan') and RMSProp with the clip (MODE 'wgan'), with and without the generator's average."""
    import ctgan_amd.tflib as lib
    from ctgan_amd.optim import LossScaler
    ends = {}
    for which in ('dynamic', 'static', 'attribute'):
        ls = {'dynamic': LossScaler(init_scale=1024.0, growth_interval=10 ** 9, device='cpu'), 'static': 1024.0, 'attribute': None}[which]
        case, tr = _trainer(lib, name, g_average=g_average, loss_scale=ls)
        try:
            if which == 'attribute':
                assert tr.loss_scale == 1.0 and tr.scaler is None
                tr.loss_scale = 1024.0            # the way bench.py sets it
            assert tr.loss_scale == (1.0 if which == 'dynamic' else 1024.0)
            assert float(tr.cost_seed()) == 1024.0
            g = torch.Generator().manual_seed(4)
            feed = [torch.rand(4, 784, generator=g) for _ in range(3)]
            outs = [tr.train_iteration(it, lambda: feed[it]) for it in range(3)]
            ends[which] = [tr.d_opt.theta.clone(), tr.g_opt.theta.clone(), tr.rng.ctr.clone(), outs[-1]['cost'].clone(),
                           outs[-1]['grads'][tr.d_named[0][0]].clone()]
            n_slots = len(tr.d_opt.slots()) + len(tr.g_opt.slots())
            ends[which] += [s.clone() for s in tr.d_opt.slots() + tr.g_opt.slots() if tr.scaler is None or s is not tr.scaler.state]
            if which == 'dynamic':
                assert tr.d_opt.scaler is tr.g_opt.scaler is tr.scaler and tr.scaler.scale() == 1024.0 and tr.scaler.skipped_steps() == 0
                assert tr.scaler.good_steps() == 3 * tr.disc_iters + 2, 'one scaler counts the updates of both networks'
                assert tr.d_opt.slots()[-1] is tr.scaler.state and tr.g_opt.slots()[-1] is tr.scaler.state
                with pytest.raises(AttributeError):
                    tr.loss_scale = 2.0
            else:
                assert n_slots == len(ends[which]) - 5
        finally:
            case.close()
    for other in ('static', 'attribute'):
        assert len(ends['dynamic']) == len(ends[other])
        for a, b in zip(ends['dynamic'], ends[other]):
            assert torch.equal(a, b), (name, other)


def test_trainer_loss_scale_argument_is_validated(scale_kernels):
    import ctgan_amd.tflib as lib
    from ctgan_amd.dcgan_step import DCGANTrainer
    case = H.Case(lib, 'mnist', 8, 4, 'cpu')
    try:
        with pytest.raises(ValueError):
            DCGANTrainer(case.M, loss_scale='auto')
        tr = DCGANTrainer(case.M, loss_scale='dynamic')
        assert tr.scaler.scale() == 2.0 ** 16 and tr.loss_scale == 1.0 and float(tr.cost_seed()) == 2.0 ** 16
        assert tr.cost_seed().data_ptr() == tr.scaler.state.data_ptr()
        assert DCGANTrainer(case.M, loss_scale=8.0).loss_scale == 8.0 and DCGANTrainer(case.M).loss_scale == 1.0
        case.M.LOSS_SCALE = 4.0
        try:
            assert DCGANTrainer(case.M).loss_scale == 4.0 and DCGANTrainer(case.M, loss_scale=2.0).loss_scale == 2.0
        finally:
            del case.M.LOSS_SCALE
    finally:
        case.close()


def test_trainer_step_with_an_inf_is_dropped_and_the_next_one_applied(scale_kernels):
    import ctgan_amd.tflib as lib
    case, tr = _trainer(lib, 'mnist', loss_scale='dynamic')
    try:
        g = torch.Generator().manual_seed(4)
        good = torch.rand(4, 784, generator=g)
        bad = good.clone(); bad[1, 5] = float('inf')
        tr.train_iteration(0, lambda: good)
        snap = H.snapshot(lib, tr)
        n = tr.disc_iters
        tr.d_step(bad)
        now = H.snapshot(lib, tr)
        assert int(now.pop('rng.ctr')) == int(snap.pop('rng.ctr')) + 1 and int(now.pop('d_opt t')) == int(snap.pop('d_opt t')) + 1
        last = 'slot %d' % (len(tr.d_opt.slots()) - 1)          # the scaler's state: the tail of both slot lists
        for k in snap:
            if k not in ('rng site', 'd_opt ' + last, 'g_opt ' + last):          # (rng site: host bookkeeping of the draws within a step)
                assert torch.equal(now[k], snap[k]), k
        assert tr.scaler.scale() == 2.0 ** 15 and tr.scaler.skipped_steps() == 1 and tr.scaler.good_steps() == 0
        out = tr.d_step(good)
        assert tr.scaler.good_steps() == 1 and not torch.equal(tr.d_opt.theta, snap['d_opt theta']) and n >= 1
        # the reported gradients are unscaled by the scale they were taken at (2^15), not the one the end of the step left
        assert all(bool(torch.isfinite(v).all()) and float(v.abs().max()) < 1e3 for v in out['grads'].values() if v is not None)
    finally:
        case.close()


# ----------------------------------------------------------------------------- checkpoints
def test_checkpoint_round_trip_and_both_cross_loads(scale_kernels, tmp_path):
    import ctgan_amd.tflib as lib
    from ctgan_amd import checkpoint
    from ctgan_amd.optim import LossScaler
    path, path_static = str(tmp_path / 'dyn.pt'), str(tmp_path / 'static.pt')
    g = torch.Generator().manual_seed(4)
    feed = [torch.rand(4, 784, generator=g) for _ in range(4)]
    bad = feed[1].clone(); bad[0, 0] = float('nan')
    ends = {}
    for run in ('whole', 'resumed'):
        case, tr = _trainer(lib, 'mnist-dcgan', loss_scale=LossScaler(init_scale=256.0, growth_interval=3, device='cpu'))
        try:
            start = 0
            if run == 'resumed':
                start = checkpoint.load(path, tr)
                assert start == 2 and (tr.scaler.scale(), tr.scaler.good_steps(), tr.scaler.skipped_steps()) == saved
            for it in range(start, 4):
                tr.train_iteration(it, lambda: bad if it == 1 else feed[it])
                if run == 'whole' and it == 1:
                    checkpoint.save(path, tr, it + 1)
                    saved = (tr.scaler.scale(), tr.scaler.good_steps(), tr.scaler.skipped_steps())
                    assert saved[2] >= 1 and saved[0] != 256.0
            ends[run] = [tr.d_opt.theta.clone(), tr.g_opt.theta.clone(), tr.d_opt.m.clone(), tr.scaler.state.clone()]
        finally:
            case.close()
    for a, b in zip(ends['whole'], ends['resumed']):
        assert torch.equal(a, b)
    ck = torch.load(path, map_location='cpu', weights_only=False)
    assert sorted(ck['loss_scaler']) == ['state'] and ck['loss_scaler']['state'].shape == (4,)
    # a static run's checkpoint keys do not change; its file loads into a dynamic trainer at init_scale; the dynamic file into a static one
    case, tr = _trainer(lib, 'mnist-dcgan', loss_scale=1024.0)
    try:
        tr.train_iteration(0, lambda: feed[0])
        checkpoint.save(path_static, tr, 1)
        assert sorted(torch.load(path_static, map_location='cpu', weights_only=False)) == ['d_opt', 'extra', 'format', 'g_opt', 'iteration', 'params', 'rng']
        assert checkpoint.load(path, tr) == 2 and tr.scaler is None and tr.loss_scale == 1024.0
        assert torch.equal(tr.d_opt.m, torch.load(path, map_location='cpu', weights_only=False)['d_opt']['m'])
    finally:
        case.close()
    case, tr = _trainer(lib, 'mnist-dcgan', loss_scale=LossScaler(init_scale=256.0, growth_interval=3, device='cpu'))
    try:
        tr.scaler.state.copy_(torch.tensor([16.0, 1.0, 2.0, 5.0]))
        assert checkpoint.load(path_static, tr) == 1
        assert tr.scaler.state.tolist() == [256.0, 0.0, 0.0, 0.0]
    finally:
        case.close()


def test_scaler_state_dict_round_trip():
    from ctgan_amd.optim import LossScaler
    a = LossScaler(init_scale=64.0, device='cpu')
    a.state.copy_(torch.tensor([8.0, 1.0, 17.0, 3.0]))
    sd = a.state_dict()
    assert sd['state'].data_ptr() != a.state.data_ptr()
    b = LossScaler(device='cpu')
    b.load_state_dict(sd)
    assert b.state.tolist() == [8.0, 0.0, 17.0, 3.0] and (b.scale(), b.good_steps(), b.skipped_steps()) == (8.0, 17, 3)
    sd['state'][0] = 3.0
    with pytest.raises(ValueError):
        b.load_state_dict(sd)


# ----------------------------------------------------------------------------- the shared train loop
def test_train_loop_passes_the_scale_through_and_logs_it(scale_kernels, tmp_path, monkeypatch):
    import json
    import ctgan_amd.gan_mnist as M
    import ctgan_amd.tflib as lib
    from ctgan_amd import dcgan_step
    lib.delete_all_params(); lib.set_device('cpu')
    M.configure(DIM=8, BATCH_SIZE=4)
    try:
        g = torch.Generator().manual_seed(1)
        tr = dcgan_step.train(M, lambda: torch.rand(4, 784, generator=g), None, iters=2, out_dir=str(tmp_path), use_graphs=False,
                              sample_every=0, checkpoint_every=0, log=lambda *a: None, loss_scale='dynamic')
        assert tr.scaler is not None and tr.scaler.good_steps() + tr.scaler.skipped_steps() == 2 * tr.disc_iters + 1
        rows = [json.loads(line) for line in open(str(tmp_path / 'log.jsonl'))]
        names = set().union(*[set(r) for r in rows])
        assert 'loss_scale' in names and 'skipped_steps' in names
        lib.delete_all_params()
        out2 = tmp_path / 'static'; out2.mkdir()
        tr = dcgan_step.train(M, lambda: torch.rand(4, 784, generator=g), None, iters=2, out_dir=str(out2), use_graphs=False,
                              sample_every=0, checkpoint_every=0, log=lambda *a: None, loss_scale=8.0)
        assert tr.scaler is None and tr.loss_scale == 8.0
        names = set().union(*[set(json.loads(line)) for line in open(str(out2 / 'log.jsonl'))])
        assert 'loss_scale' not in names and 'skipped_steps' not in names
    finally:
        lib.delete_all_params(); M.configure()


# ----------------------------------------------------------------------------- two ranks
def _worker(rank, world, port, out_dir):
    sys.path.insert(0, ROOT)
    torch.set_num_threads(2)
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank), MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port))
    import ctgan_amd.kernels as K
    from tests import loss_scale_cpu_kernels as S
    from tests.test_ddp_gloo import _patch_cpu
    lib = _patch_cpu()
    S.install(K)
    import ctgan_amd.gan_mnist as M
    from ctgan_amd import ddp
    from ctgan_amd.dcgan_step import DCGANTrainer, build_params
    from ctgan_amd.engine import GraphedDCGANTrainer
    from ctgan_amd.optim import LossScaler
    ddp.init_from_env(backend='gloo')
    lib.set_seed(7 + rank)
    M.configure(DIM=8, BATCH_SIZE=4)
    build_params(M, 'cpu')
    tr = DCGANTrainer(M, seed=1, rank=rank, world_size=world, allreduce=ddp.FlatAllReduce(),
                      loss_scale=LossScaler(init_scale=64.0, growth_interval=4, device='cpu'))
    ddp.broadcast_params([tr.d_opt.theta, tr.g_opt.theta])
    eng = GraphedDCGANTrainer(tr, (4, 784), torch.float32, use_graphs=False)
    g = torch.Generator().manual_seed(500 + rank)          # per-rank shards: different local gradients
    k = [0]

    def nb():
        x = torch.rand(4, 784, generator=g)
        k[0] += 1
        if rank == 1 and k[0] == 2:
            x[2, 100] = float('inf')          # only rank 1's second critic step overflows locally
        return x
    theta0 = tr.d_opt.theta.clone()
    trace = []
    for it in range(2):
        eng.train_iteration(it, nb)
        trace.append(tr.scaler.state.clone())
    torch.save({'d': tr.d_opt.theta.clone(), 'g': tr.g_opt.theta.clone(), 'm': tr.d_opt.m.clone(), 'scaler': tr.scaler.state.clone(),
                'trace': trace, 'moved': not torch.equal(theta0, tr.d_opt.theta), 'n': tr.disc_iters},
               os.path.join(out_dir, 'scale_rank%d.pt' % rank))
    ddp.barrier()
    torch.distributed.destroy_process_group()
    M.configure()


def test_two_ranks_skip_together_and_stay_identical(tmp_path):
    """The scan runs on the bucket after the all-reduce: the inf of one rank's local gradient reaches both, both drop the update."""
    world = 2
    s = socket.socket(); s.bind(('127.0.0.1', 0)); port = s.getsockname()[1]; s.close()
    mp.spawn(_worker, args=(world, port, str(tmp_path)), nprocs=world, join=True)
    res = [torch.load(os.path.join(str(tmp_path), 'scale_rank%d.pt' % r)) for r in range(world)]
    for k in ('d', 'g', 'm', 'scaler'):
        assert torch.equal(res[0][k], res[1][k]), k
    n = res[0]['n']
    assert res[0]['moved'] and res[0]['scaler'][3].item() == 1.0, 'exactly one update was dropped, on both ranks'
    # 2 n + 1 updates, one dropped as the second: growth_interval 4 -> 64 / 2 = 32, then doubled after every 4 good ones
    good_after = 2 * n + 1 - 2
    assert res[0]['scaler'][0].item() == 32.0 * 2 ** (good_after // 4) and res[0]['scaler'][2].item() == good_after % 4
    assert bool(torch.isfinite(res[0]['d']).all()) and bool(torch.isfinite(res[0]['m']).all())
