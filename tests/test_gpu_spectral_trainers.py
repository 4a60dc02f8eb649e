"""Spectral normalisation in the GAN trainers on the MI355X (`-m gpu`; Trainer / DCGANTrainer `spectral_norm=`, optim.SpectralNorm): off is the
trainer without the argument (state, bits, launch count); on, the critic reads M / sigma, the flat bucket holds the gradient with respect to
the raw weights, the hand-scheduled step agrees with autograd, graph replay and a checkpoint resume reproduce the eager run bit for bit.
Shapes and batch sizes are those of the existing trainer tests.

Named to be collected after tests/test_gpu_kernels.py (see tests/test_gpu_trainers_capture.py)."""
import numpy as np
import pytest
import torch

from tests import spectral_oracle as O
from tests.test_gpu_resnet_step import _cmp, _rel_l2

pytestmark = pytest.mark.gpu


def _batches(B, n=4, seed=7):
    nrng = np.random.default_rng(seed)
    return [(torch.from_numpy(nrng.integers(0, 256, (B, 3072), dtype=np.int32)).cuda(),
             torch.from_numpy(nrng.integers(0, 10, (B,), dtype=np.int32)).cuda()) for _ in range(n)]


def _feed(batches):
    k = [0]

    def nxt():
        k[0] += 1
        return batches[k[0] % len(batches)]
    return nxt


@pytest.fixture
def resnet():
    import ctgan_amd.gan_cifar_resnet as R
    import ctgan_amd.tflib as lib

    def make(dim, B, seed=4, **kw):
        lib.delete_all_params(); lib.set_device(None); lib.set_seed(seed)
        R.configure(DIM_G=dim, DIM_D=dim, BATCH_SIZE=B, **kw)
        R.build_params()
        return R, lib
    yield make
    lib.delete_all_params(); R.configure()


def _shake_biases(lib, seed=5):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for n, p in lib._params.items():
            if n.endswith(('.Biases', '.b')):
                p.add_((0.1 * torch.randn(p.shape, generator=g)).to(p.device))


def _count_kernels(fn):
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    names = [e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]
    return len([n for n in names if 'memcpy' not in n.lower() and 'memset' not in n.lower()])


def test_off_is_the_trainer_without_the_argument(resnet):
    B, dim = 8, 16
    batches = _batches(B)
    res = []
    for kw in ({}, {'spectral_norm': False}):
        R, lib = resnet(dim, B)
        tr = R.Trainer(seed=9, **kw)
        nxt = _feed(batches)
        tr.train_iteration(0, nxt)
        n = _count_kernels(lambda: tr.train_iteration(1, nxt))
        res.append((tr.d_opt.theta.clone(), tr.g_opt.theta.clone(), len(tr.d_opt.slots()), sorted(tr.d_opt.state_dict()), n, tr.spectral,
                    len(lib._param_aliases)))
    a, b = res
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and a[2:] == b[2:]
    assert a[5] is None and a[6] == 0 and 'spectral' not in a[3] and a[4] > 0
    print('kernels of one eager iteration, off: %d' % a[4])


def _check_grad_identity(tr, lib, out, before, tol_note):
    """d_opt.grad = the fp64 formula applied to out['grads'], Mbar, u, v, sigma of before the update, within the bound of
    tests/spectral_oracle.py for the gradient transform alone: ddot = g(K N) sum(abs(Gbar) abs(Mbar)) (the inputs are exact here),
    dG = (ddot abs(v) abs(u)^T + 3 e abs(dot) abs(v) abs(u)^T + e abs(Gbar - dot v u^T)) / sigma + e abs(G), times 1.01."""
    sn = tr.spectral
    bar0, u0, v0, s0 = [t.cpu() for t in before]
    jobs = dict(zip(sn.names, zip(sn.table.jobs, sn.table.u_offs, sn.table.v_offs, range(len(sn.names)))))
    grad = tr.d_opt.grad.cpu() / float(getattr(tr, 'loss_scale', 1.0))          # (a power of two: exact; out['grads'] are unscaled)
    worst = 0.0
    for (n, p), o, sz in zip(tr.d_named, tr.d_opt.offsets, tr.d_opt.sizes):
        gb = out['grads'][n]
        got = grad[o:o + sz]
        if n not in jobs:
            assert torch.equal(got, gb.reshape(-1).cpu() if gb is not None else torch.zeros(sz)), n
            continue
        (_, k, nn), uo, vo, j = jobs[n]
        Gbar = gb.reshape(k, nn).cpu().numpy().astype(np.float64)
        Mbar = bar0[o:o + sz].view(k, nn).numpy().astype(np.float64)
        u, v, sg = u0[uo:uo + nn].numpy().astype(np.float64), v0[vo:vo + k].numpy().astype(np.float64), float(s0[j])
        want = O.grad(Gbar, Mbar, u, v, sg)
        dot = (Gbar * Mbar).sum()
        vu = np.outer(np.abs(v), np.abs(u))
        ddot = O.gamma(k * nn) * (np.abs(Gbar) * np.abs(Mbar)).sum()
        bound = O.SLACK * ((ddot * vu + 3 * O.E32 * abs(dot) * vu + O.E32 * np.abs(Gbar - dot * np.outer(v, u))) / sg + O.E32 * np.abs(want))
        ratio = float(np.max(np.abs(got.view(k, nn).numpy().astype(np.float64) - want) / np.maximum(bound, 1e-300)))
        worst = max(worst, ratio)
        assert ratio <= 1.0, (n, ratio)
    print('%s: d_opt.grad against fp64, largest error / bound %.4f' % (tol_note, worst))
    # afterwards lib.param(name) is M / sigma for normalised names and the raw value otherwise
    sig = sn.sigma.cpu()
    for (n, p), o, sz in zip(tr.d_named, tr.d_opt.offsets, tr.d_opt.sizes):
        assert lib._params[n] is p
        if n in jobs:
            back, raw = lib.param(n).detach().cpu() * sig[jobs[n][3]], p.detach().cpu()
            ulp = torch.nextafter(torch.abs(raw), torch.full_like(raw, float('inf'))) - torch.abs(raw)
            assert bool((torch.abs(back - raw) <= 2 * ulp).all()), n
        else:
            assert torch.equal(lib.param(n).detach(), p.detach()), n


@pytest.mark.parametrize('proj', [False, True])
def test_resnet_d_step_on(resnet, proj):
    B, dim = 8, 64                      # DIM 64: the width from which the hand-scheduled step applies
    kw = dict(PROJECTION=True, CONDITIONAL=True, ACGAN=False) if proj else {}
    R, lib = resnet(dim, B, **kw)
    _shake_biases(lib)
    tr = R.Trainer(seed=9, spectral_norm=True)
    sn = tr.spectral
    assert ('Discriminator.Projection.W' in sn.names) == proj
    real, labels = _batches(B, 1)[0]
    before = [t.clone() for t in (sn.theta_bar, sn.u, sn.v, sn.sigma)]
    theta0 = tr.d_opt.theta.clone()
    out = tr.d_step(real, labels, iteration=0)
    assert torch.isfinite(out['cost']).item() and not torch.equal(tr.d_opt.theta, theta0)
    _check_grad_identity(tr, lib, out, before, 'resnet%s' % (' + projection' if proj else ''))


def test_hand_scheduled_step_equals_autograd_with_spectral_norm(resnet):
    """The bound of tests/test_gpu_resnet_step.py::test_hand_scheduled_critic_step_equals_the_autograd_path_on_gpu (fp32 modes)."""
    import ctgan_amd.critic_schedule as CS
    import ctgan_amd.functional as F
    B, dim = 8, 64
    res = {}
    for merged in (False, True):
        R, lib = resnet(dim, B, seed=1)
        _shake_biases(lib)
        tr = R.Trainer(seed=3, spectral_norm=True)
        real, labels = _batches(B, 1, seed=5)[0]
        old, CS.MERGED_BWD = CS.MERGED_BWD, merged
        try:
            F.prepare_filters()
            fake = tr.generate_fakes(labels)[0]
            assert CS.usable(R, None, tr.rng, real, fake) == merged
            tr.rng.begin_step()
            out, grads = tr.d_grads(real, labels, fake=fake)
        finally:
            CS.MERGED_BWD = old
        res[merged] = (out, grads, [n for n, _ in tr.d_named])
    a, b = res[False], res[True]
    for k in ('cost', 'wgan', 'acgan', 'wgan_only', 'ct', 'gp', 'acc_real', 'acc_fake', 'd_real', 'd_fake', 'real'):
        assert (a[0].get(k) is None) == (b[0].get(k) is None), k
        if a[0].get(k) is not None:
            _cmp(b[0][k], a[0][k], 1e-5, 'scheduled.' + k, atol=1e-6)
    assert _rel_l2(b[0]['slopes'], a[0]['slopes']) < 1e-5 and _rel_l2(b[0]['gp_grads'], a[0]['gp_grads']) < 1e-5
    for n, x, y in zip(a[2], a[1], b[1]):
        assert (x is None) == (y is None), n
        if x is not None and x.abs().max() > 0:
            assert _rel_l2(y, x) < 2e-5, (n, _rel_l2(y, x))


@pytest.mark.parametrize('extras', [{}, {'g_average': 1e-3, 'augment': 'color,translation,cutout'}])
def test_graph_replay_equals_eager_bit_for_bit(resnet, extras):
    from ctgan_amd.engine import GraphedTrainer
    B, dim = 8, 16
    batches = _batches(B)
    res = []
    for graphs in (False, True):
        R, lib = resnet(dim, B)
        tr = R.Trainer(seed=9, spectral_norm=True, **extras)
        eng = GraphedTrainer(tr, use_graphs=graphs)
        assert bool(eng.graphed) == graphs, getattr(eng, 'graph_error', None)
        nxt = _feed(batches)
        costs = []
        for it in range(3):
            costs.append(eng.train_iteration(it, nxt)['cost'].clone())
        sn = tr.spectral
        res.append([tr.d_opt.theta.clone(), tr.g_opt.theta.clone(), sn.u.clone(), sn.v.clone(), sn.sigma.clone(), sn.theta_bar.clone()] + costs)
    for i, (x, y) in enumerate(zip(*res)):
        assert torch.equal(x, y), i


def test_checkpoint_resume_is_bit_exact(resnet, tmp_path):
    from ctgan_amd import checkpoint
    B, dim = 8, 16
    batches = _batches(B)
    R, lib = resnet(dim, B)
    tr = R.Trainer(seed=9, spectral_norm=True)
    nxt = _feed(batches)
    for it in range(2):
        tr.train_iteration(it, nxt)
    path = str(tmp_path / 'ck.pt')
    checkpoint.save(path, tr, 2)
    ck = torch.load(path, weights_only=False)
    assert all(torch.equal(ck['params'][n], p.detach().cpu()) for n, p in tr.d_named)                # raw weights
    for it in range(2, 4):
        tr.train_iteration(it, nxt)
    sn = tr.spectral
    want = [t.clone() for t in (tr.d_opt.theta, sn.theta_bar, sn.u, sn.sigma)]
    R, lib = resnet(dim, B, seed=11)
    tr2 = R.Trainer(seed=9, spectral_norm=True)
    assert checkpoint.load(path, tr2) == 2
    nxt = _feed(batches)
    for _ in range(2 * R.cfg.N_CRITIC):
        nxt()
    for it in range(2, 4):
        tr2.train_iteration(it, nxt)
    sn2 = tr2.spectral
    for i, (x, y) in enumerate(zip(want, (tr2.d_opt.theta, sn2.theta_bar, sn2.u, sn2.sigma))):
        assert torch.equal(x, y), i


@pytest.mark.parametrize('which', ['cifar', 'mnist'])
def test_dcgan_trainer_step_on(which):
    import ctgan_amd.tflib as lib
    from ctgan_amd.dcgan_step import DCGANTrainer
    if which == 'cifar':
        import ctgan_amd.gan_cifar as M
        kw = {}
    else:
        import ctgan_amd.gan_mnist as M
        kw = {'MODE': 'dcgan'}
    B = 8
    lib.delete_all_params(); lib.set_device(None); lib.set_seed(1)
    M.configure(DIM=32, BATCH_SIZE=B, **kw)
    try:
        d = lib._dev()
        with torch.no_grad():
            M.Discriminator(M.Generator(2, noise=torch.zeros(2, 128, device=d)), u=[torch.full((2,) + tuple(s), 0.9, device=d) for s in M.feat_shapes()])
        _shake_biases(lib)
        tr = DCGANTrainer(M, seed=3, spectral_norm=True)
        sn = tr.spectral
        g = torch.Generator().manual_seed(5)
        real = (torch.randint(0, 256, (B, 3072), dtype=torch.int32, generator=g) if which == 'cifar' else torch.rand(B, 784, generator=g)).to(d)
        before = [t.clone() for t in (sn.theta_bar, sn.u, sn.v, sn.sigma)]
        theta0 = tr.d_opt.theta.clone()
        out = tr.d_step(real)
        assert torch.isfinite(out['cost']).item() and not torch.equal(tr.d_opt.theta, theta0)
        _check_grad_identity(tr, lib, out, before, 'gan_' + which)
        if which == 'mnist':
            M.configure(DIM=32, BATCH_SIZE=B, MODE='wgan')
            with pytest.raises(ValueError):
                DCGANTrainer(M, seed=3, spectral_norm=True)
    finally:
        M.configure(); lib.delete_all_params()


def test_dynamic_loss_scale_with_spectral_norm_graph_equals_eager():
    """The `hold` word of a dropped update rides inside the captured step (optim.SpectralNorm.hold): two iterations of gan_mnist 'dcgan'
    under a dynamic loss scale, graph replay against eager, bit for bit."""
    import ctgan_amd.gan_mnist as M
    import ctgan_amd.tflib as lib
    from ctgan_amd.dcgan_step import DCGANTrainer
    from ctgan_amd.engine import GraphedDCGANTrainer
    B = 8
    g = torch.Generator().manual_seed(5)
    batches = [torch.rand(B, 784, generator=g).cuda() for _ in range(3)]
    res = []
    try:
        for graphs in (False, True):
            lib.delete_all_params(); lib.set_device(None); lib.set_seed(1)
            M.configure(DIM=32, BATCH_SIZE=B, MODE='dcgan')
            d = lib._dev()
            with torch.no_grad():
                M.Discriminator(M.Generator(2, noise=torch.zeros(2, 128, device=d)), u=[torch.full((2,) + tuple(s), 0.9, device=d) for s in M.feat_shapes()])
            tr = DCGANTrainer(M, seed=3, spectral_norm=True, loss_scale='dynamic')
            assert tr.spectral.hold is not None
            eng = GraphedDCGANTrainer(tr, tuple(batches[0].shape), batches[0].dtype, use_graphs=graphs)
            assert bool(eng.graphed) == graphs, getattr(eng, 'graph_error', None)
            nxt = _feed(batches)
            costs = [eng.train_iteration(it, nxt)['cost'].clone() for it in range(2)]
            sn = tr.spectral
            assert tr.scaler.skipped_steps() == 0 and float(sn.hold[0]) == 0.0
            res.append([tr.d_opt.theta.clone(), sn.u.clone(), sn.sigma.clone(), sn.theta_bar.clone()] + costs)
        for i, (x, y) in enumerate(zip(*res)):
            assert torch.equal(x, y), i
    finally:
        M.configure(); lib.delete_all_params()
