"""The scripts' MODE switch ('wgan', 'dcgan', 'lsgan' beside the CT objective): mode table, validation, registry of the batch-normalised
MNIST nets, the fp64 oracle's TF RMSProp, and one critic + generator step of each new mode with the HIP wrappers swapped for CPU stand-ins
(the new wrappers' stand-ins are defined here) against tests/gan_modes_oracle.py.  No GPU."""
import pytest
import torch

from oracle import nets as onets, steps as osteps, tflib_ref as oref
from tests import gan_modes_oracle as O


# ----------------------------------------------------------------------------- CPU stand-ins of the new kernel wrappers
def _rmsprop_step(theta, g, ms, state, rho, eps, clip=0.0, grad_scale=1.0):
    lr = state[0].item()
    gi = g * grad_scale
    ok = torch.isfinite(gi)
    state[3] += float((~ok).sum().item())
    gi = torch.where(ok, gi, torch.zeros_like(gi))
    ms2 = ms + (gi * gi - ms) * (1 - rho)
    th2 = theta - (gi * lr) / torch.sqrt(ms2 + eps)
    ms.copy_(torch.where(ok, ms2, ms))
    theta.copy_(torch.where(ok, th2, theta))
    if clip > 0:
        theta.clamp_(-clip, clip)


def _rmsprop_step_packed(srcs, dst_offs, counts, flat, theta, ms, state, rho, eps, clip=0.0, grad_scale=1.0):
    for s, o, c in zip(srcs, dst_offs, counts):
        flat[o:o + c] = 0 if s is None else s.reshape(-1)
    _rmsprop_step(theta, flat, ms, state, rho, eps, clip, grad_scale)


def _gan_loss_terms(d, B, kind):
    import torch.nn.functional as TF
    if kind == 0:
        return (TF.binary_cross_entropy_with_logits(d[B:], torch.zeros(B)) + TF.binary_cross_entropy_with_logits(d[:B], torch.ones(B))) / 2
    if kind == 1:
        return TF.binary_cross_entropy_with_logits(d, torch.ones(B))
    if kind == 2:
        return (((d[:B] - 1) ** 2).mean() + (d[B:] ** 2).mean()) / 2
    return ((d - 1) ** 2).mean()


def _gan_loss_fwd(d, B, kind):
    return _gan_loss_terms(d.detach(), B, kind)


def _gan_loss_bwd(d, gout, B, kind):
    x = d.detach().clone().requires_grad_(True)
    with torch.enable_grad():
        (g,) = torch.autograd.grad(_gan_loss_terms(x, B, kind), x)
    return g * gout


@pytest.fixture
def mode_kernels(cpu_kernels, monkeypatch):
    import ctgan_amd.kernels as K
    for name, fn in (('rmsprop_step', _rmsprop_step), ('rmsprop_step_packed', _rmsprop_step_packed), ('gan_loss_fwd', _gan_loss_fwd),
                     ('gan_loss_bwd', _gan_loss_bwd)):
        monkeypatch.setattr(K, name, fn)
    return cpu_kernels


# ----------------------------------------------------------------------------- table, validation, registry
def test_mode_validation_and_defaults():
    import ctgan_amd.gan_64x64 as G64
    import ctgan_amd.gan_cifar as C
    import ctgan_amd.gan_mnist as M
    assert M.Config().MODE == 'wgan-CT' and G64.Config().MODE == 'wgan-ct' and C.Config().MODE == 'wgan-CT'
    assert M.Config().LR == 1e-4 and G64.Config().LR == 1e-4 and G64.ADAM_BETAS == (0.0, 0.9)
    with pytest.raises(NotImplementedError):
        M.Config(MODE='wgan-gp')
    with pytest.raises(NotImplementedError):
        G64.Config(MODE='wgan-gp')
    with pytest.raises(NotImplementedError):
        C.Config(MODE='wgan')
    with pytest.raises(NotImplementedError):
        M.Config(MODE='lsgan')            # the MNIST script has no least-squares branch
    for mod, m in ((M, 'wgan'), (M, 'dcgan'), (G64, 'wgan'), (G64, 'dcgan'), (G64, 'lsgan')):
        assert mod.Config(MODE=m).MODE == m
    assert M.cfg.MODE == 'wgan-CT' and C.cfg.MODE == 'wgan-CT' and G64.cfg.MODE == 'wgan-ct'


def test_mode_table_literals():
    import ctgan_amd.gan_64x64 as G64
    import ctgan_amd.gan_cifar as C
    import ctgan_amd.gan_mnist as M
    from ctgan_amd.dcgan_step import CT_MODE, GanMode
    assert M.MODES == {'wgan-CT': CT_MODE,
                       'wgan': GanMode('wgan', 'rmsprop', lr=5e-5, clip=0.01),
                       'dcgan': GanMode('bce', 'adam', lr=2e-4, betas=(0.5, 0.999), critic_iters=1)}
    assert G64.MODES == {'wgan-ct': CT_MODE,
                         'wgan': GanMode('wgan', 'rmsprop', lr=5e-5, clip=0.01),
                         'dcgan': GanMode('bce', 'adam', lr=2e-4, betas=(0.5, 0.999), critic_iters=1),
                         'lsgan': GanMode('ls', 'rmsprop', lr=1e-4, critic_iters=1)}
    assert C.MODES == {'wgan-CT': CT_MODE}
    assert CT_MODE == GanMode('ct', 'adam', None, None, None, None)


def test_mnist_wgan_registry(cpu_kernels):
    import ctgan_amd.gan_mnist as M
    import ctgan_amd.tflib as lib
    M.configure(MODE='wgan', DIM=8, BATCH_SIZE=4)
    try:
        with torch.no_grad():
            M.Discriminator(M.Generator(2, noise=torch.zeros(2, 128)), u=[torch.ones(2, *s) for s in M.feat_shapes()])
        shapes = {n: tuple(p.shape) for n, p in lib._params.items()}
        assert shapes['Generator.BN1.scale'] == (1, 4 * 4 * 4 * 8) and shapes['Generator.BN1.offset'] == (1, 4 * 4 * 4 * 8)
        assert 'Generator.BN1.moving_mean' not in shapes        # the axes-[0] branch keeps no moving statistics
        for n, c in (('Generator.BN2', 16), ('Generator.BN3', 8), ('Discriminator.BN2', 16), ('Discriminator.BN3', 32)):
            for k in ('offset', 'scale', 'moving_mean', 'moving_variance'):
                assert shapes[n + '.' + k] == (c,), (n, k)
            assert n + '.moving_mean' in lib._non_trainable and n + '.scale' not in lib._non_trainable
        assert not any('BN1' in n for n in shapes if n.startswith('Discriminator'))
        lib.delete_all_params()
        M.configure(DIM=8, BATCH_SIZE=4)          # default mode: no batch norm at all
        with torch.no_grad():
            M.Discriminator(M.Generator(2, noise=torch.zeros(2, 128)), u=[torch.ones(2, *s) for s in M.feat_shapes()])
        assert not any('BN' in n for n in lib._params)
    finally:
        M.configure(); lib.delete_all_params()


def test_oracle_rmsprop_first_step_uses_ones_initialised_slot():
    g = torch.tensor([1e-3, -0.5, 2.0, 0.0, 30.0], dtype=torch.float64)
    th0 = torch.tensor([0.1, -0.2, 0.3, 0.4, -0.5], dtype=torch.float64)
    th, ms = O.rmsprop_step(th0, g, torch.ones_like(g), 5e-5)
    assert torch.allclose(ms, 0.9 + 0.1 * g * g, rtol=1e-15, atol=0)
    assert torch.allclose(th, th0 - 5e-5 * g / torch.sqrt(0.9 + 0.1 * g * g + 1e-10), rtol=1e-15, atol=0)
    # ~ lr g for small gradients, not the zeros-initialised lr sign(g) sqrt(10)
    step = (th0 - th)[0].item()
    assert abs(step / (5e-5 * 1e-3 / 0.9 ** 0.5) - 1) < 1e-6 and step < 1e-3 * 5e-5 * 10 ** 0.5


def test_oracle_losses():
    x = torch.tensor([-80.0, -1.0, 0.0, 2.0, 80.0], dtype=torch.float64)
    assert torch.allclose(O.bce_with_logits(x, torch.ones_like(x)), torch.log1p(torch.exp(-x)))
    assert torch.isfinite(O.bce_with_logits(x, torch.zeros_like(x))).all()
    r, f = torch.tensor([0.5, 2.0], dtype=torch.float64), torch.tensor([-1.0, 1.0], dtype=torch.float64)
    assert abs(O.d_cost('ls', r, f).item() - ((0.25 + 1.0) / 2 + 1.0) / 2) < 1e-15
    assert abs(O.g_cost('ls', f).item() - (4.0 + 0.0) / 2) < 1e-15
    assert abs(O.d_cost('wgan', r, f).item() - (0.0 - 1.25)) < 1e-15


def test_optimizer_state_is_tagged_with_its_kind():
    from ctgan_amd.optim import FlatAdam, FlatRMSProp
    p = [('Discriminator.W', torch.nn.Parameter(torch.zeros(3)))]
    a, r = FlatAdam(p, 0.5, 0.9), FlatRMSProp([('Discriminator.V', torch.nn.Parameter(torch.zeros(3)))], clip=0.01)
    assert a.state_dict()['kind'] == 'adam' and r.state_dict()['kind'] == 'rmsprop'
    assert torch.equal(r.ms, torch.ones(3)) and r.slots()[0] is r.ms and r.slots()[-1] is r.theta
    assert [t is s for t, s in zip(a.slots(), (a.m, a.v, a.state))] == [True] * 3
    with pytest.raises(ValueError):
        r.load_state_dict(a.state_dict())
    with pytest.raises(ValueError):
        a.load_state_dict(r.state_dict())
    sd = a.state_dict(); del sd['kind']
    a.load_state_dict(sd)                     # (checkpoints from before the tag are Adam's)


def test_hand_scheduled_step_refuses_other_modes(cpu_kernels):
    import ctgan_amd.dcgan_schedule as DS
    import ctgan_amd.gan_mnist as M
    import ctgan_amd.tflib as lib
    from ctgan_amd.dcgan_step import DCGANTrainer
    M.configure(MODE='wgan', DIM=32, BATCH_SIZE=4)
    try:
        with torch.no_grad():
            M.Discriminator(M.Generator(2, noise=torch.zeros(2, 128)), u=[torch.ones(2, *s) for s in M.feat_shapes()])
        tr = DCGANTrainer(M, seed=1)
        assert tr.disc_iters == 5 and tr.lr() == 5e-5 and tr.d_opt.clip == 0.01 and tr.g_opt.clip == 0.0
        x = torch.zeros(4, 784)
        assert not DS.usable(tr, None, x, x)
    finally:
        M.configure(); lib.delete_all_params()


# ----------------------------------------------------------------------------- steps against the oracle
def oracle_from_product(lib, dtype=torch.float64):
    reg = oref.Registry(dtype=dtype)
    for n, p in lib._params.items():
        tr = n not in lib._non_trainable
        reg[n] = p.detach().cpu().clone().to(dtype).requires_grad_(tr)
        if not tr:
            reg.non_trainable.add(n)
    return reg


def mode_setup(which, mode, dim, B, g):
    """-> (module, G, D, real_in, real_o) with the module configured for `mode` (the caller builds the parameters)."""
    if which == 'mnist':
        import ctgan_amd.gan_mnist as M
        bn = mode == 'wgan'
        G = lambda reg, n, z: O.mnist_generator(reg, n, z, DIM=dim, bn=bn)            # noqa: E731
        D = lambda reg, x, u: O.mnist_discriminator(reg, x, u, DIM=dim, bn=bn)        # noqa: E731
        real_in = torch.rand(B, 784, generator=g)
        real_o = real_in.double()
    else:
        import ctgan_amd.gan_64x64 as M
        G = lambda reg, n, z: onets.good_generator(reg, n, z, dim=dim)                 # noqa: E731
        D = lambda reg, x, u: O.good_discriminator_bn(reg, x, u, dim=dim)             # noqa: E731
        real_in = torch.randint(0, 256, (B, 64 * 64 * 3), generator=g, dtype=torch.int32)
        real_o = 2 * ((real_in.double() / 255.) - .5)
    M.configure(MODE=mode, DIM=dim, BATCH_SIZE=B)
    return M, G, D, real_in, real_o


def build_params(M, dev):
    if hasattr(M, 'build_params'):
        M.build_params(dev)
    else:
        with torch.no_grad():
            M.Discriminator(M.Generator(2, noise=torch.zeros(2, 128, device=dev)), u=[torch.full((2,) + s, 0.9, device=dev) for s in M.feat_shapes()])


def oracle_opt(tr, reg, net):
    names = [n for n, _ in reg.trainable_with_name(net)]
    if tr.mode.optimizer == 'rmsprop':
        return lambda grads: O.TFRMSProp(reg, names, tr.mode.lr).apply(grads)
    b1, b2 = tr.mode.betas
    return lambda grads: osteps.TFAdam(reg, names, b1, b2).apply(grads, tr.mode.lr)


def _update_ok(new, old, ref_new, g_ref, g_prod, adam, tol=2e-2):
    """The applied update against the oracle's, in L2: within `tol` of the oracle's update plus the fp32 rounding of the weights themselves
    (an update below an ulp of its weight - the clipped critic's tiny generator gradients - is lost in any fp32 evaluation) and 1e-9 per
    element (the round-off update of a parameter whose exact gradient is zero: a bias in front of a batch norm).  Adam's first step is
    ~ lr sign(g): only elements whose gradient sign the product's fp32 gradient resolves (error below half the reference) are compared -
    the gradients themselves are checked separately."""
    d, dr, ulp = (new - old).reshape(-1), (ref_new - old).reshape(-1), ref_new.abs().reshape(-1) * 2.0 ** -23
    if adam:
        gr, gp = g_ref.reshape(-1), g_prod.detach().cpu().double().reshape(-1)
        keep = (gp - gr).abs() < 0.5 * gr.abs()
        d, dr, ulp = d[keep], dr[keep], ulp[keep]
    err = (d - dr).norm().item()
    return err <= tol * dr.norm().item() + ulp.norm().item() + 1e-9 * d.numel() ** 0.5, (err, dr.norm().item(), ulp.norm().item())


def run_mode_steps(lib, which, mode, dim, B, dev, seed=31, cost_tol=2e-4, grad_tol=3e-3, g_grad_tol=None, twin=None):
    """One critic step, then (from the oracle's updated weights) one generator step of the product on injected draws, against the fp64
    oracle: costs, per-parameter gradients (relative L2 against max(grad_tol - g_grad_tol for the generator -, 3 x the fp32 twin's error when
    `twin`) and every
    parameter after the update (the oracle's optimizer + clip on the oracle's own gradients).  Returns the number of parameters checked."""
    from ctgan_amd.dcgan_step import DCGANTrainer
    g = torch.Generator().manual_seed(seed)
    M, G, D, real_in, real_o = mode_setup(which, mode, dim, B, g)
    dv = (lambda o: [dv(t) for t in o] if isinstance(o, list) else o.float().to(dev))     # noqa: E731
    f32 = (lambda o: [f32(t) for t in o] if isinstance(o, list) else o.float())            # noqa: E731
    try:
        lib.set_seed(13)
        build_params(M, dev)
        tr = DCGANTrainer(M, seed=1)
        loss = tr.mode.loss
        adam = tr.mode.optimizer == 'adam'
        checked = 0
        for net in ('Discriminator', 'Generator'):
            reg = oracle_from_product(lib)
            before = {n: t.detach().clone() for n, t in reg.items()}
            if net == 'Discriminator':
                rnd = osteps.make_rnd_dcgan_d(B, M.feat_shapes(), g)
                out = tr.d_step(real_in.to(dev), {k: dv(v) for k, v in rnd.items()})
                cost_fn = lambda r, rd, t: O.d_losses(r, G, D, t, rd, loss)           # noqa: E731
                ref = cost_fn(reg, rnd, real_o)
            else:
                rnd = osteps.make_rnd_dcgan_g(B, M.feat_shapes(), g)
                out = tr.g_step({k: dv(v) for k, v in rnd.items()})
                cost_fn = lambda r, rd, t: O.g_losses(r, G, D, B, rd, loss)           # noqa: E731
                ref = cost_fn(reg, rnd, None)
            gref = osteps.grads_of(ref['cost'], reg, net)
            gtw = None
            if twin:
                reg32 = oref.Registry(dtype=torch.float32)
                for n, t in reg.items():
                    reg32[n] = t.detach().float().requires_grad_(t.requires_grad)
                reg32.non_trainable = set(reg.non_trainable)
                gtw = osteps.grads_of(cost_fn(reg32, {k: f32(v) for k, v in rnd.items()}, None if real_o is None else real_o.float())['cost'], reg32, net)
            a, b = out['cost'].item(), ref['cost'].item()
            assert abs(a - b) <= cost_tol * max(1.0, abs(b)), (net, 'cost', a, b)
            for n in gref:
                x, y = out['grads'][n].detach().cpu().double(), gref[n]
                fixed = grad_tol if net == 'Discriminator' or g_grad_tol is None else g_grad_tol
                tol = fixed if gtw is None else max(fixed, 3 * ((gtw[n].double() - y).norm() / y.norm().clamp_min(1e-30)).item())
                assert (x - y).norm().item() <= tol * y.norm().item() + 2e-6, (net, n, (x - y).norm().item(), y.norm().item())
            oracle_opt(tr, reg, net)(gref)
            if net == 'Discriminator' and tr.mode.clip:
                O.clip_critic(reg, tr.mode.clip)
            for n, t in reg.items():
                new = lib._params[n].detach().cpu().double()
                if not n.startswith(net):
                    assert torch.equal(new, before[n]), ('other network moved', n)
                    continue
                if n in reg.non_trainable:
                    assert torch.equal(new, t.detach().float().double()), ('moving statistic', n)
                    continue
                if n not in gref:
                    assert torch.equal(new, before[n]), ('no gradient, yet updated', n)
                    continue
                ok, how = _update_ok(new, before[n], t.detach(), gref[n], out['grads'][n], adam)
                assert ok, (net, 'update', n, how)
                checked += 1
            if net == 'Discriminator' and tr.mode.clip and which == 'mnist':
                mv = lib._params['Discriminator.BN2.moving_variance']
                assert torch.all(mv == 0.01) and float(lib._params['Discriminator.Output.W'].detach().abs().max()) <= 0.01
            lib.load_state_dict({n: t.detach().float() for n, t in reg.items()})      # continue from the oracle's weights
        return checked
    finally:
        M.configure(); lib.delete_all_params()


@pytest.mark.parametrize('which,mode', [('mnist', 'wgan'), ('mnist', 'dcgan'), ('64x64', 'wgan'), ('64x64', 'dcgan'), ('64x64', 'lsgan')])
def test_mode_steps_match_oracle_host_logic(mode_kernels, which, mode):
    import ctgan_amd.tflib as lib
    assert run_mode_steps(lib, which, mode, 8, 4, 'cpu', cost_tol=1e-5, grad_tol=1e-4, twin=True) > 0


@pytest.mark.parametrize('which,mode,n_crit', [('mnist', 'wgan', 5), ('mnist', 'dcgan', 1), ('64x64', 'lsgan', 1)])
def test_mode_training_iteration_host_logic(mode_kernels, which, mode, n_crit):
    """train_iteration runs disc_iters critic steps (one for 'dcgan' / 'lsgan') on the batched fake draw; the 'wgan' critic ends every
    iteration inside the clip bounds, its moving statistics included."""
    import ctgan_amd.tflib as lib
    from ctgan_amd.dcgan_step import DCGANTrainer
    g = torch.Generator().manual_seed(2)
    M, _, _, real_in, _ = mode_setup(which, mode, 8, 4, g)
    try:
        lib.set_seed(5)
        build_params(M, 'cpu')
        tr = DCGANTrainer(M, seed=3)
        assert tr.disc_iters == n_crit
        calls = []
        for it in range(2):
            out = tr.train_iteration(it, lambda: (calls.append(1), real_in)[1])
            assert torch.isfinite(out['cost']).item()
        assert len(calls) == 2 * n_crit and tr.d_opt.t == 2 * n_crit and tr.g_opt.t == 1
        assert int(tr.rng.ctr.item()) == 2 * (n_crit + 1) + 1
        if mode == 'wgan':
            for n, p in lib.named_params_with_name('Discriminator'):
                assert float(p.detach().abs().max()) <= 0.01, n
    finally:
        M.configure(); lib.delete_all_params()
