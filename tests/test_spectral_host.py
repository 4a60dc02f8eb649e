"""Host logic of spectral normalisation (optim.SpectralNorm, the trainers' `spectral_norm=`; NOT in the reference) on the CPU stand-ins of
tests/spectral_cpu_kernels.py: the name rule, the alias table, argument validation, slots() / state_dict() on and off, a dropped update
under a loss scale, the gradient identity of a critic step, the checkpoint round trip and a two-rank gloo run.  The kernels themselves are
checked on the GPU by tests/test_gpu_spectral.py.  No GPU."""
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from tests import spectral_oracle as O
from tests.spectral_cpu_kernels import (avg_kernels, cond_cpu_kernels, mode_kernels, projection_cpu_kernels, scale_kernels,  # noqa: F401
                                        spectral_cpu_kernels)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _module(net):
    if net == 'resnet':
        import ctgan_amd.gan_cifar_resnet as M
        M.configure(DIM_G=8, DIM_D=8, BATCH_SIZE=4)
    elif net == 'resnet_proj':
        import ctgan_amd.gan_cifar_resnet as M
        M.configure(DIM_G=8, DIM_D=8, BATCH_SIZE=4, PROJECTION=True, CONDITIONAL=True, ACGAN=False)
    elif net == 'cifar':
        import ctgan_amd.gan_cifar as M
        M.configure(DIM=8, BATCH_SIZE=2)
    elif net == 'mnist':
        import ctgan_amd.gan_mnist as M
        M.configure(DIM=8, BATCH_SIZE=2, MODE='dcgan')
    elif net == 'lsun128':
        import ctgan_amd.gan_lsun128 as M
        M.configure(BATCH_SIZE=2, DIM_G_64=4, DIM_G_32=4, DIM_G_16=4, DIM_G_8=8, DIM_G_4=8, DIM_D_64=4, DIM_D_32=4, DIM_D_16=8, DIM_D_8=8)
    else:
        import ctgan_amd.gan_64x64 as M
        M.configure(DIM=4, BATCH_SIZE=2)
    return M


def _build(M, lib, seed=5):
    lib.delete_all_params(); lib.set_device('cpu'); lib.set_seed(seed)
    if hasattr(M, 'build_params'):
        M.build_params('cpu')
    else:
        with torch.no_grad():
            M.Discriminator(M.Generator(2, noise=torch.zeros(2, 128)), u=[torch.full((2,) + tuple(s), 0.9) for s in M.feat_shapes()])


def _trainer(M, **kw):
    if M.__name__.endswith('gan_cifar_resnet'):
        return M.Trainer(seed=3, **kw)
    from ctgan_amd.dcgan_step import DCGANTrainer
    return DCGANTrainer(M, seed=3, **kw)


def _toy(lib, names_shapes, seed=1):
    lib.delete_all_params(); lib.set_device('cpu'); lib.set_seed(seed)
    g = torch.Generator().manual_seed(seed)
    return [(n, lib.param(n, torch.randn(s, generator=g) * 0.1)) for n, s in names_shapes]


TOY = [('Discriminator.1.Filters', (3, 3, 2, 5)), ('Discriminator.1.Biases', (5,)), ('Discriminator.Output.W', (5, 1)), ('Discriminator.Output.b', (1,)),
       ('Discriminator.Projection.W', (10, 5)), ('Discriminator.LN.scale', (5,))]


# ----------------------------------------------------------------------------------------------------------------- the name rule
@pytest.mark.parametrize('net', ['resnet', 'resnet_proj', 'cifar', 'mnist', 'lsun128', '64x64'])
def test_name_rule_per_module_and_width_limit(spectral_cpu_kernels, net):  # noqa: F811
    import ctgan_amd.kernels as K
    import ctgan_amd.tflib as lib
    from ctgan_amd.optim import spectral_normalised
    M = _module(net)
    try:
        _build(M, lib)
        named = lib.named_params_with_name('Discriminator', trainable_only=True)
        on = [n for n, _ in named if spectral_normalised(n)]
        off = [n for n, _ in named if not spectral_normalised(n)]
        assert on and all(n.rsplit('.', 1)[1] in ('Filters', 'W') for n in on)
        assert all(n.rsplit('.', 1)[1] in ('Biases', 'b', 'scale', 'offset', 'g') for n in off), off
        assert all(p.dim() >= 2 for n, p in named if n in on)
        assert ('Discriminator.Projection.W' in on) == (net == 'resnet_proj')
        assert not [n for n in lib._non_trainable if spectral_normalised(n)]
        tr = _trainer(M, spectral_norm=True)
        assert tr.spectral.names == on and [(k, n) for _, k, n in tr.spectral.table.jobs] == [(p.numel() // p.shape[-1], p.shape[-1]) for n_, p in named if n_ in on]
    finally:
        M.configure(); lib.delete_all_params()


@pytest.mark.parametrize('net', ['resnet', 'resnet_proj', 'cifar', 'mnist', 'lsun128', '64x64'])
def test_full_width_critics_fit_the_column_limit(spectral_cpu_kernels, net):  # noqa: F811
    """The widest last axis of any normalised critic weight at the module's DEFAULT widths, read off the registry the module itself builds
    (batch 2: the widths do not depend on it), and a job table over exactly those shapes: the fill refuses nothing."""
    import ctgan_amd.kernels as K
    import ctgan_amd.tflib as lib
    from ctgan_amd.optim import spectral_normalised
    M = _module(net)
    try:
        kw = dict(PROJECTION=True, CONDITIONAL=True, ACGAN=False) if net == 'resnet_proj' else {}
        M.configure(BATCH_SIZE=2, **kw)
        _build(M, lib)
        shapes = [tuple(p.shape) for n, p in lib.named_params_with_name('Discriminator', trainable_only=True) if spectral_normalised(n)]
        widest = max(s_[-1] for s_ in shapes)
        assert 64 <= widest <= K.SPECTRAL_MAX_N, (net, widest)
        jobs, off = [], 0
        for s_ in shapes:
            n = s_[-1]
            k = int(np.prod(s_)) // n
            jobs.append((off, k, n)); off += k * n + 1
        assert K.SpectralTable(jobs, off, torch.device('cpu')).njobs == len(shapes)
    finally:
        M.configure(); lib.delete_all_params()


# ----------------------------------------------------------------------------------------------------------------- state, aliases, validation
def test_state_init_aliases_and_views(spectral_cpu_kernels):  # noqa: F811
    import ctgan_amd.tflib as lib
    from ctgan_amd.optim import FlatAdam, SpectralNorm
    named = _toy(lib, TOY)
    opt = FlatAdam(named, 0.5, 0.9)
    raw = opt.theta.clone()
    sn = SpectralNorm(named, opt)
    assert opt.spectral is sn and sn.names == [TOY[0][0], TOY[2][0], TOY[4][0]]
    assert sn.table.jobs == [(0, 18, 5), (95, 5, 1), (101, 10, 5)]              # (the one-element Output.b sits in front of the table)
    assert torch.equal(opt.theta, raw)
    # u0 from the parameter's own '.u' stream, normalised; one iteration ran; theta_bar = M / sigma or a copy
    for (n, p), (o, k, nn), uo in zip([named[0], named[2], named[4]], sn.table.jobs, sn.table.u_offs):
        x = lib.rng_for(n + '.u').standard_normal(nn)
        u0 = (x / np.sqrt((x * x).sum())).astype(np.float32)
        assert np.array_equal(sn._u0[uo:uo + nn].numpy(), u0)
        r, b = O.normalise_bounds(p.detach().reshape(k, nn).numpy(), u0)
        assert np.all(np.abs(sn.theta_bar[o:o + k * nn].view(k, nn).numpy() - r['Mbar']) <= b['Mbar'])
        assert np.all(np.abs(sn.u[uo:uo + nn].numpy() - r['u']) <= b['u'])
    views = dict(sn.views())
    assert list(views) == opt.names and all(isinstance(v, torch.nn.Parameter) and v.is_leaf and v.requires_grad for v in views.values())
    assert all(v.data_ptr() == sn.theta_bar.data_ptr() + 4 * o and v.shape == p.shape for v, p, o in zip(views.values(), opt.params, opt.offsets))
    for n in ('Discriminator.1.Biases', 'Discriminator.Output.b', 'Discriminator.LN.scale'):
        assert torch.equal(views[n].detach(), lib._params[n].detach())
    assert sorted(sn.sigmas()) == sorted(sn.names) and all(s > 0 for s in sn.sigmas().values())
    # aliases: lib.param reads theta_bar, the registry and its state_dict keep the raw weights; group_of maps a view to its network
    assert not lib._param_aliases
    lib.alias_params(sn.aliases())
    try:
        for n, p in named:
            assert lib.param(n) is views[n] and lib._params[n] is p and lib.group_of(views[n]) == 'Discriminator'
        assert all(torch.equal(lib.state_dict()[n], p.detach()) for n, p in named)
    finally:
        lib.delete_param_aliases()
    assert lib.group_of(views[TOY[0][0]]) is None and lib.group_of(named[0][1]) == 'Discriminator'


def test_aliases_survive_the_classifiers_averaged_exit(spectral_cpu_kernels):  # noqa: F811
    """ct_common._averaged removes the aliases it installed, not the table."""
    import ctgan_amd.tflib as lib
    from ctgan_amd.ct_common import SSLTrainerBase as CTTrainer
    from ctgan_amd.optim import FlatAdam, FlatAdamTheano, SpectralNorm
    named = _toy(lib, TOY)
    sn = SpectralNorm(named, FlatAdam(named, 0.5, 0.9))
    others = [('Classifier.W', lib.param('Classifier.W', torch.ones(3, 2)))]
    lib.alias_params(sn.aliases())

    class T:
        d_opt = FlatAdamTheano(others, 0.5, 0.9, avg_rate=0.5)
    seen = CTTrainer._averaged(T(), lambda: (lib.param('Classifier.W') is not others[0][1], lib.param(TOY[0][0]) is dict(sn.views())[TOY[0][0]]), True)
    assert seen == (True, True)
    assert lib.param('Classifier.W') is others[0][1] and len(lib._param_aliases) == len(named)
    assert all(lib.param(n) is v for n, v in sn.views())
    lib.delete_param_aliases()
    CTTrainer._averaged(T(), lambda: None, True)
    assert not lib._param_aliases                      # nothing else aliased: the table is empty afterwards, as before


def test_argument_validation(spectral_cpu_kernels):  # noqa: F811
    import ctgan_amd.tflib as lib
    from ctgan_amd.optim import FlatAdam, FlatAdamTheano, FlatRMSProp, SpectralNorm
    named = _toy(lib, TOY)
    with pytest.raises(ValueError):
        SpectralNorm(named, FlatRMSProp(named, clip=0.01))
    with pytest.raises(NotImplementedError):
        SpectralNorm(named, FlatAdamTheano(named, 0.5, 0.9))
    opt = FlatAdam(named, 0.5, 0.9)
    with pytest.raises(ValueError):
        SpectralNorm(named[:3], opt)
    with pytest.raises(ValueError):
        SpectralNorm(named[1:2], FlatAdam(named[1:2], 0.5, 0.9))                # nothing to normalise
    sn = SpectralNorm(named, opt)
    with pytest.raises(ValueError):
        FlatAdam([(n, torch.nn.Parameter(p.detach().clone())) for n, p in named], 0.5, 0.9).attach_spectral(sn)    # built over another optimizer
    with pytest.raises(TypeError):
        FlatAdam(named, 0.5, 0.9, spectral=sn)                                  # no constructor argument: it could never be satisfied
    assert opt.params[0].data_ptr() == opt.theta.data_ptr()                     # (the refused calls left the parameters where they were)
    with pytest.raises(NotImplementedError):
        opt.update_clipped([None] * len(named), 1.0)
    assert SpectralNorm(named, FlatRMSProp(named)).opt.spectral is not None


def test_wgan_mode_refuses_spectral_norm(spectral_cpu_kernels):  # noqa: F811
    import ctgan_amd.gan_mnist as M
    import ctgan_amd.tflib as lib
    from ctgan_amd.dcgan_step import DCGANTrainer
    M.configure(DIM=8, BATCH_SIZE=2, MODE='wgan')
    try:
        _build(M, lib)
        with pytest.raises(ValueError):
            DCGANTrainer(M, seed=3, spectral_norm=True)
        assert DCGANTrainer(M, seed=3).spectral is None
    finally:
        M.configure(); lib.delete_all_params()


def test_slots_and_state_dict_on_and_off(spectral_cpu_kernels):  # noqa: F811
    import ctgan_amd.tflib as lib
    from ctgan_amd.optim import FlatAdam, FlatRMSProp, LossScaler, SpectralNorm
    for cls, args in ((FlatAdam, (0.5, 0.9)), (FlatRMSProp, ())):
        named = _toy(lib, TOY)
        sc = LossScaler(device='cpu')
        plain, off, on = cls(named, *args, scaler=sc), cls(named, *args, scaler=sc), cls(named, *args, scaler=sc)
        sn = SpectralNorm(named, on)
        assert len(off.slots()) == len(plain.slots()) and sorted(off.state_dict()) == sorted(plain.state_dict())
        extra = on.slots()[len(plain.slots()) - 1:-1]
        assert [t.data_ptr() for t in extra] == [t.data_ptr() for t in (sn.theta_bar, sn.u, sn.v, sn.sigma)] and on.slots()[-1] is sc.state
        assert sorted(on.state_dict()) == sorted(list(plain.state_dict()) + ['spectral'])
        assert sorted(on.state_dict()['spectral']) == ['sigma', 'u', 'v']


# ----------------------------------------------------------------------------------------------------------------- steps
def test_step_order_gradient_transform_and_one_iteration_per_update(spectral_cpu_kernels, monkeypatch):  # noqa: F811
    import ctgan_amd.kernels as K
    import ctgan_amd.tflib as lib
    from ctgan_amd.optim import FlatAdam, SpectralNorm
    named = _toy(lib, TOY)
    opt = FlatAdam(named, 0.5, 0.9)
    sn = SpectralNorm(named, opt)
    calls = []
    for name in ('spectral_grad', 'adam_step', 'adam_step_packed', 'step_advance', 'spectral_normalize'):
        monkeypatch.setattr(K, name, (lambda o, n: lambda *a, **k: (calls.append(n), o(*a, **k))[1])(getattr(K, name), name))
    g = torch.Generator().manual_seed(2)
    grads = [torch.randn(p.shape, generator=g) for _, p in named]
    bar0, u0, v0, s0, theta0 = sn.theta_bar.clone(), sn.u.clone(), sn.v.clone(), sn.sigma.clone(), opt.theta.clone()
    opt.set_lr(1e-3)
    opt.update(grads)
    assert calls == ['spectral_grad', 'adam_step', 'step_advance', 'spectral_normalize']
    # the bucket holds the fp64 formula applied to the gradients given, theta_bar, u, v, sigma of BEFORE the update
    for (o, k, n), uo, vo, j in zip(sn.table.jobs, sn.table.u_offs, sn.table.v_offs, range(3)):
        gb = dict(zip(opt.names, grads))[sn.names[j]].reshape(k, n).numpy()
        want = O.grad(gb, bar0[o:o + k * n].view(k, n).numpy(), u0[uo:uo + n].numpy(), v0[vo:vo + k].numpy(), float(s0[j]))
        assert np.allclose(opt.grad[o:o + k * n].view(k, n).numpy(), want, rtol=1e-5, atol=1e-6 * np.abs(want).max())
    gaps = torch.ones(opt.theta.numel(), dtype=torch.bool)
    for o, k, n in sn.table.jobs:
        gaps[o:o + k * n] = False
    assert torch.equal(opt.grad[gaps], torch.cat([g_.reshape(-1) for g_ in grads])[gaps])
    assert not torch.equal(opt.theta, theta0) and not torch.equal(sn.u, u0)
    assert torch.equal(sn.theta_bar[gaps], opt.theta[gaps])
    for j, (o, k, n) in enumerate(sn.table.jobs):
        assert torch.allclose(sn.theta_bar[o:o + k * n] * sn.sigma[j], opt.theta[o:o + k * n], rtol=3e-7, atol=0)


def test_dropped_update_under_a_loss_scale_keeps_the_weights(spectral_cpu_kernels):  # noqa: F811
    """A non-finite gradient: the scan sets the flag, the update is dropped and makes no new weight version - theta AND theta_bar keep
    their bits, straight after construction (one iteration from a random u: far from converged).  u may move; here it does not either,
    the iteration is skipped.  The next good update moves everything again."""
    import ctgan_amd.tflib as lib
    from ctgan_amd.optim import FlatAdam, LossScaler, SpectralNorm
    named = _toy(lib, TOY)
    sc = LossScaler(device='cpu')
    opt = FlatAdam(named, 0.5, 0.9, scaler=sc)
    sn = SpectralNorm(named, opt)
    theta0, bar0, u0, s0 = opt.theta.clone(), sn.theta_bar.clone(), sn.u.clone(), sn.sigma.clone()
    grads = [torch.ones(p.shape) for _, p in named]
    grads[0][0, 0, 0, 0] = float('inf')
    opt.set_lr(1e-3)
    opt.update(grads)
    assert sc.skipped_steps() == 1 and sc.scale() == 2.0 ** 15
    assert torch.equal(opt.theta, theta0) and torch.equal(sn.theta_bar, bar0)
    assert torch.equal(sn.sigma, s0) and bool(torch.isfinite(sn.u).all())
    grads[0][0, 0, 0, 0] = 1.0
    opt.update(grads)
    assert sc.skipped_steps() == 1 and not torch.equal(opt.theta, theta0) and not torch.equal(sn.theta_bar, bar0)
    assert not torch.equal(sn.u, u0) and not torch.equal(sn.sigma, s0)
    # a normalise of its own (construction, a load) never looks at the flag of an earlier step
    opt.update([torch.full(p.shape, float('nan')) for _, p in named])
    u1 = sn.u.clone()
    sn.normalise()
    assert not torch.equal(sn.u, u1)


def test_detach_gives_the_registry_back(spectral_cpu_kernels):  # noqa: F811
    import ctgan_amd.tflib as lib
    M = _module('resnet')
    try:
        _build(M, lib)
        tr = M.Trainer(seed=3, spectral_norm=True)
        assert len(lib._param_aliases) == len(tr.d_named) and tr.d_opt.spectral is tr.spectral
        tr.detach_spectral()
        assert not lib._param_aliases and tr.spectral is None and tr.d_opt.spectral is None
        assert all(a is b for a, (_, b) in zip(tr.d_params, tr.d_named)) and all(lib.param(n) is p for n, p in tr.d_named)
        plain = M.Trainer(seed=3)
        g = torch.Generator().manual_seed(1)
        out = plain.d_step(torch.randint(0, 256, (4, 3072), generator=g, dtype=torch.int32), torch.randint(0, 10, (4,), generator=g, dtype=torch.int32))
        assert torch.isfinite(out['cost']).item()
    finally:
        M.configure(); lib.delete_all_params()


@pytest.mark.parametrize('net', ['resnet', 'resnet_proj', 'cifar', 'mnist'])
def test_critic_step_reads_normalised_weights_and_transforms_the_gradient(spectral_cpu_kernels, net):  # noqa: F811
    import ctgan_amd.tflib as lib
    M = _module(net)
    try:
        _build(M, lib)
        tr = _trainer(M, spectral_norm=True)
        sn = tr.spectral
        assert len(lib._param_aliases) == len(tr.d_named) and tr.d_params == [v for _, v in sn.views()]
        B = M.cfg.BATCH_SIZE
        g = torch.Generator().manual_seed(1)
        bar0, u0, v0, s0, theta0 = sn.theta_bar.clone(), sn.u.clone(), sn.v.clone(), sn.sigma.clone(), tr.d_opt.theta.clone()
        if net.startswith('resnet'):
            out = tr.d_step(torch.randint(0, 256, (B, 3072), generator=g, dtype=torch.int32), torch.randint(0, 10, (B,), generator=g, dtype=torch.int32))
        elif net == 'mnist':
            out = tr.d_step(torch.rand(B, 784, generator=g))
        else:
            out = tr.d_step(torch.randint(0, 256, (B, 3072), generator=g, dtype=torch.int32))
        assert torch.isfinite(out['cost']).item() and not torch.equal(tr.d_opt.theta, theta0)
        # d_opt.grad = the fp64 formula applied to out['grads'] (with respect to the normalised weights) and the state of before the update
        jobs = dict(zip(sn.names, zip(sn.table.jobs, sn.table.u_offs, sn.table.v_offs, range(len(sn.names)))))
        for (n, p), o, sz in zip(tr.d_named, tr.d_opt.offsets, tr.d_opt.sizes):
            gb = out['grads'][n]
            got = tr.d_opt.grad[o:o + sz]
            if n not in jobs:
                assert torch.equal(got, gb.reshape(-1) if gb is not None else torch.zeros(sz))
                continue
            (_, k, nn), uo, vo, j = jobs[n]
            want = O.grad(gb.reshape(k, nn).numpy(), bar0[o:o + sz].view(k, nn).numpy(), u0[uo:uo + nn].numpy(), v0[vo:vo + k].numpy(), float(s0[j]))
            assert np.allclose(got.view(k, nn).numpy(), want, rtol=1e-4, atol=1e-5 * max(np.abs(want).max(), 1e-30)), n
        # afterwards lib.param(name) is M / sigma for normalised names and the raw value otherwise
        for (n, p), o, sz in zip(tr.d_named, tr.d_opt.offsets, tr.d_opt.sizes):
            assert lib._params[n] is p and p.data_ptr() == tr.d_opt.theta.data_ptr() + 4 * o
            if n in jobs:
                assert torch.allclose(lib.param(n).detach() * sn.sigma[jobs[n][3]], p.detach(), rtol=3e-7, atol=0), n
            else:
                assert torch.equal(lib.param(n).detach(), p.detach()), n
    finally:
        M.configure(); lib.delete_all_params()


def test_off_is_the_trainer_without_the_argument(spectral_cpu_kernels):  # noqa: F811
    import ctgan_amd.tflib as lib
    res = []
    for kw in ({}, {'spectral_norm': False}):
        M = _module('resnet')
        try:
            _build(M, lib)
            tr = M.Trainer(seed=3, **kw)
            g = torch.Generator().manual_seed(1)
            tr.d_step(torch.randint(0, 256, (4, 3072), generator=g, dtype=torch.int32), torch.randint(0, 10, (4,), generator=g, dtype=torch.int32))
            res.append((tr.d_opt.theta.clone(), len(tr.d_opt.slots()), sorted(tr.d_opt.state_dict()), tr.spectral, len(lib._param_aliases)))
        finally:
            M.configure(); lib.delete_all_params()
    assert torch.equal(res[0][0], res[1][0]) and res[0][1:] == res[1][1:] and res[0][3] is None and res[0][4] == 0
    assert 'spectral' not in res[0][2]


def test_checkpoint_round_trip_and_mixed_loads(spectral_cpu_kernels, tmp_path):  # noqa: F811
    import ctgan_amd.tflib as lib
    from ctgan_amd import checkpoint
    M = _module('resnet')
    g = torch.Generator().manual_seed(1)
    batches = [(torch.randint(0, 256, (4, 3072), generator=g, dtype=torch.int32), torch.randint(0, 10, (4,), generator=g, dtype=torch.int32))
               for _ in range(4)]

    def run(tr, which):
        for i in which:
            tr.d_step(*batches[i], iteration=i)
    try:
        _build(M, lib)
        tr = M.Trainer(seed=3, spectral_norm=True)
        run(tr, (0, 1))
        path = str(tmp_path / 'ck.pt')
        checkpoint.save(path, tr, 2)
        ck = torch.load(path, weights_only=False)
        assert sorted(ck['d_opt']['spectral']) == ['sigma', 'u', 'v'] and 'spectral' not in ck['g_opt']
        assert all(torch.equal(ck['params'][n], p.detach()) for n, p in tr.d_named)                   # raw weights under their old keys
        run(tr, (2, 3))
        want = [t.clone() for t in (tr.d_opt.theta, tr.spectral.theta_bar, tr.spectral.u, tr.spectral.sigma)]
        _build(M, lib, seed=9)                                                                    # another init: everything comes from the file
        tr2 = M.Trainer(seed=3, spectral_norm=True)
        assert checkpoint.load(path, tr2) == 2
        run(tr2, (2, 3))
        for a, b in zip(want, (tr2.d_opt.theta, tr2.spectral.theta_bar, tr2.spectral.u, tr2.spectral.sigma)):
            assert torch.equal(a, b)
        # a checkpoint with the entry loads into a plain trainer, which ignores it
        _build(M, lib, seed=9)
        tr3 = M.Trainer(seed=3)
        checkpoint.load(path, tr3)
        assert tr3.spectral is None and torch.equal(tr3.d_opt.theta, ck['d_opt']['m'] * 0 + torch.cat([ck['params'][n].reshape(-1) for n, _ in tr3.d_named]))
        # a checkpoint without the entry loads into a spectral trainer: the constructor's u, one iteration on the loaded weights
        plain = str(tmp_path / 'plain.pt')
        checkpoint.save(plain, tr3, 2)
        _build(M, lib, seed=9)
        tr4 = M.Trainer(seed=3, spectral_norm=True)
        u0 = tr4.spectral._u0.clone()
        checkpoint.load(plain, tr4)
        sn = tr4.spectral
        for j, ((o, k, n), uo) in enumerate(zip(sn.table.jobs, sn.table.u_offs)):
            r, b = O.normalise_bounds(tr4.d_opt.theta[o:o + k * n].view(k, n).numpy(), u0[uo:uo + n].numpy())
            assert abs(float(sn.sigma[j]) - r['sigma']) <= b['sigma']
    finally:
        M.configure(); lib.delete_all_params()


# ----------------------------------------------------------------------------------------------------------------- two ranks over gloo
def _worker(rank, world, port, out_dir, split=False):
    sys.path.insert(0, ROOT)
    torch.set_num_threads(2)
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank), MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port))
    import ctgan_amd.kernels as K
    import ctgan_amd.tflib as lib
    from tests import cpu_kernels as C, spectral_cpu_kernels as S
    for mod in (C, S):
        for name in mod.__all__:
            setattr(K, name, getattr(mod, name))
    lib.delete_all_params(); lib.set_device('cpu')
    import ctgan_amd.gan_cifar_resnet as R
    from ctgan_amd import ddp
    ddp.init_from_env(backend='gloo')
    lib.set_seed(7)                                   # one seed: the same weights and the same u on every rank, nothing to broadcast
    B = 2 if split else 4
    R.configure(DIM_G=8, DIM_D=64 if split else 8, BATCH_SIZE=B)        # DIM_D 64: the width from which the hand-scheduled step, which
    R.build_params('cpu')                                              # hands blocks 1-2 over early, applies
    seen = []
    orig = S.spectral_grad
    ar = ddp.FlatAllReduce()

    class Counted:
        def __call__(self, flat):
            seen.append('allreduce')
            return ar(flat)

        def wait(self):
            seen.append('wait')
            return ar.wait()
    K.spectral_grad = lambda *a, **k: (seen.append('spectral_grad'), orig(*a, **k))[1]
    tr = R.Trainer(seed=1, rank=rank, world_size=world, allreduce=Counted(), spectral_norm=True)
    tr.split_flush = split
    g = torch.Generator().manual_seed(100 + rank)
    costs = []
    for it in range(1 if split else 2):
        real, labels = torch.randint(0, 256, (B, 3072), generator=g, dtype=torch.int32), torch.randint(0, 10, (B,), generator=g, dtype=torch.int32)
        fake = None
        if split:
            import ctgan_amd.functional as F
            F.prepare_filters()
            fake = tr.generate_fakes(labels)[0]
        out = tr.d_step(real, labels, iteration=it, fake=fake)
        costs.append(out['cost'].detach().clone())
    torch.save({'theta': tr.d_opt.theta.clone(), 'u': tr.spectral.u.clone(), 'sigma': tr.spectral.sigma.clone(), 'bar': tr.spectral.theta_bar.clone(),
                'costs': costs, 'seen': seen}, os.path.join(out_dir, 'sn_rank%d.pt' % rank))
    ddp.barrier()
    torch.distributed.destroy_process_group()
    R.configure()


def test_two_ranks_over_gloo_stay_identical(tmp_path):
    s = socket.socket(); s.bind(('127.0.0.1', 0)); port = s.getsockname()[1]; s.close()
    mp.spawn(_worker, args=(2, port, str(tmp_path)), nprocs=2, join=True)
    a, b = [torch.load(os.path.join(str(tmp_path), 'sn_rank%d.pt' % r), weights_only=False) for r in range(2)]
    for k in ('theta', 'u', 'sigma', 'bar'):
        assert torch.equal(a[k], b[k]), k
    assert not torch.equal(a['costs'][0], b['costs'][0])                           # different shards
    assert a['seen'] == ['allreduce', 'wait', 'spectral_grad'] * 2                  # the transform runs on the bucket AFTER the all-reduce


def test_split_flush_transforms_after_both_parts_have_arrived(tmp_path):
    """Trainer.split_flush: the bucket goes to the all-reduce in two parts; the transform needs the whole reduced bucket (the dot is over
    a whole matrix), so it runs after the second part and the wait."""
    s = socket.socket(); s.bind(('127.0.0.1', 0)); port = s.getsockname()[1]; s.close()
    mp.spawn(_worker, args=(2, port, str(tmp_path), True), nprocs=2, join=True)
    a, b = [torch.load(os.path.join(str(tmp_path), 'sn_rank%d.pt' % r), weights_only=False) for r in range(2)]
    for k in ('theta', 'u', 'sigma', 'bar'):
        assert torch.equal(a[k], b[k]), k
    assert a['seen'] == ['allreduce', 'allreduce', 'wait', 'spectral_grad'] and b['seen'] == a['seen']
