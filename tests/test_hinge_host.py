"""Host logic of the hinge objective (gan_cifar_resnet.Trainer / dcgan_step.DCGANTrainer / every GAN train() `objective='hinge'`; NOT in the
reference) on the CPU stand-ins (tests/hinge_cpu_kernels.py, themselves held to fp64 by tests/test_hinge_standins.py): parity with the fp64
restatement, the hand schedule (ctgan_amd/hinge_schedule.py) against the autograd path, the shared dequantisation site, off-is-off, the
DCGAN family, the dev cost and the argument's validation.  The checks live in tests/hinge_step_checks.py and run on the device from
tests/test_gpu_hinge_step.py.  No GPU."""
import inspect

import pytest
import torch

from tests import hinge_step_checks as S
from tests.hinge_cpu_kernels import (avg_kernels, cond_cpu_kernels, hinge_cpu_kernels, mode_kernels, projection_cpu_kernels, scale_kernels,  # noqa: F401
                                     spectral_cpu_kernels)                                                                            # (fixtures)


@pytest.fixture
def modules(hinge_cpu_kernels):  # noqa: F811
    import ctgan_amd.gan_cifar_resnet as R
    import ctgan_amd.tflib as lib
    yield R, lib
    R.configure()
    lib.delete_all_params()


def test_objective_argument_is_validated_and_documented(modules):
    R, lib = modules
    import ctgan_amd.dcgan_step as DS
    import ctgan_amd.gan_64x64, ctgan_amd.gan_cifar, ctgan_amd.gan_lsun128, ctgan_amd.gan_mnist  # noqa: E401, F401
    S.build(R, lib, 'cpu', 8, 4)
    assert R.Trainer(seed=1).objective is None and R.Trainer(seed=1, objective='hinge').objective == 'hinge'
    for bad in ('nope', 'ct', '', 0):
        with pytest.raises(ValueError):
            R.Trainer(seed=1, objective=bad)
    for fn in (R.Trainer.__init__, R.train, DS.DCGANTrainer.__init__, DS.train):
        assert inspect.signature(fn).parameters['objective'].default is None
        assert "objective" in (fn.__doc__ or '')
    # the scripts' train() hand their keywords to dcgan_step.train
    for m in (ctgan_amd.gan_cifar, ctgan_amd.gan_mnist, ctgan_amd.gan_64x64, ctgan_amd.gan_lsun128):
        assert any(p.kind is inspect.Parameter.VAR_KEYWORD for p in inspect.signature(m.train).parameters.values())
    import ctgan_amd.kernels as K
    assert K.GAN_LOSS_KINDS[('hinge', 'd')] == 4 and K.GAN_LOSS_KINDS[('hinge', 'g')] == 5
    assert all('hinge' not in str(v) for m in (ctgan_amd.gan_mnist, ctgan_amd.gan_64x64) for v in m.MODES.values())      # the MODES tables stay


@pytest.mark.parametrize('heads', sorted(S.HEADS))
def test_parity_with_fp64(modules, heads):
    R, lib = modules
    S.check_parity(R, lib, 'cpu', heads)


def test_parity_with_fp64_layernorm_critic(modules):
    R, lib = modules
    S.check_parity(R, lib, 'cpu', 'acgan', norm_d=True, dim=32, B=4)


@pytest.mark.parametrize('heads', sorted(S.HEADS))
def test_hand_schedule_equals_the_autograd_path(modules, heads):
    R, lib = modules
    S.check_scheduled_equals_autograd(R, lib, 'cpu', 64, 8, heads)


@pytest.mark.parametrize('kw', [dict(spectral_norm=True), dict(augment='color,translation,cutout')], ids=['spectral', 'augment'])
def test_hand_schedule_equals_the_autograd_path_with(modules, kw):
    R, lib = modules
    S.check_scheduled_equals_autograd(R, lib, 'cpu', 64, 8, 'acgan', **kw)


def test_fallbacks_take_the_autograd_path(modules):
    """usable() is false for injected draws, the Layernorm critic, a fusion switch off and widths outside the few-channel kernels"""
    import ctgan_amd.hinge_schedule as HS
    R, lib = modules
    real, labels = S.batch(4, 'cpu')
    for dim, kw, rnd, switch, want in ((64, {}, None, None, True), (64, {}, {'z': 1}, None, False), (64, dict(NORMALIZATION_D=True), None, None, False),
                                       (64, {}, None, 'HEAD_FUSION', False), (8, {}, None, None, False)):
        S.build(R, lib, 'cpu', dim, 4, dim_g=8, **kw)
        tr = R.Trainer(seed=1, objective='hinge')
        fake = tr.generate_fakes(labels)[0]
        if switch:
            setattr(R, switch, False)
        try:
            assert HS.usable(R, rnd, tr.rng, real, fake) == want, (dim, kw, rnd, switch)
        finally:
            if switch:
                setattr(R, switch, True)


def test_real_is_the_ct_steps_real(modules):
    R, lib = modules
    S.check_real_is_the_ct_steps_real(R, lib, 'cpu')


def test_off_is_off(modules):
    R, lib = modules
    S.check_off_is_off_resnet(R, lib, 'cpu')
    import ctgan_amd.gan_mnist as M
    S.check_off_is_off_dcgan(M, lib, 'cpu')


@pytest.mark.parametrize('which', ['mnist', 'cifar'])
def test_dcgan_trainer_hinge_against_fp64(modules, which):
    _, lib = modules
    S.check_dcgan_hinge(lib, which, 'cpu', dim=32, B=4)


def test_dcgan_trainer_refuses_other_modes_and_values(modules):
    _, lib = modules
    S.check_dcgan_refusals(lib, 'cpu')


@pytest.mark.parametrize('heads', ['acgan', 'proj'])
def test_dev_cost_is_the_mean_hinge_cost(modules, heads):
    R, lib = modules
    S.check_dev_cost(R, lib, 'cpu', heads)


def test_train_iteration_and_the_out_keys(modules):
    R, lib = modules
    S.build(R, lib, 'cpu', 8, 4)
    tr = R.Trainer(seed=2, objective='hinge')
    batches = [S.batch(4, 'cpu', seed=s) for s in (1, 2, 3)]
    nxt = S._feed(batches)
    th0 = tr.d_opt.theta.clone()
    for it in range(2):
        out = tr.train_iteration(it, nxt)
    assert set(out) == {'cost', 'wgan', 'hinge_real', 'hinge_fake', 'acgan', 'acc_real', 'acc_fake', 'fake', 'real', 'd_real', 'd_fake', 'grads'}
    assert torch.isfinite(out['cost']).item() and not torch.equal(tr.d_opt.theta, th0)
    assert abs(out['cost'].item() - (out['wgan'].item() + R.cfg.ACGAN_SCALE * out['acgan'].item())) < 1e-5
    assert abs(out['wgan'].item() - (out['hinge_real'].item() + out['hinge_fake'].item())) < 1e-5
