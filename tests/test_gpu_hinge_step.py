"""The hinge objective's steps on the MI355X (`-m gpu`): the checks of tests/hinge_step_checks.py (which tests/test_hinge_host.py runs on the CPU
stand-ins) on the HIP kernels.  Graph replay against eager and the launch count of a hinge critic step against a CT critic step are in
tests/test_gpu_trainers_hinge.py (a graph engine creates a capture stream: that file is collected after tests/test_gpu_kernels.py)."""
import pytest
import torch

from tests import hinge_step_checks as S

pytestmark = pytest.mark.gpu


@pytest.fixture
def modules():
    import ctgan_amd.gan_cifar_resnet as R
    import ctgan_amd.tflib as lib
    lib.delete_all_params(); lib.set_device(None)
    yield R, lib
    lib.delete_all_params(); R.configure()


@pytest.mark.parametrize('heads', sorted(S.HEADS))
def test_parity_with_fp64(modules, heads):
    R, lib = modules
    S.check_parity(R, lib, 'cuda', heads)


def test_parity_with_fp64_layernorm_critic(modules):
    R, lib = modules
    S.check_parity(R, lib, 'cuda', 'acgan', norm_d=True, dim=32, B=4)


@pytest.mark.parametrize('dim,B,heads', [(64, 8, 'acgan'), (64, 8, 'uncond'), (64, 8, 'proj'), (128, 64, 'acgan')])
def test_hand_schedule_equals_the_autograd_path(modules, dim, B, heads):
    R, lib = modules
    S.check_scheduled_equals_autograd(R, lib, 'cuda', dim, B, heads)


@pytest.mark.parametrize('kw', [dict(spectral_norm=True), dict(augment='color,translation,cutout')], ids=['spectral', 'augment'])
def test_hand_schedule_equals_the_autograd_path_with(modules, kw):
    R, lib = modules
    S.check_scheduled_equals_autograd(R, lib, 'cuda', 64, 8, 'acgan', **kw)


def test_real_is_the_ct_steps_real(modules):
    R, lib = modules
    S.check_real_is_the_ct_steps_real(R, lib, 'cuda')


def test_off_is_off(modules):
    R, lib = modules
    S.check_off_is_off_resnet(R, lib, 'cuda')
    import ctgan_amd.gan_mnist as M
    S.check_off_is_off_dcgan(M, lib, 'cuda')


@pytest.mark.parametrize('which', ['mnist', 'cifar'])
def test_dcgan_trainer_hinge_against_fp64(which):
    import ctgan_amd.tflib as lib
    S.check_dcgan_hinge(lib, which, 'cuda', dim=32, B=6)


def test_dcgan_trainer_refuses_other_modes_and_values():
    import ctgan_amd.tflib as lib
    S.check_dcgan_refusals(lib, 'cuda')


@pytest.mark.parametrize('heads', ['acgan', 'proj'])
def test_dev_cost_is_the_mean_hinge_cost(modules, heads):
    R, lib = modules
    S.check_dev_cost(R, lib, 'cuda', heads)
