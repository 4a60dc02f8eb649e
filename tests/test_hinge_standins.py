"""The hinge objective's kernel checks (tests/hinge_cases.py) on the fp32 torch stand-ins (tests/hinge_cpu_kernels.py): the same case tables as
tests/test_gpu_hinge_kernels.py runs on the HIP kernels, so that what the host tests (tests/test_hinge_host.py) build on is itself held to the
fp64 references.  No GPU."""
import pytest

from tests import hinge_cases as C
from tests import loss_heads_cases as L
from tests import philox_spec as S
from tests.hinge_cpu_kernels import (avg_kernels, cond_cpu_kernels, hinge_cpu_kernels, mode_kernels, projection_cpu_kernels, scale_kernels,  # noqa: F401
                                     spectral_cpu_kernels)                                                                            # (fixtures)


@pytest.fixture
def be(hinge_cpu_kernels):  # noqa: F811
    import ctgan_amd.functional as F
    import ctgan_amd.kernels as K
    yield C.Backend(K, F, 'cpu')
    print(L.report())


@pytest.mark.parametrize('kind', C.GAN_LOSS_KINDS)
@pytest.mark.parametrize('B', C.GAN_LOSS_B)
@pytest.mark.parametrize('net', ['d', 'g'])
def test_gan_loss_hinge_kinds(be, net, B, kind):
    C.check_gan_loss_hinge(be, net, B, kind)


def test_gan_loss_kinds_0_to_3_are_delegated(be):
    L.check_gan_loss(be, 'bce', 'd', 3)
    L.check_gan_loss(be, 'ls', 'g', 3)


@pytest.mark.parametrize('B,H,W,nf,heads', C.TAIL_CASES)
def test_tail_hinge_heads(be, B, H, W, nf, heads):
    C.check_tail_hinge(be, B, H, W, nf, heads)


@pytest.mark.parametrize('B,heads,what', C.CRAFTED)
def test_tail_hinge_heads_crafted(be, B, heads, what):
    C.check_tail_hinge_crafted(be, B, heads, what)


def test_tail_hinge_heads_refusals(be):
    C.check_tail_hinge_refusals(be)


@pytest.mark.parametrize('B,d', C.PREP_CASES)
@pytest.mark.parametrize('corner', sorted(S.CORNERS))
def test_real_fake_prep(be, corner, B, d):
    C.check_real_fake_prep(be, corner, B, d)


def test_real_fake_prep_refusals(be):
    C.check_real_fake_prep_refusals(be)
