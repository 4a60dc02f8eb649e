"""The derivative order of every autograd Function of ctgan_amd/functional.py on the MI355X: the table of tests/autograd_orders_cases.py
(one or more entries per Function class, each with a declared order, a builder through the public entry point, tiny inputs and an fp64
reference in plain torch ops) with the HIP kernels underneath.  A 'twice' entry is differentiated twice, alone and behind a MulFn, and every
first- and second-order cotangent is compared with fp64 - None where fp64 is not zero is the missing edge of a backward that calls a kernel
wrapper directly; a 'once' entry matches fp64 at first order and refuses a second differentiation.
tests/test_autograd_orders_standins.py runs the same table on the stand-ins made opaque; DESIGN.md section 30 lists the largest figures.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import autograd_orders_cases as C  # noqa: E402


@pytest.fixture(scope='module')
def be():
    import ctgan_amd.functional as F
    import ctgan_amd.kernels as K
    import ctgan_amd.tflib as lib
    lib.delete_all_params()
    yield C.Backend(K, F, 'cuda')
    lib.delete_all_params()


@pytest.fixture(scope='module', autouse=True)
def _report():
    C.MEASURED.clear()
    yield
    print('\nautograd orders on the HIP kernels, largest figures against fp64:\n' + C.report())


def test_kernel_results_carry_no_graph(be):
    """The premise of the table: a wrapper's result is a constant to autograd."""
    x = torch.randn(2, 4, 2, 2, device='cuda', requires_grad=True)
    assert be.K.tanh_fwd(x).grad_fn is None and not be.K.mul(x, x).requires_grad


@pytest.mark.parametrize('e', C.entries('twice'), ids=lambda e: e.id)
def test_twice(be, e):
    C.check_twice(be, e)


@pytest.mark.parametrize('e', [e for e in C.entries('twice') if e.chain], ids=lambda e: e.id)
def test_twice_behind_a_mul(be, e):
    """op(MulFn(x, w)): the form in which a cut is silent"""
    C.check_twice(be, e, chained=True)


@pytest.mark.parametrize('e', C.entries('once'), ids=lambda e: e.id)
def test_once(be, e):
    C.check_once(be, e)
