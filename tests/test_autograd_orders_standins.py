"""The derivative order of every autograd Function of ctgan_amd/functional.py (the table of tests/autograd_orders_cases.py) on the CPU
stand-ins made OPAQUE: the fixture below installs tests/cpu_kernels.py and every per-feature stand-in module, then re-patches each installed
stand-in so that it runs under torch.no_grad().  On the device a kernel wrapper writes into a fresh torch.empty through ctypes and its
result has no grad_fn; the stand-ins are differentiable torch expressions, on which a Function.backward that calls a K.* wrapper directly
passes a second-order check the device would fail.  With the wrapping the host suite sees the graph the device sees.  (Detaching the
results is not enough: copy4d(g, out) writes into its argument, which is how CropFn's backward would slip through.)

tests/test_gpu_autograd_orders.py runs the same table on the HIP kernels; DESIGN.md section 30 lists the largest figures of both.
"""
import pytest
import torch

from tests import autograd_orders_cases as C

STANDIN_MODULES = ('score_cpu_kernels', 'arch64_cpu_kernels', 'cond_layernorm_cpu_kernels', 'projection_cpu_kernels', 'diffaug_cpu_kernels')


def install_all(K, monkeypatch):
    """every per-feature stand-in on top of the `cpu_kernels` fixture"""
    import importlib
    from tests import ssl_cifar_te_oracle, test_gan_modes_host as H
    for m in STANDIN_MODULES:
        mod = importlib.import_module('tests.' + m)
        for name in mod.__all__:
            monkeypatch.setattr(K, name, getattr(mod, name))
    monkeypatch.setattr(K, 'gan_loss_fwd', H._gan_loss_fwd)
    monkeypatch.setattr(K, 'gan_loss_bwd', H._gan_loss_bwd)
    ssl_cifar_te_oracle.install_stand_ins(monkeypatch)           # (and those of ssl_oracle and ssl_cifar_oracle)


@pytest.fixture
def be(cpu_kernels, monkeypatch):
    import ctgan_amd.functional as F
    import ctgan_amd.kernels as K
    install_all(K, monkeypatch)
    wrapped = C.make_opaque(K, monkeypatch)
    assert {'copy4d', 'tanh_bwd', 'lrelu_bwd', 'bn_bwd', 'layernorm_bwd2', 'diffaug', 'wn_bwd', 'te_head_bwd'} <= set(wrapped)
    return C.Backend(K, F, 'cpu')


@pytest.fixture(scope='module', autouse=True)
def _report():
    C.MEASURED.clear()
    yield
    print('\nautograd orders on the opaque stand-ins, largest figures against fp64:\n' + C.report())


def test_the_table_names_every_function_class():
    """A new Function cannot land without declaring its order: the table names exactly the Function subclasses defined in functional.py."""
    import ctgan_amd.functional as F
    found, named = C.function_classes(F), C.declared()
    assert len(found) >= 70
    assert set(named) == found, (sorted(found - set(named)), sorted(set(named) - found))
    assert set(named.values()) == {'once', 'twice'}
    ids = [e.id for e in C.TABLE]
    assert len(ids) == len(set(ids))


def test_the_opaque_shim_cuts_the_graph(be):
    """What the shim is for: a stand-in's result carries no graph, and an in-place write through one leaves none on its target."""
    x = torch.randn(2, 4, 2, 2, requires_grad=True)
    assert be.K.tanh_fwd(x).grad_fn is None and not be.K.mul(x, x).requires_grad
    out = be.K.copy4d(x * 2.0, be.K.empty_cl(2, 4, 2, 2, device='cpu'))
    assert out.grad_fn is None and not out.requires_grad
    assert be.F.tanh(x).grad_fn is not None                       # (the Functions themselves still record)


def test_references_against_the_other_restatements():
    """The formulas restated here against the numpy ones of tests/elementwise_cases.py and against torch's own convolution adjoints."""
    import numpy as np
    from tests import elementwise_cases as E
    w = torch.randn(3, 3, 6, 8, dtype=torch.float64, generator=C.gen('ref'))
    for flip in (False, True):
        assert np.allclose(C.spread_ref(w, 0.25, flip).numpy(), E.np_spread(w.numpy(), 0.25, flip), rtol=0, atol=1e-15)
    x = torch.randn(2, 3, 6, 6, dtype=torch.float64, generator=C.gen('ref', 1))
    wf = torch.randn(3, 3, 3, 8, dtype=torch.float64, generator=C.gen('ref', 2))
    for stride in (1, 2):           # im2col followed by the 'cols' GEMM filter is the SAME conv
        cols = C.im2col_ref(x, 3, 3, stride, 32)
        y = torch.einsum('ncpq,ck->nkpq', cols[:, :27], wf.reshape(27, 8))
        assert torch.allclose(y, C.conv_ref(x, wf, None, stride), rtol=0, atol=1e-12)
    gy = torch.randn(2, 8, 3, 3, dtype=torch.float64, generator=C.gen('ref', 3))
    wt = torch.randn(3, 3, 8, 8, dtype=torch.float64, generator=C.gen('ref', 4))
    from oracle import tf_ops
    assert torch.allclose(C.dgrad_ref(gy, wt, (2, 8, 6, 6), 2), tf_ops.conv2d_transpose_same(gy, wt, 2), rtol=0, atol=1e-12)


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
