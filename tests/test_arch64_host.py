"""The 64x64 script's architecture selector (gan_64x64.Config.ARCH: DCGAN, no-BN, MLP, gated, tanh pairs of TF/CT_gan_64x64.py:41-72): the
selector's rules, registry names and closed-form parameter counts, the init widths, which wrappers a BatchNorm + activation layer launches
with the fusion switch on and off, the first-order-only guard, and one critic + generator step of every new ARCH against
tests/arch64_oracle.py - with the HIP wrappers swapped for CPU stand-ins (tests/arch64_cpu_kernels.py).  No GPU."""
import numpy as np
import pytest
import torch

from tests import arch64_oracle as AO
from tests import test_gan_modes_host as H
from tests.arch64_cpu_kernels import arch_cpu_kernels  # noqa: F401  (fixture)

NEW_ARCHS = ('dcgan', 'wganpaper', 'fc', 'dcgan-nobn', 'multiplicative', 'dcgan-tanh')
# one valid MODE per ARCH (the pairs of the GPU step test)
ARCH_MODE = {'dcgan': 'dcgan', 'wganpaper': 'wgan', 'fc': 'lsgan', 'dcgan-nobn': 'lsgan', 'multiplicative': 'wgan', 'dcgan-tanh': 'dcgan'}


def _build(arch, mode, dim, seed=13):
    import ctgan_amd.gan_64x64 as M
    import ctgan_amd.tflib as lib
    lib.delete_all_params()
    lib.set_seed(seed)
    M.configure(MODE=mode, ARCH=arch, DIM=dim, BATCH_SIZE=4)
    M.build_params('cpu')
    return M, lib


# ----------------------------------------------------------------------------- selector
def test_arch_selector_rules():
    import ctgan_amd.gan_64x64 as M
    assert M.Config().ARCH == 'good' and M.cfg.ARCH == 'good'
    for arch in NEW_ARCHS:
        for mode in ('wgan', 'dcgan', 'lsgan'):
            assert M.Config(ARCH=arch, MODE=mode).ARCH == arch
        with pytest.raises(NotImplementedError, match='wgan-ct'):
            M.Config(ARCH=arch)                              # default MODE 'wgan-ct'
    for mode in ('wgan-ct', 'wgan', 'dcgan', 'lsgan'):
        assert M.Config(ARCH='good', MODE=mode).ARCH == 'good'
    with pytest.raises(NotImplementedError, match='resnet101.*not built'):
        M.Config(ARCH='resnet101', MODE='wgan')
    with pytest.raises(NotImplementedError, match='not supported'):
        M.Config(ARCH='vgg', MODE='wgan')
    M.configure(ARCH='dcgan', MODE='lsgan')
    assert M.cfg.ARCH == 'dcgan' and M.feat_shapes() == [] and not M.critic_is_per_sample()
    M.configure()
    assert M.cfg.ARCH == 'good' and M.cfg.MODE == 'wgan-ct' and len(M.feat_shapes()) == 3 and M.critic_is_per_sample()


def test_every_arch_builds_and_returns_the_module_interface(arch_cpu_kernels):       # noqa: F811
    import ctgan_amd.tflib as lib
    try:
        for arch in NEW_ARCHS:
            M, _ = _build(arch, ARCH_MODE[arch], 8)
            with torch.no_grad():
                x = M.Generator(4, noise=torch.randn(4, 128), groups=2)
                d, f = M.Discriminator(x, groups=2)
            assert tuple(x.shape) == (4, 64 * 64 * 3) and tuple(d.shape) == (4,) and f is None
            assert float(x.abs().max()) <= 1.0
    finally:
        M.configure(); lib.delete_all_params()


# ----------------------------------------------------------------------------- registry names and closed-form counts
def _conv(name, k, cin, cout):
    return {name + '.Filters': k * k * cin * cout, name + '.Biases': cout}


def _lin(name, cin, cout):
    return {name + '.W': cin * cout, name + '.b': cout}


def _bnp(name, c):
    return {name + '.scale': c, name + '.offset': c}


def expected_params(arch, D, out_dim=64 * 64 * 3):
    """name -> element count of every TRAINABLE parameter, from the layer lists (k, Cin, Cout) of TF/CT_gan_64x64.py:223-295, :325-399, :435-467."""
    gated = arch == 'multiplicative'
    m = 2 if gated else 1
    g, d = {}, {}
    if arch == 'fc':
        for i, cin in ((1, 128), (2, 512), (3, 512), (4, 512)):
            g.update(_lin('Generator.%d.Linear' % i, cin, 512))
        g.update(_lin('Generator.Out', 512, out_dim))
    else:
        w = (1, 1, 1, 1) if arch == 'wganpaper' else (8, 4, 2, 1)
        g_bn = arch in ('dcgan', 'multiplicative', 'dcgan-tanh')
        g.update(_lin('Generator.Input', 128, 16 * w[0] * D * m))
        if g_bn:
            g.update(_bnp('Generator.BN1', w[0] * D * m))
        for i in (2, 3, 4):
            g.update(_conv('Generator.%d' % i, 5, w[i - 2] * D, w[i - 1] * D * m))
            if g_bn:
                g.update(_bnp('Generator.BN%d' % i, w[i - 1] * D * m))
        g.update(_conv('Generator.5', 5, w[3] * D, 3))
    d_bn = arch != 'dcgan-nobn'
    d.update(_conv('Discriminator.1', 5, 3, D * m))
    for i, (ci, co) in ((2, (1, 2)), (3, (2, 4)), (4, (4, 8))):
        d.update(_conv('Discriminator.%d' % i, 5, ci * D, co * D * m))
        if d_bn:
            d.update(_bnp('Discriminator.BN%d' % i, co * D * m))
    d.update(_lin('Discriminator.Output', 16 * 8 * D, 1))
    return g, d


def test_closed_form_counts_of_the_dcgan_pair():
    g, d = expected_params('dcgan', 64)
    assert sum(g.values()) == 5364739 and sum(d.values()) == 4316545


@pytest.mark.parametrize('arch', NEW_ARCHS)
def test_registry_names_and_parameter_counts_at_dim_64(arch_cpu_kernels, arch):       # noqa: F811
    M, lib = _build(arch, ARCH_MODE[arch], 64)
    try:
        g, d = expected_params(arch, 64)
        for net, want in (('Generator', g), ('Discriminator', d)):
            got = {n: p.numel() for n, p in lib.named_params_with_name(net, trainable_only=True)}
            assert got == want, (arch, net, sorted(set(got) ^ set(want)))
        stats = sorted(n for n in lib._params if n in lib._non_trainable)
        bns = sorted(n[:-len('.scale')] for n in list(g) + list(d) if n.endswith('.scale'))
        assert stats == sorted(b + k for b in bns for k in ('.moving_mean', '.moving_variance'))
        tr = __import__('ctgan_amd.dcgan_step', fromlist=['DCGANTrainer']).DCGANTrainer(M, seed=1)
        assert tr.d_opt.theta.numel() == sum(d.values()) and tr.g_opt.theta.numel() == sum(g.values())
    finally:
        M.configure(); lib.delete_all_params()


# ----------------------------------------------------------------------------- init widths
def _stdevs_unset():
    from ctgan_amd.tflib.ops import conv2d, deconv2d, linear
    return conv2d._weights_stdev is None and deconv2d._weights_stdev is None and linear._weights_stdev is None


def _weights(lib, net):
    return {n: p.detach() for n, p in lib.named_params_with_name(net, trainable_only=True) if n.endswith(('.Filters', '.W'))}


def test_init_widths(arch_cpu_kernels):       # noqa: F811
    import ctgan_amd.gan_64x64 as M
    import ctgan_amd.tflib as lib
    D, bound = 8, 0.02 * np.sqrt(3)
    try:
        for arch in ('dcgan', 'dcgan-nobn', 'dcgan-tanh'):
            _build(arch, ARCH_MODE[arch], D)
            assert _stdevs_unset()
            for net in ('Generator', 'Discriminator'):
                for n, w in _weights(lib, net).items():
                    # inside +-0.02 sqrt(3), and not a narrower draw: U(+-b) over >= 600 elements reaches 0.9 b
                    assert float(w.abs().max()) <= bound + 1e-9 and float(w.abs().max()) > 0.9 * bound, (arch, n)
        for arch in ('wganpaper', 'fc'):
            _build(arch, ARCH_MODE[arch], D)
            assert _stdevs_unset()
            for n, w in _weights(lib, 'Discriminator').items():
                assert float(w.abs().max()) <= bound + 1e-9 and float(w.abs().max()) > 0.9 * bound, (arch, n)
        # the generators outside the set_weights_stdev bracket keep the layers' own widths: stdev * sqrt(3) of He / Glorot
        _build('fc', 'lsgan', D)
        gw = _weights(lib, 'Generator')
        for n, fan_in in (('Generator.1.Linear.W', 128), ('Generator.2.Linear.W', 512), ('Generator.4.Linear.W', 512)):
            b = np.sqrt(2. / fan_in) * np.sqrt(3)                                   # initialization='he' (:79-81)
            assert 0.95 * b < float(gw[n].abs().max()) <= b + 1e-7, n
        b = np.sqrt(2. / (512 + 64 * 64 * 3)) * np.sqrt(3)                          # Glorot (initialization=None)
        assert 0.95 * b < float(gw['Generator.Out.W'].abs().max()) <= b + 1e-7
        _build('wganpaper', 'wgan', D)
        gw = _weights(lib, 'Generator')
        b = np.sqrt(2. / (128 + 16 * D)) * np.sqrt(3)
        assert 0.95 * b < float(gw['Generator.Input.W'].abs().max()) <= b + 1e-7 and b > 2 * bound
        b = np.sqrt(4. / (D * 25 / 4. + D * 25)) * np.sqrt(3)                       # Deconv2D he_init: fan_in = Cin k^2 / 4, fan_out = Cout k^2
        assert 0.95 * b < float(gw['Generator.3.Filters'].abs().max()) <= b + 1e-7 and b > 2 * bound
        _build('multiplicative', 'wgan', D)
        assert _stdevs_unset()
        assert float(_weights(lib, 'Discriminator')['Discriminator.2.Filters'].abs().max()) > 2 * bound
    finally:
        M.configure(); lib.delete_all_params()


def test_good_build_after_a_dcgan_build_is_bit_identical(arch_cpu_kernels):       # noqa: F811
    import ctgan_amd.gan_64x64 as M
    import ctgan_amd.tflib as lib
    try:
        _build('good', 'wgan-ct', 8, seed=21)
        first = {n: p.detach().clone() for n, p in lib._params.items()}
        _build('dcgan', 'dcgan', 8, seed=21)
        assert 'Generator.Res1.Conv1.Filters' not in lib._params and _stdevs_unset()
        _build('good', 'wgan-ct', 8, seed=21)
        assert list(lib._params) == list(first)
        for n, p in lib._params.items():
            assert torch.equal(p.detach(), first[n]), n
    finally:
        M.configure(); lib.delete_all_params()


def test_stdev_is_unset_even_when_a_build_fails(arch_cpu_kernels, monkeypatch):       # noqa: F811
    import ctgan_amd.functional as F
    import ctgan_amd.gan_64x64 as M
    import ctgan_amd.tflib as lib
    try:
        lib.delete_all_params()
        M.configure(ARCH='dcgan', MODE='dcgan', DIM=8, BATCH_SIZE=4)
        monkeypatch.setattr(F, 'conv2d_transpose', lambda *a, **k: (_ for _ in ()).throw(RuntimeError('boom')))
        with pytest.raises(RuntimeError, match='boom'):
            M.build_params('cpu')
        assert _stdevs_unset()
    finally:
        M.configure(); lib.delete_all_params()


# ----------------------------------------------------------------------------- which wrappers a layer launches
def _spy(monkeypatch, mod):
    """Record the name of every ctgan_amd.kernels wrapper (stand-in) a piece of code calls."""
    import ctgan_amd.kernels as K
    from tests import cpu_kernels as C
    calls = []
    for name in list(C.__all__) + list(mod.__all__):
        fn = getattr(K, name)
        monkeypatch.setattr(K, name, (lambda f, n: lambda *a, **k: (calls.append(n), f(*a, **k))[1])(fn, name))
    return calls


LAYOUT = {'empty_cl', 'workspace', 'to_channels_last', 'to_nchw', 'match_layout'}       # allocation / layout helpers, no arithmetic


@pytest.mark.parametrize('act', ['lrelu', 'tanh', 'gate'])
def test_layer_launches_fused_and_composed(arch_cpu_kernels, monkeypatch, act):       # noqa: F811
    import ctgan_amd.functional as F
    g = torch.Generator().manual_seed(3)
    x = arch_cpu_kernels.C._cl(torch.randn(4, 8, 5, 5, generator=g)).requires_grad_(True)
    scale = (1 + 0.1 * torch.randn(8, generator=g)).requires_grad_(True)
    offset = (0.1 * torch.randn(8, generator=g)).requires_grad_(True)
    for fused in (True, False):
        monkeypatch.setattr(F, 'BN_ACT_FUSED', fused)
        with monkeypatch.context() as mp:
            calls = _spy(mp, arch_cpu_kernels)
            y = F.batch_norm_act(x, scale, offset, act, 0.2, groups=2)
            gy = torch.randn(y.shape, generator=g)
            torch.autograd.grad(y, [x, scale, offset], gy)
        assert tuple(y.shape) == (4, 4 if act == 'gate' else 8, 5, 5)
        used = set(calls) - LAYOUT
        if fused:
            assert used == {'bn_act_fwd', 'bn_act_bwd'} and calls.count('bn_act_fwd') == 1 and calls.count('bn_act_bwd') == 1, calls
        else:
            assert not used & set(arch_cpu_kernels.__all__), calls
            want = {'lrelu': {'bn_fwd', 'bn_bwd', 'lrelu_fwd', 'lrelu_bwd'}, 'tanh': {'bn_fwd', 'bn_bwd', 'tanh_fwd', 'tanh_bwd'},
                    'gate': {'bn_fwd', 'bn_bwd', 'copy4d', 'sigmoid_fwd', 'sigmoid_bwd', 'tanh_fwd', 'tanh_bwd', 'mul'}}[act]
            assert used == want, calls
    # the same function either way
    monkeypatch.setattr(F, 'BN_ACT_FUSED', True)
    ya = F.batch_norm_act(x, scale, offset, act, 0.2, groups=2)
    monkeypatch.setattr(F, 'BN_ACT_FUSED', False)
    yb = F.batch_norm_act(x, scale, offset, act, 0.2, groups=2)
    gy = torch.randn(ya.shape, generator=g)
    for a, b in zip(torch.autograd.grad(ya, [x, scale, offset], gy), torch.autograd.grad(yb, [x, scale, offset], gy)):
        assert torch.allclose(a, b, rtol=1e-4, atol=1e-5)
    assert torch.allclose(ya, yb, rtol=1e-5, atol=1e-6)


def test_standalone_gate_launches(arch_cpu_kernels, monkeypatch):       # noqa: F811
    import ctgan_amd.functional as F
    g = torch.Generator().manual_seed(4)
    for shape in ((3, 6, 4, 4), (5, 10)):
        x = torch.randn(*shape, generator=g)
        x = (arch_cpu_kernels.C._cl(x) if x.dim() == 4 else x).requires_grad_(True)
        ref = torch.sigmoid(x[:, ::2].double()) * torch.tanh(x[:, 1::2].double())
        gy = torch.randn(ref.shape, generator=g)
        (gref,) = torch.autograd.grad(ref, x, gy.double())
        for fused in (True, False):
            monkeypatch.setattr(F, 'BN_ACT_FUSED', fused)
            with monkeypatch.context() as mp:
                calls = _spy(mp, arch_cpu_kernels)
                y = F.gate(x)
                (gx,) = torch.autograd.grad(y, x, gy)
            used = set(calls) - LAYOUT
            assert used == ({'gate_fwd', 'gate_bwd'} if fused else {'copy4d', 'sigmoid_fwd', 'sigmoid_bwd', 'tanh_fwd', 'tanh_bwd', 'mul'}), calls
            assert torch.allclose(y.double(), ref.detach(), atol=1e-6) and torch.allclose(gx.double(), gref.double(), atol=1e-6)


def test_fused_layers_are_first_order_only(arch_cpu_kernels, monkeypatch):       # noqa: F811
    import ctgan_amd.functional as F
    monkeypatch.setattr(F, 'BN_ACT_FUSED', True)
    x = arch_cpu_kernels.C._cl(torch.randn(4, 4, 3, 3)).requires_grad_(True)
    s, o = torch.ones(4, requires_grad=True), torch.zeros(4, requires_grad=True)
    for make in (lambda: F.batch_norm_act(x, s, o, 'tanh'), lambda: F.batch_norm_act(x, s, o, 'gate'), lambda: F.gate(x)):
        y = make()
        with pytest.raises(RuntimeError, match='first order only'):
            torch.autograd.grad(y.sum(), x, create_graph=True)
        (gx,) = torch.autograd.grad(make().sum(), x)                 # a plain backward still works
        assert torch.isfinite(gx).all()


def test_batchnorm_act_keyword_is_build_only_and_checked(arch_cpu_kernels):       # noqa: F811
    import ctgan_amd.tflib as lib
    from ctgan_amd.tflib.ops.batchnorm import Batchnorm
    x = arch_cpu_kernels.C._cl(torch.randn(4, 6, 3, 3))
    try:
        y = Batchnorm('T.BN', [0, 2, 3], x, act='gate', groups=2)
        assert tuple(y.shape) == (4, 3, 3, 3) and sorted(lib._params) == ['T.BN.moving_mean', 'T.BN.moving_variance', 'T.BN.offset', 'T.BN.scale']
        with pytest.raises(ValueError):
            Batchnorm('T.BN', [0, 2, 3], x, act='tanh', relu=True)
        with pytest.raises(ValueError):
            Batchnorm('T.BN', [0, 2, 3], x, act='tanh', is_training=True, stats_iter=0)
        with pytest.raises(ValueError):
            Batchnorm('T.BN', [0, 2, 3], x, act='swish')
    finally:
        lib.delete_all_params()


# ----------------------------------------------------------------------------- steps against the oracle
def test_hand_scheduled_step_keeps_refusing(arch_cpu_kernels):       # noqa: F811
    import ctgan_amd.dcgan_schedule as DS
    from ctgan_amd.dcgan_step import DCGANTrainer
    M, lib = _build('dcgan', 'wgan', 8)
    try:
        tr = DCGANTrainer(M, seed=1)
        x = torch.zeros(4, 64 * 64 * 3)
        assert not DS.usable(tr, None, x, x.to(torch.int32))
    finally:
        M.configure(); lib.delete_all_params()


@pytest.mark.parametrize('arch', NEW_ARCHS)
def test_arch_steps_match_oracle_host_logic(arch_cpu_kernels, monkeypatch, arch):       # noqa: F811
    """Costs, per-parameter gradients and post-update parameters of one critic and one generator step at DIM 8, B 4 - the bounds of
    test_mode_steps_match_oracle_host_logic (cost 1e-5, gradients 1e-4 or 3 x the fp32 twin's error)."""
    import ctgan_amd.tflib as lib
    monkeypatch.setattr(H, 'mode_setup', AO.setup)
    assert H.run_mode_steps(lib, arch, ARCH_MODE[arch], 8, 4, 'cpu', cost_tol=1e-5, grad_tol=1e-4, twin=True) > 0
