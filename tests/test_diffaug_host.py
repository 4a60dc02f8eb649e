"""Differentiable augmentation (csrc/diffaug.hip, kernels.diffaug, functional.diffaug, the trainers' `augment`) - the host logic on the CPU
stand-ins of tests/diffaug_cpu_kernels.py, and the argument checks of the C entry point (validation precedes any launch)."""
import ctypes

import numpy as np
import pytest
import torch

from tests import diffaug_oracle as O
from tests.diffaug_cpu_kernels import CALLS, diffaug_kernels        # noqa: F401  (fixture)
from tests.test_gan_modes_host import build_params, mode_kernels, mode_setup        # noqa: F401  (fixture)
from tests.test_host_logic_resnet import _cmp

POLICY = 'color,translation,cutout'
MNIST = (1, 28, 28)


# ----------------------------------------------------------------------------- policy strings, reserved stream ids
def test_policy_parsing():
    import ctgan_amd.kernels as K
    assert K.diffaug_policy(POLICY) == 7
    assert K.diffaug_policy('color') == 1 and K.diffaug_policy('translation') == 2 and K.diffaug_policy('cutout') == 4
    assert K.diffaug_policy('cutout, color') == 5 and K.diffaug_policy('translation,cutout') == 6
    assert K.diffaug_policy(None) == 0 and K.diffaug_policy('') == 0
    with pytest.raises(ValueError, match='flip'):
        K.diffaug_policy('color,flip')
    assert K.DIFFAUG_NO_BRIGHTNESS & 7 == 0


def test_reserved_stream_ids_are_never_handed_out(cpu_kernels):
    from ctgan_amd import rng as R
    assert (R.AUG_REAL, R.AUG_FAKE, R.AUG_GEN) == (0xFF00, 0xFF01, 0xFF02)
    r = R.DeviceRNG(seed=1, rank=3, device='cpu')
    seen = set()
    for _ in range(0xFF00):
        seen.add(r._sid() & 0xFFFF)
    assert max(seen) == 0xFEFF and not seen & {R.AUG_REAL, R.AUG_FAKE, R.AUG_GEN}
    with pytest.raises(RuntimeError, match='too many random call sites'):
        r._sid()
    seed, sid, ctr = r.aug_spec(R.AUG_FAKE)
    assert seed == 1 and sid == (3 << 16) | 0xFF01 and ctr is r.ctr


# ----------------------------------------------------------------------------- the oracle itself
def test_oracle_adjoint_is_the_transpose_and_the_forward_is_affine():
    """<T'(x), g> = <x, T'^T g> for the linear part T' (forward without brightness), and T(x) - T'(x) does not depend on x."""
    shape = (3, 8, 12)
    n, d = 6, 3 * 8 * 12
    g = torch.Generator().manual_seed(0)
    x, x2, gy = (torch.randn(n, d, generator=g, dtype=torch.float64) for _ in range(3))
    for policy in range(8):
        p = O.params(11, 5, 2, n, 8, 12, policy)
        lin = O.forward(x, shape, p, brightness=False)
        assert abs((lin * gy).sum().item() - (x * O.adjoint(gy, shape, p)).sum().item()) < 1e-9
        off = O.forward(x, shape, p) - lin
        assert torch.allclose(off, O.forward(x2, shape, p) - O.forward(x2, shape, p, brightness=False), atol=1e-12)
        if not policy & 1:
            assert off.abs().max().item() == 0.0
    p0 = O.params(11, 5, 2, n, 8, 12, 0)
    assert torch.equal(O.forward(x, shape, p0), x) and torch.equal(O.adjoint(x, shape, p0), x)


def test_oracle_integer_draws_stay_in_range():
    for h, w in ((4, 4), (8, 12), (28, 28), (32, 32), (128, 128)):
        sh, sw, kh, kw, nh, nw = O.geometry(h, w)
        u = np.zeros((3, 8), np.float32)
        u[1] = 1.0 - 2.0 ** -24          # the largest u01
        u[2] = 0.5
        p = O.params(0, 0, 0, 3, h, w, 7, u=u)
        assert p['ty'].min() == -sh and p['ty'].max() == sh and p['tx'].min() == -sw and p['tx'].max() == sw
        assert (p['y0'] >= 0).all() and (p['y1'] <= h).all() and (p['y0'] < p['y1']).all()
        assert (p['x0'] >= 0).all() and (p['x1'] <= w).all() and (p['x0'] < p['x1']).all()
    assert O.geometry(28, 28) == (4, 4, 14, 14, 29, 29) and O.geometry(4, 4) == (1, 1, 2, 2, 5, 5) and O.geometry(32, 32)[:4] == (4, 4, 16, 16)


# ----------------------------------------------------------------------------- autograd through T
def test_autograd_through_diffaug_is_the_adjoint_and_its_own_backward_the_linear_forward(diffaug_kernels):
    import ctgan_amd.functional as F
    import ctgan_amd.kernels as K
    shape, n = (3, 8, 12), 4
    g = torch.Generator().manual_seed(3)
    x = torch.randn(n, 3 * 8 * 12, generator=g).requires_grad_(True)
    gy = torch.randn(n, 3 * 8 * 12, generator=g).requires_grad_(True)
    spec = (9, (2 << 16) | 0xFF02, torch.tensor([4], dtype=torch.int64))
    y = F.diffaug(x, shape, 7, spec)
    assert torch.equal(y, K.diffaug(x.detach(), shape, 7, spec))
    (gx,) = torch.autograd.grad(y, x, grad_outputs=gy, create_graph=True)
    assert torch.equal(gx, K.diffaug(gy.detach(), shape, 7, spec, adjoint=True))
    # second order: d <gx, v> / d gy = T'(v), the forward with the brightness off
    v = torch.randn(n, 3 * 8 * 12, generator=g)
    (ggy,) = torch.autograd.grad(gx, gy, grad_outputs=v, create_graph=True)
    assert torch.equal(ggy, K.diffaug(v, shape, 7 | K.DIFFAUG_NO_BRIGHTNESS, spec))
    assert not torch.equal(ggy, K.diffaug(v, shape, 7, spec))
    # third order closes the pair again: the adjoint
    w_ = torch.randn(n, 3 * 8 * 12, generator=g)
    v.requires_grad_(True)
    lin = F.DiffAugFn.apply(v, shape, 7 | K.DIFFAUG_NO_BRIGHTNESS, spec)
    (gv,) = torch.autograd.grad(lin, v, grad_outputs=w_)
    assert torch.equal(gv, K.diffaug(w_, shape, 7, spec, adjoint=True))
    assert F.diffaug(x, shape, 0, spec) is x


# ----------------------------------------------------------------------------- trainers
def _mnist_trainer(mode, augment, B=4, dim=8, with_keyword=True, seed=3, which='mnist'):
    import ctgan_amd.tflib as lib
    from ctgan_amd.dcgan_step import DCGANTrainer
    g = torch.Generator().manual_seed(2)
    M, _, _, real_in, _ = mode_setup(which, mode, dim, B, g)
    lib.set_seed(5)
    build_params(M, 'cpu')
    with torch.no_grad():
        for n, p in lib._params.items():
            if n.endswith(('.Biases', '.b')):
                p.add_(0.1 * torch.randn(p.shape, generator=g))
    tr = DCGANTrainer(M, seed=seed, augment=augment) if with_keyword else DCGANTrainer(M, seed=seed)
    return M, lib, tr, real_in


def _same(a, b, what):
    assert (a is None) == (b is None), what
    if a is not None:
        assert torch.equal(a.detach(), b.detach()), what


@pytest.mark.parametrize('which,mode', [('mnist', 'wgan-CT'), ('mnist', 'wgan'), ('mnist', 'dcgan'), ('64x64', 'lsgan')])
def test_augment_none_is_a_trainer_without_the_keyword(diffaug_kernels, which, mode):
    """Every mode of gan_mnist, and the fourth objective ('lsgan') on the script that has it."""
    res = []
    for kw in (False, True):
        M, lib, tr, real_in = _mnist_trainer(mode, None, with_keyword=kw, which=which)
        try:
            assert tr.aug_policy == 0
            fake = tr.generate_fakes(1)[0]
            tr.rng.begin_step()
            out, grads = tr.d_grads(real_in, fake=fake)
            tr.rng.begin_step()
            gout = tr.g_losses()
            ggr = torch.autograd.grad(gout['cost'], tr.g_params, allow_unused=True)
            res.append((out['cost'], grads, gout['cost'], ggr))
        finally:
            M.configure(); lib.delete_all_params()
    assert not CALLS
    _same(res[0][0], res[1][0], 'critic cost')
    _same(res[0][2], res[1][2], 'generator cost')
    for a, b in zip(res[0][1], res[1][1]):
        _same(a, b, 'critic gradient')
    for a, b in zip(res[0][3], res[1][3]):
        _same(a, b, 'generator gradient')


@pytest.mark.parametrize('mode,dim,scheduled', [('wgan-CT', 8, False), ('wgan-CT', 32, True), ('dcgan', 8, False)])
def test_augmented_critic_step_is_the_plain_step_on_augmented_inputs(diffaug_kernels, mode, dim, scheduled):
    """THE equivalence that defines the feature: d_grads with augment on (real, fake) == d_grads with augmentation off on
    (diffaug(real, AUG_REAL), diffaug(fake, AUG_FAKE)) at the same counter, bit for bit - gan_mnist's real_prep is the identity.  On the
    autograd form (DIM 8: outside the hand-scheduled step) and on dcgan_schedule.critic_step (DIM 32), and for one plain objective."""
    import ctgan_amd.dcgan_schedule as DS
    import ctgan_amd.kernels as K
    from ctgan_amd import rng as R
    res = []
    for augment in (POLICY, None):
        M, lib, tr, real_in = _mnist_trainer(mode, augment, dim=dim)
        try:
            fake = tr.generate_fakes(1)[0]
            assert DS.usable(tr, None, fake, real_in) == scheduled
            real = real_in
            if augment is None:
                real = K.diffaug(real_in, MNIST, 7, tr.rng.aug_spec(R.AUG_REAL))
                fake = K.diffaug(fake.contiguous(), MNIST, 7, tr.rng.aug_spec(R.AUG_FAKE))
                assert not torch.equal(real, real_in)
            tr.rng.begin_step()
            out, grads = tr.d_grads(real, fake=fake)
            res.append((out, grads, tr.rng._site))
        finally:
            M.configure(); lib.delete_all_params()
    assert sorted(c[0] for c in CALLS) == [R.AUG_REAL, R.AUG_REAL, R.AUG_FAKE, R.AUG_FAKE] and all(c[1] == 7 and not c[2] for c in CALLS)
    assert res[0][2] == res[1][2], 'the augmentation took a call site of the step'
    keys = ('cost', 'wgan_only', 'ct', 'gp', 'slopes', 'gp_grads') if mode == 'wgan-CT' else ('cost', 'd_real', 'd_fake')
    for k in keys:
        _same(res[0][0][k], res[1][0][k], k)
    assert len(res[0][1]) == len(res[1][1]) > 0
    for a, b in zip(res[0][1], res[1][1]):
        _same(a, b, 'critic gradient')


@pytest.mark.parametrize('mode', ['wgan-CT', 'dcgan'])
def test_generator_step_sees_the_critic_on_augmented_samples(diffaug_kernels, mode):
    import ctgan_amd.functional as F
    import ctgan_amd.kernels as K
    from ctgan_amd import rng as R
    M, lib, tr, _ = _mnist_trainer(mode, POLICY)
    try:
        B = M.cfg.BATCH_SIZE
        tr.rng.begin_step()
        out = tr.g_losses()
        grads = torch.autograd.grad(out['cost'], tr.g_params, allow_unused=True)
        sites = tr.rng._site
        # the same step by hand: generator, T on AUG_GEN, critic
        tr.rng.begin_step()
        x = tr._gen(B, None)
        assert torch.equal(out['samples'], x), 'samples are the un-augmented generator output'
        xa = F.diffaug(x, MNIST, 7, tr.rng.aug_spec(R.AUG_GEN))
        assert torch.equal(xa.detach(), K.diffaug(x.detach(), MNIST, 7, tr.rng.aug_spec(R.AUG_GEN))) and not torch.equal(xa, x)
        with F.weight_grads(False):
            d, _ = M.Discriminator(xa, rng=tr.rng) if mode == 'wgan-CT' else tr._critic(xa, None, tr.towers)
        cost = F.mean_diff(d, B, 0, -1.0, 0.0) if mode == 'wgan-CT' else F.gan_loss(d, B, tr.mode.loss, 'g')
        assert tr.rng._site == sites
        _same(out['cost'], cost, 'generator cost')
        for a, b in zip(grads, torch.autograd.grad(cost, tr.g_params, allow_unused=True)):
            _same(a, b, 'generator gradient through T')
        assert any(c[0] == R.AUG_GEN and c[2] for c in CALLS), 'the backward ran the adjoint launch'
    finally:
        M.configure(); lib.delete_all_params()


def test_integer_reals_are_converted_on_load(diffaug_kernels):
    """gan_cifar feeds int32 pixels: the trainer's one-launch form equals real_prep followed by diffaug."""
    import ctgan_amd.gan_cifar as C
    import ctgan_amd.kernels as K
    import ctgan_amd.tflib as lib
    from ctgan_amd import rng as R
    from ctgan_amd.dcgan_step import DCGANTrainer, image_shape_of
    C.configure(DIM=8, BATCH_SIZE=2)
    try:
        build_params(C, 'cpu')
        tr = DCGANTrainer(C, seed=1, augment='translation,cutout')
        assert tr.aug_policy == 6 and tr.aug_shape == (3, 32, 32) == image_shape_of(C)
        real_in = torch.randint(0, 256, (2, 3072), dtype=torch.int32, generator=torch.Generator().manual_seed(1))
        a = tr.aug_real(real_in)
        b = K.diffaug(C.real_prep(real_in), (3, 32, 32), 6, tr.rng.aug_spec(R.AUG_REAL))
        assert torch.equal(a, b) and len(CALLS) == 2
    finally:
        C.configure(); lib.delete_all_params()
    import ctgan_amd.gan_64x64 as G64
    import ctgan_amd.gan_cifar_resnet as RN
    import ctgan_amd.gan_lsun128 as L
    assert G64.image_shape() == (3, 64, 64) and L.image_shape() == (3, 128, 128) and RN.image_shape() == (3, 32, 32)
    assert image_shape_of(G64) == (3, 64, 64)


def _resnet_scheduled_vs_autograd(R, lib, F, B, D, dev, augment):
    """tests/test_host_logic_resnet._scheduled_vs_autograd with the trainer's `augment`."""
    import ctgan_amd.critic_schedule as CS
    res = {}
    for merged in (False, True):
        lib.delete_all_params(); lib.set_device(dev); lib.set_seed(1)
        R.configure(DIM_G=32, DIM_D=D, BATCH_SIZE=B, CONDITIONAL=True, ACGAN=True)
        R.build_params()
        g = torch.Generator().manual_seed(5)
        with torch.no_grad():
            for n, p in lib._params.items():
                if n.endswith(('.Biases', '.b')):
                    p.add_((0.1 * torch.randn(p.shape, generator=g)).to(p.device))
        tr = R.Trainer(seed=3, augment=augment)
        real = torch.randint(0, 256, (B, 3072), dtype=torch.int32, generator=g).to(tr.dev)
        labels = torch.randint(0, 10, (B,), dtype=torch.int32, generator=g).to(tr.dev)
        old, CS.MERGED_BWD = CS.MERGED_BWD, merged
        try:
            F.prepare_filters()
            fake = tr.generate_fakes(labels)[0]
            assert CS.usable(R, None, tr.rng, real, fake) == merged
            tr.rng.begin_step()
            out, grads = tr.d_grads(real, labels, fake=fake)
        finally:
            CS.MERGED_BWD = old
        res[merged] = (out, grads, [n for n, _ in tr.d_named], fake)
    return res[False], res[True]


def test_resnet_scheduled_step_equals_the_autograd_path_with_augmentation_on(diffaug_kernels):
    """The ResNet trainer with augmentation on: critic_schedule.critic_step on Trainer.augmented_prep against d_losses + autograd - the
    quantities and the tolerances (2e-6 / atol 1e-7 on the loss terms, 5e-6 / atol 1e-8 on the parameter gradients) of
    tests/test_host_logic_resnet.py::test_hand_scheduled_critic_step_equals_the_autograd_path.  The augmentation is live (the reals the
    step reports differ from the un-augmented ones) and out['fake'] stays the generator's samples."""
    import ctgan_amd.functional as F
    import ctgan_amd.gan_cifar_resnet as R
    import ctgan_amd.tflib as lib
    from ctgan_amd import rng as RNG
    try:
        a, b = _resnet_scheduled_vs_autograd(R, lib, F, 2, 64, 'cpu', POLICY)
        assert sorted(c[0] for c in CALLS) == [RNG.AUG_REAL, RNG.AUG_REAL, RNG.AUG_FAKE, RNG.AUG_FAKE]
        for k in ('cost', 'wgan', 'acgan', 'wgan_only', 'ct', 'gp', 'acc_real', 'acc_fake', 'slopes', 'gp_grads', 'd_real', 'd_fake', 'real'):
            assert (a[0].get(k) is None) == (b[0].get(k) is None), k
            if a[0].get(k) is not None:
                _cmp(b[0][k], a[0][k], 2e-6, 'scheduled.' + k, atol=1e-7)
        assert torch.equal(a[0]['real'], b[0]['real'])
        assert torch.equal(a[0]['fake'], a[3]) and torch.equal(b[0]['fake'], b[3])
        assert a[2] == b[2]
        for n, x, y in zip(a[2], a[1], b[1]):
            assert (x is None) == (y is None), n
            if x is not None:
                _cmp(y, x, 5e-6, 'scheduled grad ' + n, atol=1e-8)
        plain, _ = _resnet_scheduled_vs_autograd(R, lib, F, 2, 64, 'cpu', None)
        assert not torch.equal(plain[0]['real'], a[0]['real'])
        # the generator step: the critic on T(samples), one call over both towers' rows
        del CALLS[:]
        lib.delete_all_params(); lib.set_seed(1)
        R.configure(DIM_G=32, DIM_D=64, BATCH_SIZE=2)
        R.build_params()
        tr = R.Trainer(seed=3, augment=POLICY)
        F.prepare_filters()
        tr.rng.begin_step()
        out = tr.g_losses()
        torch.autograd.grad(out['cost'], tr.g_params, allow_unused=True)
        assert [c for c in CALLS if c[0] == RNG.AUG_GEN] == [(RNG.AUG_GEN, 7, False), (RNG.AUG_GEN, 7, True)]
        assert out['samples'].shape[0] == R.cfg.GEN_BS_MULTIPLE * 2
    finally:
        R.configure(); lib.delete_all_params()


# ----------------------------------------------------------------------------- the C entry point's argument checks
def test_entry_point_refuses_bad_arguments_before_any_launch():
    """As tests/test_abi_and_layout.py::test_error_reporting_without_gpu: validation happens before any launch.  Pointers are never
    dereferenced on the host, so dummy non-null values serve."""
    from ctgan_amd import _lib
    f = _lib.lib.ctgan_diffaug
    P = ctypes.c_void_p(4096)
    good = dict(x=P, x_int=None, denom=1.0, y=P, n=2, c=3, h=8, w=8, policy=7, adjoint=0, seed=1, sid=5, ctr=None, params=None)

    def call(**kw):
        a = dict(good, **kw)
        return f(a['x'], a['x_int'], a['denom'], a['y'], a['n'], a['c'], a['h'], a['w'], a['policy'], a['adjoint'], a['seed'], a['sid'], a['ctr'],
                 a['params'], None)
    bad = [dict(y=None), dict(x=None), dict(x_int=P), dict(x=None, x_int=P, adjoint=1), dict(n=0), dict(c=0), dict(h=0), dict(w=0), dict(c=17),
           dict(policy=8), dict(sid=1 << 32), dict(x=None, x_int=P, denom=0.0), dict(denom=0.0), dict(adjoint=3), dict(n=-1)]
    for kw in bad:
        assert call(**kw) == -1, kw
        assert b'diffaug' in _lib.lib.ctgan_last_error(), kw
    assert call(policy=8) == -1 and b'policy' in _lib.lib.ctgan_last_error()
    assert call(x=None, x_int=P, adjoint=1) == -1 and b'integer' in _lib.lib.ctgan_last_error()
