"""The second derivative of self-attention on the device: kernels.attention_bwd2 / attn_residual_bwd2 of csrc/attention.hip, the
twice-differentiable operators of ctgan_amd/attention.py (attention2, attn_residual2, SelfAttention(..., second_order=True)) and the CT critic
step of the ResNet with gan_cifar_resnet.Config.ATTENTION_D + ATTENTION_SECOND_ORDER (eager here; under graph replay in
tests/test_gpu_trainers_attention2.py, a file collected after tests/test_gpu_kernels.py because a graph engine creates a stream).

Tolerance, measured, not guessed (the rule of tests/test_gpu_attention.py): every case is evaluated three times - fp64 (tests/attention2_oracle.py:
autograd of the composite, differentiated twice), the fp32 CPU stand-in (tests/attention2_cpu_kernels.py) and the device - and the device's
largest error, relative to the fp64 result's largest magnitude per tensor, may be at most 4 x the stand-in's (the margin is for another
summation order and the device's exp); the stand-in itself must be under 1e-4.  Both figures are printed."""
import pytest
import torch

from tests import attention2_cpu_kernels as A2K
from tests import attention2_oracle as A2O
from tests import attention_cpu_kernels as AK
from tests import attention_oracle as AO

pytestmark = pytest.mark.gpu

# one block; a partial block alone; exactly one block; full plus partial; the workload's shape; both operand maxima with a partial block
SHAPES = [(1, 16, 4, 16), (2, 48, 4, 16), (3, 64, 16, 64), (2, 80, 8, 32), (2, 256, 16, 64), (1, 320, 64, 128)]
AT80 = (2, 80, 8, 32)
# (shape, kind, absent cotangents): the zero substitution of the host is covered at the full-plus-partial shape
CASES = ([(s, 'normal', '') for s in SHAPES] + [(AT80, 'scores80', ''), (AT80, 'equal_row', ''), (AT80, 'normal', 'c'), (AT80, 'normal', 'ab')])
RATIO = 4.0
NAMES = ('dq', 'dk', 'dv', 'dgout')


def _zeros_for(t, like):
    return torch.zeros_like(like) if t is None else t


_REF = {}


def _reference(shape, kind, absent):
    """(inputs with None for the absent cotangents, lse, delta, fp64 results, fp32 stand-in results): once per case, left unchanged"""
    key = (shape, kind, absent)
    if key not in _REF:
        q, k, v, gout, a, b, c = A2O.inputs(shape, kind)
        if 'a' in absent:
            a = None
        if 'b' in absent:
            b = None
        if 'c' in absent:
            c = None
        ref = A2O.core_grads2(q, k, v, gout, a, b, c)
        out, lse = AK.attention_fwd(q, k, v)
        delta = A2K.attention_bwd_delta(q, k, v, out, lse, gout)[3]
        cpu = A2K.attention_bwd2(q, k, v, lse, delta, gout, _zeros_for(a, q), _zeros_for(b, k), _zeros_for(c, v))
        _REF[key] = ((q, k, v, gout, a, b, c), ref, cpu)
    return _REF[key]


def _rel_err(a, ref):
    return float((a.detach().cpu().double() - ref).abs().max() / ref.abs().max())


def _device_bwd2(q, k, v, gout, a, b, c):
    """the device's own chain: forward, first backward (lse, delta), second backward"""
    import ctgan_amd.kernels as K
    out, lse = K.attention_fwd(q, k, v)
    delta = K.attention_bwd_delta(q, k, v, out, lse, gout)[3]
    return K.attention_bwd2(q, k, v, lse, delta, gout, _zeros_for(a, q), _zeros_for(b, k), _zeros_for(c, v))


@pytest.mark.parametrize('shape,kind,absent', CASES, ids=['%dx%dx%dx%d-%s%s' % (s + (k, '-no_' + z if z else '')) for s, k, z in CASES])
def test_core_second_derivative_against_fp64(shape, kind, absent):
    (q, k, v, gout, a, b, c), ref, cpu = _reference(shape, kind, absent)
    if kind == 'scores80':
        assert 79.9 < float((q.double() @ k.double().transpose(1, 2)).abs().max()) < 80.1
    if kind == 'equal_row':
        assert float((q[:, 5].double() @ k.double().transpose(1, 2)).abs().max()) == 0.0
    dev = _device_bwd2(*(t.cuda() if t is not None else None for t in (q, k, v, gout, a, b, c)))
    torch.cuda.synchronize()
    bad = []
    for name, d, s, r in zip(NAMES, dev, cpu, ref):
        assert torch.isfinite(d).all(), name
        if float(r.abs().max()) == 0.0:           # dv with a = b absent: W = P o (T - tau) with T = 0 is exactly zero
            assert name == 'dv' and absent == 'ab' and float(d.abs().max()) == 0.0 and float(s.abs().max()) == 0.0, name
            continue
        e_dev, e_cpu = _rel_err(d, r), _rel_err(s, r)
        print('attention_bwd2 %s %s%s %-5s: device %.3e  stand-in %.3e  ratio %.2f'
              % (shape, kind, ' no ' + absent if absent else '', name, e_dev, e_cpu, e_dev / max(e_cpu, 1e-30)))
        assert e_cpu < 1e-4, (name, e_cpu)                    # the stand-in itself is an fp32 evaluation of the same formulas
        if e_dev > RATIO * e_cpu:
            bad.append((name, e_dev, e_cpu))
    assert not bad, bad


def test_same_bits_on_every_run_and_in_any_company():
    """two runs agree bit for bit; image 0 of an n = 3 launch is the n = 1 launch of that image"""
    ins = tuple(t.cuda() for t in A2O.inputs((3, 80, 8, 32), 'normal', seed=7))
    x, y = _device_bwd2(*ins), _device_bwd2(*ins)
    alone = _device_bwd2(*(t[0:1].contiguous() for t in ins))
    torch.cuda.synchronize()
    for name, p, r, z in zip(NAMES, x, y, alone):
        assert torch.equal(p, r), name
        assert torch.equal(p[0:1], z), name


def test_bad_shapes_and_cpu_tensors_are_refused_by_name():
    import ctgan_amd.kernels as K
    for (N, dk, dv), word in (((24, 4, 16), 'N'), ((16, 6, 16), 'dk'), ((16, 4, 8), 'dv'), ((16, 68, 16), 'dk'), ((16, 4, 144), 'dv')):
        q, v, row = torch.zeros(1, N, dk).cuda(), torch.zeros(1, N, dv).cuda(), torch.zeros(1, N).cuda()
        with pytest.raises(ValueError, match=r'attention_bwd2: %s = ' % word):
            K.attention_bwd2(q, q, v, row, row, v, q, q, v)
    q, v, row = torch.zeros(1, 16, 4), torch.zeros(1, 16, 16), torch.zeros(1, 16)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        K.attention_bwd2(q, q, v, row, row, v, q, q, v)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        K.attn_residual_bwd2(torch.zeros(1, 4, 2, 2), torch.zeros(1, 4, 2, 2), torch.zeros(1), torch.zeros(1, 4, 2, 2))


@pytest.mark.parametrize('with_cgg', [True, False], ids=['cgg', 'no_cgg'])
@pytest.mark.parametrize('shape', [(2, 32, 4, 4), (3, 128, 16, 16)], ids=['2x32x4x4', '3x128x16x16'])
def test_gated_residual_second_derivative_against_fp64(shape, with_cgg):
    """Bound, of the largest magnitude of each tensor: d_o = cgg gy and (without cgg) dgy = gamma cgo are one fp32 product per element
    (2 ulp: 2.4e-7, the bound of tests/test_gpu_attention.py for go); with cgg, dgy = gamma cgo + cgg o is two products and a sum, each
    rounded once, of terms that are each at most about the result's largest magnitude (3 roundings of <= 2 x that magnitude, 2^-24 each:
    3.6e-7, taken at 4.8e-7); dgamma is an fp64 sum of exact products rounded once to fp32 (6e-8, taken at 2.4e-7)."""
    import ctgan_amd.kernels as K
    n, c, h, w = shape
    g = torch.Generator().manual_seed(3)
    gy, o, cgo = (torch.randn(n, h, w, c, generator=g).permute(0, 3, 1, 2) for _ in range(3))
    gamma, cgg = torch.tensor([0.7]), (torch.tensor([-1.3]) if with_cgg else None)
    ref = A2O.residual_grads2(gy, o, gamma, cgo, cgg)
    dev_in = [t.cuda() for t in (gy, o, gamma, cgo)] + [cgg.cuda() if with_cgg else None]
    got, again = K.attn_residual_bwd2(*dev_in), K.attn_residual_bwd2(*dev_in)
    torch.cuda.synchronize()
    assert (got[1] is None) == (ref[1] is None) == (not with_cgg)
    assert got[0].stride() == dev_in[1].stride() and tuple(got[2].shape) == (1,)
    for name, x, y, r, bound in zip(('dgy', 'd_o', 'dgamma'), got, again, ref, (4.8e-7 if with_cgg else 2.4e-7, 2.4e-7, 2.4e-7)):
        if x is None:
            continue
        assert torch.equal(x, y), name
        err = _rel_err(x, r.reshape(x.shape))
        print('attn_residual_bwd2 %s %s %s: %.3e' % (shape, 'cgg' if with_cgg else 'no cgg', name, err))
        assert err <= bound, (name, err)


# ------------------------------------------------------------------------------------------------------------------ the operator
def _block_second_grads(block, x, params, gy, cot):
    """d/d(x, params) of <d<block(x), gy>/dx, cot>: the penalty's shape of a second derivative"""
    y = block(x, *params)
    (gx,) = torch.autograd.grad(y, x, gy, create_graph=True)
    return y, gx, torch.autograd.grad((gx * cot).sum(), [x] + list(params), allow_unused=True)


def test_operator_is_twice_differentiable_on_the_device():
    """attention.SelfAttention(..., second_order=True) on the device, gamma = 0.7, random weights: the gradient in x under create_graph, then a
    second grad to every parameter and to x, against the fp64 block (tests/attention_oracle.block) at 1e-4 of each tensor's largest magnitude
    (the bound of tests/test_gpu_attention.py for the block's first-order quantities: fp32 products over at most 256 terms through a few
    chained operators stay two orders below it; a wrong term is of order 1).  A third differentiation raises by name; the forward and the
    first-order gradients are the first-order operator's bits."""
    import ctgan_amd.tflib as lib
    from ctgan_amd import attention as A
    try:
        lib.delete_all_params(); lib.set_device(None); lib.set_seed(2)
        dim, n, H = 32, 2, 8
        g = torch.Generator().manual_seed(4)
        x0 = torch.randn(n, H, H, dim, generator=g).permute(0, 3, 1, 2)
        with torch.no_grad():
            A.SelfAttention('T.Attention', dim, x0.cuda(), second_order=True)
        names = ['T.Attention.' + s for s in A.PARAMS]
        assert list(lib._params) == names
        with torch.no_grad():
            for nm in names:
                p = lib._params[nm]
                p.copy_(torch.full((1,), 0.7) if nm.endswith('gamma') else torch.randn(p.shape, generator=g) * 0.2)
        lib.bump_epoch()
        params = [lib._params[nm] for nm in names]
        gy, cot = torch.randn(x0.shape, generator=g), torch.randn(x0.shape, generator=g)

        def on_device(x, *_):
            return A.SelfAttention('T.Attention', dim, x, second_order=True)

        x = x0.cuda().requires_grad_(True)
        y, gx, second = _block_second_grads(on_device, x, params, gy.cuda(), cot.cuda())
        xr = x0.double().requires_grad_(True)
        pr = [p.detach().cpu().double().requires_grad_(True) for p in params]
        yr, gxr, second_r = _block_second_grads(AO.block, xr, pr, gy.double(), cot.double())
        for what, a, b in [('y', y, yr.detach()), ('gx', gx, gxr.detach())] + list(zip(['d2 x'] + ['d2 ' + nm for nm in names], second, second_r)):
            assert a is not None and b is not None, what
            err = _rel_err(a, b)
            print('SelfAttention second order %s: %.3e' % (what, err))
            assert float(b.abs().max()) > 1e-3, what                 # (a vanishing reference would check nothing)
            assert err <= 1e-4, (what, err)
        # the first-order operator's bits, forward and gradients
        x1 = x0.cuda().requires_grad_(True)
        y1 = A.SelfAttention('T.Attention', dim, x1)
        x2 = x0.cuda().requires_grad_(True)
        y2 = A.SelfAttention('T.Attention', dim, x2, second_order=True)
        assert torch.equal(y1, y2) and torch.equal(y1, y.detach())
        for a, b in zip(torch.autograd.grad(y1, [x1] + params, gy.cuda()), torch.autograd.grad(y2, [x2] + params, gy.cuda())):
            assert torch.equal(a, b)
        # a third differentiation is refused by name
        q, k = (torch.randn(1, 16, 4, generator=g).cuda().requires_grad_(True) for _ in range(2))
        v = torch.randn(1, 16, 16, generator=g).cuda().requires_grad_(True)
        (gq,) = torch.autograd.grad(A.attention2(q, k, v).sum(), q, create_graph=True)
        with pytest.raises(RuntimeError, match='AttentionBwdFn is first order only'):
            torch.autograd.grad(gq.sum(), k, create_graph=True)
        xs = torch.randn(1, 16, 2, 2, generator=g).cuda().requires_grad_(True)
        gamma = torch.full((1,), 0.5).cuda().requires_grad_(True)
        (go,) = torch.autograd.grad(A.attn_residual2(xs.detach(), xs * 2, gamma).sum(), xs, create_graph=True)
        with pytest.raises(RuntimeError, match='AttnResidualBwdFn is first order only'):
            torch.autograd.grad(go.sum(), gamma, create_graph=True)
    finally:
        lib.delete_all_params()


# ------------------------------------------------------------------------------------------------------------------ step level
DIM, BS = 32, 4
D_GATE = 'Discriminator.Attention.gamma'
ON = dict(ATTENTION_D=True, ATTENTION_SECOND_ORDER=True)


def _build(R, lib, dev, seed=5, **kw):
    from tests import hinge_step_checks as HC
    HC.build(R, lib, dev, DIM, BS, seed=seed, **kw)
    HC.shake(lib)
    with torch.no_grad():
        for n in ('Generator.Attention.gamma', D_GATE):
            if n in lib._params:
                lib._params[n].fill_(0.5)
    lib.bump_epoch()


def _wire_oracle(monkeypatch):
    """oracle.nets' critic with the fp64 block (tests/attention_oracle.block) in front of Discriminator.2 (and the generator's in front of
    Generator.3), as tests/test_gpu_attention.py wires it: nothing under oracle/ changes"""
    from oracle import nets as onets
    orig = onets.ResidualBlock

    def block(reg_, cfg, name, input_dim, output_dim, filter_size, inputs, **kw):
        site = {'Generator.3': 'Generator.Attention', 'Discriminator.2': 'Discriminator.Attention'}.get(name)
        if site is not None and site + '.gamma' in reg_:
            inputs = AO.block(inputs, *(reg_[site + '.' + s] for s in ('Query.Filters', 'Key.Filters', 'Value.Filters', 'Out.Filters', 'gamma')))
        return orig(reg_, cfg, name, input_dim, output_dim, filter_size, inputs, **kw)

    monkeypatch.setattr(onets, 'ResidualBlock', block)


def _ct_step_grads(R, lib, dev, real, labels, rnd_d):
    """the eager CT critic step (objective=None) with injected draws -> ({name: grad}, its fake batch, its gp)"""
    from tests import hinge_step_checks as HC
    tr = R.Trainer(seed=1)
    tr.rng.begin_step()
    out, dg = tr.d_grads(real.to(dev), labels.to(dev), {k: HC.to_dev(v, dev) for k, v in rnd_d.items()})
    d = {n: g.detach().cpu() for (n, _), g in zip(tr.d_named, dg) if g is not None}
    return d, out['fake'].detach().cpu(), float(out['gp'].detach())


def _ref_ct_d_grads(monkeypatch, reg, cfg, real, labels, rnd_d, fake):
    """fp64 critic gradients of oracle.steps.resnet_d_losses - the CT critic losses: WGAN + CT + 10 GP + ACGAN - with `fake`, the evaluation
    under test's own fake batch, in place of the fp64 generator's (an fp32 fake a few 1e-6 from the fp64 one now and then lies
    across a ReLU kink of the critic, and then every gradient differs by 1e-3 to 1e-2 with nothing wrong).  -> ({name: grad}, gp)"""
    from oracle import nets as onets, steps as osteps
    halves = list(fake.double().split(fake.shape[0] // 2))
    with monkeypatch.context() as m:
        m.setattr(onets, 'resnet_generator', lambda *a, **k: halves.pop(0))
        out = osteps.resnet_d_losses(reg, cfg, real, labels, rnd_d, B=BS)
    assert not halves and torch.equal(out['fake'], fake.double())
    return osteps.grads_of(out['cost'], reg, 'Discriminator.'), float(out['gp'].detach())


def _worst(got, want):
    """the largest per-tensor relative error; a tensor under 1e-9 of the largest gradient has no scale to measure against and must be as
    good as zero instead (tests/test_gpu_attention.py)"""
    assert set(got) == set(want), set(got) ^ set(want)
    top = max(float(w.abs().max()) for w in want.values())
    worst = 0.0
    for n, w in want.items():
        if float(w.abs().max()) < 1e-9 * top:
            assert float(got[n].abs().max()) <= 1e-5 * top, n
        else:
            worst = max(worst, _rel_err(got[n], w))
    return worst


def test_eager_ct_step_gradients_against_the_fp64_oracle(monkeypatch):
    """DIM 32, B 4, objective=None (the CT objective), ATTENTION_G + ATTENTION_D + ATTENTION_SECOND_ORDER, both gates at 0.5, injected
    draws: the critic's parameter gradients of the eager CT step on the device and on the CPU stand-ins, each against the oracle's fp64 CT
    critic losses with the fp64 block wired in front of Discriminator.2, taken at that evaluation's own fake batch.  The device's largest
    relative error (per tensor, relative to its largest magnitude) may be at most 4 x the stand-ins', and the stand-ins' under 1e-3.  The
    gate and the query filters are among the gradients and the penalty is non-zero: the second derivative of the block is in the step."""
    import ctgan_amd.gan_cifar_resnet as R
    import ctgan_amd.kernels as K
    import ctgan_amd.tflib as lib
    from oracle import steps as osteps
    from tests import cpu_kernels as C
    from tests import hinge_cpu_kernels as HK
    from tests import hinge_step_checks as HC
    kw = dict(ATTENTION_G=True, **ON)
    g = torch.Generator().manual_seed(11)
    real = torch.randint(0, 256, (BS, 3072), generator=g, dtype=torch.int32)
    labels = torch.randint(0, 10, (BS,), generator=g, dtype=torch.int32)
    rnd_d = osteps.make_rnd_resnet_d(BS, DIM, g)
    try:
        with monkeypatch.context() as m:              # the same step on the fp32 CPU stand-ins
            for mod in (C, HK, AK, A2K):
                for name in mod.__all__:
                    m.setattr(K, name, getattr(mod, name))
            _build(R, lib, 'cpu', **kw)
            cpu = _ct_step_grads(R, lib, 'cpu', real, labels, rnd_d)
        _build(R, lib, 'cuda', **kw)
        reg = HC.oracle_from_product(lib)
        dev = _ct_step_grads(R, lib, 'cuda', real, labels, rnd_d)
    finally:
        lib.delete_all_params(); lib.set_device(None); R.configure()
    _wire_oracle(monkeypatch)
    cfg = HC.oracle_cfg(DIM, HC.HEADS['acgan'])
    err = {}
    for who, (got, fake, gp) in (('device', dev), ('stand-ins', cpu)):
        want, gp_ref = _ref_ct_d_grads(monkeypatch, reg, cfg, real, labels, rnd_d, fake)
        assert all(n in want and n in got for n in (D_GATE, 'Discriminator.Attention.Query.Filters'))
        assert gp_ref > 1e-3 and gp > 1e-3, (who, gp, gp_ref)                                # the penalty term is there, and non-zero
        err[who] = _worst(got, want)
    e_dev, e_cpu = err['device'], err['stand-ins']
    print('CT step critic gradients: device %.3e  stand-ins %.3e  ratio %.2f' % (e_dev, e_cpu, e_dev / max(e_cpu, 1e-30)))
    assert e_cpu < 1e-3, e_cpu                        # the stand-ins follow the oracle: the wiring is right
    assert e_dev <= RATIO * e_cpu, (e_dev, e_cpu)
