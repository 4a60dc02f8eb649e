"""The self-attention kernels of csrc/attention.hip on the device (kernels.attention_fwd / attention_bwd / attn_residual_fwd / attn_residual_bwd),
the operator of ctgan_amd/attention.py and the ResNet steps with gan_cifar_resnet.Config.ATTENTION_G / ATTENTION_D.

Tolerance of the core, measured, not guessed: every case is evaluated three times - fp64 (tests/attention_oracle.py), the fp32 CPU stand-in
(tests/attention_cpu_kernels.py) and the device - and the device's largest error, relative to the fp64 result's largest magnitude per tensor,
may be at most 4 x the stand-in's (the margin is for another summation order and the device's exp).  Both figures are printed."""
import numpy as np
import pytest
import torch

from tests import attention_cpu_kernels as AK
from tests import attention_oracle as AO

pytestmark = pytest.mark.gpu

# one block; a partial block alone; exactly one block; full plus partial; the workload's shape; both operand maxima with a partial block
SHAPES = [(1, 16, 4, 16), (2, 48, 4, 16), (3, 64, 16, 64), (2, 80, 8, 32), (2, 256, 16, 64), (1, 320, 64, 128)]
CASES = [(s, 'normal') for s in SHAPES] + [((2, 80, 8, 32), 'scores80'), ((2, 80, 8, 32), 'equal_row')]
RATIO = 4.0


def _inputs(shape, kind, seed=0):
    n, N, dk, dv = shape
    g = torch.Generator().manual_seed(seed + 1000 * N + dk)
    q, k = torch.randn(n, N, dk, generator=g), torch.randn(n, N, dk, generator=g)
    v, gout = torch.randn(n, N, dv, generator=g), torch.randn(n, N, dv, generator=g)
    if kind == 'scores80':          # the largest |score| is 80: exp overflows fp32 (e^88) within a row sum unless the maximum is subtracted
        s = (q.double() @ k.double().transpose(1, 2)).abs().max().sqrt().item()
        q, k = q * (80 ** 0.5 / s), k * (80 ** 0.5 / s)
    if kind == 'equal_row':         # a zero query: every score of the row is 0, P is uniform
        q[:, 5] = 0.
    return q, k, v, gout


_REF = {}


def _reference(shape, kind):
    """(inputs, fp64 results, fp32 stand-in results), computed once per case and left unchanged"""
    key = (shape, kind)
    if key not in _REF:
        q, k, v, gout = _inputs(shape, kind)
        ref = AO.core_grads(q, k, v, gout)
        out, lse = AK.attention_fwd(q, k, v)
        _REF[key] = ((q, k, v, gout), ref, (out, lse) + tuple(AK.attention_bwd(q, k, v, out, lse, gout)))
    return _REF[key]


def _rel_err(a, ref):
    return float((a.detach().cpu().double() - ref).abs().max() / ref.abs().max())


@pytest.mark.parametrize('shape,kind', CASES, ids=['%dx%dx%dx%d-%s' % (s + (k,)) for s, k in CASES])
def test_core_forward_and_backward_against_fp64(shape, kind):
    import ctgan_amd.kernels as K
    (q, k, v, gout), ref, cpu = _reference(shape, kind)
    if kind == 'scores80':
        s = q.double() @ k.double().transpose(1, 2)
        assert 79.9 < float(s.abs().max()) < 80.1
    if kind == 'equal_row':
        assert float((q[:, 5].double() @ k.double().transpose(1, 2)).abs().max()) == 0.0
    qd, kd, vd, gd = (t.cuda() for t in (q, k, v, gout))
    out, lse = K.attention_fwd(qd, kd, vd)
    out_nolse, none = K.attention_fwd(qd, kd, vd, want_lse=False)
    assert none is None and torch.equal(out_nolse, out)
    dev = (out, lse) + tuple(K.attention_bwd(qd, kd, vd, out, lse, gd))
    torch.cuda.synchronize()
    bad = []
    for name, d, c, r in zip(('out', 'lse', 'gq', 'gk', 'gv'), dev, cpu, ref):
        assert torch.isfinite(d).all(), name
        e_dev, e_cpu = _rel_err(d, r), _rel_err(c, r)
        print('attention %s %s %-3s: device %.3e  stand-in %.3e  ratio %.2f' % (shape, kind, name, e_dev, e_cpu, e_dev / max(e_cpu, 1e-30)))
        assert e_cpu < 1e-4, (name, e_cpu)                    # the stand-in itself is an fp32 evaluation of the same formulas
        if e_dev > RATIO * e_cpu:
            bad.append((name, e_dev, e_cpu))
    assert not bad, bad


def test_bad_shapes_are_refused_by_name():
    import ctgan_amd.kernels as K
    for (N, dk, dv), word in (((24, 4, 16), 'N'), ((16, 6, 16), 'dk'), ((16, 4, 8), 'dv'), ((16, 68, 16), 'dk')):
        q, k, v = torch.zeros(1, N, dk).cuda(), torch.zeros(1, N, dk).cuda(), torch.zeros(1, N, dv).cuda()
        with pytest.raises(ValueError, match=r'attention_fwd: %s = ' % word):
            K.attention_fwd(q, k, v)
        with pytest.raises(ValueError, match=r'attention_bwd: %s = ' % word):
            K.attention_bwd(q, k, v, v, torch.zeros(1, N).cuda(), v)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        K.attention_fwd(torch.zeros(1, 16, 4), torch.zeros(1, 16, 4), torch.zeros(1, 16, 16))


def test_same_bits_on_every_run_and_in_any_company():
    import ctgan_amd.kernels as K
    q, k, v, gout = (t.cuda() for t in _inputs((3, 80, 8, 32), 'normal', seed=7))

    def run(q, k, v, gout):
        out, lse = K.attention_fwd(q, k, v)
        return (out, lse) + tuple(K.attention_bwd(q, k, v, out, lse, gout))

    a, b = run(q, k, v, gout), run(q, k, v, gout)
    alone = run(*(t[1:2].contiguous() for t in (q, k, v, gout)))
    torch.cuda.synchronize()
    for name, x, y, z in zip(('out', 'lse', 'gq', 'gk', 'gv'), a, b, alone):
        assert torch.equal(x, y), name
        assert torch.equal(x[1:2], z), name


@pytest.mark.parametrize('shape', [(2, 32, 4, 4), (3, 128, 16, 16)], ids=['2x32x4x4', '3x128x16x16'])
def test_gated_residual_against_fp64(shape):
    """Bound: y and go are one fp32 multiply-add per element (2 ulp of the result's magnitude: 2.4e-7 of the largest); the gate's gradient is
    an fp64 sum of exact products rounded once to fp32 (6e-8, taken at 2.4e-7 as well)."""
    import ctgan_amd.kernels as K
    n, c, h, w = shape
    g = torch.Generator().manual_seed(3)
    x, o, gy = (torch.randn(n, h, w, c, generator=g).permute(0, 3, 1, 2) for _ in range(3))
    gamma = torch.tensor([0.7])
    xd, od, gyd, gd = (t.cuda() for t in (x, o, gy, gamma))
    assert xd.permute(0, 2, 3, 1).is_contiguous()
    y = K.attn_residual_fwd(xd, od, gd)
    go, gg = K.attn_residual_bwd(gyd, od, gd)
    go2, gg2 = K.attn_residual_bwd(gyd, od, gd)
    torch.cuda.synchronize()
    assert torch.equal(gg, gg2) and torch.equal(go, go2)
    assert y.stride() == xd.stride() and go.stride() == od.stride() and tuple(gg.shape) == (1,)
    g64 = gamma.double()
    for name, got, want in (('y', y, x.double() + g64 * o.double()), ('go', go, g64 * gy.double()),
                            ('ggamma', gg, (gy.double() * o.double()).sum().reshape(1))):
        err = _rel_err(got, want)
        print('attn_residual %s %s: %.3e' % (shape, name, err))
        assert err <= 2.4e-7, (name, err)


# ------------------------------------------------------------------------------------------------------------------ the operator
def test_operator_on_the_device_matches_fp64_and_refuses_a_second_derivative():
    """attention.SelfAttention on the device, gamma = 0.7, against the fp64 block: 1e-4 of each tensor's largest magnitude (the bound of
    tests/test_attention_host.py for the same quantities); under no_grad the same output bits."""
    import ctgan_amd.tflib as lib
    from ctgan_amd import attention as A
    try:
        lib.delete_all_params(); lib.set_device(None); lib.set_seed(2)
        dim, n, H = 32, 2, 8
        g = torch.Generator().manual_seed(4)
        x0 = torch.randn(n, H, H, dim, generator=g).permute(0, 3, 1, 2)
        with torch.no_grad():
            A.SelfAttention('T.Attention', dim, x0.cuda())
        names = ['T.Attention.' + s for s in A.PARAMS]
        assert list(lib._params) == names
        with torch.no_grad():
            for nm in names:
                p = lib._params[nm]
                p.copy_(torch.full((1,), 0.7) if nm.endswith('gamma') else torch.randn(p.shape, generator=g) * 0.2)
        lib.bump_epoch()
        params = [lib._params[nm] for nm in names]
        x = x0.cuda().requires_grad_(True)
        y = A.SelfAttention('T.Attention', dim, x)
        gy = torch.randn(y.shape, generator=g)
        grads = torch.autograd.grad(y, [x] + params, gy.cuda())
        with torch.no_grad():
            assert torch.equal(A.SelfAttention('T.Attention', dim, x.detach()), y.detach())
        xr = x0.double().requires_grad_(True)
        pr = [p.detach().cpu().double().requires_grad_(True) for p in params]
        yr = AO.block(xr, *pr)
        gr = torch.autograd.grad(yr, [xr] + pr, gy.double())
        for what, a, b in [('y', y, yr.detach())] + list(zip(['x'] + names, grads, gr)):
            err = _rel_err(a, b)
            print('SelfAttention %s: %.3e' % (what, err))
            assert err <= 1e-4, (what, err)
        q, k = (torch.randn(1, 16, 4, generator=g).cuda().requires_grad_(True) for _ in range(2))
        v = torch.randn(1, 16, 16, generator=g).cuda().requires_grad_(True)
        with pytest.raises(RuntimeError, match='AttentionFn is first order only'):
            (gq,) = torch.autograd.grad(A.attention(q, k, v).sum(), q, create_graph=True)
            torch.autograd.grad(gq.sum(), k)
    finally:
        lib.delete_all_params()


# ------------------------------------------------------------------------------------------------------------------ step level
DIM, BS = 32, 4
GATES = ('Generator.Attention.gamma', 'Discriminator.Attention.gamma')


def _build(R, lib, dev, seed=5, **kw):
    from tests import hinge_step_checks as HC
    HC.build(R, lib, dev, DIM, BS, seed=seed, **kw)
    HC.shake(lib)
    with torch.no_grad():
        for n in GATES:
            if n in lib._params:
                lib._params[n].fill_(0.5)
    lib.bump_epoch()


def _wire_oracle(monkeypatch, reg):
    """oracle.nets' ResNets with the fp64 block (tests/attention_oracle.block) in front of Generator.3 and Discriminator.2"""
    from oracle import nets as onets
    orig = onets.ResidualBlock

    def block(reg_, cfg, name, input_dim, output_dim, filter_size, inputs, **kw):
        site = {'Generator.3': 'Generator.Attention', 'Discriminator.2': 'Discriminator.Attention'}.get(name)
        if site is not None and site + '.gamma' in reg_:
            inputs = AO.block(inputs, *(reg_[site + '.' + s] for s in ('Query.Filters', 'Key.Filters', 'Value.Filters', 'Out.Filters', 'gamma')))
        return orig(reg_, cfg, name, input_dim, output_dim, filter_size, inputs, **kw)

    monkeypatch.setattr(onets, 'ResidualBlock', block)


def _step_grads(R, lib, dev, real, labels, rnd_d, rnd_g):
    """eager critic and generator gradients of the hinge step with injected draws, from the registry as it stands
    -> ({name: grad}, {name: grad}, the critic step's fake batch, the generator step's samples)"""
    from tests import hinge_step_checks as HC
    tr = R.Trainer(seed=1, objective='hinge')
    tr.rng.begin_step()
    out, dg = tr.d_grads(real.to(dev), labels.to(dev), {k: HC.to_dev(v, dev) for k, v in rnd_d.items()})
    tr.rng.begin_step()
    gout = tr.g_losses({k: HC.to_dev(v, dev) for k, v in rnd_g.items()})
    gg = torch.autograd.grad(gout['cost'], tr.g_params, allow_unused=True)
    d = {n: g.detach().cpu() for (n, _), g in zip(tr.d_named, dg) if g is not None}
    g = {n: g_.detach().cpu() for (n, _), g_ in zip(tr.g_named, gg) if g_ is not None}
    return d, g, out['fake'].detach().cpu(), gout['samples'].detach().cpu()


def _ref_d_grads(reg, cfg, real, labels, rnd_d, fake):
    """fp64 critic gradients of the hinge step (tests/hinge_step_checks.ref_d_losses: one dropout pass over [real ; fake], both hinges, the
    class term on the real rows) with `fake` - the evaluation under test's own fake batch - in place of the fp64 generator's (_ref_g_grads
    says why).  -> ({name: grad}, the smallest distance of a hinge from its kink)"""
    from oracle import nets as onets, steps as osteps, tf_ops
    from tests.loss_heads_cases import hinge
    B = real.shape[0]
    rf = torch.cat([osteps.resnet_real_prep(real, rnd_d['dequant']), fake.double()], 0)
    d, _, a = onets.resnet_discriminator(reg, cfg, rf, torch.cat([labels, labels], 0), 0.8, 0.5, 0.5, rnd_d['u_pass1'])
    cost = hinge(1.0 - d[:B]).mean() + hinge(1.0 + d[B:]).mean() + tf_ops.sparse_softmax_ce(a[:B], labels).mean()
    margin = torch.cat([1.0 - d[:B], 1.0 + d[B:]]).detach().abs().min().item()
    return osteps.grads_of(cost, reg, 'Discriminator.'), margin


def _ref_g_grads(reg, cfg, rnd_g, samples):
    """fp64 generator gradients of oracle.steps.resnet_g_losses (two towers, -mean D + ACGAN_SCALE_G CE) with the critic's input gradient
    taken AT `samples` - the evaluation under test's own generator output - and carried back through the fp64 generator.  The critic is
    piecewise linear: its input gradient is piecewise constant in the samples, and an fp32 generator output (a few 1e-6 from the fp64 one
    after three blocks, batch norms and the softmax) now and then lands across a ReLU kink of the critic's 8x8 stage from the fp64 samples
    - then EVERY generator gradient differs by 1e-3 to 1e-2 although nothing is wrong (plain fp32 torch against fp64 torch, none of this
    project's code, shows it on 3 of 12 draw seeds).  Evaluated at the samples under test, the reference answers the question the test
    asks: are these the gradients of this step."""
    from oracle import nets as onets, tf_ops
    n = samples.shape[0] // 2
    xs, costs, outs = [], [], []
    for t in range(2):
        labels = (rnd_g['label_u'][t] * 10).to(torch.int32)
        outs.append(onets.resnet_generator(reg, cfg, n, labels, rnd_g['z'][t]))
        x = samples[t * n:(t + 1) * n].double().requires_grad_(True)
        d, _, a = onets.resnet_discriminator(reg, cfg, x, labels, 0.8, 0.5, 0.5, rnd_g['u'][t])
        costs.append((-d.mean() + 0.1 * tf_ops.sparse_softmax_ce(a, labels).mean()) / 2)
        xs.append(x)
    gx = torch.autograd.grad(sum(costs), xs)
    named = reg.trainable_with_name('Generator')
    gs = torch.autograd.grad(outs, [p for _, p in named], grad_outputs=list(gx), allow_unused=True)
    return {nm: g for (nm, _), g in zip(named, gs) if g is not None}


def _worst(got, want):
    """the largest per-tensor relative error.  A conv bias in front of a batch norm has gradient zero: its fp64 value is rounding noise
    (1e-17 of the others), no scale to measure against - such tensors (under 1e-9 of the largest gradient) must be as good as zero instead."""
    assert set(got) == set(want), set(got) ^ set(want)
    top = max(float(w.abs().max()) for w in want.values())
    worst = 0.0
    for n, w in want.items():
        if float(w.abs().max()) < 1e-9 * top:
            assert float(got[n].abs().max()) <= 1e-5 * top, n
        else:
            worst = max(worst, _rel_err(got[n], w))
    return worst


def test_eager_step_gradients_against_the_fp64_oracle(monkeypatch):
    """DIM 32, B 4, objective='hinge', both switches on, gamma = 0.5, injected draws: the critic's and the generator's parameter gradients on
    the device against the fp64 oracle with the fp64 block wired in, under the measured-ratio rule - the same step on the CPU stand-ins is
    evaluated against fp64 in the same way, and the device's largest relative error (per tensor, relative to its largest magnitude) may be
    at most 4 x the stand-ins'.  Each evaluation's reference is taken at that evaluation's own generator output (_ref_g_grads, _ref_d_grads):
    the critic's input gradient is piecewise constant, so a reference at the fp64 samples differs by 1e-3 to 1e-2 in every tensor whenever an
    fp32 sample lies across a ReLU kink from its fp64 value - as it did here on the device (4.6e-3 against 7.6e-6) with nothing wrong."""
    import ctgan_amd.gan_cifar_resnet as R
    import ctgan_amd.kernels as K
    import ctgan_amd.tflib as lib
    from oracle import steps as osteps
    from tests import cpu_kernels as C
    from tests import hinge_cpu_kernels as HK
    from tests import hinge_step_checks as HC
    kw = dict(ATTENTION_G=True, ATTENTION_D=True)
    g = torch.Generator().manual_seed(11)
    real = torch.randint(0, 256, (BS, 3072), generator=g, dtype=torch.int32)
    labels = torch.randint(0, 10, (BS,), generator=g, dtype=torch.int32)
    rnd_d, rnd_g = osteps.make_rnd_resnet_d(BS, DIM, g), osteps.make_rnd_resnet_g(BS, DIM, g)
    try:
        with monkeypatch.context() as m:              # the same step on the fp32 CPU stand-ins
            for mod in (C, HK, AK):
                for name in mod.__all__:
                    m.setattr(K, name, getattr(mod, name))
            _build(R, lib, 'cpu', **kw)
            cpu = _step_grads(R, lib, 'cpu', real, labels, rnd_d, rnd_g)
        _build(R, lib, 'cuda', **kw)
        reg = HC.oracle_from_product(lib)
        dev = _step_grads(R, lib, 'cuda', real, labels, rnd_d, rnd_g)
    finally:
        lib.delete_all_params(); lib.set_device(None); R.configure()
    _wire_oracle(monkeypatch, reg)
    cfg = HC.oracle_cfg(DIM, HC.HEADS['acgan'])
    # the generator itself against fp64: both evaluations' outputs are the fp64 generator's to 1e-4 of tanh's unit range - fp32 (6e-8)
    # through some 25 chained operators, three batch norms and a softmax over scores of up to 50; a wrong sample is off by 0.1
    with torch.no_grad():
        ref_fake = HC.ref_d_losses(reg, cfg, real, labels, rnd_d, BS)['fake']
        ref_samples = torch.cat(osteps.resnet_g_losses(reg, cfg, rnd_g, B=BS)['samples'], 0)
    err = {}
    for who, (got_d, got_g, fake, samples) in (('device', dev), ('stand-ins', cpu)):
        for what, x, r in (('fake', fake, ref_fake), ('samples', samples, ref_samples)):
            e = float((x.double() - r).abs().max())
            print('step %s %s: largest error %.3e' % (who, what, e))
            assert e <= 1e-4, (who, what, e)
        want_d, margin = _ref_d_grads(reg, cfg, real, labels, rnd_d, fake)
        assert margin >= 1e-4, ('a hinge within 1e-4 of its kink', who, margin)
        want_g = _ref_g_grads(reg, cfg, rnd_g, samples)
        assert all(n in want_d for n in ('Discriminator.Attention.gamma', 'Discriminator.Attention.Query.Filters'))
        assert all(n in want_g for n in ('Generator.Attention.gamma', 'Generator.Attention.Out.Filters'))
        err[who] = {'critic': _worst(got_d, want_d), 'generator': _worst(got_g, want_g)}
    for what in ('critic', 'generator'):
        e_dev, e_cpu = err['device'][what], err['stand-ins'][what]
        print('step gradients %s: device %.3e  stand-ins %.3e  ratio %.2f' % (what, e_dev, e_cpu, e_dev / max(e_cpu, 1e-30)))
        assert e_cpu < 1e-3, (what, e_cpu)            # the stand-ins follow the oracle: the wiring is right
        assert e_dev <= RATIO * e_cpu, (what, e_dev, e_cpu)


def _run(graphs, iters, cfg_kw, **trainer_kw):
    import ctgan_amd.gan_cifar_resnet as R
    import ctgan_amd.tflib as lib
    from ctgan_amd.engine import GraphedTrainer
    nrng = np.random.default_rng(1234)
    batches = [(torch.from_numpy(nrng.integers(0, 256, (BS, 3072), dtype=np.int32)).cuda(),
                torch.from_numpy(nrng.integers(0, 10, (BS,), dtype=np.int32)).cuda()) for _ in range(8)]
    try:
        _build(R, lib, 'cuda', seed=0, **cfg_kw)
        tr = R.Trainer(seed=2024, **trainer_kw)
        eng = GraphedTrainer(tr, use_graphs=graphs)
        assert eng.graphed == graphs, eng.graph_error
        cur = [0]

        def nb():
            cur[0] += 1
            return batches[cur[0] % len(batches)]
        for it in range(iters):
            eng.train_iteration(it, nb)
        torch.cuda.synchronize()
        return tr.d_opt.theta.clone(), tr.g_opt.theta.clone(), {n: lib._params[n].detach().clone() for n in GATES if n in lib._params}
    finally:
        lib.delete_all_params(); R.configure()


def test_graph_replay_equals_eager_hinge_both_switches():
    """two graph-replayed train_iterations and two eager ones: every weight bit-identical; both gates have moved (they are read on the device)"""
    kw = dict(ATTENTION_G=True, ATTENTION_D=True)
    g, e = _run(True, 2, kw, objective='hinge'), _run(False, 2, kw, objective='hinge')
    assert torch.equal(g[0], e[0]) and torch.equal(g[1], e[1])
    assert set(g[2]) == set(GATES)
    for n in GATES:
        assert torch.equal(g[2][n], e[2][n]) and float(g[2][n]) != 0.5 and torch.isfinite(g[2][n]).all(), n


def test_graph_replay_equals_eager_ct_step_with_generator_attention():
    """Trainer(objective=None): the hand-scheduled CT critic step next to a generator with the block, graph against eager"""
    kw = dict(ATTENTION_G=True)
    g, e = _run(True, 2, kw), _run(False, 2, kw)
    assert torch.equal(g[0], e[0]) and torch.equal(g[1], e[1])
    assert set(g[2]) == {GATES[0]} and torch.equal(g[2][GATES[0]], e[2][GATES[0]]) and float(g[2][GATES[0]]) != 0.5
