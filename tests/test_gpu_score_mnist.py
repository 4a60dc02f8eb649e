"""The kernels and steps of the self-trained MNIST score classifier on the device (csrc/score.hip, the moving-statistics / blend /
fused-apply entry points of csrc/bn.hip, ctgan_amd.score_mnist, engine.GraphedScoreTrainer) against fp64 (tests/score_oracle.py,
oracle/).  Runs on the MI355X box only (`-m gpu`).

Bounds.  ELU: relerr 1e-6 (as test_gpu_kernels.test_elementwise holds tanh / sigmoid to).  Batch norm: test_gpu_kernels.test_batchnorm's -
2e-5 forward, 1e-4 gradients - and 1e-6 for the moving statistics.  Convs: test_conv_fwd_dgrad_wgrad's - 2e-5 forward and data
gradient, 3e-5 weight gradient.  Step: tests/ssl_cifar_oracle.run_steps's - scalars within 2e-4 max(1, |ref|), gradients within
relative L2 max(3e-3, 3 x the oracle's fp32 twin), updates by ssl_oracle.update_ok.
Fused epilogue against the unfused composition: the operation ORDER is the same (bn_apply's expression, then shortcut + 0.3 * it, then
ELU), but whether a multiply-add pair contracts into one FMA is the compiler's choice per kernel, so the forward is held to the 2e-5
bound, not to bit equality; the backward folds 0.3 into the reduced totals instead of scaling the gradient first - another order - and
is held to the 1e-4 gradient bound."""
import collections

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import np_conv, tf_ops  # noqa: E402
from tests import score_oracle as O  # noqa: E402
from tests.ssl_oracle import update_ok  # noqa: E402

COST_TOL, GRAD_TOL = 2e-4, 3e-3


def dev(t):
    return t.to('cuda')


def cl(t):
    d = t.to('cuda')
    out = torch.empty((d.shape[0], d.shape[2], d.shape[3], d.shape[1]), device='cuda', dtype=d.dtype).permute(0, 3, 1, 2)
    out.copy_(d)
    return out


def relerr(a, b):
    a = a.detach().cpu().double(); b = b.detach().cpu().double()
    e = ((a - b).abs().max() / b.abs().max().clamp_min(1e-30)).item()
    print('relerr %.3g' % e)
    return e


@pytest.fixture
def clean():
    import ctgan_amd.score_mnist as M
    import ctgan_amd.tflib as lib
    lib.delete_all_params()
    yield M
    M.configure()
    lib.delete_all_params()


# ----------------------------------------------------------------------------------------------------- ELU
@pytest.mark.parametrize('n', [1, 3, 4, 5, 1023, 4 * 256 * 3 + 1])
def test_elu(n):
    """Vector body and scalar tail (n = 4k + r), fewer elements than one vector, more than one workgroup; 0, +-1e-8, -100, +50."""
    import ctgan_amd.kernels as K
    g = torch.Generator().manual_seed(n)
    special = torch.tensor([1e-8, -100.0, 0.0, -1e-8, 50.0])     # (n = 1 takes the first: at -100 alone the true gradient, e^-100, is below fp32)
    x = torch.randn(n, generator=g) * 3
    x[:min(n, 5)] = special[:min(n, 5)]
    if n >= 1023:
        x[-5:] = special                      # in the tail / last vector too
    gy, add = torch.randn(n, generator=g), torch.randn(n, generator=g)
    xd = x.double()
    ref = torch.where(xd > 0, xd, torch.expm1(xd))
    dref = torch.where(xd > 0, torch.ones_like(xd), torch.exp(xd))
    y = K.elu_fwd(dev(x))
    assert relerr(y, ref) < 1e-6
    assert torch.equal(y.cpu()[x > 0], x[x > 0])
    assert relerr(K.elu_bwd(dev(gy), y), gy.double() * dref) < 1e-6
    assert relerr(K.elu_bwd(dev(gy), y, dev(add)), add.double() + gy.double() * dref) < 1e-6
    # an unaligned view takes the scalar path
    if n > 4:
        assert torch.equal(K.elu_fwd(dev(x)[1:]), y[1:])


def test_elu_autograd_and_layouts():
    import ctgan_amd.functional as F
    g = torch.Generator().manual_seed(1)
    x = torch.randn(3, 8, 5, 5, generator=g)
    xd = cl(x).requires_grad_(True)
    y = F.elu(xd)
    gy = torch.randn(3, 8, 5, 5, generator=g)
    (gx,) = torch.autograd.grad(y, xd, dev(gy))             # an NCHW cotangent for a channels-last output
    xr = x.double().requires_grad_(True)
    (gr,) = torch.autograd.grad(O.elu(xr), xr, gy.double())
    assert relerr(y, O.elu(x.double())) < 1e-6 and relerr(gx, gr) < 1e-6


# ----------------------------------------------------------------------------------------------------- batch norm
BN_SHAPES = [(1, 32, 7, False), (5, 64, 7, False), (3, 40, 1, False), (2, 200, 14, False), (2, 32, 6, True), (130, 32, 28, False)]


@pytest.mark.parametrize('n,c,h,const', BN_SHAPES, ids=lambda v: str(v))
@pytest.mark.parametrize('it', [0, 999])
def test_moving_update_and_blend(n, c, h, const, it):
    """(1,32,7): B = 1.  (3,40,1): h*w = 1, every per-sample variance 0, c no multiple of 64 - the scalar kernels.  (2,32,6) const: one
    constant plane per sample and moving_variance = 0 - the blended variance is exactly 0 there.  (130,32,28): 256-position chunks."""
    import ctgan_amd.kernels as K
    g = torch.Generator().manual_seed(n + c + it)
    x = torch.randn(n, c, h, h, generator=g) * 2 + 3.0
    if const:
        x[:, 1] = 3.25
    scale, offset = torch.rand(c, generator=g) + 0.5, torch.randn(c, generator=g)
    mm0, mv0 = torch.randn(c, generator=g), (torch.zeros(c) if const else torch.rand(c, generator=g) + 0.5)
    gy = torch.randn(n, c, h, h, generator=g)
    xr = x.double().requires_grad_(True); sr = scale.double().requires_grad_(True); orr = offset.double().requires_grad_(True)
    ref, bm, bv = O.bn_training(xr, sr, orr)
    alpha = 0.3
    gr = torch.autograd.grad(ref, [xr, sr, orr], alpha * gy.double())
    mm, mv, itd = dev(mm0.clone()), dev(mv0.clone()), K.device_scalar(it, 'cuda')
    mean, rstd, x4 = K.bn_stats_moving(cl(x), 1e-5, mm, mv, itd)
    y, _ = K.bn_apply_ex(x4, mean, rstd, dev(scale), dev(offset))
    assert relerr(y, ref) < 2e-5
    want_mm, want_mv = O.moving_update(mm0.double(), bm.detach(), it), O.moving_update(mv0.double(), bv.detach(), it)
    assert (mm.cpu().double() - want_mm).abs().max().item() <= 1e-6 * max(1.0, want_mm.abs().max().item())
    assert (mv.cpu().double() - want_mv).abs().max().item() <= 1e-6 * max(1.0, want_mv.abs().max().item())
    gx, gs, go = K.bn_bwd_scaled(cl(gy), x4, mean, rstd, dev(scale), dev(offset), alpha)
    if n * h * h > 1:
        assert relerr(gx, gr[0]) < 1e-4 and relerr(gs.reshape(-1), gr[1]) < 1e-4
    assert relerr(go.reshape(-1), gr[2]) < 1e-4
    # statistics only: nothing moves
    K.bn_stats_moving(cl(x), 1e-5)
    assert (mm.cpu().double() - want_mm).abs().max().item() <= 1e-6 * max(1.0, want_mm.abs().max().item())
    # the blend, from the moved statistics
    bmean, brstd, x4 = K.bn_blend_stats(cl(x), mm, mv)
    z, _ = K.bn_apply_ex(x4, bmean, brstd, dev(scale), dev(offset))
    zref = O.bn_blend(x.double(), scale.double(), offset.double(), mm.cpu().double(), mv.cpu().double())
    assert relerr(z, zref) < 2e-5
    if const:
        want = 1.0 / np.sqrt(1e-5)                       # variance exactly 0: rstd = eps^-1/2, nothing lost to cancellation
        assert (brstd[:, 1].cpu().double() - want).abs().max().item() <= 1e-6 * want


@pytest.mark.parametrize('n,c,h', [(5, 64, 7), (3, 40, 3), (6, 32, 14)])
@pytest.mark.parametrize('training', [True, False])
def test_fused_epilogue_against_the_unfused_composition(monkeypatch, n, c, h, training):
    """shortcut + 0.3 bn(x) and its ELU in one pass against bn_apply_ex, F.add and ELU (CTGAN_SCORE_FUSED=0) and against fp64; the
    training backward with both cotangents (module docstring: 2e-5 forward, 1e-4 gradients - not bit equality)."""
    import ctgan_amd.functional as F
    import ctgan_amd.kernels as K
    g = torch.Generator().manual_seed(n + c)
    x = torch.randn(n, c, h, h, generator=g) * 2 + 3.0
    sc = torch.randn(n, c, h, h, generator=g)
    scale, offset = torch.rand(c, generator=g) + 0.5, torch.randn(c, generator=g)
    mm0, mv0 = torch.randn(c, generator=g), torch.rand(c, generator=g) + 0.5
    gs_, ge_ = torch.randn(n, c, h, h, generator=g), torch.randn(n, c, h, h, generator=g)
    leaves = [t.double().requires_grad_(True) for t in (x, scale, offset, sc)]
    if training:
        bn = O.bn_training(leaves[0], leaves[1], leaves[2])[0]
    else:
        bn = O.bn_blend(leaves[0], leaves[1], leaves[2], mm0.double(), mv0.double())
    s_ref = leaves[3] + 0.3 * bn
    e_ref = O.elu(s_ref)
    outs = {}
    for fused in (True, False):
        monkeypatch.setattr(F, 'SCORE_FUSED', fused)
        xd, scd = cl(x).requires_grad_(training), cl(sc).requires_grad_(training)
        sd, od = dev(scale).requires_grad_(training), dev(offset).requires_grad_(training)
        mm, mv = dev(mm0.clone()), dev(mv0.clone())
        if training:
            s, e = F.batch_norm_moving(xd, sd, od, (mm, mv, K.device_scalar(0, 'cuda')), shortcut=scd, alpha=0.3, want_elu=True)
            grads = torch.autograd.grad([s, e], [xd, sd, od, scd], [cl(gs_), cl(ge_)])
        else:
            with torch.no_grad():
                s, e = F.batch_norm_blend(xd, sd, od, mm, mv, shortcut=scd, alpha=0.3, want_elu=True)
            grads = ()
        outs[fused] = (s, e) + tuple(grads) + (mm, mv)
        assert relerr(s, s_ref) < 2e-5 and relerr(e, e_ref) < 2e-5
    for a, b in zip(outs[True][:2], outs[False][:2]):
        assert relerr(a, b) < 2e-5
    assert torch.equal(outs[True][-1], outs[False][-1]) and torch.equal(outs[True][-2], outs[False][-2])      # the same statistics launch
    if training:
        ref = torch.autograd.grad([s_ref, e_ref], leaves, [gs_.double(), ge_.double()], retain_graph=True)
        for k in range(4):
            assert relerr(outs[True][2 + k], ref[k]) < 1e-4 and relerr(outs[False][2 + k], ref[k]) < 1e-4
            assert relerr(outs[True][2 + k], outs[False][2 + k]) < 1e-4
        # one cotangent missing: the s-only and the e-only paths
        xd, scd = cl(x).requires_grad_(True), cl(sc).requires_grad_(True)
        monkeypatch.setattr(F, 'SCORE_FUSED', True)
        s, e = F.batch_norm_moving(xd, dev(scale), dev(offset), None, shortcut=scd, alpha=0.3, want_elu=True)
        (gx_s,) = torch.autograd.grad(s, xd, cl(gs_), retain_graph=True)
        (gx_e,) = torch.autograd.grad(e, xd, cl(ge_))
        r_s = torch.autograd.grad(s_ref, leaves[0], gs_.double(), retain_graph=True)[0]
        r_e = torch.autograd.grad(e_ref, leaves[0], ge_.double(), retain_graph=True)[0]
        assert relerr(gx_s, r_s) < 1e-4 and relerr(gx_e, r_e) < 1e-4


# ----------------------------------------------------------------------------------------------------- global norm, clip
@pytest.mark.parametrize('n', [1, 255, 143001])
def test_global_norm_and_clip(n):
    import ctgan_amd.kernels as K
    g = torch.Generator().manual_seed(n)
    x = torch.randn(n, generator=g) * (3.0 if n > 1 else 1.0) + (2.0 if n == 1 else 0.0)
    ref = x.double().norm().item()
    a, b = K.global_norm(dev(x)), K.global_norm(dev(x).clone())
    assert torch.equal(a, b)                                        # fixed-order reduction: the same bits on every run
    assert abs(a.item() - ref) <= 1e-6 * ref
    for clip in (0.5 * ref, 2.0 * ref):                             # norm above and below the clip
        xd = dev(x).clone()
        K.clip_by_norm_(xd, a, clip)
        want = x.double() * (clip / max(ref, clip))
        assert relerr(xd, want) < 1e-6
        if clip > ref:
            assert torch.equal(xd.cpu(), x)                          # factor exactly 1
        xe = dev(x).clone()
        K.clip_by_norm_(xe, a, clip)
        assert torch.equal(xd, xe)
    # an unaligned bucket slice: the scalar path gives the same norm
    if n > 4:
        y = torch.zeros(n + 1)
        y[1:] = x
        c = K.global_norm(dev(y)[1:])
        assert abs(c.item() - ref) <= 1e-6 * ref


# ----------------------------------------------------------------------------------------------------- the conv geometries
CONVS = [(32, 28, 32, 3, 2), (32, 14, 64, 3, 2), (32, 28, 32, 1, 2), (32, 14, 64, 1, 2), (1, 28, 32, 3, 1), (32, 14, 32, 3, 1), (64, 7, 64, 3, 1)]


@pytest.mark.parametrize('C,H,Ko,k,st', CONVS, ids=lambda v: str(v))
def test_conv_geometries_of_the_network(C, H, Ko, k, st):
    """The stride-2 3x3 and 1x1 convs and the one-channel first layer this network adds (and its two stride-1 3x3 shapes), through
    F.conv2d at N = 3: forward against oracle/np_conv.py, data and weight gradients against autograd of oracle/tf_ops.py in fp64."""
    import ctgan_amd.functional as F
    N = 3
    g = torch.Generator().manual_seed(C + H + Ko + k)
    x = torch.randn(N, C, H, H, generator=g)
    w = torch.randn(k, k, C, Ko, generator=g) / np.sqrt(k * k * C)
    b = torch.randn(Ko, generator=g)
    ref = np_conv.conv2d_same_np(x.numpy(), w.numpy(), st) + b.double().numpy()[None, :, None, None]
    xd, wd, bd = cl(x).requires_grad_(True), dev(w).requires_grad_(True), dev(b).requires_grad_(True)
    y = F.conv2d(xd, wd, bd, stride=st)
    assert tuple(y.shape) == ref.shape and relerr(y, torch.from_numpy(ref)) < 2e-5
    gy = torch.randn(ref.shape, generator=g)
    gx, gw, gb = torch.autograd.grad(y, [xd, wd, bd], cl(gy))
    x_, w_ = x.double().requires_grad_(True), w.double().requires_grad_(True)
    rx, rw = torch.autograd.grad(tf_ops.conv2d_same(x_, w_, st), [x_, w_], gy.double())
    assert relerr(gx, rx) < 2e-5 and relerr(gw, rw) < 3e-5
    gb_scale = gy.double().abs().sum(dim=(0, 2, 3)).max().item()
    assert (gb.cpu().double() - gy.double().sum(dim=(0, 2, 3))).abs().max().item() < 1e-6 * gb_scale


# ----------------------------------------------------------------------------------------------------- steps
def _trainer_from(M, P):
    import ctgan_amd.tflib as lib
    lib.delete_all_params(); lib.set_seed(4)
    tr = M.ScoreTrainer()
    lib.load_state_dict(collections.OrderedDict((n, v.float()) for n, v in P.items()), strict=True)
    assert [n for n in lib._params] == list(P)
    return tr


@pytest.mark.parametrize('fused', [True, False])
def test_one_step_matches_the_oracle(clean, monkeypatch, fused):
    """One train step at B = 6, the script's widths, from random weights, against the fp64 oracle (module docstring for the bounds);
    the fused epilogue and the unfused composition both."""
    import ctgan_amd.functional as F
    import ctgan_amd.tflib as lib
    M = clean
    monkeypatch.setattr(F, 'SCORE_FUSED', fused)
    M.configure(BATCH_SIZE=6)
    P = O.make_params(seed=0)
    x, y = O.step_inputs(6, 1)
    ref = O.train_step(P, O.zero_slots(P), 1, x.double(), y)
    P32 = collections.OrderedDict((n, v.float()) for n, v in P.items())
    twin = O.train_step(P32, O.zero_slots(P32), 1, x, y)
    assert O.top2_gap(ref['logits']) > 1e-3
    tr = _trainer_from(M, P)
    tr.opt.set_lr(M.cfg.LR)
    tr.stats_iter.fill_(0)
    out = tr.losses(dev(x), dev(y))
    grads = torch.autograd.grad(out['cost'], tr.params, allow_unused=True)
    gradnorm = tr.opt.update_clipped(grads, M.cfg.CLIP_NORM)
    for k, a in (('cost', out['cost'].item()), ('acc', out['acc'].item()), ('gradnorm', gradnorm.item())):
        b = float(ref[k])
        print(k, a, b)
        assert abs(a - b) <= COST_TOL * max(1.0, abs(b)), (k, a, b)
    names = [n for n in P if not O.is_moving(n)]
    assert [n for n, _ in tr.named] == names
    gp = {n: g.detach().cpu() for n, g in zip(names, grads)}
    factor = 5. / max(ref['gradnorm'], 5.)
    for n in names:
        tol = max(GRAD_TOL, 3 * O.rel_l2(twin['grads'][n], ref['grads'][n]))
        e = O.rel_l2(gp[n], ref['grads'][n])
        print('grad', n, 'rel L2 %.3g' % e, 'bound %.3g' % tol)
        assert (gp[n].double() - ref['grads'][n]).norm().item() <= tol * ref['grads'][n].norm().item() + 2e-6, (n, e, tol)
    for n in P:
        new = lib._params[n].detach().cpu().double()
        if O.is_moving(n):
            assert (new - ref['P'][n]).abs().max().item() <= 1e-6 * max(1.0, ref['P'][n].abs().max().item()), n
        else:
            ok, how = update_ok(new, P[n], ref['P'][n], ref['grads'][n] * factor, gp[n] * factor)
            assert ok, ('update', n, how)


def _state(tr):
    import ctgan_amd.tflib as lib
    s = {'p/' + n: p.detach().clone() for n, p in lib._params.items()}
    for i, b in enumerate(tr.opt.slots()):
        s['slot%d' % i] = b.clone()
    s['t'] = torch.tensor(tr.opt.t)
    return s


def test_graph_replay_equals_eager_then_stats_passes_and_evaluate(clean):
    """Three train steps and three statistics passes at B = 6: graph replay equals eager bit for bit - weights, Adam's slots, moving
    statistics, outputs.  Then evaluate on 5 rows against the oracle run from the product's weights."""
    from ctgan_amd.engine import GraphedScoreTrainer
    import ctgan_amd.tflib as lib
    M = clean
    M.configure(BATCH_SIZE=6)
    P = O.make_params(seed=3)
    batches = [O.step_inputs(6, 40 + k) for k in range(6)]
    runs = {}
    for graphed in (False, True):
        tr = _trainer_from(M, P)
        eng = GraphedScoreTrainer(tr, use_graphs=graphed)
        assert eng.graphed == graphed, eng.graph_error
        outs = []
        for k in range(3):
            outs.append(torch.stack([t.clone().reshape(()) for t in eng.step(*batches[k])]))
        mid = _state(tr)
        for i in range(3):
            eng.bn_stats_pass(batches[3 + i][0], i)
        runs[graphed] = (outs, mid, _state(tr))
        assert tr.opt.skipped() == 0 and tr.iteration == 3 and tr.opt.t == 3
    for a, b in zip(runs[False][0], runs[True][0]):
        print('eager', a.tolist(), 'graph', b.tolist())
        assert torch.isfinite(a).all() and torch.equal(a, b)
    for which in (1, 2):
        e, g = runs[False][which], runs[True][which]
        assert sorted(e) == sorted(g)
        for n in e:
            assert torch.equal(e[n], g[n]), ('graph replay differs from eager', which, n)
    assert not all(torch.equal(runs[True][1][n], runs[True][2][n]) for n in runs[True][1] if O.is_moving(n))      # the passes moved them
    for n in runs[True][1]:
        if not O.is_moving(n):
            assert torch.equal(runs[True][1][n], runs[True][2][n]), ('a statistics pass moved', n)
    # the moving statistics are the plain mean of the three batches' statistics: the oracle's passes from the trained weights
    Q = collections.OrderedDict((n, runs[True][1]['p/' + n].cpu().double()) for n in P)
    for i in range(3):
        Q = O.stats_pass(Q, batches[3 + i][0].double(), i)
    for n in P:
        if O.is_moving(n):
            assert (lib._params[n].detach().cpu().double() - Q[n]).abs().max().item() <= 1e-5 * max(1.0, Q[n].abs().max().item()), n
    x, y = O.step_inputs(5, 60)
    c, a, inc, logits = O.evaluate(Q, x.double(), y)
    assert O.top2_gap(logits) > 1e-3
    got = tr.evaluate(x, y)
    print(got, (c, a, inc))
    assert abs(got[0] - c) <= COST_TOL * max(1, abs(c)) and got[1] == a and abs(got[2] - inc) <= COST_TOL * inc


def test_short_train_under_graphs(clean):
    """train() on synthetic arrays: B = 20, a test pass every 3 iterations after 2 statistics passes, 6 iterations, graph replay."""
    M = clean
    M.configure(BATCH_SIZE=20, TEST_EVERY=3, BN_STATS_ITERS=2, STOP_AFTER=6)
    g = torch.Generator().manual_seed(0)
    mk = lambda: (torch.rand(20, 784, generator=g).numpy(), torch.randint(0, 10, (20,), generator=g).numpy())      # noqa: E731
    sets = [[mk() for _ in range(k)] for k in (4, 2, 1)]
    lines = []
    tr = M.train(tuple((lambda s=s: iter(s)) for s in sets), use_graphs=True, log=lines.append)
    assert tr.iteration == 6 and tr.opt.t == 6 and tr.opt.skipped() == 0
    tests = [ln for ln in lines if 'test cost' in ln]
    assert len(tests) == 2 and '\titeration:2\t' in tests[0] and '\titeration:5\t' in tests[1], lines
    assert len([ln for ln in lines if 'train cost' in ln]) == 6 and 'nan' not in ''.join(lines)
    print('\n'.join(lines))
