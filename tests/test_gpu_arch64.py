"""The 64x64 script's other architecture pairs on the MI355X: the folded BatchNorm + LeakyReLU / tanh / gate kernels and the gate on its own
(csrc/bn_act.hip) against fp64 built from oracle.tf_ops, the fused and the composed form of a layer on the same device inputs, critic and
generator steps of (ARCH, MODE) pairs against tests/arch64_oracle.py, hipGraph replay against the eager trainer, and the evaluator's
dev cost against the per-batch critic costs."""
import zlib

import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import tf_ops  # noqa: E402
from tests import arch64_oracle as AO  # noqa: E402
from tests import test_gan_modes_host as H  # noqa: E402

BOUND = 1e-4          # the project's bound for these reductions (tests/test_gpu_bn_paths.py): max-norm relative error
ACTS = ('lrelu', 'tanh', 'gate')
ALPHA = 0.2


def cl(t):
    d = t.to('cuda')
    out = torch.empty((d.shape[0], d.shape[2], d.shape[3], d.shape[1]), device='cuda', dtype=d.dtype).permute(0, 3, 1, 2)
    out.copy_(d)
    return out


def relerr(a, b):
    a = a.detach().cpu().double(); b = b.detach().cpu().double()
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-30)).item()


def _seed(*key):
    return zlib.crc32(repr(key).encode()) % 100000


def pre_act(x, scale, offset, groups, eps=1e-5):
    """fp64 z = batch norm of x [n,c,h,w] over (n,h,w) per statistic group (biased variance), scale / offset [c]."""
    per = x.shape[0] // groups
    outs = []
    for gi in range(groups):
        xs = x[gi * per:(gi + 1) * per]
        mean, var = tf_ops.moments(xs, [0, 2, 3])
        outs.append(tf_ops.batch_normalization(xs, mean, var, offset.view(1, -1, 1, 1), scale.view(1, -1, 1, 1), eps))
    return torch.cat(outs)


def activation(z, act):
    if act == 'lrelu':
        return tf_ops.leaky_relu(z, ALPHA)
    return torch.tanh(z) if act == 'tanh' else AO.gated(z)


def inputs(case, act):
    """x = randn * 2 + 3, scale = rand + 0.5, offset = randn, gy = randn, drawn on the CPU.  For 'lrelu' the elements whose fp64 z lies within
    2e-3 of the kink are moved away from it (a tenth of x's spread; the statistics barely move), until none is within 1e-3."""
    n, c, h, w, groups = case
    g = torch.Generator().manual_seed(_seed(case, act))
    x = torch.randn(n, c, h, w, generator=g) * 2 + 3.0
    scale = torch.rand(c, generator=g) + 0.5
    offset = torch.randn(c, generator=g)
    gy = torch.randn(n, c // 2 if act == 'gate' else c, h, w, generator=g)
    if act == 'lrelu':
        for _ in range(20):
            z = pre_act(x.double(), scale.double(), offset.double(), groups)
            bad = z.abs() < 2e-3
            if not bad.any():
                break
            x = torch.where(bad, x + torch.where(z >= 0, 0.2, -0.2).float(), x)
    return x, scale, offset, gy


def reference(x, scale, offset, gy, groups, act):
    xr, sr, orr = (t.double().requires_grad_(True) for t in (x, scale, offset))
    z = pre_act(xr, sr, orr, groups)
    y = activation(z, act)
    return y.detach(), z.detach(), torch.autograd.grad(y, [xr, sr, orr], gy.double())


# (n, c, h, w, groups)
CASES = [
    (4, 2, 4, 4, 1),          # one gated pair
    (6, 6, 5, 5, 2),          # scalar path, odd hw
    (4, 8, 4, 4, 1),
    (6, 72, 7, 9, 3),         # c > 64, not a multiple of 64
    (4, 128, 4, 4, 2),        # vector path at the hw = 16 of BN1
    (2, 256, 32, 32, 1),      # several position chunks per sample
    (8, 1024, 4, 4, 4),       # the gated BN1 width at DIM 32
]


def _check(K, x, scale, offset, gy, groups, act, two_d=False):
    ref_y, z, gr = reference(x, scale, offset, gy, groups, act)
    if act == 'lrelu':        # asserted BEFORE the device runs: a sign flip at the kink can neither mask nor fake an error
        assert (z.abs() >= 1e-3).all(), z.abs().min().item()
    if two_d:
        xin, gyin = x[:, :, 0, 0].contiguous().cuda(), gy[:, :, 0, 0].contiguous().cuda()
    else:
        xin, gyin = cl(x), cl(gy)
    y, mean, rstd, x4 = K.bn_act_fwd(xin, scale.cuda(), offset.cuda(), act, ALPHA, groups)
    assert y.dim() == (2 if two_d else 4) and x4.dim() == 4
    e = relerr(y.reshape(ref_y.shape), ref_y)
    print('bn_act_fwd %s y %.3g' % (act, e))
    assert e < BOUND, e
    gx, gs, go = K.bn_act_bwd(gyin, x4, mean, rstd, scale.cuda(), offset.cuda(), act, ALPHA, groups)
    torch.cuda.synchronize()
    es = relerr(gx.reshape(gr[0].shape), gr[0]), relerr(gs, gr[1]), relerr(go, gr[2])
    print('bn_act_bwd %s gx %.3g gscale %.3g goffset %.3g' % ((act,) + es))
    assert es[0] < BOUND and es[1] < BOUND and es[2] < BOUND, es


@pytest.mark.parametrize('act', ACTS)
@pytest.mark.parametrize('case', CASES, ids=lambda c: 'n%d_c%d_%dx%d_g%d' % c)
def test_bn_act_kernels_against_fp64(case, act):
    import ctgan_amd.kernels as K
    x, scale, offset, gy = inputs(case, act)
    _check(K, x, scale, offset, gy, case[4], act)


@pytest.mark.parametrize('act', ACTS)
@pytest.mark.parametrize('n,c,groups', [(8, 128, 2), (8, 6, 1)])
def test_bn_act_two_dimensional_input(n, c, groups, act):
    import ctgan_amd.kernels as K
    x, scale, offset, gy = inputs((n, c, 1, 1, groups), act)
    _check(K, x, scale, offset, gy, groups, act, two_d=True)


@pytest.mark.parametrize('shape', [(3, 6, 5, 5), (4, 8, 4, 4), (2, 256, 32, 32), (5, 10), (7, 2)], ids=str)
def test_standalone_gate_against_fp64(shape):
    import ctgan_amd.kernels as K
    g = torch.Generator().manual_seed(_seed('gate', shape))
    x = torch.randn(*shape, generator=g) * 2
    xr = x.double().requires_grad_(True)
    ref = AO.gated(xr)
    gy = torch.randn(ref.shape, generator=g)
    (gref,) = torch.autograd.grad(ref, xr, gy.double())
    xin, gyin = (cl(x), cl(gy)) if x.dim() == 4 else (x.cuda(), gy.cuda())
    y = K.gate_fwd(xin)
    gx = K.gate_bwd(gyin, xin)
    torch.cuda.synchronize()
    assert tuple(y.shape) == tuple(ref.shape) and tuple(gx.shape) == tuple(x.shape)
    es = relerr(y, ref), relerr(gx, gref)
    print('gate %s y %.3g gx %.3g' % ((shape,) + es))
    assert es[0] < BOUND and es[1] < BOUND, es


@pytest.mark.parametrize('act', ACTS)
@pytest.mark.parametrize('case', [(6, 6, 5, 5, 2), (4, 128, 4, 4, 2), (6, 72, 7, 9, 3)], ids=lambda c: 'n%d_c%d_%dx%d_g%d' % c)
def test_fused_and_composed_layer_on_the_same_inputs(monkeypatch, case, act):
    """functional.batch_norm_act with CTGAN_BN_ACT_FUSED on and off (F.BN_ACT_FUSED), through autograd: both within the bound of fp64."""
    import ctgan_amd.functional as F
    x, scale, offset, gy = inputs(case, act)
    ref_y, z, gr = reference(x, scale, offset, gy, case[4], act)
    if act == 'lrelu':
        assert (z.abs() >= 1e-3).all()
    xd, sd, od = (t.requires_grad_(True) for t in (cl(x), scale.cuda(), offset.cuda()))
    gyd = cl(gy)
    for fused in (True, False):
        monkeypatch.setattr(F, 'BN_ACT_FUSED', fused)
        y = F.batch_norm_act(xd, sd, od, act, ALPHA, groups=case[4])
        gx, gs, go = torch.autograd.grad(y, [xd, sd, od], gyd)
        torch.cuda.synchronize()
        es = relerr(y, ref_y), relerr(gx, gr[0]), relerr(gs, gr[1]), relerr(go, gr[2])
        print('%s %s: y %.3g gx %.3g gscale %.3g goffset %.3g' % (('fused' if fused else 'composed', act) + es))
        assert max(es) < BOUND, (fused, es)
    monkeypatch.setattr(F, 'BN_ACT_FUSED', True)
    with pytest.raises(RuntimeError, match='first order only'):
        torch.autograd.grad(F.batch_norm_act(xd, sd, od, act, ALPHA, groups=case[4]).sum(), xd, create_graph=True)


# ----------------------------------------------------------------------------- steps against the oracle
PAIRS = [('dcgan', 'dcgan'), ('dcgan', 'wgan'), ('dcgan-nobn', 'lsgan'), ('dcgan-tanh', 'dcgan'), ('multiplicative', 'wgan'),
         ('wganpaper', 'wgan'), ('fc', 'lsgan')]


@pytest.mark.parametrize('arch,mode', PAIRS)
def test_arch_steps_against_oracle(monkeypatch, arch, mode):
    """The rule of test_mode_steps_against_oracle for 64x64 at DIM 16, B 6: cost 2e-4, per-parameter gradients in relative L2 against
    max(5e-3 critic / 2e-2 generator, 3 x the fp32 twin's error), every parameter after the update against the oracle's optimizer (+ clip;
    the moving statistics bit for bit).  MODE 'wgan': every critic weight and moving statistic of the product ends inside the clip."""
    import ctgan_amd.tflib as lib
    lib.delete_all_params(); lib.set_device(None)
    monkeypatch.setattr(H, 'mode_setup', AO.setup)
    clipped = []
    orig = H.O.clip_critic

    def clip_and_look(reg, bound=0.01):
        orig(reg, bound)
        b32 = torch.tensor(bound, dtype=torch.float32).item()
        names = [n for n, _ in lib.named_params_with_name('Discriminator')]
        assert any(n in lib._non_trainable for n in names) and any(n.endswith('.Filters') for n in names)
        for n, p in lib.named_params_with_name('Discriminator'):
            assert float(p.detach().abs().max()) <= b32, n
        clipped.append(len(names))
    monkeypatch.setattr(H.O, 'clip_critic', clip_and_look)
    assert H.run_mode_steps(lib, arch, mode, 16, 6, 'cuda', cost_tol=2e-4, grad_tol=5e-3, g_grad_tol=2e-2, twin=True) > 0
    assert bool(clipped) == (mode == 'wgan')


@pytest.mark.parametrize('arch,mode', [('dcgan', 'dcgan'), ('multiplicative', 'wgan')])
def test_graphed_arch_trainer_equals_eager(arch, mode):
    """engine.GraphedDCGANTrainer against the eager DCGANTrainer, as test_graphed_mode_trainer_equals_eager: DIM 32, B 4, three iterations -
    same costs, bit-identical flat weights and non-trainable statistics, the same Philox counter."""
    import numpy as np
    import ctgan_amd.gan_64x64 as M
    import ctgan_amd.tflib as lib
    from ctgan_amd.dcgan_step import DCGANTrainer
    from ctgan_amd.engine import GraphedDCGANTrainer
    dim, B = 32, 4
    nrng = np.random.default_rng(5)
    batches = [torch.from_numpy(nrng.integers(0, 256, (B, 64 * 64 * 3), dtype=np.int32)).cuda() for _ in range(4)]

    def run(graphs):
        lib.delete_all_params(); lib.set_device(None); lib.set_seed(3)
        M.configure(MODE=mode, ARCH=arch, DIM=dim, BATCH_SIZE=B)
        M.build_params('cuda')
        tr = DCGANTrainer(M, seed=11)
        eng = GraphedDCGANTrainer(tr, (B, M.cfg.OUTPUT_DIM), batches[0].dtype, use_graphs=graphs)
        assert eng.graphed == graphs, eng.graph_error
        k = [0]

        def nb():
            k[0] += 1
            return batches[k[0] % len(batches)]
        costs = [float(eng.train_iteration(it, nb)['cost'].item()) for it in range(3)]
        return costs, tr.d_opt.theta.clone(), tr.g_opt.theta.clone(), int(tr.rng.ctr.item()), tr.disc_iters, \
            {n: p.detach().clone() for n, p in lib._params.items() if n in lib._non_trainable}
    try:
        g = run(True)
        e = run(False)
        assert g[4] == e[4] == (5 if mode == 'wgan' else 1)
        assert g[3] == e[3] == 3 * (g[4] + 1) + 2
        for a, b in zip(g[0], e[0]):
            assert abs(a) < 1e4 and abs(a - b) <= 1e-5 * max(1.0, abs(b)), (a, b)
        assert torch.equal(g[1], e[1]) and torch.equal(g[2], e[2])
        assert g[5] and g[5].keys() == e[5].keys()
        for n in g[5]:
            assert torch.equal(g[5][n], e[5][n]), n
        if mode == 'wgan':
            assert g[1].abs().max().item() <= 0.01
            assert all(t.abs().max().item() <= 0.01 for n, t in g[5].items() if n.startswith('Discriminator'))
    finally:
        lib.delete_all_params(); M.configure()


def test_dev_cost_is_the_mean_of_the_batch_costs():
    """Evaluator.dev_cost for ('dcgan', 'lsgan') over four dev batches at width 2 (two batches per pass, each critic call its own statistic
    group) against the mean of DCGANTrainer.d_losses on the same injected draws, to tests/eval_helpers.close; the training Philox counter
    stays where it was."""
    import ctgan_amd.gan_64x64 as M
    import ctgan_amd.tflib as lib
    from oracle import steps as osteps
    from ctgan_amd.dcgan_step import DCGANTrainer
    from ctgan_amd.evaluate import Evaluator
    from tests import eval_helpers as EH
    dim, B = 16, 4
    g = torch.Generator().manual_seed(8)
    try:
        lib.delete_all_params(); lib.set_device(None); lib.set_seed(2)
        M.configure(MODE='lsgan', ARCH='dcgan', DIM=dim, BATCH_SIZE=B)
        M.build_params('cuda')
        tr = DCGANTrainer(M, seed=5)
        batches = [torch.randint(0, 256, (B, 64 * 64 * 3), generator=g, dtype=torch.int32).cuda() for _ in range(4)]
        rnds = [EH.f32_rnd(osteps.make_rnd_dcgan_d(B, M.feat_shapes(), g), 'cuda') for _ in range(4)]
        c0 = int(tr.rng.ctr.item())
        with torch.no_grad():
            want = sum(float(tr.d_losses(b, r)['cost'].item()) for b, r in zip(batches, rnds)) / 4
        assert int(tr.rng.ctr.item()) == c0
        out = Evaluator(tr, width=2).dev_cost(iter(batches), rnd=rnds)
        print('dcgan / lsgan DIM %d: dev_cost %.9g, mean of the batch costs %.9g' % (dim, out['dev_cost'], want))
        assert out['n_batches'] == 4
        EH.close(out['dev_cost'], want, 'dcgan lsgan width 2')
        ev = Evaluator(tr, width=2)
        a = ev.dev_cost(iter(batches))                       # the default path: in-kernel draws from the evaluator's own stream
        assert a['dev_cost'] == a['dev_cost'] and abs(a['dev_cost']) < 1e6
        assert int(tr.rng.ctr.item()) == c0
    finally:
        lib.delete_all_params(); M.configure()
