"""The convolutional semi-supervised CT classifier on the MI355X (`-m gpu`): every kernel of csrc/ssl_conv.hip against fp64 (the
augmenting gather bit for bit), the generator's batch norm through bn.hip, the conv / transposed-conv routes at the network's layer
geometries against Theano's geometry in fp64, init + one classifier step + one generator step at reduced sizes against the oracle
(tests/ssl_cifar_oracle.py) on shared Philox streams and pinned to tests/golden/ssl_cifar_step.npz, full-size graph replay against
eager and a resumed run against an uninterrupted one bit for bit, a short graphed loop on synthetic data against the oracle's, and
train() on arrays.  Kernel bounds are the project's own (tests/test_gpu_ssl.py, tests/test_gpu_kernels.py): max |error| / max
|reference| below 2e-5 for forward results and 3e-5 for gradients."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as TF

pytestmark = pytest.mark.gpu

from oracle import philox  # noqa: E402
from tests import ssl_cifar_oracle as O  # noqa: E402

FWD_TOL, GRAD_TOL = 2e-5, 3e-5
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'ssl_cifar_step.npz')


@pytest.fixture
def K():
    import ctgan_amd.kernels as K
    return K


@pytest.fixture
def clean():
    import ctgan_amd.ct_cifar as M
    import ctgan_amd.tflib as lib
    lib.delete_all_params()
    yield M
    M.configure(); lib.delete_all_params(); lib.delete_param_aliases()


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


# ----------------------------------------------------------------------------------------------------- kernels
@pytest.mark.parametrize('shape', [(5, 5, 3, 128), (5, 5, 3, 32), (5, 5, 5, 7), (3, 3, 2, 1)])
@pytest.mark.parametrize('eps', [0.0, 1e-6])
def test_weight_norm_middle_axis_fwd_bwd(K, shape, eps):
    g = torch.Generator().manual_seed(sum(shape))
    theta = torch.randn(*shape, generator=g) * 0.05
    s = torch.rand(shape[2], generator=g) + 0.5
    gW = torch.randn(*shape, generator=g)
    w, rnorm = K.wn_mid_fwd(dev(theta), dev(s), eps)
    assert relerr(w, O.wn_mid_weight(theta.double(), s.double(), eps)) < FWD_TOL
    assert relerr(rnorm, 1.0 / torch.sqrt(eps + (theta.double() ** 2).sum(dim=(0, 1, 3)))) < FWD_TOL
    gt, gs = K.wn_mid_bwd(dev(gW), dev(theta), dev(s), rnorm)
    ft, fs = O.wn_mid_grad_formula(gW.double(), theta.double(), s.double(), eps)
    assert relerr(gt, ft) < GRAD_TOL and relerr(gs, fs) < GRAD_TOL
    gt2, none = K.wn_mid_bwd(dev(gW), dev(theta), dev(s), rnorm, want_gs=False)
    assert none is None and torch.equal(gt2, gt)


def test_weight_norm_autograd_both_layouts(K):
    import ctgan_amd.functional as F
    g = torch.Generator().manual_seed(1)
    theta = dev(torch.randn(5, 5, 3, 32, generator=g) * 0.05).requires_grad_(True)
    s = dev(torch.rand(3, generator=g) + 0.5).requires_grad_(True)
    gW = torch.randn(5, 5, 3, 32, generator=g)
    gt, gs = torch.autograd.grad(F.weight_norm_mid(theta, s, 1e-6), [theta, s], dev(gW))
    ft, fs = O.wn_mid_grad_formula(gW.double(), theta.detach().cpu().double(), s.detach().cpu().double(), 1e-6)
    assert relerr(gt, ft) < GRAD_TOL and relerr(gs, fs) < GRAD_TOL
    w = dev(torch.randn(3, 3, 32, 64, generator=g) * 0.05).requires_grad_(True)
    s2 = dev(torch.rand(64, generator=g) + 0.5)
    W_th = O.unrelabel('Classifier.2.W', w.detach().cpu().double(), None)
    ref = O.relabel('Classifier.2.W', O.wn_conv_weight(W_th, s2.cpu().double()), None)
    assert relerr(F.weight_norm_filter(w, s2, 1e-6), ref) < FWD_TOL


@pytest.mark.parametrize('rows,cols', [(4 * 36, 32), (13, 3), (500, 10), (4 * 7 * 7, 128)])
@pytest.mark.parametrize('act', ['lrelu', None, 'tanh'])
@pytest.mark.parametrize('init_stdv', [1.0, 0.1])
def test_map_init(K, rows, cols, act, init_stdv):
    g = torch.Generator().manual_seed(rows + cols)
    y = torch.randn(rows, cols, generator=g) * 3 + torch.randn(cols, generator=g)[None, :]
    s, b = torch.rand(cols, generator=g) + 0.5, torch.ones(cols)
    yd, sd, bd = dev(y), dev(s), dev(b)
    K.wn_init_map(yd, sd, bd, act, 0.2, init_stdv)
    y64 = y.double()
    mean = y64.mean(0)
    inv = init_stdv / torch.sqrt(((y64 - mean) ** 2).mean(0))
    ref = (y64 - mean) * inv
    ref = O.lrelu(ref) if act == 'lrelu' else (torch.tanh(ref) if act == 'tanh' else ref)
    assert relerr(yd, ref) < FWD_TOL
    assert relerr(sd, s.double() * inv) < FWD_TOL and relerr(bd, -mean * inv) < FWD_TOL


def test_map_init_on_a_channels_last_map(K):
    g = torch.Generator().manual_seed(3)
    y = torch.randn(4, 32, 6, 6, generator=g) + 2
    yd, sd, bd = cl(y), dev(torch.ones(32)), dev(torch.zeros(32))
    K.wn_init_map(yd, sd, bd, 'lrelu', 0.2, 1.0)
    c = y.double() - y.double().mean(dim=(0, 2, 3), keepdim=True)
    ref = O.lrelu(c / torch.sqrt((c * c).mean(dim=(0, 2, 3), keepdim=True)))
    assert relerr(yd, ref) < FWD_TOL
    with pytest.raises(AssertionError):
        K.wn_init_map(dev(y), sd, bd, 'lrelu', 0.2, 1.0)           # an NCHW map is not what the kernel indexes


@pytest.mark.parametrize('B,Fd', [(100, 128), (3, 5), (4, 32), (7, 67)])      # (7, 67): a ragged second column tile, rows < row slices
def test_loss_pieces_fwd_bwd(K, B, Fd):
    g = torch.Generator().manual_seed(B + Fd)
    f = torch.randn(4 * B, Fd, generator=g)
    logits = torch.randn(4 * B, 10, generator=g)
    logits[::2] = -logits[::2].abs()
    # feature consistency + train_err2
    out2 = K.featcons_fwd(dev(f), B, dev(logits))
    f64 = f.double()
    assert abs(out2[0].item() - ((f64[B:2 * B] - f64[2 * B:3 * B]) ** 2).mean().item()) < FWD_TOL * ((f64[B:2 * B] - f64[2 * B:3 * B]) ** 2).mean().item()
    assert out2[1].item() == pytest.approx((logits[:B].max(1).values <= 0).double().mean().item(), abs=1e-7)
    assert K.featcons_fwd(dev(f), B)[1].item() == 0.0
    gout = torch.tensor([0.7, 123.0])
    x = f64.clone().requires_grad_(True)
    (gr,) = torch.autograd.grad(((x[B:2 * B] - x[2 * B:3 * B]) ** 2).mean() * 0.7, x)
    gf = K.featcons_bwd(dev(f), dev(gout), B)
    assert relerr(gf, gr) < GRAD_TOL and gf[:B].abs().max().item() == 0.0 and gf[3 * B:].abs().max().item() == 0.0
    # L1 feature matching, with a column whose two means are equal
    f2 = f[:2 * B].clone()
    f2[B:, 1] = f2[:B, 1]
    loss, diff = K.featmatch_l1_fwd(dev(f2), B)
    assert abs(loss.item() - O.feat_match_l1(f2.double(), B).item()) < FWD_TOL * O.feat_match_l1(f2.double(), B).item()
    assert diff[1].item() == 0.0
    gm = K.featmatch_l1_bwd(diff, dev(torch.tensor(1.0)), B)
    assert relerr(gm, O.feat_match_l1_grad(f2.double(), B)) < GRAD_TOL and gm[:, 1].abs().max().item() == 0.0


def test_loss_pieces_autograd(K):
    import ctgan_amd.functional as F
    g = torch.Generator().manual_seed(0)
    B, Fd = 4, 32
    f = dev(torch.randn(4 * B, Fd, generator=g)).requires_grad_(True)
    out2 = F.feature_consistency(f, B, dev(torch.randn(4 * B, 10, generator=g)))
    (gf,) = torch.autograd.grad(out2, f, dev(torch.tensor([0.05, 0.0])))
    x = f.detach().cpu().double().requires_grad_(True)
    (gr,) = torch.autograd.grad(0.05 * ((x[B:2 * B] - x[2 * B:3 * B]) ** 2).mean(), x)
    assert relerr(gf, gr) < GRAD_TOL
    f2 = dev(torch.randn(2 * B, Fd, generator=g)).requires_grad_(True)
    (g2,) = torch.autograd.grad(F.feature_matching_l1(f2, B), f2)
    assert relerr(g2, O.feat_match_l1_grad(f2.detach().cpu().double(), B)) < GRAD_TOL


@pytest.mark.parametrize('B,C,H,W', [(100, 512, 4, 4), (4, 32, 2, 2), (3, 5, 1, 1)])
def test_generator_batch_norm(K, B, C, H, W):
    """nn.batch_norm(g=None) + ReLU: bn.hip with eps 1e-6 and a constant ones gain (ct_cifar._bn_relu)."""
    import ctgan_amd.functional as F
    g = torch.Generator().manual_seed(B + C)
    x = torch.randn(B, C, H, W, generator=g) * 2 + 1
    b = torch.randn(C, generator=g) * 0.5
    gy = torch.randn(B, C, H, W, generator=g)
    xd, bd = cl(x).requires_grad_(True), dev(b).requires_grad_(True)
    y = F.batch_norm(xd, dev(torch.ones(1, C)), bd.view(1, C), None, 1, True, 1e-6, f64_stats=True)
    x64, b64 = x.double().requires_grad_(True), b.double().requires_grad_(True)
    ref = torch.relu(O.batch_norm(x64, b64, (0, 2, 3)))
    assert relerr(y, ref) < FWD_TOL
    gx, gb = torch.autograd.grad(y, [xd, bd], cl(gy))
    rx, rb = torch.autograd.grad(ref, [x64, b64], gy.double())
    assert relerr(gx, rx) < GRAD_TOL and relerr(gb, rb) < GRAD_TOL
    # eps is what makes the difference on a nearly constant channel
    xc = torch.full((B, C, H, W), 0.5) + 1e-3 * torch.randn(B, C, H, W, generator=g)
    y6 = F.batch_norm(cl(xc), dev(torch.ones(1, C)), dev(torch.zeros(1, C)), None, 1, False, 1e-6, f64_stats=True)
    assert relerr(y6, O.batch_norm(xc.double(), torch.zeros(C, dtype=torch.float64), (0, 2, 3))) < 1e-3


def test_generator_dense_batch_norm(K):
    import ctgan_amd.functional as F
    g = torch.Generator().manual_seed(5)
    x = torch.randn(100, 8192, generator=g)
    b = torch.randn(8192, generator=g) * 0.1
    y = F.batch_norm(dev(x), dev(torch.ones(1, 8192)), dev(b).view(1, -1), None, 1, True, 1e-6, f64_stats=True)
    assert relerr(y, torch.relu(O.batch_norm(x.double(), b.double(), (0,)))) < FWD_TOL


# ----------------------------------------------------------------------------------------------------- gather
N_DATA, B_G = 37, 13


def _gather_data():
    r = np.random.RandomState(0)
    return r.randint(0, 256, size=(N_DATA, 3, 32, 32)).astype(np.uint8), r.randint(0, N_DATA, size=B_G).astype(np.int32)


def _unrot(t):
    return np.ascontiguousarray(t.cpu().numpy()[:, :, ::-1, ::-1])


@pytest.mark.parametrize('win', [32, 36])
@pytest.mark.parametrize('flip', [False, True])
def test_gather_fixed_windows_equal_numpy(K, win, flip):
    data, idx = _gather_data()
    lut = dev(torch.from_numpy(O.byte_table()))
    dd, di = dev(torch.from_numpy(data)), dev(torch.from_numpy(idx))
    top = 36 - win
    for oy, ox in {(0, 0), (0, top), (top, 0), (top, top), (top // 2, top // 2)}:
        want = O.gather_reference(data, idx, win, 2, offset=(oy, ox), flip=flip)
        # the reference itself, once more from first principles
        P = np.pad(data[idx], ((0, 0), (0, 0), (2, 2), (2, 2)), 'reflect')
        P = P[:, :, :, ::-1] if flip else P
        assert np.array_equal(want, ((-127.5 + P[:, :, oy:oy + win, ox:ox + win]) / np.float32(255.0)).astype(np.float32))
        got = K.aug_gather(dd, di, lut, win, 2, offset=(oy, ox), flip=flip)
        assert got.permute(0, 2, 3, 1).is_contiguous() and np.array_equal(_unrot(got), want)
        plain = K.aug_gather(dd, di, lut, win, 2, offset=(oy, ox), flip=flip, rot180=False, channels_last=False)
        assert plain.is_contiguous() and np.array_equal(plain.cpu().numpy(), want)
    with pytest.raises(ValueError):
        K.aug_gather(dd, di, lut, win, 2, offset=(top + 1, 0))


def test_gather_draws_are_the_documented_stream(K):
    # the second stream is corner B of tests/philox_spec.py: high key word, rank bits of the stream id and counter word 3 all non-zero
    for seed, sid, step in ((1234567891011, 17, 6), (0x9E3779B97F4A7C15, (513 << 16) | 7, (1 << 32) + 5)):
        _gather_draws_on_stream(K, seed, sid, step)


def _gather_draws_on_stream(K, seed, sid, step):
    data, idx = _gather_data()
    lut = dev(torch.from_numpy(O.byte_table()))
    dd, di = dev(torch.from_numpy(data)), dev(torch.from_numpy(idx))
    ctr = torch.tensor([step], dtype=torch.int64, device='cuda')
    u = philox.uniform(seed, sid, step, 3 * B_G).reshape(B_G, 3)
    draws = (u[:, 0] > 0.5, np.minimum((5 * u[:, 1]).astype(int), 4), np.minimum((5 * u[:, 2]).astype(int), 4))
    assert all(np.array_equal(a, b) for a, b in zip(draws, O.aug_draws(seed, sid, step, B_G, 2)))
    got = K.aug_gather(dd, di, lut, 32, 2, spec=(seed, sid, ctr))
    assert np.array_equal(_unrot(got), O.gather_reference(data, idx, 32, 2, draws))
    assert torch.equal(K.aug_gather(dd, di, lut, 32, 2, spec=(seed, sid, ctr)), got)               # same step, same batch
    ctr += 1
    assert not torch.equal(K.aug_gather(dd, di, lut, 32, 2, spec=(seed, sid, ctr)), got)
    # an index outside the set reads nothing and poisons its row only
    bad = di.clone(); bad[4] = N_DATA
    out = K.aug_gather(dd, bad, lut, 32, 2, offset=(2, 2))
    assert torch.isnan(out[4]).all() and torch.isfinite(out[:4]).all() and torch.isfinite(out[5:]).all()


# ----------------------------------------------------------------------------------------------------- routes
D_W = (128, 128, 128, 256, 256, 256, 512, 256, 128)
# (layer, C, K, stride, pad) x the sizes of the training pass and of the padded init pass
CRITIC_LAYERS = [(1, 3, D_W[0], 1, 1, (32, 36)), (2, D_W[0], D_W[1], 1, 1, (32, 36)), (3, D_W[1], D_W[2], 2, 1, (32, 36)),
                 (4, D_W[2], D_W[3], 1, 1, (16, 18)), (5, D_W[3], D_W[4], 1, 1, (16, 18)), (6, D_W[4], D_W[5], 2, 1, (16, 18)),
                 (7, D_W[5], D_W[6], 1, 0, (8, 9))]


@pytest.mark.parametrize('layer,C,Ko,stride,pad,sizes', CRITIC_LAYERS, ids=lambda v: str(v) if isinstance(v, int) else None)
def test_critic_conv_routes_against_theano_geometry(K, layer, C, Ko, stride, pad, sizes):
    import ctgan_amd.functional as F
    g = torch.Generator().manual_seed(layer)
    for S in sizes:
        x = torch.randn(4, C, S, S, generator=g)
        W = torch.randn(Ko, C, 3, 3, generator=g) / np.sqrt(9 * C)
        b = torch.randn(Ko, generator=g)
        x64, W64 = x.double().requires_grad_(True), W.double().requires_grad_(True)
        ref = TF.conv2d(x64, W64, b.double(), stride=stride, padding=pad)
        xd = cl(torch.flip(x, (2, 3))).requires_grad_(True)
        wd = dev(O.relabel('Classifier.%d.W' % layer, W, None)).requires_grad_(True)
        y = F.conv2d(xd, wd, dev(b), stride=stride)
        print('layer', layer, 'size', S, 'fwd kernel', K.last_kernel())
        if pad == 0:
            y = F.crop(y, S - 2, S - 2, 1, 1)
        assert relerr(torch.flip(y, (2, 3)), ref) < FWD_TOL
        gy = torch.randn(ref.shape, generator=g)
        gx, gw = torch.autograd.grad(y, [xd, wd], cl(torch.flip(gy, (2, 3))))
        print('layer', layer, 'size', S, 'last bwd kernel', K.last_kernel())
        rx, rw = torch.autograd.grad(ref, [x64, W64], gy.double())
        assert relerr(torch.flip(gx, (2, 3)), rx) < GRAD_TOL
        assert relerr(O.unrelabel('Classifier.%d.W' % layer, gw.detach().cpu(), None), rw) < GRAD_TOL


@pytest.mark.parametrize('C,Ko,sizes', [(D_W[6], D_W[7], (6, 7)), (D_W[7], D_W[8], (6, 7))])
def test_nin_routes(K, C, Ko, sizes):
    import ctgan_amd.functional as F
    g = torch.Generator().manual_seed(C)
    for S in sizes:
        x, W = torch.randn(4, C, S, S, generator=g), torch.randn(C, Ko, generator=g) / np.sqrt(C)
        x64, W64 = x.double().requires_grad_(True), W.double().requires_grad_(True)
        ref = torch.einsum('nchw,co->nohw', x64, W64)
        xd, wd = cl(x).requires_grad_(True), dev(W).requires_grad_(True)
        y = F.conv2d(xd, wd.view(1, 1, C, Ko))
        print('NIN', C, Ko, S, 'fwd kernel', K.last_kernel())
        assert relerr(y, ref) < FWD_TOL
        gy = torch.randn(ref.shape, generator=g)
        gx, gw = torch.autograd.grad(y, [xd, wd], cl(gy))
        rx, rw = torch.autograd.grad(ref, [x64, W64], gy.double())
        assert relerr(gx, rx) < GRAD_TOL and relerr(gw, rw) < GRAD_TOL


@pytest.mark.parametrize('Ci,Co,S', [(512, 256, 4), (256, 128, 8), (128, 3, 16)])
def test_transposed_conv_routes_against_theano_geometry(K, Ci, Co, S):
    import ctgan_amd.functional as F
    g = torch.Generator().manual_seed(Ci)
    z = torch.randn(4, Ci, S, S, generator=g)
    W = torch.randn(Ci, Co, 5, 5, generator=g) / np.sqrt(25 * Ci / 4)
    z64, W64 = z.double().requires_grad_(True), W.double().requires_grad_(True)
    ref = TF.conv_transpose2d(z64, W64, stride=2, padding=2, output_padding=1)
    zd = cl(torch.flip(z, (2, 3))).requires_grad_(True)
    wd = dev(O.relabel('Generator.2.W', W, None)).requires_grad_(True)
    y = F.conv2d_transpose(zd, wd, None, stride=2)
    print('deconv', Ci, Co, S, 'fwd kernel', K.last_kernel())
    assert relerr(torch.flip(y, (2, 3)), ref) < FWD_TOL
    gy = torch.randn(ref.shape, generator=g)
    gz, gw = torch.autograd.grad(y, [zd, wd], cl(torch.flip(gy, (2, 3))))
    print('deconv', Ci, Co, S, 'last bwd kernel', K.last_kernel())
    rz, rw = torch.autograd.grad(ref, [z64, W64], gy.double())
    assert relerr(torch.flip(gz, (2, 3)), rz) < GRAD_TOL
    assert relerr(O.unrelabel('Generator.2.W', gw.detach().cpu(), None), rw) < GRAD_TOL


# ----------------------------------------------------------------------------------------------------- steps, graphs, loop
def test_steps_match_the_oracle_and_the_committed_fixture(clean):
    """Init, one classifier step and one generator step at small_cfg(), teacher-forced on shared streams: scalars within 2e-4,
    gradients within relative L2 max(3e-3, 3 x fp32 twin), updates and averages by the update_ok rule; the oracle's outputs in the
    same run equal tests/golden/ssl_cifar_step.npz."""
    O.small_cfg()
    got = {}
    assert O.run_steps('cuda', cost_tol=2e-4, grad_tol=3e-3, log=print, golden=got) == 21 + 9
    with np.load(GOLDEN) as want:
        assert O.golden_matches(got, want) > 20


def _full_size_run(M, data, batches, init_idx, graphed, resume_after=None, tmp=None):
    """init on the padded rows + len(batches) iterations -> (trainer, engine, [outputs])."""
    import ctgan_amd.tflib as lib
    from ctgan_amd import checkpoint
    from ctgan_amd.engine import GraphedCifarSSLTrainer
    lib.delete_all_params(); lib.set_seed(3)
    tr = M.CifarSSLTrainer(seed=9, data=data)
    if resume_after is None:
        tr.init_params(tr.gather_fixed(dev(init_idx), M.cfg.IMG + 2 * M.cfg.PAD, (0, 0)))
        start = 0
    else:
        start = checkpoint.load(tmp, tr)
        assert start == resume_after
    eng = GraphedCifarSSLTrainer(tr, use_graphs=graphed)
    outs = []
    for k in range(start, len(batches)):
        out = eng.train_iteration(*batches[k])
        outs.append({n: v.clone() for n, v in out.items()})
        if tmp is not None and resume_after is None and k == 0:
            checkpoint.save(tmp, tr, 1)
    return tr, eng, outs


def _state(tr):
    import ctgan_amd.tflib as lib
    s = {'p/' + n: p.detach().clone() for n, p in lib._params.items()}
    for w, o in (('d', tr.d_opt), ('g', tr.g_opt)):
        for i, b in enumerate(o.slots()):
            s['%s/slot%d' % (w, i)] = b.clone()
        s[w + '/t'] = torch.tensor(o.t)
    s['ctr'] = tr.rng.ctr.clone()
    return s


def test_full_size_graph_replay_equals_eager_and_resume(clean, tmp_path):
    """B 100, the script's widths: init on 500 padded rows and three iterations.  Graph replay equals eager bit for bit (every
    parameter, average, Adam slot and counter), and a run resumed from a checkpoint after iteration 1 equals the uninterrupted one."""
    M = clean
    M.configure()
    r = np.random.RandomState(1)
    data = r.randint(0, 256, size=(1000, 3, 32, 32)).astype(np.uint8)
    t = lambda a: torch.from_numpy(a.astype(np.int32))          # noqa: E731
    batches = [(t(r.randint(0, 1000, 100)), t(r.randint(0, 10, 100)), t(r.randint(0, 1000, 100)), t(r.randint(0, 1000, 100))) for _ in range(3)]
    init_idx = t(r.randint(0, 1000, 500))
    ck = str(tmp_path / 'c.pt')
    tr, eng, outs_e = _full_size_run(M, data, batches, init_idx, graphed=False, tmp=ck)
    assert not eng.graphed
    eager = _state(tr)
    assert tr.d_opt.skipped() == 0 and tr.g_opt.skipped() == 0 and tr.iteration == 3
    for o in outs_e:
        for n, v in o.items():
            assert torch.isfinite(v).all(), n
        print('eager', {n: float(v) for n, v in o.items() if v.numel() == 1})
    tr, eng, outs_g = _full_size_run(M, data, batches, init_idx, graphed=True)
    assert eng.graphed, eng.graph_error
    assert tr.d_opt.skipped() == 0
    graph = _state(tr)
    assert sorted(graph) == sorted(eager)
    for n in eager:
        assert torch.equal(graph[n], eager[n]), ('graph replay differs from eager', n)
    for a, b in zip(outs_e, outs_g):
        for n in a:
            assert torch.equal(a[n], b[n]), n
    tr, eng, outs_r = _full_size_run(M, data, batches, init_idx, graphed=True, resume_after=1, tmp=ck)
    assert eng.graphed, eng.graph_error
    resumed = _state(tr)
    for n in eager:
        assert torch.equal(resumed[n], eager[n]), ('resumed run differs', n)


def test_short_loop_on_synthetic_data_against_the_oracle(clean):
    """LOOP_ITERS graphed iterations at LOOP_CFG on class-prototype images: the configuration was chosen on the CPU from the oracle
    alone (its live-weight test error on the 200 test examples is at most 0.05, asserted here); the product's live-weight error is
    within 0.025 (five examples, the margin of the MNIST loop test) of the oracle's."""
    M = clean
    cfg = M.configure(**O.LOOP_CFG)
    data = O.synthetic_data(cfg)
    init_idx, batches = O.loop_batches(cfg, data, O.LOOP_ITERS)
    ref_live, ref_avg, ref_trace = O.loop_oracle(cfg, data, init_idx, batches)
    print('oracle live %.4f averaged %.4f loss_lab %.4f -> %.4f' % (ref_live, ref_avg, ref_trace[0], ref_trace[-1]))
    assert ref_live <= 0.05
    live, avg, trace = O.loop_product(cfg, data, init_idx, batches, 'cuda', graphed=True)
    print('product live %.4f averaged %.4f loss_lab %.4f -> %.4f' % (live, avg, trace[0], trace[-1]))
    assert all(np.isfinite(trace))
    assert abs(live - ref_live) <= 0.025


def test_train_on_arrays(clean, tmp_path):
    """train() on a tiny synthetic set: two shortened epochs, the report lines, the optimiser step counts, a resume."""
    M = clean
    cfg = M.configure(**dict(O.LOOP_CFG, COUNT=3, EPOCHS=2))
    data = O.synthetic_data(cfg, n_train=200, n_test=40)
    arrays = {k: data[k] for k in ('x_train', 'y_train', 'x_test', 'y_test')}
    lines = []
    tr = M.train(arrays=arrays, epochs=2, out_dir=str(tmp_path), log=lines.append, max_batches=3)
    assert len(lines) == 2 and lines[0].startswith('Iteration 0, time = ') and lines[1].startswith('Iteration 1, time = ')
    for key in ('loss_lab = ', 'loss_unl = ', 'train err = ', 'train err2 = ', 'gen loss = ', 'test err = '):
        assert key in lines[1]
    assert tr.d_opt.t == tr.g_opt.t == 6 and tr.iteration == 6 and tr.d_opt.skipped() == 0
    want = {n: p.detach().clone() for n, p in __import__('ctgan_amd.tflib', fromlist=['x'])._params.items()}
    # resumed from the checkpoint of epoch 1... which is the final one: nothing left to run, the weights are the saved ones
    tr2 = M.train(arrays=arrays, epochs=2, out_dir=None, resume=str(tmp_path / 'checkpoint.pt'), log=lines.append, max_batches=3)
    assert len(lines) == 2 and tr2.d_opt.t == 6
    for n, p in __import__('ctgan_amd.tflib', fromlist=['x'])._params.items():
        assert torch.equal(p.detach(), want[n]), n
