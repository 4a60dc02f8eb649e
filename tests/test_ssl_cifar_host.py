"""The convolutional semi-supervised CT classifier (ctgan_amd.ct_cifar) without a GPU: self-checks of its fp64 oracle
(tests/ssl_cifar_oracle.py) - the mirror identities between Theano's padding and TF-SAME, the init statistics, the weight-norm and L1
feature-matching gradients against closed forms -, the host logic of the trainer on CPU stand-ins of the new kernel wrappers against
that oracle, the Config literals, the host data class, a checkpoint round trip, and the oracle pinned to the committed fixture
tests/golden/ssl_cifar_step.npz."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as TF

from tests import ssl_cifar_oracle as O

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'ssl_cifar_step.npz')


@pytest.fixture
def ssl_kernels(cpu_kernels, monkeypatch):
    import ctgan_amd.ct_cifar as M
    import ctgan_amd.tflib as lib
    O.install_stand_ins(monkeypatch)
    yield cpu_kernels
    M.configure(); lib.delete_all_params(); lib.delete_param_aliases()


def _small():
    import ctgan_amd.ct_cifar as M
    return M.Config(IMG=16, D_WIDTHS=(32, 32, 32, 64, 64, 64, 96, 64, 32), G_WIDTHS=(64, 32, 32), BATCH_SIZE=4, INIT_ROWS=12)


def _rand(*shape, seed=0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)


# ----------------------------------------------------------------------------------------------------- oracle self-checks
@pytest.mark.parametrize('size,stride', [(8, 2), (36, 2), (18, 2), (7, 1), (8, 1)])
def test_conv_mirror_identity(size, stride):
    """conv_theano(x; W) = R conv_same(R x; R W): pad 1 in Theano's geometry against TF-SAME in rotated coordinates."""
    x, W = _rand(2, 3, size, size, seed=1), _rand(5, 3, 3, 3, seed=2)
    ref = TF.conv2d(x, W, stride=stride, padding=1)
    got = O.rot(O.conv_same(O.rot(x), O.relabel('Classifier.1.W', W, None), stride))
    assert got.shape == ref.shape and (got - ref).abs().max().item() < 1e-12


@pytest.mark.parametrize('size', [2, 4, 16])
def test_deconv_mirror_identity(size):
    """deconv_theano(z; W) = R deconv_same(R z; R W) with W [in,out,5,5] against conv_transpose2d(stride 2, padding 2, output_padding 1)."""
    z, W = _rand(2, 4, size, size, seed=3), _rand(4, 3, 5, 5, seed=4)
    ref = TF.conv_transpose2d(z, W, stride=2, padding=2, output_padding=1)
    got = O.rot(O.deconv_same(O.rot(z), O.relabel('Generator.4.W', W, None)))
    assert got.shape == ref.shape and (got - ref).abs().max().item() < 1e-12


def test_centre_crop_is_the_unpadded_conv():
    x, W = _rand(2, 3, 8, 8, seed=5), _rand(5, 3, 3, 3, seed=6)
    ref = TF.conv2d(x, W, padding=0)
    same = O.rot(O.conv_same(O.rot(x), O.relabel('Classifier.7.W', W, None)))
    assert (same[:, :, 1:-1, 1:-1] - ref).abs().max().item() < 1e-12


def test_relabel_round_trip():
    cfg = _small()
    for n, v in O.make_params(cfg, seed=0).items():
        assert torch.equal(O.unrelabel(n, O.relabel(n, v, cfg), cfg), v), n


def test_oracle_init_normalises_every_pre_activation():
    cfg = _small()
    P = O.make_params(cfg, seed=1)
    S = cfg.IMG + 2 * cfg.PAD
    x = torch.rand(cfg.INIT_ROWS, 3, S, S, generator=torch.Generator().manual_seed(2), dtype=torch.float64) - 0.5
    pre = []
    O.init_passes(P, cfg, x, seed=3, step=0, pre=pre)
    assert len(pre) == 11                        # the generator's last layer, then the classifier's ten
    stdv = [cfg.G_INIT_STDV] + [1.0] * 9 + [cfg.D_INIT_STDV]
    for a, s in zip(pre, stdv):
        axes = (0, 2, 3) if a.dim() == 4 else (0,)
        assert a.mean(dim=axes).abs().max().item() < 1e-12 and ((a * a).mean(dim=axes).sqrt() - s).abs().max().item() < 1e-12
    # ... and the stored (g, b) reproduce them: the same noisy pass without init gives the normalised logits
    logits = O.classifier(P, cfg, x, O.site_masks(cfg, 3, 1, cfg.INIT_ROWS, S, 0, torch.float64))
    assert (logits - pre[-1]).abs().max().item() < 1e-10


@pytest.mark.parametrize('eps', [0.0, 1e-6])
def test_oracle_weight_norm_gradients_equal_the_formula(eps):
    g = torch.Generator().manual_seed(4)
    # the transposed-conv layout [k,k,out,in]
    theta = torch.randn(5, 5, 3, 7, generator=g, dtype=torch.float64, requires_grad=True)
    s = (torch.rand(3, generator=g, dtype=torch.float64) + 0.5).requires_grad_(True)
    gW = torch.randn(5, 5, 3, 7, generator=g, dtype=torch.float64)
    gt, gs = torch.autograd.grad(O.wn_mid_weight(theta, s, eps), [theta, s], gW)
    ft, fs = O.wn_mid_grad_formula(gW, theta.detach(), s.detach(), eps)
    assert (gt - ft).abs().max().item() < 1e-12 and (gs - fs).abs().max().item() < 1e-12
    # ... which is Theano's Deconv norm under the relabelling
    W_th = O.unrelabel('Generator.4.W', theta.detach(), None)
    assert (O.relabel('Generator.4.W', O.wn_deconv_weight(W_th, s.detach(), eps), None) - O.wn_mid_weight(theta, s, eps)).abs().max().item() < 1e-14
    # the HWIO conv layout through the [k k in, out] view
    from tests.ssl_oracle import wn_grad_formula, wn_weight
    th = torch.randn(3, 3, 4, 6, generator=g, dtype=torch.float64, requires_grad=True)
    s6 = (torch.rand(6, generator=g, dtype=torch.float64) + 0.5).requires_grad_(True)
    gW = torch.randn(3, 3, 4, 6, generator=g, dtype=torch.float64)
    W_th = O.unrelabel('Classifier.1.W', th, None)
    gt, gs = torch.autograd.grad(O.relabel('Classifier.1.W', O.wn_conv_weight(W_th, s6, eps), None), [th, s6], gW)
    ft, fs = wn_grad_formula(gW.reshape(36, 6), th.detach().reshape(36, 6), s6.detach(), eps)
    assert (gt.reshape(36, 6) - ft).abs().max().item() < 1e-12 and (gs - fs).abs().max().item() < 1e-12
    assert (wn_weight(th.detach().reshape(36, 6), s6.detach(), eps).reshape(3, 3, 4, 6)
            - O.relabel('Classifier.1.W', O.wn_conv_weight(W_th, s6, eps), None)).abs().max().item() < 1e-14


def test_oracle_l1_feature_match_gradient():
    f = _rand(8, 5, seed=7)
    f[4:, 2] = f[:4, 2]                       # a column whose two means are equal: gradient 0
    f = f.requires_grad_(True)
    (g,) = torch.autograd.grad(O.feat_match_l1(f, 4), f)
    assert (g - O.feat_match_l1_grad(f.detach(), 4)).abs().max().item() < 1e-15
    assert g[:, 2].abs().max().item() == 0.0


# ----------------------------------------------------------------------------------------------------- stand-ins against the oracle
def test_stand_in_losses_against_autograd():
    B, Fd = 3, 5
    f = _rand(4 * B, Fd, seed=8).float()
    logits = _rand(4 * B, 10, seed=9).float()
    logits[1] = -logits[1].abs()
    out2 = O._featcons_fwd(f, B, logits)
    assert abs(out2[0].item() - ((f[B:2 * B] - f[2 * B:3 * B]) ** 2).mean().item()) < 1e-7
    assert abs(out2[1].item() - (logits[:B].max(1).values <= 0).float().mean().item()) < 1e-7 and out2[1].item() > 0
    x = f.clone().requires_grad_(True)
    (g,) = torch.autograd.grad(((x[B:2 * B] - x[2 * B:3 * B]) ** 2).mean() * 0.7, x)
    assert (O._featcons_bwd(f, torch.tensor([0.7, 0.0]), B) - g).abs().max().item() < 1e-7
    loss, diff = O._featmatch_l1_fwd(f[:2 * B], B)
    assert abs(loss.item() - O.feat_match_l1(f[:2 * B].double(), B).item()) < 1e-7
    assert (O._featmatch_l1_bwd(diff, torch.tensor(1.0), B).double() - O.feat_match_l1_grad(f[:2 * B].double(), B)).abs().max().item() < 1e-7


def test_gather_stand_in_matches_the_documented_draws():
    r = np.random.RandomState(0)
    data = r.randint(0, 256, size=(9, 3, 8, 8)).astype(np.uint8)
    idx = np.array([3, 0, 8, 8, 1], dtype=np.int32)
    lut = torch.from_numpy(O.byte_table())
    ctr = torch.tensor([4], dtype=torch.int64)
    got = O._aug_gather(torch.from_numpy(data), torch.from_numpy(idx), lut, 8, 2, spec=(7, 16, ctr))
    assert got.permute(0, 2, 3, 1).is_contiguous()
    flip, oy, ox = O.aug_draws(7, 16, 4, 5, 2)
    assert oy.min() >= 0 and oy.max() <= 4
    P = np.pad(data[idx], ((0, 0), (0, 0), (2, 2), (2, 2)), 'reflect')
    for k in range(5):
        img = P[k][:, :, ::-1] if flip[k] else P[k]
        want = ((-127.5 + img[:, oy[k]:oy[k] + 8, ox[k]:ox[k] + 8]) / np.float32(255.0)).astype(np.float32)
        assert np.array_equal(got[k].numpy()[:, ::-1, ::-1], want)


# ----------------------------------------------------------------------------------------------------- trainer against the oracle
def test_steps_match_the_oracle_on_the_stand_ins(ssl_kernels):
    O.small_cfg()
    got = {}
    n = O.run_steps('cpu', log=print, golden=got)
    assert n == 21 + 9               # the classifier's ten W, ten b and the last g; the generator's nine
    with np.load(GOLDEN) as want:
        O.golden_matches(got, want)


def test_oracle_equals_the_golden_file():
    cfg = _small()
    with np.load(GOLDEN) as want:
        assert O.golden_matches(O.oracle_golden(cfg), want) > 20
    assert os.path.getsize(GOLDEN) < 200 * 1024


def test_public_functions_use_the_reference_orientation(ssl_kernels):
    import ctgan_amd.ct_cifar as M
    import ctgan_amd.tflib as lib
    cfg = O.small_cfg()
    lib.delete_all_params()
    M.build_params()
    P = O.make_params(cfg, seed=2, dtype=torch.float32)
    O.load_into_registry(P, cfg)
    z = torch.rand(cfg.BATCH_SIZE, cfg.Z_DIM, generator=torch.Generator().manual_seed(0))
    P64 = {n: v.double() for n, v in P.items()}
    with torch.no_grad():
        x = M.Generator(cfg.BATCH_SIZE, noise=z)
        ref = O.generator(P64, cfg, z.double())
        assert (x.double() - ref).abs().max().item() < 1e-5
        logits, feat = M.Classifier(ref.float(), deterministic=True, features='both')
        rl, rf = O.classifier(P64, cfg, ref, features='both')
    assert (logits.double() - rl).abs().max().item() < 2e-5 * max(1.0, rl.abs().max().item())
    assert (feat.double() - rf).abs().max().item() < 2e-5 * max(1.0, rf.abs().max().item())


def test_predict_uses_the_averages_and_live_g(ssl_kernels):
    import ctgan_amd.ct_cifar as M
    import ctgan_amd.tflib as lib
    cfg = O.small_cfg()
    lib.delete_all_params()
    tr = M.CifarSSLTrainer(seed=1)
    x = torch.rand(cfg.BATCH_SIZE, 3, cfg.IMG, cfg.IMG) - 0.5
    live = tr.predict(x, averaged=False)
    with torch.no_grad():
        tr.d_opt.avg.copy_(tr.d_opt.theta * 0.5)
        lib._params['Classifier.1.g'].mul_(2.0)
    avg = tr.predict(x, averaged=True)
    P = O.from_registry(cfg)
    Q = dict(P)
    Q.update({n: O.unrelabel(n, a.detach(), cfg).double() for n, a in tr.d_opt.avg_views()})
    assert torch.equal(Q['Classifier.1.g'], P['Classifier.1.g'])        # not trained: no average, stays live
    ref = O.classifier(Q, cfg, x.double())
    assert (avg.double() - ref).abs().max().item() < 2e-5 * max(1.0, ref.abs().max().item())
    assert not torch.allclose(avg, live)
    assert not lib._param_aliases


# ----------------------------------------------------------------------------------------------------- literals, data, checkpoint
def test_config_literals():
    import ctgan_amd.ct_cifar as M
    c = M.Config()
    assert (c.SEED, c.SEED_DATA, c.COUNT, c.BATCH_SIZE, c.UNLABELED_WEIGHT, c.LR, c.BETA1) == (2, 2, 400, 100, 1., 0.0003, 0.5)
    assert (c.AVG_RATE, c.EPOCHS, c.INIT_ROWS, c.Z_DIM, c.PAD, c.DROP_IN, c.DROP_HIDDEN, c.FEAT_WEIGHT) == (1e-4, 1000, 500, 50, 2, 0.2, 0.5, 0.05)
    assert (c.IMG, c.D_WIDTHS, c.G_WIDTHS) == (32, (128, 128, 128, 256, 256, 256, 512, 256, 128), (512, 256, 128))
    assert (c.G_INIT_STDV, c.D_INIT_STDV, c.N_CLASSES, c.BETA2) == (0.1, 0.1, 10, 0.999)
    with pytest.raises(AttributeError):
        M.Config(NOPE=1)
    assert np.array_equal(M.byte_table(), O.byte_table()) and M.byte_table().dtype == np.float32
    assert M.byte_table()[0] == np.float32(-0.5) and M.byte_table()[255] == np.float32(0.5)


def _arrays(n=130, n_test=20, seed=0, size=16):
    r = np.random.RandomState(seed)
    return {'x_train': r.randint(0, 256, (n, 3 * size * size)).astype(np.uint8), 'y_train': np.arange(n) % 10,
            'x_test': r.randint(0, 256, (n_test, 3, size, size)).astype(np.uint8), 'y_test': np.arange(n_test) % 10}


def test_data_class_labelled_pick_and_draw_order():
    import ctgan_amd.ct_cifar as M
    M.configure(IMG=16, BATCH_SIZE=10, INIT_ROWS=12)
    try:
        a = _arrays()
        d = M.CifarSSLData(arrays=a, count=3, seed=5, seed_data=9)
        assert d.train_x.shape == (130, 3, 16, 16) and d.train_x.dtype == np.uint8 and d.nr_batches_train == 13
        inds = np.random.RandomState(9).permutation(130)
        ys = a['y_train'][inds]
        want = np.concatenate([inds[ys == j][:3] for j in range(10)])
        assert np.array_equal(d.lab_idx, want) and np.array_equal(d.lab_y, np.repeat(np.arange(10), 3))
        r = np.random.RandomState(5)
        r.randint(2 ** 15); r.randint(2 ** 15)
        for _ in range(2):                                   # two epochs: ceil(130 / 30) = 5 permutations, then unl, then unl2
            n = d.begin_epoch()
            perms = [r.permutation(30) for _ in range(5)]
            assert n == 13 and np.array_equal(d.i_lab, np.concatenate([want[p] for p in perms]))
            assert np.array_equal(d.y_lab, a['y_train'][d.i_lab])
            assert np.array_equal(d.i_unl, r.permutation(130)) and np.array_equal(d.i_unl2, r.permutation(130))
        assert np.array_equal(d.init_indices(), d.i_lab[:12])
        i_lab, y, i_unl, i_unl2 = d.batch(12)
        assert i_lab.dtype == np.int32 and y.dtype == np.int32 and i_unl.dtype == np.int32 and len(i_unl2) == 10
        assert np.array_equal(i_unl, d.i_unl[120:130])
        with pytest.raises(IOError):
            M.CifarSSLData('/nonexistent/dir')
    finally:
        M.configure()


def test_checkpoint_round_trip(ssl_kernels, tmp_path):
    import ctgan_amd.ct_cifar as M
    import ctgan_amd.tflib as lib
    from ctgan_amd import checkpoint
    cfg = O.small_cfg()
    a = _arrays(40, 8)
    idx = lambda *v: torch.tensor(v, dtype=torch.int32)          # noqa: E731
    batch = (idx(0, 5, 9, 2), idx(1, 2, 3, 4), idx(7, 8, 30, 39), idx(11, 12, 13, 14))

    def fresh():
        lib.delete_all_params()
        tr = M.CifarSSLTrainer(seed=3, data=a['x_train'].reshape(40, 3, 16, 16))
        return tr

    tr = fresh()
    tr.init_params(tr.gather_fixed(torch.arange(12, dtype=torch.int32), cfg.IMG + 2 * cfg.PAD, (0, 0)))
    tr.train_iteration_idx(*batch)
    checkpoint.save(str(tmp_path / 'c.pt'), tr, 1)
    out1 = tr.train_iteration_idx(*batch)
    want = {n: p.detach().clone() for n, p in lib._params.items()}
    want_avg = tr.d_opt.avg.clone()
    tr2 = fresh()
    assert checkpoint.load(str(tmp_path / 'c.pt'), tr2) == 1
    assert not lib._params['Classifier.3.g'].requires_grad and lib._params['Classifier.10.g'].requires_grad
    out2 = tr2.train_iteration_idx(*batch)
    for n, p in lib._params.items():
        assert torch.equal(p.detach(), want[n]), n
    assert torch.equal(tr2.d_opt.avg, want_avg) and torch.equal(out1['out4'], out2['out4']) and torch.equal(out1['loss_gen'], out2['loss_gen'])
    assert int(tr2.rng.ctr.item()) == int(tr.rng.ctr.item()) == 2 + 4


def test_train_runs_two_short_epochs_on_arrays(ssl_kernels, tmp_path):
    import ctgan_amd.ct_cifar as M
    O.small_cfg(COUNT=2, EPOCHS=2)
    lines = []
    tr = M.train(arrays=_arrays(40, 8), epochs=2, use_graphs=False, out_dir=str(tmp_path), log=lines.append, max_batches=2)
    assert len(lines) == 2 and lines[1].startswith('Iteration 1, time = ')
    for key in ('loss_lab = ', 'loss_unl = ', 'train err = ', 'train err2 = ', 'gen loss = ', 'test err = '):
        assert key in lines[0]
    assert tr.d_opt.t == tr.g_opt.t == 4 and tr.iteration == 4
    assert os.path.isfile(tmp_path / 'checkpoint.pt') and os.path.isfile(tmp_path / 'log.jsonl')
