"""The temporal-ensembling CT classifier (ctgan_amd.ct_cifar_te) without a GPU: the CPU stand-ins of its three kernel wrappers against
fp64 autograd of the written-out expression, the Config literals, the host logic of the trainer on the stand-ins against the fp64
oracle (tests/ssl_cifar_te_oracle.py) and the oracle pinned to tests/golden/ssl_cifar_te_step.npz, the kept quirks of the tables
(epoch-0 targets, unvisited rows), train() on arrays and a checkpoint round trip with the tables."""
import os

import numpy as np
import pytest
import torch

from tests import ssl_cifar_oracle as O
from tests import ssl_cifar_te_oracle as TO

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'ssl_cifar_te_step.npz')


@pytest.fixture
def te_kernels(cpu_kernels, monkeypatch):
    import ctgan_amd.ct_cifar as M
    import ctgan_amd.ct_cifar_te as T
    import ctgan_amd.tflib as lib
    TO.install_stand_ins(monkeypatch)
    yield cpu_kernels
    T.configure(); M.configure(); lib.delete_all_params(); lib.delete_param_aliases()


def _head_inputs(B, nc, Fd, N, seed):
    g = torch.Generator().manual_seed(seed)
    logits, feat = torch.randn(3 * B, nc, generator=g) * 2, torch.randn(3 * B, Fd, generator=g)
    labels = torch.randint(0, nc, (B,), generator=g, dtype=torch.int32)
    idx = torch.randperm(N, generator=g)[:B].to(torch.int32)
    return logits, feat, labels, idx, torch.randn(N, nc, generator=g) * 2, torch.randn(N, Fd, generator=g)


# ----------------------------------------------------------------------------------------------------- stand-ins
@pytest.mark.parametrize('split', [False, True])
def test_stand_in_head_against_fp64_autograd(split):
    B, nc, Fd, N = 6, 5, 7, 11
    logits, feat, labels, idx, tg, tg2 = _head_inputs(B, nc, Fd, N, 3)
    ii = idx.long()
    gout = torch.tensor([0.7, 1.3, 5.0, 5.0, 5.0, 5.0, 5.0, 5.0])
    M = 0.0
    if split:          # a hinge offset midway between the two middle rows' arguments at M = 0 (no row sits on the kink)
        base, _, _ = TO.head_reference(logits, feat, labels, tg[ii], tg2[ii], gout, B, 1.0, 0.1, 0.0)
        s = base['CT_i'].sort().values
        M = float(0.5 * (s[B // 2 - 1] + s[B // 2]))
    ref, gl, gf = TO.head_reference(logits, feat, labels, tg[ii], tg2[ii], gout, B, 1.0, 0.1, M)
    active = int((ref['CT_i'] > 0).sum())
    assert (0 < active < B) if split else active == B
    pred, pred2 = torch.zeros(N, nc), torch.zeros(N, Fd)
    out8 = TO._te_head_fwd(logits, feat, labels, idx, tg, tg2, pred, pred2, B, 1.0, 0.1, M)
    assert out8.shape == (8,) and out8[7].item() == 0.0
    for k, name in enumerate(TO.SCALARS):
        assert abs(out8[k].item() - ref[name].item()) <= 2e-6 * max(1.0, abs(ref[name].item())), name
    assert torch.equal(pred[ii], logits[B:2 * B]) and torch.equal(pred2[ii], feat[B:2 * B])
    rest = torch.ones(N, dtype=torch.bool); rest[ii] = False
    assert pred[rest].abs().max().item() == 0.0 and pred2[rest].abs().max().item() == 0.0
    g1, g2 = TO._te_head_bwd(logits, feat, labels, idx, tg, tg2, gout, B, 1.0, 0.1, M)
    assert O._rel_l2(g1, gl) < 1e-5 and O._rel_l2(g2, gf) < 1e-5
    assert g2[:B].abs().max().item() == 0.0 and g2[2 * B:].abs().max().item() == 0.0
    # the closed form the kernel implements, for an unlabelled row
    p, q = torch.softmax(logits[B:2 * B].double(), 1), torch.softmax(tg[ii].double(), 1)
    w = (ref['CT_i'] > 0).double() * 0.5 * gout[1].item() * 1.0 / B
    lse = torch.logsumexp(logits[B:2 * B].double(), 1)
    want = (0.5 * gout[1].item() / B) * ((torch.sigmoid(lse) - 1)[:, None] * p) + w[:, None] * (2.0 / nc) * p * ((p - q) - ((p - q) * p).sum(1, keepdim=True))
    assert (want - gl[B:2 * B]).abs().max().item() < 1e-12
    wantf = w[:, None] * 0.1 * 2 * (feat[B:2 * B].double() - tg2[ii].double()) / Fd
    assert (wantf - gf[B:2 * B]).abs().max().item() < 1e-12


def test_stand_in_ensemble_update_and_bias_correction():
    g = torch.Generator().manual_seed(1)
    ens, tg, pred = torch.randn(5, 3, generator=g), torch.zeros(5, 3), torch.randn(5, 3, generator=g)
    e_ref, t_ref = TO.ensemble_reference(ens, pred, 0.6, 2)
    TO._te_ensemble_update(ens, tg, pred, 0.6, 2)
    assert (ens.double() - e_ref).abs().max().item() < 1e-6 and (tg.double() - t_ref).abs().max().item() < 1e-6 and pred.abs().max().item() == 0.0
    # a constant prediction is its own target after every epoch
    ens, tg = torch.zeros(4), torch.zeros(4)
    for epoch in range(3):
        TO._te_ensemble_update(ens, tg, torch.full((4,), 1.5), 0.6, epoch)
        assert (tg - 1.5).abs().max().item() < 1e-6


# ----------------------------------------------------------------------------------------------------- literals
def test_config_literals():
    import ctgan_amd.ct_cifar as M
    import ctgan_amd.ct_cifar_te as T
    c = T.Config()
    assert (c.INIT_ROWS, c.LAMBDA_2, c.FACTOR_M, c.FEAT_WEIGHT, c.PREDICTION_DECAY) == (1000, 1.0, 0.0, 0.1, 0.6)
    assert (c.SEED, c.SEED_DATA, c.COUNT, c.BATCH_SIZE, c.UNLABELED_WEIGHT, c.LR, c.BETA1, c.BETA2) == (2, 2, 400, 100, 1., 0.0003, 0.5, 0.999)
    assert (c.AVG_RATE, c.EPOCHS, c.Z_DIM, c.PAD, c.DROP_IN, c.DROP_HIDDEN, c.G_INIT_STDV, c.D_INIT_STDV, c.N_CLASSES) == (1e-4, 1000, 50, 2, 0.2, 0.5, 0.1, 0.1, 10)
    assert (c.IMG, c.D_WIDTHS, c.G_WIDTHS) == (32, (128, 128, 128, 256, 256, 256, 512, 256, 128), (512, 256, 128))
    with pytest.raises(AttributeError):
        T.Config(NOPE=1)
    # ct_cifar's own literals are untouched by the subclass, and configure() of either module installs its own object
    assert (M.Config.INIT_ROWS, M.Config.FEAT_WEIGHT) == (500, 0.05) and not hasattr(M.Config, 'PREDICTION_DECAY')
    try:
        assert T.configure(BATCH_SIZE=7) is M.cfg and M.cfg.INIT_ROWS == 1000
        assert M.configure() is M.cfg and M.cfg.INIT_ROWS == 500 and type(M.cfg) is M.Config
    finally:
        T.configure(); M.configure()


# ----------------------------------------------------------------------------------------------------- trainer against the oracle
def test_steps_match_the_oracle_on_the_stand_ins(te_kernels):
    TO.small_cfg()
    got = {}
    assert TO.run_steps('cpu', log=print, golden=got) == 21 + 9
    with np.load(GOLDEN) as want:
        TO.golden_matches(got, want)


def test_oracle_equals_the_golden_file():
    import ctgan_amd.ct_cifar_te as T
    cfg = T.Config(**TO.SMALL)
    with np.load(GOLDEN) as want:
        assert TO.golden_matches(TO.oracle_golden(cfg), want) > 20
        assert float(want['d/loss_ct']) > 0 and np.abs(want['d/epoch_pred2']).max() > 0
    assert os.path.getsize(GOLDEN) < 200 * 1024


# ----------------------------------------------------------------------------------------------------- the tables' quirks
def _arrays(n=40, n_test=8, seed=0, size=16):
    r = np.random.RandomState(seed)
    return {'x_train': r.randint(0, 256, (n, 3, size, size)).astype(np.uint8), 'y_train': np.arange(n) % 10,
            'x_test': r.randint(0, 256, (n_test, 3, size, size)).astype(np.uint8), 'y_test': np.arange(n_test) % 10}


def _idx(*v):
    return torch.tensor(v, dtype=torch.int32)


def _trainer(a, seed=3):
    import ctgan_amd.ct_cifar_te as T
    import ctgan_amd.tflib as lib
    lib.delete_all_params()
    tr = T.CifarTETrainer(seed=seed, data=a['x_train'])
    return tr


def test_epoch_zero_targets_are_uniform_and_zero(te_kernels):
    """No ramp-up: in epoch 0 the tables are zeros, so the class target is the uniform distribution and the feature target 0."""
    cfg = TO.small_cfg()
    tr = _trainer(_arrays())
    assert all(t.abs().max().item() == 0.0 for t in tr.tables().values()) and tr.epoch == 0
    assert tr.targets.shape == (40, 10) and tr.targets2.shape == (40, cfg.D_WIDTHS[-1])
    tr.init_params(tr.gather_fixed(torch.arange(12, dtype=torch.int32), cfg.IMG + 2 * cfg.PAD, (0, 0)))
    i_unl = _idx(7, 8, 30, 39)
    tr.d_opt.set_lr(cfg.LR)
    out = tr.d_losses(tr.gather(_idx(0, 5, 9, 2), 16), _idx(1, 2, 3, 4), tr.gather(i_unl, 17), i_unl)
    B, nc = 4, cfg.N_CLASSES
    u, f = out['logits'][B:2 * B].detach().double(), out['features'][B:2 * B].detach().double()
    ct = ((torch.softmax(u, 1) - 1.0 / nc) ** 2).mean()
    ctf = (f ** 2).mean()
    assert abs(out['ct'].item() - ct.item()) < 1e-6 and abs(out['ctf'].item() - ctf.item()) < 1e-5 * max(1.0, ctf.item())
    assert abs(out['loss_ct'].item() - (ct + 0.1 * ctf).item()) < 1e-5 * max(1.0, ctf.item())
    assert torch.equal(tr.epoch_pred[i_unl.long()], out['logits'][B:2 * B].detach())


def test_unvisited_rows_decay(te_kernels):
    """A row no batch of an epoch visited contributes a zero prediction: its ensemble shrinks by the decay."""
    cfg = TO.small_cfg()
    tr = _trainer(_arrays())
    tr.init_params(tr.gather_fixed(torch.arange(12, dtype=torch.int32), cfg.IMG + 2 * cfg.PAD, (0, 0)))
    first, second = _idx(7, 8, 30, 39), _idx(1, 8, 2, 3)
    tr.train_iteration_idx(_idx(0, 5, 9, 2), _idx(1, 2, 3, 4), first, _idx(11, 12, 13, 14))
    p0 = tr.epoch_pred.clone()
    tr.end_epoch()
    assert tr.epoch == 1 and tr.epoch_pred.abs().max().item() == 0.0 and tr.epoch_pred2.abs().max().item() == 0.0
    assert torch.allclose(tr.ensemble, 0.4 * p0, rtol=1e-6, atol=0) and torch.allclose(tr.targets, p0, rtol=1e-6, atol=1e-9)
    assert tr.targets[0].abs().max().item() == 0.0                       # never visited: still the zero target
    tr.train_iteration_idx(_idx(0, 5, 9, 2), _idx(1, 2, 3, 4), second, _idx(11, 12, 13, 14))
    p1 = tr.epoch_pred.clone()
    tr.end_epoch()
    assert torch.allclose(tr.ensemble[7], 0.6 * 0.4 * p0[7], rtol=1e-6, atol=0)                       # visited in epoch 0 only
    assert torch.allclose(tr.targets[7], 0.24 * p0[7] / 0.64, rtol=1e-6, atol=0)
    assert torch.allclose(tr.ensemble[8], 0.24 * p0[8] + 0.4 * p1[8], rtol=1e-5, atol=1e-7)          # visited in both
    assert torch.allclose(tr.ensemble2[1], 0.4 * tr.targets2[1] * 0.64 / 0.4, rtol=1e-5, atol=1e-7) and tr.ensemble2[1].abs().max().item() > 0


# ----------------------------------------------------------------------------------------------------- loop, checkpoint
def test_train_runs_two_short_epochs_on_arrays(te_kernels, tmp_path):
    import ctgan_amd.ct_cifar_te as T
    TO.small_cfg(COUNT=2, EPOCHS=2)
    lines = []
    tr = T.train(arrays=_arrays(), epochs=2, use_graphs=False, out_dir=str(tmp_path), log=lines.append, max_batches=2)
    assert len(lines) == 2 and lines[0].startswith('Epoch 0, time = ') and lines[1].startswith('Epoch 1, time = ')
    for key in ('loss_lab = ', 'loss_unl = ', 'train err = ', 'train err2 = ', 'gen loss = ', 'test err = '):
        assert key in lines[0]
    assert tr.d_opt.t == tr.g_opt.t == 4 and tr.iteration == 4 and tr.epoch == 2
    assert tr.targets.abs().max().item() > 0 and tr.epoch_pred.abs().max().item() == 0.0
    assert int((tr.ensemble.abs().sum(1) > 0).sum()) <= 2 * 2 * 4            # two shortened epochs of two batches of four rows
    assert os.path.isfile(tmp_path / 'checkpoint.pt') and os.path.isfile(tmp_path / 'log.jsonl')
    from ctgan_amd import checkpoint
    extra = checkpoint.load_extra(str(tmp_path / 'checkpoint.pt'))
    assert extra['te_epoch'] == 2 and torch.equal(extra['targets2'], tr.targets2.cpu())


def test_checkpoint_round_trip_restores_tables_and_epoch(te_kernels, tmp_path):
    import ctgan_amd.tflib as lib
    from ctgan_amd import checkpoint
    cfg = TO.small_cfg()
    a = _arrays()
    batch = (_idx(0, 5, 9, 2), _idx(1, 2, 3, 4), _idx(7, 8, 30, 39), _idx(11, 12, 13, 14))
    tr = _trainer(a)
    tr.init_params(tr.gather_fixed(torch.arange(12, dtype=torch.int32), cfg.IMG + 2 * cfg.PAD, (0, 0)))
    tr.train_iteration_idx(*batch)
    tr.end_epoch()
    path = str(tmp_path / 'c.pt')
    checkpoint.save(path, tr, 1, extra=tr.te_state())
    out1 = tr.train_iteration_idx(*batch)                      # the second epoch sees the first one's targets
    tr.end_epoch()
    want = {n: p.detach().clone() for n, p in lib._params.items()}
    want_tab = {n: t.clone() for n, t in tr.tables().items()}
    tr2 = _trainer(a)
    assert checkpoint.load(path, tr2) == 1
    assert tr2.epoch == 0 and tr2.targets.abs().max().item() == 0.0          # checkpoint.load alone knows nothing of the tables
    tr2.load_te_state(checkpoint.load_extra(path))
    assert tr2.epoch == 1 and tr2.targets.abs().max().item() > 0
    out2 = tr2.train_iteration_idx(*batch)
    tr2.end_epoch()
    assert torch.equal(out1['out8'], out2['out8']) and out1['loss_ct'].item() > 0
    for n, p in lib._params.items():
        assert torch.equal(p.detach(), want[n]), n
    for n, t in tr2.tables().items():
        assert torch.equal(t, want_tab[n]), n
    assert tr2.epoch == tr.epoch == 2
    with pytest.raises(ValueError):
        _trainer(_arrays(n=30)).load_te_state(checkpoint.load_extra(path))
