"""The temporal-ensembling CT classifier on the MI355X (`-m gpu`): the three kernels of csrc/ssl_te.hip against fp64 (the scattered
prediction rows bit for bit, out-of-range labels and indices, rows at +-80), functional.te_head through autograd, init + one
classifier step against non-zero target tables + one generator step at reduced sizes against the oracle
(tests/ssl_cifar_te_oracle.py) on shared Philox streams and pinned to tests/golden/ssl_cifar_te_step.npz, a full-size run whose graph
replay equals eager and whose resumed run equals the uninterrupted one bit for bit - all six tables included -, a short graphed
multi-epoch loop on synthetic data against the oracle's, and train() on arrays.  Kernel bounds are those of
tests/test_gpu_ssl_cifar.py: 2e-5 relative for forward scalars, 3e-5 relative L2 for gradients."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import ssl_cifar_oracle as O  # noqa: E402
from tests import ssl_cifar_te_oracle as TO  # noqa: E402

FWD_TOL, GRAD_TOL = 2e-5, 3e-5
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'ssl_cifar_te_step.npz')
LAM2, FEAT_W = 1.0, 0.1


@pytest.fixture
def K():
    import ctgan_amd.kernels as K
    return K


@pytest.fixture
def clean():
    import ctgan_amd.ct_cifar as M
    import ctgan_amd.ct_cifar_te as T
    import ctgan_amd.tflib as lib
    lib.delete_all_params()
    yield T
    T.configure(); M.configure(); lib.delete_all_params(); lib.delete_param_aliases()


def dev(t):
    return t.to('cuda')


def _guarded(rows, width, fill):
    """A contiguous [rows, width] device table between two guard rows -> (table, whole buffer)."""
    buf = fill(rows + 2, width).to('cuda')
    return buf[1:rows + 1], buf


def _head_case(B, nc, Fd, N, seed=0):
    """Random logits / features / targets, every seventh row of logits and of targets at +-80, distinct indices (a permutation's slice)."""
    g = torch.Generator().manual_seed(seed + B + nc + Fd + N)
    logits, feat = torch.randn(3 * B, nc, generator=g) * 2, torch.randn(3 * B, Fd, generator=g)
    tg, tg2 = torch.randn(N, nc, generator=g) * 2, torch.randn(N, Fd, generator=g)
    big = lambda rows: torch.where(torch.rand(rows, nc, generator=g) > 0.5, 80.0, -80.0)          # noqa: E731
    logits[::7] = big(len(logits[::7]))
    tg[::7] = big(len(tg[::7]))
    labels = torch.randint(0, nc, (B,), generator=g, dtype=torch.int32)
    idx = torch.randperm(N, generator=g)[:B].to(torch.int32)
    return logits, feat, labels, idx, tg, tg2, g


HEAD_SHAPES = [(100, 10, 128, 1000), (3, 5, 7, 11), (4, 10, 32, 16), (257, 10, 128, 600)]


# ----------------------------------------------------------------------------------------------------- head
@pytest.mark.parametrize('B,nc,Fd,N', HEAD_SHAPES)
@pytest.mark.parametrize('split', [False, True])
def test_head_fwd_bwd_against_fp64(K, B, nc, Fd, N, split):
    logits, feat, labels, idx, tg, tg2, g = _head_case(B, nc, Fd, N)
    ii = idx.long()
    gout = torch.tensor([0.7, 1.3, 9.0, 9.0, 9.0, 9.0, 9.0, 9.0])
    M = 0.0
    if split:          # midway between the two middle hinge arguments of the fp64 reference at M = 0: no row sits on the kink
        s = TO.head_reference(logits, feat, labels, tg[ii], tg2[ii], gout, B, LAM2, FEAT_W, 0.0)[0]['CT_i'].sort().values
        M = float(0.5 * (s[B // 2 - 1] + s[B // 2]))
    ref, rgl, rgf = TO.head_reference(logits, feat, labels, tg[ii], tg2[ii], gout, B, LAM2, FEAT_W, M)
    active = int((ref['CT_i'] > 0).sum())
    print('active hinge rows', active, 'of', B, 'M', M)
    assert (0 < active < B) if split else active == B
    rnd = lambda r, c: torch.randn(r, c, generator=g)          # noqa: E731
    (pred, pbuf), (pred2, pbuf2) = _guarded(N, nc, rnd), _guarded(N, Fd, rnd)
    (dtg, tbuf), (dtg2, tbuf2) = _guarded(N, nc, rnd), _guarded(N, Fd, rnd)
    dtg.copy_(tg); dtg2.copy_(tg2)
    before = [b.clone() for b in (pbuf, pbuf2, tbuf, tbuf2)]
    dl, df, dy, di = dev(logits), dev(feat), dev(labels), dev(idx)
    out8 = K.te_head_fwd(dl, df, dy, di, dtg, dtg2, pred, pred2, B, LAM2, FEAT_W, M).cpu()
    assert torch.isfinite(out8).all() and out8[7].item() == 0.0
    for k, name in enumerate(TO.SCALARS):
        a, b = out8[k].item(), ref[name].item()
        print(name, a, b)
        assert abs(a - b) <= FWD_TOL * abs(b), (name, a, b)
    # the scatter: bit-equal rows, everything else (guard rows and the read-only tables included) untouched
    assert torch.equal(pred[di.long()], dl[B:2 * B]) and torch.equal(pred2[di.long()], df[B:2 * B])
    for buf, was, written in ((pbuf, before[0], True), (pbuf2, before[1], True), (tbuf, before[2], False), (tbuf2, before[3], False)):
        keep = torch.ones(N + 2, dtype=torch.bool, device='cuda')
        if written:
            keep[di.long() + 1] = False
        assert torch.equal(buf[keep], was[keep])
    gl, gf = K.te_head_bwd(dl, df, dy, di, dtg, dtg2, dev(gout), B, LAM2, FEAT_W, M)
    el, ef = O._rel_l2(gl.cpu(), rgl), O._rel_l2(gf.cpu(), rgf)
    print('grad rel L2', el, ef)
    assert el < GRAD_TOL and ef < GRAD_TOL
    assert gf[:B].abs().max().item() == 0.0 and gf[2 * B:].abs().max().item() == 0.0


@pytest.mark.parametrize('B,nc,Fd,N', [(100, 10, 128, 1000), (3, 5, 7, 11)])
def test_head_out_of_range_label_and_index(K, B, nc, Fd, N):
    """A label outside [0, nc) makes loss_lab NaN, an index outside [0, N) loss_unl, CT_, mean ct and mean ctf; neither reads or
    writes anything it should not: after a valid call has filed the batch's rows, a call with the bad value leaves every table -
    guard rows included - byte-identical to a copy taken before it."""
    logits, feat, labels, idx, tg, tg2, g = _head_case(B, nc, Fd, N, seed=1)
    rnd = lambda r, c: torch.randn(r, c, generator=g)          # noqa: E731
    (pred, pbuf), (pred2, pbuf2) = _guarded(N, nc, rnd), _guarded(N, Fd, rnd)
    (dtg, tbuf), (dtg2, tbuf2) = _guarded(N, nc, rnd), _guarded(N, Fd, rnd)
    dtg.copy_(tg); dtg2.copy_(tg2)
    dl, df, dy, di = dev(logits), dev(feat), dev(labels), dev(idx)
    good = K.te_head_fwd(dl, df, dy, di, dtg, dtg2, pred, pred2, B, LAM2, FEAT_W, 0.0).cpu()
    assert torch.isfinite(good).all()
    before = [b.clone() for b in (pbuf, pbuf2, tbuf, tbuf2)]
    gout = dev(torch.tensor([1.0, 1.0]))
    for bad_label in (nc, -1):
        y = dy.clone(); y[B // 2] = bad_label
        out8 = K.te_head_fwd(dl, df, y, di, dtg, dtg2, pred, pred2, B, LAM2, FEAT_W, 0.0).cpu()
        assert torch.isnan(out8[0]) and torch.equal(out8[1:3], good[1:3]) and torch.equal(out8[4:], good[4:])
        assert all(torch.equal(b, w) for b, w in zip((pbuf, pbuf2, tbuf, tbuf2), before))
    for bad_idx in (N, -1, 2 ** 31 - 1):
        i2 = di.clone(); i2[B // 2] = bad_idx
        out8 = K.te_head_fwd(dl, df, dy, i2, dtg, dtg2, pred, pred2, B, LAM2, FEAT_W, 0.0).cpu()
        assert torch.isnan(out8[[1, 2, 5, 6]]).all() and torch.equal(out8[[0, 3, 4, 7]], good[[0, 3, 4, 7]])
        assert all(torch.equal(b, w) for b, w in zip((pbuf, pbuf2, tbuf, tbuf2), before))
        gl, gf = K.te_head_bwd(dl, df, dy, i2, dtg, dtg2, gout, B, LAM2, FEAT_W, 0.0)
        r = B + B // 2
        assert torch.isnan(gl[r]).all() and torch.isnan(gf[r]).all()
        assert torch.isfinite(gl[:r]).all() and torch.isfinite(gl[r + 1:]).all() and torch.isfinite(gf[:r]).all() and torch.isfinite(gf[r + 1:]).all()
    # duplicate indices (what the engine's warm-up stages) stay inside the tables: one of the rows survives
    dup = torch.zeros_like(di)
    K.te_head_fwd(dl, df, dy, dup, dtg, dtg2, pred, pred2, B, LAM2, FEAT_W, 0.0)
    assert any(torch.equal(pred[0], dl[B + i]) for i in range(B))
    keep = torch.ones(N + 2, dtype=torch.bool, device='cuda'); keep[1] = False
    assert torch.equal(pbuf[keep], before[0][keep]) and torch.equal(pbuf2[keep], before[1][keep])


def test_wrappers_refuse_what_they_cannot_index(K):
    B, nc, Fd, N = 4, 10, 32, 16
    logits, feat, labels, idx, tg, tg2, _ = _head_case(B, nc, Fd, N)
    z = lambda *s: torch.zeros(*s, device='cuda')          # noqa: E731
    args = [dev(logits), dev(feat), dev(labels), dev(idx), dev(tg), dev(tg2), z(N, nc), z(N, Fd)]
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        K.te_head_fwd(logits, *args[1:], B, LAM2, FEAT_W, 0.0)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        K.te_ensemble_update(torch.zeros(4), z(4), z(4), 0.6, 0)
    for k, bad in ((4, z(nc, N).t()), (7, z(N, 2 * Fd)[:, :Fd]), (3, dev(idx).long()), (6, z(N + 1, nc))):
        a = list(args); a[k] = bad
        with pytest.raises((AssertionError, TypeError)):
            K.te_head_fwd(*a, B, LAM2, FEAT_W, 0.0)
    with pytest.raises(AssertionError):
        K.te_ensemble_update(z(4, 6)[:, :3], z(4, 3), z(4, 3), 0.6, 0)


def test_te_head_autograd(K):
    import ctgan_amd.functional as F
    B, nc, Fd, N = 4, 10, 32, 16
    logits, feat, labels, idx, tg, tg2, _ = _head_case(B, nc, Fd, N, seed=2)
    ii = idx.long()
    dl, df = dev(logits).requires_grad_(True), dev(feat).requires_grad_(True)
    dtg, dtg2 = dev(tg).requires_grad_(True), dev(tg2)                  # a target table that asks for a gradient gets none
    pred, pred2 = torch.zeros(N, nc, device='cuda'), torch.zeros(N, Fd, device='cuda')
    out8 = F.te_head(dl, df, dev(labels), dev(idx), dtg, dtg2, pred, pred2, B, LAM2, FEAT_W, 0.0)
    seed = torch.tensor([1.0, 0.5, 0, 0, 0, 0, 0, 0])
    gl, gf = torch.autograd.grad(out8, [dl, df], dev(seed))
    ref, rgl, rgf = TO.head_reference(logits, feat, labels, tg[ii], tg2[ii], seed, B, LAM2, FEAT_W, 0.0)
    assert O._rel_l2(gl.cpu(), rgl) < GRAD_TOL and O._rel_l2(gf.cpu(), rgf) < GRAD_TOL
    assert torch.equal(pred[dev(idx).long()], dl.detach()[B:2 * B]) and not pred.requires_grad
    out8 = F.te_head(dl, df, dev(labels), dev(idx), dtg, dtg2, pred, pred2, B, LAM2, FEAT_W, 0.0)
    assert torch.autograd.grad(out8[1], dtg, allow_unused=True)[0] is None


# ----------------------------------------------------------------------------------------------------- ensemble update
@pytest.mark.parametrize('n,offset', [(1, 0), (63, 0), (64 * 4 + 3, 0), (64 * 4 + 3, 1), (1000 * 138, 0)])
def test_ensemble_update(K, n, offset):
    """offset 1: the three tensors start one element into their buffers, so no pointer is 16-byte aligned (the all-scalar path)."""
    g = torch.Generator().manual_seed(n)
    ens, pred = torch.rand(n, generator=g) + 0.5, torch.rand(n, generator=g) + 0.5          # positive: the bound below is per element
    bufs = [torch.full((n + offset + 4,), 7.0, device='cuda') for _ in range(3)]
    de, dt, dp = (b[offset:offset + n] for b in bufs)
    de.copy_(ens); dp.copy_(pred)
    for epoch in (0, 3):
        e_ref, t_ref = TO.ensemble_reference(de.cpu(), dp.cpu(), 0.6, epoch)
        K.te_ensemble_update(de, dt, dp, 0.6, epoch)
        assert ((de.cpu().double() - e_ref).abs() / e_ref).max().item() < 1e-6 and ((dt.cpu().double() - t_ref).abs() / t_ref).max().item() < 1e-6
        assert dp.abs().max().item() == 0.0
        dp.copy_(pred)
    for b in bufs:
        assert (b[:offset] == 7.0).all() and (b[offset + n:] == 7.0).all()


def test_ensemble_update_reproduces_a_constant_prediction(K):
    c = (torch.rand(1000, 138, generator=torch.Generator().manual_seed(0)) + 0.5).cuda()
    ens, tg, pred = torch.zeros_like(c), torch.zeros_like(c), torch.zeros_like(c)
    for epoch in range(2):
        pred.copy_(c)
        K.te_ensemble_update(ens, tg, pred, 0.6, epoch)
        assert ((tg - c).abs() / c).max().item() < 1e-6 and pred.abs().max().item() == 0.0


# ----------------------------------------------------------------------------------------------------- steps, graphs, loop
def test_steps_match_the_oracle_and_the_committed_fixture(clean):
    """Init, one classifier step against non-zero target tables and one generator step at small_cfg(), teacher-forced on shared
    streams, with the tolerances and the update_ok rule of tests/test_gpu_ssl_cifar.py; the oracle's outputs in the same run equal
    tests/golden/ssl_cifar_te_step.npz."""
    TO.small_cfg()
    got = {}
    assert TO.run_steps('cuda', cost_tol=2e-4, grad_tol=3e-3, log=print, golden=got) == 21 + 9
    with np.load(GOLDEN) as want:
        assert TO.golden_matches(got, want) > 20


def _state(tr):
    import ctgan_amd.tflib as lib
    s = {'p/' + n: p.detach().clone() for n, p in lib._params.items()}
    for w, o in (('d', tr.d_opt), ('g', tr.g_opt)):
        for i, b in enumerate(o.slots()):
            s['%s/slot%d' % (w, i)] = b.clone()
        s[w + '/t'] = torch.tensor(o.t)
    s['ctr'] = tr.rng.ctr.clone()
    s['epoch'] = torch.tensor(tr.epoch)
    s.update({'table/' + n: t.clone() for n, t in tr.tables().items()})
    return s


def _full_size_run(T, data, batches, init_idx, graphed, resume=None, save=None):
    """init on the padded rows, three iterations, end_epoch, [checkpoint], one more iteration -> (trainer, engine, [outputs])."""
    import ctgan_amd.tflib as lib
    from ctgan_amd import checkpoint
    from ctgan_amd.engine import GraphedCifarTETrainer
    lib.delete_all_params(); lib.set_seed(3)
    tr = T.CifarTETrainer(seed=9, data=data)
    outs = []
    if resume is None:
        tr.init_params(tr.gather_fixed(dev(init_idx), T.cfg.IMG + 2 * T.cfg.PAD, (0, 0)))
        eng = GraphedCifarTETrainer(tr, use_graphs=graphed)
        for b in batches[:3]:
            outs.append({n: v.clone() for n, v in eng.train_iteration(*b).items()})
        tr.end_epoch()
        if save:
            checkpoint.save(save, tr, 1, extra=tr.te_state())
    else:
        assert checkpoint.load(resume, tr) == 1
        tr.load_te_state(checkpoint.load_extra(resume))
        eng = GraphedCifarTETrainer(tr, use_graphs=graphed)
    outs.append({n: v.clone() for n, v in eng.train_iteration(*batches[3]).items()})
    return tr, eng, outs


def test_full_size_graph_replay_equals_eager_and_resume(clean, tmp_path):
    """B 100, the script's widths, N 1000: init on 1000 padded rows, three iterations on slices of permutations, end_epoch(), one
    more iteration (which reads the non-zero targets).  Graph replay equals eager bit for bit in every parameter, average, Adam
    slot, counter and all six tables; a run resumed from a checkpoint written after end_epoch() equals the uninterrupted one."""
    T = clean
    T.configure()
    r = np.random.RandomState(1)
    data = r.randint(0, 256, size=(1000, 3, 32, 32)).astype(np.uint8)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a).astype(np.int32))          # noqa: E731
    perm = [r.permutation(1000) for _ in range(6)]
    sl = lambda p, k: t(perm[p][100 * k:100 * (k + 1)])          # noqa: E731
    batches = [(sl(0, k), t(r.randint(0, 10, 100)), sl(1, k), sl(2, k)) for k in range(3)] + [(sl(3, 0), t(r.randint(0, 10, 100)), sl(4, 0), sl(5, 0))]
    init_idx = t(r.permutation(1000))
    ck = str(tmp_path / 'c.pt')
    tr, eng, outs_e = _full_size_run(T, data, batches, init_idx, graphed=False, save=ck)
    assert not eng.graphed and tr.epoch == 1 and tr.iteration == 4
    eager = _state(tr)
    assert tr.d_opt.skipped() == 0 and tr.g_opt.skipped() == 0
    for o in outs_e:
        for n, v in o.items():
            assert torch.isfinite(v).all(), n
        print('eager', {n: float(v) for n, v in o.items() if v.numel() == 1})
    assert outs_e[3]['ctf'].item() != outs_e[0]['ctf'].item() and eager['table/targets'].abs().max().item() > 0
    visited = torch.cat([b[2] for b in batches[:3]]).long()
    untouched = torch.ones(1000, dtype=torch.bool); untouched[visited] = False
    assert eager['table/targets2'][untouched.cuda()].abs().max().item() == 0.0 and eager['table/targets2'][visited.cuda()].abs().min(dim=1).values.max().item() > 0
    assert int((eager['table/epoch_pred'].abs().sum(1) > 0).sum()) == 100
    tr, eng, outs_g = _full_size_run(T, data, batches, init_idx, graphed=True)
    assert eng.graphed, eng.graph_error
    assert tr.d_opt.skipped() == 0
    graph = _state(tr)
    assert sorted(graph) == sorted(eager)
    for n in eager:
        assert torch.equal(graph[n], eager[n]), ('graph replay differs from eager', n)
    for a, b in zip(outs_e, outs_g):
        for n in a:
            assert torch.equal(a[n], b[n]), n
    tr, eng, outs_r = _full_size_run(T, data, batches, init_idx, graphed=True, resume=ck)
    assert eng.graphed, eng.graph_error
    resumed = _state(tr)
    for n in eager:
        if n not in ('d/t', 'g/t'):
            assert torch.equal(resumed[n], eager[n]), ('resumed run differs', n)
    assert (tr.d_opt.t, tr.g_opt.t) == (int(eager['d/t']), int(eager['g/t']))
    for n in outs_e[3]:
        assert torch.equal(outs_r[0][n], outs_e[3][n]), n


def test_short_multi_epoch_loop_on_synthetic_data_against_the_oracle(clean):
    """LOOP_EPOCHS graphed epochs at LOOP_CFG on class-prototype images, so that ensembled targets feed back: the configuration was
    chosen on the CPU from the oracle alone (its live-weight test error on the test examples is at most 0.05, asserted here); the
    product's live-weight error is within 0.025 (the existing loop tests' margin) of the oracle's, and its target tables after the
    last end_epoch() are finite and non-zero."""
    T = clean
    cfg = T.configure(**TO.LOOP_CFG)
    data = O.synthetic_data(cfg, n_train=TO.LOOP_TRAIN)
    init_idx, epochs = TO.loop_epochs(cfg, data, TO.LOOP_EPOCHS)
    assert len(epochs) >= 3
    ref_live, ref_avg, ref_trace, st = TO.loop_oracle(cfg, data, init_idx, epochs)
    print('oracle live %.4f averaged %.4f loss_lab %.4f -> %.4f' % (ref_live, ref_avg, ref_trace[0], ref_trace[-1]))
    assert ref_live <= 0.05
    live, avg, trace, tr = TO.loop_product(cfg, data, init_idx, epochs, 'cuda', graphed=True)
    print('product live %.4f averaged %.4f loss_lab %.4f -> %.4f' % (live, avg, trace[0], trace[-1]))
    assert all(np.isfinite(trace))
    assert abs(live - ref_live) <= 0.025
    assert tr.epoch == TO.LOOP_EPOCHS
    for n in ('targets', 'targets2', 'ensemble', 'ensemble2'):
        t = getattr(tr, n)
        assert torch.isfinite(t).all() and t.abs().max().item() > 0, n
    assert tr.epoch_pred.abs().max().item() == 0.0


def test_train_on_arrays(clean, tmp_path):
    """train() on a tiny synthetic set: two shortened epochs, the report lines, the optimiser step counts, the tables, a resume."""
    import ctgan_amd.tflib as lib
    T = clean
    cfg = T.configure(**dict(TO.LOOP_CFG, COUNT=3, EPOCHS=3))
    data = O.synthetic_data(cfg, n_train=200, n_test=40)
    arrays = {k: data[k] for k in ('x_train', 'y_train', 'x_test', 'y_test')}
    lines = []
    tr = T.train(arrays=arrays, epochs=2, out_dir=str(tmp_path), log=lines.append, max_batches=3)
    assert len(lines) == 2 and lines[0].startswith('Epoch 0, time = ') and lines[1].startswith('Epoch 1, time = ')
    for key in ('loss_lab = ', 'loss_unl = ', 'train err = ', 'train err2 = ', 'gen loss = ', 'test err = '):
        assert key in lines[1]
    assert tr.d_opt.t == tr.g_opt.t == 6 and tr.iteration == 6 and tr.d_opt.skipped() == 0 and tr.epoch == 2
    assert 0 < int((tr.ensemble.abs().sum(1) > 0).sum()) <= 2 * 3 * cfg.BATCH_SIZE and tr.epoch_pred.abs().max().item() == 0.0
    want = {n: p.detach().clone() for n, p in lib._params.items()}
    want_tab = {n: t.clone() for n, t in tr.tables().items()}
    # resumed from the checkpoint of epoch 1... which is the final one: nothing left to run, weights and tables are the saved ones
    tr2 = T.train(arrays=arrays, epochs=2, out_dir=None, resume=str(tmp_path / 'checkpoint.pt'), log=lines.append, max_batches=3)
    assert len(lines) == 2 and tr2.d_opt.t == 6 and tr2.epoch == 2
    for n, p in lib._params.items():
        assert torch.equal(p.detach(), want[n]), n
    for n, t in tr2.tables().items():
        assert torch.equal(t, want_tab[n]), n
    # ... and one further epoch from it runs, on the restored targets
    tr3 = T.train(arrays=arrays, epochs=3, out_dir=None, resume=str(tmp_path / 'checkpoint.pt'), log=lines.append, max_batches=3)
    assert len(lines) == 3 and lines[2].startswith('Epoch 2, time = ') and tr3.epoch == 3 and tr3.d_opt.t == 9
