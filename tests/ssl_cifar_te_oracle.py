"""Torch restatement (fp64 by default, autograd) of the temporal-ensembling CT classifier - TH/CT_CIFAR-10_TE.py (TH/ =
CT-GANs/Theano_classifier of the reference) - on top of tests/ssl_cifar_oracle.py, whose network, generator, State, dropout masks and
gather reference it imports: the classifier step against target rows (:102-126), the per-example tables and their epoch-end update
(:177-180, :273-276, :300-309), the loop.  Plus CPU stand-ins of the three kernel wrappers ctgan_amd.kernels gained for it, so that
the host logic of ctgan_amd.ct_cifar_te runs without a GPU.  TEST INFRASTRUCTURE ONLY.  Written from the script's mathematics, cited
by line; nothing of its text is reused.
"""
import collections

import numpy as np
import torch

from tests import ssl_cifar_oracle as O
from tests.ssl_cifar_oracle import (SID_AUG_LAB, SID_AUG_UNL, State, _rel_l2, aug_draws, classifier, d_names, g_names, gather_reference,  # noqa: F401
                                    generator, golden_matches, log_sum_exp, make_params, site_masks, softplus, uniforms, update_ok)

SCALARS = ('loss_lab', 'loss_unl', 'loss_ct', 'train_err', 'train_err2', 'ct', 'ctf')


# ------------------------------------------------------------------------------------------------------------ the loss head
def te_terms(logits, feat, labels, t, t2, B, lam2, feat_w, M):
    """:106-126 written out, on logits [3B, nc] / features [3B, F] = [lab ; unl ; fake] and the target rows t [B, nc], t2 [B, F] of
    the unlabelled examples (constants) -> dict of scalars plus the per-row hinge arguments CT_i."""
    lab, unl, fk = logits[:B], logits[B:2 * B], logits[2 * B:]
    idx = labels.long()
    loss_lab = -lab[torch.arange(B), idx].mean() + log_sum_exp(lab).mean()
    ct_i = ((torch.softmax(unl, 1) - torch.softmax(t.detach(), 1)) ** 2).mean(dim=1)
    ctf_i = ((feat[B:2 * B] - t2.detach()) ** 2).mean(dim=1)
    CT_i = lam2 * (ct_i + feat_w * ctf_i) - M
    CT = torch.clamp(CT_i, min=0).mean()
    l_unl = log_sum_exp(unl)
    loss_unl = 0.5 * (CT - l_unl.mean() + softplus(l_unl).mean() + softplus(log_sum_exp(fk)).mean())
    dt = logits.dtype
    return {'loss_lab': loss_lab, 'loss_unl': loss_unl, 'loss_ct': CT, 'train_err': (lab.argmax(dim=1) != idx).to(dt).mean(),
            'train_err2': (lab.max(dim=1).values <= 0).to(dt).mean(), 'ct': ct_i.mean(), 'ctf': ctf_i.mean(), 'CT_i': CT_i}


def out8_of(terms):
    return torch.stack([terms[k] for k in SCALARS] + [torch.zeros((), dtype=terms['loss_lab'].dtype)])


def head_reference(logits, feat, labels, t, t2, gout, B, lam2, feat_w, M):
    """fp64 autograd of the written-out expression -> (terms, glogits, gfeat) of gout[0] loss_lab + gout[1] loss_unl."""
    x, f = logits.double().clone().requires_grad_(True), feat.double().clone().requires_grad_(True)
    terms = te_terms(x, f, labels, t.double(), t2.double(), B, lam2, feat_w, M)
    gl, gf = torch.autograd.grad(gout[0] * terms['loss_lab'] + gout[1] * terms['loss_unl'], [x, f])
    return {k: v.detach() for k, v in terms.items()}, gl, gf


def ensemble_reference(ens, pred, decay, epoch):
    """:305-306 in fp64 -> (ens, targets)."""
    e = decay * ens.double() + (1.0 - decay) * pred.double()
    return e, e / (1.0 - decay ** (epoch + 1.0))


# ------------------------------------------------------------------------------------------------------------ step and state
def d_losses(P, cfg, x_lab, labels, x_unl, t, t2, seed, step):
    """:102-126 on one stacked batch [lab ; unl ; fake]: sites 0 (z), 1 (input dropout over 3B rows), 2, 3."""
    dtype, B = x_lab.dtype, x_lab.shape[0]
    with torch.no_grad():
        fake = generator(P, cfg, uniforms(seed, 0, step, B, cfg.Z_DIM, dtype))
    x_all = torch.cat([x_lab, x_unl, fake], 0)
    logits, feat = classifier(P, cfg, x_all, site_masks(cfg, seed, step, 3 * B, x_all.shape[2], 1, dtype), features='both')
    out = te_terms(logits, feat, labels, t, t2, B, cfg.LAMBDA_2, cfg.FEAT_WEIGHT, cfg.FACTOR_M)
    out.update({'logits': logits, 'features': feat, 'cost': out['loss_lab'] + cfg.UNLABELED_WEIGHT * out['loss_unl']})
    return out


def d_grads(P, cfg, x_lab, labels, x_unl, t, t2, seed, step):
    names = d_names(cfg)[1]
    Q = O._with_grad(P, names)
    out = d_losses(Q, cfg, x_lab, labels, x_unl, t, t2, seed, step)
    grads = torch.autograd.grad(out['cost'], [Q[n] for n in names])
    return {k: v.detach() for k, v in out.items()}, dict(zip(names, grads))


class TEState(State):
    """ssl_cifar_oracle.State plus the six tables over n_rows examples and the epoch count."""

    def __init__(self, P, cfg, seed, n_rows, dtype=torch.float64):
        super().__init__(P, cfg, seed, dtype)
        z = lambda w: torch.zeros(n_rows, w, dtype=dtype)          # noqa: E731
        nc, fd = cfg.N_CLASSES, cfg.D_WIDTHS[-1]
        self.tab = {'ensemble': z(nc), 'ensemble2': z(fd), 'targets': z(nc), 'targets2': z(fd), 'epoch_pred': z(nc), 'epoch_pred2': z(fd)}
        self.epoch = 0

    def d_step(self, x_lab, labels, x_unl, i_unl):
        ii, B = torch.as_tensor(i_unl).long(), x_lab.shape[0]
        out, grads = d_grads(self.P, self.cfg, x_lab.to(self.dtype), labels, x_unl.to(self.dtype), self.tab['targets'][ii], self.tab['targets2'][ii],
                             self.seed, self.step)
        self.tab['epoch_pred'][ii] = out['logits'][B:2 * B]          # :300-302
        self.tab['epoch_pred2'][ii] = out['features'][B:2 * B]
        self._apply(self.dn, grads, 'd')
        return out, grads

    def end_epoch(self):
        d = self.cfg.PREDICTION_DECAY
        for s in ('', '2'):
            self.tab['ensemble' + s], self.tab['targets' + s] = ensemble_reference(self.tab['ensemble' + s], self.tab['epoch_pred' + s], d, self.epoch)
            self.tab['ensemble' + s], self.tab['targets' + s] = self.tab['ensemble' + s].to(self.dtype), self.tab['targets' + s].to(self.dtype)
            self.tab['epoch_pred' + s] = torch.zeros_like(self.tab['epoch_pred' + s])          # :273-274
        self.epoch += 1


# ------------------------------------------------------------------------------------------------------------ CPU stand-ins
def _te_head_fwd(logits, feat, labels, idx, targets, targets2, pred, pred2, B, lam2, feat_w, M):
    ii = idx.long()
    terms = te_terms(logits.detach(), feat.detach(), labels, targets[ii], targets2[ii], B, lam2, feat_w, M)
    with torch.no_grad():
        pred[ii] = logits.detach()[B:2 * B]
        pred2[ii] = feat.detach()[B:2 * B]
    return out8_of(terms)


def _te_head_bwd(logits, feat, labels, idx, targets, targets2, gout, B, lam2, feat_w, M):
    ii = idx.long()
    x, f = logits.detach().clone().requires_grad_(True), feat.detach().clone().requires_grad_(True)
    with torch.enable_grad():
        terms = te_terms(x, f, labels, targets[ii], targets2[ii], B, lam2, feat_w, M)
        gl, gf = torch.autograd.grad(terms['loss_lab'] * gout[0] + terms['loss_unl'] * gout[1], [x, f])
    return gl, gf


def _te_ensemble_update(ens, targets, pred, decay, epoch):
    with torch.no_grad():
        ens.mul_(float(decay)).add_(pred * (1.0 - float(decay)))
        targets.copy_(ens * (1.0 / (1.0 - float(decay) ** (int(epoch) + 1))))
        pred.zero_()


STAND_INS = {'te_head_fwd': _te_head_fwd, 'te_head_bwd': _te_head_bwd, 'te_ensemble_update': _te_ensemble_update}


def install_stand_ins(monkeypatch):
    """ssl_cifar_oracle's stand-ins plus the three above (on top of `cpu_kernels`)."""
    import ctgan_amd.kernels as K
    O.install_stand_ins(monkeypatch)
    for name, fn in STAND_INS.items():
        monkeypatch.setattr(K, name, fn)


SMALL = dict(IMG=16, D_WIDTHS=(32, 32, 32, 64, 64, 64, 96, 64, 32), G_WIDTHS=(64, 32, 32), BATCH_SIZE=4, INIT_ROWS=12)


def small_cfg(**kw):
    """Reduced sizes for the host tests and the GPU step parity (those of ssl_cifar_oracle.small_cfg)."""
    import ctgan_amd.ct_cifar_te as T
    d = dict(SMALL)
    d.update(kw)
    return T.configure(**d)


# ------------------------------------------------------------------------------------------------------------ step parity
N_ROWS = 9          # table rows of the step parity


def step_inputs(cfg, seed):
    """ssl_cifar_oracle.step_inputs plus B distinct table rows and NON-ZERO target tables (so that the consistency gradient is
    exercised): (x_init, x_lab, x_unl, x_unl2, labels, i_unl, targets [N_ROWS, nc], targets2 [N_ROWS, F])."""
    x_init, x_lab, x_unl, x_unl2, labels = O.step_inputs(cfg, seed)
    g = torch.Generator().manual_seed(seed + 100)
    i_unl = torch.randperm(N_ROWS, generator=g)[:cfg.BATCH_SIZE].to(torch.int32)
    targets = torch.randn(N_ROWS, cfg.N_CLASSES, generator=g)
    targets2 = torch.rand(N_ROWS, cfg.D_WIDTHS[-1], generator=g) * 0.5
    return x_init, x_lab, x_unl, x_unl2, labels, i_unl, targets, targets2


def _golden_step(out, ref, gref, which, keys):
    out.update({'%s/%s' % (which, k): ref[k].numpy() for k in keys})
    out.update({'%s/grad/%s' % (which, n): g.float().numpy() for n, g in gref.items() if g.numel() <= 512})


def run_steps(dev, seed=5, cost_tol=2e-4, grad_tol=3e-3, log=None, golden=None):
    """The data-dependent init, one classifier step and one generator step of ctgan_amd.ct_cifar_te.CifarTETrainer (under the module's
    current Config, on `dev`) against the fp64 oracle on the same Philox streams and the same non-zero target tables, teacher-forced
    as ssl_cifar_oracle.run_steps, with its tolerances: scalars within cost_tol * max(1, |ref|); the prediction rows written by the
    step within cost_tol * max(1, max |ref|) and every other row untouched; gradients within relative L2 max(grad_tol, 3 x the fp32
    twin's error); updates and averages by `update_ok`; only the step's trainable set moves.  Returns the number of parameters checked."""
    import ctgan_amd.ct_cifar_te as T
    import ctgan_amd.tflib as lib
    cfg = T.cfg
    say = log or (lambda *a: None)
    x_init, x_lab, x_unl, x_unl2, labels, i_unl, tg, tg2 = step_inputs(cfg, seed)
    to_dev = lambda x: T.C.rot180(x.to(dev))          # noqa: E731
    lib.delete_all_params(); lib.set_seed(11)
    tr = T.CifarTETrainer(seed=seed, data=np.zeros((N_ROWS, cfg.CHANNELS, cfg.IMG, cfg.IMG), dtype=np.uint8))
    tr.targets.copy_(tg); tr.targets2.copy_(tg2)
    P = make_params(cfg, seed=seed, dtype=torch.float32)
    O.load_into_registry(P, cfg)
    st = TEState(P, cfg, seed, N_ROWS)
    st.tab['targets'], st.tab['targets2'] = tg.double(), tg2.double()
    reg = lambda n: O.unrelabel(n, lib._params[n].detach().cpu(), cfg).double()          # noqa: E731
    checked = 0
    # ---- init
    tr.init_params(to_dev(x_init))
    st.init(x_init)
    for n in st.P:
        if n.endswith('.W') or n.endswith('.bn_b'):
            assert torch.equal(reg(n), P[n].double()), ('init moved', n)
        else:
            e = (reg(n) - st.P[n]).abs().max().item()
            say('init', n, 'max abs err', e)
            assert e <= 2e-4 * max(1.0, st.P[n].abs().max().item()), ('init', n, e)
    if golden is not None:
        golden.update({'init/' + n: st.P[n].numpy() for n in O._golden_init_names(cfg)})
    assert int(tr.rng.ctr.item()) == st.step == 2
    avg_before = None
    for which in ('d', 'g'):
        lib.load_state_dict(collections.OrderedDict((n, O.relabel(n, v, cfg).float()) for n, v in st.P.items()), strict=True)
        before = {n: reg(n) for n in st.P}
        st.P = collections.OrderedDict((n, before[n].clone()) for n in st.P)       # the oracle continues from the fp32-rounded weights
        P32 = collections.OrderedDict((n, v.float()) for n, v in st.P.items())
        step = st.step
        if which == 'd':
            tr.d_opt.set_lr(cfg.LR)
            out, grads = tr.d_grads(to_dev(x_lab), labels.to(dev), to_dev(x_unl), i_unl.to(dev))
            tr.d_opt.update(grads, rng=tr.rng)
            ref, gref = st.d_step(x_lab, labels, x_unl, i_unl)
            ii = i_unl.long()
            _, gtw = d_grads(P32, cfg, x_lab.float(), labels, x_unl.float(), tg[ii], tg2[ii], seed, step)
            names, opt, keys = st.dn, tr.d_opt, SCALARS
            assert ref['loss_ct'].item() > 0
            for s in ('', '2'):
                got, want = getattr(tr, 'epoch_pred' + s).detach().cpu().double(), st.tab['epoch_pred' + s]
                e = (got - want).abs().max().item()
                say('d', 'epoch_pred' + s, 'max abs err', e)
                assert e <= cost_tol * max(1.0, want.abs().max().item()) and want[ii].abs().max().item() > 0
                rest = torch.ones(N_ROWS, dtype=torch.bool); rest[ii] = False
                assert got[rest].abs().max().item() == 0.0
                if golden is not None:
                    golden['d/epoch_pred' + s] = want[ii].float().numpy()
        else:
            tr.g_opt.set_lr(cfg.LR)
            out, grads = tr.g_grads(to_dev(x_unl2))
            tr.g_opt.update(grads, rng=tr.rng)
            ref, gref = st.g_step(x_unl2)
            _, gtw = O.g_grads(P32, cfg, x_unl2.float(), seed, step)
            names, opt, keys = st.gn, tr.g_opt, ('loss_gen',)
        for k in keys:
            a, b = out[k].item(), ref[k].item()
            say(which, k, a, b)
            assert abs(a - b) <= cost_tol * max(1.0, abs(b)), (k, a, b)
        if golden is not None:
            _golden_step(golden, ref, gref, which, keys)
        assert [n for n, _ in (tr.d_named if which == 'd' else tr.g_named)] == names
        gp = {n: O.unrelabel(n, g.detach().cpu(), cfg) for n, g in zip(names, grads) if g is not None}
        for n in names:
            assert n in gp, ('no gradient', n)
            tol = max(grad_tol, 3 * _rel_l2(gtw[n], gref[n]))
            e = _rel_l2(gp[n], gref[n])
            say(which, 'grad', n, 'rel L2', e, 'bound', tol)
            assert (gp[n].double() - gref[n]).norm().item() <= tol * gref[n].norm().item() + 2e-6, (which, n, e, tol)
        avgs = {n: O.unrelabel(n, a.detach().cpu(), cfg).double() for n, a in opt.avg_views()} if opt.avg is not None else {}
        for n in st.P:
            new = reg(n)
            if n not in names:
                assert torch.equal(new, before[n]), ('outside the trainable set, yet moved', which, n)
                continue
            ok, how = update_ok(new, before[n], st.P[n], gref[n], gp[n])
            say(which, 'update', n, how)
            assert ok, (which, 'update', n, how)
            if which == 'd':
                ok, how = update_ok(avgs[n], before[n], st.avg[n], gref[n], gp[n], scale=cfg.AVG_RATE)
                say(which, 'average', n, how)
                assert ok, (which, 'average', n, how)
            checked += 1
        if which == 'g':      # the generator step leaves the classifier's averages and every table alone
            for n, a in tr.d_opt.avg_views():
                assert torch.equal(a.detach().cpu().double(), avg_before[n]), ('generator step moved an average', n)
            for n, t in tr.tables().items():
                assert torch.equal(t, tab_before[n]), ('generator step moved a table', n)
        avg_before = {n: a.detach().cpu().double().clone() for n, a in tr.d_opt.avg_views()}
        tab_before = {n: t.clone() for n, t in tr.tables().items()}
        assert int(tr.rng.ctr.item()) == st.step
    return checked


def oracle_golden(cfg, seed=5):
    """The oracle alone over the sequence run_steps drives (the weights rounded to fp32 between the steps), as the name -> array dict
    run_steps collects in `golden` (tests/golden/ssl_cifar_te_step.npz)."""
    x_init, x_lab, x_unl, x_unl2, labels, i_unl, tg, tg2 = step_inputs(cfg, seed)
    st = TEState(make_params(cfg, seed=seed, dtype=torch.float32), cfg, seed, N_ROWS)
    st.tab['targets'], st.tab['targets2'] = tg.double(), tg2.double()
    st.init(x_init)
    out = {'init/' + n: st.P[n].numpy() for n in O._golden_init_names(cfg)}
    rnd = lambda: collections.OrderedDict((n, v.float().double()) for n, v in st.P.items())      # noqa: E731
    st.P = rnd()
    ref, gref = st.d_step(x_lab, labels, x_unl, i_unl)
    ii = i_unl.long()
    out['d/epoch_pred'], out['d/epoch_pred2'] = st.tab['epoch_pred'][ii].float().numpy(), st.tab['epoch_pred2'][ii].float().numpy()
    _golden_step(out, ref, gref, 'd', SCALARS)
    st.P = rnd()
    ref, gref = st.g_step(x_unl2)
    _golden_step(out, ref, gref, 'g', ('loss_gen',))
    return out


# ------------------------------------------------------------------------------------------------------------ short multi-epoch loop
# Chosen on the CPU from the oracle alone (fp64, and its fp32 twin as a check that the outcome does not hang on rounding).
# ssl_cifar_oracle.LOOP_CFG with this script's head classifies every test image after the first epoch, but at its learning rate of
# 0.001 (and at 0.0005, 0.0003, with D_INIT_STDV 0.5 or UNLABELED_WEIGHT 0.3) the later epochs jump between minima: loss_lab spikes to
# 0.8 .. 3 within an epoch and the live-weight error after an epoch is 0.06 .. 0.55 in one precision and 0 in the other.  At 0.0002
# both descend smoothly - loss_lab at most 1.13, 0.25, 0.11, 0.04 over the last ten iterations of epochs 0..3 in fp64 and 1.13, 0.26,
# 0.10, 0.06 in fp32 - with live-weight error 0.020 / 0.025 after epoch 0 and 0.0 after every later one (checked through six epochs).
# Four epochs of 20 batches, so that the targets of epochs 1..3 are ensembles of earlier predictions; about 5 s of fp64 oracle time.
LOOP_CFG = dict(O.LOOP_CFG, LR=0.0002)
LOOP_EPOCHS = 4
LOOP_TRAIN = 400          # 20 batches of 20 per epoch


def loop_epochs(cfg, data, epochs, seed=1, max_batches=None):
    """(init rows, [[(i_lab, labels, i_unl, i_unl2) per batch] per epoch]) through ctgan_amd.ct_cifar.CifarSSLData's epoch streams."""
    import ctgan_amd.ct_cifar as M
    d = M.CifarSSLData(arrays=data, count=data['count'], seed=seed, seed_data=seed)
    out, init_idx = [], None
    for _ in range(epochs):
        n = d.begin_epoch()
        n = n if max_batches is None else min(n, max_batches)
        if init_idx is None:
            init_idx = d.init_indices().copy()
        out.append([tuple(np.ascontiguousarray(a) for a in d.batch(t)) for t in range(n)])
    return init_idx, out


def loop_oracle(cfg, data, init_idx, epochs, seed=3, dtype=torch.float64):
    """The oracle over the loop -> (live-weight test error, averaged-weight test error, [loss_lab per iteration], the state)."""
    tx, S, pad = data['x_train'], cfg.IMG, cfg.PAD
    st = TEState(make_params(cfg, seed=seed, dtype=torch.float32), cfg, seed, len(tx), dtype)
    t = lambda a: torch.from_numpy(a).to(dtype)          # noqa: E731
    st.init(t(gather_reference(tx, init_idx, S + 2 * pad, pad, offset=(0, 0))))
    B, trace = cfg.BATCH_SIZE, []
    for batches in epochs:
        for i_lab, y, i_unl, i_unl2 in batches:
            x_lab = gather_reference(tx, i_lab, S, pad, aug_draws(seed, SID_AUG_LAB, st.step, B, pad))
            x_unl = gather_reference(tx, i_unl, S, pad, aug_draws(seed, SID_AUG_UNL, st.step, B, pad))
            out, _ = st.d_step(t(x_lab), torch.from_numpy(y), t(x_unl), i_unl)
            trace.append(float(out['loss_lab']))
            x_unl2 = gather_reference(tx, i_unl2, S, pad, aug_draws(seed, SID_AUG_LAB, st.step, B, pad))
            st.g_step(t(x_unl2))
        st.end_epoch()
    xs = t(gather_reference(data['x_test'], np.arange(len(data['x_test'])), S, pad))
    return st.test_error(xs, data['y_test'], averaged=False), st.test_error(xs, data['y_test'], averaged=True), trace, st


def loop_product(cfg, data, init_idx, epochs, dev, seed=3, graphed=False):
    """The product over the same loop, same weights and streams -> (live-weight, averaged-weight test error, [loss_lab], the trainer)."""
    import ctgan_amd.ct_cifar_te as T
    import ctgan_amd.tflib as lib
    lib.delete_all_params()
    tr = T.CifarTETrainer(seed=seed, data=data['x_train'])
    O.load_into_registry(make_params(cfg, seed=seed, dtype=torch.float32), cfg)
    idx = torch.from_numpy(np.ascontiguousarray(init_idx)).to(dev)
    tr.init_params(tr.gather_fixed(idx, cfg.IMG + 2 * cfg.PAD, (0, 0)))
    step = tr
    if graphed:
        from ctgan_amd.engine import GraphedCifarTETrainer
        step = GraphedCifarTETrainer(tr)
        assert step.graphed, step.graph_error
    trace = []
    for batches in epochs:
        for b in batches:
            args = [torch.from_numpy(a) for a in b]
            out = step.train_iteration(*args) if graphed else tr.train_iteration_idx(*[a.to(dev) for a in args])
            trace.append(out['loss_lab'].clone())
        tr.end_epoch()
    trace = [float(v) for v in torch.stack(trace).cpu()]
    bs = len(data['y_test'])
    return (tr.test_error(data['x_test'], data['y_test'], averaged=False, batch_size=bs),
            tr.test_error(data['x_test'], data['y_test'], batch_size=bs), trace, tr)
