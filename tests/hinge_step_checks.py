"""Step-level checks of the hinge objective (gan_cifar_resnet.Trainer / dcgan_step.DCGANTrainer `objective='hinge'`; NOT in the reference),
shared by tests/test_hinge_host.py (the CPU stand-ins, tests/hinge_cpu_kernels.py) and tests/test_gpu_hinge_step.py / tests/test_gpu_trainers_hinge.py (the device).  A plain
helper module: no fixtures, no marks; every check takes the device.

fp64 reference: oracle.nets.resnet_discriminator, oracle.steps.resnet_real_prep, tests/projection_oracle.py for the projected head and

    L_D = mean_i max(0, 1 - D(x_i)) + mean_i max(0, 1 + D(G(z_i)))   [+ ACGAN_SCALE * CE(class head of the real rows)]

with the hinge torch.where(t >= 0, t, 0), ONE dropout pass (the draws `u_pass1`).  Bounds are those of the existing tests named at each check."""
import numpy as np
import torch

from oracle import nets as onets, steps as osteps, tf_ops, tflib_ref as oref
from tests import projection_oracle as PO
from tests.loss_heads_cases import hinge

HEADS = {'acgan': dict(), 'uncond': dict(CONDITIONAL=False, ACGAN=False), 'proj': dict(CONDITIONAL=True, ACGAN=False, PROJECTION=True)}


def oracle_from_product(lib, dtype=torch.float64):
    reg = oref.Registry(dtype=dtype)
    for n, p in lib._params.items():
        t = p.detach().cpu().clone().to(dtype)
        trainable = n not in lib._non_trainable
        t.requires_grad_(trainable)
        reg[n] = t
        if not trainable:
            reg.non_trainable.add(n)
    return reg


def cmp(a, b, tol, what, atol=1e-7):
    a = a.detach().cpu().double().reshape(-1); b = b.detach().cpu().double().reshape(-1)
    err, scale = (a - b).abs().max().item(), b.abs().max().item()
    assert err <= tol * scale + atol, '%s: max err %.3e vs scale %.3e' % (what, err, scale)


def cmp_l2(a, b, tol, what, atol=1e-9):
    a = a.detach().cpu().double().reshape(-1); b = b.detach().cpu().double().reshape(-1)
    err, scale = (a - b).norm().item(), b.norm().item()
    assert err <= tol * scale + atol, '%s: L2 err %.3e vs norm %.3e' % (what, err, scale)


def rel_l2(a, b):
    a = a.detach().cpu().double().reshape(-1); b = b.detach().cpu().double().reshape(-1)
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


def to_dev(o, dev):
    if isinstance(o, list):
        return [to_dev(t, dev) for t in o]
    return o.float().to(dev)


def build(R, lib, dev, dim, B, seed=5, dim_g=None, **kw):
    lib.delete_all_params(); lib.set_device('cpu' if dev == 'cpu' else None); lib.set_seed(seed)
    R.configure(DIM_G=dim_g or dim, DIM_D=dim, BATCH_SIZE=B, **kw)
    R.build_params()


def shake(lib, seed=5):
    """biases are zero-initialised in the reference, the projection table small: make them count"""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for n, p in lib._params.items():
            if n.endswith(('.Biases', '.b')):
                p.add_((0.1 * torch.randn(p.shape, generator=g)).to(p.device))
            if n == PO.TABLE:
                p.copy_((0.3 * torch.randn(p.shape, generator=g)).to(p.device))


def batch(B, dev, seed=5):
    nrng = np.random.default_rng(seed)
    return (torch.from_numpy(nrng.integers(0, 256, (B, 3072), dtype=np.int32)).to(dev),
            torch.from_numpy(nrng.integers(0, 10, (B,), dtype=np.int32)).to(dev))


# ------------------------------------------------------------------------------------------------------------------ fp64 reference
def ref_d_losses(reg, cfg, real_int, labels, rnd, B, ACGAN_SCALE=1.0):
    h = B // 2
    with torch.no_grad():
        fake = torch.cat([onets.resnet_generator(reg, cfg, h, labels[i * h:(i + 1) * h], rnd['z'][i]) for i in range(2)], 0)
    real = osteps.resnet_real_prep(real_int, rnd['dequant'])
    rf = torch.cat([real, fake], 0)
    lab2 = torch.cat([labels, labels], 0)
    d, f, a = onets.resnet_discriminator(reg, cfg, rf, lab2, 0.8, 0.5, 0.5, rnd['u_pass1'])
    if getattr(cfg, 'PROJECTION_HEAD', False):
        d = PO.projected(reg, d, f, lab2)
    hr, hf = hinge(1.0 - d[:B]).mean(), hinge(1.0 + d[B:]).mean()
    out = dict(wgan=hr + hf, hinge_real=hr, hinge_fake=hf, fake=fake, real=real, d_real=d[:B], d_fake=d[B:], acgan=None)
    cost = hr + hf
    if cfg.CONDITIONAL and cfg.ACGAN:
        out['acgan'] = tf_ops.sparse_softmax_ce(a[:B], labels).mean()
        cost = cost + ACGAN_SCALE * out['acgan']
        out['acc_real'] = (a[:B].argmax(1) == labels).double().mean()
        out['acc_fake'] = (a[B:].argmax(1) == labels).double().mean()
    out['cost'] = cost
    return out


def oracle_cfg(dim, heads_kw, **more):
    kw = {k: v for k, v in heads_kw.items() if k != 'PROJECTION'}
    cfg = onets.ResnetCfg(DIM_G=dim, DIM_D=dim, **kw, **more)
    cfg.PROJECTION_HEAD = bool(heads_kw.get('PROJECTION'))
    return cfg


# ------------------------------------------------------------------------------------------------------------------ parity with fp64
def check_parity(R, lib, dev, heads, norm_d=False, dim=64, B=8):
    """Injected draws (the op-by-op path) against fp64.  Bounds: test_d_and_g_step_parity_teacher_forced's - scalars 2e-4 with atol 1e-6,
    gradients rel-L2 2e-3 (atol 1e-7) - for every head and for the Layernorm critic alike.  Every figure is printed before it is asserted."""
    kw = dict(HEADS[heads], **({'NORMALIZATION_D': True} if norm_d else {}))
    build(R, lib, dev, dim, B, **kw)
    shake(lib)
    if norm_d:          # a Layernorm critic's fresh outputs are large: every fake hinge would be off.  A smaller output weight keeps both sides live
        with torch.no_grad():
            lib._params['Discriminator.Output.W'].mul_(0.1)
    reg = oracle_from_product(lib)
    cfg = oracle_cfg(dim, HEADS[heads], **({'NORMALIZATION_D': True} if norm_d else {}))
    g = torch.Generator().manual_seed(11)
    real = torch.randint(0, 256, (B, 3072), generator=g, dtype=torch.int32)
    labels = torch.randint(0, 10, (B,), generator=g, dtype=torch.int32)
    rnd = osteps.make_rnd_resnet_d(B, dim, g)
    tr = R.Trainer(seed=1, objective='hinge')
    tr.rng.begin_step()
    out, grads = tr.d_grads(real.to(dev), labels.to(dev), {k: to_dev(v, dev) for k, v in rnd.items()})
    ref = ref_d_losses(reg, cfg, real, labels, rnd, B)
    assert 'ct' not in out and 'gp' not in out and 'slopes' not in out and 'gp_grads' not in out
    assert ref['hinge_real'].item() > 0 and ref['hinge_fake'].item() > 0, 'a side of the objective is switched off in the reference'
    margin = torch.cat([1.0 - ref['d_real'], 1.0 + ref['d_fake']]).detach().abs().min().item()
    assert margin >= 1e-4, ('a hinge within 1e-4 of its kink', margin)
    s_tol, g_tol = 2e-4, 2e-3
    for k in ('cost', 'wgan', 'hinge_real', 'hinge_fake', 'acgan'):
        assert (out[k] is None) == (ref[k] is None), k
        if ref[k] is not None:
            print('parity %s norm_d=%s %s: %.9g vs %.9g' % (heads, norm_d, k, out[k].item(), ref[k].item()))
            cmp(out[k], ref[k], s_tol, 'd_losses.' + k, atol=1e-6)
    if ref['acgan'] is not None:
        cmp(out['acc_real'], ref['acc_real'], 0, 'acc_real', atol=1.01 / B)          # argmax ties only
        cmp(out['acc_fake'], ref['acc_fake'], 0, 'acc_fake', atol=1.01 / B)
    else:
        assert out['acc_real'] is None and out['acc_fake'] is None
    cmp(out['real'], ref['real'], 1e-6, 'real')
    want = PO.grads_of(reg, ref['cost'], 'Discriminator.')
    got = {n: gv for (n, _), gv in zip(tr.d_named, grads) if gv is not None}
    assert set(got) == set(want), set(got) ^ set(want)
    print('parity %s norm_d=%s: largest gradient rel-L2 %.3g' % (heads, norm_d, max(rel_l2(got[n], want[n]) for n in want if want[n].abs().max() > 0)))
    for n in want:
        cmp_l2(got[n], want[n], g_tol, 'dgrad ' + n, atol=1e-7)


# ------------------------------------------------------------------------------------------------------------------ hand schedule == autograd
def scheduled_vs_autograd(R, lib, dev, dim, B, heads, **trainer_kw):
    """-> {hand: (out, grads, names)} from identical weights, inputs and Philox streams; asserts which path ran"""
    import ctgan_amd.functional as F
    import ctgan_amd.hinge_schedule as HS
    res = {}
    for hand in (False, True):
        build(R, lib, dev, dim, B, seed=1, dim_g=min(dim, 32) if dev == 'cpu' else None, **HEADS[heads])
        shake(lib)
        tr = R.Trainer(seed=3, objective='hinge', **trainer_kw)
        real, labels = batch(B, dev)
        if heads == 'proj' and B >= 4:
            labels = labels.clone(); labels[2] = labels[0]                     # a repeated class
        calls = []
        orig_u, orig = HS.usable, HS.critic_step
        if not hand:
            HS.usable = lambda *a: False
        HS.critic_step = lambda *a, **k: (calls.append(1), orig(*a, **k))[1]
        try:
            F.prepare_filters()
            fake = tr.generate_fakes(labels)[0]
            tr.rng.begin_step()
            out, grads = tr.d_grads(real, labels, fake=fake)
        finally:
            HS.usable, HS.critic_step = orig_u, orig
            if tr.spectral is not None:
                tr.detach_spectral()
        assert bool(calls) == hand, 'the critic step did not take the form under test'
        res[hand] = (out, grads, [n for n, _ in tr.d_named])
    return res


def check_scheduled_equals_autograd(R, lib, dev, dim, B, heads, **trainer_kw):
    """Bounds of test_hand_scheduled_critic_step_equals_the_autograd_path_on_gpu: scalars 1e-5 (atol 1e-6), every gradient rel-L2 < 2e-5; the
    None-pattern of grads is equal."""
    res = scheduled_vs_autograd(R, lib, dev, dim, B, heads, **trainer_kw)
    a, b = res[False], res[True]
    assert set(a[0]) == set(b[0]) and 'ct' not in b[0] and 'gp' not in b[0]
    for k in ('cost', 'wgan', 'hinge_real', 'hinge_fake', 'acgan', 'acc_real', 'acc_fake', 'd_real', 'd_fake', 'real'):
        assert (a[0][k] is None) == (b[0][k] is None), k
        if a[0][k] is not None:
            cmp(b[0][k], a[0][k], 1e-5, 'scheduled.' + k, atol=1e-6)
    assert a[2] == b[2]
    n_checked = 0
    for n, x, y in zip(a[2], a[1], b[1]):
        assert (x is None) == (y is None), n
        if x is None:
            continue
        if x.abs().max() > 0:
            assert rel_l2(y, x) < 2e-5, (n, rel_l2(y, x))
            n_checked += 1
        else:                                                                  # exact zeros under autograd: exact zeros by hand
            assert float(y.abs().max()) == 0.0, (n, float(y.abs().max()))
    assert n_checked >= 20
    if heads == 'proj':
        i = b[2].index(PO.TABLE)
        zero_a, zero_b = a[1][i].abs().sum(dim=1) == 0, b[1][i].abs().sum(dim=1) == 0
        assert torch.equal(zero_a, zero_b) and bool(zero_b.any()) and bool((~zero_b).any())     # absent classes: exact zero rows on both paths


# ------------------------------------------------------------------------------------------------------------------ shared dequantisation site
def check_real_is_the_ct_steps_real(R, lib, dev, dim=64, B=8):
    outs = {}
    for obj in (None, 'hinge'):
        build(R, lib, dev, dim, B, seed=1, dim_g=min(dim, 32) if dev == 'cpu' else None)
        tr = R.Trainer(seed=3, objective=obj)
        real, labels = batch(B, dev)
        for step in range(2):                                                  # step 0 and step 1 of the Philox counter
            out = tr.d_step(real, labels, iteration=step)
            outs[(obj, step)] = (out['real'].clone(), out['fake'].clone() if step == 0 else None)
    assert torch.equal(outs[(None, 0)][0], outs[('hinge', 0)][0]) and torch.equal(outs[(None, 0)][1], outs[('hinge', 0)][1])
    assert torch.equal(outs[(None, 1)][0], outs[('hinge', 1)][0]) and not torch.equal(outs[(None, 0)][0], outs[(None, 1)][0])


# ------------------------------------------------------------------------------------------------------------------ off is off
def _feed(batches):
    k = [0]

    def nxt():
        k[0] += 1
        return batches[k[0] % len(batches)]
    return nxt


def check_off_is_off_resnet(R, lib, dev, dim=16, B=8):
    batches = [batch(B, dev, seed=s) for s in (7, 8, 9)]
    res = []
    for kw in ({}, {'objective': None}):
        build(R, lib, dev, dim, B, seed=4)
        tr = R.Trainer(seed=9, **kw)
        nxt = _feed(batches)
        outs = [tr.train_iteration(it, nxt) for it in range(2)]
        res.append((tr, outs, tr.d_opt.theta.clone(), tr.g_opt.theta.clone(), sorted(tr.d_opt.state_dict()), sorted(tr.g_opt.state_dict()),
                    len(tr.d_opt.slots()), len(tr.g_opt.slots())))
    a, b = res
    assert a[0].objective is None and b[0].objective is None
    assert torch.equal(a[2], b[2]) and torch.equal(a[3], b[3]) and a[4:] == b[4:]
    for oa, ob in zip(a[1], b[1]):
        assert list(oa) == list(ob) and 'ct' in oa and 'gp' in oa and 'hinge_real' not in oa
        for k in oa:
            if k == 'grads':
                for n in oa[k]:
                    assert (oa[k][n] is None) == (ob[k][n] is None) and (oa[k][n] is None or torch.equal(oa[k][n], ob[k][n])), n
            else:
                assert (oa[k] is None) == (ob[k] is None) and (oa[k] is None or torch.equal(oa[k], ob[k])), k


def check_off_is_off_dcgan(M, lib, dev, dim=8, B=4):
    from ctgan_amd.dcgan_step import CT_MODE, DCGANTrainer, build_params
    g = torch.Generator().manual_seed(3)
    reals = [torch.rand(B, 784, generator=g).to(dev) for _ in range(3)]
    res = []
    try:
        for kw in ({}, {'objective': None}):
            lib.delete_all_params(); lib.set_device('cpu' if dev == 'cpu' else None); lib.set_seed(4)
            M.configure(DIM=dim, BATCH_SIZE=B)
            build_params(M)
            tr = DCGANTrainer(M, seed=9, **kw)
            nxt = _feed(reals)
            outs = [tr.train_iteration(it, nxt) for it in range(2)]
            res.append((tr.mode, outs, tr.d_opt.theta.clone(), tr.g_opt.theta.clone(), sorted(tr.d_opt.state_dict()), len(tr.d_opt.slots())))
    finally:
        M.configure(); lib.delete_all_params()
    a, b = res
    assert a[0] == b[0] == CT_MODE and torch.equal(a[2], b[2]) and torch.equal(a[3], b[3]) and a[4:] == b[4:]
    for oa, ob in zip(a[1], b[1]):
        assert list(oa) == list(ob) and 'ct' in oa and 'gp' in oa
        assert torch.equal(oa['cost'], ob['cost'])
        for n in oa['grads']:
            assert (oa['grads'][n] is None) == (ob['grads'][n] is None) and (oa['grads'][n] is None or torch.equal(oa['grads'][n], ob['grads'][n])), n


# ------------------------------------------------------------------------------------------------------------------ DCGAN family
def check_dcgan_hinge(lib, which, dev, dim=32, B=6, cost_tol=2e-4, d_tol=3e-3, g_tol=5e-3):
    """DCGANTrainer(objective='hinge') on gan_mnist / gan_cifar: critic and generator cost and gradients on injected draws against an fp64
    restatement built from oracle.steps' DCGAN pieces (the draws of make_rnd_dcgan_d / _g, the nets of oracle.nets) - D(real) under u_real,
    D(fake) under u_fake - within tests/test_gpu_gan_modes.py's bounds (cost 2e-4 max(1, |ref|); gradients rel-L2 3e-3 critic / 5e-3 generator,
    + 2e-6)."""
    from ctgan_amd.dcgan_step import HINGE_MODE, DCGANTrainer, build_params
    g = torch.Generator().manual_seed(31)
    if which == 'mnist':
        import ctgan_amd.gan_mnist as M
        G = lambda reg, n, z: onets.mnist_generator(reg, n, z, DIM=dim)               # noqa: E731
        D = lambda reg, x, u: onets.mnist_discriminator(reg, x, u, DIM=dim)           # noqa: E731
        real_in = torch.rand(B, 784, generator=g)
        real_o = real_in.double()
    else:
        import ctgan_amd.gan_cifar as M
        G = lambda reg, n, z: onets.cifar_generator(reg, n, z, DIM=dim)               # noqa: E731
        D = lambda reg, x, u: onets.cifar_discriminator(reg, x, u, DIM=dim)           # noqa: E731
        real_in = torch.randint(0, 256, (B, 3072), generator=g, dtype=torch.int32)
        real_o = 2 * ((real_in.double() / 255.) - .5)
    try:
        lib.delete_all_params(); lib.set_device('cpu' if dev == 'cpu' else None); lib.set_seed(13)
        M.configure(DIM=dim, BATCH_SIZE=B)
        build_params(M)
        tr = DCGANTrainer(M, seed=1, objective='hinge')
        assert tr.mode == HINGE_MODE and tr.mode.loss == 'hinge' and tr.disc_iters == M.cfg.CRITIC_ITERS
        reg = oracle_from_product(lib)
        rnd = osteps.make_rnd_dcgan_d(B, M.feat_shapes(), g)
        tr.rng.begin_step()
        out, grads = tr.d_grads(real_in.to(dev), {k: to_dev(v, dev) for k, v in rnd.items()})
        with torch.no_grad():
            fake = G(reg, B, rnd['z'])
        d_real, _ = D(reg, real_o, rnd['u_real'])
        d_fake, _ = D(reg, fake, rnd['u_fake'])
        ref = hinge(1.0 - d_real).mean() + hinge(1.0 + d_fake).mean()
        assert abs(out['cost'].item() - ref.item()) <= cost_tol * max(1.0, abs(ref.item())), ('critic cost', out['cost'].item(), ref.item())
        assert 'ct' not in out and 'gp' not in out
        want = osteps.grads_of(ref, reg, 'Discriminator')
        got = {n: gv for (n, _), gv in zip(tr.d_named, tr._unscaled(list(grads))) if gv is not None}
        assert set(got) == set(want)
        for n in want:
            cmp_l2(got[n], want[n], d_tol, 'dgrad ' + n, atol=2e-6)
        # the dev cost of a hinge DCGANTrainer is the same cost (evaluate.Evaluator._pass_dcgan through mode.loss)
        from ctgan_amd.evaluate import Evaluator
        dev_rnd = {k: to_dev(v, dev) for k, v in dict(rnd, u_slope=rnd['u_gp']).items()}
        got_dev = Evaluator(tr, width=1).dev_cost([real_in.to(dev)], rnd=[dev_rnd])['dev_cost']
        assert abs(got_dev - ref.item()) <= cost_tol * max(1.0, abs(ref.item())), ('dev cost', got_dev, ref.item())
        rg = osteps.make_rnd_dcgan_g(B, M.feat_shapes(), g)
        tr.rng.begin_step()
        gout = tr.g_losses({k: to_dev(v, dev) for k, v in rg.items()})
        gref = osteps.dcgan_g_losses(reg, G, D, B, rg)['cost']
        assert abs(gout['cost'].item() - gref.item()) <= cost_tol * max(1.0, abs(gref.item()))
        ggot = dict(zip([n for n, _ in tr.g_named], torch.autograd.grad(gout['cost'], tr.g_params, allow_unused=True)))
        gwant = osteps.grads_of(gref, reg, 'Generator')
        for n in gwant:
            cmp_l2(ggot[n], gwant[n], g_tol, 'ggrad ' + n, atol=2e-6)
        return M
    finally:
        M.configure(); lib.delete_all_params()


def check_dcgan_refusals(lib, dev):
    import ctgan_amd.gan_mnist as M
    from ctgan_amd.dcgan_step import DCGANTrainer, build_params
    ran = []
    try:
        for mode, obj in (('wgan', 'hinge'), ('dcgan', 'hinge'), ('lsgan', 'hinge'), (M.Config.MODE, 'nope')):
            if mode not in M.MODES:              # (gan_mnist codes no 'lsgan' branch)
                continue
            ran.append((mode, obj))
            lib.delete_all_params(); lib.set_device('cpu' if dev == 'cpu' else None); lib.set_seed(13)
            M.configure(MODE=mode, DIM=8, BATCH_SIZE=4)
            build_params(M)
            try:
                DCGANTrainer(M, seed=1, objective=obj)
            except ValueError:
                continue
            raise AssertionError('DCGANTrainer accepted objective=%r under MODE %r' % (obj, mode))
        assert ('wgan', 'hinge') in ran and ('dcgan', 'hinge') in ran and (M.Config.MODE, 'nope') in ran, ran
        assert DCGANTrainer(M, seed=1, objective='hinge').mode.loss == 'hinge'          # the CT default itself is accepted (built last, above)
    finally:
        M.configure(); lib.delete_all_params()


# ------------------------------------------------------------------------------------------------------------------ dev cost
def check_dev_cost(R, lib, dev, heads='acgan', dim=16, B=8):
    """Evaluator.dev_cost of a hinge trainer = the mean hinge cost computed separately over the same dev batches and streams, to 2e-5."""
    from ctgan_amd.evaluate import Evaluator, eval_stream
    build(R, lib, dev, dim, B, seed=13, **HEADS[heads])
    shake(lib)
    tr = R.Trainer(seed=1, objective='hinge')
    batches = [batch(B, dev, seed=s) for s in (21, 22, 23)]
    ev = Evaluator(tr, width=1)
    got = ev.dev_cost(iter(batches))
    assert got['n_batches'] == 3
    # separately: the trainer's own loss graph on the evaluation stream, batch by batch (width 1: one step of the stream per batch)
    rng = eval_stream(tr)
    rng.ctr.zero_()
    saved, tr.rng = tr.rng, rng
    costs = []
    try:
        for real, lab in batches:
            rng.begin_step()
            with torch.no_grad():
                costs.append(tr.d_losses_hinge(real, lab)['cost'].item())
            rng.end_step()
    finally:
        tr.rng = saved
    want = sum(costs) / len(costs)
    assert abs(got['dev_cost'] - want) <= 2e-5 * max(1.0, abs(want)), (got['dev_cost'], want)
    assert max(costs) - min(costs) > 1e-4 * abs(want)
    # injected draws (the op-by-op path), two batches stacked in one pass and one by one
    g = torch.Generator().manual_seed(7)
    rnds = [{k: to_dev(v, dev) for k, v in osteps.make_rnd_resnet_d(B, dim, g).items()} for _ in batches]
    costs = []
    for (real, lab), rnd in zip(batches, rnds):
        tr.rng.begin_step()
        with torch.no_grad():
            costs.append(tr.d_losses_hinge(real, lab, rnd)['cost'].item())
    want = sum(costs) / len(costs)
    for width in (2, 1):
        got = Evaluator(tr, width=width).dev_cost(iter(batches), rnd=rnds)['dev_cost']
        assert abs(got - want) <= 2e-5 * max(1.0, abs(want)), (width, got, want)
