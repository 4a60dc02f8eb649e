"""Hand-scheduled critic step of the hinge objective (gan_cifar_resnet.Trainer(objective='hinge'); NOT in the reference):

    L_D = mean_i max(0, 1 - D(x_i)) + mean_i max(0, 1 + D(G(z_i)))   [+ ACGAN_SCALE * CE(class head of the real rows)]

ONE forward and ONE backward chain over the 2B rows [real ; fake] - the launches of critic_schedule.py without everything the CT
objective adds: no x_hat rows, no second dropout pass over the reals, no clean pass, no phase C (the gradient penalty's double backward).

  forward   kernels.real_fake_prep (or the trainer's augmented [T(real) ; T(fake)]); blocks 1-2 and blocks 3-4 on 2B rows, taped, the three
            dropouts drawn inside the conv kernels from the trainer's Philox streams; kernels.tail_hinge_heads_fwd (mean, output head with the
            optional projection table, optional class head, both hinges, the batch means: two launches);
  backward  kernels.tail_hinge_heads_bwd writes the gradient w.r.t. the last conv's result and the head gradients (one launch); then phase
            B of critic_schedule.py on 2B rows: the same `_dgrad` calls with the same mask / resid / drop epilogues and the same cached spread
            filters, down to the weight gradient of Discriminator.1.Conv1 (no dD/dx is needed); ONE weight-gradient request per filter, so the
            grouped launch has one segment per filter.

Each launch calls the same C-ABI entry points as the autograd path (Trainer.d_losses_hinge + torch.autograd.grad), which stays: it serves
injected draws, the Layernorm critic, a fusion switch off and widths outside the few-channel kernels, draws at the same Philox call sites
in the same order (dequantisation, then the three dropouts in network order), and is what tests/test_hinge_host.py /
test_gpu_hinge_step.py compare this schedule with.
"""
from . import critic_schedule as CS
from . import functional as F
from . import kernels as K
from . import tflib as lib
from .kernels import ConvGeom


def usable(R, rnd, rng, real_int, fake):
    """Is the hand-scheduled hinge step the same computation as Trainer.d_losses_hinge + autograd here?  The conditions of
    critic_schedule.usable: the fully fused default path, in-kernel Philox draws, a piecewise-linear critic on the few-channel kernels -
    and no attention block in the critic (cfg.ATTENTION_D: its launches are not in this schedule, the autograd path serves the step)."""
    return not getattr(R.cfg, 'ATTENTION_D', False) and CS.usable(R, rnd, rng, real_int, fake)


def critic_step(tr, R, real_int, labels, fake, prep=None):
    """One hinge critic step's losses AND parameter gradients -> (out, grads aligned with tr.d_params).  Must run inside torch.no_grad()
    and functional.deferred_wgrads() (the caller flushes the queue by leaving the latter).  prep: the prepared rf [2B,d] in place of the
    kernels.real_fake_prep launch - the trainer's augmented inputs (Trainer.hinge_prep, which draws at the same call site)."""
    import torch
    cfg = R.cfg
    B, D = cfg.BATCH_SIZE, cfg.DIM_D
    rng = tr.rng
    P = lib.param
    use_ac = cfg.CONDITIONAL and cfg.ACGAN
    assert not torch.is_grad_enabled()
    N = 2 * B

    # ------------------------------------------------------------------ forward
    rf = prep if prep is not None else K.real_fake_prep(real_int, fake, rng.seed, rng._sid(), rng.ctr, 0.0, 1. / 128, 256.0)
    with F.tape_record() as trunk:
        R.DiscriminatorTrunk(rf)
    y1, _c12, pool_x, h1, a2, _c22, h2 = trunk
    specs = (F.drop_spec(rng, 0.8), F.drop_spec(rng, 0.5), F.drop_spec(rng, 0.5))
    with F.tape_record() as tail:
        R.DiscriminatorTailBody(h2, 0.8, 0.5, 0.5, rng=rng, mask_done=True, specs=specs)
    tin, a31, b3, a41, y = tail
    w_out, b_out = P('Discriminator.Output.W'), P('Discriminator.Output.b')
    w_ac = P('Discriminator.ACGANOutput.W') if use_ac else None
    b_ac = P('Discriminator.ACGANOutput.b') if use_ac else None
    emb = R.projection_table() if cfg.PROJECTION else None
    scale = cfg.ACGAN_SCALE if use_ac else 0.0
    out5, f_all, d_all, _a, probs, acc = K.tail_hinge_heads_fwd(y, B, w_out, b_out, labels=labels, emb=emb, w_ac=w_ac, b_ac=b_ac, scale=scale)

    # ------------------------------------------------------------------ backward: phase B of critic_schedule.py on the 2B rows
    G = CS._Grads()
    _dgrad = CS._dgrad
    one = tr.cost_seed(out5[0]).reshape(1)
    g3 = ConvGeom(D, 8, 8, D, 3, 3, 1)
    gy = K.empty_cl(N, D, 8, 8, y.device)
    _, gw_out, gb_out, g_emb, gw_ac, gb_ac = K.tail_hinge_heads_bwd(y, d_all, f_all, probs, labels, one, B, scale, 1.0 / 0.5, w_out, emb=emb,
                                                                     w_ac=w_ac, out=gy)
    W42, W41 = P('Discriminator.4.Conv2.Filters'), P('Discriminator.4.Conv1.Filters')
    W32, W31 = P('Discriminator.3.Conv2.Filters'), P('Discriminator.3.Conv1.Filters')
    g_a41 = _dgrad(gy, W42, g3, N, mask=a41)
    g_z3 = _dgrad(g_a41, W41, g3, N, mask=b3, resid=gy, drop=specs[1])
    g_a31 = _dgrad(g_z3, W32, g3, N, mask=a31)
    g_h2 = _dgrad(g_a31, W31, g3, N, mask=tin, resid=g_z3, drop=specs[0])
    G.wgrad('Discriminator.4.Conv2', a41, gy, W42, g3, True, True)
    G.wgrad('Discriminator.4.Conv1', b3, g_a41, W41, g3, True, True)
    G.wgrad('Discriminator.3.Conv2', a31, g_z3, W32, g3, True, True)
    G.wgrad('Discriminator.3.Conv1', tin, g_a31, W31, g3, True, True)

    W21 = P('Discriminator.2.Conv1.Filters')
    w22 = F._cached_filter(P('Discriminator.2.Conv2.Filters'), K.FILTER_SPREAD, (0, 0), 0.25)
    wsc2 = F._cached_filter(P('Discriminator.2.Shortcut.Filters'), K.FILTER_SPREAD, (0, 0), 0.25)
    w12 = F._cached_filter(P('Discriminator.1.Conv2.Filters'), K.FILTER_SPREAD, (0, 0), 0.25)
    W11, Wsc1 = P('Discriminator.1.Conv1.Filters'), P('Discriminator.1.Shortcut.Filters')
    g21 = ConvGeom(D, 16, 16, D, 3, 3, 1)
    g22 = ConvGeom(D, 16, 16, D, 4, 4, 2)
    gsc2 = ConvGeom(D, 16, 16, D, 2, 2, 2)
    g12 = ConvGeom(D, 32, 32, D, 4, 4, 2)
    g11 = ConvGeom(3, 32, 32, D, 3, 3, 1)
    gsc1 = ConvGeom(3, 16, 16, D, 1, 1, 1)
    gx_sc2 = _dgrad(g_h2, wsc2, gsc2, N)
    G.wgrad('Discriminator.2.Shortcut', h1, g_h2, wsc2, gsc2, False, True, spread=0.25)
    g_a2 = _dgrad(g_h2, w22, g22, N, mask=a2)
    G.wgrad('Discriminator.2.Conv2', a2, g_h2, w22, g22, True, True, spread=0.25)
    g_h1 = _dgrad(g_a2, W21, g21, N, mask=h1, resid=gx_sc2)
    G.wgrad('Discriminator.2.Conv1', h1, g_a2, W21, g21, True, True)
    g_y1 = _dgrad(g_h1, w12, g12, N, mask=y1)
    G.wgrad('Discriminator.1.Conv2', y1, g_h1, w12, g12, True, True, spread=0.25)
    G.wgrad('Discriminator.1.Shortcut', pool_x, g_h1, Wsc1, gsc1, False, True)
    G.wgrad('Discriminator.1.Conv1', rf.reshape(N, 3, 32, 32), g_y1, W11, g11, False, True)      # the chain's end: no dD/dx is needed

    by = G.by_name
    by['Discriminator.Output.W'], by['Discriminator.Output.b'] = gw_out, gb_out
    if use_ac:
        by['Discriminator.ACGANOutput.W'], by['Discriminator.ACGANOutput.b'] = gw_ac, gb_ac
    if emb is not None:
        by['Discriminator.Projection.W'] = g_emb
    grads = [by.get(n) for n, _ in tr.d_named]
    out = {'cost': out5[0], 'wgan': out5[1], 'hinge_real': out5[2], 'hinge_fake': out5[3], 'acgan': out5[4] if use_ac else None,
           'acc_real': acc[0] if use_ac else None, 'acc_fake': acc[1] if use_ac else None, 'fake': fake, 'real': rf[:B],
           'd_real': d_all[:B], 'd_fake': d_all[B:2 * B]}
    return out, grads
