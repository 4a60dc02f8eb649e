"""Case tables, fp64 references and the checks of the hinge objective's kernels (ctgan_amd/csrc/loss.hip: ctgan_gan_loss_* kinds 4 / 5,
ctgan_tail_hinge_heads_fwd/bwd; csrc/optim_rng.hip: ctgan_real_fake_prep), shared by tests/test_gpu_hinge_kernels.py (the HIP kernels) and
tests/test_hinge_standins.py (their fp32 torch stand-ins, tests/hinge_cpu_kernels.py).  A plain helper module: no fixtures, no marks.

References: forward-only fp64 torch with the hinge torch.where(t >= 0, t, 0) (its gradient at the tie t == 0 is 1, the project's rule:
tests/loss_heads_cases.py); every gradient is torch.autograd.grad of that forward.  Conditions asserted on the reference: no |1 - d_real| or
|1 + d_fake| below 1e-4 except in the crafted ties, and the top-two logit gap is >= 1e-3 wherever an argmax is counted.

Bounds (the project's existing ones, tests/loss_heads_cases.py; none is derived from what the code under test returns):
  gan_loss          value 1e-5 * max(1, |ref|); gradient rtol 1e-5, atol 1e-9
  fused scalars     close_scalar: |got - ref| <= 2e-5 * max(1, |ref|)
  fused gradients   close_l2: ||got - ref|| <= 2e-5 ||ref|| + 1e-6 scale_all; gb_out against 1e-6 * sum |gd|
  f / d, a          FWD_TOL 1e-6 / DOT_TOL 1e-5 in relerr, as check_tail_critic has them
  real_fake_prep    bit-equal to the unfused launches; 2^-22 absolute against the float64 evaluation on the numpy generator
                    (tests/philox_checks.check_critic_prep's bound for the same expression)
"""
import numpy as np
import torch

from tests.loss_heads_cases import (DOT_TOL, FWD_TOL, SENTINEL, Backend, close, close_l2, close_scalar, f32, gen, head_params, hinge, note,  # noqa: F401
                                    ref_ce, ref_tail_heads, relerr)

TIE_MARGIN = 1e-4


# ------------------------------------------------------------------------------------------------------------------ references
def ref_hinge_d(d, B):
    """-> (hinge_real + hinge_fake, hinge_real, hinge_fake) over d = [D(real) ; D(fake)]"""
    hr, hf = hinge(1.0 - d[:B]).mean(), hinge(1.0 + d[B:]).mean()
    return hr + hf, hr, hf


def ref_hinge_g(d):
    return -d.mean()


def margins(d, B):
    return torch.cat([1.0 - d[:B], 1.0 + d[B:]]).detach()


def assert_off_tie(d, B, but=()):
    m = margins(d, B).abs()
    for i in range(2 * B):
        assert i in but or float(m[i]) >= TIE_MARGIN, ('a hinge within %g of its kink' % TIE_MARGIN, i, float(m[i]))


def assert_gap(a):
    if a.shape[1] > 1:
        top = a.detach().topk(2, dim=1).values
        assert bool(((top[:, 0] - top[:, 1]) >= 1e-3).all()), 'an argmax within 1e-3 of a tie'


# ------------------------------------------------------------------------------------------------------------------ gan_loss kinds 4, 5
GAN_LOSS_B = (1, 3, 300)            # 300: past one pass of the 256-thread loop
GAN_LOSS_KINDS = ('plain', 'ties', 'off')


def check_gan_loss_hinge(be, net, B, kind):
    K = be.K
    assert K.GAN_LOSS_KINDS[('hinge', 'd')] == 4 and K.GAN_LOSS_KINDS[('hinge', 'g')] == 5
    n = 2 * B if net == 'd' else B
    d = (torch.randn(n, generator=gen('hinge', net, B, kind)) * 2).float()
    ties = ()
    if net == 'd' and kind == 'ties':
        d[0], d[B] = 1.0, -1.0                       # exactly at both kinks: the gradient there is -gout/B and +gout/B
        ties = (0, B)
    if net == 'd' and kind == 'off':
        d[:B] = 1.5 + d[:B].abs(); d[B:] = -1.5 - d[B:].abs()
    x = d.double().requires_grad_(True)
    if net == 'd':
        assert_off_tie(x, B, ties)
        ref = ref_hinge_d(x, B)[0]
    else:
        ref = ref_hinge_g(x)
    (gref,) = torch.autograd.grad(ref, x)
    code = K.GAN_LOSS_KINDS[('hinge', net)]
    dv = be.dev(d)
    out = K.gan_loss_fwd(dv, B, code)
    gd = K.gan_loss_bwd(dv, be.dev(torch.tensor(0.75)), B, code)
    assert torch.isfinite(out).item() and torch.isfinite(gd).all() and gd.numel() == n
    e = abs(out.item() - ref.item()) / max(1.0, abs(ref.item()))
    note('gan_loss hinge fwd', e)
    assert e <= 1e-5, (out.item(), ref.item())
    assert torch.allclose(gd.cpu().double(), 0.75 * gref, rtol=1e-5, atol=1e-9)
    if ties:
        assert abs(gd[0].item() + 0.75 / B) <= 1e-5 * 0.75 / B and abs(gd[B].item() - 0.75 / B) <= 1e-5 * 0.75 / B      # on, not 0 and not 1/2
    if net == 'd' and kind == 'off':
        assert out.item() == 0.0 and bool((gd == 0).all())
    # through autograd (functional.GanLossFn serves the new kinds as it is)
    xv = be.dev(d).requires_grad_(True)
    cost = be.F.gan_loss(xv, B, 'hinge', net)
    (g2,) = torch.autograd.grad(cost, xv)
    assert torch.allclose(g2.cpu().double(), gref, rtol=1e-5, atol=1e-9)


# ------------------------------------------------------------------------------------------------------------------ tail_hinge_heads
TAIL_B = (1, 3, 65)                 # 1: every mean over one row; 3: a repeated label, absent classes; 65: more rows than a wave has lanes
TAIL_HW = ((1, 1), (8, 8))
TAIL_NF = (32, 128)
TAIL_HEADS = ('plain', 'class', 'proj')
TAIL_CASES = [(B, H, W, nf, heads) for B in TAIL_B for (H, W) in TAIL_HW for nf in TAIL_NF for heads in TAIL_HEADS]
NCLS = N_LABELS = 10
KEEP = 0.5


def tail_labels(B, g):
    if B == 1:
        return torch.tensor([4], dtype=torch.int32)
    if B == 3:
        return torch.tensor([3, 7, 3], dtype=torch.int32)            # a label repeated; classes no row carries
    return torch.randint(0, NCLS, (B,), generator=g, dtype=torch.int32)


def tail_inputs(B, H, W, nf, heads, trial=0):
    """-> dict: z, mask (y = relu(z) * mask is what the last conv's epilogue writes), head parameters, table, labels - the first seed whose
    reference keeps every hinge off its kink and every counted argmax clear (check_tail_hinge_crafted edits the result)."""
    for s in range(64):
        g = gen('hinge-tail', B, H, W, nf, heads, trial, s)
        z = torch.randn(2 * B, nf, H, W, generator=g)
        mask = (torch.rand(2 * B, nf, H, W, generator=g) < KEEP).float() / KEEP
        w_out, b_out, w_ac, b_ac = head_params(g, nf, NCLS)
        emb = torch.randn(N_LABELS, nf, generator=g) * 0.3
        lab = tail_labels(B, g)
        inp = dict(z=z, mask=mask, w_out=w_out, b_out=b_out, w_ac=w_ac, b_ac=b_ac, emb=emb, lab=lab, B=B, heads=heads)
        ref = tail_ref(inp)
        ok = bool((margins(ref['d'], B).abs() >= TIE_MARGIN).all())
        if heads == 'class' and NCLS > 1:
            top = ref['a'].detach().topk(2, dim=1).values
            ok = ok and bool(((top[:, 0] - top[:, 1]) >= 1e-3).all())
        if ok:
            return inp
    raise AssertionError('no seed with every hinge off its kink')


def tail_ref(inp, scale=0.0, double_leaves=None):
    """fp64 forward -> dict of d, f, a, out5 (cost, hinge, hinge_real, hinge_fake, acgan), acc"""
    B, heads = inp['B'], inp['heads']
    L = double_leaves or {k: inp[k].double() for k in ('z', 'w_out', 'b_out', 'w_ac', 'b_ac', 'emb')}
    y = torch.relu(L['z']) * inp['mask'].double()
    with_a = heads == 'class'
    f, d, a = ref_tail_heads(y, L['w_out'], L['b_out'], L['w_ac'] if with_a else None, L['b_ac'] if with_a else None)
    if heads == 'proj':
        d = d + (f * L['emb'][inp['lab'].long().repeat(2)]).sum(dim=1)
    hsum, hr, hf = ref_hinge_d(d, B)
    ac = ref_ce(a[:B], inp['lab']) if with_a else torch.zeros((), dtype=torch.float64)
    acc = None
    if with_a:
        am = a.detach().argmax(dim=1)
        acc = ((am[:B] == inp['lab'].long()).double().mean().item(), (am[B:] == inp['lab'].long()).double().mean().item())
    return dict(y=y, f=f, d=d, a=a, out5=(hsum + scale * ac, hsum, hr, hf, ac), acc=acc)


def _run(be, inp, y, scale, gout, out=None):
    K = be.K
    heads = inp['heads']
    P = {k: be.dev(inp[k]) for k in ('w_out', 'b_out', 'w_ac', 'b_ac', 'emb')}
    lab = be.dev(inp['lab'])
    kw = dict(labels=lab, emb=P['emb'] if heads == 'proj' else None, w_ac=P['w_ac'] if heads == 'class' else None,
              b_ac=P['b_ac'] if heads == 'class' else None, scale=scale if heads == 'class' else 0.0)
    yd = be.cl(y)
    fwd = K.tail_hinge_heads_fwd(yd, inp['B'], P['w_out'], P['b_out'], **kw)
    out5, f, d, a, probs, acc = fwd
    bwd = K.tail_hinge_heads_bwd(yd, d, f, probs, lab, be.dev(torch.tensor([gout])), inp['B'], kw['scale'], 1.0 / KEEP, P['w_out'], emb=kw['emb'],
                                 w_ac=kw['w_ac'], out=out)
    return fwd, bwd


def check_tail_hinge(be, B, H, W, nf, heads):
    scale, gout = f32(0.7), f32(0.8)
    inp = tail_inputs(B, H, W, nf, heads)
    with_a, proj = heads == 'class', heads == 'proj'
    names = ['z', 'w_out', 'b_out'] + (['w_ac', 'b_ac'] if with_a else []) + (['emb'] if proj else [])
    L = {k: inp[k].double() for k in ('z', 'w_out', 'b_out', 'w_ac', 'b_ac', 'emb')}
    for k in names:
        L[k].requires_grad_(True)
    ref = tail_ref(inp, scale if with_a else 0.0, L)
    assert_off_tie(ref['d'], B)
    if with_a:
        assert_gap(ref['a'])
    y = (torch.relu(inp['z']) * inp['mask'])
    (out5, f, d, a, probs, acc), (gy, gw_out, gb_out, g_emb, gw_ac, gb_ac) = _run(be, inp, y, scale, gout)
    for x, r in zip(out5, ref['out5']):
        close_scalar('tail_hinge_heads fwd', x, r)
    close('tail_hinge_heads fwd f', f, ref['f'].detach(), FWD_TOL)
    close('tail_hinge_heads fwd d', d, ref['d'].detach(), DOT_TOL)
    if with_a:
        close('tail_hinge_heads fwd a', a, ref['a'].detach(), DOT_TOL)
        close('tail_hinge_heads fwd probs', probs, torch.softmax(ref['a'][:B].detach(), dim=1), DOT_TOL)
        for k in (0, 1):
            assert abs(acc[k].item() - ref['acc'][k]) < 1e-6, (acc, ref['acc'])
    else:
        assert a is None and probs is None and acc is None and gw_ac is None and gb_ac is None
    gr = torch.autograd.grad(gout * ref['out5'][0], [L[k] for k in names] + [ref['d']], retain_graph=True)
    gd_ref = gr[-1]
    got = [gy, gw_out, gb_out] + ([gw_ac, gb_ac] if with_a else []) + ([g_emb] if proj else [])
    scale_all = max(float(t.abs().max()) for t in gr[:-1])
    for i, (x, r) in enumerate(zip(got, gr[:-1])):
        close_l2('tail_hinge_heads bwd', x, r, float(gd_ref.abs().sum()) if i == 2 else scale_all)
    if proj:
        absent = [c for c in range(N_LABELS) if c not in inp['lab'].tolist()]
        if absent:
            assert torch.equal(g_emb[absent].cpu(), torch.zeros(len(absent), nf)), 'a class no row carries gets exact zeros'
        # a zero table gives the plain head's bits
        zero = dict(inp, emb=torch.zeros_like(inp['emb']))
        plain = dict(inp, heads='plain')
        (o_z, f_z, d_z, _, _, _), (gy_z, gw_z, gb_z, ge_z, _, _) = _run(be, zero, y, scale, gout)
        (o_p, f_p, d_p, _, _, _), (gy_p, gw_p, gb_p, _, _, _) = _run(be, plain, y, scale, gout)
        for u, v in ((o_z, o_p), (f_z, f_p), (d_z, d_p), (gy_z, gy_p), (gw_z, gw_p), (gb_z, gb_p)):
            assert torch.equal(u, v), 'zero table'
    # two runs give equal bits
    again = _run(be, inp, y, scale, gout)
    for u, v in zip((out5, f, d, a, probs, acc, gy, gw_out, gb_out, g_emb, gw_ac, gb_ac), again[0] + again[1]):
        assert (u is None and v is None) or torch.equal(u, v), 'two runs differ'


CRAFTED = [(B, heads, what) for B in (3, 65) for heads in TAIL_HEADS for what in ('ties', 'off', 'buffer')]


def check_tail_hinge_crafted(be, B, heads, what):
    """ties: d == 1.0 on real row 0, then d == -1.0 on fake row B, exactly, on rows with NON-ZERO features (the unit feature e_0, weight
    w_out[0] = +1 / -1, no bias, a table whose column 0 is zero): the hinge on its kink counts as on, which the kernel shows in gy of that
    row, in gw_out[0], in g_emb and in gb_out; off: every hinge off - gy, gw_out, g_emb exactly 0 without the class head; buffer: gy into
    the leading rows of a larger buffer whose other rows keep their sentinel."""
    H, W, nf = 2, 2, 32
    scale, gout = f32(0.7), f32(0.8)
    inp = tail_inputs(B, H, W, nf, heads, trial=1)
    with_a, proj = heads == 'class', heads == 'proj'
    ties = ()
    if what == 'ties':
        # rows 0 and B: y = e_0 at every position (mean over hw = 1 exactly), so f = e_0 and d = w_out[0] exactly in fp32 and in fp64:
        # w_out[0] = 1 puts real row 0 on its kink (fake row B then has 1 + d = 2: on); a second run with w_out[0] = -1 puts fake row B on
        # its kink (real row 0 at 1 - d = 2).
        for i in (0, B):
            inp['z'][i] = -1.0; inp['z'][i, 0] = 1.0; inp['mask'][i, 0] = 1.0
        inp['b_out'] = torch.zeros_like(inp['b_out'])
        inp['emb'][:, 0] = 0.0
    for w0 in ((1.0, -1.0) if what == 'ties' else (None,)):
        if w0 is not None:
            inp['w_out'] = inp['w_out'].clone()
            inp['w_out'].view(-1)[0] = w0
            ties = (0,) if w0 > 0 else (B,)
        y = torch.relu(inp['z']) * inp['mask']
        if what == 'off':
            # every feature >= 1 on the real rows and <= -1 on the fake rows, unit weights, no table: d_real >= nf + b, d_fake <= -nf + b
            inp['w_out'] = torch.ones_like(inp['w_out']); inp['emb'] = torch.zeros_like(inp['emb'])
            y = torch.cat([y[:B] + 1.0, -y[B:] - 1.0], 0)               # (not a relu output on the fake rows: the kernels only ask y > 0)
        names = ['w_out', 'b_out'] + (['w_ac', 'b_ac'] if with_a else []) + (['emb'] if proj else [])
        L = {k: inp[k].double() for k in ('w_out', 'b_out', 'w_ac', 'b_ac', 'emb')}
        for k in names:
            L[k].requires_grad_(True)
        yr = y.double().requires_grad_(True)
        f, d, a = ref_tail_heads(yr, L['w_out'], L['b_out'], L['w_ac'] if with_a else None, L['b_ac'] if with_a else None)
        if proj:
            d = d + (f * L['emb'][inp['lab'].long().repeat(2)]).sum(dim=1)
        if what == 'off':
            assert bool((margins(d, B) < -TIE_MARGIN).all())
        else:
            assert_off_tie(d, B, ties)
            for i in ties:
                assert float(margins(d, B)[i]) == 0.0
        hsum = ref_hinge_d(d, B)[0]
        cost = hsum + (scale * ref_ce(a[:B], inp['lab']) if with_a else 0.0)
        gr = torch.autograd.grad(gout * cost, [yr] + [L[k] for k in names] + [d], allow_unused=True)
        gy_ref = gr[0] * (y > 0).double() * (1.0 / KEEP)                 # the kernel returns the gradient w.r.t. the PRE-activation of relu + dropout
        gy_buf = None
        out = None
        if what == 'buffer':
            out, gy_buf = be.cl(torch.zeros_like(y), extra_rows=2)
            out.fill_(SENTINEL)
        (out5, fk, dk, ak, probs, acc), (gy, gw_out, gb_out, g_emb, gw_ac, gb_ac) = _run(be, inp, y, scale, gout, out=out)
        close_scalar('tail_hinge_heads fwd crafted', out5[0], cost)
        close_scalar('tail_hinge_heads fwd crafted', out5[1], hsum)
        got = [gy, gw_out, gb_out] + ([gw_ac, gb_ac] if with_a else []) + ([g_emb] if proj else [])
        refs = [gy_ref] + list(gr[1:-1])
        scale_all = max(max(float(t.abs().max()) for t in refs), 1e-30)
        for i, (x, r) in enumerate(zip(got, refs)):
            close_l2('tail_hinge_heads bwd crafted', x, r, float(gr[-1].abs().sum()) if i == 2 else scale_all)
        for i in ties:
            # the row sits on its kink exactly and counts as on.  The witnesses are the KERNEL's outputs: gy of the tied row (channel 0 is its
            # only live feature), gw_out[0] = sum_r f_r0 gd_r, g_emb and gb_out = sum_r gd_r - all held to the reference above, in which
            # gd_i = -gout/B (real) / +gout/B (fake); a tie taken as off moves gw_out[0] and gb_out by gout/B and zeroes that row of gy.
            assert dk[i].item() == (1.0 if i == 0 else -1.0)
            assert abs(float(gr[-1][i]) - (-gout / B if i == 0 else gout / B)) < 1e-12
            if i == B or not with_a:                                     # (a real row's gy also carries the class head's term)
                want = (-gout / B if i == 0 else gout / B) * w0 / (H * W) / KEEP
                assert bool(((gy[i, 0].cpu().double() - want).abs() <= 1e-6 * abs(want)).all()), (gy[i, 0], want)
            assert bool((gy[i, 1:] == 0).all())
        if what == 'off':
            assert out5[1].item() == 0.0 and out5[2].item() == 0.0 and out5[3].item() == 0.0
            if not with_a:
                assert bool((gy == 0).all()) and bool((gw_out == 0).all()) and gb_out.item() == 0.0
                if proj:
                    assert bool((g_emb == 0).all())
        if what == 'buffer':
            be.sync()
            assert gy is out and bool((gy_buf[2 * B:] == SENTINEL).all())


def check_tail_hinge_refusals(be):
    """emb and w_ac together, B = 0 and nf % 4 != 0 fail before any launch (CTGAN_E_BADARG from the C entry, or the wrapper's own assertion)."""
    K = be.K
    g = gen('hinge-refuse')
    for B, nf, both in ((2, 32, True), (0, 32, False), (2, 30, False)):
        y = be.cl(torch.rand(max(2 * B, 0), nf, 2, 2, generator=g))
        w_out, b_out, w_ac, b_ac = (be.dev(t) for t in head_params(g, nf, NCLS))
        emb = be.dev(torch.zeros(N_LABELS, nf))
        lab = be.dev(torch.zeros(max(B, 0), dtype=torch.int32))
        kw = dict(labels=lab, emb=emb if both else None, w_ac=w_ac if both else None, b_ac=b_ac if both else None)
        try:
            K.tail_hinge_heads_fwd(y, B, w_out, b_out, **kw)
        except (AssertionError, RuntimeError, ValueError):
            pass
        else:
            raise AssertionError('tail_hinge_heads_fwd accepted B=%d nf=%d both=%s' % (B, nf, both))
        try:
            K.tail_hinge_heads_bwd(y, be.dev(torch.zeros(2 * B)), be.dev(torch.zeros(2 * B, nf)), be.dev(torch.zeros(max(B, 0), NCLS)) if both else None,
                                   lab, be.dev(torch.ones(1)), B, 0.0, 2.0, w_out,
                                   emb=kw['emb'], w_ac=kw['w_ac'])
        except (AssertionError, RuntimeError, ValueError):
            pass
        else:
            raise AssertionError('tail_hinge_heads_bwd accepted B=%d nf=%d both=%s' % (B, nf, both))


# ------------------------------------------------------------------------------------------------------------------ real_fake_prep
PREP_CASES = [(1, 4), (3, 3072)]


def check_real_fake_prep(be, corner, B, d):
    from tests import philox_spec as S
    K = be.K
    seed, sid, step = S.CORNERS[corner]
    lo, hi, denom = 0.0, 1.0 / 128, 256.0
    r = np.random.RandomState(B * d + 7)
    xi = torch.from_numpy(r.randint(0, 256, size=(B, d)).astype(np.int32))
    fake = torch.from_numpy((r.rand(B, d) * 2 - 1).astype(np.float32))
    ctr = torch.tensor([step], dtype=torch.int64, device=be.device)
    rf = K.real_fake_prep(be.dev(xi), be.dev(fake), seed, sid, ctr, lo, hi, denom)
    assert tuple(rf.shape) == (2 * B, d) and int(ctr.item()) == step
    deq = K.rng_uniform(torch.empty(B, d, device=be.device), seed, sid, ctr, lo, hi)
    want = torch.cat([K.real_prep(be.dev(xi), deq, denom), be.dev(fake)], 0)
    assert torch.equal(rf, want), 'not the bits of rng_uniform + real_prep + cat'
    real64, fake_w, _ = S.critic_prep(xi.numpy(), fake.numpy(), seed, sid, sid + 1, step, lo, hi, denom)
    assert np.array_equal(rf[B:].cpu().numpy().view(np.uint32), fake_w.view(np.uint32)), 'fake rows'
    dist = np.max(np.abs(rf[:B].cpu().numpy().astype(np.float64) - real64))
    note('real_fake_prep real', dist)
    assert dist <= 2.0 ** -22, dist


def check_real_fake_prep_refusals(be):
    K = be.K
    ctr = torch.zeros(1, dtype=torch.int64, device=be.device)
    xi = be.dev(torch.zeros(2, 6, dtype=torch.int32))
    fake = be.dev(torch.zeros(2, 6))
    try:
        K.real_fake_prep(xi, fake, 1, 0, ctr, 0.0, 1.0, 256.0)            # d % 4 != 0
    except (AssertionError, RuntimeError, ValueError):
        pass
    else:
        raise AssertionError('real_fake_prep accepted d = 6')
    if be.gpu:
        xi = be.dev(torch.zeros(2, 8, dtype=torch.int32))
        mis = be.off16(torch.zeros(2, 8))
        try:
            K.real_fake_prep(xi, mis, 1, 0, ctr, 0.0, 1.0, 256.0)
        except (AssertionError, RuntimeError, ValueError):
            pass
        else:
            raise AssertionError('real_fake_prep accepted a misaligned pointer')
