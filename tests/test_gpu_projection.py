"""The projection head on the device (csrc/loss.hip: the six ctgan_*_proj entry points; gan_cifar_resnet.Config.PROJECTION):
  * every launch against the fp64 reference of tests/projection_oracle.py at the edge shapes of tests/loss_heads_cases.TAIL_CRITIC_CASES, with
    1, 10 and 13 labels and four label patterns, outputs in sentinel-filled buffers, at the bounds loss_heads_cases applies to the twin's
    matching output; rows of g_emb no sample carries are exact zeros; two runs give the same bits;
  * with a table of zeros every launch gives its twin's bits;
  * the critic step: hand-scheduled against autograd, graph replay against eager (plain, and with augmentation and weight averaging on).
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import loss_heads_cases as C  # noqa: E402
from tests import projection_oracle as PO  # noqa: E402

SENT = C.SENTINEL
PATTERNS = ('one', 'last', 'absent', 'own')
COND = dict(CONDITIONAL=True, ACGAN=False)


@pytest.fixture(scope='module')
def be():
    import ctgan_amd.functional as F
    import ctgan_amd.kernels as K
    return C.Backend(K, F, 'cuda')


@pytest.fixture(scope='module', autouse=True)
def _report():
    C.MEASURED.clear()
    yield
    print('\nprojection head, largest errors against fp64:\n' + C.report())


def label_pattern(pattern, n, L, g):
    """n labels in [0, L) -> (labels, classes no label carries)"""
    if pattern == 'one':
        lab = torch.full((n,), min(1, L - 1))
    elif pattern == 'last':
        lab = torch.full((n,), L - 1)
    elif pattern == 'absent':                                # every class but one may occur (L = 1: nothing can be absent)
        gone = L // 2
        lab = torch.randint(0, max(L - 1, 1), (n,), generator=g)
        lab = lab + (lab >= gone).long() if L > 1 else lab
    else:                                                    # every row its own class (wrapping where there are more rows than classes)
        lab = torch.arange(n) % L
    lab = lab.to(torch.int32)
    return lab, [c for c in range(L) if c not in lab.tolist()]


def _inputs(B, nf, H, W, L, pattern, zero_table=False):
    g = C.gen('proj', B, nf, H, W, L, pattern)
    keep = 0.5

    def make(trial):
        gt = C.gen('proj', B, nf, H, W, L, pattern, trial)
        z, mask = C.masked_relu_inputs(gt, 3 * B, nf, H, W, keep)
        w_out, b_out, _, _ = C.head_params(gt, nf, 1)
        emb = torch.zeros(L, nf) if zero_table else torch.randn(L, nf, generator=gt) * (2 / nf ** 0.5)
        lab, absent = label_pattern(pattern, B, L, gt)
        ct_i0 = PO.critic_heads(z.double(), mask.double(), w_out.double(), b_out.double(), emb.double(), lab, B, 2.0, 0.0, None)[3]
        Ms = [0.0] + ([C.midpoint_M(ct_i0)] if B > 1 else [])
        return (z, mask, w_out, b_out, emb, lab, absent, Ms) if all(C.off_tie(ct_i0, M) for M in Ms) else None
    return (g,) + C.seeded(make)


def _raw_bwd_proj(K, y, d, f, lab, ct_i, gout, B, lam2, M, ms, w_out, emb):
    """ctgan_tail_heads_bwd_proj through the C ABI into sentinel-filled outputs (the wrapper allocates gw_out / gb_out / g_emb itself)"""
    from ctgan_amd import _lib
    n, hw, nf = K._cl_rows(y)
    gy = K.empty_cl(n, nf, y.shape[2], y.shape[3], y.device).fill_(SENT)
    gw = torch.full_like(w_out, SENT); gb = torch.full((1,), SENT, device=y.device); ge = torch.full_like(emb, SENT)
    p = K._ptr
    _lib.check(_lib.lib.ctgan_tail_heads_bwd_proj(p(y), p(d), p(f), p(lab), p(ct_i), p(gout), gout.numel(), B, hw, nf, lam2, M, ms, p(w_out), p(emb),
                                                 emb.shape[0], p(gy), p(gw), p(gb), p(ge), None, 0, None, K._stream()), 'tail_heads_bwd_proj')
    return gy, gw, gb, ge


@pytest.mark.parametrize('L', [1, 10, 13])
@pytest.mark.parametrize('B,nf,H,W', [c[:4] for c in C.TAIL_CRITIC_CASES])
def test_projection_launches_against_fp64(be, B, nf, H, W, L):
    """tail_critic_heads_fwd_proj (with the penalty's mean folded in), tail_heads_bwd_proj (n_gout 1 and 4, outputs in the leading rows of larger
    buffers, the penalty rows riding the launch), gen_heads_fwd_proj / _bwd_proj, gp_head_grad_proj and gp_head_wgrad_proj (writing and
    accumulating; nf = 12, 260, 1020 are quarters that do not divide 256) - through the wrappers and through functional's autograd forms."""
    K, F = be.K, be.F
    lam2, keep, gp0 = 2.0, 0.5, C.f32(0.37)
    ms = 1.0 / keep
    for pattern in (PATTERNS if L > 1 else PATTERNS[:1]):
        g, z, mask, w_out, b_out, emb, lab, absent, Ms = _inputs(B, nf, H, W, L, pattern)
        y = torch.relu(z) * mask
        zr = z.double().requires_grad_(True)
        P = [t.double().requires_grad_(True) for t in (w_out, b_out, emb)]
        labd, lab3 = be.dev(lab), lab.repeat(3)
        n_gp = min(B, 7)
        for M in Ms:
            outs, fr, dr, ct_ref = PO.critic_heads(zr, mask.double(), P[0], P[1], P[2], lab, B, lam2, M, gp0)
            C.assert_off_tie(ct_ref, M)
            # ---- through autograd (F.critic_tail_heads(..., emb=...)), n_gout = 1 and 4
            yd = be.cl(y).requires_grad_(True)
            Pd = [be.dev(t).requires_grad_(True) for t in (w_out, b_out, emb)]
            gpv = be.dev(torch.tensor(gp0)).requires_grad_(True)
            got = F.critic_tail_heads(yd, Pd[0], Pd[1], None, None, labd, B, lam2, M, 0.0, ms, gp=gpv, emb=Pd[2])
            for x, r in zip(got[:5], outs):
                C.close_scalar('proj tail_critic_heads fwd', x, r)
            C.close('proj tail_critic_heads fwd d', got[5], dr.detach(), C.DOT_TOL)
            assert got[6].numel() == 0
            for w in ([1.0, 0.0, 0.0, 0.0], C.HEAD_W):
                comb = got[0] if w[0] == 1.0 else sum(wi * gi for wi, gi in zip(w, got[:4]))
                combr = outs[0] if w[0] == 1.0 else sum(wi * ri for wi, ri in zip(w, outs[:4]))
                gg = torch.autograd.grad(comb, [yd] + Pd, retain_graph=True)
                gr = torch.autograd.grad(combr, [zr] + P + [dr], retain_graph=True)
                # (gy, gw_out, gb_out, g_emb): g_emb at gw_out's bound (check_tail_grads: every entry but gb_out against the common scale)
                C.check_tail_grads('proj tail_heads bwd', gg, gr[:-1], gr[-1])
                assert torch.equal(gg[3][absent].cpu(), torch.zeros(len(absent), nf))
                scale_all = max(float(t.abs().max()) for t in gr[:-1])
                C.close_l2('proj sum_c g_emb[c] = gw_out', gg[3].sum(dim=0).reshape(-1, 1), gr[1], scale_all)
            # ---- the wrappers: the penalty's mean folded into the forward ...
            sl = torch.tensor([C.GP_TARGETS[i % 4] for i in range(B)]) + torch.rand(B, generator=g) * 0.1
            gp_ref = 10.0 * ((sl.double() - 1) ** 2).mean()
            slot = be.dev(torch.full((1,), SENT))
            Pk = [be.dev(w_out), be.dev(b_out), be.off16(emb)]     # the table 4 bytes past a 16-byte boundary, as the flat bucket holds it
            out, f, d, ct_i = K.tail_critic_heads_fwd_proj(be.cl(y), B, Pk[0], Pk[1], Pk[2], labd, slot, lam2, M, slopes=be.dev(sl), gp_lambda=10.0)
            C.close('proj fwd gp slot', slot, gp_ref.reshape(1), C.FWD_TOL)
            for x, r in zip(out, [outs[0] - gp0 + gp_ref, outs[1], outs[2], outs[3], outs[4] - gp0 + gp_ref]):
                C.close_scalar('proj tail_critic_heads fwd', x, r)
            assert out[3].item() == 0.0
            C.close('proj tail_heads fwd f', f, fr.detach(), C.FWD_TOL)
            C.close('proj tail_critic_heads fwd d', d, dr.detach(), C.DOT_TOL)
            C.close('proj tail_critic_heads fwd ct_i', ct_i, ct_ref.detach(), C.FUSED_TOL)
            # ... and the backward with its outputs in the leading rows of larger buffers and the penalty pass's rows riding the launch
            w = C.HEAD_W
            gout = be.dev(torch.tensor(w))
            gr = torch.autograd.grad(sum(wi * ri for wi, ri in zip(w, outs[:4])), [zr] + P + [dr], retain_graph=True)
            z_gp, m_gp = C.masked_relu_inputs(g, n_gp, nf, H, W, keep)
            zg = z_gp.double().requires_grad_(True)
            gz_ref = PO.gp_seed(zg, m_gp.double(), P[0].detach(), P[2].detach(), lab[:n_gp])
            y_gp = be.cl(torch.relu(z_gp) * m_gp)
            runs = []
            for _ in range(2):
                gy, gy_buf = be.cl(torch.zeros_like(y), extra_rows=2)
                gy.fill_(SENT)
                gz, gz_buf = be.cl(torch.zeros_like(z_gp), extra_rows=2)
                gz.fill_(SENT)
                res = K.tail_heads_bwd_proj(be.cl(y), d, f, labd, ct_i, gout, B, lam2, M, ms, Pk[0], Pk[2], out=gy, y_gp=y_gp, out_gp=gz)
                assert res[0] is gy
                be.sync()
                assert (gy_buf[3 * B:] == SENT).all() and (gz_buf[n_gp:] == SENT).all()
                runs.append([t.clone() for t in res] + [gz.clone()])
            C.check_tail_grads('proj tail_heads bwd', runs[0][:4], gr[:-1], gr[-1])
            C.close('proj gp_head_grad (riding)', runs[0][4], gz_ref, C.FWD_TOL)
            assert torch.equal(runs[0][3][absent].cpu(), torch.zeros(len(absent), nf))
            for a, b in zip(*runs):
                assert torch.equal(a, b)                     # the same bits on every run
            raw = _raw_bwd_proj(K, be.cl(y), d, f, labd, ct_i, gout, B, lam2, M, ms, Pk[0], Pk[2])
            for a, b in zip(raw, runs[0][:4]):
                assert torch.equal(a, b)                     # every element written over the sentinel, absent classes' zeros included
        # ---- generator step: one label per row
        n = 3 * B
        costr, dgr = PO.gen_heads(zr, mask.double(), P[0], P[1], P[2], lab3)
        go = C.f32(0.6)
        (gref,) = torch.autograd.grad(costr * go, zr)
        lab3d = be.dev(lab3)
        cost, dg = K.gen_heads_fwd_proj(be.cl(y), Pk[0], Pk[1], Pk[2], lab3d)
        C.close_scalar('proj gen_heads fwd', cost, costr.detach())
        C.close('proj gen_heads fwd d', dg, dgr.detach(), C.DOT_TOL)
        gy = K.gen_heads_bwd_proj(be.cl(y), lab3d, be.dev(torch.tensor([go])), ms, Pk[0], Pk[2])
        C.close_l2('proj gen_heads bwd', gy, gref, float(gref.abs().max()))
        yg = be.cl(y).requires_grad_(True)
        cost2, d2 = F.gen_tail_heads(yg, Pk[0], Pk[1], None, None, lab3d, 0.0, ms, emb=Pk[2])
        assert torch.equal(cost2.reshape(1), cost) and torch.equal(d2, dg)
        (gy2,) = torch.autograd.grad(cost2 * go, yg)
        assert torch.equal(gy2, gy)
        # ---- the penalty's seed and its adjoint, one label per row
        gg = torch.randn(n, nf, H, W, generator=g)
        wr, er = w_out.double().requires_grad_(True), emb.double().requires_grad_(True)
        gz_ref = PO.gp_seed(zr, mask.double(), wr, er, lab3, create_graph=True)
        gw_ref, ge_ref = torch.autograd.grad((gz_ref * gg.double()).sum(), [wr, er])
        absent3 = [c for c in range(L) if c not in lab3.tolist()]
        gz, buf = be.cl(torch.zeros_like(y), extra_rows=1)
        gz.fill_(SENT)
        assert K.gp_head_grad_proj(be.cl(y), Pk[0], ms, Pk[2], lab3d, out=gz) is gz
        C.close('proj gp_head_grad', gz, gz_ref.detach(), C.FWD_TOL)
        be.sync()
        assert (buf[n:] == SENT).all()
        runs = [K.gp_head_wgrad_proj(be.cl(gg), be.cl(y), ms, Pk[0], Pk[2], lab3d) for _ in range(2)]
        assert tuple(runs[0][0].shape) == (nf, 1) and tuple(runs[0][1].shape) == (L, nf)
        C.close('proj gp_head_wgrad gw', runs[0][0], gw_ref, C.GRAD_TOL)
        C.close('proj gp_head_wgrad g_emb', runs[0][1], ge_ref, C.GRAD_TOL)
        assert torch.equal(runs[0][1][absent3].cpu(), torch.zeros(len(absent3), nf))
        assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
        base_w, base_e = torch.randn(nf, 1, generator=g), torch.randn(L, nf, generator=g)
        acc_w, acc_e = be.dev(base_w), be.dev(base_e)
        res = K.gp_head_wgrad_proj(be.cl(gg), be.cl(y), ms, Pk[0], Pk[2], lab3d, add_to=acc_w, add_to_emb=acc_e)
        assert res[0] is acc_w and res[1] is acc_e
        C.close('proj gp_head_wgrad gw', acc_w, base_w.double() + gw_ref, C.GRAD_TOL)
        C.close('proj gp_head_wgrad g_emb', acc_e, base_e.double() + ge_ref, C.GRAD_TOL)
        assert torch.equal(acc_e[absent3].cpu(), base_e[absent3])
        # through autograd: GpHeadGradProjFn returns both adjoints from one launch pair
        wd, ed = be.dev(w_out).requires_grad_(True), be.dev(emb).requires_grad_(True)
        gz2 = F.gp_head_grad(be.cl(y), wd, ms, emb=ed, labels=lab3d)
        gw2, ge2 = torch.autograd.grad((gz2 * be.cl(gg)).sum(), [wd, ed])
        assert torch.equal(gz2, gz) and torch.equal(gw2, runs[0][0]) and torch.equal(ge2, runs[0][1])


@pytest.mark.parametrize('B,nf,H,W', [c[:4] for c in C.TAIL_CRITIC_CASES] + [(64, 128, 8, 8)])
def test_zero_table_gives_the_twins_bits(be, B, nf, H, W):
    """Every `_proj` launch with a table of zeros against its twin, torch.equal on the device: w_out + 0.0 is exact and the launches share
    their kernels' bodies, grids and summation orders.  gp_head_wgrad_proj reads no table at all; its gw differs from the twin's in the ORDER
    of the additions wherever the twin's 64 slices of the (row, hw) axis are not whole rows (the per-row first stage this form needs), so
    there it is held to the twin's bound against fp64 instead - and to the twin's bits at 64 rows, the critic step's shape."""
    K = be.K
    L, lam2, keep = 10, 2.0, 0.5
    ms = 1.0 / keep
    g, z, mask, w_out, b_out, emb, lab, _, Ms = _inputs(B, nf, H, W, L, 'own', zero_table=True)
    assert not emb.any()
    y = be.cl(torch.relu(z) * mask)
    labd, lab3d = be.dev(lab), be.dev(lab.repeat(3))
    w, b, e = be.dev(w_out), be.dev(b_out), be.dev(emb)
    n_gp = min(B, 7)
    z_gp, m_gp = C.masked_relu_inputs(g, n_gp, nf, H, W, keep)
    y_gp = be.cl(torch.relu(z_gp) * m_gp)
    sl = be.dev(torch.rand(B, generator=g) + 0.5)
    for M in Ms:
        s0, s1 = be.dev(torch.full((1,), SENT)), be.dev(torch.full((1,), SENT))
        t_out, t_f, t_d, t_a, t_ct, t_probs, t_acc = K.tail_critic_heads_fwd(y, B, w, b, None, None, labd, s0, lam2, M, 0.0, slopes=sl, gp_lambda=10.0)
        p_out, p_f, p_d, p_ct = K.tail_critic_heads_fwd_proj(y, B, w, b, e, labd, s1, lam2, M, slopes=sl, gp_lambda=10.0)
        for a, c in ((p_out, t_out), (p_f, t_f), (p_d, t_d), (p_ct, t_ct), (s1, s0)):
            assert torch.equal(a, c)
        for gout in (be.dev(torch.tensor([C.f32(0.8)])), be.dev(torch.tensor(C.HEAD_W))):
            gz_t, gz_p = torch.full_like(y_gp, SENT), torch.full_like(y_gp, SENT)
            t = K.tail_heads_bwd(y, t_d, t_f, None, labd, t_ct, gout, B, lam2, M, 0.0, ms, w, None, y_gp=y_gp, out_gp=gz_t)
            p = K.tail_heads_bwd_proj(y, p_d, p_f, labd, p_ct, gout, B, lam2, M, ms, w, e, y_gp=y_gp, out_gp=gz_p)
            for a, c in zip(p[:3] + (gz_p,), t[:3] + (gz_t,)):
                assert torch.equal(a, c)
    t_cost, _, t_d = K.gen_heads_fwd(y, w, b, None, None, lab3d, 0.0)
    p_cost, p_d = K.gen_heads_fwd_proj(y, w, b, e, lab3d)
    assert torch.equal(p_cost, t_cost) and torch.equal(p_d, t_d)
    go = be.dev(torch.tensor([C.f32(0.6)]))
    assert torch.equal(K.gen_heads_bwd_proj(y, lab3d, go, ms, w, e), K.gen_heads_bwd(y, None, lab3d, go, 0.0, ms, w, None))
    assert torch.equal(K.gp_head_grad_proj(y, w, ms, e, lab3d), K.gp_head_grad(y, w, ms))
    n = 3 * B
    rows = 64 if n >= 64 else n
    gg = be.cl(torch.randn(rows, nf, H, W, generator=g))
    yw = y[:rows]
    p_gw, _ = K.gp_head_wgrad_proj(gg, yw, ms, w, e, lab3d[:rows].contiguous())
    gw_ref = (gg.double() * (yw > 0)).sum(dim=(0, 2, 3)).reshape(nf, 1).cpu() * (ms / (H * W))
    C.close('proj gp_head_wgrad gw', p_gw, gw_ref, C.GRAD_TOL)
    if (nf // 4) <= 256 and 256 % (nf // 4) == 0:           # the shapes the twin accepts
        t_gw = K.gp_head_wgrad(gg, yw, ms, w)
        C.close('gp_head_wgrad', t_gw, gw_ref, C.GRAD_TOL)
        if rows == 64:                                       # one slice of the twin = one row: the same additions in the same order
            assert torch.equal(p_gw, t_gw)
            base = be.dev(torch.randn(nf, 1, generator=g))
            a_w, a_e = base.clone(), torch.zeros_like(e)
            K.gp_head_wgrad_proj(gg, yw, ms, w, e, lab3d[:rows].contiguous(), add_to=a_w, add_to_emb=a_e)
            assert torch.equal(a_w, K.gp_head_wgrad(gg, yw, ms, w, add_to=base.clone()))


# ----------------------------------------------------------------------------------------------------------------- the critic step
DIM, BS = 64, 8          # the smallest configuration tests/test_gpu_resnet_step.py runs hand-scheduled


def _build(R, lib, seed=1, **kw):
    lib.delete_all_params(); lib.set_device(None); lib.set_seed(seed)
    R.configure(DIM_G=32, DIM_D=DIM, BATCH_SIZE=BS, PROJECTION=True, **COND, **kw)
    R.build_params()


def test_hand_scheduled_step_equals_the_autograd_step_with_the_projection():
    """critic_schedule.critic_step with its three `_proj` call sites against d_losses + autograd (the fused heads' autograd forms), same weights,
    inputs and Philox streams - at the tolerances of test_hand_scheduled_critic_step_equals_the_autograd_path_on_gpu."""
    import ctgan_amd.critic_schedule as CS
    import ctgan_amd.functional as F
    import ctgan_amd.gan_cifar_resnet as R
    import ctgan_amd.tflib as lib
    from tests.test_gpu_resnet_step import _cmp, _rel_l2
    res = {}
    try:
        for merged in (False, True):
            _build(R, lib)
            g = torch.Generator().manual_seed(5)
            with torch.no_grad():
                for n, p in lib._params.items():
                    if n.endswith(('.Biases', '.b')):
                        p.add_((0.1 * torch.randn(p.shape, generator=g)).to(p.device))
                lib._params[PO.TABLE].copy_((0.3 * torch.randn(10, DIM, generator=g)).to(lib._dev()))
            tr = R.Trainer(seed=3)
            real = torch.randint(0, 256, (BS, 3072), dtype=torch.int32, generator=g).to(tr.dev)
            labels = torch.tensor([3, 7, 3, 0, 9, 9, 3, 1], dtype=torch.int32).to(tr.dev)       # a repeated class, absent classes
            old, CS.MERGED_BWD = CS.MERGED_BWD, merged
            try:
                F.prepare_filters()
                fake = tr.generate_fakes(labels)[0]
                assert CS.usable(R, None, tr.rng, real, fake) == merged
                tr.rng.begin_step()
                out, grads = tr.d_grads(real, labels, fake=fake)
            finally:
                CS.MERGED_BWD = old
            res[merged] = (out, grads, [n for n, _ in tr.d_named])
    finally:
        lib.delete_all_params(); R.configure()
    a, b = res[False], res[True]
    for k in ('cost', 'wgan', 'wgan_only', 'ct', 'gp', 'd_real', 'd_fake', 'real'):
        _cmp(b[0][k], a[0][k], 1e-5, 'scheduled.' + k, atol=1e-6)
    assert a[0]['acgan'] is None and b[0]['acgan'] is None
    assert _rel_l2(b[0]['slopes'], a[0]['slopes']) < 1e-5 and _rel_l2(b[0]['gp_grads'], a[0]['gp_grads']) < 1e-5
    assert a[2] == b[2] and a[2][-1] == PO.TABLE
    for n, x, y in zip(a[2], a[1], b[1]):
        assert (x is None) == (y is None), n
        if x is not None and x.abs().max() > 0:
            assert _rel_l2(y, x) < 2e-5, (n, _rel_l2(y, x))
    ge = b[1][-1]
    assert ge is not None and torch.equal(ge[[2, 4, 5, 6, 8]].cpu(), torch.zeros(5, DIM)) and float(ge[[0, 1, 3, 7, 9]].abs().max(dim=1).values.min()) > 0


def _run(graphs, iters=3, **trainer_kw):
    """-> (critic theta, generator theta, the table, the table at its initial value) after `iters` iterations; labels of classes 0..6 only"""
    import ctgan_amd.gan_cifar_resnet as R
    import ctgan_amd.tflib as lib
    from ctgan_amd.engine import GraphedTrainer
    nrng = np.random.default_rng(1234)
    batches = [(torch.from_numpy(nrng.integers(0, 256, (BS, 3072), dtype=np.int32)).cuda(),
                torch.from_numpy(nrng.integers(0, 7, (BS,), dtype=np.int32)).cuda()) for _ in range(8)]
    try:
        _build(R, lib, seed=0)
        init = lib._params[PO.TABLE].detach().clone()
        tr = R.Trainer(seed=2024, **trainer_kw)
        assert tr.d_named[-1][0] == PO.TABLE
        eng = GraphedTrainer(tr, use_graphs=graphs)
        assert eng.graphed == graphs, eng.graph_error
        cur = [0]

        def nb():
            cur[0] += 1
            return batches[cur[0] % len(batches)]
        for it in range(iters):
            eng.train_iteration(it, nb)
        torch.cuda.synchronize()
        return tr.d_opt.theta.clone(), tr.g_opt.theta.clone(), lib._params[PO.TABLE].detach().clone(), init
    finally:
        lib.delete_all_params(); R.configure()


@pytest.mark.parametrize('kw', [{}, dict(augment='color,translation,cutout', g_average=1e-4)], ids=['plain', 'augment+average'])
def test_graph_replay_equals_eager_and_the_table_learns(kw):
    """Three iterations graph-replayed and three eager with PROJECTION on: every weight bit-identical, the table included (one more entry of
    the critic's flat bucket, nothing else knows it); the table has moved in the rows of the classes that occurred and in no other."""
    g, e = _run(True, **kw), _run(False, **kw)
    for a, b in zip(g, e):
        assert torch.equal(a, b)
    table, init = g[2], g[3]
    moved = (table != init).any(dim=1).cpu()
    assert moved[:7].all() and not moved[7:].any(), moved
    assert torch.isfinite(table).all()
