"""Every kernel and every host branch of the loss-head family (ctgan_amd/csrc/loss.hip: 28 kernels, 26 C entry points) against the fp64
references of tests/loss_heads_cases.py, at the shapes where they can go wrong: every one-workgroup batch loop past its first pass (B, 2B, 3B >
256), the one-workgroup-per-sample CT_i kernel on both sides of its threshold and of its alignment test, head_row at every slicing of its 256
threads, tail_heads_bwd_kernel with both orders of its shared-memory maximum and with the penalty pass's rows riding the launch, the weight
gradient of the penalty head with empty and ragged row slices, gp_finish on strided inputs, the guards and ties, and the refusals of the entry
points.  The case tables, the references, the input conditions and the bounds are in tests/loss_heads_cases.py (DESIGN.md section 18 lists which
case reaches which branch); tests/test_loss_standins.py runs the same checks on the fp32 stand-ins.

loss.hip's launchers record no kernel name (ctgan_last_kernel is the conv family's), so a case cannot assert which kernel ran: the routing of
ctgan_critic_heads_fwd is pinned by the four cases around its threshold instead, which differ in nothing else.

Largest errors measured on an MI355X (relerr = max-abs over the reference's max-abs; "of bound" = fraction of the l2 bound used):
  gp fwd 7.3e-8, bwd 1.1e-7                    ct fwd 8.7e-7, bwd 1.3e-7                   softmax_ce fwd 8.2e-8, bwd 5.8e-7
  mean_diff fwd 7.9e-8, bwd 4.5e-8             gan_loss fwd 8.8e-8, bwd 1.2e-7             accuracy2 2.4e-8
  critic_heads scalars 3.3e-7, ct_i 1.3e-7, gradients 0.0038 of bound                     gen_heads cost 3.1e-7, d 3.1e-7, gradient 0.012 of bound
  tail_heads f 3.3e-7, d and a 7.6e-7          tail_critic_heads scalars 1.8e-7, d 1.2e-7, ct_i 9.0e-7, gp slot 1.4e-7; gradients 0.058 of bound
  gp_head_grad 7.9e-8, gp_head_wgrad 2.7e-7    gp_finish 4.5e-8
(143 cases, 3.3 s.)  The stand-ins' figures for the same cases are in DESIGN.md section 18.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import loss_heads_cases as C  # noqa: E402


@pytest.fixture(scope='module')
def K():
    import ctgan_amd.kernels as K
    return K


@pytest.fixture(scope='module')
def be(K):
    import ctgan_amd.functional as F
    return C.Backend(K, F, 'cuda')


@pytest.fixture(scope='module', autouse=True)
def _report():
    C.MEASURED.clear()
    yield
    print('\nloss.hip, largest errors against fp64:\n' + C.report())


@pytest.mark.parametrize('B,d', C.GP_CASES)
def test_gp(be, B, d):
    """gp_slopes_kernel, gp_mean_kernel, gp_bwd_kernel (with its s > 0 guard on an all-zero row), gp_bwd_mean_kernel with and without out5."""
    C.check_gp(be, B, d)


@pytest.mark.parametrize('Mkind', C.CT_MS)
@pytest.mark.parametrize('B,nf', C.CT_CASES)
def test_ct(be, B, nf, Mkind):
    """ct_rows_kernel, ct_mean_kernel, ct_bwd_kernel at M = 0, a midpoint M (half of the hinges off) and an exact tie ct_i == M."""
    C.check_ct(be, B, nf, Mkind)


@pytest.mark.parametrize('kind', C.CE_KINDS)
@pytest.mark.parametrize('B,ncls', C.CE_CASES)
def test_softmax_ce(be, B, ncls, kind):
    """softmax_ce_fwd_kernel / softmax_ce_bwd_kernel: plain logits, logits of magnitude 80 (finite), an argmax tie in n_correct."""
    C.check_softmax_ce(be, B, ncls, kind)


@pytest.mark.parametrize('na,nb', C.MEAN_DIFF_CASES)
def test_mean_diff(be, na, nb):
    C.check_mean_diff(be, na, nb)


@pytest.mark.parametrize('loss,net,B', C.GAN_LOSS_CASES)
def test_gan_loss(be, loss, net, B):
    """gan_loss_fwd_kernel / gan_loss_bwd_kernel, all four kinds at B = 1 and past one pass of the loop (test_gpu_gan_modes has B = 37)."""
    C.check_gan_loss(be, loss, net, B)


@pytest.mark.parametrize('B,ncls,tie', C.ACC_CASES)
def test_accuracy2(be, B, ncls, tie):
    C.check_accuracy2(be, B, ncls, tie)


@pytest.mark.parametrize('B,nf,ncls,misaligned', C.CRITIC_HEADS_CASES)
def test_critic_heads(be, B, nf, ncls, misaligned):
    """critic_heads_fwd_kernel with and without its one-wave-per-row CT_i loop, critic_heads_ct_rows_kernel on its float4 and scalar branches,
    critic_heads_bwd_kernel with n_gout 1 and 4; each with and without the class head and the penalty, at M = 0, a midpoint and a tie."""
    C.check_critic_heads(be, B, nf, ncls, misaligned)


@pytest.mark.parametrize('n,nf,H,W,relu,heads,biases,ncls', C.TAIL_FWD_CASES)
def test_tail_heads_fwd(be, n, nf, H, W, relu, heads, biases, ncls):
    """tail_heads_rows_kernel / head_row over nf x hw."""
    C.check_tail_fwd(be, n, nf, H, W, relu, heads, biases, ncls)


@pytest.mark.parametrize('B,nf,H,W,ncls', C.TAIL_CRITIC_CASES)
def test_tail_critic_heads(be, B, nf, H, W, ncls):
    """tail_heads_rows_kernel with paired rows and with the clean pass's rows (clean_relu off and on), critic_heads_final_kernel with the
    penalty's mean and the accuracies folded in, tail_heads_bwd_kernel through autograd and with out / y_gp / out_gp into sentinel-guarded
    buffers."""
    C.check_tail_critic(be, B, nf, H, W, ncls)


@pytest.mark.parametrize('clean_relu', [False, True])
@pytest.mark.parametrize('B,nf,H,W,ncls', C.TAIL_CRITIC_CASES)
def test_clean_rows_of_the_folded_forward(K, be, B, nf, H, W, ncls, clean_relu):
    """ctgan_tail_critic_heads_fwd with the clean rows, through the C ABI: the wrapper keeps only the two accuracies of the clean pass, and an accuracy over a few
    rows does not move when the logits are slightly wrong.  Here f_clean and a_clean themselves are compared with fp64, for clean_relu off and
    on, next to main rows that hold negative values (they are averaged as they are: `relu` and `relu2` must not be swapped)."""
    from ctgan_amd._lib import check, lib
    g = C.gen('clean', B, nf, H, W, ncls)
    y = torch.randn(3 * B, nf, H, W, generator=g)
    w_out, b_out, w_ac, b_ac = C.head_params(g, nf, ncls)
    lab = torch.randint(0, ncls, (B,), generator=g, dtype=torch.int32)
    yc, a_c_ref = C.clean_rows_with_gap(('clean-rows', B, nf, H, W, clean_relu), 2 * B, nf, H, W, w_ac, b_ac, clean_relu)
    f_c_ref, _, _ = C.ref_tail_heads(yc.double(), None, None, w_ac.double(), b_ac.double(), relu=clean_relu)
    f_ref, d_ref, a_ref = C.ref_tail_heads(y.double(), w_out.double(), b_out.double(), w_ac.double(), b_ac.double())
    new = lambda *shape: torch.full(shape, C.SENTINEL, device='cuda')
    f, d, a, ct_i, probs, ce_i, out = new(3 * B, nf), new(3 * B), new(3 * B, ncls), new(B), new(B, ncls), new(B), new(5)
    f_c, a_c, acc = new(2 * B, nf), new(2 * B, ncls), new(2)
    ins = [be.cl(y), be.dev(w_out), be.dev(b_out), be.dev(w_ac), be.dev(b_ac), be.dev(lab), be.cl(yc)]
    p = K._ptr
    check(lib.ctgan_tail_critic_heads_fwd(p(ins[0]), B, H * W, nf, p(ins[1]), p(ins[2]), p(ins[3]), p(ins[4]), ncls, p(ins[5]), None, None, 0.0,
                                          p(ins[6]), 1 if clean_relu else 0, p(f_c), p(a_c), p(acc), 2.0, 0.0, 1.0, p(f), p(d), p(a), p(ct_i),
                                          p(probs), p(ce_i), p(out), K._stream()), 'tail_critic_heads_fwd')
    C.close('tail_heads fwd f', f_c, f_c_ref, C.FWD_TOL)
    C.close('tail_heads fwd d, a', a_c, a_c_ref, C.DOT_TOL)
    C.close('tail_heads fwd f', f, f_ref, C.FWD_TOL)
    C.close('tail_heads fwd d, a', d, d_ref, C.DOT_TOL)
    C.close('tail_heads fwd d, a', a, a_ref, C.DOT_TOL)
    want = C.acc_ref(a_c_ref, lab, B)
    assert abs(acc[0].item() - want[0]) < 1e-6 and abs(acc[1].item() - want[1]) < 1e-6


@pytest.mark.parametrize('with_a', [True, False])
@pytest.mark.parametrize('n,nf,H,W', C.GEN_HEADS_CASES)
def test_gen_heads(be, n, nf, H, W, with_a):
    """gen_heads_loss_kernel (after tail_heads_rows_kernel) and gen_heads_bwd_kernel, through the wrappers and through F.gen_tail_heads."""
    C.check_gen_heads(be, n, nf, H, W, with_a)


@pytest.mark.parametrize('nf,rows', C.GP_HEAD_CASES)
def test_gp_head(be, nf, rows):
    """gp_head_grad_kernel (also into the leading rows of a larger buffer), gp_head_wgrad_stage1/2 in their writing and accumulating forms."""
    C.check_gp_head(be, nf, rows)


def test_gp_head_grad_past_the_block_cap(be):
    C.check_gp_head_grad_large(be)


@pytest.mark.parametrize('B,C_,H,W,layout', C.GP_FINISH_CASES)
def test_gp_finish(be, B, C_, H, W, layout):
    C.check_gp_finish(be, B, C_, H, W, layout)


# ------------------------------------------------------------------------------------------------------------------------------------ refusals
def _refusals(K):
    """name -> (C entry point, arguments, outputs): each names one `return ctgan_fail` of loss.hip's entry points.  All of them are argument
    checks that return before any launch; the outputs are filled with a sentinel."""
    from ctgan_amd._lib import I64x4
    p, st = K._ptr, K._stream()
    keep, R = [], {}

    def sent(k):
        keep.append(torch.full((k + 8,), C.SENTINEL, device='cuda'))
        return keep[-1]

    def rnd(k, off=0):
        keep.append(torch.rand(k + 8, device='cuda')[off:])
        assert keep[-1].data_ptr() % 16 == 4 * off
        return keep[-1]

    lab = torch.zeros(64, dtype=torch.int32, device='cuda')
    hw, ncls = 1, 3

    def tail_fwd(name, nf, off=0, n=2):
        outs = [sent(2 * nf), sent(2), sent(2 * ncls)]
        R['tail_heads_fwd ' + name] = ('ctgan_tail_heads_fwd', [p(rnd(2 * hw * nf, off)), n, hw, nf, 0, p(rnd(nf)), p(rnd(1)), p(rnd(nf * ncls)),
                                                                p(rnd(ncls)), ncls] + [p(o) for o in outs] + [st], outs)

    def tail_critic_fwd(name, nf, off=0, B=1, gp=True, slopes=False, clean=False, w_ac=True):
        # f, d, a, ct_i, probs, ce_i, out
        outs = [sent(3 * nf), sent(3), sent(3 * ncls), sent(1), sent(ncls), sent(1), sent(5)]
        extra = [sent(2 * nf), sent(2 * ncls), sent(2)]                  # f_clean, a_clean, acc
        head = [p(rnd(3 * hw * nf, off)), B, hw, nf, p(rnd(nf)), p(rnd(1)), p(rnd(nf * ncls)) if w_ac else None, p(rnd(ncls)) if w_ac else None,
                ncls, p(lab), p(rnd(1)) if gp else None]
        tail = [2.0, 0.0, 1.0] + [p(o) for o in outs] + [st]
        if slopes or clean:
            mid = [p(rnd(1)) if slopes else None, 10.0, p(rnd(2 * hw * nf)) if clean else None, 0] + [p(o) for o in extra]
            R['tail_critic_heads_fwd (folded) ' + name] = ('ctgan_tail_critic_heads_fwd', head + mid + tail, outs + extra)
        else:
            R['tail_critic_heads_fwd ' + name] = ('ctgan_tail_critic_heads_fwd', head + [None, 0.0, None, 0, None, None, None] + tail, outs)

    def gen_fwd(name, nf, off=0, n=2):
        outs = [sent(2 * nf), sent(2), sent(2 * ncls), sent(2 * ncls), sent(1)]          # f, d, a, probs, out
        R['gen_heads_fwd ' + name] = ('ctgan_gen_heads_fwd', [p(rnd(2 * hw * nf, off)), n, hw, nf, p(rnd(nf)), p(rnd(1)), p(rnd(nf * ncls)),
                                                              p(rnd(ncls)), ncls, p(lab), 0.1] + [p(o) for o in outs] + [st], outs)

    def gen_bwd(name, nf, off=0, gy_off=0, n=2):
        gy = sent(2 * hw * nf)[gy_off:]
        R['gen_heads_bwd ' + name] = ('ctgan_gen_heads_bwd', [p(rnd(2 * hw * nf, off)), p(rnd(2 * ncls)), p(lab), p(rnd(1)), n, hw, nf, ncls, 0.1,
                                                              2.0, p(rnd(nf)), p(rnd(nf * ncls)), p(gy), st], [gy])

    def tail_bwd(name, nf=8, off=0, gy_off=0, n_gout=4, B=1, n_gp=0, gp_off=0, w_off=0):
        gy = sent(3 * hw * nf)[gy_off:]
        outs = [gy, sent(nf), sent(1), sent(nf * ncls), sent(ncls), sent(max(n_gp, 1) * hw * nf)]       # gy, gw_out, gb_out, gw_ac, gb_ac, gz_gp
        R['tail_heads_bwd ' + name] = ('ctgan_tail_heads_bwd',
                                       [p(rnd(3 * hw * nf, off)), p(rnd(3)), p(rnd(3 * nf)), p(rnd(ncls)), p(lab), p(rnd(1)), p(rnd(4)), n_gout, B, hw, nf,
                                        ncls, 2.0, 0.0, 1.0, 2.0, p(rnd(nf, w_off)), p(rnd(nf * ncls))] + [p(o) for o in outs[:5]] +
                                       [p(rnd(max(n_gp, 1) * hw * nf, gp_off)) if n_gp else None, n_gp, p(outs[5]) if n_gp else None, st], outs)

    def head_grad(name, nf=8, off=0, w_off=0, gz_off=0, n=2, hw=1):
        gz = sent(2 * nf)[gz_off:]
        R['gp_head_grad ' + name] = ('ctgan_gp_head_grad', [p(rnd(2 * nf, off)), p(rnd(nf, w_off)), n, hw, nf, 2.0, p(gz), st], [gz])

    def head_wgrad(name, nf=8, off=0, gg_off=0, ws_off=0, n=2):
        for acc in (0, 1):
            gw, ws = sent(nf), sent(64 * nf)[ws_off:]
            R['gp_head_wgrad%s %s' % (' (accumulating)' if acc else '', name)] = (
                'ctgan_gp_head_wgrad', [p(rnd(2 * hw * nf, gg_off)), p(rnd(2 * hw * nf, off)), n, hw, nf, 2.0, p(gw), p(ws), acc, st], [gw, ws])

    def finish(name, B, Cn, H, W):
        ga, sl = sent(max(B, 1) * Cn * H * W), sent(max(B, 1))
        gs = rnd(max(B, 1) * Cn * H * W)
        strides = I64x4(Cn * (H // 2) * (W // 2), (H // 2) * (W // 2), W // 2, 1)
        keep.append(strides)
        R['gp_finish ' + name] = ('ctgan_gp_finish', [p(ga), p(gs), strides, B, Cn, H, W, 0.25, p(sl), st], [ga, sl])

    for nf, why in ((6, 'nf % 4'), (1028, 'nf > 1024')):
        tail_fwd(why, nf); tail_critic_fwd(why, nf); tail_critic_fwd(why, nf, slopes=True); gen_fwd(why, nf)
    tail_fwd('y off 16 bytes', 8, off=1); tail_critic_fwd('y off 16 bytes', 8, off=1); gen_fwd('y off 16 bytes', 8, off=1)
    tail_fwd('n = 0', 8, n=0); tail_critic_fwd('B = 0', 8, B=0); gen_fwd('n = 0', 8, n=0)
    tail_critic_fwd('slopes without a gp slot', 8, gp=False, slopes=True)
    tail_critic_fwd('clean rows without the class head', 8, clean=True, w_ac=False)
    gen_bwd('nf % 4', 6); gen_bwd('y off 16 bytes', 8, off=1); gen_bwd('gy off 16 bytes', 8, gy_off=1); gen_bwd('n = 0', 8, n=0)
    tail_bwd('n_gout = 2', n_gout=2); tail_bwd('nf % 4', nf=6); tail_bwd('B = 0', B=0)
    tail_bwd('y off 16 bytes', off=1); tail_bwd('gy off 16 bytes', gy_off=1)
    tail_bwd('y_gp off 16 bytes', n_gp=2, gp_off=1); tail_bwd('w_out off 16 bytes with penalty rows', n_gp=2, w_off=1)
    head_grad('nf % 4', nf=6); head_grad('n = 0', n=0)
    head_grad('more float4s than a grid of 256-thread blocks can take', nf=1024, n=65536, hw=65536)      # (refused on the counts alone)
    head_grad('y off 16 bytes', off=1); head_grad('w_out off 16 bytes', w_off=1); head_grad('gz off 16 bytes', gz_off=1)
    head_wgrad('nf / 4 does not divide 256', nf=12); head_wgrad('nf % 4', nf=6); head_wgrad('nf / 4 > 256', nf=1028); head_wgrad('n = 0', n=0)
    head_wgrad('y off 16 bytes', off=1); head_wgrad('gg off 16 bytes', gg_off=1); head_wgrad('ws off 16 bytes', ws_off=1)
    finish('odd H', 2, 3, 5, 4); finish('odd W', 2, 3, 4, 5); finish('B = 0', 0, 3, 4, 4)
    gd, gf, ga = sent(3), sent(3 * 8), sent(3 * ncls)
    R['critic_heads_bwd n_gout = 2'] = ('ctgan_critic_heads_bwd', [p(rnd(3)), p(rnd(3 * 8)), p(rnd(ncls)), p(lab), p(rnd(1)), p(rnd(4)), 2, 1, 8, ncls,
                                                                   2.0, 0.0, 1.0, p(gd), p(gf), p(ga), st], [gd, gf, ga])
    out, gx = sent(1), sent(1)
    R['mean_diff_fwd na + nb = 0'] = ('ctgan_mean_diff_fwd', [p(rnd(1)), 0, 0, -1.0, 1.0, p(out), st], [out])
    R['mean_diff_bwd na + nb = 0'] = ('ctgan_mean_diff_bwd', [p(rnd(1)), 0, 0, -1.0, 1.0, p(gx), st], [gx])
    return R, keep


def test_entry_points_refuse_before_any_launch(K):
    """Each refusal surfaces as the ValueError that test_errors_surface_as_python_exceptions expects of a bad argument, and writes nothing."""
    from ctgan_amd._lib import check, lib
    R, keep = _refusals(K)
    assert len(R) >= 50
    for name, (fn, args, outs) in R.items():
        with pytest.raises(ValueError):
            check(getattr(lib, fn)(*args), name)
    torch.cuda.synchronize()
    for name, (fn, args, outs) in R.items():
        for o in outs:
            assert (o == C.SENTINEL).all(), name


def test_wrappers_refuse_an_empty_batch(K):
    """The `b <= 0` arm of the entry points that the wrappers reach with an empty tensor, and gan_loss's kind range."""
    e = lambda *shape: torch.empty(shape, device='cuda')
    lab = torch.empty(0, dtype=torch.int32, device='cuda')
    one = torch.ones((), device='cuda')
    calls = [lambda: K.gp_fwd(e(0, 5), 10.0), lambda: K.gp_bwd(e(0, 5), e(0), one, 10.0), lambda: K.gp_bwd_mean(e(0, 5), e(0), one, 10.0),
             lambda: K.ct_fwd(e(0), e(0), e(0, 4), e(0, 4), 2.0, 0.0), lambda: K.ct_bwd(e(0), e(0), e(0, 4), e(0, 4), e(0), one, 2.0, 0.0),
             lambda: K.softmax_ce_fwd(e(0, 3), lab), lambda: K.softmax_ce_bwd(e(0, 3), lab, one),
             lambda: K.critic_heads_fwd(e(0), e(0, 4), None, None, 0, 2.0, 0.0, 0.0), lambda: K.accuracy2(e(0, 3), lab, 0),
             lambda: K.gan_loss_fwd(e(0), 0, 0), lambda: K.gan_loss_bwd(e(0), one, 0, 0),
             lambda: K.gan_loss_fwd(torch.ones(3, device='cuda'), 3, 7), lambda: K.gan_loss_bwd(torch.ones(3, device='cuda'), one, 3, 7),
             lambda: K.mean_diff_fwd(e(0), 0, 0, -1.0, 1.0), lambda: K.mean_diff_bwd(one, 0, 0, -1.0, 1.0)]
    for i, call in enumerate(calls):
        with pytest.raises(ValueError):
            call()
