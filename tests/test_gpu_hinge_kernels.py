"""The hinge objective's HIP kernels (csrc/loss.hip: ctgan_gan_loss_* kinds 4 / 5, ctgan_tail_hinge_heads_fwd/bwd; csrc/optim_rng.hip:
ctgan_real_fake_prep) against the fp64 references, case tables and bounds of tests/hinge_cases.py - the table tests/test_hinge_standins.py runs
on the CPU stand-ins."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import hinge_cases as C  # noqa: E402
from tests import loss_heads_cases as L  # noqa: E402
from tests import philox_spec as S  # noqa: E402


@pytest.fixture(scope='module')
def be():
    import ctgan_amd.functional as F
    import ctgan_amd.kernels as K
    yield C.Backend(K, F, 'cuda')
    print(L.report())


@pytest.mark.parametrize('kind', C.GAN_LOSS_KINDS)
@pytest.mark.parametrize('B', C.GAN_LOSS_B)
@pytest.mark.parametrize('net', ['d', 'g'])
def test_gan_loss_hinge_kinds(be, net, B, kind):
    C.check_gan_loss_hinge(be, net, B, kind)


def test_gan_loss_kind_7_stays_a_bad_argument(be):
    from ctgan_amd._lib import check, lib
    d = torch.zeros(4, device='cuda'); out = torch.zeros((), device='cuda')
    for kind in (6, 7, -1):
        with pytest.raises(ValueError):
            check(lib.ctgan_gan_loss_fwd(d.data_ptr(), 2, kind, out.data_ptr(), None), 'gan_loss_fwd')
        with pytest.raises(ValueError):
            check(lib.ctgan_gan_loss_bwd(d.data_ptr(), out.data_ptr(), 2, kind, d.data_ptr(), None), 'gan_loss_bwd')


@pytest.mark.parametrize('B,H,W,nf,heads', C.TAIL_CASES)
def test_tail_hinge_heads(be, B, H, W, nf, heads):
    C.check_tail_hinge(be, B, H, W, nf, heads)


@pytest.mark.parametrize('B,heads,what', C.CRAFTED)
def test_tail_hinge_heads_crafted(be, B, heads, what):
    C.check_tail_hinge_crafted(be, B, heads, what)


def test_tail_hinge_heads_refusals(be):
    C.check_tail_hinge_refusals(be)


def test_tail_hinge_heads_refuses_at_the_c_entry(be):
    """emb and w_ac together, B = 0, nf % 4 != 0, nf > 1024, a misaligned or null y: CTGAN_E_BADARG (the ValueError of _lib.check) before any
    launch - nothing is written."""
    from ctgan_amd._lib import check, lib
    buf = torch.zeros(1 << 16, device='cuda')
    lab = torch.zeros(8, dtype=torch.int32, device='cuda')
    p, lp = buf.data_ptr(), lab.data_ptr()

    def fwd(y=p, B=2, nf=32, emb=None, w_ac=None):
        return lib.ctgan_tail_hinge_heads_fwd(y, B, 4, nf, p, p, emb, 10, w_ac, p if w_ac else None, 10, lp, 0.5, p, p, p, p, p, p, p, None)

    def bwd(y=p, B=2, nf=32, emb=None, w_ac=None):
        return lib.ctgan_tail_hinge_heads_bwd(y, p, p, p, lp, p, B, 4, nf, 10, 0.5, 2.0, p, emb, 10, w_ac, p, p, p, p, p, p, None)
    for f in (fwd, bwd):
        for kw in (dict(emb=p, w_ac=p), dict(B=0), dict(nf=30), dict(nf=1028), dict(y=p + 4), dict(y=None)):
            with pytest.raises(ValueError):
                check(f(**kw), 'tail_hinge_heads')
    torch.cuda.synchronize()
    assert bool((buf == 0).all())


@pytest.mark.parametrize('B,d', C.PREP_CASES)
@pytest.mark.parametrize('corner', sorted(S.CORNERS))
def test_real_fake_prep(be, corner, B, d):
    C.check_real_fake_prep(be, corner, B, d)


def test_real_fake_prep_refusals(be):
    C.check_real_fake_prep_refusals(be)
