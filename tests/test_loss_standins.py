"""The fp32 torch stand-ins of the loss-head kernels (tests/cpu_kernels.py, gp_fwd ... mean_diff_bwd: every host-logic test runs on them) against
the fp64 references of tests/loss_heads_cases.py, over the case tables of tests/test_gpu_loss_paths.py - that module's fp32 twin on the CPU.  What a
stand-in has no notion of is left out: pointer alignment (the misaligned views are passed all the same), the refusals of the C entry points, and
ctgan_gan_loss_fwd/bwd, which have no stand-in.

Largest errors measured (relerr = max-abs over the reference's max-abs; "of bound" = fraction of the l2 bound used): see DESIGN.md section 18.
"""
import pytest
import torch

from tests import loss_heads_cases as C


@pytest.fixture
def be(cpu_kernels):
    import ctgan_amd.functional as F
    import ctgan_amd.kernels as K
    return C.Backend(K, F, 'cpu')


@pytest.fixture(scope='module', autouse=True)
def _report():
    C.MEASURED.clear()
    yield
    print('\nloss stand-ins, largest errors against fp64:\n' + C.report())


def test_case_tables_reach_what_they_claim():
    """Every value of every axis of the tail-heads table occurs, and the pairs that reach head_row's corners; the shared-memory orders and the
    loop passes that the tail-critic table claims."""
    T = C.TAIL_FWD_CASES
    assert {c[0] for c in T} == {1, 5} and {c[1] for c in T} == set(C.TAIL_NF) and {(c[2], c[3]) for c in T} == set(C.TAIL_HW)
    assert {c[4] for c in T} == {False, True} and {c[5] for c in T} == set(C.TAIL_HEADS) and {c[6] for c in T} == {False, True}
    assert {c[7] for c in T if c[5] in ('both', 'class')} == {1, 10, 13}
    assert {c[6] for c in T if c[5] != 'neither'} == {False, True}
    S = lambda nf: 256 // (nf // 4)
    assert any(256 % (c[1] // 4) for c in T) and any(c[1] > 256 for c in T)
    assert {c[1] for c in T if S(c[1]) == 1} == {1020, 1024}
    assert any(S(c[1]) == 256 and c[2] * c[3] < 256 for c in T) and any(c[2] * c[3] == 1 for c in T)
    assert all(c[0] * c[1] * c[2] * c[3] * 4 <= (1 << 20) for c in T)
    R = C.TAIL_CRITIC_CASES
    assert any(3 * B > nf for B, nf, *_ in R) and any(nf > 3 * B for B, nf, *_ in R)
    assert any(3 * B > 256 >= B for B, *_ in R) and any(B > 256 for B, *_ in R)
    n_all = lambda nf, nac: nf * (1 + nac) + 1 + nac
    assert {n_all(nf, ncls) % 4 for _, nf, _, _, ncls in R} == {0, 2, 3} and all(n_all(nf, 0) % 4 == 1 for _, nf, *_ in R)
    assert {rows for _, rows in C.GP_HEAD_CASES} == {1, 63, 64, 65, 1000} and all(256 % (nf // 4) == 0 for nf, _ in C.GP_HEAD_CASES)
    for rows, (n, H, W) in C.GP_HEAD_ROWS.items():
        assert n * H * W == rows


def test_reference_hinge_and_guard_conventions():
    """The two rules of the references: where(t >= 0, t, 0) has gradient 1 at the tie (torch.maximum would give 0.5), and the penalty's
    autograd gradient of an all-zero row is NaN (which the checks mask to the kernels' 0)."""
    t = torch.zeros(3, dtype=torch.float64, requires_grad=True)
    assert torch.equal(torch.autograd.grad(C.hinge(t).sum(), t)[0], torch.ones(3, dtype=torch.float64))
    assert torch.equal(torch.autograd.grad(torch.maximum(t, 0.0 * t).sum(), t)[0], torch.full((3,), 0.5, dtype=torch.float64))
    g = torch.zeros(2, 3, dtype=torch.float64); g[1] = 1.0
    g.requires_grad_(True)
    (gg,) = torch.autograd.grad(C.ref_gp(g, 10.0)[0], g)
    assert torch.isnan(gg[0]).all() and torch.isfinite(gg[1]).all()


@pytest.mark.parametrize('B,d', C.GP_CASES)
def test_gp(be, B, d):
    C.check_gp(be, B, d)


@pytest.mark.parametrize('Mkind', C.CT_MS)
@pytest.mark.parametrize('B,nf', C.CT_CASES)
def test_ct(be, B, nf, Mkind):
    C.check_ct(be, B, nf, Mkind)


@pytest.mark.parametrize('kind', C.CE_KINDS)
@pytest.mark.parametrize('B,ncls', C.CE_CASES)
def test_softmax_ce(be, B, ncls, kind):
    C.check_softmax_ce(be, B, ncls, kind)


@pytest.mark.parametrize('na,nb', C.MEAN_DIFF_CASES)
def test_mean_diff(be, na, nb):
    C.check_mean_diff(be, na, nb)


@pytest.mark.parametrize('B,ncls,tie', C.ACC_CASES)
def test_accuracy2(be, B, ncls, tie):
    C.check_accuracy2(be, B, ncls, tie)


@pytest.mark.parametrize('B,nf,ncls,misaligned', C.CRITIC_HEADS_CASES)
def test_critic_heads(be, B, nf, ncls, misaligned):
    C.check_critic_heads(be, B, nf, ncls, misaligned)


@pytest.mark.parametrize('n,nf,H,W,relu,heads,biases,ncls', C.TAIL_FWD_CASES)
def test_tail_heads_fwd(be, n, nf, H, W, relu, heads, biases, ncls):
    C.check_tail_fwd(be, n, nf, H, W, relu, heads, biases, ncls)


@pytest.mark.parametrize('B,nf,H,W,ncls', C.TAIL_CRITIC_CASES)
def test_tail_critic_heads(be, B, nf, H, W, ncls):
    C.check_tail_critic(be, B, nf, H, W, ncls)


@pytest.mark.parametrize('with_a', [True, False])
@pytest.mark.parametrize('n,nf,H,W', C.GEN_HEADS_CASES)
def test_gen_heads(be, n, nf, H, W, with_a):
    C.check_gen_heads(be, n, nf, H, W, with_a)


@pytest.mark.parametrize('nf,rows', C.GP_HEAD_CASES)
def test_gp_head(be, nf, rows):
    C.check_gp_head(be, nf, rows)


def test_gp_head_grad_past_the_block_cap(be):
    C.check_gp_head_grad_large(be)


@pytest.mark.parametrize('B,C_,H,W,layout', C.GP_FINISH_CASES)
def test_gp_finish(be, B, C_, H, W, layout):
    C.check_gp_finish(be, B, C_, H, W, layout)
