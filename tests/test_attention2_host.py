"""Host logic of the second derivative of self-attention (ctgan_amd/attention.py: attention2, attn_residual2, SelfAttention(..., second_order=True);
gan_cifar_resnet.Config.ATTENTION_SECOND_ORDER): the switch, the Trainer's acceptance and its pinned refusal, the registry, the two
schedule predicates, the block's double backward against fp64 (tests/attention_oracle.py differentiated twice), the refused third derivative
and the checkpoint across the switch - on the CPU stand-ins (tests/attention2_cpu_kernels.py).  The kernels themselves are checked on the GPU
by tests/test_gpu_attention2.py.  No GPU."""
import pytest
import torch

from tests import attention_oracle as AO
from tests.attention2_cpu_kernels import attention2_kernels  # noqa: F401  (fixture)
from tests.attention_cpu_kernels import attention_kernels  # noqa: F401  (fixture)
from tests.test_gan_modes_host import mode_kernels  # noqa: F401  (fixture)

D_NAMES = ['Discriminator.Attention.' + s for s in ('Query.Filters', 'Key.Filters', 'Value.Filters', 'Out.Filters', 'gamma')]
ON = dict(ATTENTION_D=True, ATTENTION_SECOND_ORDER=True)


@pytest.fixture
def modules(attention2_kernels):  # noqa: F811
    import ctgan_amd.gan_cifar_resnet as R
    import ctgan_amd.tflib as lib
    yield R, lib
    lib.delete_all_params()
    R.configure()


def _build(R, lib, dim=32, B=2, seed=5, **kw):
    lib.delete_all_params(); lib.set_device('cpu'); lib.set_seed(seed)
    R.configure(DIM_G=dim, DIM_D=dim, BATCH_SIZE=B, **kw)
    R.build_params()
    return list(lib._params)


def _randomise(lib, prefix, seed=3, gamma=0.7):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for n, p in lib._params.items():
            if n.startswith(prefix):
                if n.endswith('gamma'):
                    p.fill_(gamma)
                else:
                    p.copy_(torch.randn(p.shape, generator=g) * 0.2)


# ----------------------------------------------------------------------------------------------------------------- the switch
def test_switch_defaults_off_and_needs_the_critic_block(modules):
    R, _ = modules
    assert R.Config.ATTENTION_SECOND_ORDER is False
    before = R.cfg
    for kw in (dict(ATTENTION_SECOND_ORDER=True), dict(ATTENTION_SECOND_ORDER=True, ATTENTION_G=True)):
        with pytest.raises(ValueError) as e:
            R.configure(**kw)
        assert 'ATTENTION_SECOND_ORDER' in str(e.value) and 'ATTENTION_D' in str(e.value)
        assert R.cfg is before
    assert R.configure(**ON).ATTENTION_SECOND_ORDER


def test_trainer_accepts_the_ct_objective_with_the_switch_and_still_refuses_without(modules):
    R, lib = modules
    _build(R, lib, **ON)
    for objective in (None, 'hinge'):                                # under the hinge objective the switch is harmless
        tr = R.Trainer(seed=1, objective=objective)
        assert [n for n, _ in tr.d_named if 'Attention' in n] == D_NAMES
    _build(R, lib, ATTENTION_D=True)
    with pytest.raises(ValueError) as e:
        R.Trainer(seed=1)
    assert all(w in str(e.value) for w in ('ATTENTION_D', 'hinge', 'second derivative', 'ATTENTION_SECOND_ORDER'))


def test_registry_is_the_first_order_blocks(modules):
    """names, creation order, shapes and initial values do not depend on the switch"""
    R, lib = modules
    off = _build(R, lib, ATTENTION_G=True, ATTENTION_D=True)
    values = {n: p.detach().clone() for n, p in lib._params.items()}
    on = _build(R, lib, ATTENTION_G=True, **ON)
    assert on == off and [n for n in on if n.startswith('Discriminator.Attention')] == D_NAMES
    for n, p in lib._params.items():
        assert torch.equal(p.detach(), values[n]), n
    assert not [n for n in D_NAMES if n in lib._non_trainable]


def test_both_hand_schedules_stand_aside_for_the_critic_block(modules):
    """critic_schedule.usable says no because of ATTENTION_D itself: the same call without the block says yes"""
    R, lib = modules
    import ctgan_amd.critic_schedule as CS
    import ctgan_amd.hinge_schedule as HS
    real = torch.zeros(2, 3072, dtype=torch.int32)
    fake = torch.zeros(2, 3072)
    seen = {}
    for name, kw in (('plain', {}), ('block', dict(ATTENTION_D=True)), ('second', ON)):
        _build(R, lib, dim=64, **kw)                                 # (64: the width from which the hand schedules apply at all)
        tr = R.Trainer(seed=1, objective='hinge')
        seen[name] = (CS.usable(R, None, tr.rng, real, fake), HS.usable(R, None, tr.rng, real, fake), R._critic_piecewise_linear())
    assert seen['plain'] == (True, True, True)
    assert seen['block'] == (False, False, False) and seen['second'] == (False, False, False)


# ----------------------------------------------------------------------------------------------------------------- the block against fp64
def _second_grads(block, x, params, gy, cot):
    y = block(x, *params)
    (gx,) = torch.autograd.grad(y, x, gy, create_graph=True)
    return y, gx, torch.autograd.grad((gx * cot).sum(), [x] + list(params), allow_unused=True)


def test_double_backward_of_the_block_matches_the_fp64_oracle(modules):
    """gamma = 0.7, all weights random: d<block(x), gy>/dx under create_graph, then the gradient of <that, cot> in x and in every parameter.
    Bound: 1e-4 of each tensor's largest magnitude (that of tests/test_attention_host.py: fp32 products summed over at most 256 terms through
    a few chained operators stay two orders below it; a wrong or missing term is of order 1).  Forward and first-order gradients are the
    first-order operator's bits, with the same stand-in launches."""
    R, lib = modules
    from ctgan_amd import attention as A
    from tests import attention_cpu_kernels as M
    lib.delete_all_params(); lib.set_device('cpu'); lib.set_seed(2)
    dim, n, H = 32, 2, 8
    g = torch.Generator().manual_seed(4)
    x0 = torch.randn(n, H, H, dim, generator=g).permute(0, 3, 1, 2)
    with torch.no_grad():
        A.SelfAttention('T.Attention', dim, x0, second_order=True)      # creates the parameters
    _randomise(lib, 'T.Attention')
    names = ['T.Attention.' + s for s in A.PARAMS]
    assert list(lib._params) == names
    params = [lib._params[n_] for n_ in names]
    gy, cot = torch.randn(x0.shape, generator=g), torch.randn(x0.shape, generator=g)

    x = x0.clone().requires_grad_(True)
    y, gx, second = _second_grads(lambda x_, *_: A.SelfAttention('T.Attention', dim, x_, second_order=True), x, params, gy, cot)
    assert [c[0] for c in M.CALLS if c[0].endswith('bwd2')] == ['attention_bwd2', 'attn_residual_bwd2']
    xr = x0.double().requires_grad_(True)
    pr = [p.detach().double().requires_grad_(True) for p in params]
    yr, gxr, second_r = _second_grads(AO.block, xr, pr, gy.double(), cot.double())
    for what, a, b in [('y', y, yr), ('gx', gx, gxr)] + list(zip(['d2 x'] + ['d2 ' + n_ for n_ in names], second, second_r)):
        assert a is not None and b is not None, what
        err = float((a.detach().double() - b.detach()).abs().max())
        assert float(b.detach().abs().max()) > 1e-3, what                     # (a vanishing reference would check nothing)
        assert err <= 1e-4 * float(b.detach().abs().max()), (what, err)

    outs = []
    for second_order in (False, True):
        del M.CALLS[:]
        x1 = x0.clone().requires_grad_(True)
        y1 = A.SelfAttention('T.Attention', dim, x1, second_order=second_order)
        outs.append((y1.detach(),) + torch.autograd.grad(y1, [x1] + params, gy) + (list(M.CALLS),))
    assert outs[0][-1] == outs[1][-1] and not [c for c in outs[1][-1] if c[0].endswith('bwd2')]
    for a, b in zip(outs[0][:-1], outs[1][:-1]):
        assert torch.equal(a, b)


def test_third_derivative_is_refused_by_name(modules):
    from ctgan_amd import attention as A
    g = torch.Generator().manual_seed(4)
    q, k = (torch.randn(1, 16, 4, generator=g).requires_grad_(True) for _ in range(2))
    v = torch.randn(1, 16, 16, generator=g).requires_grad_(True)
    (gq,) = torch.autograd.grad(A.attention2(q, k, v).sum(), q, create_graph=True)
    with pytest.raises(RuntimeError, match='AttentionBwdFn is first order only'):
        torch.autograd.grad(gq.sum(), k, create_graph=True)
    (gk,) = torch.autograd.grad(gq.sum(), k)                             # the second derivative itself is fine
    assert gk.shape == k.shape and float(gk.abs().max()) > 0
    x = torch.randn(1, 16, 2, 2, generator=g).requires_grad_(True)
    gamma = torch.full((1,), 0.5, requires_grad=True)
    (go,) = torch.autograd.grad(A.attn_residual2(x.detach(), x * 2, gamma).sum(), x, create_graph=True)
    with pytest.raises(RuntimeError, match='AttnResidualBwdFn is first order only'):
        torch.autograd.grad(go.sum(), gamma, create_graph=True)
    (gg,) = torch.autograd.grad(go.sum(), gamma)
    assert float(gg) == pytest.approx(2.0 * x.numel())                   # go = 2 gamma 1: d sum(go) / d gamma = 2 numel


def test_ct_critic_step_runs_on_the_autograd_path_and_reaches_the_block(modules):
    """Trainer(objective=None).d_step with the block: the penalty is non-zero and every parameter of the block has a gradient"""
    R, lib = modules
    from tests import attention_cpu_kernels as M
    _build(R, lib, B=2, **ON)
    _randomise(lib, 'Discriminator.Attention', seed=9, gamma=0.5)
    lib.bump_epoch()
    tr = R.Trainer(seed=1)
    nrng = torch.Generator().manual_seed(2)
    real = torch.randint(0, 256, (2, 3072), generator=nrng, dtype=torch.int32)
    labels = torch.randint(0, 10, (2,), generator=nrng, dtype=torch.int32)
    before = lib._params[D_NAMES[4]].detach().clone()
    del M.CALLS[:]
    out = tr.d_step(real, labels, iteration=0)
    assert [c[0] for c in M.CALLS if c[0].endswith('bwd2')] == ['attention_bwd2', 'attn_residual_bwd2']
    assert float(out['gp']) > 0 and torch.isfinite(out['cost'])
    for n in D_NAMES:
        assert out['grads'][n] is not None and float(out['grads'][n].abs().max()) > 0, n
    assert not torch.equal(lib._params[D_NAMES[4]].detach(), before)


def test_checkpoint_round_trip_across_the_switch(modules, tmp_path):
    R, lib = modules
    from ctgan_amd import checkpoint
    for first, then in ((dict(ATTENTION_D=True), ON), (ON, dict(ATTENTION_D=True))):
        _build(R, lib, **first)
        _randomise(lib, 'Discriminator.Attention', seed=9, gamma=-0.2)
        tr = R.Trainer(seed=1, objective='hinge')
        want = {n: p.detach().clone() for n, p in lib._params.items()}
        path = str(tmp_path / ('ck_%d.pt' % len(first)))
        checkpoint.save(path, tr, 7)
        _build(R, lib, seed=6, **then)
        tr = R.Trainer(seed=1, objective='hinge')
        assert checkpoint.load(path, tr) == 7
        assert list(lib._params) == list(want)
        for n, p in lib._params.items():
            assert torch.equal(p.detach(), want[n]), n
