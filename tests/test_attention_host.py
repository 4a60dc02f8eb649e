"""Host logic of the self-attention block (ctgan_amd/attention.py, gan_cifar_resnet.Config.ATTENTION_G / ATTENTION_D; NOT in the reference): the
switches, the parameter registry, the identity at gamma = 0, the block and its gradients against the fp64 oracle (tests/attention_oracle.py),
the spectral-norm name rule, the checkpoint and the refused second derivative - on the CPU stand-ins (tests/attention_cpu_kernels.py).  The
kernels themselves are checked on the GPU by tests/test_gpu_attention.py.  No GPU."""
import pytest
import torch

from tests import attention_oracle as AO
from tests.attention_cpu_kernels import attention_kernels  # noqa: F401  (fixture)
from tests.test_gan_modes_host import mode_kernels  # noqa: F401  (fixture)

G_NAMES = ['Generator.Attention.' + s for s in ('Query.Filters', 'Key.Filters', 'Value.Filters', 'Out.Filters', 'gamma')]
D_NAMES = ['Discriminator.Attention.' + s for s in ('Query.Filters', 'Key.Filters', 'Value.Filters', 'Out.Filters', 'gamma')]


@pytest.fixture
def modules(attention_kernels):  # noqa: F811
    import ctgan_amd.gan_cifar_resnet as R
    import ctgan_amd.tflib as lib
    yield R, lib
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


# ----------------------------------------------------------------------------------------------------------------- switches
def test_switches_default_off_and_need_a_width_of_32s(modules):
    R, _ = modules
    assert R.Config.ATTENTION_G is False and R.Config.ATTENTION_D is False
    before = R.cfg
    for kw, words in ((dict(ATTENTION_G=True, DIM_G=48), ('ATTENTION_G', 'DIM_G')), (dict(ATTENTION_D=True, DIM_D=16), ('ATTENTION_D', 'DIM_D')),
                      (dict(ATTENTION_G=True, ATTENTION_D=True, DIM_G=64, DIM_D=72), ('ATTENTION_D', 'DIM_D'))):
        with pytest.raises(ValueError) as e:
            R.configure(**kw)
        assert all(w in str(e.value) for w in words)
        assert R.cfg is before
    assert R.configure(ATTENTION_G=True, DIM_G=96, DIM_D=72).ATTENTION_G            # the other network's width is free
    assert R.configure(ATTENTION_D=True, DIM_D=32, DIM_G=8).ATTENTION_D
    with pytest.raises(AttributeError):
        R.configure(ATTENTION=True)


def test_trainer_refuses_critic_attention_without_the_hinge_objective(modules):
    R, lib = modules
    import ctgan_amd.hinge_schedule as HS
    _build(R, lib, ATTENTION_D=True)
    with pytest.raises(ValueError) as e:
        R.Trainer(seed=1)
    assert all(w in str(e.value) for w in ('ATTENTION_D', 'hinge', 'second derivative'))
    tr = R.Trainer(seed=1, objective='hinge')
    assert [n for n, _ in tr.d_named if 'Attention' in n] == D_NAMES
    assert HS.usable(R, None, tr.rng, None, None) is False           # the autograd path serves the step
    _build(R, lib, ATTENTION_G=True)
    for objective in (None, 'hinge'):                                # the generator is only ever differentiated once
        tr = R.Trainer(seed=1, objective=objective)
        assert [n for n, _ in tr.g_named if 'Attention' in n] == G_NAMES


# ----------------------------------------------------------------------------------------------------------------- registry
def _insert(names, new, before_prefix):
    at = next(i for i, n in enumerate(names) if n.startswith(before_prefix))
    return names[:at] + new + names[at:]


def test_registry_order_off_and_on(modules):
    R, lib = modules
    lib.delete_all_params(); lib.set_device('cpu'); lib.set_seed(5)
    R.configure()
    R.configure(DIM_G=32, DIM_D=32, BATCH_SIZE=2)
    R.build_params()
    plain = list(lib._params)
    values = {n: p.detach().clone() for n, p in lib._params.items()}
    assert not [n for n in plain if 'Attention' in n]
    assert _build(R, lib, ATTENTION_G=False, ATTENTION_D=False) == plain
    on_g = _build(R, lib, ATTENTION_G=True)
    assert on_g == _insert(plain, G_NAMES, 'Generator.3.')
    on_d = _build(R, lib, ATTENTION_D=True)
    assert on_d == _insert(plain, D_NAMES, 'Discriminator.2.')
    both = _build(R, lib, ATTENTION_G=True, ATTENTION_D=True)
    assert both == _insert(_insert(plain, G_NAMES, 'Generator.3.'), D_NAMES, 'Discriminator.2.')
    for n, p in lib._params.items():                                 # every other parameter keeps its value
        if 'Attention' not in n:
            assert torch.equal(p.detach(), values[n]), n
    P = lib._params
    assert tuple(P[G_NAMES[0]].shape) == (1, 1, 32, 4) and tuple(P[G_NAMES[1]].shape) == (1, 1, 32, 4)
    assert tuple(P[G_NAMES[2]].shape) == (1, 1, 32, 16) and tuple(P[G_NAMES[3]].shape) == (1, 1, 16, 32)
    assert tuple(P[G_NAMES[4]].shape) == (1,) and float(P[G_NAMES[4]].detach()) == 0.0 and float(P[D_NAMES[4]].detach()) == 0.0
    assert not [n for n in both if 'Attention' in n and n.endswith('.Biases')]
    assert not [n for n in G_NAMES + D_NAMES if n in lib._non_trainable]


def test_zero_gate_is_the_network_without_the_block_bit_for_bit(modules):
    R, lib = modules
    g = torch.Generator().manual_seed(1)
    noise = torch.randn(4, 128, generator=g)
    labels = torch.tensor([1, 4, 7, 9], dtype=torch.int32)
    x = torch.rand(4, 3072, generator=g) * 2 - 1
    outs = {}
    for on in (False, True):
        _build(R, lib, ATTENTION_G=on, ATTENTION_D=on)
        if on:                       # the projections are present and random; only the gates are zero
            assert float(lib._params[G_NAMES[0]].abs().max()) > 0 and float(lib._params[D_NAMES[3]].abs().max()) > 0
        with torch.no_grad():
            outs[on] = (R.Generator(4, labels, noise=noise, groups=2), R.Discriminator(x, labels, 1.0, 1.0, 1.0))
    assert torch.equal(outs[True][0], outs[False][0])
    for a, b in zip(outs[True][1], outs[False][1]):
        assert (a is None and b is None) or torch.equal(a, b)


def test_forward_under_no_grad_writes_no_row_statistics(modules):
    R, lib = modules
    from tests import attention_cpu_kernels as M
    _build(R, lib, ATTENTION_G=True)
    del M.CALLS[:]
    with torch.no_grad():
        R.Generator(2, torch.zeros(2, dtype=torch.int32), noise=torch.zeros(2, 128))
    fwd = [c for c in M.CALLS if c[0] == 'attention_fwd']
    assert fwd == [('attention_fwd', (2, 256, 4, 16), False)]
    del M.CALLS[:]
    R.Generator(2, torch.zeros(2, dtype=torch.int32), noise=torch.zeros(2, 128))
    assert [c for c in M.CALLS if c[0] == 'attention_fwd'] == [('attention_fwd', (2, 256, 4, 16), True)]


# ----------------------------------------------------------------------------------------------------------------- the block against fp64
def test_block_and_every_gradient_match_the_fp64_oracle(modules):
    """gamma = 0.7, all weights random.  Bound: 1e-4 of each tensor's largest magnitude - fp32 products (eps 6e-8) summed over at most 256
    terms through four chained operators stay two orders below it; a wrong term is of order 1."""
    R, lib = modules
    from ctgan_amd import attention as A
    lib.delete_all_params(); lib.set_device('cpu'); lib.set_seed(2)
    dim, n, H = 32, 2, 8
    g = torch.Generator().manual_seed(4)
    x0 = torch.randn(n, H, H, dim, generator=g).permute(0, 3, 1, 2)
    x = x0.clone().requires_grad_(True)
    with torch.no_grad():
        A.SelfAttention('T.Attention', dim, x0)                      # creates the parameters
    _randomise(lib, 'T.Attention')
    names = ['T.Attention.' + s for s in A.PARAMS]
    assert [n_ for n_ in lib._params] == names
    params = [lib._params[n_] for n_ in names]
    y = A.SelfAttention('T.Attention', dim, x)
    gy = torch.randn(y.shape, generator=g)
    grads = torch.autograd.grad(y, [x] + params, gy)

    xr = x0.double().requires_grad_(True)
    pr = [p.detach().double().requires_grad_(True) for p in params]
    yr = AO.block(xr, *pr)
    gr = torch.autograd.grad(yr, [xr] + pr, gy.double())
    for what, a, b in [('y', y.detach(), yr.detach())] + [(nm, a, b) for nm, a, b in zip(['x'] + names, grads, gr)]:
        err = float((a.double() - b).abs().max())
        assert err <= 1e-4 * float(b.abs().max()), (what, err, float(b.abs().max()))
        assert float(b.abs().max()) > 1e-3, what                     # (a vanishing reference would check nothing)


def test_second_derivative_is_refused_by_name(modules):
    R, lib = modules
    from ctgan_amd import attention as A
    g = torch.Generator().manual_seed(4)
    q, k = (torch.randn(1, 16, 4, generator=g).requires_grad_(True) for _ in range(2))
    v = torch.randn(1, 16, 16, generator=g).requires_grad_(True)
    with pytest.raises(RuntimeError, match='AttentionFn is first order only'):
        (gq,) = torch.autograd.grad(A.attention(q, k, v).sum(), q, create_graph=True)
        torch.autograd.grad(gq.sum(), k)
    x = torch.randn(1, 16, 2, 2, generator=g).requires_grad_(True)
    gamma = torch.full((1,), 0.5, requires_grad=True)
    with pytest.raises(RuntimeError, match='AttnResidualFn is first order only'):
        (go,) = torch.autograd.grad(A.attn_residual(x, x * 2, gamma).sum(), x, create_graph=True)
        torch.autograd.grad(go.sum(), gamma)
    (gq,) = torch.autograd.grad(A.attention(q, k, v).sum(), q)        # first order is fine
    assert gq.shape == q.shape


# ----------------------------------------------------------------------------------------------------------------- neighbours
def test_spectral_name_rule_takes_the_four_filters_and_leaves_the_gate(modules):
    R, lib = modules
    from ctgan_amd.optim import spectral_normalised
    _build(R, lib, ATTENTION_D=True)
    tr = R.Trainer(seed=1, objective='hinge')
    picked = [n for n, _ in tr.d_named if 'Attention' in n and spectral_normalised(n)]
    assert picked == D_NAMES[:4] and not spectral_normalised(D_NAMES[4])


def test_checkpoint_round_trip_carries_the_block(modules, tmp_path):
    R, lib = modules
    from ctgan_amd import checkpoint
    _build(R, lib, ATTENTION_G=True, ATTENTION_D=True)
    _randomise(lib, 'Generator.Attention', seed=8, gamma=0.3)
    _randomise(lib, 'Discriminator.Attention', seed=9, gamma=-0.2)
    tr = R.Trainer(seed=1, objective='hinge')
    want = {n: p.detach().clone() for n, p in lib._params.items()}
    path = str(tmp_path / 'ck.pt')
    checkpoint.save(path, tr, 7)
    assert all(n in torch.load(path, weights_only=False)['params'] for n in G_NAMES + D_NAMES)
    with torch.no_grad():
        for n in G_NAMES + D_NAMES:
            lib._params[n].zero_()
    assert checkpoint.load(path, tr) == 7
    for n, p in lib._params.items():
        assert torch.equal(p.detach(), want[n]), n
    assert float(lib._params[G_NAMES[4]].detach()) == pytest.approx(0.3) and float(lib._params[D_NAMES[4]].detach()) == pytest.approx(-0.2)
