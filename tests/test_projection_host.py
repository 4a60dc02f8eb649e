"""Host logic of the projection head of the conditional ResNet critic (gan_cifar_resnet.Config.PROJECTION; NOT in the reference): the switch, the
table parameter, the three forms of the critic step (op-by-op head / fused heads under autograd / critic_schedule.critic_step), the generator
step, the dev cost and the checkpoint - on the CPU stand-ins (tests/projection_cpu_kernels.py) against the fp64 oracle
(tests/projection_oracle.py).  The kernels themselves are checked on the GPU by tests/test_gpu_projection.py.  No GPU."""
import numpy as np
import pytest
import torch

from oracle import nets as onets, philox, steps as osteps
from tests import eval_helpers as H
from tests import loss_heads_cases as C
from tests import projection_oracle as PO
from tests import cond_layernorm_oracle as LO
from tests.projection_cpu_kernels import cond_cpu_kernels, projection_cpu_kernels  # noqa: F401  (fixtures)
from tests.test_cond_layernorm_model import cmp_l2, cmp_max, randomise_tables
from tests.test_host_logic_resnet import _cmp, _oracle_from_product

TABLE = PO.TABLE
COND = dict(CONDITIONAL=True, ACGAN=False)


def _build(R, lib, dim, B, seed=5, dim_g=None, **kw):
    lib.delete_all_params(); lib.set_device('cpu'); lib.set_seed(seed)
    R.configure(DIM_G=dim_g or dim, DIM_D=dim, BATCH_SIZE=B, **kw)
    R.build_params()


def _set_table(lib, value=None, seed=11):
    """value None: a random table of the output weight's size; else a constant"""
    with torch.no_grad():
        p = lib._params[TABLE]
        if value is None:
            p.copy_(torch.randn(p.shape, generator=torch.Generator().manual_seed(seed)) * 0.3)
        else:
            p.fill_(value)


def _shake_biases(lib, seed=5):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for n, p in lib._params.items():
            if n.endswith(('.Biases', '.b')):                # zero-initialised in the reference: make them count
                p.add_(0.1 * torch.randn(p.shape, generator=g))


@pytest.fixture
def modules(projection_cpu_kernels):  # noqa: F811
    import ctgan_amd.gan_cifar_resnet as R
    import ctgan_amd.tflib as lib
    yield R, lib
    R.configure()


# ----------------------------------------------------------------------------------------------------------------- 1: switch semantics
def test_projection_needs_a_conditional_critic_without_the_classifier(modules):
    R, _ = modules
    before = R.cfg
    for kw in (dict(PROJECTION=True, ACGAN=True), dict(PROJECTION=True, CONDITIONAL=False), dict(PROJECTION=True, CONDITIONAL=False, ACGAN=False),
               dict(PROJECTION=True)):
        with pytest.raises(ValueError) as e:
            R.configure(**kw)
        assert all(flag in str(e.value) for flag in ('PROJECTION', 'CONDITIONAL', 'ACGAN'))
        assert R.cfg is before                               # a rejected configuration changes nothing
    assert R.configure(PROJECTION=True, NORMALIZATION_D=True, **COND).PROJECTION        # the normalised critic stays allowed
    assert R.Config.PROJECTION is False and not R.configure().PROJECTION


def test_projection_silences_the_effectively_unconditional_warning(modules, capsys):
    R, _ = modules
    R.configure(**COND)
    assert 'effectively unconditional' in capsys.readouterr().out
    R.configure(PROJECTION=True, **COND)
    assert 'WARNING' not in capsys.readouterr().out


def test_table_is_registered_last_and_only_when_on(modules):
    R, lib = modules
    snaps = {}
    for key, kw in (('default', dict(COND)), ('off', dict(PROJECTION=False, **COND)), ('on', dict(PROJECTION=True, **COND))):
        _build(R, lib, 8, 4, **kw)
        tr = R.Trainer(seed=1)
        snaps[key] = ([(n, p.detach().clone()) for n, p in lib._params.items()], [n for n, _ in tr.d_named], tr._n_early)
    (d_all, d_names, d_early), (f_all, f_names, f_early), (n_all, n_names, n_early) = snaps['default'], snaps['off'], snaps['on']
    assert TABLE not in dict(d_all) and [n for n, _ in f_all] == [n for n, _ in d_all] and f_names == d_names
    # on: every existing parameter keeps its place and value; the table comes after all of them - in the registry and in the critic's flat bucket
    assert [n for n, _ in n_all] == [n for n, _ in d_all] + [TABLE] and n_names == d_names + [TABLE] and n_early == d_early == f_early
    for (n, a), (_, b), (_, c) in zip(d_all, f_all, n_all):
        assert torch.equal(a, b) and torch.equal(a, c), n
    table = dict(n_all)[TABLE]
    assert tuple(table.shape) == (10, 8) and table.dtype == torch.float32 and TABLE not in lib._non_trainable
    # each row drawn as Discriminator.Output.W is: Linear's default initialiser at fan-in DIM_D, fan-out 1, from the parameter's own stream
    bound = np.sqrt(2. / (8 + 1)) * np.sqrt(3)
    want = lib.rng_for(TABLE).uniform(low=-bound, high=bound, size=(10, 8)).astype('float32')
    assert np.array_equal(table.numpy(), want) and float(table.abs().max()) <= bound and float(table.std()) > 0.3 * bound
    assert float(dict(n_all)['Discriminator.Output.W'].abs().max()) <= bound


# ----------------------------------------------------------------------------------------------------------------- 2: zero table == no table
def _critic_and_generator_step(R, lib, dim, B, proj, merged, table, labels, real):
    """losses and gradients of one critic step (d_grads, which draws its own fakes) and one generator step from identical weights, inputs
    and Philox streams (both at stream position 0)"""
    import ctgan_amd.critic_schedule as CS
    import ctgan_amd.functional as F
    _build(R, lib, dim, B, PROJECTION=proj, **COND)
    _shake_biases(lib)
    if proj:
        _set_table(lib, table)
    tr = R.Trainer(seed=3)
    calls = []
    old, orig = CS.MERGED_BWD, CS.critic_step
    CS.MERGED_BWD = merged
    CS.critic_step = lambda *a, **k: (calls.append(1), orig(*a, **k))[1]
    try:
        F.prepare_filters()
        tr.rng.begin_step()
        out, grads = tr.d_grads(real, labels)
        tr.rng.begin_step()
        gout = tr.g_losses()
        ggrads = torch.autograd.grad(gout['cost'], tr.g_params, allow_unused=True)
    finally:
        CS.MERGED_BWD, CS.critic_step = old, orig
    assert bool(calls) == merged, 'the critic step did not take the form under test'
    return out, dict(zip([n for n, _ in tr.d_named], grads)), gout['cost'].detach(), dict(zip([n for n, _ in tr.g_named], ggrads))


@pytest.mark.parametrize('merged', [False, True])
def test_zero_table_is_the_unprojected_critic_bit_for_bit(modules, merged):
    """w_out + 0.0 is exact: with Discriminator.Projection.W = 0 every loss, every shared parameter's gradient and the generator step equal the
    configuration without PROJECTION at the same seed and counter - on the fused heads under autograd and on critic_schedule.critic_step.
    The gradient of the table itself does not vanish: it is checked against the fp64 oracle (the tolerances
    test_hand_scheduled_critic_step_matches_oracle_on_identical_philox_streams uses for the same quantities)."""
    R, lib = modules
    B, dim = 2, (64 if merged else 8)
    labels = torch.tensor([3, 7], dtype=torch.int32)
    real = torch.randint(0, 256, (B, 3072), dtype=torch.int32, generator=torch.Generator().manual_seed(5))
    off = _critic_and_generator_step(R, lib, dim, B, False, merged, None, labels, real)
    on = _critic_and_generator_step(R, lib, dim, B, True, merged, 0.0, labels, real)
    for k in ('cost', 'wgan', 'wgan_only', 'ct', 'gp', 'slopes', 'gp_grads', 'd_real', 'd_fake', 'real'):
        assert torch.equal(on[0][k], off[0][k]), k
    assert on[0]['acgan'] is None and 'acc_real' not in on[0]
    assert list(on[1]) == list(off[1]) + [TABLE]
    for n, gv in off[1].items():
        assert (gv is None) == (on[1][n] is None) and (gv is None or torch.equal(on[1][n], gv)), n
    assert torch.equal(on[2], off[2])
    for n, gv in off[3].items():
        assert (gv is None) == (on[3][n] is None) and (gv is None or torch.equal(on[3][n], gv)), n
    # the table's own gradient: fp64 oracle on the step's Philox streams (the `on` build is the live one)
    g_table = on[1][TABLE]
    assert g_table is not None and float(g_table.abs().max()) > 0
    reg = _oracle_from_product(lib)
    cfg = onets.ResnetCfg(DIM_G=dim, DIM_D=dim, **COND)
    ref = PO.d_losses(reg, cfg, real, labels, philox.rnd_resnet_d(3, 0, 0, B, dim), B)
    _cmp(on[0]['cost'], ref['cost'], 2e-4, 'cost', atol=1e-6)
    want = PO.grads_of(reg, ref['cost'], 'Discriminator.')
    _cmp(g_table, want[TABLE], 1e-3, 'table gradient', atol=1e-6)
    absent = [c for c in range(10) if c not in labels.tolist()]
    assert torch.equal(g_table[absent], torch.zeros(len(absent), dim))


# ----------------------------------------------------------------------------------------------------------------- 3: it is the projection
@pytest.mark.parametrize('norm_d', [False, True])
def test_projection_identity_and_steps_against_the_oracle(modules, monkeypatch, norm_d):
    """Parity mode (injected draws, the op-by-op head; with NORMALIZATION_D also the label-conditioned Layernorm): for fixed dropout draws
    D(x, y) - D(x, y') = f(x) . (E[y] - E[y']); d_losses, g_losses and every parameter gradient, the table's included, against fp64 - at the
    tolerances test_host_logic_resnet.py applies to the same quantities (test_d_step_and_g_step_match_oracle), and for the label-conditioned
    Layernorm critic at those of tests/test_cond_layernorm_model.py's check_steps (scalars 5e-4 max, dD/dx_hat 2e-3 and gradients 5e-3 in L2)."""
    R, lib = modules
    B, dim = 4, 8
    if norm_d:                     # the oracle's Normalize with the label-conditioned Layernorm, as tests/test_cond_layernorm_model.py installs it
        monkeypatch.setattr(onets, 'Normalize', LO.normalize)
    _build(R, lib, dim, B, PROJECTION=True, NORMALIZATION_D=norm_d, **COND)
    if norm_d:
        randomise_tables(lib)
    _set_table(lib)
    E = lib._params[TABLE].detach()
    g = torch.Generator().manual_seed(1)
    x = torch.rand(6, 3072, generator=g) * 2 - 1
    u = [torch.rand(6, dim, 8, 8, generator=g) for _ in range(3)]
    y0 = torch.tensor([0, 1, 2, 3, 9, 9], dtype=torch.int32)
    y1 = torch.tensor([9, 1, 5, 0, 9, 2], dtype=torch.int32)
    with torch.no_grad():
        d0, f0, a0 = R.Discriminator(x, y0, 0.8, 0.5, 0.5, u=u)
        d1, f1, _ = R.Discriminator(x, y1, 0.8, 0.5, 0.5, u=u)
    assert a0 is None
    if not norm_d:                 # (a Layernorm critic's feature depends on the label too: there the identity holds for equal labels only)
        assert torch.equal(f0, f1)
        want = (f0.double() * (E[y0.long()] - E[y1.long()]).double()).sum(dim=1)
        assert float(want.abs().max()) > 1e-3
        C.close('D(x, y) - D(x, y\')', d0.double() - d1.double(), want, C.DOT_TOL * float(d0.abs().max() / want.abs().max()))
        assert torch.equal(d0[[1, 4]], d1[[1, 4]])
    reg = _oracle_from_product(lib)
    cfg = onets.ResnetCfg(DIM_G=dim, DIM_D=dim, NORMALIZATION_D=norm_d, **COND)
    real = torch.randint(0, 256, (B, 3072), generator=g, dtype=torch.int32)
    labels = torch.tensor([3, 7, 3, 0], dtype=torch.int32)
    rnd64 = osteps.make_rnd_resnet_d(B, dim, g)
    rnd32 = {k: ([t.float() for t in v] if isinstance(v, list) else v.float()) for k, v in rnd64.items()}
    tr = R.Trainer(seed=1)
    tr.rng.begin_step()
    out, grads = tr.d_grads(real, labels, rnd32)
    ref = PO.d_losses(reg, cfg, real, labels, rnd64, B)
    assert out['acgan'] is None
    want = PO.grads_of(reg, ref['cost'], 'Discriminator.')
    got = {n: gv for (n, _), gv in zip(tr.d_named, grads) if gv is not None}
    assert set(got) == set(want) and TABLE in got
    if norm_d:
        for k in ('cost', 'wgan', 'ct', 'gp', 'wgan_only'):
            cmp_max(out[k], ref[k], 5e-4, 'd_losses.' + k, atol=1e-6)
        cmp_l2(out['gp_grads'], ref['gp_grads'], 2e-3, 'dD/dx_hat')
        for n in want:
            cmp_l2(got[n], want[n], 5e-3, 'dgrad ' + n, atol=1e-7)
    else:
        for k in ('cost', 'wgan', 'ct', 'gp', 'wgan_only'):
            _cmp(out[k], ref[k], 2e-4, 'd_losses.' + k)
        _cmp(out['gp_grads'], ref['gp_grads'], 2e-4, 'gp grads')
        for n in want:
            _cmp(got[n], want[n], 5e-4, 'dgrad ' + n)
    assert torch.equal(got[TABLE][[1, 2, 4, 5, 6, 8, 9]], torch.zeros(7, dim))
    rg64 = osteps.make_rnd_resnet_g(B, dim, g)
    rg32 = {'z': [t.float() for t in rg64['z']], 'label_u': [t.float() for t in rg64['label_u']], 'u': [[t.float() for t in tw] for tw in rg64['u']]}
    tr.rng.begin_step()
    gout = tr.g_losses(rg32)
    gref = PO.g_losses(reg, cfg, rg64, B)
    ggot = dict(zip([n for n, _ in tr.g_named], torch.autograd.grad(gout['cost'], tr.g_params, allow_unused=True)))
    gwant = PO.grads_of(reg, gref['cost'], 'Generator')
    assert set(n for n, v in ggot.items() if v is not None) == set(gwant)
    if norm_d:
        cmp_max(gout['cost'], gref['cost'], 5e-4, 'g cost', atol=1e-6)
        for n in gwant:
            cmp_l2(ggot[n], gwant[n], 5e-3, 'ggrad ' + n, atol=1e-7)
    else:
        _cmp(gout['cost'], gref['cost'], 2e-4, 'g cost')
        for n in gwant:
            _cmp(ggot[n], gwant[n], 1e-3, 'ggrad ' + n)


# ----------------------------------------------------------------------------------------------------------------- 4: the three forms agree
def test_unfused_fused_and_hand_scheduled_forms_agree(modules):
    """Op-by-op head vs fused heads under autograd vs critic_schedule.critic_step, from identical weights, inputs and Philox streams, with a random
    table and labels in which a class repeats and classes are absent - at the tolerances of
    test_hand_scheduled_critic_step_equals_the_autograd_path."""
    import ctgan_amd.critic_schedule as CS
    import ctgan_amd.functional as F
    R, lib = modules
    B, D = 4, 64
    labels = torch.tensor([3, 7, 3, 0], dtype=torch.int32)
    res = {}
    for form in ('unfused', 'fused', 'scheduled'):
        _build(R, lib, D, B, seed=1, dim_g=32, PROJECTION=True, **COND)
        _shake_biases(lib)
        _set_table(lib)
        tr = R.Trainer(seed=3)
        g = torch.Generator().manual_seed(5)
        real = torch.randint(0, 256, (B, 3072), dtype=torch.int32, generator=g)
        old = CS.MERGED_BWD
        CS.MERGED_BWD = form == 'scheduled'
        R.HEAD_FUSION = R.PREP_FUSION = R.TRUNK_SHARE = R.TAIL_SHARE = form != 'unfused'
        calls = []
        orig = CS.critic_step
        CS.critic_step = lambda *a, **k: (calls.append(1), orig(*a, **k))[1]
        try:
            F.prepare_filters()
            fake = tr.generate_fakes(labels)[0]
            tr.rng.begin_step()
            out, grads = tr.d_grads(real, labels, fake=fake)
            tr.rng.begin_step()
            gout = tr.g_losses()
            ggrads = torch.autograd.grad(gout['cost'], tr.g_params, allow_unused=True)
        finally:
            CS.MERGED_BWD, CS.critic_step = old, orig
            R.HEAD_FUSION = R.PREP_FUSION = R.TRUNK_SHARE = R.TAIL_SHARE = True
        assert bool(calls) == (form == 'scheduled')
        res[form] = (out, grads, [n for n, _ in tr.d_named], gout['cost'].detach(), ggrads)
    a = res['fused']
    for form in ('unfused', 'scheduled'):
        b = res[form]
        for k in ('cost', 'wgan', 'wgan_only', 'ct', 'gp', 'slopes', 'gp_grads', 'd_real', 'd_fake', 'real'):
            _cmp(b[0][k], a[0][k], 2e-6, '%s.%s' % (form, k), atol=1e-7)
        assert a[2] == b[2] and a[2][-1] == TABLE
        for n, x, y in zip(a[2], a[1], b[1]):
            assert (x is None) == (y is None), n
            if x is not None:
                _cmp(y, x, 5e-6, '%s grad %s' % (form, n), atol=1e-8)
        _cmp(b[3], a[3], 2e-6, form + ' g cost', atol=1e-7)
        for x, y in zip(a[4], b[4]):
            assert (x is None) == (y is None)
            if x is not None:
                _cmp(y, x, 5e-6, form + ' g grad', atol=1e-8)
    g_table = a[1][-1]
    assert float(g_table[[0, 3, 7]].abs().min(dim=1).values.min()) > 0 and torch.equal(g_table[[1, 2, 4, 5, 6, 8, 9]], torch.zeros(7, D))


# ----------------------------------------------------------------------------------------------------------------- 5: dev cost
def test_dev_cost_over_stacked_batches_uses_each_batch_own_labels(modules):
    """Evaluator.dev_cost over G stacked batches with different labels per batch = the mean of the per-batch d_losses costs on the same draws
    (tests/eval_helpers.close, the bound of the existing dev-cost comparisons); with in-kernel draws (the fused heads) a zero table gives the
    unprojected dev cost bit for bit."""
    from ctgan_amd.evaluate import Evaluator
    R, lib = modules
    B, dim = 4, 8
    _build(R, lib, dim, B, seed=13, PROJECTION=True, **COND)
    _shake_biases(lib)
    _set_table(lib)
    g = torch.Generator().manual_seed(7)
    batches = [(torch.randint(0, 256, (B, 3072), generator=g, dtype=torch.int32), lab)
               for lab in (torch.tensor([0, 1, 2, 3], dtype=torch.int32), torch.tensor([9, 9, 4, 0], dtype=torch.int32),
                           torch.tensor([5, 6, 7, 8], dtype=torch.int32))]
    rnds = [H.f32_rnd(osteps.make_rnd_resnet_d(B, dim, g), 'cpu') for _ in batches]
    tr = R.Trainer(seed=1)
    costs = []
    for (real, lab), rnd in zip(batches, rnds):
        tr.rng.begin_step()
        costs.append(tr.d_losses(real, lab, rnd)['cost'].item())
    want = sum(costs) / len(costs)
    assert max(costs) - min(costs) > 1e-3 * abs(want)
    for width in (3, 2, 1):
        got = Evaluator(tr, width=width).dev_cost(iter(batches), rnd=rnds)
        assert got['n_batches'] == 3
        H.close(got['dev_cost'], want, 'dev cost at width %d' % width)
    # the labels matter: the same pass with the batches' labels rotated is a different number
    rot = [(batches[i][0], batches[(i + 1) % 3][1]) for i in range(3)]
    assert abs(Evaluator(tr, width=3).dev_cost(iter(rot), rnd=rnds)['dev_cost'] - want) > 1e-4 * abs(want)
    vals = {}
    for proj in (True, False):
        _build(R, lib, dim, B, seed=13, PROJECTION=proj, **COND)
        _shake_biases(lib)
        if proj:
            _set_table(lib, 0.0)
        vals[proj] = Evaluator(R.Trainer(seed=1), width=2).dev_cost(iter(batches))['dev_cost']
    assert vals[True] == vals[False]


# ----------------------------------------------------------------------------------------------------------------- 6: checkpoint
def test_checkpoint_round_trip_and_resume_with_the_table(modules, tmp_path):
    from ctgan_amd import checkpoint
    R, lib = modules
    B, dim = 4, 8
    path = str(tmp_path / 'ck.pt')
    g = torch.Generator().manual_seed(4)
    feed = [(torch.randint(0, 256, (B, 3072), generator=g, dtype=torch.int32), torch.randint(0, 10, (B,), generator=g, dtype=torch.int32))
            for _ in range(3 * 5)]
    ends = {}
    for run in ('whole', 'resumed'):
        _build(R, lib, dim, B, PROJECTION=True, **COND)
        tr = R.Trainer(seed=2)
        it_feed = iter(feed)
        start = 0
        if run == 'resumed':
            start = checkpoint.load(path, tr)
            assert start == 2 and torch.equal(lib._params[TABLE].detach(), saved_table)
            it_feed = iter(feed[2 * 5:])
        init = lib._params[TABLE].detach().clone()
        for it in range(start, 3):
            tr.train_iteration(it, lambda: next(it_feed))
            if run == 'whole' and it == 1:
                checkpoint.save(path, tr, it + 1)
                saved_table = lib._params[TABLE].detach().clone()
                assert not torch.equal(saved_table, init)
        ends[run] = {'d': tr.d_opt.theta.clone(), 'g': tr.g_opt.theta.clone(), 'm': tr.d_opt.m.clone(), 'table': lib._params[TABLE].detach().clone()}
    for k in ends['whole']:
        assert torch.equal(ends['whole'][k], ends['resumed'][k]), k
    ck = torch.load(path, map_location='cpu', weights_only=False)
    assert TABLE in ck['params'] and torch.equal(ck['params'][TABLE], saved_table)
