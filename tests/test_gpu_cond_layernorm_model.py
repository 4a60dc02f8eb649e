"""GPU twin of tests/test_cond_layernorm_model.py - the "vanilla" conditional ResNet critic (CONDITIONAL=True, ACGAN=False,
NORMALIZATION_D=True) on the fused label-conditioned Layernorm kernels: parameters, label dependence, forward and step parity against the
fp64 oracle (tolerances of test_gpu_resnet_step.py::test_layernorm_critic_d_step_on_gpu), hipGraph replay against eager, a checkpoint
round trip - and the paths that must not have changed (ACGAN critic with Layernorm: [C] parameters, the label-free kernels, the same bits)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import test_cond_layernorm_model as M  # noqa: E402


@pytest.fixture
def resnet():
    import ctgan_amd.gan_cifar_resnet as R
    import ctgan_amd.tflib as lib
    lib.delete_all_params(); lib.set_device(None)
    yield R, lib
    lib.delete_all_params(); R.configure()


def test_vanilla_conditional_critic_parameters_on_gpu(resnet):
    M.check_parameters(*resnet, None)


def test_critic_output_depends_on_labels_and_matches_oracle_on_gpu(resnet, monkeypatch):
    M.check_label_dependence_and_oracle(*resnet, None, monkeypatch)


def test_d_step_and_g_step_match_oracle_on_gpu(resnet, monkeypatch):
    import ctgan_amd.kernels as K
    calls = []
    orig = K.layernorm_cond_bwd2
    monkeypatch.setattr(K, 'layernorm_cond_bwd2', lambda *a, **k: (calls.append(1), orig(*a, **k))[1])
    M.check_steps(*resnet, None, monkeypatch)
    assert calls, 'the penalty did not reach the fused double-backward kernel'


def _batches(n=10, seed=1234):
    import numpy as np
    nrng = np.random.default_rng(seed)
    return [(torch.from_numpy(nrng.integers(0, 256, (M.B, 3072), dtype=np.int32)).cuda(),
             torch.from_numpy(nrng.integers(0, 10, (M.B,), dtype=np.int32)).cuda()) for _ in range(n)]


def test_graph_replay_equals_eager(resnet):
    """engine.GraphedTrainer on the autograd path of this configuration: two iterations replayed are the bits of two eager iterations."""
    R, lib = resnet
    from ctgan_amd.engine import GraphedTrainer
    batches = _batches()

    def run(graphs):
        M.build(R, lib, None, seed=0)
        M.randomise_tables(lib)
        tr = R.Trainer(seed=2024)
        eng = GraphedTrainer(tr, use_graphs=graphs)
        assert eng.graphed == graphs, eng.graph_error
        cur = [0]

        def nb():
            cur[0] = (cur[0] + 1) % len(batches)
            return batches[cur[0]]
        costs = [float(eng.train_iteration(it, nb)['cost'].item()) for it in range(2)]
        tables = {n: lib._params[n].detach().clone() for n in M.TABLES}
        return costs, tr.d_opt.theta.clone(), tr.g_opt.theta.clone(), tables
    g, e = run(True), run(False)
    assert g[0] == e[0]
    assert torch.equal(g[1], e[1]) and torch.equal(g[2], e[2])
    assert all(torch.equal(g[3][n], e[3][n]) for n in M.TABLES)


def test_checkpoint_round_trip_restores_the_tables(resnet, tmp_path):
    R, lib = resnet
    from ctgan_amd import checkpoint
    batches = _batches(4, seed=7)

    def run(n_iters, resume_from=None, save_at=None):
        M.build(R, lib, None, seed=4)
        if not resume_from:
            M.randomise_tables(lib)
        tr = R.Trainer(seed=9)
        start = checkpoint.load(resume_from, tr) if resume_from else 0
        k = [start * 5]

        def nxt():
            k[0] += 1
            return batches[k[0] % 4]
        saved = None
        for it in range(start, n_iters):
            tr.train_iteration(it, nxt)
            if save_at is not None and it + 1 == save_at:
                checkpoint.save(str(tmp_path / 'ck.pt'), tr, iteration=it + 1)
                saved = {n: lib._params[n].detach().clone() for n in M.TABLES}
        return (tr.d_opt.theta.clone(), tr.g_opt.theta.clone(), tr.d_opt.m.clone()), saved, {n: lib._params[n].detach().clone() for n in M.TABLES}
    a, saved, _ = run(2, save_at=1)
    M.build(R, lib, None, seed=4)
    tr = R.Trainer(seed=9)
    assert checkpoint.load(str(tmp_path / 'ck.pt'), tr) == 1
    for n in M.TABLES:          # restored (a fresh build holds ones / zeros), shape [10, C]
        assert torch.equal(lib._params[n].detach(), saved[n]) and tuple(saved[n].shape) == (10, M.DIM), n
    b, _, _ = run(2, resume_from=str(tmp_path / 'ck.pt'))
    for x, y in zip(a, b):
        assert torch.equal(x, y)


def test_acgan_layernorm_critic_is_unchanged(resnet, monkeypatch):
    """ACGAN=True, NORMALIZATION_D=True: the labels do not survive Normalize's filters - [C] parameters, no conditional entry point, and one
    critic step gives the bits of the label-free module (the parent commit's path: Layernorm(name, [1,2,3], inputs) -> F.layer_norm)."""
    R, lib = resnet
    import ctgan_amd.functional as F
    import ctgan_amd.kernels as K
    from ctgan_amd.tflib.ops import layernorm as ln
    called = []
    for name in ('layernorm_cond_fwd', 'layernorm_cond_bwd', 'layernorm_cond_bwd2', 'rows_gather', 'rows_sum_by_label'):
        monkeypatch.setattr(K, name, lambda *a, _n=name, **k: called.append(_n))
    g = torch.Generator().manual_seed(2)
    real = torch.randint(0, 256, (M.B, 3072), generator=g, dtype=torch.int32).cuda()
    labels = torch.tensor(M.LABELS, dtype=torch.int32).cuda()

    def run(parent):
        M.build(R, lib, None, ACGAN=True)
        for n in M.TABLES:
            assert tuple(lib._params[n].shape) == (M.DIM,), n
        assert 'Discriminator.ACGANOutput.W' in lib._params
        if parent:       # the operator as the parent commit had it: no labels argument at all
            def plain(name, norm_axes, inputs, labels=None, n_labels=None, relu=False):
                assert labels is None and n_labels is None
                scale, offset = lib.param(name + '.scale'), lib.param(name + '.offset')
                return F.layer_norm(inputs, scale, offset, 1e-5, relu=relu)
            monkeypatch.setattr(ln, 'Layernorm', plain)
        tr = R.Trainer(seed=1)
        out = tr.d_step(real, labels, None, iteration=0)
        return out['cost'].clone(), out['gp_grads'].clone(), tr.d_opt.theta.clone()
    a = run(False)
    b = run(True)
    assert not called, called
    for x, y in zip(a, b):
        assert torch.equal(x, y)
