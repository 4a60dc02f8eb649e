"""The CT critic step with the twice-differentiable attention block under graph replay (`-m gpu`; gan_cifar_resnet.Config.ATTENTION_D +
ATTENTION_SECOND_ORDER).  The kernels, the operator and the eager step are in tests/test_gpu_attention2.py.

The file is named to be collected after tests/test_gpu_kernels.py: a graph engine creates a capture stream, and the clock-probe test
there depends on which hardware queue the next stream created in the process is given (as tests/test_gpu_trainers_diffaug.py notes)."""
import numpy as np
import pytest
import torch

from tests.test_gpu_attention2 import BS, D_GATE, ON, _build

pytestmark = pytest.mark.gpu


def _run(graphs, iters, cfg_kw, **trainer_kw):
    import ctgan_amd.gan_cifar_resnet as R
    import ctgan_amd.tflib as lib
    from ctgan_amd.engine import GraphedTrainer
    nrng = np.random.default_rng(1234)
    batches = [(torch.from_numpy(nrng.integers(0, 256, (BS, 3072), dtype=np.int32)).cuda(),
                torch.from_numpy(nrng.integers(0, 10, (BS,), dtype=np.int32)).cuda()) for _ in range(8)]
    try:
        _build(R, lib, 'cuda', seed=0, **cfg_kw)
        tr = R.Trainer(seed=2024, **trainer_kw)
        eng = GraphedTrainer(tr, use_graphs=graphs)
        assert eng.graphed == graphs, eng.graph_error
        cur = [0]

        def nb():
            cur[0] += 1
            return batches[cur[0] % len(batches)]
        for it in range(iters):
            eng.train_iteration(it, nb)
        torch.cuda.synchronize()
        return tr.d_opt.theta.clone(), tr.g_opt.theta.clone(), lib._params[D_GATE].detach().clone()
    finally:
        lib.delete_all_params(); R.configure()


def test_graph_replay_equals_eager_ct_step_with_critic_attention():
    """two graph-replayed CT train_iterations and two eager ones: every weight bit-identical, and the critic's gate has moved (it is read on
    the device, in the forward and in both derivatives)"""
    g, e = _run(True, 2, ON), _run(False, 2, ON)
    assert torch.equal(g[0], e[0]) and torch.equal(g[1], e[1])
    assert torch.equal(g[2], e[2]) and float(g[2]) != 0.5 and torch.isfinite(g[2]).all()
