"""The trainers' differentiable augmentation (`augment=`) under graph replay on the MI355X (`-m gpu`): gan_mnist at the loop
tests' small width and the ResNet trainer, 3 iterations with augment='color,translation,cutout' graph-replayed against eager - weights
bit-identical, no graph error, the whole-iteration graph wherever the trainer has one without the augmentation - and a run with
augment=None beside one without the keyword.  The kernel and the one-step equivalence are in tests/test_gpu_diffaug.py.

The file is named to be collected after tests/test_gpu_kernels.py: a graph engine creates a capture stream, and the clock-probe test
there depends on which hardware queue the next stream created in the process is given (as tests/test_gpu_score_cifar_frechet.py notes)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests.test_gan_modes_host import build_params, mode_setup  # noqa: E402

POLICY = 'color,translation,cutout'


def _mnist_run(graphs, kw, iters, dim=32, B=8):
    import ctgan_amd.gan_mnist as M
    import ctgan_amd.tflib as lib
    from ctgan_amd.dcgan_step import DCGANTrainer
    from ctgan_amd.engine import GraphedDCGANTrainer
    nrng = np.random.default_rng(5)
    batches = [torch.from_numpy(nrng.random((B, 784), dtype=np.float32)).cuda() for _ in range(4)]
    lib.delete_all_params(); lib.set_device(None); lib.set_seed(3)
    mode_setup('mnist', 'wgan-CT', dim, B, torch.Generator().manual_seed(0))
    try:
        build_params(M, 'cuda')
        tr = DCGANTrainer(M, seed=11, **kw)
        eng = GraphedDCGANTrainer(tr, (B, M.cfg.OUTPUT_DIM), batches[0].dtype, use_graphs=graphs)
        assert eng.graphed == graphs and (eng.graph_error is None or not graphs), eng.graph_error
        k = [0]

        def nb():
            k[0] += 1
            return batches[k[0] % len(batches)]
        for it in range(iters):
            out = eng.train_iteration(it, nb)
        assert torch.isfinite(out['cost']).item()
        return tr.d_opt.theta.clone(), tr.g_opt.theta.clone(), eng.it_graph is not None
    finally:
        lib.delete_all_params(); M.configure()


def test_mnist_trainer_graph_replay_equals_eager_with_augmentation_on():
    g, e = _mnist_run(True, dict(augment=POLICY), 3), _mnist_run(False, dict(augment=POLICY), 3)
    assert torch.equal(g[0], e[0]) and torch.equal(g[1], e[1])
    plain = _mnist_run(True, {}, 3)
    assert g[2] == plain[2], 'the whole-iteration graph exists with augmentation on wherever it does without'
    assert not torch.equal(plain[0], g[0]), 'the augmentation is live'


def test_mnist_trainer_with_augment_none_is_the_trainer_without_the_keyword():
    off, plain = _mnist_run(True, dict(augment=None), 2), _mnist_run(True, {}, 2)
    assert torch.equal(off[0], plain[0]) and torch.equal(off[1], plain[1])


def _resnet_run(graphs, kw, iters, dim=32, B=8):
    import ctgan_amd.gan_cifar_resnet as R
    import ctgan_amd.tflib as lib
    from ctgan_amd.engine import GraphedTrainer
    nrng = np.random.default_rng(1234)
    batches = [(torch.from_numpy(nrng.integers(0, 256, (B, 3072), dtype=np.int32)).cuda(),
                torch.from_numpy(nrng.integers(0, 10, (B,), dtype=np.int32)).cuda()) for _ in range(8)]
    lib.delete_all_params(); lib.set_device(None); lib.set_seed(0)
    R.configure(DIM_G=dim, DIM_D=dim, BATCH_SIZE=B)
    try:
        R.build_params()
        tr = R.Trainer(seed=2024, **kw)
        eng = GraphedTrainer(tr, use_graphs=graphs)
        assert eng.graphed == graphs and (eng.graph_error is None or not graphs), eng.graph_error
        if graphs:
            assert eng.it_graph is not None, eng.it_graph_error          # (tests/test_gpu_graph_loop.py asserts it without augmentation)
        cur = [0]

        def nb():
            cur[0] += 1
            return batches[cur[0] % len(batches)]
        for it in range(iters):
            out = eng.train_iteration(it, nb)
        assert torch.isfinite(out['cost']).item()
        return tr.d_opt.theta.clone(), tr.g_opt.theta.clone()
    finally:
        lib.delete_all_params(); R.configure()


def test_resnet_trainer_graph_replay_equals_eager_with_augmentation_on():
    g, e = _resnet_run(True, dict(augment=POLICY), 3), _resnet_run(False, dict(augment=POLICY), 3)
    assert torch.equal(g[0], e[0]) and torch.equal(g[1], e[1])


def test_resnet_trainer_with_augment_none_is_the_trainer_without_the_keyword():
    off, plain = _resnet_run(True, dict(augment=None), 2), _resnet_run(True, {}, 2)
    assert torch.equal(off[0], plain[0]) and torch.equal(off[1], plain[1])
