"""Graph replay of the hinge objective's trainers equals eager bit for bit (`-m gpu`): gan_cifar_resnet.Trainer(objective='hinge') with and
without spectral_norm through engine.GraphedTrainer, dcgan_step.DCGANTrainer(gan_cifar, objective='hinge') through GraphedDCGANTrainer - the
engines need no change for the objective: they call d_grads and filter `out` by key - and the launch count of one hinge critic step against one CT critic step.  The other step tests are in tests/test_gpu_hinge_step.py.

The file is named to be collected after tests/test_gpu_kernels.py (see tests/test_gpu_trainers_capture.py): a graph engine creates a capture
stream."""
import pytest
import torch

from tests import hinge_step_checks as S

pytestmark = pytest.mark.gpu


@pytest.fixture
def modules():
    import ctgan_amd.gan_cifar_resnet as R
    import ctgan_amd.tflib as lib
    lib.delete_all_params(); lib.set_device(None)
    yield R, lib
    lib.delete_all_params(); R.configure()


@pytest.mark.parametrize('spectral', [False, True])
def test_graph_replay_equals_eager_bit_for_bit(modules, spectral):
    """The protocol of tests/test_gpu_spectral_trainers.py::test_graph_replay_equals_eager_bit_for_bit, three train_iterations."""
    from ctgan_amd.engine import GraphedTrainer
    R, lib = modules
    B, dim = 8, 64                      # DIM 64: the hand-scheduled hinge step is what gets captured
    batches = [S.batch(B, 'cuda', seed=s) for s in (7, 8, 9, 10)]
    res = []
    for graphs in (False, True):
        S.build(R, lib, 'cuda', dim, B, seed=4)
        tr = R.Trainer(seed=9, objective='hinge', spectral_norm=spectral)
        eng = GraphedTrainer(tr, use_graphs=graphs)
        assert bool(eng.graphed) == graphs, getattr(eng, 'graph_error', None)
        nxt = S._feed(batches)
        vals = []
        for it in range(3):
            out = eng.train_iteration(it, nxt)          # (a replay returns its static output buffers: copy at once)
            assert 'ct' not in out and 'gp' not in out and 'acc_real' in out
            vals += [out['cost'].clone(), out['wgan'].clone(), out['acc_real'].clone()]
        res.append([tr.d_opt.theta.clone(), tr.g_opt.theta.clone()] + vals)
        if tr.spectral is not None:
            tr.detach_spectral()
    for i, (x, y) in enumerate(zip(*res)):
        assert torch.equal(x, y), i


def test_graph_replay_equals_eager_bit_for_bit_gan_cifar():
    import ctgan_amd.gan_cifar as M
    import ctgan_amd.tflib as lib
    from ctgan_amd.dcgan_step import DCGANTrainer, build_params
    from ctgan_amd.engine import GraphedDCGANTrainer
    B, dim = 8, 32
    g = torch.Generator().manual_seed(3)
    reals = [torch.randint(0, 256, (B, 3072), generator=g, dtype=torch.int32).cuda() for _ in range(4)]
    res = []
    try:
        for graphs in (False, True):
            lib.delete_all_params(); lib.set_device(None); lib.set_seed(4)
            M.configure(DIM=dim, BATCH_SIZE=B)
            build_params(M)
            tr = DCGANTrainer(M, seed=9, objective='hinge')
            eng = GraphedDCGANTrainer(tr, tuple(reals[0].shape), reals[0].dtype, use_graphs=graphs)
            assert bool(eng.graphed) == graphs, getattr(eng, 'graph_error', None)
            nxt = S._feed(reals)
            costs = [eng.train_iteration(it, nxt)['cost'].clone() for it in range(3)]
            res.append([tr.d_opt.theta.clone(), tr.g_opt.theta.clone()] + costs)
    finally:
        M.configure(); lib.delete_all_params()
    for i, (x, y) in enumerate(zip(*res)):
        assert torch.equal(x, y), i


def _count_kernels(fn):
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    names = [e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]
    return len([n for n in names if 'memcpy' not in n.lower() and 'memset' not in n.lower()])


def test_a_hinge_critic_step_launches_fewer_kernels_than_a_ct_critic_step(modules):
    """A condition, not a measurement: the hinge step's launches are a subset of the CT step's work.  Counted on the device's kernel
    trace (the count tests/test_gpu_spectral_trainers.py takes), one eager critic step each at the same configuration, after a warm-up step."""
    R, lib = modules
    B, dim = 8, 64
    counts = {}
    for obj in (None, 'hinge'):
        S.build(R, lib, 'cuda', dim, B, seed=4)
        tr = R.Trainer(seed=9, objective=obj)
        real, labels = S.batch(B, 'cuda')
        tr.d_step(real, labels, iteration=0)
        counts[obj] = _count_kernels(lambda: tr.d_step(real, labels, iteration=1))
    print('kernels of one eager critic step: CT %d, hinge %d' % (counts[None], counts['hinge']))
    assert 0 < counts['hinge'] < counts[None]
