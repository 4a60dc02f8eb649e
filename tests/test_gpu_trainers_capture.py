"""A failed graph capture leaves no trace (`-m gpu`): the engines' constructors fall back to eager launches when anything in
engine._capture_graphs raises, and the trainer must then be exactly what it was before the attempt.  The failure here is a plain
Python exception raised on the host in the first warm-up pass - after the passes before it have run at learning rate 0 and written the
Adam slots and the Philox counter, before any capture has begun.  Checked on the ResNet trainer (tr.g_losses raises: a fake-batch pass
and a critic pass have run) and on the semi-supervised MNIST trainer (tr.g_body raises: a classifier pass has run): not graphed, the
reason in graph_error, every graph handle and output None, optimizer slots / step counts / Philox counter as cloned before, and two
iterations through the fallen-back engine bit-identical to two through an engine built with use_graphs=False.

The file is named to be collected after tests/test_gpu_kernels.py: a graph engine creates a capture stream, and the clock-probe test
there depends on which hardware queue the next stream created in the process is given (as tests/test_gpu_trainers_diffaug.py notes)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _raise_injected(*a, **kw):
    raise RuntimeError('injected')


def _failed_engine(make_engine, tr, method, handles):
    """Build an engine while tr.<method> raises -> the engine, after the asserts on what the failed capture left behind."""
    opts = (tr.d_opt, tr.g_opt)
    slots = [b for o in opts for b in o.slots()] + [tr.rng.ctr]
    before = [b.clone() for b in slots]
    steps = [o.t for o in opts]
    setattr(tr, method, _raise_injected)
    try:
        eng = make_engine(tr)
    finally:
        delattr(tr, method)              # the instance attribute: the class's method is back
    assert eng.graphed is False
    assert eng.graph_error == 'RuntimeError: injected'
    for name in handles:
        assert getattr(eng, name) is None, name
    for i, (b, sn) in enumerate(zip(slots, before)):
        assert torch.equal(b, sn), i
    assert [o.t for o in opts] == steps
    return eng


def test_resnet_engine_after_a_failed_capture():
    import ctgan_amd.gan_cifar_resnet as R
    import ctgan_amd.tflib as lib
    from ctgan_amd.engine import GraphedTrainer
    B, dim = 8, 16
    nrng = np.random.default_rng(7)
    batches = [(torch.from_numpy(nrng.integers(0, 256, (B, 3072), dtype=np.int32)).cuda(),
                torch.from_numpy(nrng.integers(0, 10, (B,), dtype=np.int32)).cuda()) for _ in range(4)]

    def run(fail):
        lib.delete_all_params(); lib.set_device(None); lib.set_seed(4)
        R.configure(DIM_G=dim, DIM_D=dim, BATCH_SIZE=B)
        R.build_params()
        tr = R.Trainer(seed=9)
        if fail:
            eng = _failed_engine(GraphedTrainer, tr, 'g_losses',
                                 ('d_graph', 'g_graph', 'f_graph', 'it_graph', 'd_out', 'g_out', 'fake_all', 'it_out'))
            assert eng.it_graph_error is None
        else:
            eng = GraphedTrainer(tr, use_graphs=False)
        k = [0]

        def nxt():
            k[0] += 1
            return batches[k[0] % 4]
        for it in range(2):
            eng.train_iteration(it, nxt)
        return tr.d_opt.theta.clone(), tr.g_opt.theta.clone(), tr.d_opt.t, tr.g_opt.t
    try:
        a, b = run(True), run(False)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
        assert a[2:] == b[2:] == (10, 1)
    finally:
        lib.delete_all_params(); R.configure()


def test_ssl_engine_after_a_failed_capture():
    import ctgan_amd.ct_mnist as M
    import ctgan_amd.tflib as lib
    from ctgan_amd.engine import GraphedSSLTrainer
    from tests import ssl_oracle as O
    lib.delete_all_params()
    try:
        cfg = M.configure()                  # the sizes of test_gpu_ssl.py's graph test
        g = torch.Generator().manual_seed(4)
        B = cfg.BATCH_SIZE
        batches = [(torch.rand(B, cfg.IN_DIM, generator=g), torch.randint(0, 10, (B,), generator=g, dtype=torch.int32),
                    torch.rand(B, cfg.IN_DIM, generator=g), torch.rand(B, cfg.IN_DIM, generator=g)) for _ in range(2)]
        x0 = torch.rand(cfg.INIT_ROWS, cfg.IN_DIM, generator=g).cuda()
        P = O.make_params(cfg, seed=8, dtype=torch.float32)

        def run(fail):
            lib.delete_all_params()
            tr = M.SSLTrainer(seed=21)
            O.load_into_registry(P)
            tr.init_params(x0)
            if fail:
                eng = _failed_engine(GraphedSSLTrainer, tr, 'g_body', ('d_graph', 'g_graph', 'd_out', 'g_out'))
            else:
                eng = GraphedSSLTrainer(tr, use_graphs=False)
            for b in batches:
                eng.train_iteration(*b)
            return tr.d_opt.theta.clone(), tr.g_opt.theta.clone(), tr.d_opt.t, tr.g_opt.t
        a, b = run(True), run(False)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
        assert a[2:] == b[2:] == (2, 2)
    finally:
        M.configure(); lib.delete_all_params(); lib.delete_param_aliases()
