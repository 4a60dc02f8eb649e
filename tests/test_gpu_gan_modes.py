"""The scripts' other MODE branches on the MI355X: the TF-RMSProp (+ clip) kernels and the BCE / least-squares loss heads against fp64,
critic and generator steps of each new (module, mode) against the oracle (tests/gan_modes_oracle.py), hipGraph replay against the eager
trainer, and a bit-exact resume with the RMSProp slots."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import gan_modes_oracle as O  # noqa: E402
from tests.test_gan_modes_host import mode_setup, build_params, run_mode_steps  # noqa: E402


def _rmsprop_fp64(th, g, ms, lr, gscale, clip):
    g = g.double() * gscale
    ok = torch.isfinite(g)
    g0 = torch.where(ok, g, torch.zeros_like(g))
    th2, ms2 = O.rmsprop_step(th, g0, ms, lr)
    th2, ms2 = torch.where(ok, th2, th), torch.where(ok, ms2, ms)
    return (th2.clamp(-clip, clip) if clip else th2), ms2, int((~ok).sum())


@pytest.mark.parametrize('clip', [0.0, 0.05])
def test_rmsprop_kernels_against_fp64_plain_equals_packed(clip):
    import ctgan_amd.kernels as K
    gen = torch.Generator().manual_seed(4)
    sizes = [7, 64, 1, 130, 4096, 3]                 # lengths not a multiple of 4 and 16-B misaligned segments
    offs = [sum(sizes[:i]) for i in range(len(sizes))]
    n = sum(sizes)
    th0 = torch.randn(n, generator=gen) * 0.04
    lr, gscale = 5e-5, 0.5
    runs = {}
    for form in ('plain', 'packed'):
        th, ms = th0.clone().cuda(), torch.ones(n, device='cuda')
        state = torch.tensor([lr, 1.0, 1.0, 0.0], device='cuda')
        flat = torch.zeros(n, device='cuda')
        g2 = torch.Generator().manual_seed(9)
        ref_th, ref_ms, ref_skip = th0.double(), torch.ones(n, dtype=torch.float64), 0
        for step in range(3):
            grads = [None if i == 2 else torch.randn(c, generator=g2) * 10 ** (i - 3) for i, c in enumerate(sizes)]
            if step == 1:
                grads[3][5] = float('nan'); grads[4][7] = float('inf')
            dev = [None if t is None else t.cuda() for t in grads]
            if form == 'plain':
                K.pack(dev, offs, sizes, flat)
                K.rmsprop_step(th, flat, ms, state, 0.9, 1e-10, clip, gscale)
            else:
                K.rmsprop_step_packed(dev, offs, sizes, flat, th, ms, state, 0.9, 1e-10, clip, gscale)
            gfull = torch.zeros(n)
            for t, o, c in zip(grads, offs, sizes):
                if t is not None:
                    gfull[o:o + c] = t
            ref_th, ref_ms, k = _rmsprop_fp64(ref_th, gfull, ref_ms, lr, gscale, clip)
            ref_skip += k
        torch.cuda.synchronize()
        assert int(state[3].item()) == ref_skip == 2
        assert torch.isfinite(th).all() and torch.isfinite(ms).all()
        err = (th.cpu().double() - ref_th).abs().max().item()
        assert err <= 2e-7 * ref_th.abs().max().item(), err
        assert ((ms.cpu().double() - ref_ms).abs() / ref_ms).max().item() <= 1e-6
        if clip:
            c32 = torch.tensor(clip, dtype=torch.float32).item()       # (the bound as the kernel holds it)
            assert th.abs().max().item() <= c32 and (th.abs() == c32).any()
        runs[form] = (th.clone(), ms.clone(), flat.clone())
    for a, b in zip(runs['plain'], runs['packed']):
        assert torch.equal(a, b)


def test_rmsprop_first_step_is_lr_g_over_sqrt_of_ones_slot():
    import ctgan_amd.kernels as K
    g = torch.tensor([1e-3, -0.5, 2.0, 0.0], device='cuda')
    th = torch.zeros(4, device='cuda')
    ms = torch.ones(4, device='cuda')
    state = torch.tensor([5e-5, 1.0, 1.0, 0.0], device='cuda')
    K.rmsprop_step(th, g, ms, state, 0.9, 1e-10)
    want = -5e-5 * g.cpu().double() / torch.sqrt(0.9 + 0.1 * g.cpu().double() ** 2 + 1e-10)
    assert torch.allclose(th.cpu().double(), want, rtol=1e-6, atol=0)


@pytest.mark.parametrize('loss,net', [('bce', 'd'), ('bce', 'g'), ('ls', 'd'), ('ls', 'g')])
def test_loss_heads_against_fp64(loss, net):
    import ctgan_amd.kernels as K
    B = 37
    gen = torch.Generator().manual_seed(1)
    n = 2 * B if net == 'd' else B
    d = torch.randn(n, generator=gen, dtype=torch.float64) * 3
    d[0], d[1], d[-1], d[-2] = 80.0, -80.0, 80.0, -80.0
    x = d.clone().requires_grad_(True)
    ref = O.d_cost(loss, x[:B], x[B:]) if net == 'd' else O.g_cost(loss, x)
    (gref,) = torch.autograd.grad(ref, x)
    kind = K.GAN_LOSS_KINDS[(loss, net)]
    dv = d.float().cuda()
    out = K.gan_loss_fwd(dv, B, kind)
    gout = torch.tensor(0.75, device='cuda')
    gd = K.gan_loss_bwd(dv, gout, B, kind)
    torch.cuda.synchronize()
    assert torch.isfinite(out).item() and torch.isfinite(gd).all()
    assert abs(out.item() - ref.item()) <= 1e-5 * max(1.0, abs(ref.item())), (out.item(), ref.item())
    assert torch.allclose(gd.cpu().double(), 0.75 * gref, rtol=1e-5, atol=1e-9)
    if loss == 'bce':           # gradient = (sigmoid(x) - z) / n: saturates at the +-80 logits, never NaN
        z = torch.ones(n, dtype=torch.float64)
        if net == 'd':
            z[B:] = 0
        w = 2 * B if net == 'd' else B
        assert torch.allclose(gd.cpu().double(), 0.75 * (torch.sigmoid(d) - z) / w, rtol=1e-5, atol=1e-9)


@pytest.mark.parametrize('which,mode,dim,B', [('mnist', 'wgan', 16, 6), ('mnist', 'wgan', 64, 50), ('mnist', 'dcgan', 16, 6),
                                              ('mnist', 'dcgan', 64, 50), ('64x64', 'wgan', 16, 6), ('64x64', 'dcgan', 16, 6),
                                              ('64x64', 'lsgan', 16, 6)])
def test_mode_steps_against_oracle(which, mode, dim, B):
    """Costs to test_gpu_dcgan_step's tolerances, per-parameter gradients in L2 against max(fixed, 3 x the fp32 twin's error), every
    parameter after the update against the oracle's optimizer (+ clip) on its own gradients; MODE 'wgan' leaves the MNIST critic's moving
    variance at the clip bound 0.01."""
    import ctgan_amd.tflib as lib
    lib.delete_all_params(); lib.set_device(None)
    # fixed gradient bounds of the module's existing GPU step tests: test_gpu_dcgan_step (MNIST) and test_gan_64x64 (100 / 400 x 5e-5)
    d_tol, g_tol = (3e-3, 5e-3) if which == 'mnist' else (5e-3, 2e-2)
    assert run_mode_steps(lib, which, mode, dim, B, 'cuda', cost_tol=2e-4 if dim < 64 else 1e-3, grad_tol=d_tol, g_grad_tol=g_tol, twin=True) > 0


@pytest.mark.parametrize('which,mode', [('mnist', 'wgan'), ('mnist', 'dcgan'), ('64x64', 'wgan'), ('64x64', 'dcgan'), ('64x64', 'lsgan')])
def test_graphed_mode_trainer_equals_eager(which, mode):
    """engine.GraphedDCGANTrainer against the eager DCGANTrainer for the new objectives, as test_graphed_unconditional_trainer_equals_eager:
    same costs, bit-identical weights, the Philox step count of disc_iters critic steps + the batched fake draw per iteration."""
    import numpy as np
    import ctgan_amd.tflib as lib
    from ctgan_amd.dcgan_step import DCGANTrainer
    from ctgan_amd.engine import GraphedDCGANTrainer
    dim, B = (32, 8) if which == 'mnist' else (32, 4)
    nrng = np.random.default_rng(5)

    def run(graphs):
        lib.delete_all_params(); lib.set_device(None); lib.set_seed(3)
        M, _, _, _, _ = mode_setup(which, mode, dim, B, torch.Generator().manual_seed(0))
        build_params(M, 'cuda')
        tr = DCGANTrainer(M, seed=11)
        eng = GraphedDCGANTrainer(tr, (B, M.cfg.OUTPUT_DIM), batches[0].dtype, use_graphs=graphs)
        assert eng.graphed == graphs, eng.graph_error
        k = [0]

        def nb():
            k[0] += 1
            return batches[k[0] % len(batches)]
        costs = [float(eng.train_iteration(it, nb)['cost'].item()) for it in range(3)]
        return costs, tr.d_opt.theta.clone(), tr.g_opt.theta.clone(), int(tr.rng.ctr.item()), tr.disc_iters, \
            {n: p.detach().clone() for n, p in lib._params.items() if n in lib._non_trainable}
    try:
        if which == 'mnist':
            batches = [torch.from_numpy(nrng.random((B, 784), dtype=np.float32)).cuda() for _ in range(4)]
        else:
            batches = [torch.from_numpy(nrng.integers(0, 256, (B, 64 * 64 * 3), dtype=np.int32)).cuda() for _ in range(4)]
        g = run(True)
        e = run(False)
        assert g[4] == e[4] == (5 if mode == 'wgan' else 1)
        assert g[3] == e[3] == 3 * (g[4] + 1) + 2
        for a, b in zip(g[0], e[0]):
            assert abs(a) < 1e4 and abs(a - b) <= 1e-5 * max(1.0, abs(b)), (a, b)
        assert torch.equal(g[1], e[1]) and torch.equal(g[2], e[2])
        for n in g[5]:
            assert torch.equal(g[5][n], e[5][n]), n
        if mode == 'wgan':
            assert g[1].abs().max().item() <= 0.01
            assert all(t.abs().max().item() <= 0.01 for n, t in g[5].items() if n.startswith('Discriminator'))
    finally:
        lib.delete_all_params()
        import ctgan_amd.gan_64x64 as G64
        import ctgan_amd.gan_mnist as M
        M.configure(); G64.configure()


def test_mnist_wgan_bit_exact_resume(tmp_path):
    import ctgan_amd.gan_mnist as M
    import ctgan_amd.tflib as lib
    from ctgan_amd import checkpoint
    from ctgan_amd.dcgan_step import DCGANTrainer
    g = torch.Generator().manual_seed(0)
    batches = [torch.rand(8, 784, generator=g).cuda() for _ in range(4)]

    def run(n_iters, resume_from=None, save_at=None):
        lib.delete_all_params(); lib.set_device(None); lib.set_seed(4)
        M.configure(MODE='wgan', DIM=16, BATCH_SIZE=8)
        build_params(M, 'cuda')
        tr = DCGANTrainer(M, seed=9)
        start = checkpoint.load(resume_from, tr) if resume_from else 0
        k = [start * tr.disc_iters]

        def nxt():
            k[0] += 1
            return batches[k[0] % 4]
        for it in range(start, n_iters):
            tr.train_iteration(it, nxt)
            if save_at is not None and it + 1 == save_at:
                checkpoint.save(str(tmp_path / 'ck.pt'), tr, iteration=it + 1)
        return tr.d_opt.theta.clone(), tr.g_opt.theta.clone(), tr.d_opt.ms.clone(), tr.g_opt.ms.clone(), \
            lib._params['Discriminator.BN3.moving_variance'].clone()
    try:
        a = run(3, save_at=2)
        b = run(3, resume_from=str(tmp_path / 'ck.pt'))
        for x, y in zip(a, b):
            assert torch.equal(x, y)
        assert not torch.equal(a[2], torch.ones_like(a[2]))
    finally:
        lib.delete_all_params(); M.configure()
