"""Helpers of the evaluation tests (tests/test_eval_host.py, tests/test_gpu_eval.py): the CPU stand-in of kernels.pixels_u8, the fp64
restatement of slope_real, and the cases - module, trainer, dev batches, injected draws and the fp64 oracle's per-batch critic cost - that
the host and the device tests share.  Tests only."""
import torch

from oracle import nets as onets, steps as osteps
from tests import gan_modes_oracle as O
from tests.test_gan_modes_host import build_params, mode_setup, oracle_from_product

COST_RTOL, COST_ATOL = 2e-4, 1e-6        # the project's bound for `cost` against the oracle (tests/test_gpu_resnet_step.py:117)


def pixels_u8_cpu(x, channels, scale):
    """kernels.pixels_u8 on the host: the torch expression it replaces, NCHW -> NHWC, uint8; a non-finite input gives 0."""
    n, hw = x.shape[0], x.shape[1] // channels
    px = ((x + 1.) * scale)
    px = torch.where(torch.isfinite(x), px, torch.zeros_like(px)).clamp(0, 256).to(torch.int32).clamp(0, 255)
    return px.reshape(n, channels, hw).permute(0, 2, 1).contiguous().to(torch.uint8)


def pixels_reference(x, channels, scale):
    """((x + 1.) * scale).to(int32).clamp(0, 255), permuted to NHWC - for finite x, evaluated where x lives."""
    n, hw = x.shape[0], x.shape[1] // channels
    return ((x + 1.) * scale).to(torch.int32).clamp(0, 255).reshape(n, channels, hw).permute(0, 2, 1)


def close(a, b, what=''):
    assert abs(a - b) <= COST_RTOL * abs(b) + COST_ATOL, '%s: %.9g vs %.9g (err %.3e)' % (what, a, b, abs(a - b))


def slope_real_ref(reg, D, real_o, u_slope):
    """max_b ||dD(real_b)/dreal_b||_2 in fp64 (TF/CT_gan_cifar.py:145,149,227)."""
    x = real_o.detach().clone().requires_grad_(True)
    d = D(reg, x, u_slope)[0]
    (g,) = torch.autograd.grad(d.sum(), x)
    return torch.sqrt((g ** 2).sum(dim=1)).max().item()


def _f32(o, dev):
    if isinstance(o, list):
        return [_f32(t, dev) for t in o]
    return o.float().to(dev)


def f32_rnd(rnd, dev):
    return {k: _f32(v, dev) for k, v in rnd.items()}


CASES = ('resnet', 'cifar', 'mnist', '64x64', 'mnist-wgan', 'mnist-dcgan', '64x64-lsgan')


class Case:
    """One configured module with its parameters built on `dev`.  close() restores the module's configuration and empties the registry."""

    def __init__(self, lib, name, dim, B, dev, seed=7):
        self.lib, self.name, self.dim, self.B, self.dev = lib, name, dim, B, dev
        self.resnet = name == 'resnet'
        self.g = torch.Generator().manual_seed(seed)
        lib.set_seed(13)
        if self.resnet:
            import ctgan_amd.gan_cifar_resnet as R
            self.M = R
            R.configure(DIM_G=dim, DIM_D=dim, BATCH_SIZE=B)
            R.build_params(dev)
            self.cfg = onets.ResnetCfg(DIM_G=dim, DIM_D=dim)
            return
        which, _, mode = name.partition('-')
        if mode:
            self.M, self.G, self.D, _, _ = mode_setup(which, mode, dim, B, self.g)
        elif which == 'cifar':
            import ctgan_amd.gan_cifar as M
            M.configure(DIM=dim, BATCH_SIZE=B)
            self.M = M
            self.G = lambda reg, n, z: onets.cifar_generator(reg, n, z, DIM=dim)          # noqa: E731
            self.D = lambda reg, x, u: onets.cifar_discriminator(reg, x, u, DIM=dim)      # noqa: E731
        elif which == 'mnist':
            import ctgan_amd.gan_mnist as M
            M.configure(DIM=dim, BATCH_SIZE=B)
            self.M = M
            self.G = lambda reg, n, z: onets.mnist_generator(reg, n, z, DIM=dim)          # noqa: E731
            self.D = lambda reg, x, u: onets.mnist_discriminator(reg, x, u, DIM=dim)      # noqa: E731
        else:
            import ctgan_amd.gan_64x64 as M
            M.configure(DIM=dim, BATCH_SIZE=B)
            self.M = M
            self.G = lambda reg, n, z: onets.good_generator(reg, n, z, dim=dim)                      # noqa: E731
            self.D = lambda reg, x, u: onets.good_discriminator(reg, x, 0.8, 0.5, 0.5, u, dim=dim)   # noqa: E731
        build_params(self.M, dev)

    def close(self):
        self.M.configure()
        self.lib.delete_all_params()

    def trainer(self, seed=1):
        if self.resnet:
            return self.M.Trainer(seed=seed)
        from ctgan_amd.dcgan_step import DCGANTrainer
        return DCGANTrainer(self.M, seed=seed)

    def batch(self):
        """One dev batch as the feeds hand it over (host tensors) and the oracle's form of it."""
        B, g = self.B, self.g
        if self.resnet:
            real = torch.randint(0, 256, (B, 3072), generator=g, dtype=torch.int32)
            labels = torch.randint(0, 10, (B,), generator=g, dtype=torch.int32)
            return (real, labels), (real, labels)
        if self.M.__name__.endswith('gan_mnist'):
            real = torch.rand(B, 784, generator=g)
            return real, real.double()
        real = torch.randint(0, 256, (B, self.M.cfg.OUTPUT_DIM), generator=g, dtype=torch.int32)
        return real, 2 * ((real.double() / 255.) - .5)

    def draws(self, dtype=torch.float64):
        if self.resnet:
            return osteps.make_rnd_resnet_d(self.B, self.dim, self.g, dtype=dtype)
        rnd = osteps.make_rnd_dcgan_d(self.B, self.M.feat_shapes(), self.g, dtype=dtype)
        rnd['u_slope'] = [torch.rand(self.B, *s, generator=self.g, dtype=torch.float32).to(dtype) for s in self.M.feat_shapes()]
        return rnd

    def on_dev(self, batch):
        if isinstance(batch, tuple):
            return tuple(t.to(self.dev) for t in batch)
        return batch.to(self.dev)

    def oracle_costs(self, tr, batches_o, rnds):
        """The fp64 oracle's disc_cost of every dev batch, from the product's current weights."""
        reg = oracle_from_product(self.lib)
        costs = []
        for bo, rnd in zip(batches_o, rnds):
            if self.resnet:
                c = osteps.resnet_d_losses(reg, self.cfg, bo[0], bo[1], rnd, B=self.B, create_graph=False)['cost']
            elif tr.mode.loss == 'ct':
                c = osteps.dcgan_d_losses(reg, self.G, self.D, bo, rnd)['cost']
            else:
                c = O.d_losses(reg, self.G, self.D, bo, rnd, tr.mode.loss)['cost']
            costs.append(c.item())
        return costs, reg


def snapshot(lib, tr):
    """Everything an evaluation must leave alone."""
    snap = {'param ' + n: p.detach().clone() for n, p in lib._params.items()}
    for tag, opt in (('d_opt', tr.d_opt), ('g_opt', tr.g_opt)):
        for i, s in enumerate(opt.slots()):
            snap['%s slot %d' % (tag, i)] = s.detach().clone()
        snap[tag + ' theta'] = opt.theta.detach().clone()
        snap[tag + ' t'] = torch.tensor(opt.t)
    snap['rng.ctr'] = tr.rng.ctr.clone()
    snap['rng site'] = torch.tensor(tr.rng._site)
    return snap


def assert_same(a, b):
    assert a.keys() == b.keys()
    for k in a:
        assert torch.equal(a[k], b[k]), k
