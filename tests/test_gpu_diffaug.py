"""Differentiable augmentation on the MI355X (`-m gpu`): csrc/diffaug.hip through kernels.diffaug against tests/diffaug_oracle.py, the
autograd pair of functional.py, and the equivalence that defines the trainers' `augment` (one critic step).  The trainers under graph
replay are in tests/test_gpu_trainers_diffaug.py: a graph engine creates a capture stream, and the clock-probe test of
tests/test_gpu_kernels.py depends on which hardware queue the next stream created in the process is given - files that capture graphs
and are new to the suite are named to be collected after it (as tests/test_gpu_score_cifar_frechet.py is).

Tolerance of the colour arithmetic (masks with COLOR), derived from the reduction shape documented in csrc/diffaug.hip - not tuned:
  * the image mean: per lane at most ceil(n / 256) + 3 serial additions, an 8-level LDS tree, one division: DEPTH(n) = ceil(n / 256) + 12
    roundings, and one more for `+ b`;
  * per element, with no operation contracted: x + b (1), the channel sum and its division (C), 1 - s, s x1, (1 - s) mean_c and their
    sum (4), 1 - q, q x2, (1 - q) m and the final sum (4), the `+ b` of m (1): C + 10 roundings;
  * every rounding is at most 2^-24 relative to an intermediate bounded by the largest coefficient product |q s| <= 1.5 * 2 = 3 times
    the magnitude max(1, max|x| + .5) of the brightened input (|b| <= .5), taken per image;
  bound(image) = (C + 10 + DEPTH(n)) * 2^-24 * 3 * max(1, max|x| + .5).
Masks without COLOR move or zero values and compute nothing: torch.equal against the oracle."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import diffaug_oracle as O  # noqa: E402
from tests.test_gan_modes_host import build_params, mode_setup  # noqa: E402

SEED = 1                                     # chosen on the CPU: test_draws_cover_every_branch holds at n = 65, both counters
SID = (1 << 16) | 0xFF00                     # rank 1, the reserved stream AUG_REAL
CTRS = (0, (1 << 32) + 5)
SHAPES = [(1, 1, 4, 4), (3, 3, 8, 12), (5, 1, 28, 28), (65, 3, 32, 32), (2, 3, 128, 128),
          (2, 3, 7, 9)]          # w % 4 != 0: the scalar path
CASES = [(s, m) for s in SHAPES for m in (7, 1, 2, 4)] + [((65, 3, 32, 32), m) for m in (0, 3, 5, 6)]
POLICY = 'color,translation,cutout'


@pytest.fixture
def K():
    import ctgan_amd.kernels as K
    return K


def _ctr(v):
    return torch.tensor([v], dtype=torch.int64, device='cuda')


def _bound(x, shape):
    """per image [n, 1]: the docstring's bound"""
    n, c, h, w = shape
    depth = math.ceil(c * h * w / 256) + 12
    mag = torch.clamp(x.double().abs().reshape(n, -1).max(1).values + .5, min=1.0)
    return ((c + 10 + depth) * 2.0 ** -24 * 3.0 * mag).reshape(n, 1)


def _input(shape, seed):
    n, c, h, w = shape
    x = torch.randn(n, c * h * w, generator=torch.Generator().manual_seed(seed))
    x[0] = 0.75                               # an all-constant image
    if n > 1:
        x[1, (c * h * w) // 2] = 1e4         # one huge pixel
    return x


def test_draws_cover_every_branch():
    """From the numpy generator alone, before anything runs on the device: at (SEED, n = 65) on 32 x 32 every shift in [-4, 4] occurs in
    both directions and a cut rectangle is clipped at each of the four borders - at both counters."""
    sh, sw, kh, kw, nh, nw = O.geometry(32, 32)
    assert (sh, sw, kh, kw, nh, nw) == (4, 4, 16, 16, 33, 33)
    for step in CTRS:
        p = O.params(SEED, SID, step, 65, 32, 32, 7)
        u = O.draws(SEED, SID, step, 65)
        oy = np.minimum((np.float32(nh) * u[:, 5]).astype(np.int64), nh - 1)
        ox = np.minimum((np.float32(nw) * u[:, 6]).astype(np.int64), nw - 1)
        assert set(p['ty']) == set(range(-4, 5)) and set(p['tx']) == set(range(-4, 5))
        assert (oy - kh // 2 < 0).any() and (oy - kh // 2 + kh > 32).any() and (ox - kw // 2 < 0).any() and (ox - kw // 2 + kw > 32).any()
        assert (p['tx'] % 4 != 0).any() and (p['tx'] % 4 == 0).any()          # aligned and unaligned source quads


@pytest.mark.parametrize('shape,mask', CASES, ids=lambda v: 'x'.join(map(str, v)) if isinstance(v, tuple) else 'm%d' % v)
def test_forward_adjoint_and_params_against_the_oracle(K, shape, mask):
    n, c, h, w = shape
    x = _input(shape, 3)
    g = _input(shape, 4)
    for step in CTRS:
        p = O.params(SEED, SID, step, n, h, w, mask)
        ctr = _ctr(step)
        params = torch.full((n, 8), float('nan'), device='cuda')
        y = K.diffaug(x.cuda(), (c, h, w), mask, (SEED, SID, ctr), params=params)
        assert np.array_equal(params.cpu().numpy(), O.params_table(p, mask)), (shape, mask, step)
        if step == 0 and mask:
            continue                           # the draws at counter 0 are checked; the arithmetic runs at the 64-bit counter
        gx = K.diffaug(g.cuda(), (c, h, w), mask, (SEED, SID, ctr), adjoint=True)
        lin = K.diffaug(x.cuda(), (c, h, w), mask | K.DIFFAUG_NO_BRIGHTNESS, (SEED, SID, ctr))
        ry, rgx, rlin = O.forward(x, (c, h, w), p), O.adjoint(g, (c, h, w), p), O.forward(x, (c, h, w), p, brightness=False)
        if not mask & 1:
            assert torch.equal(y.cpu().double(), ry) and torch.equal(gx.cpu().double(), rgx) and torch.equal(lin.cpu(), y.cpu())
            if mask == 0:
                assert torch.equal(y.cpu(), x)
            continue
        for got, ref, src, what in ((y, ry, x, 'forward'), (gx, rgx, g, 'adjoint'), (lin, rlin, x, 'linear forward')):
            err = (got.cpu().double() - ref).abs()
            bound = _bound(src, shape)
            print('%s %s mask %d: max err / bound = %.3g' % (what, shape, mask, (err / bound).max().item()))
            assert (err <= bound).all(), (what, shape, mask, (err / bound).max().item())
        # exact zeros where the forward writes none of the input: under the cut and where the shift left the image
        assert (y.cpu()[ry == 0] == 0).all()


def test_integer_input_equals_real_prep_then_diffaug(K):
    for shape in SHAPES:
        n, c, h, w = shape
        xi = torch.randint(0, 256, (n, c * h * w), dtype=torch.int32, generator=torch.Generator().manual_seed(7)).cuda()
        for mask in (7, 6, 0):
            spec = (SEED, SID, _ctr(CTRS[1]))
            a = K.diffaug(xi, (c, h, w), mask, spec, denom=255.0)
            b = K.diffaug(K.real_prep(xi, None, 255.0), (c, h, w), mask, spec)
            assert torch.equal(a, b), (shape, mask)
    # 4 bytes into an aligned buffer: the scalar path on a shape that would take the 16-byte one
    buf = torch.randn(2 * 3 * 32 * 32 + 4, generator=torch.Generator().manual_seed(8)).cuda()
    x = buf[1:1 + 2 * 3072].view(2, 3072)
    assert x.data_ptr() % 16 == 4
    spec = (SEED, SID, _ctr(3))
    assert torch.equal(K.diffaug(x, (3, 32, 32), 6, spec), K.diffaug(x.clone(), (3, 32, 32), 6, spec))
    # (with COLOR the two paths sum the image mean in different orders: each within the bound of the oracle, not bit-equal to each other)
    ref = O.forward(x.cpu(), (3, 32, 32), O.params(SEED, SID, 3, 2, 32, 32, 7))
    assert ((K.diffaug(x, (3, 32, 32), 7, spec).cpu().double() - ref).abs() <= _bound(x.cpu(), (2, 3, 32, 32))).all()


def test_non_finite_values_stay_in_their_image(K):
    shape = (4, 3, 8, 12)
    n, c, h, w = shape
    x = torch.randn(n, c * h * w, generator=torch.Generator().manual_seed(9))
    bad = x.clone()
    bad[2, 5], bad[2, 100], bad[2, 17] = float('inf'), float('nan'), float('-inf')
    for mask in (7, 6):
        spec = (SEED, SID, _ctr(11))
        for adj in (False, True):
            a = K.diffaug(x.cuda(), (c, h, w), mask, spec, adjoint=adj).cpu()
            b = K.diffaug(bad.cuda(), (c, h, w), mask, spec, adjoint=adj).cpu()
            keep = [0, 1, 3]
            assert torch.equal(a[keep], b[keep]) and torch.isfinite(b[keep]).all(), (mask, adj)
            if mask & 1:          # the image mean spreads them over their own image; without COLOR they may be cut or shifted out
                # (a forward zero - cut or shifted in - is written after the colour map and stays 0)
                assert not torch.isfinite(b[2]).all() and (~torch.isfinite(b[2]) | ((b[2] == 0) & (a[2] == 0))).all()


def test_same_counter_same_bits_and_the_next_step_differs(K):
    from ctgan_amd.rng import AUG_FAKE, DeviceRNG
    rng = DeviceRNG(seed=5, rank=2)
    x = torch.randn(9, 3072, generator=torch.Generator().manual_seed(1)).cuda()
    a = K.diffaug(x, (3, 32, 32), 7, rng.aug_spec(AUG_FAKE))
    b = K.diffaug(x, (3, 32, 32), 7, rng.aug_spec(AUG_FAKE))
    assert torch.equal(a, b)
    K.rng_advance(rng.ctr, 1)
    c = K.diffaug(x, (3, 32, 32), 7, rng.aug_spec(AUG_FAKE))
    assert not torch.equal(a, c)
    p = O.params(5, (2 << 16) | AUG_FAKE, 1, 9, 32, 32, 7)
    assert (c.cpu().double() - O.forward(x.cpu(), (3, 32, 32), p)).abs().max().item() < 1e-4


def test_autograd_first_and_second_order(K):
    import ctgan_amd.functional as F
    shape, n = (3, 8, 12), 5
    g = torch.Generator().manual_seed(3)
    x = torch.randn(n, 288, generator=g).cuda().requires_grad_(True)
    gy = torch.randn(n, 288, generator=g).cuda().requires_grad_(True)
    v = torch.randn(n, 288, generator=g).cuda()
    spec = (SEED, SID, _ctr(2))
    y = F.diffaug(x, shape, 7, spec)
    assert torch.equal(y, K.diffaug(x.detach(), shape, 7, spec))
    (gx,) = torch.autograd.grad(y, x, grad_outputs=gy, create_graph=True)
    assert torch.equal(gx, K.diffaug(gy.detach(), shape, 7, spec, adjoint=True))
    (ggy,) = torch.autograd.grad(gx, gy, grad_outputs=v)
    assert torch.equal(ggy, K.diffaug(v, shape, 7 | K.DIFFAUG_NO_BRIGHTNESS, spec))
    assert not torch.equal(ggy, K.diffaug(v, shape, 7, spec))


# ----------------------------------------------------------------------------------------------------- trainers
@pytest.mark.parametrize('scheduled', [True, False])
def test_augmented_critic_step_is_the_plain_step_on_augmented_inputs_on_the_device(K, scheduled):
    """tests/test_diffaug_host.py's equivalence on the device, gan_mnist: d_grads with `augment` on (real, fake) == d_grads without on
    (diffaug(real, AUG_REAL), diffaug(fake, AUG_FAKE)) at the same counter, bit for bit - on dcgan_schedule.critic_step and, with that
    switch off, on the autograd form."""
    import ctgan_amd.dcgan_schedule as DS
    import ctgan_amd.gan_mnist as M
    import ctgan_amd.tflib as lib
    from ctgan_amd import rng as R
    from ctgan_amd.dcgan_step import DCGANTrainer
    B, dim = 8, 32
    real_in = torch.rand(B, 784, generator=torch.Generator().manual_seed(2)).cuda()
    res = []
    for augment in (POLICY, None):
        lib.delete_all_params(); lib.set_device(None); lib.set_seed(3)
        mode_setup('mnist', 'wgan-CT', dim, B, torch.Generator().manual_seed(0))
        try:
            build_params(M, 'cuda')
            tr = DCGANTrainer(M, seed=11, augment=augment)
            fake = tr.generate_fakes(1)[0]
            real = real_in
            if augment is None:
                real = K.diffaug(real_in, (1, 28, 28), 7, tr.rng.aug_spec(R.AUG_REAL))
                fake = K.diffaug(fake.contiguous(), (1, 28, 28), 7, tr.rng.aug_spec(R.AUG_FAKE))
                assert not torch.equal(real, real_in)
            old, DS.MERGED_BWD = DS.MERGED_BWD, scheduled
            try:
                assert DS.usable(tr, None, fake, real_in) == scheduled
                tr.rng.begin_step()
                out, grads = tr.d_grads(real, fake=fake)
            finally:
                DS.MERGED_BWD = old
            res.append(([out[k].clone() for k in ('cost', 'wgan_only', 'ct', 'gp', 'slopes')], [None if t is None else t.clone() for t in grads]))
        finally:
            lib.delete_all_params(); M.configure()
    for a, b in zip(res[0][0] + res[0][1], res[1][0] + res[1][1]):
        assert (a is None) == (b is None) and (a is None or torch.equal(a, b))
