"""The generator's weight average on the MI355X (`-m gpu`): the `avg` operand of the four update launches and ctgan_exchange
(csrc/optim_rng.hip), the trainers' `g_average` / `averaged()` under graph replay, checkpoint resume, and the `averaged` flag of the
scoring.  Not in the reference, so every check is the feature's own contract and every comparison is bit for bit:
  * theta, the slots, the bucket and the skip count of an averaging launch equal the launch without the average (the same code);
  * the average equals a + rate * (theta - a) in numpy float32 on the kernel's own theta - two IEEE operations with contraction off, so
    equality is the derived bound, not a tolerance;
  * `averaged()` is a pure exchange: nothing a later graph replay reads has moved by a bit, and no derived-filter cache serves the other
    set of weights."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import eval_helpers as H  # noqa: E402
from tests import score_cifar_oracle as O  # noqa: E402
from tests.test_gan_modes_host import build_params, mode_setup  # noqa: E402
from tests.test_gpu_score_cifar import _full_width_trainer, clean  # noqa: E402,F401  (fixture and helper)

RATE = 0.125
LENGTHS = (1, 3, 4, 5, 255, 256, 257, 1027)          # one element, below / at / above the 4-wide body, around one block, several blocks
STEPS = 5


@pytest.fixture
def K():
    import ctgan_amd.kernels as K
    return K


def recurrence(avg, theta, rate):
    """avg + rate * (theta - avg) in IEEE fp32, one rounding per operation, on the device's own theta."""
    a, t = avg.cpu().numpy().astype(np.float32), theta.cpu().numpy().astype(np.float32)
    return torch.from_numpy((a + np.float32(rate) * (t - a)).astype(np.float32))


def _segments(n):
    """Segment sizes of a packed update over n elements: a 4-aligned segment, one of odd length, one at an odd offset without a source
    (zero gradient), the rest (at offset 16; its length is a multiple of 4 for n = 256 only)."""
    if n < 16:
        return [4, n - 4] if n > 4 else [n]
    return [8, 5, 3, n - 16]


def _gradients(n, g):
    """STEPS flat gradients; steps 1 and 3 carry one inf and one NaN (both on the only element of n = 1, in turn)."""
    out = []
    for k in range(STEPS):
        x = torch.randn(n, generator=g)
        if k in (1, 3):
            if n == 1:
                x[0] = float('inf') if k == 1 else float('nan')
            else:
                x[0], x[n - 1] = float('inf'), float('nan')
        out.append(x.cuda())
    return out


def _run(K, kind, n, form, averaging, grads, theta0):
    """STEPS updates of one form -> per step (theta, slots..., state, bucket, avg or None), on the host."""
    adam = kind == 'adam'
    clip = {'adam': 0.0, 'rmsprop': 0.0, 'rmsprop-clip': 0.01}[kind]
    theta = theta0.clone().cuda()
    slots = [torch.zeros(n, device='cuda'), torch.zeros(n, device='cuda')] if adam else [torch.ones(n, device='cuda')]
    state = torch.tensor([0.003, 0.5, 0.9, 0.0] if adam else [0.003, 1.0, 1.0, 0.0], device='cuda')
    flat = torch.zeros(n, device='cuda')
    avg = theta.clone() if averaging else None
    kw = {'avg': avg, 'avg_rate': RATE} if averaging else {}
    sizes = _segments(n)
    offs = [sum(sizes[:i]) for i in range(len(sizes))]
    rows = []
    for g in grads:
        if form == 'plain':
            flat.copy_(g)
            if adam:
                K.adam_step(theta, flat, slots[0], slots[1], state, 0.5, 0.9, 1e-8, 0.5, **kw)
            else:
                K.rmsprop_step(theta, flat, slots[0], state, 0.9, 1e-10, clip, 0.5, **kw)
        else:
            srcs = [None if (len(sizes) == 4 and i == 2) else g[o:o + s].clone() for i, (o, s) in enumerate(zip(offs, sizes))]
            if adam:
                K.adam_step_packed(srcs, offs, sizes, flat, theta, slots[0], slots[1], state, 0.5, 0.9, 1e-8, 0.5, **kw)
            else:
                K.rmsprop_step_packed(srcs, offs, sizes, flat, theta, slots[0], state, 0.9, 1e-10, clip, 0.5, **kw)
        K.step_advance(state, 0.5 if adam else 1.0, 0.9 if adam else 1.0)
        rows.append([t.cpu().clone() for t in [theta] + slots + [state, flat]] + [avg.cpu().clone() if averaging else None])
    return rows


# ----------------------------------------------------------------------------------------------------- the update kernels
@pytest.mark.parametrize('kind', ['adam', 'rmsprop', 'rmsprop-clip'])
def test_update_kernels_with_the_average(K, kind):
    g = torch.Generator().manual_seed(11)
    for n in LENGTHS:
        theta0 = torch.randn(n, generator=g) * 0.02          # (inside and outside the clip bound of 0.01)
        grads = _gradients(n, g)
        got = {}
        for form in ('plain', 'packed'):
            # the packed form zeroes the gradient of the sourceless segment: the plain form gets the same bucket
            sizes = _segments(n)
            gs = [x.clone() for x in grads]
            if len(sizes) == 4:
                for x in gs:
                    x[13:16] = 0.0
            off, on = _run(K, kind, n, form, False, gs, theta0), _run(K, kind, n, form, True, gs, theta0)
            want = theta0.clone()
            for k in range(STEPS):
                for i, (a, b) in enumerate(zip(on[k][:-1], off[k][:-1])):          # theta, m, v / ms, state (skip count), the bucket
                    assert torch.equal(a, b) or (torch.equal(torch.isnan(a), torch.isnan(b)) and torch.equal(a.nan_to_num(7.0), b.nan_to_num(7.0))), \
                        (kind, n, form, k, i)
                want = recurrence(want, on[k][0], RATE)
                assert torch.equal(on[k][-1], want), (kind, n, form, k)
            assert float(on[-1][-3][3]) == (2.0 if n == 1 else 4.0)          # the skipped elements are counted, and averaged all the same
            assert torch.isfinite(on[-1][-1]).all() and not torch.equal(on[-1][-1], on[-1][0])
            got[form] = on
        for k in range(STEPS):
            assert torch.equal(got['plain'][k][-1], got['packed'][k][-1]) and torch.equal(got['plain'][k][0], got['packed'][k][0]), (kind, n, k)
        if kind == 'rmsprop-clip':
            assert float(got['plain'][-1][0].abs().max()) <= 0.01


def test_update_kernels_refuse_bad_average_arguments_and_launch_nothing(K):
    from ctgan_amd._lib import lib
    n = 8
    th, g, m, v, a = (torch.full((n,), x, device='cuda') for x in (1.0, 0.5, 0.0, 0.0, 3.0))
    state = torch.tensor([0.1, 0.5, 0.9, 0.0], device='cuda')
    flat = torch.zeros(n, device='cuda')
    p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None          # noqa: E731
    P, Of, C = (ctypes.c_void_p * 1)(g.data_ptr()), (ctypes.c_int64 * 1)(0), (ctypes.c_int64 * 1)(n)
    for avg, rate in ((None, 0.5), (a, 0.0), (a, -0.5), (a, 1.5), (a, float('nan'))):
        assert lib.ctgan_adam_step(p(th), p(g), p(m), p(v), n, p(state), 0.5, 0.9, 1e-8, 1.0, p(avg), rate, None, None) == -1
        assert b'avg' in lib.ctgan_last_error()
        assert lib.ctgan_rmsprop_step(p(th), p(g), p(m), n, p(state), 0.9, 1e-10, 0.0, 1.0, p(avg), rate, None, None) == -1
        assert lib.ctgan_adam_step_packed(P, Of, C, 1, p(flat), p(th), p(m), p(v), p(state), 0.5, 0.9, 1e-8, 1.0, p(avg), rate, None, None) == -1
        assert lib.ctgan_rmsprop_step_packed(P, Of, C, 1, p(flat), p(th), p(m), p(state), 0.9, 1e-10, 0.0, 1.0, p(avg), rate, None, None) == -1
    big = torch.full((n + 1,), 3.0, device='cuda')
    odd = big[1:]                                                                    # 4 bytes past a 16-byte boundary
    assert lib.ctgan_adam_step_packed(P, Of, C, 1, p(flat), p(th), p(m), p(v), p(state), 0.5, 0.9, 1e-8, 1.0, p(odd), 0.5, None, None) == -2
    assert lib.ctgan_rmsprop_step_packed(P, Of, C, 1, p(flat), p(th), p(m), p(state), 0.9, 1e-10, 0.0, 1.0, p(odd), 0.5, None, None) == -2
    torch.cuda.synchronize()
    for t, x in ((th, 1.0), (m, 0.0), (v, 0.0), (a, 3.0), (flat, 0.0), (big, 3.0)):
        assert torch.equal(t, torch.full_like(t, x))
    with pytest.raises(ValueError):
        K.adam_step(th, g, m, v, state, 0.5, 0.9, avg=a, avg_rate=0.0)
    K.adam_step(th, g, m, v, state, 0.5, 0.9, avg=a, avg_rate=1.0)                    # rate 1 is allowed: the average jumps to the weights
    assert torch.equal(a.cpu(), recurrence(torch.full((n,), 3.0), th, 1.0)) and not torch.equal(th, torch.ones_like(th))


# ----------------------------------------------------------------------------------------------------- exchange_
def test_exchange_swaps_exactly_on_both_paths(K):
    g = torch.Generator().manual_seed(2)
    for n in (0, 1, 3, 4, 5, 1027, 4096):
        for shift in (0, 1):                          # 1: slices 4 bytes into an aligned buffer - the scalar path whatever n is
            A, B = torch.randn(n + 2, generator=g).cuda(), torch.randn(n + 2, generator=g).cuda()
            A0, B0 = A.clone(), B.clone()
            a, b = A[shift:shift + n], B[shift:shift + n]
            assert a.data_ptr() % 16 == 4 * shift or n == 0
            K.exchange_(a, b)
            assert torch.equal(a, B0[shift:shift + n]) and torch.equal(b, A0[shift:shift + n]), (n, shift)
            for full, keep in ((A, A0), (B, B0)):          # nothing outside the slices moved
                assert torch.equal(full[:shift], keep[:shift]) and torch.equal(full[shift + n:], keep[shift + n:]), (n, shift)
            K.exchange_(a, b)
            assert torch.equal(A, A0) and torch.equal(B, B0), (n, shift)
    x = torch.zeros(8, device='cuda')
    with pytest.raises(ValueError):
        K.exchange_(x[:6], x[2:])                     # overlapping buffers cannot be swapped elementwise in parallel
    with pytest.raises(AssertionError):
        K.exchange_(x[:4], x[4:7])


# ----------------------------------------------------------------------------------------------------- trainers
def _resnet_batches(B, n=8, seed=1234):
    nrng = np.random.default_rng(seed)
    return [(torch.from_numpy(nrng.integers(0, 256, (B, 3072), dtype=np.int32)).cuda(),
             torch.from_numpy(nrng.integers(0, 10, (B,), dtype=np.int32)).cuda()) for _ in range(n)]


def _resnet_run(dim, B, iters, graphs, g_average, batches, between=None, at=None, resume=None, save=None, seed=0):
    """-> final (g theta, g avg or None, g m, g v, d theta) of `iters` iterations; `between(trainer)` runs after iteration `at`."""
    import ctgan_amd.gan_cifar_resnet as R
    import ctgan_amd.tflib as lib
    from ctgan_amd import checkpoint
    from ctgan_amd.engine import GraphedTrainer
    lib.delete_all_params(); lib.set_device(None); lib.set_seed(seed)
    R.configure(DIM_G=dim, DIM_D=dim, BATCH_SIZE=B)
    try:
        R.build_params()
        tr = R.Trainer(seed=2024, g_average=g_average)
        start = checkpoint.load(resume, tr) if resume else 0
        eng = GraphedTrainer(tr, use_graphs=graphs)
        assert eng.graphed == graphs, eng.graph_error
        if graphs:
            assert eng.it_graph is not None and eng.adam_in_graph          # one graph per iteration, the update inside it
        cur = [start * R.cfg.N_CRITIC]

        def nb():
            cur[0] += 1
            return batches[cur[0] % len(batches)]
        extra = None
        for it in range(start, iters):
            eng.train_iteration(it, nb)
            if save is not None and it + 1 == save[1]:
                checkpoint.save(save[0], tr, iteration=it + 1)
            if between is not None and it + 1 == at:
                extra = between(tr)
        o = tr.g_opt
        return (o.theta.clone(), None if o.avg is None else o.avg.clone(), o.m.clone(), o.v.clone(), tr.d_opt.theta.clone()), extra
    finally:
        lib.delete_all_params(); R.configure()


def test_resnet_graph_replay_equals_eager_and_the_average_changes_no_weight():
    """The Adam script: per-step graphs in iteration 0, then one graph per iteration with the update (and so the average) inside it."""
    dim, B, iters = 32, 8, 3
    batches = _resnet_batches(B)
    (g, _), (e, _), (off, _) = (_resnet_run(dim, B, iters, graphs, rate, batches) for graphs, rate in ((True, RATE), (False, RATE), (True, 0.0)))
    for a, b in zip(g, e):
        assert torch.equal(a, b)
    assert off[1] is None and not torch.equal(g[1], g[0])
    for i in (0, 2, 3, 4):
        assert torch.equal(g[i], off[i]), i


def test_rmsprop_mode_graph_replay_equals_eager_and_the_average_changes_no_weight():
    import ctgan_amd.gan_mnist as M
    import ctgan_amd.tflib as lib
    from ctgan_amd.dcgan_step import DCGANTrainer
    from ctgan_amd.engine import GraphedDCGANTrainer
    dim, B = 32, 8
    nrng = np.random.default_rng(5)
    batches = [torch.from_numpy(nrng.random((B, 784), dtype=np.float32)).cuda() for _ in range(4)]

    def run(graphs, rate):
        lib.delete_all_params(); lib.set_device(None); lib.set_seed(3)
        mode_setup('mnist', 'wgan', dim, B, torch.Generator().manual_seed(0))
        build_params(M, 'cuda')
        tr = DCGANTrainer(M, seed=11, g_average=rate)
        assert tr.g_opt.kind == 'rmsprop' and tr.d_opt.avg is None
        eng = GraphedDCGANTrainer(tr, (B, M.cfg.OUTPUT_DIM), batches[0].dtype, use_graphs=graphs)
        assert eng.graphed == graphs, eng.graph_error
        k = [0]

        def nb():
            k[0] += 1
            return batches[k[0] % len(batches)]
        for it in range(3):
            eng.train_iteration(it, nb)
        o = tr.g_opt
        return o.theta.clone(), None if o.avg is None else o.avg.clone(), o.ms.clone(), tr.d_opt.theta.clone()
    try:
        g, e, off = run(True, RATE), run(False, RATE), run(True, 0.0)
        for a, b in zip(g, e):
            assert torch.equal(a, b)
        assert off[1] is None and not torch.equal(g[1], g[0])
        for i in (0, 2, 3):
            assert torch.equal(g[i], off[i]), i
    finally:
        lib.delete_all_params(); M.configure()


@pytest.mark.parametrize('mma', [None, 'bf16'])
def test_averaged_context_serves_no_stale_filter_image_and_leaves_graph_replay_alone(K, mma):
    import ctgan_amd.tflib as lib
    dim, B = 64, 8                                       # 64 channels: the generator's convs take the 16-bit family under 'bf16'
    batches = _resnet_batches(B)
    noise = torch.randn(16, 128, generator=torch.Generator().manual_seed(0)).cuda()
    labels = (torch.arange(16, dtype=torch.int32) % 10).cuda()

    def visit(tr):
        before = tr.generate_samples(noise, labels)[0].clone()          # (also fills the host-side caches with the live weights' images)
        with tr.averaged():
            inside = tr.generate_samples(noise, labels)[0].clone()
        after = tr.generate_samples(noise, labels)[0].clone()
        # the same thing the slow way: the average copied over the weights with plain torch ops, every cache told
        keep = tr.g_opt.theta.clone()
        tr.g_opt.theta.copy_(tr.g_opt.avg); lib.bump_epoch()
        ref = tr.generate_samples(noise, labels)[0].clone()
        tr.g_opt.theta.copy_(keep); lib.bump_epoch()
        again = tr.generate_samples(noise, labels, averaged=True)[0].clone()
        return before, inside, after, ref, again
    old = K.set_mma_dtype(mma)
    try:
        visited, (before, inside, after, ref, again) = _resnet_run(dim, B, 4, True, RATE, batches, between=visit, at=2)
        straight, _ = _resnet_run(dim, B, 4, True, RATE, batches)
    finally:
        K.set_mma_dtype(old)
    assert torch.equal(inside, ref) and torch.equal(again, ref) and torch.equal(after, before) and not torch.equal(inside, before)
    for a, b in zip(visited, straight):
        assert torch.equal(a, b)


def test_graphed_trainer_resumes_the_average_bit_exactly(tmp_path):
    dim, B = 16, 8
    batches = _resnet_batches(B, n=4, seed=7)
    path = str(tmp_path / 'ck.pt')
    whole, _ = _resnet_run(dim, B, 4, True, RATE, batches, save=(path, 2), seed=4)
    resumed, _ = _resnet_run(dim, B, 4, True, RATE, batches, resume=path, seed=4)
    for a, b in zip(whole, resumed):
        assert torch.equal(a, b)
    assert not torch.equal(whole[1], whole[0])


# ----------------------------------------------------------------------------------------------------- scoring
def test_score_generator_of_the_average(K, clean):          # noqa: F811
    import ctgan_amd.tflib as lib
    from ctgan_amd import evaluate
    from ctgan_amd.score_cifar import ClassifierScore
    M = clean
    ctr = _full_width_trainer(M)
    lib.delete_params_with_name('Generator.')          # the classifier trainer's own generator: its names are the GAN's
    scorer = ClassifierScore(ctr)
    case = H.Case(lib, 'resnet', 16, 4, 'cuda')
    try:
        gan = case.M.Trainer(seed=1, g_average=RATE)
        (real, labels), _ = case.batch()
        real, labels = real.cuda(), labels.cuda()
        for it in range(2):
            gan.train_iteration(it, lambda: (real, labels))
        assert not torch.equal(gan.g_opt.avg, gan.g_opt.theta)
        stream = evaluate.eval_stream(gan)
        c0 = int(stream.ctr.item())
        before = H.snapshot(lib, gan)
        live = scorer.score_generator(gan, 300)
        c1 = int(stream.ctr.item())
        got = scorer.score_generator(gan, 300, averaged=True)          # the loops' order: the average on the next steps of the stream
        assert int(stream.ctr.item()) - c1 == c1 - c0 > 0
        H.assert_same(before, H.snapshot(lib, gan))
        stream.ctr.fill_(c1)
        with gan.averaged():
            want = scorer.score_generator(gan, 300)
        assert set(got) == set(want) == set(live)
        for k in got:
            assert np.array_equal(np.asarray(got[k]), np.asarray(want[k])), k
        assert not np.array_equal(np.asarray(got['hist']), np.asarray(live['hist'])) or got['mean'] != live['mean']
        stream.ctr.fill_(c1)
        fa = scorer.features_generator(gan, 300, averaged=True).features
        stream.ctr.fill_(c1)
        with gan.averaged():
            fb = scorer.features_generator(gan, 300).features
        assert torch.equal(fa, fb)
        H.assert_same(before, H.snapshot(lib, gan))
        # without the flag: what a trainer built without an average scores on the same weights at the same stream position
        plain = case.M.Trainer(seed=1)
        evaluate.eval_stream(plain).ctr.fill_(c0)
        base = scorer.score_generator(plain, 300)
        assert set(base) == set(live)
        for k in live:
            assert np.array_equal(np.asarray(base[k]), np.asarray(live[k])), k
        with pytest.raises(ValueError):
            scorer.score_generator(plain, 300, averaged=True)
    finally:
        case.close()
