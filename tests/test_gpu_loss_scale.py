"""The dynamic loss scale on the device: the gradient scan against torch.isfinite on tables built to hit every path of the kernel, the
scaled update / end-of-step launches bit for bit against tests/loss_scale_cpu_kernels.py layered on the STATIC launches, a run that
starts at a scale far too large and corrects itself, graph replay against eager, the fp16 mode, and an exact resume."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

FLT_MAX = 3.4028234663852886e38
PACK_MAX = 64


def _special(bits):
    return torch.tensor([bits], dtype=torch.int32).view(torch.float32).item()


# +inf, -inf, a quiet NaN, a negative NaN
NONFINITE = [float('inf'), float('-inf'), _special(0x7fc00000), _special(0xffc00000 - (1 << 32))]


def _same_bits(a, b):
    """torch.equal that also holds for NaN against the same NaN."""
    if a.dtype == torch.float32:
        a, b = a.view(torch.int32), b.view(torch.int32)
    return torch.equal(a, b)


def _fresh_scaler():
    return torch.tensor([1024.0, 0.0, 7.0, 3.0], dtype=torch.float32, device='cuda')


def _scan(K, srcs):
    """-> the flag after one scan launch over `srcs`; the other three words must come back untouched."""
    sc = _fresh_scaler()
    K.grads_nonfinite(srcs, sc)
    got = sc.tolist()
    assert got[0] == 1024.0 and got[2:] == [7.0, 3.0] and got[1] in (0.0, 1.0)
    return got[1] == 1.0


def _offset_tensor(n, g):
    """n elements that start 4 bytes past a 16-byte boundary."""
    base = torch.randn(n + 1, generator=g).cuda()
    t = base[1:]
    assert t.data_ptr() % 16 == 4 and t.is_contiguous()
    return t


def _finite_fill(t, k):
    """Values that are finite but look extreme: +-FLT_MAX, denormals, -0."""
    vals = torch.tensor([FLT_MAX, -FLT_MAX, 1e-45, -1e-45, 1.1754942e-38, -0.0, 0.0, 1.0], dtype=torch.float32)
    t.copy_(vals[(torch.arange(t.numel()) + k) % len(vals)].to(t.device))


def test_scan_kernel_against_isfinite_on_every_path():
    import ctgan_amd.kernels as K
    g = torch.Generator().manual_seed(0)
    sizes = [1, 3, 4, 5, 1023]
    # ---- the table form: the odd sizes, a None entry, a tensor 4 bytes off alignment, one that needs a second trip of the strided loop
    probe = [torch.empty(s, device='cuda') for s in sizes] + [None, torch.empty(1023, device='cuda')]
    gx, gy, threads, per = K.grads_nonfinite_grid(probe + [torch.empty(1 << 22, device='cuda')])
    assert (gy, threads, per) == (len(probe) + 1, 256, 4)
    n_big = (gx * threads + 1) * per          # one 16-byte item past what one pass of the launched grid covers
    table = [torch.randn(s, generator=g).cuda() for s in sizes] + [None, _offset_tensor(1023, g), torch.randn(n_big, generator=g).cuda()]
    assert K.grads_nonfinite_grid(table)[0] == gx and (n_big // per) == gx * threads + 1
    full = [torch.randn(1 + (i % 9), generator=g).cuda() for i in range(PACK_MAX)]          # a full table of PACK_MAX entries
    flat_gx = K.grads_nonfinite_grid(torch.empty(1 << 24, device='cuda'))[0]
    flat = torch.randn((flat_gx * threads + 1) * per + 3, generator=g).cuda()                 # the flat-bucket form: second trip + a tail
    assert K.grads_nonfinite_grid(flat) == (flat_gx, 1, 256, 4)
    cases = {'table': table, 'full': full, 'flat': [flat], 'flat offset': [_offset_tensor(1023 + 6, g)]}
    for name, srcs in cases.items():
        arg = srcs[0] if name.startswith('flat') else srcs
        assert _scan(K, arg) is False, name
        last = [t for t in srcs if t is not None][-1]
        spots = []
        for t in [t for t in srcs if t is not None]:
            n = t.numel()
            head = ((16 - t.data_ptr() % 16) % 16) // 4
            body_end = head + ((n - head) // 4) * 4          # one past the last element of the 16-byte body
            spots += [(t, 0)]
            if body_end > head:
                spots += [(t, body_end - 1)]
            if body_end < n:
                spots += [(t, n - 1), (t, body_end)]          # inside the scalar tail
            if head:
                spots += [(t, head - 1)]                       # the elements in front of the first 16-byte boundary
        if name == 'full':
            spots = [s for s in spots if s[0] is srcs[0] or s[0] is last or s[0].numel() in (4, 5, 8)]
        spots += [(last, last.numel() - 1), (last, last.numel() // 2)]          # the last table entry; the second trip of the big ones
        for i, (t, pos) in enumerate(spots):
            for bad in (NONFINITE if i < 8 else [NONFINITE[i % 4]]):
                keep = t[pos].clone()
                t[pos] = bad
                assert not bool(torch.isfinite(t).all())
                assert _scan(K, arg) is True, (name, t.numel(), pos, bad)
                t[pos] = keep
        assert _scan(K, arg) is False, name
        for k, t in enumerate(t for t in srcs if t is not None):
            _finite_fill(t, k)
            assert bool(torch.isfinite(t).all())
        assert _scan(K, arg) is False, (name, 'FLT_MAX, denormals and -0 are finite')
    # the flag is only ever set: a clean scan after a dirty one leaves it (the end of the step clears it)
    sc = _fresh_scaler()
    K.grads_nonfinite([torch.tensor([float('nan')], device='cuda')], sc)
    K.grads_nonfinite([torch.ones(5, device='cuda')], sc)
    assert sc[1].item() == 1.0
    with pytest.raises(Exception):
        K.grads_nonfinite([torch.ones(2, device='cuda')] * (PACK_MAX + 1), sc)


@pytest.fixture
def on_static_launches(monkeypatch):
    """tests/loss_scale_cpu_kernels.py's wrappers forwarding to the real STATIC launches of ctgan_amd.kernels."""
    import ctgan_amd.kernels as K
    from tests import loss_scale_cpu_kernels as S
    for name in S.__all__:
        monkeypatch.setitem(S._BASE, name, getattr(K, name))
    return S


@pytest.mark.parametrize('kind', ['adam', 'rmsprop-clip'])
@pytest.mark.parametrize('with_avg', [False, True])
def test_scaled_update_and_advance_forms_against_the_stand_ins(on_static_launches, kind, with_avg):
    """Good and dropped steps, plain and packed launches, at odd sizes and more than one workgroup: the scaled launch against the stand-in,
    which on a good step IS the static launch at grad_scale / S - bit equality with the static kernels - and on a dropped one the
    contract in torch ops.  Then the end of the step against its stand-in."""
    import ctgan_amd.kernels as K
    S = on_static_launches
    g = torch.Generator().manual_seed(1)
    sizes = [1, 3, 4, 5, 1023, (1 << 20) + 4]          # the last: three trips of the packed launch's strided loop, 16-byte path
    offsets = [sum(sizes[:i]) for i in range(len(sizes))]
    total = sum(sizes)
    consts = (3, 2.0, 4096.0)

    def fresh():
        gg = torch.Generator().manual_seed(2)
        d = {'theta': torch.randn(total, generator=gg).cuda() * 0.1, 'flat': torch.zeros(total, device='cuda'),
             'state': torch.tensor([0.01, 0.5, 0.9, 0.0], device='cuda') if kind == 'adam' else torch.tensor([0.01, 1.0, 1.0, 0.0], device='cuda'),
             'scaler': torch.tensor([1024.0, 0.0, 1.0, 0.0], device='cuda'), 'ctr': torch.tensor([5], dtype=torch.int64, device='cuda')}
        if kind == 'adam':
            d['m'] = torch.zeros(total, device='cuda'); d['v'] = torch.zeros(total, device='cuda')
        else:
            d['ms'] = torch.ones(total, device='cuda')
        if with_avg:
            d['avg'] = d['theta'].clone() * 0.5
        return d

    def step(mod, d, srcs, packed):
        kw = {'avg': d['avg'], 'avg_rate': 0.125} if with_avg else {}
        mod.grads_nonfinite(srcs if packed else d['flat'], d['scaler'])
        if kind == 'adam':
            if packed:
                mod.adam_step_packed(srcs, offsets, sizes, d['flat'], d['theta'], d['m'], d['v'], d['state'], 0.5, 0.9, 1e-8, 0.5, scaler=d['scaler'], **kw)
            else:
                mod.adam_step(d['theta'], d['flat'], d['m'], d['v'], d['state'], 0.5, 0.9, 1e-8, 0.5, scaler=d['scaler'], **kw)
        else:
            if packed:
                mod.rmsprop_step_packed(srcs, offsets, sizes, d['flat'], d['theta'], d['ms'], d['state'], 0.9, 1e-10, 0.05, 0.5, scaler=d['scaler'], **kw)
            else:
                mod.rmsprop_step(d['theta'], d['flat'], d['ms'], d['state'], 0.9, 1e-10, 0.05, 0.5, scaler=d['scaler'], **kw)
        mod.step_advance(d['state'], 0.5, 0.9, d['ctr'], 1, scaler=d['scaler'], scaler_consts=consts)

    dev, ref = fresh(), fresh()
    # steps: good, good (growth at 3 good: the scaler starts with one), dropped, good, dropped, dropped
    plan = [None, None, (4, 700), None, (0, 0), (5, (1 << 20) + 3)]
    prev = None
    scales = []
    for k, bad in enumerate(plan):
        srcs = [torch.randn(s, generator=g).cuda() * 1024.0 for s in sizes]
        srcs[1] = None if k == 1 else srcs[1]
        if bad is not None:
            srcs[bad[0]][bad[1]] = NONFINITE[k % 4]
        packed = k % 2 == 0
        for mod, d in ((K, dev), (S, ref)):
            if not packed:
                K.pack(srcs, offsets, sizes, d['flat'])
            step(mod, d, srcs, packed)
        for name in dev:
            assert _same_bits(dev[name], ref[name]), (kind, with_avg, k, name)
        if bad is not None:
            for name in ('m', 'v', 'ms'):
                if name in dev:
                    assert torch.equal(dev[name], prev[name]), (k, name)
            assert torch.equal(dev['state'], prev['state'])
            if kind == 'adam':
                assert torch.equal(dev['theta'], prev['theta'])
            else:
                assert torch.equal(dev['theta'], prev['theta'].clamp(-0.05, 0.05))
            if with_avg:
                assert not torch.equal(dev['avg'], prev['avg'])
        prev = {n: t.clone() for n, t in dev.items()}
        scales.append(dev['scaler'].tolist())
    assert [s[0] for s in scales] == [1024.0, 2048.0, 1024.0, 1024.0, 512.0, 256.0]
    assert scales[-1] == [256.0, 0.0, 0.0, 3.0] and dev['ctr'].item() == 5 + len(plan) and dev['state'][3].item() == 0.0
    # the clamps
    for flag, start, want in ((1.0, 2.0, 2.0), (0.0, 4096.0, 4096.0)):
        sc = torch.tensor([start, flag, 2.0, 0.0], device='cuda')
        K.step_advance(dev['state'], 0.5, 0.9, None, 1, scaler=sc, scaler_consts=consts)
        assert sc[0].item() == want and sc[1].item() == 0.0
    with pytest.raises(ValueError):
        K.step_advance(dev['state'], 0.5, 0.9, None, 1, scaler=sc, scaler_consts=(3, 3.0, 4096.0))


def test_scaled_good_step_is_bit_equal_to_the_static_kernel_directly():
    """The same statement without any stand-in in between: adam_step(scaler=) at S against adam_step(grad_scale / S)."""
    import ctgan_amd.kernels as K
    g = torch.Generator().manual_seed(3)
    for n in (1, 3, 4, 5, 1023, 70001):
        for S in (1.0, 1024.0, 2.0 ** 24):
            grad = torch.randn(n, generator=g).cuda() * S
            a = [torch.randn(n, generator=g).cuda(), torch.rand(n, generator=g).cuda(), torch.rand(n, generator=g).cuda()]
            b = [t.clone() for t in a]
            sa, sb = (torch.tensor([0.01, 0.5, 0.9, 0.0], device='cuda') for _ in range(2))
            K.adam_step(a[0], grad, a[1], a[2], sa, 0.5, 0.9, 1e-8, 0.25, scaler=torch.tensor([S, 0.0, 0.0, 0.0], device='cuda'))
            K.adam_step(b[0], grad, b[1], b[2], sb, 0.5, 0.9, 1e-8, 0.25 / S)
            assert all(torch.equal(x, y) for x, y in zip(a, b)) and not torch.equal(a[0], grad)


# ----------------------------------------------------------------------------- trainers
def _mnist(mode, dim=16, B=8):
    import ctgan_amd.gan_mnist as M
    import ctgan_amd.tflib as lib
    from tests.test_gan_modes_host import build_params
    lib.delete_all_params(); lib.set_device(None); lib.set_seed(3)
    M.configure(DIM=dim, BATCH_SIZE=B, **({'MODE': mode} if mode else {}))
    build_params(M, 'cuda')
    return M


def _batches(B, n=6):
    g = torch.Generator().manual_seed(0)
    return [torch.rand(B, 784, generator=g).cuda() for _ in range(n)]


def _cleanup():
    import ctgan_amd.gan_mnist as M
    import ctgan_amd.kernels as K
    import ctgan_amd.tflib as lib
    K.set_mma_dtype(None)
    lib.delete_all_params(); M.configure()


def _scaler(init, growth=4):
    from ctgan_amd.optim import LossScaler
    return LossScaler(init_scale=init, growth_interval=growth, max_scale=max(init, 2.0 ** 24), device='cuda')


@pytest.mark.parametrize('log2_init', [120, 127])
def test_a_scale_far_too_large_corrects_itself(log2_init):
    """The CT objective on gan_mnist at DIM 16, batch 8 (the smallest configuration tests/test_gpu_gan_modes.py trains), every step
    eager, one host read of the scaler per update.  While updates are dropped the scale halves at each and both networks' weights stay
    as they are to the bit; an applied update moves weights; at the end everything is finite and the number of dropped updates is log2
    of (initial / final scale) - no growth in this run (growth_interval beyond its length).

    2^120 is the scale this test was specified with.  On this configuration the gradients stay below 2^8 (measured on the CPU stand-ins:
    no update is dropped at 2^120, five at 2^127, which ends at 2^122), so the 2^120 case checks that a large scale that does NOT
    overflow is left alone and costs no update, and the 2^127 case - a gradient element of magnitude 2 overflows there - is the one
    that has to see dropped updates first and applied ones after."""
    from ctgan_amd.dcgan_step import DCGANTrainer
    try:
        M = _mnist(None)
        init = 2.0 ** log2_init
        tr = DCGANTrainer(M, seed=11, loss_scale=_scaler(init, growth=10 ** 9))
        batches = _batches(8)
        S, dropped, applied, applied_after_drop = init, 0, 0, 0
        k = 0
        for it in range(4):
            steps = ([('g', None)] if it else []) + [('d', batches[(k + i) % 6]) for i in range(tr.disc_iters)]
            for which, real in steps:
                k += 1
                before = (tr.d_opt.theta.clone(), tr.g_opt.theta.clone(), tr.d_opt.m.clone(), tr.g_opt.v.clone(), tr.d_opt.state[1:].clone())          # (state[0]: the learning rate, set per step)
                tr.iteration = it
                tr.d_step(real) if which == 'd' else tr.g_step()
                now, n_drop = tr.scaler.scale(), tr.scaler.skipped_steps()
                after = (tr.d_opt.theta, tr.g_opt.theta, tr.d_opt.m, tr.g_opt.v, tr.d_opt.state[1:])
                if n_drop > dropped:
                    assert n_drop == dropped + 1 and now == S / 2
                    assert all(torch.equal(a, b) for a, b in zip(before, after)), 'a dropped update changes no weight and no slot'
                else:
                    assert now == S
                    opt_i = 0 if which == 'd' else 1
                    assert not torch.equal(before[opt_i], after[opt_i])
                    applied += 1
                    applied_after_drop += dropped > 0
                S, dropped = now, n_drop
        assert applied > 0 and tr.scaler.good_steps() > 0
        assert bool(torch.isfinite(tr.d_opt.theta).all()) and bool(torch.isfinite(tr.g_opt.theta).all())
        assert bool(torch.isfinite(tr.d_opt.m).all()) and bool(torch.isfinite(tr.d_opt.v).all())
        assert tr.scaler.skipped_steps() == round(math.log2(init / tr.scaler.scale())) and tr.d_opt.skipped() == 0 and tr.g_opt.skipped() == 0
        print('log2_init %d: dropped %d, applied %d, final scale 2^%d' % (log2_init, dropped, applied, round(math.log2(S))))
        if log2_init == 127:
            assert dropped >= 1 and applied_after_drop >= 1, 'after the scale came down the updates are applied'
    finally:
        _cleanup()


def _run(mode, scaler_of, graphs, dtype=None, dim=16, n_it=4, ckpt=None):
    """n_it iterations through the engine -> everything that has to agree between two runs."""
    import ctgan_amd.kernels as K
    from ctgan_amd import checkpoint
    from ctgan_amd.dcgan_step import DCGANTrainer
    from ctgan_amd.engine import GraphedDCGANTrainer
    K.set_mma_dtype(dtype)
    M = _mnist(mode, dim=dim)
    tr = DCGANTrainer(M, seed=11, loss_scale=scaler_of())
    start = 0
    if ckpt and ckpt[0] == 'load':
        start = checkpoint.load(ckpt[1], tr)
    before = tr.scaler.state.clone()
    eng = GraphedDCGANTrainer(tr, (8, 784), torch.float32, use_graphs=graphs)
    assert eng.graphed == graphs, eng.graph_error
    if graphs:
        assert eng.it_graph is not None, eng.it_graph_error
    assert torch.equal(tr.scaler.state, before), 'capture leaves the scaler state as it found it'
    batches = _batches(8)
    k = [start * tr.disc_iters]

    def nb():
        k[0] += 1
        return batches[k[0] % 6]
    trace, costs = [], []
    for it in range(start, n_it):
        out = eng.train_iteration(it, nb)          # iteration 0: the separate critic graph; later ones: the one-iteration graph
        costs.append(float(out['cost'].item()))
        trace.append(tr.scaler.state.tolist())
        if ckpt and ckpt[0] == 'save' and it + 1 == ckpt[2]:
            checkpoint.save(ckpt[1], tr, it + 1)
    if graphs:          # ... and the separate generator and critic graphs once more, behind the iteration graph
        eng.g_step(); eng.d_step(batches[0])
    else:
        tr.iteration = n_it - 1
        tr.g_step(); tr.d_step(batches[0], fake=tr.generate_fakes(1)[0])          # (what the engine's stand-alone critic step does)
    trace.append(tr.scaler.state.tolist())
    return {'trace': trace, 'costs': costs, 'd': tr.d_opt.theta.clone(), 'g': tr.g_opt.theta.clone(), 'ctr': int(tr.rng.ctr.item()),
            'd_slots': [s.clone() for s in tr.d_opt.slots()], 'g_slots': [s.clone() for s in tr.g_opt.slots()],
            'skipped_elems': tr.d_opt.skipped() + tr.g_opt.skipped()}


def _same(a, b):
    assert a['trace'] == b['trace'] and a['ctr'] == b['ctr']
    assert torch.equal(a['d'], b['d']) and torch.equal(a['g'], b['g'])
    for x, y in zip(a['d_slots'] + a['g_slots'], b['d_slots'] + b['g_slots']):
        assert torch.equal(x, y)
    for x, y in zip(a['costs'], b['costs']):
        assert x == y or abs(x - y) <= 1e-5 * max(1.0, abs(y)), (x, y)


@pytest.mark.parametrize('mode,log2_init', [(None, 120), (None, 127), ('wgan', 127)])
def test_graph_replay_equals_eager_while_the_scale_changes(mode, log2_init):
    """The self-correcting run through GraphedDCGANTrainer: the separate critic graph (iteration 0), the one-iteration graph, then the
    separate generator and critic graphs again, against the same steps eager - bit-equal weights, slots and scaler state after every
    iteration, those during which the scale halves or (growth_interval 4) doubles included."""
    try:
        e = _run(mode, lambda: _scaler(2.0 ** log2_init), False)
        g = _run(mode, lambda: _scaler(2.0 ** log2_init), True)
        _same(g, e)
        scales = [t[0] for t in g['trace']]
        print('mode %s 2^%d: scales 2^%s, dropped %d' % (mode, log2_init, [round(math.log2(s)) for s in scales], g['trace'][-1][3]))
        if mode is None and log2_init == 127:
            assert len(set(scales)) > 1 and g['trace'][-1][3] >= 1, 'the run has to cover iterations during which the scale changes'
        assert bool(torch.isfinite(g['d']).all()) and bool(torch.isfinite(g['g']).all()) and g['skipped_elems'] == 0
    finally:
        _cleanup()


@pytest.mark.parametrize('dim', [16, 32])
@pytest.mark.parametrize('mode', [None, 'dcgan'])
def test_fp16_mode_under_the_dynamic_scale(mode, dim):
    """set_mma_dtype('f16') with the default scaler (2^16), the CT objective and MODE 'dcgan': finite losses, no element ever skipped by
    the per-element check, graph replay equal to eager.  At DIM 16, the tiny configuration of the tests above, and at DIM 32 (the width
    of this module's graph-replay test in tests/test_gpu_gan_modes.py), where more layers have the channel counts - multiples of 32 /
    64 - that the 16-bit matrix-core kernels take."""
    from ctgan_amd.optim import LossScaler
    try:
        e = _run(mode, lambda: LossScaler(device='cuda'), False, dtype='f16', dim=dim, n_it=3)
        g = _run(mode, lambda: LossScaler(device='cuda'), True, dtype='f16', dim=dim, n_it=3)
        _same(g, e)
        assert all(math.isfinite(c) for c in g['costs']) and g['skipped_elems'] == 0
        assert bool(torch.isfinite(g['d']).all()) and bool(torch.isfinite(g['g']).all())
    finally:
        _cleanup()


def test_resume_mid_run_with_a_moved_scale_is_bit_exact(tmp_path):
    path = str(tmp_path / 'ck.pt')
    try:
        whole = _run(None, lambda: _scaler(2.0 ** 127, growth=7), False, n_it=4, ckpt=('save', path, 2))
        saved = torch.load(path, map_location='cpu', weights_only=False)['loss_scaler']['state'].tolist()
        assert saved[0] != 2.0 ** 127 and saved[2] > 0, 'the checkpoint has to hold a non-initial scale and a non-zero good count'
        resumed = _run(None, lambda: _scaler(2.0 ** 127, growth=7), False, n_it=4, ckpt=('load', path))
        assert resumed['trace'] == whole['trace'][2:] and resumed['ctr'] == whole['ctr']
        assert torch.equal(resumed['d'], whole['d']) and torch.equal(resumed['g'], whole['g'])
        for x, y in zip(resumed['d_slots'] + resumed['g_slots'], whole['d_slots'] + whole['g_slots']):
            assert torch.equal(x, y)
    finally:
        _cleanup()


def test_a_fixed_scale_launches_what_it_always_launched():
    """Launch introspection (ctgan_debug_optim_launches): a trainer with a fixed scale makes one static update and one static end-of-step
    launch per update and none of the scan / scaled kinds; a dynamic one makes one scan, one scaled update and one scaled end of step per
    update and none of the static kinds."""
    from ctgan_amd._lib import lib as L
    from ctgan_amd.dcgan_step import DCGANTrainer
    from ctgan_amd.optim import LossScaler
    try:
        for ls, moved in ((None, (0, 1)), (1024.0, (0, 1)), (LossScaler(init_scale=1024.0, device='cuda'), (2, 3, 4))):
            M = _mnist(None)
            tr = DCGANTrainer(M, seed=11, loss_scale=ls)
            batches = _batches(8)
            before = [L.ctgan_debug_optim_launches(k) for k in range(5)]
            for it in range(2):
                tr.train_iteration(it, lambda: batches[it])
            torch.cuda.synchronize()
            diff = [L.ctgan_debug_optim_launches(k) - before[k] for k in range(5)]
            n_updates = 2 * tr.disc_iters + 1
            assert diff == [n_updates if k in moved else 0 for k in range(5)], (ls, diff)
        assert L.ctgan_debug_optim_launches(9) == 0
    finally:
        _cleanup()
