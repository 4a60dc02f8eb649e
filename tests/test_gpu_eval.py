"""ctgan_amd.evaluate on the MI355X: the held-out critic cost against the fp64 oracle at reduced width, one full-width ResNet pass against
the sum of its parts, the score-sample pixel kernel (ctgan_pixels_u8) against the torch expression it replaces, and dev passes between
hipGraph replays."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import eval_helpers as H  # noqa: E402


def _dev_set(case, n, dtype=torch.float64):
    pairs = [case.batch() for _ in range(n)]
    return [case.on_dev(p[0]) for p in pairs], [p[1] for p in pairs], [case.draws(dtype) for _ in range(n)]


# ----------------------------------------------------------------------------- 7: parity with the fp64 oracle at reduced width
@pytest.mark.parametrize('name,dim,B', [('resnet', 16, 8), ('resnet', 32, 8), ('cifar', 16, 8), ('mnist', 8, 8), ('mnist-wgan', 16, 8),
                                        ('mnist-dcgan', 16, 8), ('64x64-lsgan', 8, 4)])
def test_dev_cost_matches_the_oracle_on_the_device(name, dim, B):
    import ctgan_amd.tflib as lib
    from ctgan_amd.evaluate import Evaluator
    lib.delete_all_params(); lib.set_device(None)
    case = H.Case(lib, name, dim, B, 'cuda')
    try:
        tr = case.trainer()
        batches, batches_o, rnds = _dev_set(case, 3)
        costs, reg = case.oracle_costs(tr, batches_o, rnds)
        want = sum(costs) / len(costs)
        rnd32 = [H.f32_rnd(r, 'cuda') for r in rnds]
        for width in (2, 1):                     # width 2: a full pass and a ragged one
            out = Evaluator(tr, width=width).dev_cost(iter(batches), rnd=rnd32)
            print('%s DIM %d width %d: dev_cost %.9g, oracle %.9g' % (name, dim, width, out['dev_cost'], want))
            H.close(out['dev_cost'], want, '%s DIM %d width %d' % (name, dim, width))
            if name == 'cifar':
                ref = H.slope_real_ref(reg, case.D, batches_o[-1], rnds[-1]['u_slope'])
                print('cifar width %d: slope_real %.9g, fp64 %.9g' % (width, out['slope_real'], ref))
                H.close(out['slope_real'], ref, 'slope_real')
        # the default path (in-kernel Philox draws, fused heads): finite, and reproducible from the same counter
        ev = Evaluator(tr, width=2)
        c0 = int(ev.rng.ctr.item())
        a = ev.dev_cost(iter(batches))
        ev.rng.ctr.fill_(c0)
        b = ev.dev_cost(iter(batches))
        assert a == b and all(v == v and abs(v) < 1e6 for v in a.values()), (a, b)
        c = ev.dev_cost(iter(batches))
        assert c['dev_cost'] != a['dev_cost']
    finally:
        case.close()


# ----------------------------------------------------------------------------- 8: one full-width pass against the sum of its parts
def test_full_width_resnet_pass_equals_the_sum_of_its_parts():
    import ctgan_amd.kernels as K
    import ctgan_amd.tflib as lib
    from ctgan_amd.evaluate import Evaluator
    lib.delete_all_params(); lib.set_device(None)
    case = H.Case(lib, 'resnet', 128, 64, 'cuda')
    try:
        tr = case.trainer()
        batches, _, rnds = _dev_set(case, 4, dtype=torch.float32)
        rnd32 = [H.f32_rnd(r, 'cuda') for r in rnds]
        wide = Evaluator(tr, width=4).dev_cost(iter(batches), rnd=rnd32)
        parts = Evaluator(tr, width=1).dev_cost(iter(batches), rnd=rnd32)
        print('ResNet DIM 128 B 64: width 4 %.9g, width 1 %.9g' % (wide['dev_cost'], parts['dev_cost']))
        assert wide['n_batches'] == parts['n_batches'] == 4
        assert abs(wide['dev_cost'] - parts['dev_cost']) <= 2e-4 * abs(parts['dev_cost'])
        del rnd32, rnds
        calls = []
        wrapped = {nm: getattr(K, nm) for nm in dir(K) if nm.startswith('conv_wgrad') and callable(getattr(K, nm))}
        for nm, f in wrapped.items():
            setattr(K, nm, (lambda f, nm: lambda *a, **kw: (calls.append(nm), f(*a, **kw))[1])(f, nm))
        try:
            ev = Evaluator(tr, width=4)
            before = H.snapshot(lib, tr)
            c0 = int(ev.rng.ctr.item())
            a = ev.dev_cost(iter(batches))
            ev.rng.ctr.fill_(c0)
            b = ev.dev_cost(iter(batches))
        finally:
            for nm, f in wrapped.items():
                setattr(K, nm, f)
        print('ResNet DIM 128 B 64, in-kernel draws: %.9g' % a['dev_cost'])
        assert a == b and a['dev_cost'] == a['dev_cost'] and abs(a['dev_cost']) < 1e6
        assert not calls, calls
        H.assert_same(before, H.snapshot(lib, tr))
    finally:
        case.close()


# ----------------------------------------------------------------------------- 9: the pixel kernel
def _check_pixels(x, channels):
    import ctgan_amd.kernels as K
    for scale in (255.99 / 2, 255. / 2):
        got = K.pixels_u8(x, channels, scale)
        assert got.dtype == torch.uint8 and tuple(got.shape) == (x.shape[0], x.shape[1] // channels, channels) and got.is_contiguous()
        finite = torch.isfinite(x).reshape(x.shape[0], channels, -1).permute(0, 2, 1)
        want = H.pixels_reference(torch.where(torch.isfinite(x), x, torch.zeros_like(x)), channels, scale)
        assert torch.equal(got.to(torch.int32)[finite], want[finite])
        assert (got[~finite] == 0).all()


@pytest.mark.parametrize('name,dim,n', [('resnet', 32, 100), ('64x64', 8, 100), ('resnet', 32, 7), ('64x64', 8, 7)])
def test_pixels_u8_equals_the_torch_expression_on_generator_outputs(name, dim, n):
    import ctgan_amd.tflib as lib
    from ctgan_amd.evaluate import Evaluator
    lib.delete_all_params(); lib.set_device(None)
    case = H.Case(lib, name, dim, 4, 'cuda')
    try:
        tr = case.trainer()
        rng = Evaluator(tr).rng
        rng.begin_step()
        with torch.no_grad():
            if case.resnet:
                x = case.M.Generator(n, rng.labels(n, 10), rng=rng)
            else:
                x = case.M.Generator(n, rng=rng)
        assert x.shape == (n, case.M.cfg.OUTPUT_DIM) and torch.isfinite(x).all()
        _check_pixels(x.contiguous(), 3)
        # samples near and beyond the ends of tanh's range, scaled so that products land on and around integers
        _check_pixels((x * 1.003).contiguous(), 3)
    finally:
        case.close()


def test_pixels_u8_edges_and_the_scalar_path():
    import ctgan_amd.kernels as K
    vals = torch.tensor([-1.0, 1.0, -1.5, 1.5, -100.0, 100.0, 0.0, -0.0, float('nan'), float('inf'), float('-inf'), 0.999999, -0.999999,
                         1.0000001, 7.0, -7.0], device='cuda')
    g = torch.Generator().manual_seed(1)
    x = (torch.rand(6, 3 * 64, generator=g) * 2.4 - 1.2).cuda()
    x.view(-1)[:vals.numel()] = vals
    x.view(-1)[-vals.numel():] = vals
    _check_pixels(x, 3)
    got = K.pixels_u8(x, 3, 255.99 / 2).cpu()
    assert got[0, :11, 0].tolist() == [0, 255, 0, 255, 0, 255, 127, 127, 0, 0, 0]      # -1 -> 0, 1 -> trunc(255.99), beyond: clamped, 0 -> 127, non-finite -> 0
    # the scalar kernel: one channel, an extent that is not a multiple of 4, an unaligned view
    y = (torch.rand(5, 49, generator=g) * 2.4 - 1.2).cuda()
    _check_pixels(y, 1)
    z = (torch.rand(3, 3 * 25, generator=g) * 2.4 - 1.2).cuda()
    _check_pixels(z, 3)
    w = torch.rand(2 * 48 + 1, generator=g).cuda()[1:].reshape(2, 48)
    _check_pixels(w, 3)
    with pytest.raises(ValueError):
        K.pixels_u8(y, 1, 0.0)


# ----------------------------------------------------------------------------- 10: dev passes between graph replays
@pytest.mark.parametrize('name,dim,B', [('resnet', 32, 8), ('cifar', 32, 8)])
def test_dev_passes_between_graph_replays_leave_the_trajectory_bit_identical(name, dim, B):
    import ctgan_amd.tflib as lib
    from ctgan_amd.engine import GraphedDCGANTrainer, GraphedTrainer
    from ctgan_amd.evaluate import Evaluator
    res = {}
    for with_dev in (False, True):
        lib.delete_all_params(); lib.set_device(None)
        case = H.Case(lib, name, dim, B, 'cuda')
        try:
            tr = case.trainer(seed=5)
            batches = _dev_set(case, 3)[0]
            if case.resnet:
                eng = GraphedTrainer(tr, use_graphs=True)
            else:
                eng = GraphedDCGANTrainer(tr, (B, case.M.cfg.OUTPUT_DIM), torch.int32, use_graphs=True)
            assert eng.graphed, eng.graph_error
            ev = Evaluator(tr, width=2)
            k = [0]

            def nb():
                k[0] += 1
                return batches[k[0] % len(batches)]
            costs, devs = [], []
            for it in range(4):
                costs.append(eng.train_iteration(it, nb)['cost'].item())
                if with_dev:
                    devs.append(ev.dev_cost(iter(batches))['dev_cost'])
            res[with_dev] = (costs, tr.d_opt.theta.clone(), tr.g_opt.theta.clone(), tr.d_opt.m.clone(), tr.g_opt.m.clone(), tr.d_opt.v.clone(),
                             tr.rng.ctr.clone())
            if with_dev:
                print('%s: dev costs between replays %s' % (name, devs))
                assert all(v == v and abs(v) < 1e6 for v in devs) and len(set(devs)) == len(devs)
        finally:
            case.close()
    assert res[False][0] == res[True][0]
    for x, y in zip(res[False][1:], res[True][1:]):
        assert torch.equal(x, y)


# ----------------------------------------------------------------------------- the loops on the device, hipGraph steps
def _fake_cifar(path, rows):
    import os
    import pickle

    import numpy as np
    g = np.random.default_rng(0)
    for name in ['data_batch_%d' % k for k in range(1, 6)] + ['test_batch']:
        with open(os.path.join(path, name), 'wb') as f:
            pickle.dump({'data': g.integers(0, 256, (rows, 3072), dtype=np.uint8), 'labels': [int(v) for v in g.integers(0, 10, rows)]}, f, protocol=2)


def _log(path):
    import json
    import os
    return [json.loads(line) for line in open(os.path.join(path, 'log.jsonl'))]


def test_resnet_loop_logs_dev_cost(tmp_path):
    import numpy as np
    import ctgan_amd.gan_cifar_resnet as R
    import ctgan_amd.tflib as lib
    _fake_cifar(str(tmp_path), 64)
    lib.delete_all_params(); lib.set_device(None); lib.set_seed(1)
    R.configure(DIM_G=16, DIM_D=16, BATCH_SIZE=8, ITERS=6)
    scored = []

    def classifier(x):
        scored.append(x.shape)
        return np.full((x.shape[0], 10), 0.1)
    try:
        tr = R.train(str(tmp_path), n_examples=200, out_dir=str(tmp_path), sample_every=3, checkpoint_every=4, dev_every=2, log=lambda *a: None)
        assert tr.d_opt.t == 30 and tr.g_opt.t == 5
        log = _log(str(tmp_path))
        assert [r['iter'] for r in log if 'dev_cost' in r] == [1, 3, 5] and all(abs(r['dev_cost']) < 1e6 for r in log if 'dev_cost' in r)
        assert not any('inception_50k' in r for r in log)
        from ctgan_amd.evaluate import Evaluator
        mean, std = Evaluator(tr).get_inception_score(500, classifier)
        assert abs(mean - 1.0) < 1e-6 and std < 1e-6 and sum(s[0] for s in scored) == 500 and all(s[1:] == (32, 32, 3) for s in scored)
    finally:
        lib.delete_all_params(); R.configure()


def test_cifar_dcgan_loop_logs_dev_cost_and_slope_under_graphs(tmp_path):
    import os

    import ctgan_amd.gan_cifar as M
    import ctgan_amd.tflib as lib
    _fake_cifar(str(tmp_path), 32)
    lib.delete_all_params(); lib.set_device(None); lib.set_seed(2)
    M.configure(DIM=32, BATCH_SIZE=8)
    try:
        tr = M.train(str(tmp_path), n_examples=160, iters=4, out_dir=str(tmp_path), use_graphs=True, sample_every=2, dev_every=2,
                     checkpoint_every=4, log=None)
        assert tr.d_opt.t == 20 and tr.g_opt.t == 3
        log = _log(str(tmp_path))
        assert [r['iter'] for r in log] == [0, 1, 2, 3]
        assert [r['iter'] for r in log if 'dev disc cost' in r] == [1, 3] == [r['iter'] for r in log if 'slope_real' in r]
        assert all(abs(r['dev disc cost']) < 1e6 and r['slope_real'] > 0 for r in log if 'slope_real' in r)
        assert all(os.path.exists(os.path.join(str(tmp_path), f)) for f in ('samples_1.png', 'samples_3.png', 'checkpoint.pt'))
    finally:
        M.configure(); lib.delete_all_params()
