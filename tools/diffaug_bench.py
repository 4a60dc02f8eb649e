#!/usr/bin/env python
"""Times the differentiable augmentation on one GPU, in one process.

(a) The kernel - kernels.diffaug forward, adjoint and integer-input form, policy color,translation,cutout - at the scripts' own batches:
    64 x 1 x 28 x 28 (gan_mnist), 64 x 3 x 32 x 32 (gan_cifar, the ResNet), 64 x 3 x 64 x 64 (gan_64x64), 64 x 3 x 128 x 128 (gan_lsun128).
    A sample is one replay, between two device events, of a captured graph of `--launches` back-to-back launches of one form (launched
    from Python the host's enqueue rate, ~10 us per call, hides every shape but the largest: `eager` keeps that figure for the forward);
    the forms alternate sample by sample for `--rounds` rounds after `--warmup` untimed ones; a figure is the median (with min / max) of
    a form's samples and includes the boundary between two dependent launches.  Beside each: the bytes the
    launch has to move (one read and one write of the batch - the second read of the colour pass is served by L2 and is not counted),
    that over the time, and its share of the HBM rate a float4 copy reaches on this part (6.29 TB/s; 8 TB/s is the data-sheet peak).
(b) The step - train_iteration of gan_cifar and of the headline ResNet (full width), graph-replayed, with the augmentation off and on:
    the configuration is rebuilt for every sample (a trainer owns the parameter registry), off and on alternating for `--step-rounds`
    rounds; a sample is `--iters` iterations after 3 untimed ones, host clock around a device synchronise.

Prints one JSON line; --out writes it to a file.

    python tools/diffaug_bench.py [--out profiles/diffaug_bench.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402

SHAPES = [(64, 1, 28, 28), (64, 3, 32, 32), (64, 3, 64, 64), (64, 3, 128, 128)]
POLICY = 'color,translation,cutout'
HBM_COPY_TBS = 6.29          # float4 copy, measured; the data-sheet peak is 8.0


def _stats(v, unit):
    return {'median_' + unit: statistics.median(v), 'min_' + unit: min(v), 'max_' + unit: max(v), 'samples': len(v)}


def _timed(fn, launches):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(launches):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / launches


def _graph_of(fn, launches):
    """-> a callable replaying a captured graph of `launches` launches of fn (what a graph-replayed step pays per launch)."""
    fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(launches):
            fn()
    return g.replay


def kernel_times(launches, rounds, warmup):
    import ctgan_amd.kernels as K
    mask = K.diffaug_policy(POLICY)
    ctr = torch.tensor([7], dtype=torch.int64, device='cuda')
    spec = (2024, 0xFF00, ctr)
    out = {}
    for shape in SHAPES:
        n, c, h, w = shape
        x = torch.randn(n, c * h * w, device='cuda')
        xi = torch.randint(0, 256, (n, c * h * w), dtype=torch.int32, device='cuda')
        y = torch.empty_like(x)
        forms = {'forward': lambda: K.diffaug(x, (c, h, w), mask, spec, out=y),
                 'adjoint': lambda: K.diffaug(x, (c, h, w), mask, spec, adjoint=True, out=y),
                 'forward_int': lambda: K.diffaug(xi, (c, h, w), mask, spec, denom=255.0, out=y)}
        times = {k: [] for k in list(forms) + ['eager_forward']}
        replays = {k: _graph_of(fn, launches) for k, fn in forms.items()}
        for r in range(warmup + rounds):
            for k, replay in replays.items():
                t = _timed(replay, 1) / launches
                if r >= warmup:
                    times[k].append(t)
            t = _timed(forms['forward'], launches)
            if r >= warmup:
                times['eager_forward'].append(t)
        nbytes = 2 * 4 * x.numel()
        row = {'bytes_moved': nbytes}
        for k, us in times.items():
            st = _stats(us, 'us')
            st['gbytes_per_s'] = nbytes / st['median_us'] * 1e-3
            st['share_of_hbm_copy_rate'] = st['gbytes_per_s'] / (HBM_COPY_TBS * 1e3)
            row[k] = st
        out['x'.join(map(str, shape))] = row
    return out


def _dcgan_engine(modname, augment):
    import importlib
    import ctgan_amd.tflib as lib
    from ctgan_amd.dcgan_step import DCGANTrainer
    from ctgan_amd.engine import GraphedDCGANTrainer
    M = importlib.import_module('ctgan_amd.' + modname)
    lib.delete_all_params(); lib.set_seed(0); lib.set_device(None)
    M.configure()
    B = M.cfg.BATCH_SIZE
    with torch.no_grad():
        M.Discriminator(M.Generator(2, noise=torch.zeros(2, 128, device='cuda')), u=[torch.ones(2, *s, device='cuda') for s in M.feat_shapes()])
    tr = DCGANTrainer(M, seed=2024, augment=augment)
    g = torch.Generator().manual_seed(1)
    batches = [torch.randint(0, 256, (B, M.cfg.OUTPUT_DIM), dtype=torch.int32, generator=g).cuda() for _ in range(4)]
    eng = GraphedDCGANTrainer(tr, (B, M.cfg.OUTPUT_DIM), torch.int32, use_graphs=True)
    return eng, batches, M


def _resnet_engine(augment):
    import ctgan_amd.gan_cifar_resnet as R
    import ctgan_amd.tflib as lib
    from ctgan_amd.engine import GraphedTrainer
    lib.delete_all_params(); lib.set_seed(0); lib.set_device(None)
    R.configure()
    R.build_params()
    B = R.cfg.BATCH_SIZE
    tr = R.Trainer(seed=2024, augment=augment)
    g = torch.Generator().manual_seed(1)
    batches = [(torch.randint(0, 256, (B, 3072), dtype=torch.int32, generator=g).cuda(),
                torch.randint(0, 10, (B,), dtype=torch.int32, generator=g).cuda()) for _ in range(8)]
    return GraphedTrainer(tr, use_graphs=True), batches, R


def step_times(which, iters, rounds):
    import ctgan_amd.tflib as lib
    times = {'off': [], 'on': []}
    graphs = {}
    for _ in range(rounds):
        for key, augment in (('off', None), ('on', POLICY)):
            eng, batches, M = _dcgan_engine(which, augment) if which != 'resnet' else _resnet_engine(augment)
            try:
                cur = [0]

                def nb():
                    cur[0] = (cur[0] + 1) % len(batches)
                    return batches[cur[0]]
                it = 0
                for _ in range(4):          # iteration 0 has no generator step; then three untimed replays
                    eng.train_iteration(it, nb); it += 1
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(iters):
                    eng.train_iteration(it, nb); it += 1
                torch.cuda.synchronize()
                times[key].append(1e3 * (time.perf_counter() - t0) / iters)
                graphs[key] = {'hipgraph': bool(eng.graphed), 'graph_error': eng.graph_error, 'iteration_graph': eng.it_graph is not None}
            finally:
                del eng
                lib.delete_all_params(); M.configure()
    off, on = _stats(times['off'], 'ms'), _stats(times['on'], 'ms')
    return {'off': off, 'on': on, 'added_ms': on['median_ms'] - off['median_ms'], 'time_ratio': on['median_ms'] / off['median_ms'],
            'off_spread_ms': off['max_ms'] - off['min_ms'], 'iterations_per_sample': iters, 'graphs': graphs}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--launches', type=int, default=200, help='back-to-back kernel launches per sample')
    ap.add_argument('--rounds', type=int, default=9)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--iters', type=int, default=20, help='train_iteration calls per step sample')
    ap.add_argument('--step-rounds', type=int, default=3)
    ap.add_argument('--skip-steps', action='store_true')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'diffaug_bench needs the GPU'
    res = {'what': 'differentiable augmentation (color,translation,cutout): (a) kernels.diffaug per launch at the scripts\' batches, device events '
                   'around back-to-back launches, forms alternating; (b) train_iteration, graph-replayed, augmentation off / on, rebuilt and '
                   'alternating per sample',
           'device_name': torch.cuda.get_device_name(0), 'launches_per_sample': a.launches, 'rounds': a.rounds, 'warmup_rounds': a.warmup,
           'hbm_copy_rate_tbytes_per_s': HBM_COPY_TBS, 'kernel': kernel_times(a.launches, a.rounds, a.warmup)}
    if not a.skip_steps:
        res['train_iteration'] = {'gan_cifar': step_times('gan_cifar', a.iters, a.step_rounds),
                                  'gan_cifar_resnet': step_times('resnet', a.iters, a.step_rounds)}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
