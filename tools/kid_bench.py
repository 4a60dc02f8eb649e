#!/usr/bin/env python
"""Times the kernel-distance tile sums (csrc/kid.hip) and what the kernel distance adds to the scripts' own scoring, on one GPU, in one
process:

    kernels     kernels.kernel_tile_sums per launch at `--shapes` (m x n x d), beside kernels.knn_cover (with radii) at the same shape
                in the same run - existing code, the yardstick - device events around `--launches` back-to-back launches after a
                warm-up (fewer for the large shapes: about `--budget-gflop` of work per figure).  With the arithmetic floor
                2 m n d FLOP at `--fp64-matrix-tflops` (the part's fp64 matrix rate) the achieved fraction is written next to each time.
    plain       ClassifierScore.score_generator without a kernel reference: the baseline, the path of tools/score_cifar_bench.py's
                `device`
    kernel      the same scorer with a kernel reference of `--reference-rows` rows whose own tile sums are already there: the features
                of the same classifier passes into one device buffer, two kernel_tile_sums launches at the end, the estimate and its
                blocks in the scoring's one host copy

A scoring figure is the median (and min / max) of `--runs` scorings after `--warmup` untimed ones, host clock around a scoring that ends
in a device synchronise; the two alternate run by run and score the same samples (the evaluation stream's counter is put back before
each scoring; the score keys of the two must be equal).  The classifier is tools/score_cifar_bench.py's (full width, init on random
uint8 data, no training: the time does not depend on the weights; the kernel distance of such a network means nothing).  Prints one
JSON line; --out writes it to a file.

    python tools/kid_bench.py [--out profiles/kid_bench.json]
"""
import argparse
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import score_cifar_bench as B  # noqa: E402
from knn_bench import SCORE_KEYS, _ms, _per_launch_us  # noqa: E402

KID_KEYS = ('kid', 'kid_std', 'kid_blocks')


def kernel_times(shapes, launches, budget_gflop, peak_tflops, k):
    import ctgan_amd.kernels as K
    out = {}
    for m, n, d in shapes:
        g = torch.Generator(device='cuda').manual_seed(m + n)
        a = torch.randn(m, d, device='cuda', generator=g)
        b = torch.randn(n, d, device='cuda', generator=g)
        r2 = K.knn_radii(b, k)
        bufs = (torch.empty(m, dtype=torch.int32, device='cuda'), torch.empty(m, dtype=torch.float64, device='cuda'),
                torch.empty(m, dtype=torch.int32, device='cuda'))
        sums = torch.empty(-(-m // K.KERNEL_TILE), -(-n // K.KERNEL_TILE), dtype=torch.float64, device='cuda')
        flop = 2.0 * m * n * d
        count = int(max(2, min(launches, budget_gflop * 1e9 / flop)))
        row = {'fp64_flop': flop, 'launches': count, 'floor_us': flop / peak_tflops * 1e-6}
        for name, fn in (('kernel_tile_sums', lambda: K.kernel_tile_sums(a, b, out=sums)), ('knn_cover', lambda: K.knn_cover(a, b, r2, *bufs))):
            us = _per_launch_us(fn, count)
            row[name] = {'us_per_launch': us, 'tflops': flop / us * 1e-6, 'fraction_of_fp64_matrix_rate': flop / us * 1e-6 / peak_tflops}
        row['kernel_tile_sums']['tiles'] = sums.numel()
        row['knn_cover']['workgroups'] = (m + 63) // 64
        row['kernel_tile_sums_over_knn_cover'] = row['kernel_tile_sums']['us_per_launch'] / row['knn_cover']['us_per_launch']
        out['%dx%dx%d' % (m, n, d)] = row
    return out


def measure(name, n, scorer, reference, dev, runs, warmup):
    from ctgan_amd import evaluate
    mod, gan = B.gan_trainer(name, dev)
    try:
        times, last = {'plain': [], 'kernel': []}, {}
        c0 = int(evaluate.eval_stream(gan).ctr.item())
        for run in range(warmup + runs):
            for path in ('plain', 'kernel'):
                scorer.set_kernel_reference(reference if path == 'kernel' else None)
                evaluate.eval_stream(gan).ctr.fill_(c0)          # every scoring draws the same samples
                t, last[path] = _ms(lambda: scorer.score_generator(gan, n), dev)
                if run >= warmup:
                    times[path].append(t)
        for key in SCORE_KEYS:
            assert np.array_equal(np.asarray(last['plain'][key]), np.asarray(last['kernel'][key])), key
        assert not set(KID_KEYS) & set(last['plain']) and set(last['kernel']) == set(last['plain']) | set(KID_KEYS)
        out = {'samples': n, 'reference_rows': reference.n, 'plain': B._stats(times['plain']), 'kernel': B._stats(times['kernel']),
               'score': last['plain']['mean'], 'kid': last['kernel']['kid'], 'kid_std': last['kernel']['kid_std'],
               'blocks': len(last['kernel']['kid_blocks'])}
        out['added_ms'] = out['kernel']['median_ms'] - out['plain']['median_ms']
        out['plain_spread_ms'] = out['plain']['max_ms'] - out['plain']['min_ms']
        return out
    finally:
        scorer.set_kernel_reference(None)
        mod.configure()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--runs', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=1)
    ap.add_argument('--init-rows', type=int, default=100)
    ap.add_argument('--reference-rows', type=int, default=50000)
    ap.add_argument('--k', type=int, default=3)
    ap.add_argument('--launches', type=int, default=50)
    ap.add_argument('--budget-gflop', type=float, default=4000.0)
    ap.add_argument('--fp64-matrix-tflops', type=float, default=78.6, help="the part's fp64 matrix rate (MI355X: 78.6)")
    ap.add_argument('--shapes', default='1000x50000x128,50000x1000x128,10000x10000x128,50000x50000x128')
    ap.add_argument('--kernel-only', action='store_true', help='only the kernel launches (for a kernel trace of its own)')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'kid_bench needs the GPU'
    from ctgan_amd import evaluate
    dev = 'cuda'
    shapes = [tuple(int(v) for v in s.split('x')) for s in a.shapes.split(',')]
    res = {'what': 'kernel_tile_sums per launch beside knn_cover at the same shape (device events), and one scoring of the script\'s sample '
                   'count under a full-width CT classifier with a kernel reference set and without (plain: the baseline); wall clock ended '
                   'by a device synchronise, the two alternating on the same samples',
           'device_name': torch.cuda.get_device_name(0), 'runs': a.runs, 'warmup': a.warmup, 'k': a.k,
           'fp64_matrix_tflops': a.fp64_matrix_tflops, 'kernels': kernel_times(shapes, a.launches, a.budget_gflop, a.fp64_matrix_tflops, a.k)}
    if not a.kernel_only:
        scorer = B.build_scorer(dev, a.init_rows)
        images = torch.from_numpy(np.random.RandomState(4).randint(0, 256, (a.reference_rows, 3, 32, 32)).astype(np.uint8)).to(dev)
        scorer.features(images[:2000])                                          # warm-up: the filters, the code objects
        reference = scorer.features(images)
        t_tiles = _ms(reference.kernel_tiles, dev)[0]
        res['reference'] = {'rows': reference.n, 'features': reference.width, 'kernel_tiles_once_ms': t_tiles}
        for name in ('gan_cifar_resnet', 'gan_cifar'):
            res[name] = measure(name, evaluate.SCORE_SAMPLES[name], scorer, reference, dev, a.runs, a.warmup)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
