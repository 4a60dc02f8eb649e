#!/usr/bin/env python
"""Times what the classifier Frechet distance adds to the scripts' own scoring - 50,000 samples of gan_cifar_resnet, 1,000 of gan_cifar,
at the scripts' widths, under a full-width CT classifier (tools/score_cifar_bench.py's: init on random uint8 data, no training; the
time does not depend on the weights) - on one GPU, in one process:

    plain       ClassifierScore.score_generator without a reference: the baseline, the path of tools/score_cifar_bench.py's `device`
    reference   the same scorer with a reference set: the features of the same classifier passes -> kernels.moments_accum per chunk,
                the moments in the scoring's one host copy, the distance on the host (numpy)

A figure is the median (and min / max) of `--runs` scorings after `--warmup` untimed ones, host clock around a scoring that ends in a
device synchronise; the two alternate run by run and score the same samples (the evaluation stream's counter is put back before each
scoring; the score keys of the two must be equal).  Also timed: building the one-off reference over `--reference-rows` uint8 images
(ClassifierScore.statistics; from a host array, and from a tensor already on the device), the host-side distance alone, and
kernels.moments_accum and kernels.class_moments_accum (`--classes` uniformly random labels) per launch at `--shapes` (device events around `--launches` back-to-back launches; the kernel's own time comes from
a rocprofv3 --kernel-trace run of this tool with --kernel-only).  Prints one JSON line; --out writes it to a file.

    python tools/frechet_bench.py [--out profiles/frechet_bench.json]
"""
import argparse
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import score_cifar_bench as B  # noqa: E402

SCORE_KEYS = ('mean', 'std', 'splits', 'hist', 'acc')


def _ms(fn, dev):
    B._sync(dev)
    t0 = time.perf_counter()
    out = fn()
    B._sync(dev)
    return (time.perf_counter() - t0) * 1e3, out


def kernel_times(shapes, launches):
    """kernels.moments_accum per launch, microseconds: device events around `launches` back-to-back launches after a warm-up."""
    import ctgan_amd.kernels as K
    out = {}
    for m, d in shapes:
        f = torch.randn(m, d, device='cuda')
        s1, s2 = torch.zeros(d, dtype=torch.float64, device='cuda'), torch.zeros(d, d, dtype=torch.float64, device='cuda')
        for _ in range(10):
            K.moments_accum(f, s1, s2)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(launches):
            K.moments_accum(f, s1, s2)
        b.record()
        torch.cuda.synchronize()
        out['%dx%d' % (m, d)] = {'us_per_launch': a.elapsed_time(b) * 1e3 / launches, 'launches': launches,
                                 'workgroups': ((d + 15) // 16) * ((d + 15) // 16 + 1) // 2, 'fp64_flop': 2 * m * d * d}
    return out


def class_kernel_times(shapes, classes, launches):
    """kernels.class_moments_accum per launch over uniformly random labels of `classes` classes, microseconds, as kernel_times."""
    import ctgan_amd.kernels as K
    out = {}
    for m, d in shapes:
        f = torch.randn(m, d, device='cuda')
        lab = torch.randint(0, classes, (m,), device='cuda', dtype=torch.int32)
        cnt = torch.zeros(classes, dtype=torch.int64, device='cuda')
        s1 = torch.zeros(classes, d, dtype=torch.float64, device='cuda')
        s2 = torch.zeros(classes, d, d, dtype=torch.float64, device='cuda')
        for _ in range(10):
            K.class_moments_accum(f, lab, cnt, s1, s2)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(launches):
            K.class_moments_accum(f, lab, cnt, s1, s2)
        b.record()
        torch.cuda.synchronize()
        out['%dx%dx%d' % (m, d, classes)] = {'us_per_launch': a.elapsed_time(b) * 1e3 / launches, 'launches': launches,
                                             'workgroups': ((d + 15) // 16) * ((d + 15) // 16 + 1) // 2 * classes}
    return out


def measure(name, n, scorer, reference, dev, runs, warmup):
    from ctgan_amd import evaluate
    mod, gan = B.gan_trainer(name, dev)
    try:
        times, last = {'plain': [], 'reference': []}, {}
        c0 = int(evaluate.eval_stream(gan).ctr.item())
        for run in range(warmup + runs):
            for path in ('plain', 'reference'):
                scorer.set_reference(reference if path == 'reference' else None)
                evaluate.eval_stream(gan).ctr.fill_(c0)          # every scoring draws the same samples
                t, last[path] = _ms(lambda: scorer.score_generator(gan, n), dev)
                if run >= warmup:
                    times[path].append(t)
        for k in SCORE_KEYS:
            assert np.array_equal(np.asarray(last['plain'][k]), np.asarray(last['reference'][k])), k
        assert 'frechet' not in last['plain']
        out = {'samples': n, 'plain': B._stats(times['plain']), 'reference': B._stats(times['reference']), 'frechet': last['reference']['frechet'],
               'score': last['plain']['mean']}
        out['added_ms'] = out['reference']['median_ms'] - out['plain']['median_ms']
        out['plain_spread_ms'] = out['plain']['max_ms'] - out['plain']['min_ms']
        return out
    finally:
        scorer.set_reference(None)
        mod.configure()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--runs', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=1)
    ap.add_argument('--init-rows', type=int, default=100)
    ap.add_argument('--reference-rows', type=int, default=50000)
    ap.add_argument('--launches', type=int, default=200)
    ap.add_argument('--shapes', default='1000x192,1000x128,100x128')
    ap.add_argument('--classes', type=int, default=10, help='classes of the class_moments_accum launches at --shapes')
    ap.add_argument('--kernel-only', action='store_true', help='only the moments_accum launches (for a kernel trace of its own)')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'frechet_bench needs the GPU'
    from ctgan_amd import evaluate
    from ctgan_amd.score_cifar import frechet_distance
    dev = 'cuda'
    shapes = [tuple(int(v) for v in s.split('x')) for s in a.shapes.split(',')]
    res = {'what': 'one scoring of the script\'s sample count under a full-width CT classifier, with a Frechet reference set and without '
                   '(plain: the baseline); wall clock ended by a device synchronise, the two alternating on the same samples',
           'device_name': torch.cuda.get_device_name(0), 'runs': a.runs, 'warmup': a.warmup, 'moments_accum': kernel_times(shapes, a.launches),
           'class_moments_accum': class_kernel_times(shapes, a.classes, a.launches)}
    if not a.kernel_only:
        scorer = B.build_scorer(dev, a.init_rows)
        images = np.random.RandomState(4).randint(0, 256, (a.reference_rows, 3, 32, 32)).astype(np.uint8)
        scorer.statistics(images[:2000])                                        # warm-up: the filters, the code objects
        t_host = [_ms(lambda: scorer.statistics(images), dev) for _ in range(3)]
        on_dev = torch.from_numpy(images).to(dev)
        t_dev = [_ms(lambda: scorer.statistics(on_dev), dev)[0] for _ in range(3)]
        reference = t_host[-1][1]
        var = np.diag(reference.cov)
        ratio = reference.mean ** 2 / var
        res['reference'] = {'rows': a.reference_rows, 'features': int(reference.mean.size), 'from_host_array_ms': B._stats([t for t, _ in t_host]),
                            'from_device_tensor_ms': B._stats(t_dev), 'mean2_over_var_median': float(np.median(ratio)),
                            'mean2_over_var_max': float(ratio.max()), 'cov_eig_min': float(np.linalg.eigvalsh(reference.cov)[0]),
                            'cov_eig_max': float(np.linalg.eigvalsh(reference.cov)[-1])}
        small = scorer.statistics(images[:1000])
        res['host_distance_ms'] = B._stats([_ms(lambda: frechet_distance(small, reference), 'cpu')[0] for _ in range(5)])
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
