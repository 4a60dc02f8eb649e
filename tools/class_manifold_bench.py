#!/usr/bin/env python
"""What the grouped (per-class) launches of DESIGN 27 take beside a loop of the pooled launches over the gathered classes.

    python tools/class_manifold_bench.py --out profiles/class_manifold_bench.json

Shapes: 10 classes, 128 features, 10,000 x 50,000 rows (samples x reference) and 50,000 x 50,000, labels uniform over the classes, fp32
ReLU-Gaussian rows.  Two groups of launches, the ones a scoring with the class references runs after its last chunk:
    manifold   the samples against the reference balls, the samples' radii, the reference against the sample balls (k = 3)
                 grouped: knn_cover_seg, knn_radii_seg, knn_cover_seg - 3 launches          loop: knn_cover, knn_radii, knn_cover per class - 30
    kernel     the samples' own kernel sums and the sums across, reduced to per-class totals
                 grouped: 2 kernel_tile_sums_seg + 2 segment_sums - 4 launches               loop: 2 kernel_tile_sums + 2 sums per class - 40
The loop is given what it cannot have inside a scoring without a synchronisation: the class counts on the host and the gathered rows,
both made before the clock starts.  The reference's own radii and totals are cached by a FeatureSet and are in neither.

A sample is a FRESH process (`--mode sample`) that builds the inputs, runs `--warmup` rounds of its variant and times `--iters` more,
host clock around a device synchronise (what a scoring waits for: launch overhead included); it prints the mean per round.  The two
variants alternate sample by sample for `--reps` rounds inside the one call.  Reported per variant and group: the median, minimum and
maximum of its samples; per group the ratio of the medians beside the spread (max - min) of the loop's own samples, which a difference
has to exceed to mean anything."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SHAPES = {'10000x50000': (10000, 50000), '50000x50000': (50000, 50000)}
CLASSES, WIDTH, NEIGHBOURS = 10, 128, 3


def sample(a):
    import numpy as np
    import torch
    import ctgan_amd.kernels as K
    assert torch.cuda.is_available(), 'class_manifold_bench needs the GPU'
    m, n = SHAPES[a.shape]
    r = np.random.RandomState(3)
    fa = torch.from_numpy(np.maximum(0.0, r.randn(m, WIDTH)).astype(np.float32)).cuda()
    fb = torch.from_numpy((1.05 * np.maximum(0.0, r.randn(n, WIDTH))).astype(np.float32)).cuda()
    la, lb = torch.from_numpy(r.randint(0, CLASSES, m)).cuda(), torch.from_numpy(r.randint(0, CLASSES, n)).cuda()
    (pa, sa), (pb, sb) = K.class_segments(la, CLASSES), K.class_segments(lb, CLASSES)
    fa, fb = fa.index_select(0, pa).contiguous(), fb.index_select(0, pb).contiguous()
    r2b = K.knn_radii_seg(fb, sb, NEIGHBOURS)
    if a.variant == 'grouped':
        def manifold():
            K.knn_cover_seg(fa, sa, fb, sb, r2b)
            K.knn_cover_seg(fb, sb, fa, sa, K.knn_radii_seg(fa, sa, NEIGHBOURS))

        def kernel():
            K.segment_sums(*K.kernel_tile_sums_seg(fa, sa, fa, sa, exclude_diag=True))
            K.segment_sums(*K.kernel_tile_sums_seg(fa, sa, fb, sb))
    else:
        ha, hb = sa.tolist(), sb.tolist()
        ga = [fa[ha[c]:ha[c + 1]].clone() for c in range(CLASSES)]
        gb = [fb[hb[c]:hb[c + 1]].clone() for c in range(CLASSES)]
        gr = [r2b[hb[c]:hb[c + 1]].clone() for c in range(CLASSES)]

        def manifold():
            for c in range(CLASSES):
                K.knn_cover(ga[c], gb[c], gr[c])
                K.knn_cover(gb[c], ga[c], K.knn_radii(ga[c], NEIGHBOURS))

        def kernel():
            for c in range(CLASSES):
                K.kernel_tile_sums(ga[c], ga[c], exclude_diag=True).sum()
                K.kernel_tile_sums(ga[c], gb[c]).sum()
    rec = {'shape': a.shape, 'variant': a.variant}
    for name, fn in (('manifold', manifold), ('kernel', kernel)):
        for _ in range(a.warmup):
            fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.iters):
            fn()
        torch.cuda.synchronize()
        rec[name + '_ms'] = 1e3 * (time.perf_counter() - t0) / a.iters
    print('SAMPLE ' + json.dumps(rec))


def _stats(v):
    return {'median_ms': statistics.median(v), 'min_ms': min(v), 'max_ms': max(v), 'spread_ms': max(v) - min(v), 'samples': len(v)}


def measure(a):
    out = {}
    for shape in a.shape_list:
        recs = {'grouped': [], 'loop': []}
        for _ in range(a.reps):
            for variant in ('grouped', 'loop'):
                cmd = [sys.executable, os.path.abspath(__file__), '--mode', 'sample', '--shape', shape, '--variant', variant, '--iters', str(a.iters),
                       '--warmup', str(a.warmup)]
                p = subprocess.run(cmd, env=dict(os.environ, PYTHONPATH=ROOT), capture_output=True, text=True, timeout=a.sample_timeout)
                lines = [ln for ln in p.stdout.splitlines() if ln.startswith('SAMPLE ')]
                if p.returncode != 0 or not lines:
                    raise SystemExit('sample %s/%s failed (rc %d): %s' % (shape, variant, p.returncode, p.stderr[-2000:]))
                recs[variant].append(json.loads(lines[-1][7:]))
        row = {'rounds_per_sample': a.iters, 'warmup_rounds': a.warmup}
        for group in ('manifold', 'kernel'):
            g = {v: _stats([r[group + '_ms'] for r in recs[v]]) for v in recs}
            g['grouped_over_loop'] = g['grouped']['median_ms'] / g['loop']['median_ms']
            g['loop_minus_grouped_ms'] = g['loop']['median_ms'] - g['grouped']['median_ms']
            row[group] = g
        out[shape] = row
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--mode', choices=('measure', 'sample'), default='measure')
    ap.add_argument('--shape', action='append', default=None, choices=sorted(SHAPES))
    ap.add_argument('--variant', choices=('grouped', 'loop'), default='grouped')
    ap.add_argument('--iters', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--sample-timeout', type=int, default=240)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    a.shape_list = a.shape or sorted(SHAPES)
    sys.path.insert(0, ROOT)
    if a.mode == 'sample':
        a.shape = a.shape_list[0]
        return sample(a)
    res = {'what': 'grouped per-class launches (knn_cover_seg / knn_radii_seg; kernel_tile_sums_seg + segment_sums) against a loop of the pooled '
                   'launches over the gathered classes: %d classes, %d features, k = %d; one fresh process per sample, the variants alternating; '
                   'host clock around a device synchronise' % (CLASSES, WIDTH, NEIGHBOURS),
           'reps': a.reps, 'shapes': measure(a)}
    line = json.dumps(res, indent=1)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
