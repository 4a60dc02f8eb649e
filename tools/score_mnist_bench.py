#!/usr/bin/env python
"""Times the train step and the statistics pass of the self-trained MNIST score classifier (ctgan_amd/score_mnist.py) at the
script's sizes (B 500, 28x28, widths 32/32/32/64/64) on one GPU, graph-replayed (engine.GraphedScoreTrainer), with the residual
block's fused epilogue on and off (functional.SCORE_FUSED = CTGAN_SCORE_FUSED) - both engines in ONE process on the same weights,
in alternating rounds.  A figure is the median / minimum / 90th percentile of `--iters` timed calls per round after `--warmup`
untimed ones, each call ended by a device synchronize (wall clock), pooled over `--rounds` rounds.  Prints one JSON line; --out
writes it to a file.

    python tools/score_mnist_bench.py --iters 50 --warmup 10 [--out profiles/score_mnist_bench.json]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402


def samples(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return ts


def stats(ts):
    ts = sorted(ts)
    return {'median_ms': ts[len(ts) // 2], 'min_ms': ts[0], 'p90_ms': ts[int(len(ts) * 0.9)], 'n': len(ts)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=50)
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--batch', type=int, default=500)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'score_mnist_bench needs the GPU'
    import ctgan_amd.functional as F
    import ctgan_amd.score_mnist as M
    import ctgan_amd.tflib as lib
    from ctgan_amd.engine import GraphedScoreTrainer
    dev = torch.device('cuda', 0)
    M.configure(BATCH_SIZE=a.batch)
    lib.delete_all_params(); lib.set_seed(1)
    tr = M.ScoreTrainer()
    g = torch.Generator().manual_seed(0)
    x = torch.rand(a.batch, 784, generator=g).to(dev)
    y = torch.randint(0, 10, (a.batch,), generator=g, dtype=torch.int32).to(dev)
    engines = {}
    for name, fused in (('fused', True), ('unfused', False)):
        F.SCORE_FUSED = fused
        engines[name] = GraphedScoreTrainer(tr, use_graphs=True)
        assert engines[name].graphed, engines[name].graph_error
    F.SCORE_FUSED = True
    pool = {k: [] for k in ('step_fused', 'step_unfused', 'stats_fused', 'stats_unfused')}
    for _ in range(a.rounds):
        for name in ('fused', 'unfused'):
            e = engines[name]
            pool['step_' + name] += samples(lambda: e.step(x, y), a.iters, a.warmup)
            pool['stats_' + name] += samples(lambda: e.bn_stats_pass(x, 1), a.iters, a.warmup)
    res = {'what': 'score_mnist train step / statistics pass, graph replay, B=%d, one GPU, wall clock per call ended by a synchronize' % a.batch,
           'device': torch.cuda.get_device_name(0), 'iters': a.iters, 'warmup': a.warmup, 'rounds': a.rounds}
    res.update({k: stats(v) for k, v in pool.items()})
    res['skipped'] = tr.opt.skipped()
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
