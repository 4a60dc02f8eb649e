#!/usr/bin/env python
"""Times the convolutional semi-supervised CT classifier (ctgan_amd/ct_cifar.py) at the script's sizes (B 100, 32x32, the full
widths) on one GPU: ms per classifier step and per generator step, graph-replayed (engine.GraphedCifarSSLTrainer; the augmenting
gathers are inside the graphs) and eager, and ms per augmenting-gather launch on its own.  Every figure is the median of `--iters`
timed calls after `--warmup` untimed ones, each call ended by a device synchronize.  Also counts the kernel launches of one eager
iteration (torch.profiler).  Prints one JSON line; --out writes it to a file.

    python tools/ssl_cifar_bench.py --iters 100 --warmup 10 [--out profiles/ssl_cifar_bench.json]
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402


def timed(fn, iters, warmup):
    """Median, minimum and 90th percentile of `iters` wall-clock times of fn() (each ended by a device synchronize), after `warmup` calls; ms."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    ts.sort()
    return {'median_ms': ts[len(ts) // 2], 'min_ms': ts[0], 'p90_ms': ts[int(len(ts) * 0.9)]}


def count_launches(fn):
    from torch.profiler import ProfilerActivity, profile
    fn(); torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    names = [e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]
    kernels = [n for n in names if 'memcpy' not in n.lower() and 'memset' not in n.lower()]
    return {'kernels': len(kernels), 'copies_and_memsets': len(names) - len(kernels)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=100)
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--out', default=None)
    ap.add_argument('--no-launch-count', action='store_true')
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'ssl_cifar_bench needs the GPU'
    import ctgan_amd.ct_cifar as M
    import ctgan_amd.tflib as lib
    from ctgan_amd.engine import GraphedCifarSSLTrainer
    cfg = M.configure()
    dev = torch.device('cuda', 0)
    r = np.random.RandomState(0)
    B, n = cfg.BATCH_SIZE, 5000
    data = r.randint(0, 256, size=(n, 3, cfg.IMG, cfg.IMG)).astype(np.uint8)
    idx = [torch.from_numpy(r.randint(0, n, B).astype(np.int32)).to(dev) for _ in range(3)]
    y = torch.from_numpy(r.randint(0, 10, B).astype(np.int32)).to(dev)
    init_idx = torch.from_numpy(r.randint(0, n, cfg.INIT_ROWS).astype(np.int32)).to(dev)

    def fresh():
        lib.delete_all_params(); lib.set_seed(1)
        tr = M.CifarSSLTrainer(seed=1, data=data)
        tr.init_params(tr.gather_fixed(init_idx, cfg.IMG + 2 * cfg.PAD, (0, 0)))
        return tr
    res = {'what': 'ct_cifar classifier step / generator step / augmenting gather, B=%d' % B, 'device': torch.cuda.get_device_name(0),
           'iters': a.iters, 'warmup': a.warmup}
    try:
        res['commit'] = subprocess.run(['git', 'rev-parse', '--short', 'HEAD'], cwd=ROOT, capture_output=True, text=True).stdout.strip() or None
    except OSError:
        res['commit'] = None
    tr = fresh()
    res['gather'] = timed(lambda: tr.gather(idx[0], M.SID_AUG_LAB), a.iters, a.warmup)
    tr.d_opt.set_lr(cfg.LR); tr.g_opt.set_lr(cfg.LR)
    res['eager'] = {'d_step': timed(lambda: tr.d_body_idx(idx[0], y, idx[1]), a.iters, a.warmup),
                    'g_step': timed(lambda: tr.g_body_idx(idx[2]), a.iters, a.warmup)}
    if not a.no_launch_count:
        try:
            res['launches'] = {'d_step': count_launches(lambda: tr.d_body_idx(idx[0], y, idx[1])),
                               'g_step': count_launches(lambda: tr.g_body_idx(idx[2]))}
        except Exception as e:       # the profiler is optional: the timings stand without it
            res['launches'] = 'unavailable: %s' % type(e).__name__
    tr = fresh()
    eng = GraphedCifarSSLTrainer(tr)
    res['graphed'] = eng.graphed
    if eng.graphed:
        res['graph'] = {'d_step': timed(lambda: eng.d_step(idx[0], y, idx[1]), a.iters, a.warmup),
                        'g_step': timed(lambda: eng.g_step(idx[2]), a.iters, a.warmup)}
    else:
        res['graph_error'] = eng.graph_error
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(line + '\n')
    M.configure(); lib.delete_all_params()


if __name__ == '__main__':
    main()
