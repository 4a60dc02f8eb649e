#!/usr/bin/env python
"""Times the temporal-ensembling CT classifier (ctgan_amd/ct_cifar_te.py) at the script's sizes (B 100, 32x32, the full widths, the
tables over N = 50,000 examples) on one GPU, and - in the SAME run, alternating with it - ct_cifar's classifier step, which it is to
be compared with: ms per classifier step graph-replayed (engine.GraphedCifarTETrainer / GraphedCifarSSLTrainer; gathers, target
reads and prediction writes are inside the graph) and eager, per generator step, per `end_epoch()` (two launches over 50,000 x 138
elements), and per launch of the fused head (kernels.te_head_fwd, and te_head_bwd) against the pair it replaces
(kernels.ssl_head_fwd + featcons_fwd, and their two backward launches).  Step figures are the median / minimum / 90th percentile of
`--iters` timed calls per round after `--warmup` untimed ones, each call ended by a device synchronize, pooled over `--rounds`
alternating rounds; a head figure is one call of `--reps` back-to-back launches ended by a synchronize, divided by reps.  Prints one
JSON line; --out writes it to a file.

    python tools/ssl_cifar_te_bench.py --iters 100 --warmup 10 [--out profiles/ssl_cifar_te_bench.json]
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


def samples(fn, iters, warmup, reps=1):
    """`iters` wall-clock times (ms per call of fn) of `reps` calls ended by one device synchronize, after `warmup` untimed calls."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        t0 = time.perf_counter()
        for _ in range(reps):
            fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3 / reps)
    return ts


def stats(ts):
    ts = sorted(ts)
    return {'median_ms': ts[len(ts) // 2], 'min_ms': ts[0], 'p90_ms': ts[int(len(ts) * 0.9)], 'n': len(ts)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=100)
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--rounds', type=int, default=2)
    ap.add_argument('--reps', type=int, default=50)
    ap.add_argument('--rows', type=int, default=50000)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'ssl_cifar_te_bench needs the GPU'
    import ctgan_amd.ct_cifar as M
    import ctgan_amd.ct_cifar_te as T
    import ctgan_amd.kernels as K
    import ctgan_amd.tflib as lib
    from ctgan_amd.engine import GraphedCifarSSLTrainer, GraphedCifarTETrainer
    dev = torch.device('cuda', 0)
    r = np.random.RandomState(0)
    B, n = 100, a.rows
    data = torch.from_numpy(r.randint(0, 256, size=(n, 3, 32, 32)).astype(np.uint8)).to(dev)
    idx = [torch.from_numpy(r.permutation(n)[:B].astype(np.int32)).to(dev) for _ in range(3)]
    y = torch.from_numpy(r.randint(0, 10, B).astype(np.int32)).to(dev)
    init_idx = torch.from_numpy(r.permutation(n)[:1000].astype(np.int32)).to(dev)

    def fresh(mod, cls):
        cfg = mod.configure()
        lib.delete_all_params(); lib.set_seed(1)
        tr = cls(seed=1, data=data)
        tr.init_params(tr.gather_fixed(init_idx[:cfg.INIT_ROWS], cfg.IMG + 2 * cfg.PAD, (0, 0)))
        tr.d_opt.set_lr(cfg.LR); tr.g_opt.set_lr(cfg.LR)
        return tr

    res = {'what': 'ct_cifar_te classifier step / generator step / end_epoch / fused head against ct_cifar, B=%d, N=%d' % (B, n),
           'device': torch.cuda.get_device_name(0), 'iters': a.iters, 'warmup': a.warmup, 'rounds': a.rounds, 'reps': a.reps}
    try:
        res['commit'] = subprocess.run(['git', 'rev-parse', '--short', 'HEAD'], cwd=ROOT, capture_output=True, text=True).stdout.strip() or None
    except OSError:
        res['commit'] = None
    pool = {}
    add = lambda k, ts: pool.setdefault(k, []).extend(ts)          # noqa: E731
    for _ in range(a.rounds):
        for name, mod, cls, eng_cls in (('te', T, T.CifarTETrainer, GraphedCifarTETrainer), ('ct_cifar', M, M.CifarSSLTrainer, GraphedCifarSSLTrainer)):
            tr = fresh(mod, cls)
            add(name + '/eager/d_step', samples(lambda: tr.d_body_idx(idx[0], y, idx[1]), a.iters, a.warmup))
            tr = fresh(mod, cls)
            eng = eng_cls(tr)
            res.setdefault('graphed', {})[name] = eng.graphed
            if eng.graphed:
                add(name + '/graph/d_step', samples(lambda: eng.d_step(idx[0], y, idx[1]), a.iters, a.warmup))
                add(name + '/graph/g_step', samples(lambda: eng.g_step(idx[2]), a.iters, a.warmup))
            else:
                res.setdefault('graph_error', {})[name] = eng.graph_error
            if name == 'te':
                add('te/end_epoch', samples(tr.end_epoch, max(a.iters // 4, 5), 2))
            del eng, tr
        # the heads on their own: the fused launch against the two it replaces, on the script's shapes
        g = torch.Generator().manual_seed(0)
        l3, f3 = torch.randn(3 * B, 10, generator=g).to(dev), torch.randn(3 * B, 128, generator=g).to(dev)
        l4, f4 = torch.randn(4 * B, 10, generator=g).to(dev), torch.randn(4 * B, 128, generator=g).to(dev)
        tab = [torch.randn(n, w, generator=g).to(dev) for w in (10, 128, 10, 128)]
        go8, go4, go2 = (torch.ones(k, device=dev) for k in (8, 4, 2))
        add('head/te_head_fwd', samples(lambda: K.te_head_fwd(l3, f3, y, idx[1], tab[0], tab[1], tab[2], tab[3], B, 1.0, 0.1, 0.0), a.iters, a.warmup, a.reps))

        def pair_fwd():
            K.ssl_head_fwd(l4, y, B, 1.0, 0.0)
            K.featcons_fwd(f4, B, l4)
        add('head/ssl_head_fwd+featcons_fwd', samples(pair_fwd, a.iters, a.warmup, a.reps))
        add('head/te_head_bwd', samples(lambda: K.te_head_bwd(l3, f3, y, idx[1], tab[0], tab[1], go8, B, 1.0, 0.1, 0.0), a.iters, a.warmup, a.reps))

        def pair_bwd():
            K.ssl_head_bwd(l4, y, go4, B, 1.0, 0.0)
            K.featcons_bwd(f4, go2, B)
        add('head/ssl_head_bwd+featcons_bwd', samples(pair_bwd, a.iters, a.warmup, a.reps))
    res['ms'] = {k: stats(v) for k, v in sorted(pool.items())}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(line + '\n')
    T.configure(); M.configure(); lib.delete_all_params()


if __name__ == '__main__':
    main()
