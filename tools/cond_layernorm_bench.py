#!/usr/bin/env python
"""Times the label-conditioned Layernorm kernels (csrc/layernorm.hip: ctgan_layernorm_cond_{fwd,bwd,bwd2}) beside the unconditional ones
at the critic's two sites, [128,128,16,16] and [128,128,8,8] - forward, backward (with the parameter gradients) and double backward -
and one graph-replayed critic step (engine.GraphedTrainer) of the "vanilla" conditional ResNet configuration (CONDITIONAL, not ACGAN,
NORMALIZATION_D) at B = 64 beside the same step with ACGAN=True, NORMALIZATION_D=True.  Every figure is the median of `--iters` timed
calls after `--warmup` untimed ones, each call ended by a device synchronize.  Prints one JSON line; --out writes it to a file.

    python tools/cond_layernorm_bench.py --iters 50 --warmup 10 [--out profiles/cond_layernorm_bench.json]
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


def kernels_at(shape, iters, warmup):
    import ctgan_amd.kernels as K
    g = torch.Generator().manual_seed(0)
    N, C = shape[0], shape[1]

    def cl(t):
        return t.cuda().contiguous(memory_format=torch.channels_last)
    x, gy, u = (cl(torch.randn(*shape, generator=g)) for _ in range(3))
    scale_t = (torch.rand(10, C, generator=g) + 0.5).cuda()
    offset_t = torch.randn(10, C, generator=g).cuda()
    scale, offset = scale_t[0].contiguous(), offset_t[0].contiguous()
    labels = torch.randint(0, 10, (N,), generator=g, dtype=torch.int32).cuda()
    y, mean, rstd = K.layernorm_fwd(x, scale, offset, 1e-5, True)
    yc, meanc, rstdc = K.layernorm_cond_fwd(x, scale_t, offset_t, labels, 1e-5, True)
    return {
        'fwd': {'plain': timed(lambda: K.layernorm_fwd(x, scale, offset, 1e-5, True), iters, warmup),
                'cond': timed(lambda: K.layernorm_cond_fwd(x, scale_t, offset_t, labels, 1e-5, True), iters, warmup)},
        'bwd': {'plain': timed(lambda: K.layernorm_bwd(gy, x, scale, mean, rstd, True, y), iters, warmup),
                'cond': timed(lambda: K.layernorm_cond_bwd(gy, x, scale_t, labels, meanc, rstdc, True, yc), iters, warmup)},
        'bwd2': {'plain': timed(lambda: K.layernorm_bwd2(u, gy, x, scale, mean, rstd, True, True, True, y), iters, warmup),
                 'cond': timed(lambda: K.layernorm_cond_bwd2(u, gy, x, scale_t, labels, meanc, rstdc, True, True, True, yc), iters, warmup)},
    }


def critic_step(iters, warmup, **kw):
    import ctgan_amd.gan_cifar_resnet as R
    import ctgan_amd.tflib as lib
    from ctgan_amd.engine import GraphedTrainer
    B = 64
    lib.delete_all_params(); lib.set_device(None); lib.set_seed(1)
    R.configure(BATCH_SIZE=B, NORMALIZATION_D=True, **kw)
    R.build_params()
    tr = R.Trainer(seed=1)
    eng = GraphedTrainer(tr)
    g = torch.Generator().manual_seed(0)
    real = torch.randint(0, 256, (B, 3072), generator=g, dtype=torch.int32).cuda()
    labels = torch.randint(0, 10, (B,), generator=g, dtype=torch.int32).cuda()
    fake = tr.generate_fakes(labels)[0].clone()
    res = {'graphed': eng.graphed, 'd_step': timed(lambda: eng.d_step(real, labels, 1, fake=fake), iters, warmup)}
    if not eng.graphed:
        res['graph_error'] = eng.graph_error
    lib.delete_all_params(); R.configure()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=50)
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'cond_layernorm_bench needs the GPU'
    res = {'what': 'label-conditioned vs unconditional Layernorm kernels; graph-replayed critic step, B=64, DIM 128',
           'device': torch.cuda.get_device_name(0), 'iters': a.iters, 'warmup': a.warmup}
    try:
        res['commit'] = subprocess.run(['git', 'rev-parse', '--short', 'HEAD'], cwd=ROOT, capture_output=True, text=True).stdout.strip() or None
    except OSError:
        res['commit'] = None
    res['kernels'] = {'x'.join(map(str, s)): kernels_at(s, a.iters, a.warmup) for s in ((128, 128, 16, 16), (128, 128, 8, 8))}
    res['critic_step'] = {'vanilla_conditional': critic_step(a.iters, a.warmup, CONDITIONAL=True, ACGAN=False),
                          'acgan_layernorm': critic_step(a.iters, a.warmup, CONDITIONAL=True, ACGAN=True)}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
