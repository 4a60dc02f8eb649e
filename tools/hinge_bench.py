#!/usr/bin/env python
"""Cost of the hinge objective (objective='hinge': Trainer / DCGANTrainer, hinge_schedule.py, csrc/loss.hip ctgan_tail_hinge_heads_*), on the
protocol of tools/spectral_bench.py.

  iteration one graph-replayed train_iteration of the headline ResNet (B = 64, DIM 128, N_CRITIC 5) in five forms - the parent commit
            (--parent-root, a built tree of it), this commit with objective=None, 'hinge', None + spectral_norm, 'hinge' + spectral_norm -
            and of gan_cifar (B = 64, DIM 128) with None and with 'hinge'
  launches  the kernels of ONE eager critic step of the ResNet (after a warm-up step) under the CT objective and under 'hinge', counted on
            the device's kernel trace (torch.profiler; memcpy / memset nodes left out)

Protocol: every sample is a fresh child process that builds the model, captures the graphs, runs `--warmup` iterations and then times
`--iters` iterations one by one, each ended by a device synchronise, and reports their median.  The parent process runs `--rounds` rounds,
each visiting the configurations in turn, so that drift of a shared machine falls on all alike, and reports per configuration the median
over the rounds' medians with [min, max].  A child that fails ends the run: nothing more is started on the device.  Prints one JSON line;
--out writes it to a file.

    python tools/hinge_bench.py --rounds 3 --iters 30 --warmup 5 [--parent-root DIR] [--out profiles/hinge_bench.json]
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _median(ts):
    ts = sorted(ts)
    return ts[len(ts) // 2]


def _trainer_kw(objective, spectral):
    kw = {}
    if objective is not None:                                # (the parent commit's trainers do not know the argument)
        kw['objective'] = objective
    if spectral:
        kw['spectral_norm'] = True
    return kw


def _batches(net, B):
    import numpy as np
    import torch
    nrng = np.random.default_rng(0)
    if net == 'resnet':
        return [(torch.from_numpy(nrng.integers(0, 256, (B, 3072), dtype=np.int32)).cuda(),
                 torch.from_numpy(nrng.integers(0, 10, (B,), dtype=np.int32)).cuda()) for _ in range(10)]
    return [torch.from_numpy(nrng.integers(0, 256, (B, 3072), dtype=np.int32)).cuda() for _ in range(10)]


def child_iteration(root, net, objective, spectral, iters, warmup):
    sys.path.insert(0, root)
    import torch
    assert torch.cuda.is_available(), 'hinge_bench needs the GPU'
    import ctgan_amd.tflib as lib
    B = 64
    lib.set_seed(1)
    kw = _trainer_kw(objective, spectral)
    batches = _batches(net, B)
    if net == 'resnet':
        import ctgan_amd.gan_cifar_resnet as R
        from ctgan_amd.engine import GraphedTrainer
        R.configure(BATCH_SIZE=B)
        R.build_params()
        tr = R.Trainer(seed=1, **kw)
        eng = GraphedTrainer(tr)
    else:
        import ctgan_amd.gan_cifar as M
        from ctgan_amd import dcgan_step
        from ctgan_amd.engine import GraphedDCGANTrainer
        M.configure(BATCH_SIZE=B)
        dcgan_step.build_params(M)
        tr = dcgan_step.DCGANTrainer(M, seed=1, **kw)
        eng = GraphedDCGANTrainer(tr, tuple(batches[0].shape), batches[0].dtype)
    cur = [0]

    def nb():
        cur[0] += 1
        return batches[cur[0] % len(batches)]
    it = 0
    for _ in range(warmup + 1):
        eng.train_iteration(it, nb); it += 1
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        t0 = time.perf_counter()
        out = eng.train_iteration(it, nb); it += 1
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    res = {'median_ms': _median(ts), 'min_ms': min(ts), 'graphed': bool(eng.graphed), 'cost_finite': bool(torch.isfinite(out['cost']).item()),
           'out_keys': sorted(out)}
    print('RESULT ' + json.dumps(res))


def child_launches(root, objective):
    sys.path.insert(0, root)
    import torch
    from torch.profiler import ProfilerActivity, profile
    assert torch.cuda.is_available(), 'hinge_bench needs the GPU'
    import ctgan_amd.gan_cifar_resnet as R
    import ctgan_amd.tflib as lib
    B = 64
    lib.set_seed(1)
    R.configure(BATCH_SIZE=B)
    R.build_params()
    tr = R.Trainer(seed=1, **_trainer_kw(objective, False))
    real, labels = _batches('resnet', B)[0]
    tr.d_step(real, labels, iteration=0)
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        tr.d_step(real, labels, iteration=1)
        torch.cuda.synchronize()
    names = [e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]
    names = [n for n in names if 'memcpy' not in n.lower() and 'memset' not in n.lower()]
    print('RESULT ' + json.dumps({'kernels_per_critic_step': len(names), 'distinct_kernels': len(set(names))}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--iters', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--parent-root', default=None, help='a built tree of the parent commit: the objective=None form is also sampled from it')
    ap.add_argument('--timeout', type=int, default=240, help='seconds one child may take')
    ap.add_argument('--out', default=None)
    ap.add_argument('--child', default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        spec = json.loads(a.child)
        if spec['what'] == 'launches':
            return child_launches(spec['root'], spec['objective'])
        return child_iteration(spec['root'], spec['net'], spec['objective'], spec['spectral'], a.iters, a.warmup)

    def run_child(spec):
        cmd = [sys.executable, os.path.abspath(__file__), '--iters', str(a.iters), '--warmup', str(a.warmup), '--child', json.dumps(spec)]
        p = subprocess.run(cmd, cwd=spec['root'], capture_output=True, text=True, timeout=a.timeout)
        lines = [ln for ln in p.stdout.splitlines() if ln.startswith('RESULT ')]
        if p.returncode != 0 or not lines:
            sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
            raise SystemExit('hinge_bench: the child for %s ended with status %d' % (json.dumps(spec), p.returncode))
        return json.loads(lines[-1][7:])
    res = {'what': "hinge objective: graph-replayed train_iteration at B=64, DIM 128 (median over rounds of per-process medians, alternating) "
                   "and the kernels of one eager ResNet critic step, CT against hinge", 'rounds': a.rounds, 'iters': a.iters, 'warmup': a.warmup}
    res['launches'] = {name: run_child({'what': 'launches', 'root': ROOT, 'objective': obj}) for name, obj in (('ct', None), ('hinge', 'hinge'))}
    sys.stderr.write(json.dumps(res['launches']) + '\n')

    def it(root, net, objective, spectral=False):
        return {'what': 'iteration', 'root': root, 'net': net, 'objective': objective, 'spectral': spectral}
    plan = []
    if a.parent_root:
        plan.append(('resnet@parent', it(os.path.abspath(a.parent_root), 'resnet', None)))
    plan += [('resnet@none', it(ROOT, 'resnet', None)), ('resnet@hinge', it(ROOT, 'resnet', 'hinge')),
             ('resnet@none+sn', it(ROOT, 'resnet', None, True)), ('resnet@hinge+sn', it(ROOT, 'resnet', 'hinge', True)),
             ('gan_cifar@none', it(ROOT, 'gan_cifar', None)), ('gan_cifar@hinge', it(ROOT, 'gan_cifar', 'hinge'))]
    samples, meta = {k: [] for k, _ in plan}, {}
    for rnd in range(a.rounds):
        for key, spec in plan:
            r = run_child(spec)
            samples[key].append(r['median_ms'])
            meta[key] = {k: v for k, v in r.items() if k not in ('median_ms', 'min_ms')}
            sys.stderr.write('round %d %s: %.3f ms\n' % (rnd, key, r['median_ms']))
    res['train_iteration'] = {k: dict(median_ms=_median(v), min_ms=min(v), max_ms=max(v), samples_ms=v, **meta[k]) for k, v in samples.items()}
    if a.parent_root:
        p, n = res['train_iteration']['resnet@parent'], res['train_iteration']['resnet@none']
        res['none_inside_parent_spread'] = bool(p['min_ms'] <= n['median_ms'] <= p['max_ms'])
    try:
        import torch
        res['device'] = torch.cuda.get_device_name(0)
    except (ImportError, RuntimeError):
        pass
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
