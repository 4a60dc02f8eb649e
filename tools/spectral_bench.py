#!/usr/bin/env python
"""Cost of spectral normalisation (spectral_norm=, optim.SpectralNorm, csrc/spectral.hip), on the protocol of tools/projection_bench.py.

  kernels   the `normalise` (3 launches) and `grad` (2 launches) groups, graph-replayed, at the job tables of the CIFAR-10 ResNet critic
            (DIM_D 128) and of the gan_lsun128 critic at their default widths: microseconds per call, and the bytes the group has to move
            at least (normalise: theta read and theta_bar written once = 8 bytes per bucket element; grad: the gradient and theta_bar read
            for the dot, the gradient read and written by the apply = 16 bytes per normalised element) over that time
  iteration one graph-replayed train_iteration of the headline ResNet (B = 64, DIM 128) and of gan_cifar (B = 64, DIM 128) in three forms:
            the parent commit (--parent-root, a built tree of it), this commit off, this commit on

Protocol: every sample is a fresh child process that builds the model, captures the graphs, runs `--warmup` iterations and then times
`--iters` iterations one by one, each ended by a device synchronise, and reports their median.  The parent process runs `--rounds` rounds,
each visiting the configurations in turn, so that drift of a shared machine falls on all alike, and reports per configuration the median
over the rounds' medians with [min, max].  A child that fails ends the run: nothing more is started on the device.  Prints one JSON line;
--out writes it to a file.

    python tools/spectral_bench.py --rounds 3 --iters 30 --warmup 5 [--parent-root DIR] [--out profiles/spectral_bench.json]
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


def child_kernels(root, net, reps=20, samples=15):
    sys.path.insert(0, root)
    import torch
    assert torch.cuda.is_available(), 'spectral_bench needs the GPU'
    import ctgan_amd.tflib as lib
    from ctgan_amd.optim import FlatAdam, SpectralNorm
    lib.set_seed(1)
    if net == 'resnet':
        import ctgan_amd.gan_cifar_resnet as M
        M.configure()
        M.build_params()
        named = lib.named_params_with_name('Discriminator.', trainable_only=True)
    else:
        import ctgan_amd.gan_lsun128 as M
        from ctgan_amd import dcgan_step
        M.configure(BATCH_SIZE=2)
        dcgan_step.build_params(M)
        named = lib.named_params_with_name('Discriminator', trainable_only=True)
    opt = FlatAdam(named, 0.0, 0.9)
    sn = SpectralNorm(named, opt)
    opt.grad.normal_()
    gsave = opt.grad.clone()
    out = {'net': net, 'jobs': sn.table.njobs, 'row_slices': sn.table.nslices, 'bucket_elements': sn.table.total,
           'normalised_elements': sum(k * n for _, k, n in sn.table.jobs), 'widest_n': max(n for _, _, n in sn.table.jobs),
           'scratch_bytes': 4 * sn.table.scratch_floats}
    for name, fn, nbytes in (('normalise', sn.normalise, 8 * out['bucket_elements']), ('grad', lambda: sn.grad_(opt.grad), 16 * out['normalised_elements'])):
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):
            fn()
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            for _ in range(reps):
                fn()
        ts = []
        for _ in range(samples + 2):
            opt.grad.copy_(gsave)                 # (grad is in place: each replay starts from finite values)
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(); g.replay(); b.record()
            torch.cuda.synchronize()
            ts.append(a.elapsed_time(b) * 1e3 / reps)
        ts = sorted(ts[2:])
        out[name] = {'us_per_call': _median(ts), 'min_us': ts[0], 'max_us': ts[-1], 'bytes_at_least': nbytes,
                     'gb_per_s': nbytes / (_median(ts) * 1e-6) / 1e9}
    print('RESULT ' + json.dumps(out))


def child_iteration(root, net, on, iters, warmup):
    sys.path.insert(0, root)
    import numpy as np
    import torch
    assert torch.cuda.is_available(), 'spectral_bench needs the GPU'
    import ctgan_amd.tflib as lib
    B = 64
    lib.set_seed(1)
    kw = {'spectral_norm': True} if on else {}           # (the parent commit's trainers do not know the argument)
    nrng = np.random.default_rng(0)
    if net == 'resnet':
        import ctgan_amd.gan_cifar_resnet as R
        from ctgan_amd.engine import GraphedTrainer
        R.configure(BATCH_SIZE=B)
        R.build_params()
        tr = R.Trainer(seed=1, **kw)
        eng = GraphedTrainer(tr)
        batches = [(torch.from_numpy(nrng.integers(0, 256, (B, 3072), dtype=np.int32)).cuda(),
                    torch.from_numpy(nrng.integers(0, 10, (B,), dtype=np.int32)).cuda()) for _ in range(10)]
    else:
        import ctgan_amd.gan_cifar as M
        from ctgan_amd import dcgan_step
        from ctgan_amd.engine import GraphedDCGANTrainer
        M.configure(BATCH_SIZE=B)
        dcgan_step.build_params(M)
        tr = dcgan_step.DCGANTrainer(M, seed=1, **kw)
        batches = [torch.from_numpy(nrng.integers(0, 256, (B, 3072), dtype=np.int32)).cuda() for _ in range(10)]
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
    res = {'median_ms': _median(ts), 'min_ms': min(ts), 'graphed': bool(eng.graphed), 'cost_finite': bool(torch.isfinite(out['cost']).item())}
    if on:
        sig = tr.spectral.sigmas().values()
        res.update(sn_sigma_max=max(sig), sn_sigma_min=min(sig))
    print('RESULT ' + json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--iters', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--parent-root', default=None, help='a built tree of the parent commit: the off form is also sampled from it')
    ap.add_argument('--timeout', type=int, default=240, help='seconds one child may take')
    ap.add_argument('--out', default=None)
    ap.add_argument('--child', default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        spec = json.loads(a.child)
        if spec['what'] == 'kernels':
            return child_kernels(spec['root'], spec['net'])
        return child_iteration(spec['root'], spec['net'], spec['on'], a.iters, a.warmup)

    def run_child(spec):
        cmd = [sys.executable, os.path.abspath(__file__), '--iters', str(a.iters), '--warmup', str(a.warmup), '--child', json.dumps(spec)]
        p = subprocess.run(cmd, cwd=spec['root'], capture_output=True, text=True, timeout=a.timeout)
        lines = [ln for ln in p.stdout.splitlines() if ln.startswith('RESULT ')]
        if p.returncode != 0 or not lines:
            sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
            raise SystemExit('spectral_bench: the child for %s ended with status %d' % (json.dumps(spec), p.returncode))
        return json.loads(lines[-1][7:])
    res = {'what': 'spectral normalisation: launch groups graph-replayed (us per call), and graph-replayed train_iteration at B=64, DIM 128 '
                   '(median over rounds of per-process medians, alternating)', 'rounds': a.rounds, 'iters': a.iters, 'warmup': a.warmup}
    res['kernels'] = {net: run_child({'what': 'kernels', 'root': ROOT, 'net': net}) for net in ('resnet', 'lsun128')}
    sys.stderr.write(json.dumps(res['kernels']) + '\n')
    plan = []
    for net in ('resnet', 'gan_cifar'):
        if a.parent_root:
            plan.append((net + '@parent', {'what': 'iteration', 'root': os.path.abspath(a.parent_root), 'net': net, 'on': False}))
        plan.append((net + '@off', {'what': 'iteration', 'root': ROOT, 'net': net, 'on': False}))
        plan.append((net + '@on', {'what': 'iteration', 'root': ROOT, 'net': net, 'on': True}))
    samples, meta = {k: [] for k, _ in plan}, {}
    for rnd in range(a.rounds):
        for key, spec in plan:
            r = run_child(spec)
            samples[key].append(r['median_ms'])
            meta[key] = {k: v for k, v in r.items() if k not in ('median_ms', 'min_ms')}
            sys.stderr.write('round %d %s: %.3f ms\n' % (rnd, key, r['median_ms']))
    res['train_iteration'] = {k: dict(median_ms=_median(v), min_ms=min(v), max_ms=max(v), samples_ms=v, **meta[k]) for k, v in samples.items()}
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
