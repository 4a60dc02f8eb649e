#!/usr/bin/env python
"""Times one graph-replayed training iteration (engine.GraphedTrainer.train_iteration: generator step, the fake batches, N_CRITIC critic steps
and both updates) of the CIFAR-10 ResNet at B = 64, DIM 128 in four configurations:

  a  the default (CONDITIONAL, ACGAN)                                - the no-regression gate; with --parent-root also from that other tree
  b  CONDITIONAL, not ACGAN, no normalisation in D                   - the fast piecewise-linear critic, effectively unconditional
  c  b + PROJECTION                                                  - the projection head
  d  CONDITIONAL, not ACGAN, NORMALIZATION_D                         - the label-conditioned Layernorm critic the projection is meant to replace

Protocol: every sample is a fresh child process (the configuration and the parameter registry are process-wide) that builds the model, captures
the graphs, runs `--warmup` iterations and then times `--iters` iterations one by one, each ended by a device synchronise; it reports their median.
The parent runs `--rounds` rounds, each visiting the configurations in turn (a, a-parent, b, c, d, a, ...), so that drift of the shared machine
falls on all of them alike, and reports per configuration the median over the rounds' medians and their spread (min, max).  After the timing, one
more child per configuration counts the kernel launches of one EAGER iteration with the torch profiler (the launches the graphs capture; a
profile of a replay does not list a graph's kernels reliably).  Prints one JSON line; --out writes it to a file.

    python tools/projection_bench.py --rounds 5 --iters 30 --warmup 5 [--parent-root DIR] [--out profiles/projection_bench.json]
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CONFIGS = {
    'a_acgan_default': {},
    'b_unconditional_head': dict(CONDITIONAL=True, ACGAN=False, NORMALIZATION_D=False),
    'c_projected_head': dict(CONDITIONAL=True, ACGAN=False, NORMALIZATION_D=False, PROJECTION=True),
    'd_layernorm_conditional': dict(CONDITIONAL=True, ACGAN=False, NORMALIZATION_D=True),
}


def child(root, kw, iters, warmup, count):
    """One sample: the median time of a graph-replayed iteration in configuration `kw`, from the tree at `root` - or (count) the kernel
    launches of one eager iteration."""
    sys.path.insert(0, root)
    import numpy as np
    import torch
    assert torch.cuda.is_available(), 'projection_bench needs the GPU'
    import ctgan_amd.gan_cifar_resnet as R
    import ctgan_amd.tflib as lib
    from ctgan_amd.engine import GraphedTrainer
    B = 64
    lib.set_seed(1)
    R.configure(BATCH_SIZE=B, **kw)
    R.build_params()
    tr = R.Trainer(seed=1)
    eng = GraphedTrainer(tr, use_graphs=not count)
    nrng = np.random.default_rng(0)
    batches = [(torch.from_numpy(nrng.integers(0, 256, (B, 3072), dtype=np.int32)).cuda(),
                torch.from_numpy(nrng.integers(0, 10, (B,), dtype=np.int32)).cuda()) for _ in range(10)]
    cur = [0]

    def nb():
        cur[0] += 1
        return batches[cur[0] % len(batches)]
    it = 0
    if count:
        from torch.profiler import ProfilerActivity, profile
        for _ in range(3):
            eng.train_iteration(it, nb); it += 1
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            eng.train_iteration(it, nb)
            torch.cuda.synchronize()
        names = [e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]
        kernels = [n for n in names if 'memcpy' not in n.lower() and 'memset' not in n.lower()]
        heads = {}
        for n in kernels:
            if 'heads' in n or 'gp_head' in n:
                key = n.split('(anonymous namespace)::')[1].split('(')[0]
                heads[key] = heads.get(key, 0) + 1
        print('RESULT ' + json.dumps({'kernels': len(kernels), 'copies_and_memsets': len(names) - len(kernels), 'head_kernels': heads}))
        return
    for _ in range(warmup + 1):                  # iteration 0 has no generator step and captures the per-step graphs
        eng.train_iteration(it, nb); it += 1
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        t0 = time.perf_counter()
        eng.train_iteration(it, nb); it += 1
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    ts.sort()
    res = {'median_ms': ts[len(ts) // 2], 'min_ms': ts[0], 'p90_ms': ts[int(len(ts) * 0.9)], 'graphed': bool(eng.graphed),
           'iteration_graph': eng.it_graph is not None, 'critic_parameters': sum(p.numel() for p in tr.d_params)}
    print('RESULT ' + json.dumps(res))


def spread(vals):
    s = sorted(vals)
    return {'median_ms': s[len(s) // 2], 'min_ms': s[0], 'max_ms': s[-1], 'samples_ms': vals}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--iters', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--parent-root', default=None, help='a built tree of the parent commit: configuration a is also sampled from it')
    ap.add_argument('--timeout', type=int, default=240, help='seconds one child may take')
    ap.add_argument('--out', default=None)
    ap.add_argument('--child', default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        spec = json.loads(a.child)
        return child(spec['root'], spec['kw'], a.iters, a.warmup, spec['count'])
    plan = [('a_acgan_default', ROOT)]
    if a.parent_root:
        plan.append(('a_acgan_default@parent', os.path.abspath(a.parent_root)))
    plan += [(k, ROOT) for k in CONFIGS if k != 'a_acgan_default']
    samples = {k: [] for k, _ in plan}
    meta = {}

    def run_child(key, root, count):
        spec = {'root': root, 'kw': CONFIGS[key.split('@')[0]], 'count': count}
        cmd = [sys.executable, os.path.abspath(__file__), '--iters', str(a.iters), '--warmup', str(a.warmup), '--child', json.dumps(spec)]
        p = subprocess.run(cmd, cwd=root, capture_output=True, text=True, timeout=a.timeout)
        lines = [ln for ln in p.stdout.splitlines() if ln.startswith('RESULT ')]
        if p.returncode != 0 or not lines:       # a child that failed ends the run: nothing more is started on the device
            sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
            raise SystemExit('projection_bench: the child for %s ended with status %d' % (key, p.returncode))
        return json.loads(lines[-1][7:])
    for rnd in range(a.rounds):
        for key, root in plan:
            r = run_child(key, root, False)
            samples[key].append(r['median_ms'])
            meta.setdefault(key, {k: v for k, v in r.items() if k not in ('median_ms', 'min_ms', 'p90_ms')})
            sys.stderr.write('round %d %s: %.3f ms\n' % (rnd, key, r['median_ms']))
    for key, root in plan:
        meta[key]['launches_per_eager_iteration'] = run_child(key, root, True)
        sys.stderr.write('%s: %s\n' % (key, json.dumps(meta[key]['launches_per_eager_iteration'])))
    res = {'what': 'graph-replayed train_iteration, CIFAR-10 ResNet, B=64, DIM 128: median over rounds of per-process medians, alternating',
           'rounds': a.rounds, 'iters': a.iters, 'warmup': a.warmup}
    try:
        import torch
        res['device'] = torch.cuda.get_device_name(0)
        res['commit'] = subprocess.run(['git', 'rev-parse', '--short', 'HEAD'], cwd=ROOT, capture_output=True, text=True).stdout.strip() or None
    except (OSError, RuntimeError):
        pass
    res['configurations'] = {k: dict(spread(v), **meta[k]) for k, v in samples.items()}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
