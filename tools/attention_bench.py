#!/usr/bin/env python
"""Cost of the self-attention block (ctgan_amd/attention.py, csrc/attention.hip, gan_cifar_resnet.Config.ATTENTION_G / ATTENTION_D), on the
protocol of tools/hinge_bench.py.

  core       at (n, N, dk, dv) = (128, 256, 16, 64), inside a replayed graph of `--reps` repetitions: the forward launch and the backward
             (both launches) of the fused kernels, and on the same device the same quantities of the unfused fp32 torch composite
             softmax(q @ k^T) @ v and its autograd backward - the yardstick for keeping a hand-written kernel at all.  forward = a graph of
             forwards; backward = a graph of forward + backward minus that.  For the fused kernels the two backward launches are also
             split by the device's kernel trace (torch.profiler) of one replay.
  iteration  one graph-replayed train_iteration of the headline ResNet (B = 64, DIM 128, N_CRITIC 5) under objective='hinge': the parent
             commit (--parent-root, a built tree of it), switches off, ATTENTION_G, ATTENTION_G + ATTENTION_D.

Protocol: every sample is a fresh child process; the parent process runs `--rounds` rounds, each visiting the configurations in turn, so
that drift of a shared machine falls on all alike, and reports per configuration the median over the rounds' medians with [min, max].  A
child that fails ends the run: nothing more is started on the device.  Prints one JSON line; --out writes it to a file.

    python tools/attention_bench.py --rounds 3 --iters 30 --warmup 5 [--parent-root DIR] [--out profiles/attention_bench.json]
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPE = (128, 256, 16, 64)


def _median(ts):
    ts = sorted(ts)
    return ts[len(ts) // 2]


def child_core(root, which, reps, iters):
    sys.path.insert(0, root)
    import torch
    assert torch.cuda.is_available(), 'attention_bench needs the GPU'
    from torch.profiler import ProfilerActivity, profile
    import ctgan_amd.kernels as K
    torch.backends.cuda.matmul.allow_tf32 = False
    n, N, dk, dv = SHAPE
    g = torch.Generator().manual_seed(0)
    q, k = (torch.randn(n, N, dk, generator=g).cuda() for _ in range(2))
    v, gout = (torch.randn(n, N, dv, generator=g).cuda() for _ in range(2))

    if which == 'fused':
        def fwd():
            return K.attention_fwd(q, k, v)

        def both():
            out, lse = K.attention_fwd(q, k, v)
            return K.attention_bwd(q, k, v, out, lse, gout)
    else:
        qg, kg, vg = (t.clone().requires_grad_(True) for t in (q, k, v))

        def fwd():
            with torch.no_grad():
                return torch.softmax(q @ k.transpose(1, 2), dim=2) @ v

        def both():
            out = torch.softmax(qg @ kg.transpose(1, 2), dim=2) @ vg
            return torch.autograd.grad(out, (qg, kg, vg), gout)

    def graph_of(fn):
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(3):
                fn()
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gr):
            for _ in range(reps):
                keep = fn()
        return gr, keep

    def time_graph(gr):
        for _ in range(3):
            gr.replay()
        torch.cuda.synchronize()
        ts = []
        for _ in range(iters):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(); gr.replay(); b.record()
            torch.cuda.synchronize()
            ts.append(a.elapsed_time(b) * 1e3 / reps)
        return _median(ts)

    g_f, _ = graph_of(fwd)
    t_f = time_graph(g_f)
    g_b, _ = graph_of(both)
    t_b = time_graph(g_b)
    res = {'fwd_us': t_f, 'fwd_bwd_us': t_b, 'bwd_us': t_b - t_f}
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        g_b.replay()
        torch.cuda.synchronize()
    per = {}
    for e in prof.events():
        if e.device_type == torch.autograd.DeviceType.CUDA and 'memcpy' not in e.name.lower() and 'memset' not in e.name.lower():
            per.setdefault(e.name, []).append(e.device_time if hasattr(e, 'device_time') else e.cuda_time)
    res['kernels_per_fwd_bwd'] = sum(len(v_) for v_ in per.values()) / float(reps)
    if which == 'fused':
        for key, frag in (('trace_fwd_us', 'attention_fwd_kernel'), ('trace_bwd_q_us', 'attention_bwd_q_kernel'), ('trace_bwd_kv_us', 'attention_bwd_kv_kernel')):
            ts = [t for name, v_ in per.items() if frag in name for t in v_]
            res[key] = _median(ts) if ts else None
    print('RESULT ' + json.dumps(res))


def child_iteration(root, att_g, att_d, iters, warmup):
    sys.path.insert(0, root)
    import numpy as np
    import torch
    assert torch.cuda.is_available(), 'attention_bench needs the GPU'
    import ctgan_amd.gan_cifar_resnet as R
    import ctgan_amd.tflib as lib
    from ctgan_amd.engine import GraphedTrainer
    B = 64
    lib.set_seed(1)
    kw = {}
    if att_g:                                                # (the parent commit does not know the switches)
        kw['ATTENTION_G'] = True
    if att_d:
        kw['ATTENTION_D'] = True
    R.configure(BATCH_SIZE=B, **kw)
    R.build_params()
    tr = R.Trainer(seed=1, objective='hinge')
    eng = GraphedTrainer(tr)
    nrng = np.random.default_rng(0)
    batches = [(torch.from_numpy(nrng.integers(0, 256, (B, 3072), dtype=np.int32)).cuda(),
                torch.from_numpy(nrng.integers(0, 10, (B,), dtype=np.int32)).cuda()) for _ in range(10)]
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
    print('RESULT ' + json.dumps({'median_ms': _median(ts), 'min_ms': min(ts), 'graphed': bool(eng.graphed),
                                  'cost_finite': bool(torch.isfinite(out['cost']).item())}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--iters', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--reps', type=int, default=20, help='repetitions of the core inside one graph')
    ap.add_argument('--parent-root', default=None, help='a built tree of the parent commit: its train_iteration is sampled too')
    ap.add_argument('--timeout', type=int, default=240, help='seconds one child may take')
    ap.add_argument('--out', default=None)
    ap.add_argument('--child', default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        spec = json.loads(a.child)
        if spec['what'] == 'core':
            return child_core(spec['root'], spec['which'], a.reps, a.iters)
        return child_iteration(spec['root'], spec['att_g'], spec['att_d'], a.iters, a.warmup)

    def run_child(spec):
        cmd = [sys.executable, os.path.abspath(__file__), '--iters', str(a.iters), '--warmup', str(a.warmup), '--reps', str(a.reps),
               '--child', json.dumps(spec)]
        p = subprocess.run(cmd, cwd=spec['root'], capture_output=True, text=True, timeout=a.timeout)
        lines = [ln for ln in p.stdout.splitlines() if ln.startswith('RESULT ')]
        if p.returncode != 0 or not lines:
            sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
            raise SystemExit('attention_bench: the child for %s ended with status %d' % (json.dumps(spec), p.returncode))
        return json.loads(lines[-1][7:])

    res = {'what': 'self-attention: the core at (n, N, dk, dv) = %s inside a replayed graph, fused kernels against the unfused fp32 torch composite '
                   '(us per call), and a graph-replayed hinge train_iteration at B=64, DIM 128 (ms); median over rounds of per-process medians, '
                   'alternating' % (SHAPE,), 'rounds': a.rounds, 'iters': a.iters, 'warmup': a.warmup, 'reps': a.reps}
    core_plan = [('fused', {'what': 'core', 'root': ROOT, 'which': 'fused'}), ('composite', {'what': 'core', 'root': ROOT, 'which': 'composite'})]

    def it(root, att_g, att_d):
        return {'what': 'iteration', 'root': root, 'att_g': att_g, 'att_d': att_d}
    it_plan = []
    if a.parent_root:
        it_plan.append(('resnet@parent', it(os.path.abspath(a.parent_root), False, False)))
    it_plan += [('resnet@off', it(ROOT, False, False)), ('resnet@G', it(ROOT, True, False)), ('resnet@G+D', it(ROOT, True, True))]
    core = {k: {} for k, _ in core_plan}
    samples = {k: [] for k, _ in it_plan}
    meta = {}
    for rnd in range(a.rounds):
        for key, spec in core_plan:
            r = run_child(spec)
            for f, val in r.items():
                core[key].setdefault(f, []).append(val)
            sys.stderr.write('round %d core %s: %s\n' % (rnd, key, json.dumps(r)))
        for key, spec in it_plan:
            r = run_child(spec)
            samples[key].append(r['median_ms'])
            meta[key] = {k: v for k, v in r.items() if k not in ('median_ms', 'min_ms')}
            sys.stderr.write('round %d %s: %.3f ms\n' % (rnd, key, r['median_ms']))
    res['core'] = {k: {f: (dict(median=_median(v), min=min(v), max=max(v), samples=v) if all(x is not None for x in v) else None)
                       for f, v in fields.items()} for k, fields in core.items()}
    fu, co = res['core']['fused'], res['core']['composite']
    res['fused_forward_no_slower_than_composite'] = bool(fu['fwd_us']['median'] <= co['fwd_us']['median'])
    res['fused_backward_no_slower_than_composite'] = bool(fu['bwd_us']['median'] <= co['bwd_us']['median'])
    res['train_iteration'] = {k: dict(median_ms=_median(v), min_ms=min(v), max_ms=max(v), samples_ms=v, **meta[k]) for k, v in samples.items()}
    if a.parent_root:
        p, n = res['train_iteration']['resnet@parent'], res['train_iteration']['resnet@off']
        res['off_samples_inside_parent_spread'] = bool(all(p['min_ms'] <= s <= p['max_ms'] for s in n['samples_ms']))
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
