#!/usr/bin/env python
"""Cost of the second derivative of self-attention (ctgan_amd/attention.py: AttentionBwdFn; csrc/attention.hip: attention_bwd2;
gan_cifar_resnet.Config.ATTENTION_SECOND_ORDER), on the protocol of tools/attention_bench.py.

  core       at (n, N, dk, dv) = (64, 256, 16, 64) - the penalty's rows at the headline batch - inside a replayed graph of `--reps`
             repetitions: kernels.attention_bwd2 (both launches), and on the same device the double backward of the unfused fp32 torch
             composite softmax(q @ k^T) @ v: a graph of forward + first backward (create_graph) + second backward minus a graph of forward +
             first backward.  The fused launches are also split by the device's kernel trace (torch.profiler) of one replay.
  iteration  one graph-replayed train_iteration of the headline ResNet (B = 64, DIM 128, N_CRITIC 5) under the CT objective (objective=None):
             the parent commit (--parent-root, a built tree of it), switches off, ATTENTION_G, ATTENTION_G + ATTENTION_D +
             ATTENTION_SECOND_ORDER, and - to tell the cost of the path from the cost of the block - switches off with the hand-scheduled
             critic step disabled (CTGAN_MERGED_BWD=0: the autograd path of Trainer.d_losses, still with the shared forwards and the fused
             heads), and switches off on exactly the path a critic with the block takes (gan_cifar_resnet._critic_piecewise_linear
             answering False: Trainer.d_losses op by op, no shared forwards, no fused heads, the penalty pass's own weight gradients).
             Of the last attention configuration one iteration's kernel trace is summed: all kernels, and the attention kernels alone.

Protocol: every sample is a fresh child process; the parent process runs `--rounds` rounds, each visiting the configurations in turn, so
that drift of a shared machine falls on all alike, and reports per configuration the median over the rounds' medians with [min, max].  A
child that fails ends the run: nothing more is started on the device.  Prints one JSON line; --out writes it to a file.

    python tools/attention2_bench.py --rounds 3 --iters 30 --warmup 5 [--parent-root DIR] [--out profiles/attention2_bench.json]
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPE = (64, 256, 16, 64)


def _median(ts):
    ts = sorted(ts)
    return ts[len(ts) // 2]


def _kernel_times(prof, torch):
    per = {}
    for e in prof.events():
        if e.device_type == torch.autograd.DeviceType.CUDA and 'memcpy' not in e.name.lower() and 'memset' not in e.name.lower():
            per.setdefault(e.name, []).append(e.device_time if hasattr(e, 'device_time') else e.cuda_time)
    return per


def child_core(root, which, reps, iters):
    sys.path.insert(0, root)
    import torch
    assert torch.cuda.is_available(), 'attention2_bench needs the GPU'
    from torch.profiler import ProfilerActivity, profile
    import ctgan_amd.kernels as K
    torch.backends.cuda.matmul.allow_tf32 = False
    n, N, dk, dv = SHAPE
    g = torch.Generator().manual_seed(0)
    q, k, a, b = (torch.randn(n, N, dk, generator=g).cuda() for _ in range(4))
    v, gout, c = (torch.randn(n, N, dv, generator=g).cuda() for _ in range(3))

    if which == 'fused':
        out, lse = K.attention_fwd(q, k, v)
        delta = K.attention_bwd_delta(q, k, v, out, lse, gout)[3]
        base = None

        def full():
            return K.attention_bwd2(q, k, v, lse, delta, gout, a, b, c)
    else:
        qg, kg, vg, gg = (t.clone().requires_grad_(True) for t in (q, k, v, gout))

        def first():
            out = torch.softmax(qg @ kg.transpose(1, 2), dim=2) @ vg
            return torch.autograd.grad(out, (qg, kg, vg), gg, create_graph=True)

        def base():
            return [t.detach() for t in first()]

        def full():
            gq, gk, gv = first()
            return torch.autograd.grad((gq * a).sum() + (gk * b).sum() + (gv * c).sum(), (qg, kg, vg, gg))

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
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); gr.replay(); e1.record()
            torch.cuda.synchronize()
            ts.append(e0.elapsed_time(e1) * 1e3 / reps)
        return _median(ts)

    g_full, _ = graph_of(full)
    t_full = time_graph(g_full)
    res = {'graph_us': t_full}
    if base is not None:
        g_base, _ = graph_of(base)
        res['first_order_graph_us'] = time_graph(g_base)
    res['bwd2_us'] = t_full - res.get('first_order_graph_us', 0.0)
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        g_full.replay()
        torch.cuda.synchronize()
    per = _kernel_times(prof, torch)
    res['kernels_per_call'] = sum(len(v_) for v_ in per.values()) / float(reps)
    if which == 'fused':
        for key, frag in (('trace_q_us', 'attention_bwd2_q_kernel'), ('trace_kv_us', 'attention_bwd2_kv_kernel')):
            ts = [t for name, v_ in per.items() if frag in name for t in v_]
            res[key] = _median(ts) if ts else None
    print('RESULT ' + json.dumps(res))


def child_iteration(root, cfg_kw, iters, warmup, trace, path_only=False):
    sys.path.insert(0, root)
    import numpy as np
    import torch
    assert torch.cuda.is_available(), 'attention2_bench needs the GPU'
    import ctgan_amd.gan_cifar_resnet as R
    import ctgan_amd.tflib as lib
    from ctgan_amd.engine import GraphedTrainer
    B = 64
    lib.set_seed(1)
    R.configure(BATCH_SIZE=B, **cfg_kw)                      # (the parent commit is only ever given switches it knows)
    R.build_params()
    if path_only:            # the critic step a critic with the block takes - Trainer.d_losses op by op, no shared forwards, no fused heads,
        R._critic_piecewise_linear = lambda: False           # the penalty pass's own weight gradients - without the block in it
    tr = R.Trainer(seed=1)
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
    res = {'median_ms': _median(ts), 'min_ms': min(ts), 'graphed': bool(eng.graphed), 'cost_finite': bool(torch.isfinite(out['cost']).item())}
    if trace:
        from torch.profiler import ProfilerActivity, profile
        per = {}
        for _ in range(5):          # (a profiled pass may come back without the replayed kernels: take the fullest of a few)
            with profile(activities=[ProfilerActivity.CUDA]) as prof:
                eng.train_iteration(it, nb); it += 1
                torch.cuda.synchronize()
            seen = _kernel_times(prof, torch)
            if sum(len(v) for v in seen.values()) > sum(len(v) for v in per.values()):
                per = seen
        res['trace_all_kernels_ms'] = sum(sum(v) for v in per.values()) * 1e-3
        res['trace_attention_kernels_ms'] = sum(sum(v) for name, v in per.items() if 'attention' in name or 'attn_residual' in name) * 1e-3
        res['trace_attention_bwd2_kernels_ms'] = sum(sum(v) for name, v in per.items() if 'bwd2' in name and 'att' in name) * 1e-3
        res['trace_kernels'] = sum(len(v) for v in per.values())
        top = sorted(per.items(), key=lambda kv: -sum(kv[1]))[:12]
        res['trace_top'] = [[name[:72], len(v), round(sum(v) * 1e-3, 3)] for name, v in top]
    print('RESULT ' + json.dumps(res))


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
        return child_iteration(spec['root'], spec['cfg'], a.iters, a.warmup, spec.get('trace', False), spec.get('path_only', False))

    def run_child(spec):
        cmd = [sys.executable, os.path.abspath(__file__), '--iters', str(a.iters), '--warmup', str(a.warmup), '--reps', str(a.reps),
               '--child', json.dumps(spec)]
        env = dict(os.environ, **spec.get('env', {}))
        p = subprocess.run(cmd, cwd=spec['root'], capture_output=True, text=True, timeout=a.timeout, env=env)
        lines = [ln for ln in p.stdout.splitlines() if ln.startswith('RESULT ')]
        if p.returncode != 0 or not lines:
            sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
            raise SystemExit('attention2_bench: the child for %s ended with status %d' % (json.dumps(spec), p.returncode))
        return json.loads(lines[-1][7:])

    res = {'what': 'second derivative of self-attention: attention_bwd2 at (n, N, dk, dv) = %s inside a replayed graph against the double backward '
                   'of the unfused fp32 torch composite (us per call), and a graph-replayed CT train_iteration at B=64, DIM 128 (ms); median '
                   'over rounds of per-process medians, alternating' % (SHAPE,), 'rounds': a.rounds, 'iters': a.iters, 'warmup': a.warmup,
           'reps': a.reps}
    core_plan = [('fused', {'what': 'core', 'root': ROOT, 'which': 'fused'}), ('composite', {'what': 'core', 'root': ROOT, 'which': 'composite'})]

    def it(root, cfg, **more):
        return dict({'what': 'iteration', 'root': root, 'cfg': cfg}, **more)
    it_plan = []
    if a.parent_root:
        it_plan.append(('resnet@parent', it(os.path.abspath(a.parent_root), {})))
    it_plan += [('resnet@off', it(ROOT, {})), ('resnet@off,autograd-critic', it(ROOT, {}, env={'CTGAN_MERGED_BWD': '0'})),
                ('resnet@off,path-of-the-block', it(ROOT, {}, path_only=True, env={'CTGAN_MERGED_BWD': '0'})),
                ('resnet@G', it(ROOT, {'ATTENTION_G': True})),
                ('resnet@G+D+second', it(ROOT, {'ATTENTION_G': True, 'ATTENTION_D': True, 'ATTENTION_SECOND_ORDER': True}, trace=True))]
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
    res['fused_bwd2_over_composite'] = fu['bwd2_us']['median'] / co['bwd2_us']['median']
    res['fused_bwd2_no_slower_than_composite'] = bool(fu['bwd2_us']['median'] <= co['bwd2_us']['median'])
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
