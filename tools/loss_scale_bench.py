#!/usr/bin/env python
"""What the dynamic loss scale costs a graph-replayed training iteration, on the `lsun128_f16` and `cifar_dcgan_f32` trainer
configurations of bench.py, and what its scan kernel takes by itself.

    python tools/loss_scale_bench.py --out profiles/loss_scale_bench.json [--parent-root DIR]          # iteration times
    rocprofv3 --kernel-trace --stats -d DIR -o trace -- python tools/loss_scale_bench.py --mode kernels
    python tools/loss_scale_bench.py --mode merge --db DIR/.../trace_results.db --out profiles/loss_scale_bench.json

Iteration times (`--mode iter`): a sample is a FRESH process (`--mode sample`) that builds the configuration, captures its graphs, runs
`--warmup` iterations of engine.GraphedDCGANTrainer.train_iteration and times `--iters` more, host clock around a device synchronise;
it prints the mean.  The variants - `fixed` (the fixed scale of this build: 1024 in the fp16 mode, as bench.py sets it, 1 otherwise),
`dynamic` (LossScaler at its defaults) and, with --parent-root (a checkout of the parent commit with its library built), `parent` (the
fixed scale there) - alternate sample by sample for `--reps` rounds inside the one call.  Reported per variant: the median, minimum and
maximum of its samples; per pair the difference of the medians beside the spread (max - min) of the baseline's own samples, which a
difference has to exceed to mean anything.  The dynamic samples also report the scale they ended at and the updates dropped on the way.

Kernel times: a rocprofv3 kernel trace of a run of its own (`--mode kernels`: both configurations under the dynamic scale, `--iters`
replayed iterations each), merged from the rocpd database per kernel name and grid (`--mode merge`): calls, mean and minimum duration of
nonfinite_scan_kernel, of the scaled update kernels and of step_advance_scaled_kernel."""
import argparse
import json
import os
import sqlite3
import statistics
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

CONFIGS = {'lsun128_f16': ('gan_lsun128', 'f16'), 'cifar_dcgan_f32': ('gan_cifar', None)}


def build_engine(config, variant):
    """bench.py's construction of the configuration (run_alt), with the scale of `variant`."""
    import importlib
    import numpy as np
    import torch
    import ctgan_amd.kernels as K
    import ctgan_amd.tflib as lib
    from ctgan_amd.dcgan_step import DCGANTrainer
    from ctgan_amd.engine import GraphedDCGANTrainer
    modname, dtype = CONFIGS[config]
    M = importlib.import_module('ctgan_amd.' + modname)
    lib.delete_all_params(); lib.set_seed(0); lib.set_device(None)
    M.configure()
    B = M.cfg.BATCH_SIZE
    if hasattr(M, 'build_params'):
        M.build_params('cuda')
    else:
        with torch.no_grad():
            M.Discriminator(M.Generator(2, noise=torch.zeros(2, 128, device='cuda')), u=[torch.ones(2, *s, device='cuda') for s in M.feat_shapes()])
    K.set_mma_dtype(dtype)
    if variant == 'dynamic':
        tr = DCGANTrainer(M, seed=2024, loss_scale='dynamic')
    else:
        tr = DCGANTrainer(M, seed=2024)
        if dtype == 'f16':
            tr.loss_scale = 1024.0          # (the attribute: what the parent commit has too)
    nrng = np.random.default_rng(1234)
    batches = [torch.from_numpy(nrng.integers(0, 256, (B, M.cfg.OUTPUT_DIM), dtype=np.int32)).cuda() for _ in range(8)]
    eng = GraphedDCGANTrainer(tr, (B, M.cfg.OUTPUT_DIM), torch.int32, use_graphs=True)
    return eng, tr, batches


def run_iterations(eng, batches, n, first):
    cur = [0]

    def nb():
        cur[0] = (cur[0] + 1) % len(batches)
        return batches[cur[0]]
    for it in range(first, first + n):
        eng.train_iteration(it, nb)
    return first + n


def sample(a):
    import torch
    assert torch.cuda.is_available(), 'loss_scale_bench needs the GPU'
    eng, tr, batches = build_engine(a.config, a.variant)
    it = run_iterations(eng, batches, a.warmup + 1, 0)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    run_iterations(eng, batches, a.iters, it)
    torch.cuda.synchronize()
    ms = 1e3 * (time.perf_counter() - t0) / a.iters
    rec = {'config': a.config, 'variant': a.variant, 'ms_per_iteration': ms, 'hipgraph': bool(eng.graphed), 'iteration_graph': eng.it_graph is not None,
           'graph_error': eng.graph_error, 'skipped_elements': tr.d_opt.skipped() + tr.g_opt.skipped()}
    scaler = getattr(tr, 'scaler', None)
    if scaler is not None:
        rec.update({'final_scale': scaler.scale(), 'skipped_steps': scaler.skipped_steps()})
    print('SAMPLE ' + json.dumps(rec))


def _stats(v):
    return {'median_ms': statistics.median(v), 'min_ms': min(v), 'max_ms': max(v), 'spread_ms': max(v) - min(v), 'samples': len(v)}


def iteration_times(a):
    variants = [('fixed', ROOT), ('dynamic', ROOT)] + ([('parent', os.path.abspath(a.parent_root))] if a.parent_root else [])
    out = {}
    for config in a.config_list:
        iters = a.iters if config != 'lsun128_f16' else max(a.iters // 3, 5)
        recs = {v: [] for v, _ in variants}
        for _ in range(a.reps):
            for variant, root in variants:
                env = dict(os.environ, PYTHONPATH=root)
                env.pop('CTGAN_LIB', None)
                cmd = [sys.executable, os.path.abspath(__file__), '--mode', 'sample', '--config', config, '--variant',
                       'fixed' if variant == 'parent' else variant, '--iters', str(iters), '--warmup', str(a.warmup), '--root', root]
                p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=a.sample_timeout)
                lines = [ln for ln in p.stdout.splitlines() if ln.startswith('SAMPLE ')]
                if p.returncode != 0 or not lines:
                    raise SystemExit('sample %s/%s failed (rc %d): %s' % (config, variant, p.returncode, p.stderr[-2000:]))
                recs[variant].append(json.loads(lines[-1][7:]))
        row = {'iterations_per_sample': iters, 'warmup_iterations': a.warmup + 1}
        for v in recs:
            row[v] = _stats([r['ms_per_iteration'] for r in recs[v]])
            row[v]['all_graphed'] = all(r['hipgraph'] and r['iteration_graph'] for r in recs[v])
            row[v]['skipped_elements'] = [r['skipped_elements'] for r in recs[v]]
        row['dynamic']['final_scale'] = [r['final_scale'] for r in recs['dynamic']]
        row['dynamic']['skipped_steps'] = [r['skipped_steps'] for r in recs['dynamic']]
        row['dynamic_minus_fixed_ms'] = row['dynamic']['median_ms'] - row['fixed']['median_ms']
        row['dynamic_over_fixed'] = row['dynamic']['median_ms'] / row['fixed']['median_ms']
        if 'parent' in row:
            row['fixed_minus_parent_ms'] = row['fixed']['median_ms'] - row['parent']['median_ms']
            row['fixed_over_parent'] = row['fixed']['median_ms'] / row['parent']['median_ms']
        out[config] = row
    return out


def run_kernels(a):
    import torch
    for config in a.config_list:
        eng, tr, batches = build_engine(config, 'dynamic')
        run_iterations(eng, batches, a.iters, 0)
        torch.cuda.synchronize()
        print('KERNELS %s: scale %g, dropped %d' % (config, tr.scaler.scale(), tr.scaler.skipped_steps()))
        del eng, tr


def merge_stats(a):
    cur = sqlite3.connect(a.db).cursor()
    sym_cols = [r[1] for r in cur.execute("pragma table_info(rocpd_info_kernel_symbol)")]
    namecol = 'display_name' if 'display_name' in sym_cols else ('kernel_name' if 'kernel_name' in sym_cols else sym_cols[-1])
    dcols = [r[1] for r in cur.execute("pragma table_info(rocpd_kernel_dispatch)")]
    gx = 'd.grid_size_x' if 'grid_size_x' in dcols else ('d.grid_x' if 'grid_x' in dcols else '0')
    gy = 'd.grid_size_y' if 'grid_size_y' in dcols else ('d.grid_y' if 'grid_y' in dcols else '0')
    rows = cur.execute("select s.%s, %s, %s, count(*), sum(d.end - d.start), min(d.end - d.start), max(d.end - d.start) from rocpd_kernel_dispatch d "
                       "join rocpd_info_kernel_symbol s on d.kernel_id = s.id group by s.%s, %s, %s" % (namecol, gx, gy, namecol, gx, gy)).fetchall()
    keep = ('nonfinite_scan_kernel', 'step_advance_scaled_kernel', 'adam_packed_kernel', 'adam_kernel', 'step_advance_kernel')
    res = []
    for name, x, y, calls, tot, mn, mx in rows:
        if any(k in name for k in keep):
            res.append({'kernel': name[:100], 'grid_x': x, 'grid_y': y, 'calls': calls, 'mean_us': tot / calls / 1e3, 'min_us': mn / 1e3, 'max_us': mx / 1e3})
    return sorted(res, key=lambda r: (r['kernel'], r['grid_x']))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--mode', choices=('iter', 'sample', 'kernels', 'merge'), default='iter')
    ap.add_argument('--config', action='append', default=None, choices=sorted(CONFIGS))
    ap.add_argument('--variant', choices=('fixed', 'dynamic'), default='fixed')
    ap.add_argument('--iters', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--parent-root', default=None, help='a checkout of the parent commit with its library built: adds the `parent` variant')
    ap.add_argument('--root', default=ROOT, help='(sample) the tree to import ctgan_amd from')
    ap.add_argument('--sample-timeout', type=int, default=300)
    ap.add_argument('--db', default=None)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    a.config_list = a.config or sorted(CONFIGS)
    if a.mode == 'sample':
        a.config = a.config_list[0]
        sys.path.insert(0, os.path.abspath(a.root))
        return sample(a)
    sys.path.insert(0, ROOT)
    if a.mode == 'kernels':
        return run_kernels(a)
    res = {}
    if a.out and os.path.exists(a.out):
        res = json.load(open(a.out))                         # the two runs fill one file
    if a.mode == 'merge':
        res['kernels'] = merge_stats(a)
    else:
        res.update({'what': 'dynamic loss scale: graph-replayed train_iteration, fixed scale vs dynamic scale of this build (vs the fixed scale of the '
                            'parent commit), one fresh process per sample, variants alternating; kernel times from a rocprofv3 trace of its own',
                    'reps': a.reps, 'iteration': iteration_times(a)})
    line = json.dumps(res, indent=1)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
