#!/usr/bin/env python
"""The 64x64 script's other architecture pairs (gan_64x64.Config.ARCH) at DIM 64, B 64, graph-replayed: per ARCH (one valid MODE each) the
training-iteration time with the folded BatchNorm + activation kernels of csrc/bn_act.hip and with CTGAN_BN_ACT_FUSED=0 (batch_norm plus
the separate activation launches), the two alternated in blocks inside one call; and the kernel times of the new kernels from a
rocprofv3 run of their own, with each kernel's share of its HBM bound (bytes from shapes).

    python tools/arch64_bench.py --out profiles/arch64_bench.json                     # iteration times, fused vs composed
    rocprofv3 --kernel-trace --stats -d DIR -o trace -- python tools/arch64_bench.py --mode kernels --out DIR/shapes.json
    python tools/arch64_bench.py --mode merge --db DIR/.../trace_results.db --shapes DIR/shapes.json --out profiles/arch64_bench.json

An iteration is engine.GraphedDCGANTrainer.train_iteration (generator step + the mode's critic steps), ended by a device synchronize;
each block rebuilds the parameters and captures its own graphs with the switch set, times `--iters` iterations after `--warmup`, and the
blocks alternate fused, composed, fused, ... `--reps` times.  Figures: the median over all timed iterations of a variant, the medians of
its blocks and their range (the spread a difference has to exceed)."""
import argparse
import json
import os
import sqlite3
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

ARCH_MODE = (('dcgan', 'dcgan'), ('dcgan-tanh', 'dcgan'), ('multiplicative', 'wgan'), ('wganpaper', 'wgan'), ('fc', 'lsgan'), ('dcgan-nobn', 'lsgan'))
DIM, B = 64, 64
HBM_SPEC_TBS, HBM_COPY_TBS = 8.0, 6.29          # HBM3E peak, and the measured float4 copy rate


def _median(ts):
    ts = sorted(ts)
    return ts[len(ts) // 2]


def block(arch, mode, fused, iters, warmup, batches):
    """One block: fresh parameters and graphs under the switch -> the times of `iters` iterations, ms."""
    import torch
    import ctgan_amd.functional as F
    import ctgan_amd.gan_64x64 as M
    import ctgan_amd.tflib as lib
    from ctgan_amd.dcgan_step import DCGANTrainer
    from ctgan_amd.engine import GraphedDCGANTrainer
    F.BN_ACT_FUSED = fused
    lib.delete_all_params(); lib.set_device(None); lib.set_seed(1)
    M.configure(MODE=mode, ARCH=arch, DIM=DIM, BATCH_SIZE=B)
    M.build_params('cuda')
    tr = DCGANTrainer(M, seed=1)
    eng = GraphedDCGANTrainer(tr, (B, M.cfg.OUTPUT_DIM), batches[0].dtype, use_graphs=True)
    if not eng.graphed:
        raise RuntimeError('graph capture failed: %s' % eng.graph_error)
    k = [0]

    def nb():
        k[0] += 1
        return batches[k[0] % len(batches)]
    ts = []
    for it in range(warmup + iters):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = eng.train_iteration(it, nb)
        torch.cuda.synchronize()
        if it >= warmup:
            ts.append((time.perf_counter() - t0) * 1e3)
    cost = float(out['cost'].item())
    lib.delete_all_params(); M.configure()
    return ts, cost, tr.disc_iters


def iteration_times(a):
    import torch
    import ctgan_amd.functional as F
    g = torch.Generator().manual_seed(0)
    batches = [torch.randint(0, 256, (B, 64 * 64 * 3), generator=g, dtype=torch.int32).cuda() for _ in range(4)]
    default = F.BN_ACT_FUSED
    res = {}
    try:
        for arch, mode in ARCH_MODE:
            if a.arch and arch not in a.arch:
                continue
            per = {True: [], False: []}
            costs = {}
            for _ in range(a.reps):
                for fused in (True, False):
                    ts, costs[fused], n_crit = block(arch, mode, fused, a.iters, a.warmup, batches)
                    per[fused].append(ts)
            row = {'mode': mode, 'critic_steps_per_iteration': n_crit}
            for fused, key in ((True, 'fused'), (False, 'composed')):
                meds = [_median(ts) for ts in per[fused]]
                row[key] = {'median_ms': _median([t for ts in per[fused] for t in ts]), 'block_medians_ms': meds,
                            'block_range_ms': max(meds) - min(meds), 'last_cost': costs[fused]}
            row['fused_minus_composed_ms'] = row['fused']['median_ms'] - row['composed']['median_ms']
            row['spread_ms'] = max(row['fused']['block_range_ms'], row['composed']['block_range_ms'])
            res[arch] = row
            print(arch, json.dumps(row), file=sys.stderr)
    finally:
        F.BN_ACT_FUSED = default
    return res


# the largest folded layer of each kind at DIM 64, B 64: Discriminator.BN2 on the critic's rows [real ; fake] = 128, two statistic groups.
# One shape per activation kind, so that a kernel symbol's average in the trace is the time AT that shape.
def kernel_shapes():
    return [('lrelu', 128, 2 * DIM, 16, 16, 2), ('tanh', 128, 2 * DIM, 16, 16, 2), ('gate', 128, 4 * DIM, 16, 16, 2)]


def layer_bytes(act, n, c, h, w):
    """Bytes from shapes: forward reads x and writes y (half for the gate); the backward reads gy and x in each of its two passes and
    writes gx."""
    x = 4 * n * c * h * w
    y = x // 2 if act == 'gate' else x
    return {'apply': x + y, 'bwd_partial': y + x, 'bwd_apply': y + x + x}


def run_kernels(a):
    """Each new kernel `--iters` times at kernel_shapes() plus the gate alone at Discriminator.1's [128, 2 DIM, 32, 32]; run under rocprofv3."""
    import torch
    import ctgan_amd.kernels as K
    g = torch.Generator().manual_seed(0)
    shapes = kernel_shapes()
    out = {'shapes': [], 'iters': a.iters}

    def cl(*s):
        return torch.randn(*s, generator=g).cuda().contiguous(memory_format=torch.channels_last)
    for i in range(len(shapes) + 1):
        if i == len(shapes):
            x, gy = cl(128, 2 * DIM, 32, 32), cl(128, DIM, 32, 32)
            for _ in range(a.warmup + a.iters):
                K.gate_fwd(x); K.gate_bwd(gy, x)
            nb = x.numel() * 4
            out['shapes'].append({'kernel': 'gate', 'shape': list(x.shape), 'bytes': {'gate_fwd': nb + nb // 2, 'gate_bwd': nb // 2 + 2 * nb}})
            continue
        act, n, c, h, w, groups = shapes[i]
        x, gy = cl(n, c, h, w), cl(n, c // 2 if act == 'gate' else c, h, w)
        scale, offset = (torch.rand(c, generator=g) + 0.5).cuda(), torch.randn(c, generator=g).cuda()
        for _ in range(a.warmup + a.iters):
            y, mean, rstd, x4 = K.bn_act_fwd(x, scale, offset, act, 0.2, groups)
            K.bn_act_bwd(gy, x4, mean, rstd, scale, offset, act, 0.2, groups)
        out['shapes'].append({'kernel': 'bn_act', 'act': act, 'code': K.BN_ACTS[act], 'shape': [n, c, h, w], 'groups': groups,
                              'bytes': layer_bytes(act, n, c, h, w)})
    torch.cuda.synchronize()
    return out


def merge_stats(a):
    """Kernel times (rocpd database of the rocprofv3 run) + the bytes of --shapes -> per kernel: average time, achieved bytes/s, share of
    the HBM bound (bytes / peak bandwidth over kernel time)."""
    shapes = json.load(open(a.shapes))
    db = sqlite3.connect(a.db)
    cur = db.cursor()
    sym_cols = [r[1] for r in cur.execute("pragma table_info(rocpd_info_kernel_symbol)")]
    namecol = 'display_name' if 'display_name' in sym_cols else ('kernel_name' if 'kernel_name' in sym_cols else sym_cols[-1])
    rows = cur.execute("select s.%s, count(*), sum(d.end - d.start), min(d.end - d.start) from rocpd_kernel_dispatch d join "
                       "rocpd_info_kernel_symbol s on d.kernel_id = s.id group by s.%s" % (namecol, namecol)).fetchall()
    res = []
    for sh in shapes['shapes']:
        for part, nbytes in sh['bytes'].items():
            want = part if sh['kernel'] == 'gate' else 'bn_act_%s' % part
            hits = [r for r in rows if want in r[0] and (sh['kernel'] == 'gate' or '<%d>' % sh['code'] in r[0] or 'ILi%dE' % sh['code'] in r[0])]
            for name, calls, tot, mn in hits:
                avg_us = tot / calls / 1e3
                res.append({'kernel': name[:120], 'layer': sh.get('act', 'gate'), 'shape': sh['shape'], 'calls': calls, 'avg_us': avg_us,
                            'min_us': mn / 1e3, 'bytes': nbytes, 'tb_per_s': nbytes / (avg_us * 1e-6) / 1e12,
                            'share_of_hbm_spec': (nbytes / (HBM_SPEC_TBS * 1e12)) / (avg_us * 1e-6),
                            'share_of_hbm_copy_rate': (nbytes / (HBM_COPY_TBS * 1e12)) / (avg_us * 1e-6)})
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--mode', choices=('iter', 'kernels', 'merge'), default='iter')
    ap.add_argument('--iters', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--arch', action='append', default=None)
    ap.add_argument('--db', default=None)
    ap.add_argument('--shapes', default=None)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    res = {}
    if a.out and os.path.exists(a.out) and a.mode != 'kernels':
        res = json.load(open(a.out))                         # the two runs fill one file
    if a.mode == 'merge':
        res.setdefault('kernels', []).extend(merge_stats(a))
        res['hbm_peaks_tb_per_s'] = {'spec': HBM_SPEC_TBS, 'float4_copy': HBM_COPY_TBS}
    else:
        import torch
        assert torch.cuda.is_available(), 'arch64_bench needs the GPU'
        if a.mode == 'kernels':
            res = run_kernels(a)
        else:
            res.update({'what': 'gan_64x64 ARCH pairs, DIM %d, B %d, graph-replayed training iteration: bn_act.hip fused vs CTGAN_BN_ACT_FUSED=0' % (DIM, B),
                        'device': torch.cuda.get_device_name(0), 'iters': a.iters, 'warmup': a.warmup, 'reps': a.reps})
            try:
                res['commit'] = subprocess.run(['git', 'rev-parse', '--short', 'HEAD'], cwd=ROOT, capture_output=True, text=True).stdout.strip() or None
            except OSError:
                res['commit'] = None
            res['iteration'] = iteration_times(a)
    line = json.dumps(res, indent=1)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
