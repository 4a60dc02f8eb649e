#!/usr/bin/env python
"""Times what the generator's weight average adds to an optimizer update launch, on one GPU, in one process: the four update
launches - adam_step, adam_step_packed, rmsprop_step, rmsprop_step_packed - without and with the average, on the two flat buckets of the
headline ResNet (its generator's and its critic's parameter tensors as optim.FlatAdam lays them out; the critic's is there as a second
size - the trainers never average it), and kernels.exchange_ on the generator's bucket.

A sample is `--launches` back-to-back launches of one form between two device events; the forms alternate sample by sample for `--rounds`
rounds after `--warmup` untimed ones, and a figure is the median (with min / max) of a form's samples.  Beside each pair: the bytes per
element each form moves (counted from the kernels' loads and stores), their ratio, the time ratio, and the spread of the plain form's
samples to judge the difference by.  The learning rate is 0 (the values stay put; the traffic is that of any step) and the gradients are
random.  Prints one JSON line; --out writes it to a file.

    python tools/avg_bench.py [--out profiles/avg_bench.json]
"""
import argparse
import json
import os
import statistics
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402

# bytes per element: loads + stores of the kernel bodies in csrc/optim_rng.hip (the packed forms also read the source and write the bucket)
BYTES = {'adam_step': 28, 'adam_step_packed': 32, 'rmsprop_step': 20, 'rmsprop_step_packed': 24}
AVG_BYTES = 8          # one more 4-byte load and store per element
EXCHANGE_BYTES = 16


def _stats(us):
    return {'median_us': statistics.median(us), 'min_us': min(us), 'max_us': max(us), 'samples': len(us)}


def _timed(fn, launches):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(launches):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / launches


def bucket_forms(sizes):
    """-> {form: {False: launch without the average, True: with it}} on buffers laid out like a FlatAdam over tensors of `sizes`."""
    import ctgan_amd.kernels as K
    n = sum(sizes)
    offs = [sum(sizes[:i]) for i in range(len(sizes))]
    new = lambda fill=None: torch.randn(n, device='cuda') * 0.02 if fill is None else torch.full((n,), fill, device='cuda')      # noqa: E731
    theta, grad, m, v, ms, avg = new(), new(), new(0.0), new(0.0), new(1.0), new()
    srcs = [torch.randn(s, device='cuda') * 0.01 for s in sizes]
    state = torch.tensor([0.0, 0.5, 0.9, 0.0], device='cuda')
    rate = 1e-4
    packed = len(sizes) <= K.ADAM_PACKED_MAX
    forms = {
        'adam_step': lambda kw: K.adam_step(theta, grad, m, v, state, 0.0, 0.9, 1e-8, 1.0, **kw),
        'rmsprop_step': lambda kw: K.rmsprop_step(theta, grad, ms, state, 0.9, 1e-10, 0.0, 1.0, **kw),
    }
    if packed:
        forms['adam_step_packed'] = lambda kw: K.adam_step_packed(srcs, offs, sizes, grad, theta, m, v, state, 0.0, 0.9, 1e-8, 1.0, **kw)
        forms['rmsprop_step_packed'] = lambda kw: K.rmsprop_step_packed(srcs, offs, sizes, grad, theta, ms, state, 0.9, 1e-10, 0.0, 1.0, **kw)
    out = {}
    for name, fn in forms.items():
        out[name] = {False: (lambda fn=fn: fn({})), True: (lambda fn=fn: fn({'avg': avg, 'avg_rate': rate}))}
    return out, (theta, avg), n


def measure(pairs, launches, rounds, warmup):
    """pairs: {name: {key: launch}} -> {name: {key: stats}}; every launch of every pair takes its turn in every round."""
    times = {name: {key: [] for key in forms} for name, forms in pairs.items()}
    for r in range(warmup + rounds):
        for name, forms in pairs.items():
            for key, fn in forms.items():
                t = _timed(fn, launches)
                if r >= warmup:
                    times[name][key].append(t)
    return {name: {key: _stats(us) for key, us in by.items()} for name, by in times.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--launches', type=int, default=300, help='back-to-back launches per sample')
    ap.add_argument('--rounds', type=int, default=9)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'avg_bench needs the GPU'
    import ctgan_amd.gan_cifar_resnet as R
    import ctgan_amd.kernels as K
    import ctgan_amd.tflib as lib
    lib.delete_all_params(); lib.set_seed(1)
    R.configure()
    R.build_params()
    tr = R.Trainer(seed=1)
    buckets = {'generator': list(tr.g_opt.sizes), 'critic': list(tr.d_opt.sizes)}
    lib.delete_all_params()
    res = {'what': 'optimizer update launches without / with the fused weight average on the flat buckets of the headline ResNet; device '
                   'events around back-to-back launches, the forms alternating sample by sample; microseconds per launch',
           'device_name': torch.cuda.get_device_name(0), 'launches_per_sample': a.launches, 'rounds': a.rounds, 'warmup_rounds': a.warmup}
    for bucket, sizes in buckets.items():
        forms, (theta, avg), n = bucket_forms(sizes)
        pairs = dict(forms)
        if bucket == 'generator':
            pairs['exchange_'] = {'exchange': lambda theta=theta, avg=avg: K.exchange_(theta, avg)}
        got = measure(pairs, a.launches, a.rounds, a.warmup)
        rows = {}
        for name in forms:
            plain, with_avg = got[name][False], got[name][True]
            b0, b1 = BYTES[name], BYTES[name] + AVG_BYTES
            rows[name] = {
                'plain': plain, 'with_average': with_avg,
                'bytes_per_element': {'plain': b0, 'with_average': b1, 'ratio': b1 / b0},
                'time_ratio': with_avg['median_us'] / plain['median_us'],
                'added_us': with_avg['median_us'] - plain['median_us'],
                'plain_spread_us': plain['max_us'] - plain['min_us'],
                'gbytes_per_s': {'plain': n * b0 / plain['median_us'] * 1e-3, 'with_average': n * b1 / with_avg['median_us'] * 1e-3},
            }
        if 'exchange_' in got:
            ex = got['exchange_']['exchange']
            rows['exchange_'] = {'time': ex, 'bytes_per_element': EXCHANGE_BYTES, 'gbytes_per_s': n * EXCHANGE_BYTES / ex['median_us'] * 1e-3,
                                 'sixteen_byte_path': theta.data_ptr() % 16 == 0 and avg.data_ptr() % 16 == 0}
        res[bucket] = {'elements': n, 'tensors': len(sizes), 'forms': rows}
    R.configure()
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
