#!/usr/bin/env python
"""Times one iteration (classifier step + generator step) of the semi-supervised CT classifier (ctgan_amd/ct_mnist.py) at the script's
sizes on one GPU, three ways:
  1. graph replay (engine.GraphedSSLTrainer),
  2. the same trainer eager,
  3. the yardstick: the torch restatement of tests/ssl_oracle.py run in fp32 on the device through PyTorch's own kernels (autograd,
     noise from torch.randn on the device instead of the Philox streams) - not the code under test.
Also counts the kernel launches of one eager iteration (torch.profiler).  Prints one JSON line; --out writes it to a file.

    python tools/ssl_bench.py --iters 200 --warmup 20 [--out profiles/ssl_bench.json]
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
    """Median and minimum of `iters` wall-clock times of fn() (each ended by a device synchronize), after `warmup` calls; ms."""
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


def batch_throughput(fn, iters, warmup):
    """ms per call when `iters` calls are queued back to back and the device is synchronised once (what a training loop sees)."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / iters


class TorchYardstick:
    """The oracle's mathematics in fp32 on the device with torch's kernels and torch.randn noise; Adam and the average as tensor ops."""

    def __init__(self, cfg, P, dev):
        from tests import ssl_oracle as O
        self.O, self.cfg, self.dev = O, cfg, dev
        self.P = {n: v.to(dev, torch.float32).clone() for n, v in P.items()}
        self.dn, self.gn = O.d_names(cfg)[1], O.g_names(cfg)
        z = lambda names: {n: torch.zeros_like(self.P[n]) for n in names}      # noqa: E731
        self.m, self.v, self.avg = z(self.dn + self.gn), z(self.dn + self.gn), z(self.dn)
        self.t = {'d': 1, 'g': 1}

    def _noise(self, rows, n_hidden):
        widths = [self.cfg.IN_DIM] + list(self.cfg.HIDDEN)[:n_hidden]
        return [torch.randn(rows, w, device=self.dev) for w in widths]

    def _apply(self, names, grads, which):
        O, c = self.O, self.cfg
        for n, g in zip(names, grads):
            self.P[n], self.m[n], self.v[n] = O.adam_theano(self.P[n].detach(), g, self.m[n], self.v[n], self.t[which], c.LR, c.BETA1, c.BETA2)
            if which == 'd':
                self.avg[n] = self.avg[n] + c.AVG_RATE * (self.P[n] - self.avg[n])
        self.t[which] += 1

    def iteration(self, x_lab, labels, x_unl, x_unl2):
        O, c = self.O, self.cfg
        B = x_lab.shape[0]
        Q = {n: (v.detach().requires_grad_(True) if n in self.dn else v.detach()) for n, v in self.P.items()}
        with torch.no_grad():
            fake = O.generator(Q, c, torch.rand(B, c.Z_DIM, device=self.dev))
        logits = O.classifier(Q, c, torch.cat([x_lab, x_unl, x_unl, fake], 0), self._noise(4 * B, len(c.HIDDEN)))
        out4, _ = O._head_terms(logits, labels, B, c.LAMBDA_2, c.Factor_M)
        self._apply(self.dn, torch.autograd.grad(out4[0] + c.UNLABELED_WEIGHT * out4[1], [Q[n] for n in self.dn]), 'd')
        Q = {n: (v.detach().requires_grad_(True) if n in self.gn else v.detach()) for n, v in self.P.items()}
        fake = O.generator(Q, c, torch.rand(B, c.Z_DIM, device=self.dev))
        f = O.classifier(Q, c, torch.cat([fake, x_unl2], 0), self._noise(2 * B, len(c.HIDDEN) - 1), features=True)
        loss = ((f[:B].mean(0) - f[B:].mean(0)) ** 2).mean()
        self._apply(self.gn, torch.autograd.grad(loss, [Q[n] for n in self.gn]), 'g')
        return out4


def count_launches(fn):
    from torch.profiler import ProfilerActivity, profile
    fn(); torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    names = [e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]
    kernels = [n for n in names if 'memcpy' not in n.lower() and 'memset' not in n.lower()]
    return {'kernels': len(kernels), 'copies_and_memsets': len(names) - len(kernels)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=200)
    ap.add_argument('--warmup', type=int, default=20)
    ap.add_argument('--out', default=None)
    ap.add_argument('--no-launch-count', action='store_true')
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'ssl_bench needs the GPU'
    import ctgan_amd.ct_mnist as M
    import ctgan_amd.tflib as lib
    from ctgan_amd.engine import GraphedSSLTrainer
    from tests import ssl_oracle as O
    cfg = M.configure()
    dev = torch.device('cuda', 0)
    g = torch.Generator().manual_seed(0)
    B = cfg.BATCH_SIZE
    x = [torch.rand(B, cfg.IN_DIM, generator=g).to(dev) for _ in range(3)]
    y = torch.randint(0, 10, (B,), generator=g, dtype=torch.int32).to(dev)
    x0 = torch.rand(cfg.INIT_ROWS, cfg.IN_DIM, generator=g).to(dev)
    P = O.make_params(cfg, seed=1, dtype=torch.float32)

    def fresh():
        lib.delete_all_params()
        tr = M.SSLTrainer(seed=1)
        O.load_into_registry(P)
        tr.init_params(x0)
        return tr
    res = {'what': 'ct_mnist iteration (classifier step + generator step), B=%d' % B, 'device': torch.cuda.get_device_name(0),
           'iters': a.iters, 'warmup': a.warmup}
    try:
        res['commit'] = subprocess.run(['git', 'rev-parse', '--short', 'HEAD'], cwd=ROOT, capture_output=True, text=True).stdout.strip() or None
    except OSError:
        res['commit'] = None
    tr = fresh()
    eager = lambda: tr.train_iteration(x[0], y, x[1], x[2])          # noqa: E731
    res['eager'] = timed(eager, a.iters, a.warmup)
    res['eager']['queued_ms'] = batch_throughput(eager, a.iters, a.warmup)
    if not a.no_launch_count:
        try:
            res['launches_per_iteration'] = count_launches(eager)
        except Exception as e:       # the profiler is optional: the timings stand without it
            res['launches_per_iteration'] = 'unavailable: %s' % type(e).__name__
    tr = fresh()
    eng = GraphedSSLTrainer(tr)
    res['graphed'] = eng.graphed
    if eng.graphed:
        replay = lambda: eng.train_iteration(x[0], y, x[1], x[2])      # noqa: E731
        res['graph'] = timed(replay, a.iters, a.warmup)
        res['graph']['queued_ms'] = batch_throughput(replay, a.iters, a.warmup)
    else:
        res['graph_error'] = eng.graph_error
    st = O.State(P, cfg, 1, dtype=torch.float32)
    st.init(x0.cpu())
    ys = TorchYardstick(cfg, st.P, dev)
    yl = y.long()
    yard = lambda: ys.iteration(x[0], yl, x[1], x[2])                  # noqa: E731
    res['torch_fp32_yardstick'] = timed(yard, a.iters, a.warmup)
    res['torch_fp32_yardstick']['queued_ms'] = batch_throughput(yard, a.iters, a.warmup)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(line + '\n')
    M.configure(); lib.delete_all_params()


if __name__ == '__main__':
    main()
