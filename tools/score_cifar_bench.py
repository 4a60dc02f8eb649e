#!/usr/bin/env python
"""Times the scripts' own scoring - 50,000 samples of gan_cifar_resnet, 1,000 of gan_cifar, at the scripts' widths - under a full-width
CT classifier (ct_cifar after its data-dependent init on random uint8 data; no training: the time does not depend on the weights), on
one GPU, two ways in one process:

    device   score_cifar.ClassifierScore.score_generator: samples -> kernels.score_input -> logits -> kernels.score_accum, one host copy
    host     evaluate.Evaluator.get_inception_score with the SAME classifier wrapped as a host callable: uint8 pixels -> numpy float32
             NHWC -> (the callable: back to the device, the composition of launches score_input replaces, logits, softmax) ->
             numpy probabilities -> score_from_probabilities on the concatenated [n, 10] array

A figure is the median (and min / max) of `--runs` scorings after `--warmup` untimed ones, host clock around a scoring that ends in a
device synchronise; the two paths alternate run by run and score the same samples (the evaluation stream's counter is put back before
each scoring; `score_abs_diff` is the difference of their means).  Prints one JSON line; --out writes it to a file.

    python tools/score_cifar_bench.py [--out profiles/score_cifar_bench.json]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402


def _sync(dev):
    if torch.device(dev).type == 'cuda':
        torch.cuda.synchronize()


def build_scorer(dev, init_rows, cifar_cfg=None):
    """A full-width classifier after init_params on random uint8 data, averages at the live values -> ClassifierScore(trainer) with
    the classifier trainer's own Generator.* parameters removed (the GAN's have the same names)."""
    import ctgan_amd.ct_cifar as M
    import ctgan_amd.tflib as lib
    from ctgan_amd.score_cifar import ClassifierScore
    M.configure(**dict(cifar_cfg or {}, INIT_ROWS=init_rows))
    lib.delete_all_params(); lib.set_seed(1)
    cfg = M.cfg
    data = np.random.RandomState(0).randint(0, 256, (init_rows, 3, cfg.IMG, cfg.IMG)).astype(np.uint8)
    tr = M.CifarSSLTrainer(seed=1, data=data)
    tr.init_params(tr.gather_fixed(torch.arange(init_rows, dtype=torch.int32, device=tr.dev), cfg.IMG + 2 * cfg.PAD, (0, 0)))
    with torch.no_grad():
        tr.d_opt.avg.copy_(tr.d_opt.theta)
    lib.delete_params_with_name('Generator.')
    return ClassifierScore(tr)


def host_callable(scorer):
    """The same classifier as a host callable of Evaluator.get_inception_score: float32 [m, H, W, 3] in [0, 255] -> probabilities [m, 10]."""
    import ctgan_amd.ct_cifar as M
    import ctgan_amd.kernels as K
    tr = scorer.trainer

    def classify(x):
        data = torch.from_numpy(x).to(tr.dev).to(torch.uint8).permute(0, 3, 1, 2).contiguous()
        idx = torch.arange(data.shape[0], dtype=torch.int32, device=tr.dev)
        logits = tr._averaged(lambda: M._classifier(K.aug_gather(data, idx, scorer.lut, M.cfg.IMG, M.cfg.PAD), deterministic=True), True)
        return torch.softmax(logits.double(), dim=1).cpu().numpy()
    return classify


def gan_trainer(name, dev, gan_cfg=None):
    import ctgan_amd.tflib as lib
    lib.delete_params_with_name('Generator.'); lib.delete_params_with_name('Discriminator.')
    lib.set_seed(2)
    if name == 'gan_cifar_resnet':
        import ctgan_amd.gan_cifar_resnet as R
        R.configure(**(gan_cfg or {}))
        R.build_params(None if dev == 'cuda' else dev)
        return R, R.Trainer(seed=3)
    import ctgan_amd.gan_cifar as G
    from ctgan_amd import dcgan_step
    G.configure(**(gan_cfg or {}))
    dcgan_step.build_params(G, None if dev == 'cuda' else dev)
    return G, dcgan_step.DCGANTrainer(G, seed=3)


def _stats(ts):
    ts = sorted(ts)
    return {'median_ms': ts[len(ts) // 2], 'min_ms': ts[0], 'max_ms': ts[-1], 'n': len(ts)}


def measure(name, n, scorer, dev, runs, warmup, gan_cfg=None):
    from ctgan_amd import evaluate
    mod, gan = gan_trainer(name, dev, gan_cfg)
    try:
        ev = evaluate.Evaluator(gan)
        classify = host_callable(scorer)
        times = {'device': [], 'host': []}
        last = {}
        c0 = int(evaluate.eval_stream(gan).ctr.item())
        for run in range(warmup + runs):
            for path in ('device', 'host'):
                evaluate.eval_stream(gan).ctr.fill_(c0)          # every scoring draws the same samples: the two paths must agree
                _sync(dev)
                t0 = time.perf_counter()
                if path == 'device':
                    res = ev.get_classifier_score(n, scorer)
                    last[path] = (res['mean'], res['std'])
                else:
                    last[path] = ev.get_inception_score(n, classify)
                _sync(dev)
                if run >= warmup:
                    times[path].append((time.perf_counter() - t0) * 1e3)
        out = {'samples': n, 'device': _stats(times['device']), 'host': _stats(times['host']),
               'last_score_device': list(last['device']), 'last_score_host': list(last['host'])}
        out['host_over_device'] = out['host']['median_ms'] / out['device']['median_ms']
        out['score_abs_diff'] = abs(last['device'][0] - last['host'][0])
        return out
    finally:
        mod.configure()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--runs', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=1)
    ap.add_argument('--init-rows', type=int, default=100)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'score_cifar_bench needs the GPU'
    from ctgan_amd import evaluate
    dev = 'cuda'
    scorer = build_scorer(dev, a.init_rows)
    res = {'what': 'one scoring of the script\'s sample count under a full-width CT classifier: ClassifierScore (device) vs get_inception_score with '
                   'the same classifier as a host callable (host); wall clock ended by a device synchronise, the two alternating',
           'device_name': torch.cuda.get_device_name(0), 'runs': a.runs, 'warmup': a.warmup}
    for name in ('gan_cifar_resnet', 'gan_cifar'):
        res[name] = measure(name, evaluate.SCORE_SAMPLES[name], scorer, dev, a.runs, a.warmup)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
