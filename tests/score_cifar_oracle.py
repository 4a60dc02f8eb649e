"""TEST-ONLY fp64 restatement (numpy) of the classifier-score path of ctgan_amd.score_cifar: the three steps of csrc/score_cifar.hip
- per-chunk accumulation into [splits, K + 1] sums and 2 K counts, the finish - `streaming_score`; the statistic it must equal,
tflib.inception_score.score_from_probabilities on the fp64 softmax of the same logits - `reference_score`; and the three-launch
composition kernels.score_input replaces - `compose_input`.  Nothing under ctgan_amd/ imports this file."""
import numpy as np

# (n, splits, chunk, logit scale): the cases the restatement was checked on against score_from_probabilities
CASES = [(103, 10, 100, 3.0), (250, 10, 100, 3.0), (10, 10, 100, 3.0), (1000, 10, 300, 30.0), (37, 3, 7, 3.0)]


def logits_for(n, K=10, scale=3.0, seed=0):
    """fp32 logits [n, K] with a planted class per row (so that argmax, the marginal and the accuracy are not trivial)."""
    r = np.random.RandomState(seed)
    z = r.randn(n, K)
    cls = r.randint(0, K, n)
    z[np.arange(n), cls] += 1.5
    labels = np.where(r.rand(n) < 0.7, cls, r.randint(0, K, n)).astype(np.int32)
    return (scale * z).astype(np.float32), labels


def log_softmax64(z):
    z = np.asarray(z, dtype=np.float64)
    d = z - z.max(axis=1, keepdims=True)
    return d - np.log(np.exp(d).sum(axis=1, keepdims=True))


def reference_score(logits, splits):
    """(mean, std) of score_from_probabilities on the fp64 softmax of the logits."""
    from ctgan_amd.tflib.inception_score import score_from_probabilities
    return score_from_probabilities(np.exp(log_softmax64(logits)), splits)


def accumulate(acc, cnt, logits, r0, n, splits, labels=None):
    """ctgan_score_accum: the chunk of global rows [r0, r0 + m) into acc [splits, K + 1] and cnt [2 K], in place."""
    m, K = logits.shape
    with np.errstate(invalid='ignore', over='ignore', divide='ignore'):
        lp = log_softmax64(logits)
        p = np.exp(lp)
        term = np.where((p == 0) & np.isfinite(lp), 0.0, p * lp)
    arg = np.argmax(np.asarray(logits), axis=1)
    for k in range(splits):
        a, b = max(k * n // splits, r0) - r0, min((k + 1) * n // splits, r0 + m) - r0
        if a < b:
            acc[k, :K] += p[a:b].sum(axis=0)
            acc[k, K] += term[a:b].sum()
    cnt[:K] += np.bincount(arg, minlength=K)
    if labels is not None:
        hit = arg == np.asarray(labels)
        cnt[K:] += np.bincount(arg[hit], minlength=K)


def finish(acc, n, splits):
    """ctgan_score_finish -> [2 + splits] = mean, population std, the per-split scores."""
    K = acc.shape[1] - 1
    out = np.empty(2 + splits)
    for k in range(splits):
        nk = (k + 1) * n // splits - k * n // splits
        m = acc[k, :K] / nk
        with np.errstate(invalid='ignore', divide='ignore'):
            h = np.where(m == 0, 0.0, m * np.log(m)).sum()
        out[2 + k] = np.exp(acc[k, K] / nk - h)
    out[0], out[1] = out[2:].mean(), out[2:].std()
    return out


def streaming_score(logits, splits=10, chunk=None, labels=None):
    """The dict ClassifierScore returns, from the logits [n, K] taken in chunks of `chunk` rows."""
    logits = np.asarray(logits, dtype=np.float32)
    n, K = logits.shape
    chunk = n if chunk is None else chunk
    acc, cnt = np.zeros((splits, K + 1)), np.zeros(2 * K, dtype=np.int64)
    for r0 in range(0, n, chunk):
        accumulate(acc, cnt, logits[r0:r0 + chunk], r0, n, splits, None if labels is None else labels[r0:r0 + chunk])
    out = finish(acc, n, splits)
    return {'mean': float(out[0]), 'std': float(out[1]), 'splits': out[2:].copy(), 'hist': cnt[:K].copy(),
            'acc': float(cnt[K:].sum()) / n if labels is not None else None}


def report_dir():
    """The directory the measured figures of a GPU run go to, created if need be: $CTGAN_OUT_DIR if set, else the repository's
    run-output directory, where the other GPU tests leave their reports - the first `*_out/` entry of .gitignore (`run_out` if the
    file or such an entry is missing, so that a report is written in any case)."""
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    d = os.environ.get('CTGAN_OUT_DIR')
    if not d:
        try:
            with open(os.path.join(root, '.gitignore')) as f:
                names = [ln.strip() for ln in f if ln.strip().endswith('_out/') and not ln.startswith('#')]
        except OSError:
            names = []
        d = os.path.join(root, names[0] if names else 'run_out')
    os.makedirs(d, exist_ok=True)
    return d


def check_result(got, ref, tol):
    """mean, std and every per-split score within tol * max(1, mean); hist and acc exact.  Returns the largest relative difference."""
    bound = tol * max(1.0, abs(ref['mean']))
    errs = [abs(got['mean'] - ref['mean']), abs(got['std'] - ref['std'])] + list(np.abs(np.asarray(got['splits']) - ref['splits']))
    worst = max(errs)
    print('score: got %.17g +- %.17g, ref %.17g +- %.17g, worst abs diff %.3e (bound %.3e)' % (got['mean'], got['std'], ref['mean'], ref['std'],
                                                                                             worst, bound))
    assert worst <= bound, (worst, bound)
    assert np.array_equal(np.asarray(got['hist']), ref['hist']), (got['hist'], ref['hist'])
    assert got['acc'] == ref['acc'], (got['acc'], ref['acc'])
    return worst / max(1.0, abs(ref['mean']))


def compose_input(K, x, channels, scale, lut, pad):
    """The three launches kernels.score_input replaces, through the wrappers of `K` (ctgan_amd.kernels, or its stand-ins):
    pixels_u8 -> view [n, S, S, C] -> [n, C, S, S] contiguous -> aug_gather's fixed mode."""
    import torch
    n = x.shape[0]
    side = int(round((x.shape[1] // channels) ** 0.5))
    data = K.pixels_u8(x, channels, scale).reshape(n, side, side, channels).permute(0, 3, 1, 2).contiguous()
    return K.aug_gather(data, torch.arange(n, dtype=torch.int32, device=x.device), lut, side, pad, offset=None)


def edge_samples(n, dim, seed=0):
    """Generator-like fp32 [n, dim] in about [-1, 1] with the corners planted: exactly -1 and 1, the neighbours just outside, far outside,
    values on both sides of byte boundaries, NaN and +-inf."""
    r = np.random.RandomState(seed)
    x = np.tanh(1.5 * r.randn(n, dim)).astype(np.float32)
    one = np.float32(1.0)
    edges = np.array([-1.0, 1.0, np.nextafter(-one, np.float32(-2)), np.nextafter(one, np.float32(2)), -1.5, 1.5, -3e38, 3e38, 0.0, -0.0,
                      np.nan, np.inf, -np.inf, 1.0 - 2.0 ** -24, 2.0 / 255 - 1.0, 2.0 / 255.99 - 1.0], dtype=np.float32)
    pos = r.permutation(n * dim)[:4 * len(edges)]
    x.reshape(-1)[pos] = np.tile(edges, 4)[:len(pos)]
    x.reshape(-1)[:len(edges)] = edges          # (also at the very first elements: n = 1 keeps them)
    return x


# ------------------------------------------------------------------------------------------------ a classifier to score with
SMALL = dict(IMG=32, D_WIDTHS=(8, 8, 8, 16, 16, 16, 16, 16, 8), G_WIDTHS=(16, 8, 8), BATCH_SIZE=4, INIT_ROWS=8, COUNT=2)


def random_images(n, size=32, seed=0):
    return np.random.RandomState(seed).randint(0, 256, (n, 3, size, size)).astype(np.uint8)


def classifier_trainer(seed=3, avg_factor=0.75):
    """A ct_cifar.CifarSSLTrainer under the module's current Config after the data-dependent init on random uint8 data, no training;
    the parameter averages (zero until a step moves them) are put at avg_factor x the live values, so that the averaged pass is
    neither trivial nor the live one."""
    import torch
    import ctgan_amd.ct_cifar as M
    import ctgan_amd.tflib as lib
    cfg = M.cfg
    lib.delete_all_params(); lib.set_seed(seed)
    tr = M.CifarSSLTrainer(seed=seed, data=random_images(cfg.INIT_ROWS, cfg.IMG, seed=seed + 1))
    idx = torch.arange(cfg.INIT_ROWS, dtype=torch.int32, device=tr.dev)
    tr.init_params(tr.gather_fixed(idx, cfg.IMG + 2 * cfg.PAD, (0, 0)))
    with torch.no_grad():
        tr.d_opt.avg.copy_(tr.d_opt.theta * avg_factor)
    return tr


def predict_chunks(tr, images_u8, chunk):
    """trainer.predict(averaged=True) on the float images of a uint8 set, in chunks of `chunk` rows -> fp32 logits [N, K] (numpy)."""
    import torch
    import ctgan_amd.ct_cifar as M
    lut = torch.from_numpy(M.byte_table()).to(tr.dev)
    data = torch.as_tensor(images_u8).to(tr.dev)
    out = [tr.predict(lut[data[i:i + chunk].long()], averaged=True) for i in range(0, data.shape[0], chunk)]
    return torch.cat(out, 0).cpu().numpy()
