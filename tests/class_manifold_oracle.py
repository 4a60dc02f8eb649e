"""fp64 numpy restatement of the per-class precision, recall and kernel distance (ctgan_amd.score_cifar.class_precision_recall,
class_kernel_distance; the grouped kernels of csrc/knn.hip and csrc/kid.hip); no torch.

Nothing is derived here: the functions of tests/knn_oracle.py (d2_direct, bound, radii, cover, decidable, nearest_is_unambiguous) and
tests/kid_oracle.py (kernel_distance with its e_kid) are applied to the rows of one class at a time, so every bound is theirs.

The labelled cases.  Features: knn_oracle.inputs(m, n, d, k, offset, seed=11) with m and n the sums of the sizes; labels: class c
repeated size_c times, shuffled with RandomState(1) (samples) and RandomState(2) (reference).  The smallest shapes that reach every
branch: empty classes, classes below k + 1 rows, one row, exact tiles, one past a tile, a tail in every tile, unaligned rows, two feature
chunks, one class, 32 classes.
"""
import numpy as np

from tests import kid_oracle as KD
from tests import knn_oracle as KO

SEED = 11
# name: (d, k, offset, sample sizes per class, reference sizes per class)
CASES = {
    'L1': (10, 3, 0.0, [0, 3, 64, 70], [5, 4, 65, 1]),
    'L2': (128, 3, 5.0, [100] * 10, [210] * 10),
    'L3': (33, 8, 0.0, [129, 64, 9], [130, 9, 200]),
    'L4': (17, 1, 5.0, [(7 * c) % 23 for c in range(32)], [(5 * c) % 29 + (c % 3 == 0) for c in range(32)]),
    'L5': (16, 2, 5.0, [65], [129]),
}
# L4 again: a few rows that belong to no class (labels -1 and 32), and a width that is no multiple of 4 either way
OUTSIDE = {'samples': {3: -1, 40: 32, 41: -1, 200: 32}, 'reference': {0: 32, 17: -1, 300: 32}}
# L5 again with knn_oracle's planted copies, here inside the one class: a[:5] = b[:5], b[10 .. 10 + k] = b[10], a[COPY_OF_B10] = b[10]
VARIANTS = {'L4_outside': ('L4', 17, True), 'L4_d19': ('L4', 19, False), 'L5_planted': ('L5', 16, False)}
NAMES = list(CASES) + list(VARIANTS)


def labels(sizes, seed):
    lab = np.concatenate([np.full(s, c, dtype=np.int32) for c, s in enumerate(sizes)])
    np.random.RandomState(seed).shuffle(lab)
    return lab


def inputs(name):
    """-> (a fp32 [m, d], labels int32 [m], b fp32 [n, d], labels int32 [n], classes, k)."""
    base, d_over, outside = VARIANTS.get(name, (name, None, False))
    d, k, offset, sa, sb = CASES[base]
    d = d if d_over is None else d_over
    a, b = KO.inputs(sum(sa), sum(sb), d, k, offset, seed=SEED)
    la, lb = labels(sa, 1), labels(sb, 2)
    if name == 'L5_planted':
        b[10:10 + k + 1] = b[10]
        a[:5] = b[:5]
        a[KO.COPY_OF_B10] = b[10]
    if outside:
        for lab, where in ((la, OUTSIDE['samples']), (lb, OUTSIDE['reference'])):
            for i, v in where.items():
                lab[i] = v
    return a, la, b, lb, len(sa), k


class ClassOracle:
    """One class of a case: what tests/knn_oracle.Case holds, for the rows of the class alone; None where undefined."""

    def __init__(self, a, b, k):
        self.a, self.b, self.k = a, b, k
        m, n = a.shape[0], b.shape[0]
        self.m, self.n = m, n
        self.r2_b, self.e_r2_b = KO.radii(b, k) if n >= k + 1 else (None, None)
        self.r2_a, self.e_r2_a = KO.radii(a, k) if m >= k + 1 else (None, None)
        self.dist = self.e_dist = self.nn_d2 = self.nn_idx = self.e_nn = self.nn_sure = None
        self.covered = self.decidable = self.back = self.back_decidable = None
        if m and n:
            self.dist = KO.d2_direct(a, b)
            self.e_dist = KO.bound(a, b, self.dist)
            self.nn_d2, self.nn_idx = KO.nearest(self.dist)
            self.e_nn = self.e_dist[np.arange(m), self.nn_idx]
            self.nn_sure = KO.nearest_is_unambiguous(self.dist, self.e_dist, b)
            if self.r2_b is not None:
                self.covered = KO.cover(self.dist, self.r2_b)
                self.decidable = KO.decidable(self.dist, self.r2_b, self.e_dist, self.e_r2_b)
            if self.r2_a is not None:
                self.back = KO.cover(self.dist.T, self.r2_a)
                self.back_decidable = KO.decidable(self.dist.T, self.r2_a, self.e_dist.T, self.e_r2_a)
        self.kid = KD.kernel_distance(a, b) if m >= 2 and n >= 2 else None


class Case:
    """Everything the tests compare against for one labelled case, computed once."""

    def __init__(self, name):
        self.name = name
        self.a, self.la, self.b, self.lb, self.classes, self.k = inputs(name)
        self.of = [ClassOracle(self.a[self.la == c], self.b[self.lb == c], self.k) for c in range(self.classes)]
        self.result = class_precision_recall(self.a, self.la, self.b, self.lb, self.classes, self.k, self.of)
        self.kernel = class_kernel_distance(self.a, self.la, self.b, self.lb, self.classes, self.of)


def _nanmean(v):
    return float(np.nanmean(v)) if not np.isnan(v).all() else float('nan')


def class_precision_recall(fa, la, fb, lb, classes, k, of=None):
    """The dict of ctgan_amd.score_cifar.class_precision_recall for labelled sample features against labelled reference features."""
    of = of or [ClassOracle(fa[la == c], fb[lb == c], k) for c in range(classes)]
    prec, rec, dist = np.full(classes, np.nan), np.full(classes, np.nan), np.full(classes, np.nan)
    zero = np.zeros(classes, dtype=np.int64)
    for c, o in enumerate(of):
        if o.covered is not None:
            prec[c] = o.covered.mean()
        if o.back is not None:
            rec[c] = o.back.mean()
        if o.nn_d2 is not None:
            dist[c] = np.median(np.sqrt(o.nn_d2))
            zero[c] = (o.nn_d2 == 0).sum()
    return {'precision_class': prec, 'recall_class': rec, 'nn_dist_class': dist, 'nn_zero_class': zero,
            'n_class': np.array([o.m for o in of], dtype=np.int64), 'n_class_reference': np.array([o.n for o in of], dtype=np.int64),
            'intra_precision': _nanmean(prec), 'intra_recall': _nanmean(rec), 'k': k}


def class_kernel_distance(fa, la, fb, lb, classes, of=None):
    """The dict of ctgan_amd.score_cifar.class_kernel_distance, plus 'e_kid_class': kid_oracle's bound of every class's estimate."""
    of = of or [ClassOracle(fa[la == c], fb[lb == c], 1) for c in range(classes)]
    kid = np.array([np.nan if o.kid is None else o.kid['kid'] for o in of])
    return {'kid_class': kid, 'intra_kid': _nanmean(kid), 'n_class': np.array([o.m for o in of], dtype=np.int64),
            'n_class_reference': np.array([o.n for o in of], dtype=np.int64),
            'e_kid_class': np.array([np.nan if o.kid is None else o.kid['e_kid'] for o in of])}


def undecidable(of):
    """-> (rows the oracle cannot decide, rows it was asked about) over both directions of every defined class."""
    left, rows = 0, 0
    for o in of:
        for flags in (o.decidable, o.back_decidable):
            if flags is not None:
                left += int((~flags).sum())
                rows += flags.size
    return left, rows


_CACHE = {}


def case(name):
    if name not in _CACHE:
        _CACHE[name] = Case(name)
    return _CACHE[name]
