"""The score of CIFAR-10 samples under the project's own CT classifier (ct_cifar.py / ct_cifar_te.py), kept on the device.

The CIFAR scripts' headline number is the score of generator samples (`inception_50k` of TF/CT_gan_cifar_resnet.py:350-360,414-418,
`inception score` of TF/CT_gan_cifar.py:167-176,210-212) under the 2015 Inception graph, which the reference downloads at import and
which cannot ship here.  `ClassifierScore` puts the self-trained CT classifier - evaluated on its averaged parameters, as
`predict(averaged=True)` - in its place, the move score_mnist.py makes for MNIST.  It is a CLASSIFIER score: the Inception-score
formula (TF/tflib/inception_score.py:60-69, tflib.inception_score.score_from_probabilities) over that classifier's 10 CIFAR classes.
Its values are not comparable to published Inception scores (1000 ImageNet classes, another network).

    samples -> classifier input    kernels.score_input   one launch: quantise as the saved pixels (kernels.pixels_u8's bytes), byte table,
                                                         channels-last, rotated by 180 degrees - the classifier's internal form
    classifier input -> logits     ct_cifar._classifier  the deterministic pass on the averaged parameters
    logits -> statistic            kernels.score_accum   per chunk, fp64, into caller-owned device state; kernels.score_finish at the end
No [n, K] prediction array exists; one device -> host copy per scoring (the scores and the class counts).

The normalised filters W g / sqrt(1e-6 + |W|^2) of the ten layers do not change within a scoring: they are made by the layers' own
normalisation launches in the first chunk (tflib.ops.wn_conv.constant_filters) and reused by every later chunk - the logits stay
bit-equal to `predict(averaged=True)` - and made again when the registry's parameter version moves (a classifier that trains on, or
any registry-wide bump: a GAN training between two scorings makes each scoring normalise once).  They are plain tensors owned by the
scorer: no cache outside it holds their addresses, so the conv wrappers pack them per call as they do for `predict`.

The classifier Frechet distance.  With a reference set (`reference=` / `set_reference`), `score` and `score_generator` also return
`'frechet'`: the Frechet distance between the Gaussian fits of the classifier's pooled feature layer (disc_layers[-2], D_WIDTHS[-1] =
128 wide, the layer the classifier's generator is trained against) over the scored samples and over the reference set, usually the
training images (`statistics`, once, saved with `FeatureStatistics.save`).
    features [m, D] -> raw moments    kernels.moments_accum   per chunk, fp64 sum f and sum f f^T into caller-owned device state
    moments -> mean, covariance       FeatureStatistics       on the host in fp64, from the scoring's one device -> host copy
    two fits -> distance              frechet_distance        numpy only (two eigh and one eigvalsh of D x D)
The features come from the SAME classifier pass as the logits (`_classifier(..., features='both')`): no launch of the classifier is
added or changed, and without a reference the launches and the returned dict are exactly those of a scorer that knows nothing of this.
Like the score it is a CLASSIFIER statistic, under a self-trained 10-class network: it is NOT comparable to published FID numbers
(Inception pool3, 2048 features, ImageNet).  A reference records a hash of the classifier's averaged parameters; under any other
classifier it is refused.

Precision and recall.  With a manifold set (`manifold=` / `set_manifold`, a FeatureSet: the reference FEATURES, not their fit), `score`
and `score_generator` also return the k-nearest-neighbour manifold estimate of Kynkaanniemi et al. 2019 in the same feature space:
`'precision'`, the share of samples inside some reference row's k-th-neighbour ball, `'recall'`, the share of reference rows inside
some sample's ball, and the memorisation signal: `'nn_dist'`, the median distance of a sample to its nearest reference row, and
`'nn_zero'`, the number of samples AT distance 0 from one (a replayed reference image).
    features [m, D] -> one [n, D] buffer   a device copy per chunk, from the same classifier pass as the logits
    samples vs reference balls             kernels.knn_cover: covered, nearest reference row (fp64 MFMA, no [m, n] array)
    sample radii, reference vs them        kernels.knn_radii, kernels.knn_cover
                                           all three once, after the last chunk: a workgroup owns 64 sample rows, so a launch per chunk
                                           of 1,000 would leave most of the chip idle (measured: DESIGN 19)
    counts and the median                  reduced on the device, in the scoring's one device -> host copy
Classifier statistics again: a manifold estimate under a self-trained 10-class network's 128 features, NOT comparable to published
precision / recall (VGG-16 or Inception features).  A FeatureSet records the classifier's hash as a FeatureStatistics does.

Per-class statistics.  The headline generator is class-conditional, and every statistic above pools its ten classes: a collapse inside
one class, or good images under the wrong label, hardly moves them.  With a class reference set (`class_reference=` /
`set_class_reference`, a ClassStatistics: one Gaussian fit per label, `class_statistics` of the labelled training images, once),
`score` with labels and `score_generator` of a conditional generator also return `'frechet_class'` [K], the Frechet distance per
conditioned label, `'intra_frechet'`, its mean, `'n_class'` [K], `'confusion'` [K, K] (conditioned label x predicted class) and
`'acc_class'` [K], its diagonal over its row sums.
    features [m, D], labels [m] -> raw moments per class   kernels.class_moments_accum   one launch per chunk: every workgroup compacts
                                                           its class's rows and runs moments_accum's loop over them (the same bits)
    logits [m, K], labels [m] -> confusion matrix          kernels.confusion_accum       one launch per chunk, integer counters
    moments -> fits -> distances                           ClassStatistics, intra_frechet  on the host, from the one device -> host copy
Samples without labels are refused before any launch; a label outside [0, K) shows in the counts and is refused after the copy.  Again
classifier statistics under a self-trained 10-class network: NOT comparable to published intra-FID numbers.

The kernel distance.  The Frechet distance is biased in the sample count - two sets from one distribution are at 1.6 with 1,000 samples
and at 0.15 with 20,000 - and the two CIFAR loops score at 1,000 and at 50,000.  With a kernel reference set
(`kernel_reference=` / `set_kernel_reference`, a FeatureSet), `score` and `score_generator` also return `'kid'`: the unbiased estimate
of the squared maximum mean discrepancy under the cubic kernel k(x, y) = (x . y / D + 1)^3 of Binkowski et al. 2018, whose expectation
does not depend on either count, with `'kid_blocks'`, the same estimate on disjoint blocks of rows, and `'kid_std'`, their spread.
    features [m, D] -> one [n, D] buffer   the manifold's buffer: one buffer and one copy per chunk when both are set
    all-pairs kernel sums                  kernels.kernel_tile_sums: samples x samples and samples x reference, once, after the last
                                           chunk (fp64 MFMA, one fp64 sum per 64 x 64 tile, no [m, n] array); the reference's own sums
                                           once per FeatureSet (`kernel_tiles`, saved with it)
    tile sums -> estimate, blocks          fp64 torch reductions on the device, in the scoring's one device -> host copy
A classifier-feature kernel distance under a self-trained 10-class network's 128 features: NOT comparable to published KID (Inception
pool3, 2048 features).

Per-class precision, recall and kernel distance.  The two distances above pool the ten classes as well: a conditional generator that
drops modes inside class 3 keeps a good pooled recall, because the other nine classes cover the reference set.  With a class manifold
(`class_manifold=` / `set_class_manifold`) or a class kernel reference (`class_kernel_reference=` / `set_class_kernel_reference`), LABELLED
FeatureSets (`features(images, labels=...)`), `score` with labels and `score_generator` of a conditional generator also return
`'precision_class'`, `'recall_class'`, `'nn_dist_class'`, `'nn_zero_class'`, `'intra_precision'`, `'intra_recall'`, or `'kid_class'` and
`'intra_kid'`, with `'n_class'` and `'n_class_reference'` (class_precision_recall, class_kernel_distance).
    features [n, D], labels [n] -> sorted by class   kernels.class_segments: torch on the device, the segment starts stay there
    every class in one launch                        kernels.knn_cover_seg, knn_radii_seg, kernel_tile_sums_seg: the pooled kernels' bodies
                                                     on a class's segment (the same bits as on its gathered rows), once, after the last chunk
    ragged tile sums -> per-class totals             kernels.segment_sums: one fixed order
    counts, medians                                  cumsum differences and sorts on the device, in the scoring's one device -> host copy
No class count comes to the host before that copy.  Classifier statistics under a self-trained 10-class network once more: NOT
comparable to published per-class precision / recall or intra-class KID.
"""
import hashlib
import os

import numpy as np
import torch

from . import ct_cifar
from . import kernels as K
from . import tflib as lib
from .tflib.ops import wn_conv as _wn

MAX_CLASSES = 32            # kernels.score_accum keeps a row's class accumulators in registers
DEFAULT_CHUNK = 1000        # rows per classifier pass


class FeatureStatistics:
    """The Gaussian fit of a feature layer over `n` rows: `mean` fp64 [D], `cov` fp64 [D, D] (unbiased, n - 1), and `classifier`, the
    hash (ClassifierScore.fingerprint) of the averaged parameters the features were computed under - None for a synthetic fit."""

    def __init__(self, n, mean, cov, classifier=None):
        self.n = int(n)
        self.mean = np.ascontiguousarray(mean, dtype=np.float64).reshape(-1)
        self.cov = np.ascontiguousarray(cov, dtype=np.float64)
        self.classifier = None if classifier is None else str(classifier)
        if self.n < 1 or self.cov.shape != (self.mean.size, self.mean.size):
            raise ValueError('FeatureStatistics: n %d, mean %s, cov %s' % (self.n, self.mean.shape, self.cov.shape))

    @classmethod
    def from_moments(cls, n, s1, s2, classifier=None):
        """From the raw moments s1 = sum_i f_i, s2 = sum_i f_i f_i^T (fp64, what kernels.moments_accum leaves): mean = s1 / n,
        cov = (s2 - n mean mean^T) / (n - 1); n = 1 has no covariance (NaN), and frechet_distance refuses it."""
        s1, s2 = np.asarray(s1, dtype=np.float64), np.asarray(s2, dtype=np.float64)
        mean = s1 / n
        cov = (s2 - n * np.outer(mean, mean)) / (n - 1) if n > 1 else np.full(s2.shape, np.nan)
        return cls(n, mean, cov, classifier)

    def save(self, path):
        """-> `path` (numpy .npz; the name is taken as given)."""
        with open(path, 'wb') as f:
            np.savez(f, n=np.int64(self.n), mean=self.mean, cov=self.cov, classifier=np.str_(self.classifier or ''))

    @classmethod
    def load(cls, path):
        with np.load(path, allow_pickle=False) as z:
            return cls(int(z['n']), z['mean'], z['cov'], str(z['classifier']) or None)


def _psd_sqrt(cov):
    w, v = np.linalg.eigh(cov)
    return (v * np.sqrt(np.maximum(w, 0.0))) @ v.T


def frechet_distance(a, b):
    """|mu_a - mu_b|^2 + tr S_a + tr S_b - 2 tr (S_a^1/2 S_b S_a^1/2)^1/2 between two FeatureStatistics, on the host in fp64 with numpy
    only: S_a^1/2 from eigh(S_a) with negative eigenvalues clipped at 0, the last trace as the sum of sqrt(max(lambda_k, 0)) over the
    eigenvalues of the symmetrised product.  Singular covariances (n < D) are fine; n < 2 on either side, different widths, or fits
    recorded under two different classifiers raise."""
    if a.n < 2 or b.n < 2:
        raise ValueError('frechet_distance: a covariance needs at least 2 rows (got %d and %d)' % (a.n, b.n))
    if a.mean.shape != b.mean.shape:
        raise ValueError('frechet_distance: %d and %d features' % (a.mean.size, b.mean.size))
    if a.classifier is not None and b.classifier is not None and a.classifier != b.classifier:
        raise ValueError('frechet_distance: the two statistics were computed under different classifiers')
    root = _psd_sqrt(a.cov)
    prod = root @ b.cov @ root
    lam = np.linalg.eigvalsh((prod + prod.T) / 2)
    diff = a.mean - b.mean
    return float(diff @ diff + np.trace(a.cov) + np.trace(b.cov) - 2.0 * np.sqrt(np.maximum(lam, 0.0)).sum())


class ClassStatistics:
    """The Gaussian fits of a feature layer per class label: `n` int64 [K] rows per class, `mean` fp64 [K, D], `cov` fp64 [K, D, D]
    (unbiased), and `classifier` as FeatureStatistics records it.  A class with fewer than 2 rows has a NaN covariance, an empty one a
    NaN mean too.  The raw moments are not kept: `pooled` rebuilds them per class from the fit, s1 = n mean and
    s2 = (n - 1) cov + n mean mean^T, each within a few roundings (under 8 2^-53 (|s2| + n |mean| |mean|^T) elementwise) of the sums
    the fit was made from - below the summation error n 2^-52 |F|^T |F| those sums are known to once a class has a handful of rows."""

    def __init__(self, n, mean, cov, classifier=None):
        self.n = np.ascontiguousarray(n, dtype=np.int64).reshape(-1)
        self.mean = np.ascontiguousarray(mean, dtype=np.float64)
        self.cov = np.ascontiguousarray(cov, dtype=np.float64)
        self.classifier = None if classifier is None else str(classifier)
        k = self.n.size
        if k < 1 or (self.n < 0).any() or self.mean.ndim != 2 or self.mean.shape[0] != k or self.cov.shape != (k, self.mean.shape[1], self.mean.shape[1]):
            raise ValueError('ClassStatistics: n %s, mean %s, cov %s' % (self.n.shape, self.mean.shape, self.cov.shape))

    @property
    def classes(self):
        return self.n.size

    @property
    def width(self):
        return self.mean.shape[1]

    @classmethod
    def from_moments(cls, cnt, s1, s2, classifier=None):
        """From the per-class raw moments kernels.class_moments_accum leaves (cnt [K], s1 [K, D], s2 [K, D, D]):
        FeatureStatistics.from_moments per class; NaN where a class has too few rows."""
        cnt = np.asarray(cnt, dtype=np.int64).reshape(-1)
        s1, s2 = np.asarray(s1, dtype=np.float64), np.asarray(s2, dtype=np.float64)
        mean, cov = np.full(s1.shape, np.nan), np.full(s2.shape, np.nan)
        for c in range(cnt.size):
            if cnt[c] > 0:
                fit = FeatureStatistics.from_moments(int(cnt[c]), s1[c], s2[c])
                mean[c], cov[c] = fit.mean, fit.cov
        return cls(cnt, mean, cov, classifier)

    def of(self, c):
        """The FeatureStatistics of class `c` (which must have at least one row)."""
        if self.n[c] < 1:
            raise ValueError('ClassStatistics: class %d has no rows' % c)
        return FeatureStatistics(int(self.n[c]), self.mean[c], self.cov[c], self.classifier)

    def pooled(self):
        """The FeatureStatistics of all counted rows together, from the sum over the classes of the rebuilt raw moments."""
        d = self.width
        s1, s2 = np.zeros(d), np.zeros((d, d))
        for c in range(self.classes):
            nc = int(self.n[c])
            if nc > 0:
                outer = nc * np.outer(self.mean[c], self.mean[c])
                s1 += nc * self.mean[c]
                s2 += outer if nc == 1 else (nc - 1) * self.cov[c] + outer
        total = int(self.n.sum())
        if total < 1:
            raise ValueError('ClassStatistics: no rows')
        return FeatureStatistics.from_moments(total, s1, s2, self.classifier)

    def save(self, path):
        """-> `path` (numpy .npz; the name is taken as given)."""
        with open(path, 'wb') as f:
            np.savez(f, n=self.n, mean=self.mean, cov=self.cov, classifier=np.str_(self.classifier or ''))

    @classmethod
    def load(cls, path):
        with np.load(path, allow_pickle=False) as z:
            return cls(z['n'], z['mean'], z['cov'], str(z['classifier']) or None)


def intra_frechet(a, b):
    """The per-class Frechet distance between two ClassStatistics -> {'frechet_class': fp64 [K], frechet_distance(a.of(c), b.of(c)), NaN
    where either side has fewer than 2 rows of class c; 'intra_frechet': its mean over the classes that are not NaN}.  Different class
    counts, widths or recorded classifiers raise, and so does a pair without a class of 2 rows on both sides."""
    if a.classes != b.classes:
        raise ValueError('intra_frechet: %d and %d classes' % (a.classes, b.classes))
    if a.width != b.width:
        raise ValueError('intra_frechet: %d and %d features' % (a.width, b.width))
    if a.classifier is not None and b.classifier is not None and a.classifier != b.classifier:
        raise ValueError('intra_frechet: the two statistics were computed under different classifiers')
    dist = np.full(a.classes, np.nan)
    for c in range(a.classes):
        if a.n[c] >= 2 and b.n[c] >= 2:
            dist[c] = frechet_distance(a.of(c), b.of(c))
    if np.isnan(dist).all():
        raise ValueError('intra_frechet: no class has 2 rows on both sides')
    return {'frechet_class': dist, 'intra_frechet': float(np.nanmean(dist))}


class FeatureSet:
    """The feature rows themselves, fp32 [n, D], of a set under the classifier with hash `classifier` (None: synthetic), with the squared
    k-th-neighbour radii that `radii(k)` computes on the device once per k and keeps (and `save` writes with the features), and the set's
    own kernel tile sums that `kernel_tiles()` computes once and keeps (and `save` writes once they exist).
    labels (int [n], with classes, 1 to MAX_CLASSES): the class of every row, for class_precision_recall and class_kernel_distance; a
    label outside [0, classes) belongs to no class.  `by_class()` sorts the rows by class on the device once; `class_radii(k)` and
    `class_kernel_totals()` are the per-class counterparts of `radii` and `kernel_tiles`, computed once, kept and saved.  A set without
    labels holds, and saves, exactly what it did before labels existed."""

    def __init__(self, features, classifier=None, radii=None, kernel_tiles=None, labels=None, classes=None, class_radii=None,
                 class_kernel_totals=None):
        f = features if isinstance(features, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(features, dtype=np.float32))
        if f.dim() != 2 or f.dtype != torch.float32 or f.shape[0] < 1 or f.shape[1] < 1:
            raise ValueError('FeatureSet: fp32 [n, D] features expected (got %s %s)' % (f.dtype, tuple(f.shape)))
        self.features = f.detach().contiguous()
        self.classifier = None if classifier is None else str(classifier)
        self._radii = {}
        for k, r in (radii or {}).items():
            r = r if isinstance(r, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(r, dtype=np.float64))
            if r.dtype != torch.float64 or tuple(r.shape) != (self.n,):
                raise ValueError('FeatureSet: radii of k = %s are not fp64 [%d]' % (k, self.n))
            self._radii[int(k)] = r.contiguous()
        self._kernel_tiles = None
        if kernel_tiles is not None:
            t = kernel_tiles if isinstance(kernel_tiles, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(kernel_tiles, dtype=np.float64))
            tiles = -(-self.n // K.KERNEL_TILE)
            if t.dtype != torch.float64 or tuple(t.shape) != (tiles, tiles):
                raise ValueError('FeatureSet: kernel tile sums are not fp64 [%d, %d]' % (tiles, tiles))
            self._kernel_tiles = t.contiguous()
        self.labels, self.classes = None, None
        self._by_class, self._class_radii, self._class_kernel_totals = None, {}, None
        if labels is None:
            if classes is not None or class_radii or class_kernel_totals is not None:
                raise ValueError('FeatureSet: classes, class radii or class kernel totals without labels')
            return
        lab = labels if isinstance(labels, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(labels))
        if lab.dim() != 1 or lab.shape[0] != self.n or lab.dtype.is_floating_point or lab.dtype == torch.bool:
            raise ValueError('FeatureSet: int labels [%d] expected (got %s %s)' % (self.n, lab.dtype, tuple(lab.shape)))
        if classes is None or int(classes) < 1 or int(classes) > MAX_CLASSES:
            raise ValueError('FeatureSet: labels need classes= (1 to %d; got %s)' % (MAX_CLASSES, classes))
        self.labels, self.classes = lab.detach().to(torch.int32).contiguous(), int(classes)
        for k, r in (class_radii or {}).items():
            r = r if isinstance(r, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(r, dtype=np.float64))
            if r.dtype != torch.float64 or tuple(r.shape) != (self.n,):
                raise ValueError('FeatureSet: class radii of k = %s are not fp64 [%d]' % (k, self.n))
            self._class_radii[int(k)] = r.contiguous()
        if class_kernel_totals is not None:
            t = class_kernel_totals
            t = t if isinstance(t, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(t, dtype=np.float64))
            if t.dtype != torch.float64 or tuple(t.shape) != (self.classes,):
                raise ValueError('FeatureSet: class kernel totals are not fp64 [%d]' % self.classes)
            self._class_kernel_totals = t.contiguous()

    @property
    def n(self):
        return self.features.shape[0]

    @property
    def width(self):
        return self.features.shape[1]

    def device_features(self):
        """The features on the project's device (moved there once)."""
        dev = lib._dev()
        if self.features.device != dev:
            self.features = self.features.to(dev)
        return self.features

    def radii(self, k):
        """fp64 [n] on the device: the squared distance of every row to its k-th nearest other row (kernels.knn_radii, once per k)."""
        k = int(k)
        if k not in self._radii:
            if self.n < k + 1:
                raise ValueError('FeatureSet: %d rows have no %d-th other neighbour' % (self.n, k))
            self._radii[k] = K.knn_radii(self.device_features(), k)
        dev = lib._dev()
        if self._radii[k].device != dev:
            self._radii[k] = self._radii[k].to(dev)
        return self._radii[k]

    def kernel_tiles(self):
        """fp64 [ceil(n / 64), ceil(n / 64)] on the device: the sums of (f_i . f_j / D + 1)^3 over the pairs i != j of every 64 x 64 tile of
        the set against itself (kernels.kernel_tile_sums, once)."""
        if self._kernel_tiles is None:
            f = self.device_features()
            self._kernel_tiles = K.kernel_tile_sums(f, f, exclude_diag=True)
        dev = lib._dev()
        if self._kernel_tiles.device != dev:
            self._kernel_tiles = self._kernel_tiles.to(dev)
        return self._kernel_tiles

    def _need_labels(self, what):
        if self.labels is None:
            raise ValueError('FeatureSet.%s: the set has no labels' % what)

    def by_class(self):
        """-> (the features sorted by class fp32 [n, D], perm int64 [n], seg int32 [classes + 1]) on the device, made once: sorted =
        features[perm], the stable sort by label (kernels.class_segments), class c its rows [seg[c], seg[c + 1]), the rows of no class
        behind seg[classes].  Torch alone; no count comes to the host."""
        self._need_labels('by_class')
        if self._by_class is None:
            f = self.device_features()
            perm, seg = K.class_segments(self.labels.to(f.device), self.classes)
            self._by_class = (f.index_select(0, perm).contiguous(), perm, seg)
        return self._by_class

    def class_radii(self, k):
        """fp64 [n] on the device, in by_class() order: the squared distance of every row to its k-th nearest other row of its own class
        (kernels.knn_radii_seg, once per k); +inf in a class of fewer than k + 1 rows."""
        self._need_labels('class_radii')
        k = int(k)
        if k < 1 or k > K.KNN_MAX_K:
            raise ValueError('FeatureSet: k = %d (1 to %d)' % (k, K.KNN_MAX_K))
        if k not in self._class_radii:
            f, _, seg = self.by_class()
            self._class_radii[k] = K.knn_radii_seg(f, seg, k, out=torch.full((self.n,), float('inf'), dtype=torch.float64, device=f.device))
        dev = lib._dev()
        if self._class_radii[k].device != dev:
            self._class_radii[k] = self._class_radii[k].to(dev)
        return self._class_radii[k]

    def class_kernel_totals(self):
        """fp64 [classes] on the device: for every class the sum of (f_i . f_j / D + 1)^3 over the pairs i != j of its rows
        (kernels.kernel_tile_sums_seg of the sorted set against itself, then kernels.segment_sums: one fixed order; once)."""
        self._need_labels('class_kernel_totals')
        if self._class_kernel_totals is None:
            f, _, seg = self.by_class()
            self._class_kernel_totals = K.segment_sums(*K.kernel_tile_sums_seg(f, seg, f, seg, exclude_diag=True))
        dev = lib._dev()
        if self._class_kernel_totals.device != dev:
            self._class_kernel_totals = self._class_kernel_totals.to(dev)
        return self._class_kernel_totals

    def save(self, path):
        """-> `path` (numpy .npz; the name is taken as given): the features, the classifier's hash, every radius computed so far and the
        kernel tile sums if they have been computed; of a labelled set also the labels, the class count, every class radius computed so
        far and the class kernel totals if they have been computed."""
        arrays = {'radii_%d' % k: r.cpu().numpy() for k, r in self._radii.items()}
        if self._kernel_tiles is not None:
            arrays['kernel_tiles'] = self._kernel_tiles.cpu().numpy()
        if self.labels is not None:
            arrays.update({'class_radii_%d' % k: r.cpu().numpy() for k, r in self._class_radii.items()})
            arrays.update(labels=self.labels.cpu().numpy(), classes=np.int64(self.classes),
                          class_radii_k=np.asarray(sorted(self._class_radii), dtype=np.int64))
            if self._class_kernel_totals is not None:
                arrays['class_kernel_totals'] = self._class_kernel_totals.cpu().numpy()
        with open(path, 'wb') as f:
            np.savez(f, features=self.features.cpu().numpy(), classifier=np.str_(self.classifier or ''),
                     radii_k=np.asarray(sorted(self._radii), dtype=np.int64), **arrays)

    @classmethod
    def load(cls, path):
        with np.load(path, allow_pickle=False) as z:
            kw = {}
            if 'labels' in z.files:
                kw = {'labels': z['labels'], 'classes': int(z['classes']),
                      'class_radii': {int(k): z['class_radii_%d' % k] for k in z['class_radii_k']},
                      'class_kernel_totals': z['class_kernel_totals'] if 'class_kernel_totals' in z.files else None}
            return cls(z['features'], str(z['classifier']) or None, {int(k): z['radii_%d' % k] for k in z['radii_k']},
                       z['kernel_tiles'] if 'kernel_tiles' in z.files else None, **kw)


def _manifold_counts(samples, reference, k):
    """The device half of precision_recall -> fp64 [5] on the device: the samples inside some reference ball, the reference rows inside
    some sample ball, the samples at distance 0 from a reference row, and the square roots of the two middle elements of the sorted
    nearest-reference distances (their mean is the median).  samples: device features [m, D]."""
    m = samples.shape[0]
    ref = reference.device_features()
    covered, nn_d2, _ = K.knn_cover(samples, ref, reference.radii(k))
    back, _, _ = K.knn_cover(ref, samples, K.knn_radii(samples, k))
    ordered = torch.sort(nn_d2).values
    mid = torch.sqrt(torch.stack([ordered[(m - 1) // 2], ordered[m // 2]]))
    return torch.cat([torch.stack([covered.sum(), back.sum(), (nn_d2 == 0).sum()]).to(torch.float64), mid])


def _manifold_result(host, m, n, k):
    return {'precision': float(host[0]) / m, 'recall': float(host[1]) / n, 'k': int(k), 'nn_dist': float((host[3] + host[4]) / 2),
            'nn_zero': int(host[2])}


def _check_sets(samples, reference, k):
    if samples.width != reference.width:
        raise ValueError('precision_recall: %d and %d features' % (samples.width, reference.width))
    if samples.classifier is not None and reference.classifier is not None and samples.classifier != reference.classifier:
        raise ValueError('precision_recall: the two feature sets were computed under different classifiers')
    if k < 1 or k > K.KNN_MAX_K:
        raise ValueError('precision_recall: k = %d (1 to %d)' % (k, K.KNN_MAX_K))
    if samples.n < k + 1 or reference.n < k + 1:
        raise ValueError('precision_recall: %d and %d rows have no %d-th other neighbour' % (samples.n, reference.n, k))


def precision_recall(samples, reference, k=3):
    """The k-nearest-neighbour manifold estimate (Kynkaanniemi et al. 2019) between two FeatureSets, on the device:
    -> {'precision': the share of samples within the k-th-neighbour radius of some reference row, 'recall': the share of reference rows
    within that of some sample, 'k', 'nn_dist': the median over the samples of the distance to the nearest reference row, 'nn_zero': the
    number of samples at distance exactly 0 from a reference row - bit-identical features}.  Different widths, sets recorded under two
    different classifiers, or fewer than k + 1 rows on a side raise."""
    k = int(k)
    _check_sets(samples, reference, k)
    host = _manifold_counts(samples.device_features(), reference, k).cpu().numpy()
    return _manifold_result(host, samples.n, reference.n, k)


def kernel_subset(m, n, subset=None):
    """The block size of kernel_distance's error bar for `m` samples and `n` reference rows: a given `subset` must be a positive multiple
    of the kernel tile (64); None: 64 max(1, min(1024, min(m, n) // 4) // 64) - 1024 at 50,000 rows, near the conventional 1,000, and
    192 at 1,000."""
    tile = K.KERNEL_TILE
    if subset is None:
        return tile * max(1, min(1024, min(m, n) // 4) // tile)
    s = int(subset)
    if s != subset or s < tile or s % tile:
        raise ValueError('kernel_distance: subset = %s (a positive multiple of %d)' % (subset, tile))
    return s


def _kernel_values(xx, yy, xy, m, n, s):
    """The device half of kernel_distance -> fp64 [1 + P] on the device: the estimate over all rows, then the P = min(m // s, n // s)
    block estimates.  xx [ceil(m / 64)]^2 and yy [ceil(n / 64)]^2: the two sets' own tile sums without the diagonal, xy: the cross sums."""
    parts = [xx.sum() / (m * (m - 1.0)) + yy.sum() / (n * (n - 1.0)) - 2.0 * xy.sum() / (float(m) * n)]
    t, p = s // K.KERNEL_TILE, min(m // s, n // s)
    if p > 0:
        idx = torch.arange(p, device=xx.device)

        def diagonal(tiles):          # the sums of the p diagonal t x t blocks of a tile matrix
            return tiles[:p * t, :p * t].reshape(p, t, p, t)[idx, :, idx, :].sum(dim=(1, 2))

        parts.append((diagonal(xx) + diagonal(yy)) / (s * (s - 1.0)) - 2.0 * diagonal(xy) / (float(s) * s))
    return torch.cat([v.reshape(-1) for v in parts])


def _kernel_result(host, s):
    blocks = np.array(host[1:], dtype=np.float64)
    return {'kid': float(host[0]), 'kid_std': float(blocks.std(ddof=1)) if blocks.size >= 2 else None, 'kid_blocks': blocks, 'subset': int(s)}


def _check_kernel_sets(samples, reference):
    if samples.width != reference.width:
        raise ValueError('kernel_distance: %d and %d features' % (samples.width, reference.width))
    if samples.classifier is not None and reference.classifier is not None and samples.classifier != reference.classifier:
        raise ValueError('kernel_distance: the two feature sets were computed under different classifiers')
    if samples.n < 2 or reference.n < 2:
        raise ValueError('kernel_distance: %d and %d rows (at least 2 on each side)' % (samples.n, reference.n))


def kernel_distance(samples, reference, subset=None):
    """The unbiased kernel distance (Binkowski et al. 2018: the squared maximum mean discrepancy under k(x, y) = (x . y / D + 1)^3)
    between two FeatureSets of m and n rows, on the device:
    -> {'kid': Sxx / (m (m - 1)) + Syy / (n (n - 1)) - 2 Sxy / (m n) over ALL rows of both sets, Sxx and Syy the kernel sums over the
    pairs i != j within a set and Sxy over all pairs across; 'kid_blocks' fp64 [P]: the same estimate on the P = min(m // s, n // s)
    disjoint blocks of s = `subset` consecutive rows of either set (kernel_subset; rows are i.i.d. draws or a shuffled file, so
    consecutive blocks serve); 'kid_std': their standard deviation (ddof = 1), None when P < 2; 'subset': s}.  Its expectation does not
    depend on m or n, and it may be negative.  Different widths, sets recorded under two different classifiers, or fewer than 2 rows on
    a side raise."""
    _check_kernel_sets(samples, reference)
    m, n = samples.n, reference.n
    s = kernel_subset(m, n, subset)
    xy = K.kernel_tile_sums(samples.device_features(), reference.device_features())
    host = _kernel_values(samples.kernel_tiles(), reference.kernel_tiles(), xy, m, n, s).cpu().numpy()
    return _kernel_result(host, s)


def _class_sums(values, seg):
    """Per-class sums of an integer-valued [rows] array in class-sorted order -> int64 [K]: differences of one cumsum at the segment
    starts - exact, whatever the order.  What lies at or behind seg[K] is never counted."""
    total = torch.zeros(values.numel() + 1, dtype=torch.int64, device=values.device)
    total[1:] = torch.cumsum(values.to(torch.int64), 0)
    at = total.index_select(0, seg.to(torch.int64))
    return at[1:] - at[:-1]


def _class_manifold_values(feat, seg, reference, k):
    """The device half of class_precision_recall -> fp64 [7 K] on the device: per class the samples inside some ball of the class's
    reference rows, the reference rows inside some ball of the class's samples, the samples at distance 0 from a reference row of
    their class, the two row counts, and the two middle elements of the class's sorted squared nearest-reference distances (their
    square roots, and the median, are the host's: a correctly rounded sqrt).
    feat, seg: the samples' class-sorted features [m, D] and segment starts on the device; four grouped launches, no count on the host."""
    m, dev = feat.shape[0], feat.device
    ref, _, rseg = reference.by_class()
    covered, nn_d2, _ = K.knn_cover_seg(feat, seg, ref, rseg, reference.class_radii(k), torch.zeros(m, dtype=torch.int32, device=dev),
                                        torch.full((m,), float('inf'), dtype=torch.float64, device=dev))
    r2 = K.knn_radii_seg(feat, seg, k, out=torch.full((m,), float('inf'), dtype=torch.float64, device=dev))
    back, _, _ = K.knn_cover_seg(ref, rseg, feat, seg, r2, torch.zeros(ref.shape[0], dtype=torch.int32, device=dev))
    seg64, rseg64 = seg.to(torch.int64), rseg.to(torch.int64)
    cnt, rcnt = seg64[1:] - seg64[:-1], rseg64[1:] - rseg64[:-1]
    # the class's distances in ascending order at its own rows: sort by value, then stably by class (the rows of no class hold +inf, last)
    cls = torch.searchsorted(seg64[1:].contiguous(), torch.arange(m, dtype=torch.int64, device=dev), right=True)
    by_value = torch.argsort(nn_d2)
    ordered = nn_d2.index_select(0, by_value).index_select(0, torch.argsort(cls.index_select(0, by_value), stable=True))
    lo = (seg64[:-1] + (cnt - 1).clamp(min=0) // 2).clamp(max=m - 1)
    hi = (seg64[:-1] + cnt // 2).clamp(max=m - 1)
    mid = torch.cat([ordered.index_select(0, lo), ordered.index_select(0, hi)])
    counts = torch.cat([_class_sums(covered, seg), _class_sums(back, rseg), _class_sums(nn_d2 == 0, seg), cnt, rcnt])
    return torch.cat([counts.to(torch.float64), mid])


def _nanmean(values):
    return float(np.nanmean(values)) if not np.isnan(values).all() else float('nan')


def _class_manifold_result(host, classes, k):
    nc = classes
    cov, back, zero, n, nref = (host[i * nc:(i + 1) * nc].astype(np.int64) for i in range(5))
    lo, hi = host[5 * nc:6 * nc], host[6 * nc:7 * nc]
    nan = np.full(nc, np.nan)
    precision = np.where((n > 0) & (nref >= k + 1), cov / np.maximum(n, 1), nan)
    recall = np.where((nref > 0) & (n >= k + 1), back / np.maximum(nref, 1), nan)
    with np.errstate(invalid='ignore'):
        dist = np.where((n > 0) & (nref > 0), (np.sqrt(lo) + np.sqrt(hi)) / 2, nan)
    return {'precision_class': precision, 'recall_class': recall, 'nn_dist_class': dist, 'nn_zero_class': np.where(nref > 0, zero, 0),
            'n_class': n, 'n_class_reference': nref, 'intra_precision': _nanmean(precision), 'intra_recall': _nanmean(recall), 'k': int(k)}


def _check_class_sets(samples, reference, what):
    if samples.labels is None or reference.labels is None:
        raise ValueError('%s: both feature sets need labels' % what)
    if samples.width != reference.width:
        raise ValueError('%s: %d and %d features' % (what, samples.width, reference.width))
    if samples.classes != reference.classes:
        raise ValueError('%s: %d and %d classes' % (what, samples.classes, reference.classes))
    if samples.classifier is not None and reference.classifier is not None and samples.classifier != reference.classifier:
        raise ValueError('%s: the two feature sets were computed under different classifiers' % what)


def class_precision_recall(samples, reference, k=3):
    """precision_recall per class between two LABELLED FeatureSets, on the device, every class in the same four launches
    (kernels.knn_cover_seg, kernels.knn_radii_seg): the precision of class c is the share of the samples with label c that lie inside the
    k-th-neighbour ball of some reference row of class c, the radii taken INSIDE the class; the recall is the mirror image.
    -> {'precision_class', 'recall_class', 'nn_dist_class' (the per-class median distance to the nearest reference row of the class):
    fp64 [K], NaN where undefined - precision where the class has no sample or its reference fewer than k + 1 rows, recall where it has
    no reference row or fewer than k + 1 samples, nn_dist where either side is empty; 'nn_zero_class' int [K]; 'n_class',
    'n_class_reference' int [K]; 'intra_precision', 'intra_recall': the means over the classes that are not NaN (NaN when none is);
    'k'}.  One device -> host copy.  Unlabelled sets, different widths, class counts or recorded classifiers raise."""
    k = int(k)
    _check_class_sets(samples, reference, 'class_precision_recall')
    if k < 1 or k > K.KNN_MAX_K:
        raise ValueError('class_precision_recall: k = %d (1 to %d)' % (k, K.KNN_MAX_K))
    feat, _, seg = samples.by_class()
    host = _class_manifold_values(feat, seg, reference, k).cpu().numpy()
    return _class_manifold_result(host, samples.classes, k)


def _class_kernel_values(feat, seg, own, reference):
    """The device half of class_kernel_distance -> fp64 [5 K] on the device: per class Sxx (own: the samples' own totals), Syy, Sxy and
    the two row counts.  One grouped launch and one segment_sums here; the two sets' own totals once per set."""
    ref, _, rseg = reference.by_class()
    xy = K.segment_sums(*K.kernel_tile_sums_seg(feat, seg, ref, rseg))
    seg64, rseg64 = seg.to(torch.int64), rseg.to(torch.int64)
    return torch.cat([own, reference.class_kernel_totals(), xy, (seg64[1:] - seg64[:-1]).to(torch.float64),
                      (rseg64[1:] - rseg64[:-1]).to(torch.float64)])


def _class_kernel_result(host, classes):
    nc = classes
    xx, yy, xy = host[:nc], host[nc:2 * nc], host[2 * nc:3 * nc]
    m, n = host[3 * nc:4 * nc], host[4 * nc:5 * nc]
    ok = (m >= 2) & (n >= 2)
    ms, ns = np.where(ok, m, 2.0), np.where(ok, n, 2.0)
    kid = np.where(ok, xx / (ms * (ms - 1.0)) + yy / (ns * (ns - 1.0)) - 2.0 * xy / (ms * ns), np.nan)
    return {'kid_class': kid, 'intra_kid': _nanmean(kid), 'n_class': m.astype(np.int64), 'n_class_reference': n.astype(np.int64)}


def class_kernel_distance(samples, reference):
    """kernel_distance per class between two LABELLED FeatureSets, on the device, every class in the same launch
    (kernels.kernel_tile_sums_seg, then kernels.segment_sums: the per-class totals in one fixed order):
    -> {'kid_class' fp64 [K]: Sxx_c / (m_c (m_c - 1)) + Syy_c / (n_c (n_c - 1)) - 2 Sxy_c / (m_c n_c) over the rows of class c, NaN
    with fewer than 2 rows on a side; 'intra_kid': its mean over the classes that are not NaN; 'n_class', 'n_class_reference'}.  One
    device -> host copy.  Unlabelled sets, different widths, class counts or recorded classifiers raise."""
    _check_class_sets(samples, reference, 'class_kernel_distance')
    feat, _, seg = samples.by_class()
    host = _class_kernel_values(feat, seg, samples.class_kernel_totals(), reference).cpu().numpy()
    return _class_kernel_result(host, samples.classes)


def _avg_kw(averaged):
    """Keyword of Evaluator.score_draws for samples of the generator's weight average (nothing is passed for the live generator: the
    call is then the one it always was)."""
    return {'averaged': True} if averaged else {}


def _module(te):
    if te:
        from . import ct_cifar_te
        return ct_cifar_te
    return ct_cifar


class ClassifierScore:
    """ClassifierScore(trainer): scores through a live ct_cifar.CifarSSLTrainer / ct_cifar_te.CifarTETrainer's averaged parameters.
    ClassifierScore(weights=PATH): from a checkpoint ct_cifar.train / ct_cifar_te.train wrote (under the module's current Config): only the
    `Classifier.*` entries are loaded, with the averaged values written into the parameters themselves; no generator parameter is
    created (ct_cifar's `Generator.*` names would be picked up by the GAN modules' params_with_name('Generator')).  When PATH does not
    exist and `data_dir` (or `arrays`) is given, the classifier is trained first - ct_cifar.train (te=True: ct_cifar_te.train) for `epochs`
    epochs, which EMPTIES the registry, so construct the scorer before the GAN's parameters - saved to PATH, and the run's
    `Generator.*` entries are removed.
    reference: a FeatureStatistics, or the path of a saved one (see set_reference): `score` and `score_generator` then also return
    the classifier Frechet distance to it, `'frechet'`.
    manifold: a FeatureSet, or the path of a saved one (see set_manifold), manifold_k: the neighbour count: `score` and `score_generator`
    then also return `'precision'`, `'recall'`, `'nn_dist'` and `'nn_zero'` against it (precision_recall).
    class_reference: a ClassStatistics, or the path of a saved one (see set_class_reference): `score` (with labels) and `score_generator`
    (of a conditional generator) then also return `'frechet_class'`, `'intra_frechet'`, `'n_class'`, `'confusion'` and `'acc_class'`.
    kernel_reference: a FeatureSet, or the path of a saved one (see set_kernel_reference), kernel_subset: the block size of the error
    bar (None: kernel_subset's rule): `score` and `score_generator` then also return `'kid'`, `'kid_std'` and `'kid_blocks'`
    (kernel_distance).
    class_manifold: a LABELLED FeatureSet, or the path of a saved one (see set_class_manifold), class_manifold_k: the neighbour count;
    class_kernel_reference: a labelled FeatureSet, or the path of a saved one (see set_class_kernel_reference): `score` (with labels) and
    `score_generator` (of a conditional generator) then also return the keys of class_precision_recall / class_kernel_distance."""

    def __init__(self, trainer=None, weights=None, data_dir=None, epochs=None, te=False, reference=None, manifold=None, manifold_k=3,
                 class_reference=None, kernel_reference=None, kernel_subset=None, class_manifold=None, class_manifold_k=3,
                 class_kernel_reference=None, **train_kw):
        if (trainer is None) == (weights is None):
            raise ValueError('ClassifierScore: pass a trainer or weights=PATH')
        self.trainer = trainer
        if trainer is None:
            if os.path.isfile(weights):
                self._load(weights)
            else:
                if data_dir is None and train_kw.get('arrays') is None:
                    raise ValueError('ClassifierScore: no checkpoint at %s - pass data_dir= (the CIFAR-10 python batches) to train' % weights)
                self._train(weights, data_dir, epochs, te, train_kw)
        self.cfg = ct_cifar.cfg
        if self.cfg.N_CLASSES > MAX_CLASSES:
            raise ValueError('ClassifierScore: %d classes (the score kernels take at most %d)' % (self.cfg.N_CLASSES, MAX_CLASSES))
        self.dev = lib._dev()
        self.lut = torch.from_numpy(ct_cifar.byte_table()).to(self.dev)
        self._filters, self._version = {}, None
        self._fingerprint, self._fp_version = None, None
        self.reference = None
        if reference is not None:
            self.set_reference(reference)
        self.manifold, self.manifold_k = None, int(manifold_k)
        if manifold is not None:
            self.set_manifold(manifold, manifold_k)
        self.class_reference = None
        if class_reference is not None:
            self.set_class_reference(class_reference)
        self.set_kernel_reference(kernel_reference, kernel_subset)
        self.class_manifold, self.class_manifold_k = None, int(class_manifold_k)
        self.set_class_manifold(class_manifold, class_manifold_k)
        self.set_class_kernel_reference(class_kernel_reference)

    # ---- construction
    @staticmethod
    def _build_classifier():
        cfg = ct_cifar.cfg
        with torch.no_grad():
            ct_cifar._classifier(K.empty_cl(2, cfg.CHANNELS, cfg.IMG, cfg.IMG, lib._dev()).zero_(), deterministic=True)

    def _load(self, path):
        if [n for n, _ in lib.named_params_with_name('Classifier.') if n.startswith('Classifier.')]:
            raise ValueError('ClassifierScore: the registry already holds Classifier.* parameters')
        ck = torch.load(path, map_location='cpu', weights_only=False)
        sd = {n: v for n, v in ck['params'].items() if n.startswith('Classifier.')}
        avg = ck['d_opt'].get('avg')
        if not sd or avg is None:
            raise ValueError('ClassifierScore: %s holds no CT classifier with parameter averages' % path)
        self._build_classifier()
        named = lib.named_params_with_name('Classifier.')
        trained = lib.named_params_with_name('Classifier.', trainable_only=True)
        bad = [n for n, p in named if n not in sd or tuple(sd[n].shape) != tuple(p.shape)]
        if bad or len(named) != len(sd) or sum(p.numel() for _, p in trained) != avg.numel():
            lib.delete_params_with_name('Classifier.')
            raise ValueError("ClassifierScore: %s does not fit the classifier of ct_cifar's current Config (%s)" % (path, bad[:3]))
        lib.load_state_dict(sd, strict=False)
        off = 0
        with torch.no_grad():
            for _, p in trained:              # the optimizer's flat layout: the trained parameters in registry order
                p.copy_(avg[off:off + p.numel()].view(p.shape))
                off += p.numel()
        lib.bump_epoch('Classifier')

    def _train(self, path, data_dir, epochs, te, train_kw):
        from . import checkpoint
        mod = _module(te)
        tr = mod.train(data_dir, epochs=epochs, **train_kw)
        done = (mod.cfg.EPOCHS if epochs is None else epochs)
        checkpoint.save(path, tr, done, extra=tr.checkpoint_extra())
        with torch.no_grad():
            for p, (_, a) in zip(tr.d_opt.params, tr.d_opt.avg_views()):
                p.copy_(a)
        lib.delete_params_with_name('Generator.')
        lib.bump_epoch('Classifier')

    # ---- the reference of the Frechet distance
    def fingerprint(self):
        """sha256 over the names, shapes and values of the Classifier.* parameters as the averaged pass sees them.  Made again (one
        device -> host copy of the parameters) when the registry's parameter version moves; only a scorer with a reference asks."""
        version = lib.epoch('Classifier')
        if self._fingerprint is None or version != self._fp_version:
            avg = dict(self.trainer.d_opt.avg_views()) if self.trainer is not None else {}
            named = [(n, avg.get(n, p)) for n, p in lib.named_params_with_name('Classifier.') if n.startswith('Classifier.')]
            h = hashlib.sha256()
            for n, p in named:
                h.update(('%s%s;' % (n, tuple(p.shape))).encode())
            with torch.no_grad():
                h.update(torch.cat([p.detach().reshape(-1).float() for _, p in named]).cpu().numpy().tobytes())
            self._fingerprint, self._fp_version = h.hexdigest(), version
        return self._fingerprint

    def _check_reference(self, ref):
        if ref.classifier is None:
            raise ValueError('ClassifierScore: the reference statistics do not record the classifier they were computed under')
        if ref.classifier != self.fingerprint():
            raise ValueError('ClassifierScore: the reference statistics were computed under another classifier (%s..., this one is %s...)'
                             % (ref.classifier[:12], self.fingerprint()[:12]))
        if ref.mean.size != self.cfg.D_WIDTHS[-1]:
            raise ValueError('ClassifierScore: %d reference features, %d in the classifier' % (ref.mean.size, self.cfg.D_WIDTHS[-1]))

    def set_reference(self, stats_or_path):
        """The FeatureStatistics (or the path of a saved one; None: none) that `score` / `score_generator` measure the Frechet distance
        to.  It must have been computed under this classifier's averaged parameters - checked here and again at every scoring."""
        ref = stats_or_path
        if ref is not None and not isinstance(ref, FeatureStatistics):
            ref = FeatureStatistics.load(ref)
        if ref is not None:
            self._check_reference(ref)
        self.reference = ref

    # ---- the reference of the per-class Frechet distance
    def _check_class_reference(self, ref):
        if ref.classifier is None:
            raise ValueError('ClassifierScore: the class reference statistics do not record the classifier they were computed under')
        if ref.classifier != self.fingerprint():
            raise ValueError('ClassifierScore: the class reference statistics were computed under another classifier (%s..., this one is %s...)'
                             % (ref.classifier[:12], self.fingerprint()[:12]))
        if ref.width != self.cfg.D_WIDTHS[-1]:
            raise ValueError('ClassifierScore: %d class reference features, %d in the classifier' % (ref.width, self.cfg.D_WIDTHS[-1]))
        if ref.classes != self.cfg.N_CLASSES:
            raise ValueError('ClassifierScore: %d reference classes, %d in the classifier' % (ref.classes, self.cfg.N_CLASSES))

    def set_class_reference(self, stats_or_path):
        """The ClassStatistics (or the path of a saved one; None: none) that `score` / `score_generator` measure the per-class Frechet
        distance to.  It must have been computed under this classifier's averaged parameters, at its width and class count - checked
        here and again at every scoring."""
        ref = stats_or_path
        if ref is not None and not isinstance(ref, ClassStatistics):
            ref = ClassStatistics.load(ref)
        if ref is not None:
            self._check_class_reference(ref)
        self.class_reference = ref

    # ---- the manifold of precision and recall
    def _check_manifold(self, ref):
        if ref.classifier is None:
            raise ValueError('ClassifierScore: the manifold features do not record the classifier they were computed under')
        if ref.classifier != self.fingerprint():
            raise ValueError('ClassifierScore: the manifold features were computed under another classifier (%s..., this one is %s...)'
                             % (ref.classifier[:12], self.fingerprint()[:12]))
        if ref.width != self.cfg.D_WIDTHS[-1]:
            raise ValueError('ClassifierScore: %d manifold features, %d in the classifier' % (ref.width, self.cfg.D_WIDTHS[-1]))

    def set_manifold(self, features_or_path, k=None):
        """The FeatureSet (or the path of a saved one; None: none) that `score` / `score_generator` measure precision and recall
        against, with `k` neighbours (None: as it is).  It must have been computed under this classifier's averaged parameters and hold
        at least k + 1 rows - checked here and again at every scoring."""
        ref = features_or_path
        if ref is not None and not isinstance(ref, FeatureSet):
            ref = FeatureSet.load(ref)
        k = self.manifold_k if k is None else int(k)
        if k < 1 or k > K.KNN_MAX_K:
            raise ValueError('ClassifierScore: manifold_k = %d (1 to %d)' % (k, K.KNN_MAX_K))
        if ref is not None:
            self._check_manifold(ref)
            if ref.n < k + 1:
                raise ValueError('ClassifierScore: %d manifold rows have no %d-th other neighbour' % (ref.n, k))
        self.manifold, self.manifold_k = ref, k

    # ---- the reference of the kernel distance
    def _check_kernel_reference(self, ref):
        if ref.classifier is None:
            raise ValueError('ClassifierScore: the kernel reference features do not record the classifier they were computed under')
        if ref.classifier != self.fingerprint():
            raise ValueError('ClassifierScore: the kernel reference features were computed under another classifier (%s..., this one is %s...)'
                             % (ref.classifier[:12], self.fingerprint()[:12]))
        if ref.width != self.cfg.D_WIDTHS[-1]:
            raise ValueError('ClassifierScore: %d kernel reference features, %d in the classifier' % (ref.width, self.cfg.D_WIDTHS[-1]))

    def set_kernel_reference(self, features_or_path, subset=None):
        """The FeatureSet (or the path of a saved one; None: none) that `score` / `score_generator` measure the kernel distance to, with
        blocks of `subset` rows for its error bar (None: kernel_subset's rule at every scoring).  It must have been computed under this
        classifier's averaged parameters and hold at least 2 rows - checked here and again at every scoring.  Its own tile sums are
        computed at the first scoring unless it carries them (FeatureSet.kernel_tiles, saved with it)."""
        ref = features_or_path
        if ref is not None and not isinstance(ref, FeatureSet):
            ref = FeatureSet.load(ref)
        if subset is not None:
            kernel_subset(2, 2, subset)
        if ref is not None:
            self._check_kernel_reference(ref)
            if ref.n < 2:
                raise ValueError('ClassifierScore: a kernel reference of %d rows (at least 2)' % ref.n)
        self.kernel_reference, self.kernel_subset = ref, None if subset is None else int(subset)

    # ---- the labelled sets of the per-class precision, recall and kernel distance
    def _check_class_set(self, ref, what):
        if ref.labels is None:
            raise ValueError('ClassifierScore: the %s features have no labels' % what)
        if ref.classifier is None:
            raise ValueError('ClassifierScore: the %s features do not record the classifier they were computed under' % what)
        if ref.classifier != self.fingerprint():
            raise ValueError('ClassifierScore: the %s features were computed under another classifier (%s..., this one is %s...)'
                             % (what, ref.classifier[:12], self.fingerprint()[:12]))
        if ref.width != self.cfg.D_WIDTHS[-1]:
            raise ValueError('ClassifierScore: %d %s features, %d in the classifier' % (ref.width, what, self.cfg.D_WIDTHS[-1]))
        if ref.classes != self.cfg.N_CLASSES:
            raise ValueError('ClassifierScore: %d %s classes, %d in the classifier' % (ref.classes, what, self.cfg.N_CLASSES))

    def set_class_manifold(self, features_or_path, k=None):
        """The LABELLED FeatureSet (or the path of a saved one; None: none) that `score` / `score_generator` measure the per-class precision
        and recall against (class_precision_recall), with `k` neighbours (None: as it is).  It must have been computed under this
        classifier's averaged parameters, at its width and class count - checked here and again at every scoring."""
        ref = features_or_path
        if ref is not None and not isinstance(ref, FeatureSet):
            ref = FeatureSet.load(ref)
        k = self.class_manifold_k if k is None else int(k)
        if k < 1 or k > K.KNN_MAX_K:
            raise ValueError('ClassifierScore: class_manifold_k = %d (1 to %d)' % (k, K.KNN_MAX_K))
        if ref is not None:
            self._check_class_set(ref, 'class manifold')
        self.class_manifold, self.class_manifold_k = ref, k

    def set_class_kernel_reference(self, features_or_path):
        """The LABELLED FeatureSet (or the path of a saved one; None: none) that `score` / `score_generator` measure the per-class kernel
        distance to (class_kernel_distance), under the checks of set_class_manifold.  Its own per-class totals are computed at the first
        scoring unless it carries them (FeatureSet.class_kernel_totals, saved with it)."""
        ref = features_or_path
        if ref is not None and not isinstance(ref, FeatureSet):
            ref = FeatureSet.load(ref)
        if ref is not None:
            self._check_class_set(ref, 'class kernel reference')
        self.class_kernel_reference = ref

    # ---- samples in internal form -> logits
    def _forward(self, x, features=False):
        """-> logits [m, K]; features: (logits, the pooled features [m, D]) of the same pass."""
        version = lib.epoch('Classifier')
        if version != self._version:        # (the version also counts registry-wide bumps: a GAN that trains makes every scoring renormalise once)
            self._filters.clear()
            self._version = version

        def run():
            with _wn.constant_filters(self._filters):
                return ct_cifar._classifier(x, deterministic=True, features='both' if features else False)

        if self.trainer is not None:
            out = self.trainer._averaged(run, True)
        else:
            with torch.no_grad():
                out = run()
        return (out[0].contiguous(), out[1].contiguous()) if features else out.contiguous()

    def _logits(self, x):
        return self._forward(x)

    # ---- the statistic
    def _begin(self, n, splits):
        nc = self.cfg.N_CLASSES
        if n < splits or splits < 1:
            raise ValueError('ClassifierScore: %d samples for %d splits' % (n, splits))
        return (torch.zeros(splits, nc + 1, dtype=torch.float64, device=self.dev), torch.zeros(2 * nc, dtype=torch.int64, device=self.dev))

    def _begin_moments(self):
        """The caller-owned state of kernels.moments_accum, s1 [D] and s2 [D, D] as views of one zeroed fp64 buffer."""
        d = self.cfg.D_WIDTHS[-1]
        buf = torch.zeros(d + d * d, dtype=torch.float64, device=self.dev)
        return buf, buf[:d], buf[d:].view(d, d)

    def _begin_class_moments(self):
        """The caller-owned state of kernels.class_moments_accum and kernels.confusion_accum: cnt [K] and conf [K, K] as views of one zeroed
        int64 buffer, s1 [K, D] and s2 [K, D, D] as views of one zeroed fp64 buffer."""
        k, d = self.cfg.N_CLASSES, self.cfg.D_WIDTHS[-1]
        ints = torch.zeros(k + k * k, dtype=torch.int64, device=self.dev)
        mom = torch.zeros(k * d + k * d * d, dtype=torch.float64, device=self.dev)
        return {'ints': ints, 'cnt': ints[:k], 'conf': ints[k:].view(k, k), 'mom': mom, 's1': mom[:k * d].view(k, d), 's2': mom[k * d:].view(k, d, d)}

    def _begin_class(self, with_labels, what):
        if self.class_reference is None:
            return None
        if not with_labels:
            raise ValueError('ClassifierScore.%s: a class reference is set and the samples have no labels' % what)
        self._check_class_reference(self.class_reference)
        return self._begin_class_moments()

    def _class_statistics(self, host_cnt, host_mom, n):
        k, d = self.cfg.N_CLASSES, self.cfg.D_WIDTHS[-1]
        cnt = np.asarray(host_cnt).astype(np.int64)
        if int(cnt.sum()) != n:
            raise ValueError('ClassifierScore: %d of %d rows have a label in [0, %d)' % (int(cnt.sum()), n, k))
        return ClassStatistics.from_moments(cnt, host_mom[:k * d].reshape(k, d), host_mom[k * d:].reshape(k, d, d), self.fingerprint())

    def _statistics(self, host, n):
        d = self.cfg.D_WIDTHS[-1]
        return FeatureStatistics.from_moments(n, host[:d], host[d:].reshape(d, d), self.fingerprint())

    def _finish(self, acc, cnt, n, splits, with_labels, moments=None, man=None, cls=None, ker=None, cset=None):
        nc = self.cfg.N_CLASSES
        out = K.score_finish(acc, n, splits)
        parts = [out, cnt.to(torch.float64)] + ([] if moments is None else [moments])
        if cls is not None:
            parts += [cls['ints'].to(torch.float64), cls['mom']]
        if ker is not None:                                  # two launches over all n samples, once, after the last chunk
            ref, feat = self.kernel_reference, ker['feat']
            parts.append(_kernel_values(K.kernel_tile_sums(feat, feat, exclude_diag=True), ref.kernel_tiles(),
                                        K.kernel_tile_sums(feat, ref.device_features()), n, ref.n, ker['subset']))
            tail = parts[-1].numel()
        if man is not None:                                  # three launches over all n samples, once, after the last chunk
            parts.append(_manifold_counts(man['feat'], self.manifold, self.manifold_k))
        if cset is not None:                                 # the grouped launches over all n samples, once, after the last chunk
            perm, seg = K.class_segments(cset['lab'], nc)
            feat = cset['feat'].index_select(0, perm)
            if self.class_manifold is not None:
                parts.append(_class_manifold_values(feat, seg, self.class_manifold, self.class_manifold_k))
            if self.class_kernel_reference is not None:
                own = K.segment_sums(*K.kernel_tile_sums_seg(feat, seg, feat, seg, exclude_diag=True))
                parts.append(_class_kernel_values(feat, seg, own, self.class_kernel_reference))
        host = torch.cat(parts).cpu().numpy()                # the scoring's one device -> host copy (counts < 2^53: exact)
        extra = {}
        if cset is not None:
            if self.class_kernel_reference is not None:
                extra.update(_class_kernel_result(host[-5 * nc:], nc))
                host = host[:-5 * nc]
            if self.class_manifold is not None:
                extra.update(_class_manifold_result(host[-7 * nc:], nc, self.class_manifold_k))
                del extra['k']
                host = host[:-7 * nc]
            if int(extra['n_class'].sum()) != n:
                raise ValueError('ClassifierScore: %d of %d rows have a label in [0, %d)' % (int(extra['n_class'].sum()), n, nc))
        counts = host[2 + splits:2 + splits + 2 * nc].astype(np.int64)
        res = {'mean': float(host[0]), 'std': float(host[1]), 'splits': host[2:2 + splits].copy(), 'hist': counts[:nc].copy(),
               'acc': float(counts[nc:].sum()) / n if with_labels else None}
        if moments is not None:
            res['frechet'] = frechet_distance(self._statistics(host[2 + splits + 2 * nc:2 + splits + 2 * nc + moments.numel()], n), self.reference)
        if cls is not None:
            at = 2 + splits + 2 * nc + (0 if moments is None else moments.numel())
            ints = host[at:at + nc + nc * nc].astype(np.int64)
            stats = self._class_statistics(ints[:nc], host[at + nc + nc * nc:at + nc + nc * nc + cls['mom'].numel()], n)
            res.update(intra_frechet(stats, self.class_reference))
            conf = ints[nc:].reshape(nc, nc)
            rows = conf.sum(axis=1)
            res.update({'n_class': stats.n.copy(), 'confusion': conf,
                        'acc_class': np.where(rows > 0, np.diag(conf) / np.maximum(rows, 1), np.nan)})
        if man is not None:
            res.update(_manifold_result(host[-5:], n, self.manifold.n, self.manifold_k))
            del res['k']
            host = host[:-5]
        if ker is not None:
            res.update(_kernel_result(host[-tail:], ker['subset']))
            del res['subset']
        res.update(extra)
        return res

    def _score_chunk(self, x, mom, man=None, r0=0, cls=None, lab=None, ker=None, cset=None):
        """One classifier pass -> logits; with the moment state of a scoring that has a reference, the pass's features go into it; with
        the state of one that has a manifold, they are copied to rows r0.. of its buffer; with the state of one that has a class reference,
        the features go into the state of their label `lab` and the logits into the confusion matrix; the state of one that has a kernel
        reference holds the manifold's buffer when there is one: one copy serves both; the state of one that has a class manifold
        or a class kernel reference shares that buffer too and keeps the labels."""
        man = ker if man is None else man
        if cset is not None:
            cset['lab'][r0:r0 + lab.shape[0]].copy_(lab)
            man = cset if man is None else man
        if mom is None and man is None and cls is None:
            return self._logits(x)
        logits, feat = self._forward(x, True)
        if cls is not None:
            K.class_moments_accum(feat, lab, cls['cnt'], cls['s1'], cls['s2'])
            K.confusion_accum(logits, lab, cls['conf'])
        if mom is not None:
            K.moments_accum(feat, mom[1], mom[2])
        if man is not None:
            man['feat'][r0:r0 + feat.shape[0]].copy_(feat)
        return logits

    def _begin_manifold(self, n):
        """The state of a scoring with a manifold: the one [n, D] device buffer the chunks' features are copied into."""
        if self.manifold is None:
            return None
        if n < self.manifold_k + 1:
            raise ValueError('ClassifierScore: %d samples have no %d-th other neighbour' % (n, self.manifold_k))
        self._check_manifold(self.manifold)
        return {'feat': torch.empty(n, self.cfg.D_WIDTHS[-1], dtype=torch.float32, device=self.dev)}

    def _begin_kernel(self, n, man):
        """The state of a scoring with a kernel reference: the block size and the [n, D] device buffer of the chunks' features - the
        manifold's when there is one."""
        ref = self.kernel_reference
        if ref is None:
            return None
        if n < 2:
            raise ValueError('ClassifierScore: the kernel distance needs at least 2 samples')
        self._check_kernel_reference(ref)
        feat = man['feat'] if man is not None else torch.empty(n, self.cfg.D_WIDTHS[-1], dtype=torch.float32, device=self.dev)
        return {'feat': feat, 'subset': kernel_subset(n, ref.n, self.kernel_subset)}

    def _begin_class_sets(self, n, with_labels, what, shared):
        """The state of a scoring with a class manifold or a class kernel reference: the [n, D] buffer of the chunks' features - the
        manifold's or the kernel reference's when there is one - and the [n] labels."""
        if self.class_manifold is None and self.class_kernel_reference is None:
            return None
        if not with_labels:
            raise ValueError('ClassifierScore.%s: a class manifold or class kernel reference is set and the samples have no labels' % what)
        for ref, name in ((self.class_manifold, 'class manifold'), (self.class_kernel_reference, 'class kernel reference')):
            if ref is not None:
                self._check_class_set(ref, name)
        feat = shared['feat'] if shared is not None else torch.empty(n, self.cfg.D_WIDTHS[-1], dtype=torch.float32, device=self.dev)
        return {'feat': feat, 'lab': torch.empty(n, dtype=torch.int32, device=self.dev)}

    def _begin_frechet(self, n):
        if self.reference is None:
            return None
        if n < 2:
            raise ValueError('ClassifierScore: the Frechet distance needs at least 2 samples')
        self._check_reference(self.reference)
        return self._begin_moments()

    def _labels(self, labels, n):
        if labels is None:
            return None
        t = torch.as_tensor(labels).reshape(-1)
        if t.numel() != n:
            raise ValueError('ClassifierScore: %d labels for %d samples' % (t.numel(), n))
        return t.to(device=self.dev, dtype=torch.int32).contiguous()

    def score(self, images_u8, labels=None, splits=10, chunk=None):
        """The score of a uint8 set [N, CHANNELS, IMG, IMG] (the reference's orientation, as CifarSSLData holds it), read through
        kernels.aug_gather's fixed mode in chunks of `chunk` rows (None: min(1000, N)); labels [N]: also the accuracy.
        -> {'mean', 'std', 'splits' [splits], 'hist' [K] predicted-class counts, 'acc' (None without labels)}, and with a reference
        set 'frechet', the classifier Frechet distance of the set's features to it, and with a manifold set 'precision', 'recall',
        'nn_dist' and 'nn_zero' (precision_recall) of them against it, and with a kernel reference set 'kid', 'kid_std' and 'kid_blocks'
        (kernel_distance) of them against it."""
        cfg = self.cfg
        data = torch.as_tensor(images_u8)
        if data.dtype != torch.uint8 or data.dim() != 4 or tuple(data.shape[1:]) != (cfg.CHANNELS, cfg.IMG, cfg.IMG):
            raise ValueError('ClassifierScore.score: uint8 [N, %d, %d, %d] images expected (got %s %s)'
                             % (cfg.CHANNELS, cfg.IMG, cfg.IMG, data.dtype, tuple(data.shape)))
        n = data.shape[0]
        cls = self._begin_class(labels is not None, 'score')
        acc, cnt = self._begin(n, splits)
        mom = self._begin_frechet(n)
        man = self._begin_manifold(n)
        ker = self._begin_kernel(n, man)
        cset = self._begin_class_sets(n, labels is not None, 'score', ker if man is None else man)
        data = data.to(self.dev).contiguous()
        labels = self._labels(labels, n)
        chunk = min(DEFAULT_CHUNK, n) if chunk is None else int(chunk)
        if chunk < 1:
            raise ValueError('ClassifierScore.score: chunk must be positive')
        for r0 in range(0, n, chunk):
            m = min(chunk, n - r0)
            idx = torch.arange(r0, r0 + m, dtype=torch.int32, device=self.dev)
            lab = None if labels is None else labels[r0:r0 + m]
            logits = self._score_chunk(K.aug_gather(data, idx, self.lut, cfg.IMG, cfg.PAD), mom, man, r0, cls, lab, ker, cset)
            K.score_accum(logits, r0, n, splits, acc, cnt, lab)
        return self._finish(acc, cnt, n, splits, labels is not None, None if mom is None else mom[0], man, cls, ker, cset)

    def score_generator(self, gan_trainer, n, labels=None, splits=10, chunk=None, averaged=False):
        """The score of `n` samples of a gan_cifar / gan_cifar_resnet trainer's generator, drawn exactly as evaluate.Evaluator.score_samples
        draws them - on the trainer's EVALUATION stream, in statistic groups of 100, `chunk` (a multiple of 100; None: 1000) per
        generator call, the ResNet's labels drawn there unless given - and quantised with the script's SCORE_SCALE as the saved pixels
        are: the training stream, the weights and the optimizers stay untouched.  The ResNet's labels feed the accuracy count.  With a
        reference set the result also holds 'frechet', with a manifold set 'precision', 'recall', 'nn_dist' and 'nn_zero', with a kernel
        reference set 'kid', 'kid_std' and 'kid_blocks', all from the features of the same classifier passes.  averaged (NOT in the reference):
        the samples come from the generator's weight average (the trainer's `averaged()`; ValueError when it keeps none)."""
        ev, scale = self._evaluator(gan_trainer, 'score_generator')
        cfg = self.cfg
        cls = self._begin_class(ev.resnet, 'score_generator')      # (only the ResNet's generator is conditional: score_draws yields its labels)
        acc, cnt = self._begin(n, splits)
        mom = self._begin_frechet(n)
        man = self._begin_manifold(n)
        ker = self._begin_kernel(n, man)
        cset = self._begin_class_sets(n, ev.resnet, 'score_generator', ker if man is None else man)
        labels = self._labels(labels, n)
        r0, with_labels = 0, False
        for x, lab in ev.score_draws(n, labels, chunk, **_avg_kw(averaged)):
            lab = None if lab is None else lab.contiguous()
            logits = self._score_chunk(K.score_input(x, cfg.CHANNELS, scale, self.lut), mom, man, r0, cls, lab, ker, cset)
            K.score_accum(logits, r0, n, splits, acc, cnt, lab)
            with_labels = lab is not None
            r0 += x.shape[0]
        return self._finish(acc, cnt, n, splits, with_labels, None if mom is None else mom[0], man, cls, ker, cset)

    def _evaluator(self, gan_trainer, what):
        from . import evaluate
        ev = evaluate.Evaluator(gan_trainer)
        cfg = self.cfg
        if ev.name not in evaluate.SCORE_SCALE or ev.mod.cfg.OUTPUT_DIM != cfg.CHANNELS * cfg.IMG * cfg.IMG:
            raise ValueError('ClassifierScore.%s: %s samples are not %dx%dx%d images' % (what, ev.name, cfg.CHANNELS, cfg.IMG, cfg.IMG))
        return ev, evaluate.SCORE_SCALE[ev.name]

    # ---- the feature statistics alone
    def statistics(self, images_u8, chunk=None):
        """The FeatureStatistics of a uint8 set [N, CHANNELS, IMG, IMG], read exactly as `score` reads it: what a reference is made of
        (the training images, once; `.save(path)` keeps it)."""
        cfg = self.cfg
        data = torch.as_tensor(images_u8)
        if data.dtype != torch.uint8 or data.dim() != 4 or tuple(data.shape[1:]) != (cfg.CHANNELS, cfg.IMG, cfg.IMG):
            raise ValueError('ClassifierScore.statistics: uint8 [N, %d, %d, %d] images expected (got %s %s)'
                             % (cfg.CHANNELS, cfg.IMG, cfg.IMG, data.dtype, tuple(data.shape)))
        n = data.shape[0]
        if n < 1:
            raise ValueError('ClassifierScore.statistics: no images')
        buf, s1, s2 = self._begin_moments()
        data = data.to(self.dev).contiguous()
        chunk = min(DEFAULT_CHUNK, n) if chunk is None else int(chunk)
        if chunk < 1:
            raise ValueError('ClassifierScore.statistics: chunk must be positive')
        for r0 in range(0, n, chunk):
            idx = torch.arange(r0, min(r0 + chunk, n), dtype=torch.int32, device=self.dev)
            K.moments_accum(self._forward(K.aug_gather(data, idx, self.lut, cfg.IMG, cfg.PAD), True)[1], s1, s2)
        return self._statistics(buf.cpu().numpy(), n)

    def statistics_generator(self, gan_trainer, n, labels=None, chunk=None, averaged=False):
        """The FeatureStatistics of `n` generator samples, drawn and quantised exactly as `score_generator` draws them (the evaluation
        stream; the training stream, the weights and the optimizers stay untouched)."""
        ev, scale = self._evaluator(gan_trainer, 'statistics_generator')
        if n < 1:
            raise ValueError('ClassifierScore.statistics_generator: no samples')
        buf, s1, s2 = self._begin_moments()
        for x, _ in ev.score_draws(n, self._labels(labels, n), chunk, **_avg_kw(averaged)):
            K.moments_accum(self._forward(K.score_input(x, self.cfg.CHANNELS, scale, self.lut), True)[1], s1, s2)
        return self._statistics(buf.cpu().numpy(), n)

    # ---- the per-class feature statistics alone
    def class_statistics(self, images_u8, labels, chunk=None):
        """The ClassStatistics of a labelled uint8 set [N, CHANNELS, IMG, IMG], labels [N] in [0, N_CLASSES), read exactly as `statistics`
        reads it: what a class reference is made of (the labelled training images, once; `.save(path)` keeps it)."""
        cfg = self.cfg
        data = torch.as_tensor(images_u8)
        if data.dtype != torch.uint8 or data.dim() != 4 or tuple(data.shape[1:]) != (cfg.CHANNELS, cfg.IMG, cfg.IMG):
            raise ValueError('ClassifierScore.class_statistics: uint8 [N, %d, %d, %d] images expected (got %s %s)'
                             % (cfg.CHANNELS, cfg.IMG, cfg.IMG, data.dtype, tuple(data.shape)))
        n = data.shape[0]
        if n < 1 or labels is None:
            raise ValueError('ClassifierScore.class_statistics: no images, or no labels')
        labels = self._labels(labels, n)
        st = self._begin_class_moments()
        data = data.to(self.dev).contiguous()
        chunk = min(DEFAULT_CHUNK, n) if chunk is None else int(chunk)
        if chunk < 1:
            raise ValueError('ClassifierScore.class_statistics: chunk must be positive')
        for r0 in range(0, n, chunk):
            idx = torch.arange(r0, min(r0 + chunk, n), dtype=torch.int32, device=self.dev)
            feat = self._forward(K.aug_gather(data, idx, self.lut, cfg.IMG, cfg.PAD), True)[1]
            K.class_moments_accum(feat, labels[r0:r0 + chunk], st['cnt'], st['s1'], st['s2'])
        return self._class_statistics(st['cnt'].cpu().numpy(), st['mom'].cpu().numpy(), n)

    def class_statistics_generator(self, gan_trainer, n, labels=None, chunk=None, averaged=False):
        """The ClassStatistics of `n` samples of a conditional generator under the labels they were generated from, drawn and quantised
        exactly as `statistics_generator` draws them (the evaluation stream; the training stream, the weights and the optimizers stay
        untouched).  An unconditional generator's samples have no labels: ValueError."""
        ev, scale = self._evaluator(gan_trainer, 'class_statistics_generator')
        if n < 1:
            raise ValueError('ClassifierScore.class_statistics_generator: no samples')
        if not ev.resnet:
            raise ValueError('ClassifierScore.class_statistics_generator: %s samples have no labels' % ev.name)
        st = self._begin_class_moments()
        for x, lab in ev.score_draws(n, self._labels(labels, n), chunk, **_avg_kw(averaged)):
            feat = self._forward(K.score_input(x, self.cfg.CHANNELS, scale, self.lut), True)[1]
            K.class_moments_accum(feat, lab.contiguous(), st['cnt'], st['s1'], st['s2'])
        return self._class_statistics(st['cnt'].cpu().numpy(), st['mom'].cpu().numpy(), n)

    # ---- the features themselves
    def features(self, images_u8, chunk=None, labels=None):
        """The FeatureSet of a uint8 set [N, CHANNELS, IMG, IMG], read exactly as `statistics` reads it: what a manifold is made of (the
        training images, once; `.save(path)` keeps it with its radii).  labels [N]: a labelled set of N_CLASSES classes - what a class
        manifold or a class kernel reference is made of."""
        cfg = self.cfg
        data = torch.as_tensor(images_u8)
        if data.dtype != torch.uint8 or data.dim() != 4 or tuple(data.shape[1:]) != (cfg.CHANNELS, cfg.IMG, cfg.IMG):
            raise ValueError('ClassifierScore.features: uint8 [N, %d, %d, %d] images expected (got %s %s)'
                             % (cfg.CHANNELS, cfg.IMG, cfg.IMG, data.dtype, tuple(data.shape)))
        n = data.shape[0]
        if n < 1:
            raise ValueError('ClassifierScore.features: no images')
        out = torch.empty(n, cfg.D_WIDTHS[-1], dtype=torch.float32, device=self.dev)
        data = data.to(self.dev).contiguous()
        chunk = min(DEFAULT_CHUNK, n) if chunk is None else int(chunk)
        if chunk < 1:
            raise ValueError('ClassifierScore.features: chunk must be positive')
        for r0 in range(0, n, chunk):
            idx = torch.arange(r0, min(r0 + chunk, n), dtype=torch.int32, device=self.dev)
            out[r0:r0 + chunk].copy_(self._forward(K.aug_gather(data, idx, self.lut, cfg.IMG, cfg.PAD), True)[1])
        if labels is not None:
            return FeatureSet(out, self.fingerprint(), labels=self._labels(labels, n), classes=cfg.N_CLASSES)
        return FeatureSet(out, self.fingerprint())

    def features_generator(self, gan_trainer, n, labels=None, chunk=None, averaged=False):
        """The FeatureSet of `n` generator samples, drawn and quantised exactly as `statistics_generator` draws them (the evaluation
        stream; the training stream, the weights and the optimizers stay untouched).  A conditional generator's samples carry the labels
        they were generated from: a labelled set."""
        ev, scale = self._evaluator(gan_trainer, 'features_generator')
        if n < 1:
            raise ValueError('ClassifierScore.features_generator: no samples')
        out = torch.empty(n, self.cfg.D_WIDTHS[-1], dtype=torch.float32, device=self.dev)
        r0, labs = 0, []
        for x, lab in ev.score_draws(n, self._labels(labels, n), chunk, **_avg_kw(averaged)):
            out[r0:r0 + x.shape[0]].copy_(self._forward(K.score_input(x, self.cfg.CHANNELS, scale, self.lut), True)[1])
            r0 += x.shape[0]
            if lab is not None:
                labs.append(lab.reshape(-1).to(torch.int32))
        if labs:
            return FeatureSet(out, self.fingerprint(), labels=torch.cat(labs), classes=self.cfg.N_CLASSES)
        return FeatureSet(out, self.fingerprint())
