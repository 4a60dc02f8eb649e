"""fp64 numpy restatement of the k-nearest-neighbour manifold estimate (csrc/knn.hip, ctgan_amd.score_cifar.precision_recall); no torch.

Distances in the DIRECT form sum_k (a_ik - b_jk)^2 over the fp32 features widened to fp64 (two bit-identical rows: exactly 0), radii by a
stable sort with self excluded by index, coverage, the lowest-index nearest neighbour.

The bound on a device distance.  The device forms d2 = |a|^2 + |b|^2 - 2 a.b with exact products and fp64 sums of d terms each, in the
MFMA's own order; for any order a sum of d exact terms is within (d - 1) u sum |terms| of its value (u = 2^-53, first order), so with
Cauchy-Schwarz  |d2_dev - d2| <= (d - 1) u (|a|^2 + |b|^2 + 2 |a| |b|) + 2 u (...) for the two final operations
                               <= (d + 1) u (|a| + |b|)^2 < E(i, j) = (d + 4) 2^-52 (|a_i| + |b_j|)^2,
which leaves a factor of two and the direct form's own error ((d + 2) u d2 <= (d + 2) u (|a| + |b|)^2) inside.  `gemm_form` is the
same expression in numpy; the host test checks that it stays within 0.10 E of the direct form on the cases below.  A radius is one of
those distances and carries the bound of its own pair.  Two bit-identical rows are at exactly 0 on the device by contract (the three
chains are one and the same number), so the bound of such a pair is 0: the tests then ask for the exact 0, and a copy of a reference row
whose radius is 0 is decidably covered.

Coverage compares d2(i, j) with r2[j]; a row is DECIDABLE when some j has d2 - r2 <= -E' or every j has d2 - r2 > E', E' the bound of
the distance plus the bound of the radius: only then is the oracle's flag the one every implementation within the bounds must give.
"""
import numpy as np

KNN_MAX_K = 8
U52 = 2.0 ** -52

# (m, n, d, k, offset): one element; ...; row and column tails inside one tile; three column tiles with all the tails; exact tiles; one past
# a tile with KNN_MAX_K; the classifier's width; few owners and a long stream; many owners and a short stream
CASES = [(1, 2, 1, 1, 0.0), (3, 5, 1, 1, 0.0), (57, 70, 10, 3, 0.0), (301, 130, 33, 3, 0.0), (64, 64, 16, 1, 5.0), (65, 129, 17, 8, 5.0),
         (1000, 1000, 128, 3, 5.0), (130, 2100, 192, 5, 5.0), (2100, 130, 192, 5, 0.0)]
MULTI_ROW = [c for c in CASES if c[0] >= 57]
COPY_OF_B10 = 7        # the further row of `a` that is set to b[10] in the planted cases


def planted(m, n, d, k, offset):
    return d >= 128


def inputs(m, n, d, k, offset, seed=7):
    """-> (a fp32 [m, d], b fp32 [n, d]): b ~ N(offset, 1); a ~ s N(offset, 1) with s = 1.15 and a mean shift of 0.3 / sqrt(d) for
    d <= 33, s = 1.03 for d >= 128 - so that precision and recall are both strictly inside (0, 1).  In the planted (large) cases
    a[:5] = b[:5], b[10 .. 10 + k] = b[10] (k + 1 radii exactly 0) and a[COPY_OF_B10] = b[10]."""
    r = np.random.RandomState(seed)
    b = (offset + r.randn(n, d)).astype(np.float32)
    s = 1.15 if d <= 33 else 1.03
    a = s * (offset + r.randn(m, d))
    if d <= 33:
        a = a + 0.3 / np.sqrt(d)
    a = a.astype(np.float32)
    if planted(m, n, d, k, offset):
        b[10:10 + k + 1] = b[10]
        a[:5] = b[:5]
        a[COPY_OF_B10] = b[10]
    return a, b


def d2_direct(a, b):
    """fp64 [m, n]: sum_k (a_ik - b_jk)^2 (a few rows of `a` at a time: the [rows, n, d] differences stay near 8M elements)."""
    a64, b64 = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    out = np.empty((a64.shape[0], b64.shape[0]))
    rows = max(1, 8000000 // (b64.shape[0] * b64.shape[1]))
    for r0 in range(0, a64.shape[0], rows):
        diff = a64[r0:r0 + rows, None, :] - b64[None, :, :]
        out[r0:r0 + rows] = np.einsum('ijk,ijk->ij', diff, diff)
    return out


def gemm_form(a, b):
    """max(0, |a|^2 + |b|^2 - 2 a.b) in fp64 numpy: the device's expression in numpy's summation order."""
    a64, b64 = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    na, nb = (a64 * a64).sum(axis=1), (b64 * b64).sum(axis=1)
    return np.maximum(0.0, (na[:, None] + nb[None, :]) - 2.0 * (a64 @ b64.T))


def bound(a, b, dist=None):
    """E [m, n] = (d + 4) 2^-52 (|a_i| + |b_j|)^2, and 0 for a pair of identical rows (dist: d2_direct(a, b) if already at hand)."""
    a64, b64 = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    na, nb = np.sqrt((a64 * a64).sum(axis=1)), np.sqrt((b64 * b64).sum(axis=1))
    e = (a.shape[1] + 4) * U52 * (na[:, None] + nb[None, :]) ** 2
    e[(d2_direct(a, b) if dist is None else dist) == 0] = 0.0
    return e


def first_copy(f):
    """[n]: for every row the lowest index of a row identical to it."""
    _, first, inverse = np.unique(np.asarray(f), axis=0, return_index=True, return_inverse=True)
    return first[np.asarray(inverse).reshape(-1)]


def radii(f, k):
    """-> (r2 fp64 [n], the bound of each radius' own pair): the k-th smallest distance to another row, self excluded by INDEX, by a
    stable sort (ties: the lowest index first - immaterial for the value)."""
    n = f.shape[0]
    assert 1 <= k <= n - 1
    dist = d2_direct(f, f)
    e = bound(f, f, dist)
    dist[np.arange(n), np.arange(n)] = np.inf
    order = np.argsort(dist, axis=1, kind='stable')[:, k - 1]
    rows = np.arange(n)
    return dist[rows, order], e[rows, order]


def nearest(dist):
    """-> (nn_d2, nn_idx): the minimum of every row and the LOWEST index attaining it."""
    idx = dist.argmin(axis=1)
    return dist[np.arange(dist.shape[0]), idx], idx


def cover(dist, r2):
    return (dist <= r2[None, :]).any(axis=1)


def decidable(dist, r2, e_dist, e_r2):
    margin = e_dist + e_r2[None, :]
    diff = dist - r2[None, :]
    return (diff <= -margin).any(axis=1) | (diff > margin).all(axis=1)


def nearest_is_unambiguous(dist, e_dist, b):
    """Rows whose runner-up is more than the two pairs' bounds (2 E) above the minimum: the index is then the same for every
    implementation within the bounds.  Rows of b identical to the nearest one are no runners-up: their distances are the same bits, and
    the lowest-index rule decides among them."""
    m = dist.shape[0]
    nn, idx = nearest(dist)
    gap = dist - nn[:, None] - (e_dist + e_dist[np.arange(m), idx][:, None])
    copy = first_copy(b)
    gap[copy[None, :] == copy[idx][:, None]] = np.inf
    return (gap > 0).all(axis=1)


class Case:
    """Everything the tests compare against for one (m, n, d, k, offset), computed once."""

    def __init__(self, m, n, d, k, offset, seed=7):
        self.shape = (m, n, d, k, offset)
        self.k = k
        self.a, self.b = inputs(m, n, d, k, offset, seed)
        self.planted = planted(m, n, d, k, offset)
        self.dist = d2_direct(self.a, self.b)
        self.e_dist = bound(self.a, self.b, self.dist)
        self.r2_b, self.e_r2_b = radii(self.b, k)
        self.covered = cover(self.dist, self.r2_b)
        self.decidable = decidable(self.dist, self.r2_b, self.e_dist, self.e_r2_b)
        self.nn_d2, self.nn_idx = nearest(self.dist)
        self.e_nn = self.e_dist[np.arange(m), self.nn_idx]
        self.nn_sure = nearest_is_unambiguous(self.dist, self.e_dist, self.b)
        if m >= k + 1:                                   # the other direction: recall
            self.r2_a, self.e_r2_a = radii(self.a, k)
            self.back = cover(self.dist.T, self.r2_a)
            self.back_decidable = decidable(self.dist.T, self.r2_a, self.e_dist.T, self.e_r2_a)
        else:
            self.r2_a = self.e_r2_a = self.back = self.back_decidable = None

    @property
    def precision(self):
        return float(self.covered.mean())

    @property
    def recall(self):
        return None if self.back is None else float(self.back.mean())


_CACHE = {}


def case(*shape, seed=7):
    key = tuple(shape) + (seed,)
    if key not in _CACHE:
        _CACHE[key] = Case(*shape, seed=seed)
    return _CACHE[key]


def precision_recall(fa, fb, k):
    """The dict of ctgan_amd.score_cifar.precision_recall for sample features fa against reference features fb."""
    dist = d2_direct(fa, fb)
    nn, _ = nearest(dist)
    return {'precision': float(cover(dist, radii(fb, k)[0]).mean()), 'recall': float(cover(dist.T, radii(fa, k)[0]).mean()), 'k': k,
            'nn_dist': float(np.median(np.sqrt(nn))), 'nn_zero': int((nn == 0).sum())}
