"""TEST-ONLY fp64 restatement (numpy) of the classifier Frechet distance of ctgan_amd.score_cifar: the two-pass (centred) mean and
covariance of a feature array, the distance formula written independently of score_cifar.frechet_distance, and the error bounds the
tests hold the device path to.  Nothing under ctgan_amd/ imports this file.

The bounds.  u = 2^-53 is the unit roundoff of fp64.  A sum of n terms t_i in ANY order has error <= (n - 1) u sum |t_i| (to first
order; Higham, Accuracy and Stability of Numerical Algorithms, section 4.2).  The products f_ia f_ib of two fp32 values are exact in
fp64, so the raw moments have no other error and
    |s2 - exact| <= n 2^-52 (|F|^T |F|)  elementwise,      |s1 - exact| <= n 2^-52 sum_i |f_i|
hold with a factor 2 to spare, for the kernel's order, for numpy's, and for the chunked accumulation into the state.  `moment_bound`
returns the two right-hand sides.  The references they are measured against are exact (math.fsum) on a corner block and numpy's fp64
f.T @ f elsewhere, whose own error is within half of the same bound."""
import math

import numpy as np

EPS = 2.0 ** -52


def gaussian_features(n, d, seed=0, offset=0.0):
    """fp32 [n, d]: Gaussian rows through a well-conditioned mixing matrix (orthogonal times scales in [0.5, 2]), plus `offset`."""
    r = np.random.RandomState(seed)
    q, _ = np.linalg.qr(r.randn(d, d))
    mix = q * np.linspace(0.5, 2.0, d)
    return (r.randn(n, d) @ mix.T + offset + 0.1 * r.randn(d)).astype(np.float32)


def two_pass_statistics(f):
    """(n, mean [D], unbiased covariance [D, D]) of fp32 features in fp64: the mean first, then the centred second moment."""
    f = np.asarray(f, dtype=np.float64)
    n = f.shape[0]
    mean = f.sum(axis=0) / n
    c = f - mean
    return n, mean, (c.T @ c) / (n - 1)


def psd_root(a):
    w, v = np.linalg.eigh(a)
    return v @ np.diag(np.sqrt(np.clip(w, 0.0, None))) @ v.T


def product_eigenvalues(cov_a, cov_b):
    """Eigenvalues (ascending) of the symmetrised A^1/2 B A^1/2."""
    r = psd_root(cov_a)
    m = r @ cov_b @ r
    return np.linalg.eigvalsh(0.5 * (m + m.T))


def distance(mean_a, cov_a, mean_b, cov_b):
    lam = product_eigenvalues(cov_a, cov_b)
    d = np.asarray(mean_a) - np.asarray(mean_b)
    return float(np.dot(d, d) + np.trace(cov_a) + np.trace(cov_b) - 2.0 * np.sqrt(np.clip(lam, 0.0, None)).sum())


def features_distance(fa, fb):
    _, ma, ca = two_pass_statistics(fa)
    _, mb, cb = two_pass_statistics(fb)
    return distance(ma, ca, mb, cb)


# ------------------------------------------------------------------------------------------------ raw moments and their bound
def reference_moments(f, corner=6):
    """(s1 [D], s2 [D, D]) of fp32 features in fp64: numpy's sums, with the leading `corner` entries / `corner` x `corner` block
    replaced by the exactly rounded sums (math.fsum over the exact products)."""
    f = np.asarray(f, dtype=np.float64)
    s1, s2 = f.sum(axis=0), f.T @ f
    c = min(corner, f.shape[1])
    for a in range(c):
        s1[a] = math.fsum(f[:, a])
        for b in range(c):
            s2[a, b] = math.fsum(f[:, a] * f[:, b])
    return s1, s2


def moment_bound(f):
    """(bound on |s1 - ref| [D], bound on |s2 - ref| [D, D]): n 2^-52 sum |f|, n 2^-52 |F|^T |F|."""
    g = np.abs(np.asarray(f, dtype=np.float64))
    n = g.shape[0]
    return n * EPS * g.sum(axis=0), n * EPS * (g.T @ g)


def statistics_bound(f):
    """(bound on |mean - two-pass mean| [D], bound on |cov - two-pass cov| [D, D]) for mean = s1 / n, cov = (s2 - n mean mean^T) /
    (n - 1) formed in fp64 from raw moments within `moment_bound`: the moment bounds propagated through the two formulas
        d mean <= b1 / n + EPS |mean|
        d cov  <= [b2 + n (d mean |mean|^T + |mean| d mean^T + d mean d mean^T) + 4 EPS (|s2| + n |mean| |mean|^T)] / (n - 1)
    (the last term: the roundings of the outer product, the scaling, the subtraction and the division), plus the two-pass side's own
    summation error, within n EPS |C|^T |C| / (n - 1) on the centred rows C."""
    f = np.asarray(f, dtype=np.float64)
    n = f.shape[0]
    b1, b2 = moment_bound(f)
    mean = np.abs(f.sum(axis=0) / n)
    dmean = b1 / n + EPS * mean
    c = np.abs(f - f.sum(axis=0) / n)
    s2 = np.abs(f).T @ np.abs(f)
    mm = np.outer(mean, mean)
    dcov = (b2 + n * (np.outer(dmean, mean) + np.outer(mean, dmean) + np.outer(dmean, dmean)) + 4 * EPS * (s2 + n * mm) + n * EPS * (c.T @ c)) / (n - 1)
    return dmean, dcov


def _root_change(dnorm, lam_min):
    """||A^1/2 - B^1/2|| for PSD A, B with ||A - B|| <= dnorm: <= dnorm / (2 sqrt(lambda_min)) to first order (doubled here for the
    higher orders), and never more than sqrt(dnorm) (the square root is operator monotone), which also covers a singular matrix."""
    first = 2.0 * dnorm / (2.0 * math.sqrt(lam_min)) if lam_min > 0 else math.inf
    return min(first, math.sqrt(dnorm))


def distance_tolerance(fa, fb):
    """A bound on |frechet_distance(statistics from raw moments) - features_distance(fa, fb)| from `statistics_bound` on both sides and
    the oracle's own eigenvalues.  With M = A^1/2 B A^1/2 (A, B the covariances, D wide):
        |d tr sqrt(M)| <= D ||dM|| / (2 sqrt(lambda_min(M)))         (and <= D sqrt(||dM||) in any case)
        ||dM|| <= 2 ||d A^1/2|| ||B|| ||A^1/2|| + ||A|| ||dB||,        ||d A^1/2|| from _root_change
    with Frobenius norms of the elementwise bounds standing in for the spectral norms of the changes; the mean term changes by at most
    2 |mu_a - mu_b| |d mu| + |d mu|^2 and the traces by the traces of the covariance bounds.  Eigenvalue routines return results
    accurate to a few EPS ||M||: D^2 EPS ||M|| / sqrt(lambda_min) of slack covers both implementations' eigensolves."""
    _, ma, ca = two_pass_statistics(fa)
    _, mb, cb = two_pass_statistics(fb)
    dma, dca = statistics_bound(fa)
    dmb, dcb = statistics_bound(fb)
    D = ma.size
    dmu = float(np.linalg.norm(dma) + np.linalg.norm(dmb))
    mean_term = 2.0 * float(np.linalg.norm(ma - mb)) * dmu + dmu * dmu
    trace_term = float(np.trace(dca) + np.trace(dcb))
    la = np.linalg.eigvalsh(ca)
    lam = product_eigenvalues(ca, cb)
    na, nb = float(la[-1]), float(np.linalg.eigvalsh(cb)[-1])
    droot = _root_change(float(np.linalg.norm(dca)), float(la[0]))
    dM = 2.0 * droot * nb * math.sqrt(na) + na * float(np.linalg.norm(dcb)) + D * D * EPS * float(lam[-1])
    sqrt_term = 2.0 * D * _root_change(dM, float(lam[0]))
    return mean_term + trace_term + sqrt_term, {'lambda_min_product': float(lam[0]), 'lambda_min_a': float(la[0]), 'dM': dM}
