"""fp64 numpy restatement of the unbiased kernel distance (csrc/kid.hip, ctgan_amd.score_cifar.kernel_distance); no torch.

The kernel values in the DIRECT form, in long double (x86: a 64-bit significand) from the fp32 features on: the dot products
sum_k a_ik b_jk (numpy's own loop: no BLAS there), v = gamma dot + coef0, k = (v v) v, the tile sums and every further total (math.fsum
checks the sums).  A product of two fp32 values is exact there and each of the few hundred roundings is 2^-11 of an fp64 one: what the
oracle adds to a bound is under a thousandth of it, and the bounds below budget for an fp64 oracle all the same.

The bounds, derived here and not tuned (u = 2^-53; first order in u, with the slack named):
  the dot.   The products of two widened fp32 values are exact in fp64.  A sum of d exact terms in ANY order is within (d - 1) u T of its
             value, T = sum_k |a_ik| |b_jk|.  The device's chain and the oracle's loop each stay inside that, so the two differ by at most
             2 (d - 1) u T = (d - 1) 2^-52 T < E_t = (d + 4) 2^-52 T, which leaves 10 u T.
  the cube.  v = fl(fl(gamma dot) + coef0) (or one fused operation) adds at most u |gamma dot| + u |v| per side: the first is inside the
             10 u T |gamma| left above, the second goes with the cube's two roundings, 2 u |v|^3, into (3 + 2) u |v|^3 per side,
             10 u |v|^3 < 8 2^-52 |v|^3 for both.  A perturbation e = |gamma| E_t of v moves v^3 by at most 3 (|v| + e)^2 e.  Hence
             E_k = 3 (|v| + |gamma| E_t)^2 |gamma| E_t + 8 2^-52 |v|^3                                            per pair.
  a tile.    The sum of its pairs' E_k, plus the device's summation of at most 4096 values in its fixed order, within
             4095 u sum |k| < 4096 2^-52 sum |k| (the oracle's long double sum adds 2^-11 of that).
  kid.       S / c with the tile bounds summed and divided by the same c, plus the device's fp64 reduction of T tile sums in an order
             of torch's choosing, (T - 1) u sum |tile sums|, and its handful of divisions and additions: (T + 8) 2^-53 sum |tile sums|
             / c per term of the formula.
`gemm_form` is the same kernel matrix through numpy's BLAS product; the host test checks that at d = 128 it stays within 0.06 E_k of the
direct form on every pair.
"""
import math

import numpy as np

TILE = 64
U52 = 2.0 ** -52

# (m, n, d, exclude_diag): one element; one row against two; row and column tails inside one tile; exact tiles; one past a tile on either
# side at the classifier's width; unaligned rows (no float4 path); a set against itself with tails, three tiles; inside one tile; at the
# classifier's width; several slabs of several tiles; one tile of a against the same b (slabs of one tile)
CASES = [(1, 1, 1, False), (1, 2, 1, False), (17, 70, 10, False), (64, 64, 4, False), (65, 129, 128, False), (57, 70, 67, False),
         (130, 130, 192, True), (57, 57, 10, True), (200, 200, 128, True), (1000, 2100, 128, False), (64, 2100, 128, False)]
SIGNED = (150, 141, 24, False)          # gamma = 1, coef0 = -0.5 on zero-mean Gaussian rows: v changes sign


def relu_rows(rows, d, seed, shift=0.0, scale=1.0):
    """fp32 [rows, d]: scale max(0, N(shift, 1)) - what a pooled ReLU layer looks like."""
    r = np.random.RandomState(seed)
    return (scale * np.maximum(0.0, shift + r.randn(rows, d))).astype(np.float32)


def inputs(m, n, d, exclude_diag, seed=7):
    """-> (a, b): ReLU-Gaussian rows, b slightly wider than a; the (64, 2100, 128) case is the first tile of the (1000, 2100, 128) one, and
    a set against itself is one array."""
    if exclude_diag:
        a = relu_rows(m, d, seed)
        return a, a
    b = relu_rows(n, d, seed + 1, scale=1.1)
    rows = 1000 if (m, n, d) == (64, 2100, 128) else m
    return relu_rows(rows, d, seed)[:m], b


def signed_inputs(seed=7):
    m, n, d, _ = SIGNED
    r = np.random.RandomState(seed)
    return r.randn(m, d).astype(np.float32), r.randn(n, d).astype(np.float32)


def kernel_direct(a, b, gamma=None, coef0=1.0):
    """-> (k long double [m, n], E_k fp64 [m, n]): the kernel values in the direct form and the bound of each.  gamma None is the fp64
    quotient 1 / d, the number the wrapper hands to the device."""
    d = a.shape[1]
    gamma = 1.0 / d if gamma is None else float(gamma)
    dot = np.asarray(a, dtype=np.longdouble) @ np.asarray(b, dtype=np.longdouble).T
    v = np.longdouble(gamma) * dot + np.longdouble(coef0)
    e = abs(gamma) * (d + 4) * U52 * (np.abs(np.asarray(a, dtype=np.float64)) @ np.abs(np.asarray(b, dtype=np.float64)).T)
    av = np.abs(np.asarray(v, dtype=np.float64))
    return (v * v) * v, 3.0 * (av + e) ** 2 * e + 8.0 * U52 * av ** 3


def gemm_form(a, b, gamma=None, coef0=1.0):
    gamma = 1.0 / a.shape[1] if gamma is None else float(gamma)
    v = gamma * (np.asarray(a, dtype=np.float64) @ np.asarray(b, dtype=np.float64).T) + coef0
    return (v * v) * v


def _tiles(x, dtype=np.longdouble):
    """[m, n] -> [ceil(m / 64), ceil(n / 64)]: the sum of every tile, accumulated in `dtype`."""
    m, n = x.shape
    mt, nt = -(-m // TILE), -(-n // TILE)
    pad = np.zeros((mt * TILE, nt * TILE), dtype=dtype)
    pad[:m, :n] = x
    return pad.reshape(mt, TILE, nt, TILE).sum(axis=(1, 3))


def tile_sums(a, b, gamma=None, coef0=1.0, exclude_diag=False):
    """-> (sums long double [mt, nt], bound fp64 [mt, nt]) of kernels.kernel_tile_sums."""
    k, e = kernel_direct(a, b, gamma, coef0)
    if exclude_diag:
        assert a.shape == b.shape
        i = np.arange(a.shape[0])
        k[i, i] = 0.0
        e[i, i] = 0.0
    return _tiles(k), np.asarray(_tiles(e, np.float64) + 4096 * U52 * _tiles(np.abs(k)), dtype=np.float64)


def tile_sums_fsum(a, b, gamma=None, coef0=1.0, exclude_diag=False):
    """The same sums by math.fsum over plain loops - the check of the long double path (small shapes)."""
    k, _ = kernel_direct(a, b, gamma, coef0)
    m, n = k.shape
    out = np.zeros((-(-m // TILE), -(-n // TILE)))
    for p in range(out.shape[0]):
        for q in range(out.shape[1]):
            out[p, q] = math.fsum(float(k[i, j]) for i in range(TILE * p, min(TILE * p + TILE, m)) for j in range(TILE * q, min(TILE * q + TILE, n))
                                  if not (exclude_diag and i == j))
    return out


def default_subset(m, n):
    return TILE * max(1, min(1024, min(m, n) // 4) // TILE)


def _estimate(xx, yy, xy, exx, eyy, exy, m, n):
    """One estimate from three (sub)matrices of tile sums and of their bounds -> (value, bound)."""
    cx, cy, cxy = m * (m - 1.0), n * (n - 1.0), float(m) * n
    value = float(xx.sum() / cx + yy.sum() / cy - 2 * xy.sum() / cxy)
    bound = 0.0
    for s, e, c, w in ((xx, exx, cx, 1.0), (yy, eyy, cy, 1.0), (xy, exy, cxy, 2.0)):
        bound += w * (float(e.sum()) + (s.size + 8) * 2.0 ** -53 * float(np.abs(s).sum())) / c
    return value, bound


def kernel_distance(fa, fb, subset=None):
    """The dict of ctgan_amd.score_cifar.kernel_distance for sample features fa against reference features fb, plus 'e_kid' and
    'e_blocks': the bounds of `kid` and of every element of `kid_blocks`."""
    m, n = fa.shape[0], fb.shape[0]
    s = default_subset(m, n) if subset is None else int(subset)
    (xx, exx), (yy, eyy), (xy, exy) = tile_sums(fa, fa, exclude_diag=True), tile_sums(fb, fb, exclude_diag=True), tile_sums(fa, fb)
    kid, e_kid = _estimate(xx, yy, xy, exx, eyy, exy, m, n)
    t, p = s // TILE, min(m // s, n // s)
    blocks, e_blocks = np.zeros(p), np.zeros(p)
    for i in range(p):
        w = slice(i * t, i * t + t)
        blocks[i], e_blocks[i] = _estimate(xx[w, w], yy[w, w], xy[w, w], exx[w, w], eyy[w, w], exy[w, w], s, s)
    return {'kid': kid, 'kid_std': float(blocks.std(ddof=1)) if p >= 2 else None, 'kid_blocks': blocks, 'subset': s, 'e_kid': e_kid,
            'e_blocks': e_blocks}


def std_bound(blocks, e_blocks):
    """|std(x + dx) - std(x)| <= |dx - mean dx| / sqrt(P - 1) <= 2 max |dx| sqrt(P / (P - 1)) (the triangle inequality of the norm)."""
    p = len(blocks)
    return 2.0 * float(np.max(e_blocks)) * math.sqrt(p / (p - 1.0))


_CACHE = {}


def case(m, n, d, exclude_diag, seed=7):
    """-> (a, b, sums, bound), computed once."""
    key = (m, n, d, exclude_diag, seed)
    if key not in _CACHE:
        a, b = inputs(m, n, d, exclude_diag, seed)
        _CACHE[key] = (a, b) + tile_sums(a, b, exclude_diag=exclude_diag)
    return _CACHE[key]
