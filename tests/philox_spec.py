"""What every Philox-drawing entry point of ctgan_amd.kernels must produce, written once in numpy.  TEST INFRASTRUCTURE ONLY.

Built on oracle.philox (philox_blocks / uniform / normal / labels) alone: the device tests (tests/test_gpu_philox_streams.py) and the
tests of the CPU stand-ins (tests/test_philox_standins.py) both compare with these functions, so the HIP kernels, the stand-ins that
the host tests and the golden fixtures rest on, and the oracle's streams are pinned to one contract.

Conventions: every tensor is taken in PHYSICAL (storage) order as a 1-D array, or [rows, row_elems] for the row kernels - the
stream index of an element is its physical index.  Float32 arithmetic is written in the kernels' operand order, one rounding per
operation (numpy float32 arrays round after each operation, and the kernels' products `x * inv * mask` hold no addition a compiler
could contract)."""
import functools

import numpy as np

from oracle import philox

F32 = np.float32

# (seed, stream id, step)
CORNERS = {
    'A': (2024, 5, 0),                                                   # the suite's first anchor
    'B': (0x9E3779B97F4A7C15, (513 << 16) | 7, (1 << 32) + 5),           # high key word, rank bits and counter word 3 all non-zero
    'C': (2 ** 64 - 1, 2 ** 32 - 1, 2 ** 63 - 1),                        # every word saturated (the counter tensor is int64)
}
# 2,097,157 = 4*256*2048 + 5: launches are capped at 2048 workgroups of 256 lanes with one four-value block per lane and pass, so
# this is the smallest size at which a lane takes a second block AND a ragged tail exists
GRID_ELEMS = 4 * 256 * 2048
SIZES = (1, 3, 4, 5, 1001, GRID_ELEMS + 5)
U_MAX = F32(1.0 - 2.0 ** -24)                                            # the largest value u01 produces


@functools.lru_cache(maxsize=6)
def uniform(seed, sid, step, n, first=0):
    """float32 [n], read-only: elements first .. first+n-1 of the U[0,1) stream (kept for the next case: the 2M-element streams take
    numpy a third of a second each)."""
    u = philox.uniform(seed, sid, step, n, first=first)
    u.setflags(write=False)
    return u


def scaled64(seed, sid, step, n, lo, hi):
    """float64 [n]: lo32 + (hi32 - lo32) * u without any rounding - what rng_uniform(lo, hi) rounds twice."""
    lo32, hi32 = np.float64(F32(lo)), np.float64(F32(hi))
    return lo32 + (hi32 - lo32) * uniform(seed, sid, step, n).astype(np.float64)


def keep_pattern(keep, u):
    """bool: True where tf.nn.dropout keeps the element, floor(keep + u) >= 1 in float32; keep >= 1 keeps everything (1.0f + (1 - 2^-24)
    rounds to 2.0f: the mask is 1 all the same)."""
    if keep >= 1.0:
        return np.ones(u.shape, dtype=bool)
    return np.floor(F32(keep) + u.astype(F32)) >= 1


def _inv(keep):
    return F32(1.0) / F32(keep)                                           # the hosts compute 1.f / keep in float32


def dropout_given_u(x, u, keep):
    """-> (y, kept): y = float32(float32(x * float32(1/keep)) * mask), mask = floor(float32(keep) + u), 1 for keep >= 1."""
    x = np.asarray(x, dtype=F32)
    kept = keep_pattern(keep, u)
    return ((x * _inv(keep)).astype(F32) * kept.astype(F32)).astype(F32), kept


def dropout(x, keep, seed, sid, step, first=0):
    """-> (y, kept) of dropout_rng on the physical 1-D x; u = elements first.. of the stream."""
    x = np.asarray(x, dtype=F32).reshape(-1)
    return dropout_given_u(x, uniform(seed, sid, step, x.size, first), keep)


def lrelu(x, ref, alpha):
    """float32: x * slope(ref), slope = 1 where ref > 0 else float32(alpha) - lrelu_bwd(x, ref, alpha)."""
    x, ref = np.asarray(x, dtype=F32).reshape(-1), np.asarray(ref, dtype=F32).reshape(-1)
    return (x * np.where(ref > 0, F32(1.0), F32(alpha)).astype(F32)).astype(F32)


def lrelu_dropout(x, ref, alpha, keep, seed, sid, step, first=0):
    """-> (y, kept) of lrelu_dropout_rng: x * slope(ref) is rounded first, then the dropout."""
    return dropout(lrelu(x, ref, alpha), keep, seed, sid, step, first)


def lrelu_dropout2(x, ref, n1, alpha, keep, seed, sid, sid2, step):
    """-> (y, kept) of lrelu_dropout_rng2 on physical 1-D x: elements [0, n1) draw stream sid, elements [n1, n) draw stream sid2
    indexed from n1 (each part the draws of a launch of its own)."""
    x, ref = np.asarray(x, dtype=F32).reshape(-1), np.asarray(ref, dtype=F32).reshape(-1)
    ya, ka = lrelu_dropout(x[:n1], ref[:n1], alpha, keep, seed, sid, step)
    yb, kb = lrelu_dropout(x[n1:], ref[n1:], alpha, keep, seed, sid2, step)
    return np.concatenate([ya, yb]), np.concatenate([ka, kb])


def dropout_mask(x, ref, keep, seed, sid, step):
    """-> (y, ym, kept) of dropout_rng_mask: y = dropout(x), ym = y where ref > 0 else 0."""
    y, kept = dropout(x, keep, seed, sid, step)
    ref = np.asarray(ref, dtype=F32).reshape(-1)
    return y, np.where(ref > 0, y, F32(0.0)).astype(F32), kept


def critic_prep(x_int, fake, seed, sid_deq, sid_alpha, step, lo, hi, denom):
    """-> (real, fake, interp) of critic_prep on [B, d] inputs; real and interp in float64 without rounding:
        real = 2 (x / denom - .5) + lo32 + (hi32 - lo32) u[i]      u = stream sid_deq at the element index i
        interp = real + alpha[r] (fake - real)                      alpha[r] = element r of stream sid_alpha (U[0,1))
    The fake rows pass through unchanged (float32)."""
    x_int, fake = np.asarray(x_int), np.asarray(fake, dtype=F32)
    B, d = x_int.shape
    noise = scaled64(seed, sid_deq, step, B * d, lo, hi).reshape(B, d)
    real = 2.0 * (x_int.astype(np.float64) / np.float64(F32(denom)) - 0.5) + noise
    alpha = uniform(seed, sid_alpha, step, B).astype(np.float64).reshape(B, 1)
    return real, fake, real + alpha * (fake.astype(np.float64) - real)


def rows_cat(x, n_extra, keep, seed, sid, step):
    """-> (y, kept) of rows_cat_dropout on physical [rows, row_elems] x: dropout of [x ; x[:n_extra]] indexed by the element of the
    RESULT; keep >= 1: the plain concatenation."""
    x = np.asarray(x, dtype=F32)
    cat = np.concatenate([x, x[:n_extra]], 0)
    y, kept = dropout(cat, keep, seed, sid, step)
    return y.reshape(cat.shape), kept.reshape(cat.shape)


def rows_gather(x, segs, seed, step):
    """-> (y, kept) of rows_gather_dropout on physical [rows, row_elems] x.  segs = [(src_row0, rows, keep, sid, index_row0), ...]:
    the result is the concatenation of the segments' source rows; an element of a segment with keep < 1 draws stream `sid` at its
    element index in the result RELATIVE to result row index_row0 (so a group of segments sharing sid and index_row0 reproduces the
    dropout of its own concatenated tensor)."""
    x = np.asarray(x, dtype=F32)
    row_elems = x.shape[1]
    ys, ks, row = [], [], 0
    for r0, rows, keep, sid, idx0 in segs:
        part = x[r0:r0 + rows]
        assert 0 <= idx0 <= row
        y, kept = dropout(part, keep, seed, sid, step, first=(row - idx0) * row_elems)
        ys.append(y.reshape(part.shape)); ks.append(kept.reshape(part.shape))
        row += rows
    return np.concatenate(ys, 0), np.concatenate(ks, 0)


def rows_cat_bwd(g, n_src, n_extra, n_pass=0):
    """Adjoint of [x ; x[:n_extra]] on physical [rows, row_elems] g, with n_pass rows behind the concat passing straight through:
    one float32 addition per element of the first n_extra rows."""
    g = np.asarray(g, dtype=F32)
    out = np.concatenate([g[:n_src], g[n_src + n_extra:n_src + n_extra + n_pass]], 0).copy()
    out[:n_extra] = (out[:n_extra] + g[n_src:n_src + n_extra]).astype(F32)
    return out


def normal64(seed, sid, step, n, first=0):
    """float64 [n]: Box-Muller on lane pairs (0,1) and (2,3) of each block with u1 = ((x >> 8) + .5) 2^-24, u2 = (x >> 8) 2^-24 and the
    angle 2 pi u2 rounded to float32 exactly as the kernel rounds them, and log, sqrt, sin, cos in float64: element 2k of a pair is
    r cos, element 2k+1 is r sin.  `first` must be a multiple of 4."""
    assert first % 4 == 0
    b0, b1 = first >> 2, (first + n + 3) >> 2
    x = philox.philox_blocks(seed, sid, step, b1 - b0, b0)
    out = np.empty((b1 - b0, 4), dtype=np.float64)
    for k in range(2):
        u1 = (((x[:, 2 * k] >> np.uint32(8)).astype(F32) + F32(0.5)).astype(F32) * F32(1.0 / 16777216.0)).astype(F32)
        u2 = ((x[:, 2 * k + 1] >> np.uint32(8)).astype(F32) * F32(1.0 / 16777216.0)).astype(F32)
        ang = (F32(6.283185307179586) * u2).astype(F32).astype(np.float64)
        r = np.sqrt(-2.0 * np.log(u1.astype(np.float64)))
        out[:, 2 * k] = r * np.cos(ang)
        out[:, 2 * k + 1] = r * np.sin(ang)
    return out.reshape(-1)[:n]


def normal_distance(got, ref64):
    """max |got - ref| / max(1, |ref|): the measure of the rng_normal comparison."""
    got, ref64 = np.asarray(got, dtype=np.float64), np.asarray(ref64, dtype=np.float64)
    return float(np.max(np.abs(got - ref64) / np.maximum(1.0, np.abs(ref64)))) if got.size else 0.0


def labels(seed, sid, step, n, nlab):
    """int32 [n] = trunc(u * nlab) in float32: oracle.philox.labels on the stream kept by uniform()."""
    return (uniform(seed, sid, step, n) * F32(nlab)).astype(np.int32)
