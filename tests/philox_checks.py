"""The case tables of tests/philox_spec.py run against one implementation of the kernel wrappers.  TEST INFRASTRUCTURE ONLY.

tests/test_gpu_philox_streams.py runs them against ctgan_amd.kernels on the device, tests/test_philox_standins.py against the CPU
stand-ins of tests/cpu_kernels.py.  Draws, labels and keep/drop patterns are exact on both.  Kept VALUES are bit-equal on the device;
the stand-in divides by keep where the kernels multiply by float32(1/keep), which is worth 2^-23 relative."""
import functools

import numpy as np
import torch

from oracle import philox
from tests import philox_spec as S

F32 = np.float32
KEEPS = (0.8, 0.5, 0.3)
EXACT_RANGES = ((0.0, 1.0), (0.0, 1.0 / 128), (-1.0, 1.0))   # lo + (hi - lo) u is exact in float32 with or without a fused multiply-add
ROUNDED_RANGE = (0.1, 0.7)                                   # here a fused evaluation differs from the separate one: bounded, not bit-equal
LABEL_COUNTS = (1, 2, 3, 7, 10, 1000)
NORMAL_SIZES = (1, 2, 3, 4, 5, 1001, S.SIZES[-1])            # 1, 2, 3 and 5 end in the middle of a Box-Muller pair or block

# d_ref: the largest |oracle.philox.normal - philox_spec.normal64| / max(1, |normal64|) over the streams of check_normal (every corner
# of philox_spec.CORNERS x NORMAL_SIZES), measured on the CPU, where numpy's float32 log / cos / sin are good to 1 ulp: 2.310e-7, met
# at corner A, n = 2,097,157 (5.2e-7 absolute; corner B there 2.20e-7 and 5.5e-7, corner C 2.14e-7).  The constant is that figure rounded up
# in its third digit; tests/test_philox_standins.py measures it again with every run.  The device gets 4 d_ref = 9.28e-7: its math
# library documents 1-2 ulp for logf and sincosf against 1 ulp, and r * cs rounds once more.  A swapped pair, a wrong lane or a wrong
# u1 offset is wrong by order 1.
D_REF = 2.32e-7
DEVICE_NORMAL_TOL = 4 * D_REF


class Backend:
    """K: the module under test (ctgan_amd.kernels or tests.cpu_kernels); exact: kept values are compared bit for bit."""

    def __init__(self, K, device, exact):
        self.K, self.device, self.exact = K, device, exact
        self.seen = {}                                       # largest observed distances, for the record (printed by the tests)

    def ctr(self, step):
        return torch.tensor([step], dtype=torch.int64, device=self.device)

    def dev(self, a):
        return torch.from_numpy(np.array(a)).to(self.device)          # (a copy: the cached inputs are read-only)

    def cl(self, a):
        """channels-last tensor of the logical [N,C,H,W] array a"""
        t = self.dev(a)
        out = torch.empty((t.shape[0], t.shape[2], t.shape[3], t.shape[1]), device=self.device, dtype=t.dtype).permute(0, 3, 1, 2)
        out.copy_(t)
        return out

    def note(self, name, value):
        self.seen[name] = max(self.seen.get(name, 0.0), float(value))


def phys(t):
    """numpy 1-D copy of a dense tensor in physical (storage) order"""
    return t.as_strided((t.numel(),), (1,)).cpu().numpy()


def rows(t):
    """numpy [rows, row_elems] copy of a dense tensor whose dim 0 is outermost in memory"""
    return phys(t).reshape(t.shape[0], -1)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=F32), np.ascontiguousarray(b, dtype=F32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def assert_dropped(be, got, want, kept, live, what):
    """got against the specification's (want, kept): the pattern exactly (live: where the undropped value is non-zero), the values bit
    for bit (device) or to 2^-23 relative (stand-in)."""
    got, want = np.asarray(got).reshape(-1), np.asarray(want).reshape(-1)
    kept, live = np.asarray(kept).reshape(-1), np.asarray(live).reshape(-1)
    assert got.shape == want.shape, what
    assert np.array_equal(got != 0, kept & live), (what, 'keep/drop pattern', int(((got != 0) != (kept & live)).sum()))
    if be.exact:
        assert same_bits(got, want), (what, 'values', int((got.view(np.uint32) != want.view(np.uint32)).sum()))
    else:
        g, w = got.astype(np.float64), want.astype(np.float64)
        assert np.all(np.abs(g - w) <= 2.0 ** -23 * np.abs(w)), (what, 'values', float(np.max(np.abs(g - w) / np.maximum(np.abs(w), 1e-30))))


@functools.lru_cache(maxsize=4)
def _base(n):
    """n + 1 standard normals: [:n] is the aligned input, [1:] the one whose pointer is 4 bytes past a 16-byte boundary"""
    a = np.random.RandomState(n % 1000003).standard_normal(n + 1).astype(F32)
    a.setflags(write=False)
    return a


def inputs_1d(be, n):
    """[(name, tensor)]: a 16-byte-aligned 1-D tensor of n elements and the misaligned view base[1:1+n] (scalar path of the kernels)"""
    base = be.dev(_base(n))
    return [('aligned', base[:n].clone()), ('misaligned', base[1:1 + n])]


def input_cl(be, seed=3):
    return be.cl(np.random.RandomState(seed).standard_normal((3, 8, 2, 2)).astype(F32))


# ------------------------------------------------------------------------------------------------------------- plain draws
def check_uniform(be, corner, n):
    seed, sid, step = S.CORNERS[corner]
    ctr = be.ctr(step)
    for lo, hi in EXACT_RANGES:
        out = be.K.rng_uniform(torch.empty(n, device=be.device), seed, sid, ctr, lo, hi)
        assert np.array_equal(out.cpu().numpy(), philox.uniform(seed, sid, step, n, lo, hi)), (corner, n, lo, hi)
    lo, hi = ROUNDED_RANGE
    out = be.K.rng_uniform(torch.empty(n, device=be.device), seed, sid, ctr, lo, hi).cpu().numpy().astype(np.float64)
    dist = np.max(np.abs(out - S.scaled64(seed, sid, step, n, lo, hi)))
    bound = 2.0 ** -23 * max(abs(F32(lo)), abs(F32(hi)), abs(np.float64(F32(hi)) - np.float64(F32(lo))))
    print('uniform(0.1, 0.7) corner %s n %d: max distance %.3g (bound %.3g)' % (corner, n, dist, bound))
    be.note('uniform_0.1_0.7', dist)
    assert dist <= bound, (corner, n, dist, bound)
    assert int(ctr.item()) == step                           # a draw does not move the counter


def check_uniform_channels_last(be, corner):
    seed, sid, step = S.CORNERS[corner]
    out = be.K.rng_uniform(be.K.empty_cl(3, 8, 2, 2, be.device), seed, sid, be.ctr(step), -1.0, 1.0)
    want = philox.uniform(seed, sid, step, 96, -1.0, 1.0)
    assert np.array_equal(phys(out), want)                                                       # physical order is the index
    assert np.array_equal(out.cpu().numpy(), want.reshape(3, 2, 2, 8).transpose(0, 3, 1, 2))    # = the channels-last element index


def check_normal(be, corner, n, tol):
    seed, sid, step = S.CORNERS[corner]
    out = be.K.rng_normal(torch.empty(n, device=be.device), seed, sid, be.ctr(step)).cpu().numpy()
    dist = S.normal_distance(out, S.normal64(seed, sid, step, n))
    print('normal corner %s n %d: distance %.3g (tolerance %.3g)' % (corner, n, dist, tol))
    be.note('normal', dist)
    assert out.shape == (n,) and dist <= tol, (corner, n, dist, tol)


def check_labels(be, corner, n):
    seed, sid, step = S.CORNERS[corner]
    ctr = be.ctr(step)
    for nlab in LABEL_COUNTS:
        out = be.K.rng_labels(torch.empty(n, dtype=torch.int32, device=be.device), nlab, seed, sid, ctr).cpu().numpy()
        assert out.dtype == np.int32 and np.array_equal(out, S.labels(seed, sid, step, n, nlab)), (corner, n, nlab)
        assert out.min() >= 0 and out.max() < nlab, (corner, n, nlab)


# ------------------------------------------------------------------------------------------------------------- dropout family
def _check_dropouts_on(be, x, corner, keeps, what):
    """dropout_rng, lrelu_dropout_rng (ref = x and ref = a forward result) and dropout_rng_mask (with and without the dropped tensor) on
    the dense tensor x."""
    K = be.K
    seed, sid, step = S.CORNERS[corner]
    ctr = be.ctr(step)
    xp = phys(x)
    live = xp != 0
    alpha = 0.2
    for keep in keeps:
        tag = (what, corner, keep)
        y, kept = S.dropout(xp, keep, seed, sid, step)
        got = K.dropout_rng(x, keep, seed, sid, ctr)
        assert got.shape == x.shape and got.stride() == x.stride()
        assert_dropped(be, phys(got), y, kept, live, tag + ('dropout_rng',))
        # forward of the fused pair: ref = x
        yf, kf = S.lrelu_dropout(xp, xp, alpha, keep, seed, sid, step)
        fwd = K.lrelu_dropout_rng(x, x, alpha, keep, seed, sid, ctr)
        assert_dropped(be, phys(fwd), yf, kf, live, tag + ('lrelu_dropout_rng fwd',))
        # its backward: x = the arriving gradient, ref = the forward RESULT (0 where dropped: slope alpha there, and the mask drops it again)
        yb, kb = S.lrelu_dropout(xp, phys(fwd), alpha, keep, seed, sid, step)
        bwd = K.lrelu_dropout_rng(x, fwd, alpha, keep, seed, sid, ctr)
        assert_dropped(be, phys(bwd), yb, kb, live, tag + ('lrelu_dropout_rng bwd',))
        assert np.array_equal(kb, kf)                        # the same mask again
        # dropout + ReLU mask of another tensor
        yd, ym, kd = S.dropout_mask(xp, phys(fwd), keep, seed, sid, step)
        d, m = K.dropout_rng_mask(x, fwd, keep, seed, sid, ctr)
        assert_dropped(be, phys(d), yd, kd, live, tag + ('dropout_rng_mask y',))
        assert_dropped(be, phys(m), ym, kd & (phys(fwd) > 0), live, tag + ('dropout_rng_mask ym',))
        none, m2 = K.dropout_rng_mask(x, fwd, keep, seed, sid, ctr, want_dropped=False)
        assert none is None and same_bits(phys(m2), phys(m)), tag


def check_dropouts_1d(be, corner, n, keeps=KEEPS):
    for name, x in inputs_1d(be, n):
        _check_dropouts_on(be, x, corner, keeps, '%s n=%d' % (name, n))


def check_dropouts_channels_last(be, corner):
    _check_dropouts_on(be, input_cl(be), corner, KEEPS, 'channels-last (3,8,2,2)')


def check_lrelu_dropout2(be, corner, n1_rows):
    seed, sid, step = S.CORNERS[corner]
    sid2 = sid ^ 0x30000                                     # another rank's stream
    x = be.dev(np.random.RandomState(5).standard_normal((5, 12)).astype(F32))
    ref = be.dev(np.random.RandomState(6).standard_normal((5, 12)).astype(F32))
    for keep in KEEPS:
        want, kept = S.lrelu_dropout2(phys(x), phys(ref), n1_rows * 12, 0.2, keep, seed, sid, sid2, step)
        got = be.K.lrelu_dropout_rng2(x, ref, n1_rows, 0.2, keep, seed, sid, sid2, be.ctr(step))
        assert_dropped(be, phys(got), want, kept, phys(x) != 0, ('lrelu_dropout_rng2', corner, n1_rows, keep))
    if 0 < n1_rows < 5:                                      # the second part is indexed from its own first element
        _, k_own = S.dropout(phys(x)[n1_rows * 12:], KEEPS[-1], seed, sid2, step)
        assert np.array_equal(kept[n1_rows * 12:], k_own)


# ------------------------------------------------------------------------------------------------------------- critic inputs
def check_critic_prep(be, corner, B, d, denom):
    seed, sid, step = S.CORNERS[corner]
    sid_a = sid + 1
    lo, hi = 0.0, 1.0 / 128
    r = np.random.RandomState(B * d + int(denom))
    xi = r.randint(0, 256, size=(B, d)).astype(np.int32)
    fake = (r.rand(B, d) * 2 - 1).astype(F32)
    rf, interp, both = be.K.critic_prep(be.dev(xi), be.dev(fake), seed, sid, sid_a, be.ctr(step), lo, hi, denom)
    real64, fake_w, interp64 = S.critic_prep(xi, fake, seed, sid, sid_a, step, lo, hi, denom)
    assert tuple(rf.shape) == (2 * B, d) and tuple(interp.shape) == (B, d) and tuple(both.shape) == (3 * B, d)
    assert same_bits(rf[B:].cpu().numpy(), fake_w), 'fake rows'
    assert torch.equal(both[:2 * B], rf) and torch.equal(both[2 * B:], interp)
    d_real = np.max(np.abs(rf[:B].cpu().numpy().astype(np.float64) - real64))
    d_int = np.max(np.abs(interp.cpu().numpy().astype(np.float64) - interp64))
    print('critic_prep corner %s (%d,%d) denom %g: real %.3g (bound %.3g) interp %.3g (bound %.3g)'
          % (corner, B, d, denom, d_real, 2.0 ** -22, d_int, 2.0 ** -21))
    be.note('critic_prep_real', d_real); be.note('critic_prep_interp', d_int)
    # per element, absolute: four float32 roundings on values of magnitude at most about 1 (real), two more on the way to interp
    assert d_real <= 2.0 ** -22 and d_int <= 2.0 ** -21, (d_real, d_int)


# ------------------------------------------------------------------------------------------------------------- row kernels
ROW_SHAPES = ('rows4', 'cl8192')


def _row_source(be, shape, n_rows, seed=0):
    """dense source of n_rows rows: 'rows4' = [n_rows, 4] (the smallest legal row), 'cl8192' = channels-last [n_rows, 128, 8, 8]"""
    r = np.random.RandomState(seed + n_rows)
    if shape == 'rows4':
        return be.dev(r.standard_normal((n_rows, 4)).astype(F32))
    return be.cl(r.standard_normal((n_rows, 128, 8, 8)).astype(F32))


def check_rows_cat(be, corner, shape):
    seed, sid, step = S.CORNERS[corner]
    n_src, n_extra = (3, 2) if shape == 'rows4' else (10, 4)
    x = _row_source(be, shape, n_src)
    for keep in (0.8, 0.3, 1.0):
        want, kept = S.rows_cat(rows(x), n_extra, keep, seed, sid, step)
        got = be.K.rows_cat_dropout(x, n_extra, keep, seed, sid, be.ctr(step))
        assert got.shape[0] == n_src + n_extra and tuple(got.shape[1:]) == tuple(x.shape[1:])
        assert_dropped(be, rows(got), want, kept, np.ones(kept.shape, bool), ('rows_cat_dropout', corner, shape, keep))
        if keep == 1.0:
            assert same_bits(rows(got), np.concatenate([rows(x), rows(x)[:n_extra]], 0))
    for n_pass in (0, 3):
        g = _row_source(be, shape, n_src + n_extra + n_pass, seed=7)
        out = be.K.rows_cat_bwd(g, n_src, n_extra, n_pass)
        assert out.shape[0] == n_src + n_pass
        assert same_bits(rows(out), S.rows_cat_bwd(rows(g), n_src, n_extra, n_pass)), ('rows_cat_bwd', shape, n_pass)


def gather_segments(n_rows, sid):
    """Six segments (CTGAN_ROW_SEGMENTS) over a source of n_rows rows: two that share index_row0 and stream (the dropout of their own
    concatenated tensor), one with keep 1, one with a stream and an index origin of its own, one indexed from an origin BEHIND its first
    row on a third stream, one more on the first stream from its own row."""
    a = (2 * n_rows) // 3
    b = n_rows - a
    s0, s1, s2 = sid, sid + 4, sid ^ 0x10000
    return [(0, a, 0.8, s0, 0), (0, b, 0.8, s0, 0), (0, a, 1.0, 0, a + b), (a, b, 0.5, s1, 2 * a + b), (1, 2, 0.3, s2, 2 * a + b),
            (n_rows - 2, 2, 0.8, s0, 2 * a + 2 * b + 2)]


def check_rows_gather(be, corner, shape):
    seed, sid, step = S.CORNERS[corner]
    n_rows = 5 if shape == 'rows4' else 12
    x = _row_source(be, shape, n_rows, seed=11)
    segs = gather_segments(n_rows, sid)
    assert len(segs) == 6 and segs[0][4] == segs[1][4] and segs[2][2] == 1.0
    want, kept = S.rows_gather(rows(x), segs, seed, step)
    got = be.K.rows_gather_dropout(x, segs, seed, be.ctr(step))
    assert got.shape[0] == sum(sg[1] for sg in segs)
    assert_dropped(be, rows(got), want, kept, np.ones(kept.shape, bool), ('rows_gather_dropout', corner, shape))
    a, b = segs[0][1], segs[1][1]
    head, _ = S.rows_cat(rows(x)[:a], b, 0.8, seed, sid, step)                  # the first two segments = rows_cat_dropout of their own
    assert same_bits(want[:a + b], head) and same_bits(want[a + b:2 * a + b], rows(x)[:a])


# ------------------------------------------------------------------------------------------------------------- counter
def check_counter_arithmetic(be):
    K = be.K
    seed, sid, _ = S.CORNERS['B']
    top = 2 ** 32 - 1
    ctr = be.ctr(top)
    K.rng_advance(ctr, 1)
    assert int(ctr.item()) == 2 ** 32
    ctr2 = be.ctr(top)
    state = torch.tensor([1e-3, 0.5, 0.9, 0.0], dtype=torch.float32, device=be.device)
    K.step_advance(state, 0.5, 0.9, ctr2, 1)
    assert int(ctr2.item()) == 2 ** 32 and state.cpu().tolist() == [F32(1e-3), 0.25, F32(0.9) * F32(0.9), 0.0]
    for c in (ctr, ctr2):                                    # the carry into counter word 3 reaches the draw
        out = K.rng_uniform(torch.empty(1001, device=be.device), seed, sid, c).cpu().numpy()
        assert np.array_equal(out, philox.uniform(seed, sid, 2 ** 32, 1001))
        assert not np.array_equal(out, philox.uniform(seed, sid, 0, 1001))
    K.rng_advance(ctr, 2 ** 33 + 1)
    assert int(ctr.item()) == 2 ** 32 + 2 ** 33 + 1
    out = K.rng_uniform(torch.empty(5, device=be.device), seed, sid, ctr).cpu().numpy()
    assert np.array_equal(out, philox.uniform(seed, sid, 2 ** 32 + 2 ** 33 + 1, 5))


# ------------------------------------------------------------------------------------------------------------- keep = 1
def check_keep_one(be):
    """keep = 1 is inside the documented (0,1] and keeps every element AS IT IS: floor(1.0f + u) is 2 for the largest u01 = 1 - 2^-24."""
    K = be.K
    assert np.floor(F32(1.0) + S.U_MAX) == 2.0               # the arithmetic the entry points must not fall for
    x = be.dev(np.array([1.5, -2.25, 3.0, 0.1, -0.0, 7.0, -1e-30, 5.5], dtype=F32))
    u = be.dev(np.array([S.U_MAX, 0.0, 0.5, S.U_MAX, S.U_MAX, 0.0, S.U_MAX, 0.5], dtype=F32))
    assert same_bits(K.dropout(x, u, 1.0).cpu().numpy(), x.cpu().numpy())
    seed, sid, step = S.CORNERS['B']
    ctr = be.ctr(step)
    for name, t in inputs_1d(be, 1001) + [('channels-last', input_cl(be))]:
        ref = t.flip(0).clone() if t.dim() == 1 else input_cl(be, seed=4)
        assert same_bits(phys(K.dropout_rng(t, 1.0, seed, sid, ctr)), phys(t)), name
        plain = K.lrelu_bwd(t, ref, 0.2)
        assert same_bits(phys(K.lrelu_dropout_rng(t, ref, 0.2, 1.0, seed, sid, ctr)), phys(plain)), name
        y, ym = K.dropout_rng_mask(t, ref, 1.0, seed, sid, ctr)
        masked = np.where(phys(ref) > 0, phys(t), F32(0.0)).astype(F32)    # +0 where masked (lrelu_bwd(., ., 0) leaves 0 * x = -0 for x < 0)
        assert same_bits(phys(y), phys(t)), name
        assert same_bits(phys(ym), masked) if be.exact else np.array_equal(phys(ym), masked), name
    x2, r2 = be.dev(_base(60)[:60].reshape(5, 12).copy()), be.dev(_base(60)[1:61].reshape(5, 12).copy())
    got = K.lrelu_dropout_rng2(x2, r2, 2, 0.2, 1.0, seed, sid, sid + 1, ctr)
    assert same_bits(phys(got), phys(K.lrelu_bwd(x2, r2, 0.2)))
