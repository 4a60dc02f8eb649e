"""Case tables, fp64 references and the checks of the elementwise / layout / filter kernels (ctgan_amd/csrc/elementwise.hip) and of the four
small-linear kernels (ctgan_amd/csrc/skinny.hip), shared by tests/test_gpu_elementwise_paths.py (the HIP kernels) and
tests/test_elementwise_standins.py (their fp32 torch stand-ins in tests/cpu_kernels.py).  A plain helper module: no fixtures, no marks.

References: every operation is written once, forward only, in fp64 (torch or numpy) after the comments of elementwise.hip, skinny.hip,
igemm.hip (the two data-gradient filter layouts), include/ctgan_hip.h and oracle/tf_ops.py.  None of them calls a function of
ctgan_amd.kernels or of tests/cpu_kernels.py.  Scalars are taken as the C ABI's float argument holds them (f32).

Bounds (none is derived from what the code under test returns), U = 2^-24:
  exact         torch.equal against the fp32 expression: pure data movement (copy4d, the broadcasts at scale 1, upsample2, the ROTATE and
                PHASES layouts without `pre`) and operations of one rounding (a scale times one value, mul, lrelu_* without scale, real_prep
                without noise, the 0 / 1 rows of interpolate); the dropout mask, whose floor(keep + u) is one correctly rounded addition
  relerr        max-abs over the reference's max-abs, the figures of test_elementwise: 1e-6 for tanh_*, sigmoid_*, the kept values of
                dropout, axpby, real_prep with noise, interpolate; 1e-7 for lrelu (lrelu_bwd_scaled rounds twice on its alpha branch only,
                where the values are alpha times smaller than on the other)
  per element   rsqrt: |got - ref| <= 4 U |ref| (add, sqrt, divide: three roundings); channel_affine: <= 4 U (|x s| + |o|)
  sums          |got - ref| <= d U sum|terms| per output element, the worst case of fp32 summation in any order whose longest path from a
                term to the result has d additions (fused multiply-adds); d is read from the kernel's loop structure (the *_d functions
                below; the addition onto the zero accumulator is counted, which covers the bound's second-order term), plus one for a
                scale and one for a bias.  The stand-ins sum in torch's order: for them d is the number of terms plus two (any order).
Input conditions are asserted on the reference: where the ReLU flag is on, no pre-activation lies within 1e-4 of zero relative to the sum of
its term magnitudes (the inputs are drawn again under the next seed until that holds).
"""
import itertools
import zlib

import numpy as np
import torch

from oracle import tf_ops

U = 2.0 ** -24
SENTINEL = 123.0
TOL, LRELU_TOL = 1e-6, 1e-7

# largest figure seen per kernel group in this process (printed by the test modules' teardown)
MEASURED = {}


def note(group, err):
    MEASURED[group] = max(MEASURED.get(group, 0.0), float(err))


def report():
    return '\n'.join('%-44s %.3g' % kv for kv in sorted(MEASURED.items()))


def f32(x):
    """x as the C ABI's float argument holds it."""
    return float(np.float32(x))


def gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()) % 100000)


class Backend:
    """Where the code under test runs: K = ctgan_amd.kernels (HIP, or patched with the stand-ins), F = ctgan_amd.functional over the same K."""

    def __init__(self, K, F, device):
        self.K, self.F, self.device = K, F, device
        self.gpu = device != 'cpu'

    def dev(self, t):
        return t.detach().clone().contiguous().to(self.device)

    def cl(self, t, extra_rows=0, fill=SENTINEL):
        """dense channels-last copy; extra_rows: the copy is the leading rows of a buffer whose other rows hold `fill` -> (view, buffer)"""
        n, c, h, w = t.shape
        buf = torch.full((n + extra_rows, h, w, c), fill, device=self.device, dtype=t.dtype).permute(0, 3, 1, 2)
        buf[:n].copy_(t.to(self.device))
        return (buf[:n], buf) if extra_rows else buf

    def off16(self, t):
        """the same values, contiguous, one float into a larger buffer: the data pointer is 4 past a 16-byte boundary"""
        buf = torch.zeros(t.numel() + 8, device=self.device, dtype=t.dtype)
        v = buf[1:1 + t.numel()].view(t.shape)
        v.copy_(t.to(self.device))
        assert not self.gpu or v.data_ptr() % 16 == 4
        return v

    def put(self, t, how):
        return self.off16(t) if how == 'off16' else self.dev(t)

    def d(self, kernel_d, nterms):
        """additions on the longest path: the kernel's on the device, any order (torch's) for the stand-ins"""
        return kernel_d if self.gpu else max(kernel_d, nterms + 2)

    def sync(self):
        if self.gpu:
            torch.cuda.synchronize()


def relerr(a, b):
    a = a.detach().cpu().double(); b = b.detach().cpu().double()
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-30)).item()


def close(group, got, ref, tol):
    ref = torch.as_tensor(ref)
    assert tuple(got.shape) == tuple(ref.shape), (group, got.shape, ref.shape)
    assert torch.isfinite(got).all(), group
    e = relerr(got, ref)
    note(group, e)
    assert e < tol, (group, e, tol)


def exact(group, got, want):
    assert tuple(got.shape) == tuple(want.shape), (group, got.shape, want.shape)
    assert torch.equal(got.detach().cpu(), want), group


def within(group, got, ref, mag, d):
    """|got - ref| <= d U mag per element; records the largest fraction of the bound used"""
    ref = torch.as_tensor(ref).double(); mag = torch.as_tensor(mag).double()
    got = got.detach().cpu().double()
    assert got.numel() == ref.numel() == mag.numel(), (group, got.shape, ref.shape)
    got = got.reshape(ref.shape); mag = mag.reshape(ref.shape)
    assert torch.isfinite(got).all(), group
    diff, bound = (got - ref).abs(), d * U * mag
    assert (diff[bound == 0] == 0).all(), group
    frac = float((diff / bound.clamp_min(1e-300)).max()) if diff.numel() else 0.0
    note(group + ' (of bound)', frac)
    assert frac <= 1.0, (group, frac, d)


def npf(t):
    return t.detach().cpu().double().numpy()


# ------------------------------------------------------------------------------------------------------------------ map kernels
MAP_SIZES = (1, 3, 4, 5, 1023, 1025)
MAP_BIG = 2 * 2048 * 256 * 4 + 7          # ctgan_blocks caps map1 / map2 at 2048 workgroups of 256 float4 lanes: the second pass, and a tail
LRELU_SPECIAL = (0.0, -0.0, 1.4e-45, -1.4e-45)
KEEPS = (0.5, 0.8, 1.0)


def _plant(x, values):
    k = min(len(values), x.numel())
    x.view(-1)[:k] = torch.tensor(values[:k], dtype=x.dtype)
    return x


def dropout_u(n, keep, g):
    """uniform draws holding 0, 1 - 2^-24 and 1 - keep with its two fp32 neighbours (in [0, 1))"""
    u = torch.rand(n, generator=g)
    t = np.float32(1) - np.float32(keep)
    sp = [0.0, 1.0 - 2.0 ** -24, float(t), float(np.nextafter(t, np.float32(1))), max(float(np.nextafter(t, np.float32(-1))), 0.0)]
    return _plant(u, sp)


def dropout_mask(u, keep):
    """floor(float32(keep) + float32(u)) in fp32: one correctly rounded addition; keep = 1 is the identity (oracle/tf_ops.py dropout)"""
    if keep == 1.0:
        return torch.ones_like(u)
    return torch.from_numpy(np.floor(np.float32(keep) + u.numpy().astype(np.float32)).astype(np.float32))


def _away(x, eps=0.1):
    """no value within eps of zero (a kept element of dropout is told from a dropped one by y != 0)"""
    return x + eps * torch.where(x >= 0, torch.ones_like(x), -torch.ones_like(x))


class MapOp:
    def __init__(self, name, template, nin, make, run, check):
        self.name, self.template, self.nin, self.make, self.run, self.check = name, template, nin, make, run, check


def _rand(n, g, special=()):
    return _plant(torch.randn(n, generator=g), special)


def _lrelu_ops():
    ops = []
    for alpha in (0.0, 0.2, 1.0):
        a32 = torch.tensor(alpha, dtype=torch.float32)

        def chk_f(got, x, alpha=alpha, a32=a32):
            exact('lrelu_fwd', got, torch.where(x > 0, x, a32 * x))
            close('lrelu_fwd', got, torch.where(x > 0, x.double(), f32(alpha) * x.double()), LRELU_TOL)
        ops.append(MapOp('lrelu_fwd(%g)' % alpha, 'map1', 1, lambda n, g: [_rand(n, g, LRELU_SPECIAL)],
                         lambda K, x, alpha=alpha: K.lrelu_fwd(x, alpha), chk_f))

        def chk_b(got, gy, ref, alpha=alpha, a32=a32):
            exact('lrelu_bwd', got, torch.where(ref > 0, gy, a32 * gy))
        ops.append(MapOp('lrelu_bwd(%g)' % alpha, 'map2', 2, lambda n, g: [_rand(n, g), _rand(n, g, LRELU_SPECIAL)],
                         lambda K, gy, ref, alpha=alpha: K.lrelu_bwd(gy, ref, alpha), chk_b))
        sc = f32(0.37)

        def chk_s(got, gy, ref, alpha=alpha):
            gd = gy.double()
            close('lrelu_bwd_scaled', got, torch.where(ref > 0, gd, f32(alpha) * gd) * sc, LRELU_TOL)
        ops.append(MapOp('lrelu_bwd_scaled(%g)' % alpha, 'map2', 2, lambda n, g: [_rand(n, g), _rand(n, g, LRELU_SPECIAL)],
                         lambda K, gy, ref, alpha=alpha: K.lrelu_bwd(gy, ref, alpha, scale=sc), chk_s))
    return ops


def _dropout_ops():
    ops = []
    for keep in KEEPS:
        def chk(got, x, u, keep=keep):
            mask = dropout_mask(u, keep)
            assert set(mask.unique().tolist()) <= {0.0, 1.0}
            exact('dropout mask', (got.detach().cpu() != 0).float(), mask)
            close('dropout', got, x.double() / f32(keep) * mask.double(), TOL)
            if keep == 1.0:
                assert torch.equal(tf_ops.dropout(x, 1.0, u), x)
        ops.append(MapOp('dropout(%g)' % keep, 'map2', 2, lambda n, g, keep=keep: [_away(torch.randn(n, generator=g)), dropout_u(n, keep, g)],
                         lambda K, x, u, keep=keep: K.dropout(x, u, keep), chk))
    return ops


def _smooth_ops():
    def tanh_y(n, g):
        return [_rand(n, g), torch.tanh(_rand(n, g, (20.0, -20.0)))]

    def sig_y(n, g):
        return [_rand(n, g), torch.sigmoid(_rand(n, g, (100.0, -100.0)) * 2)]
    a, b = f32(2.0), f32(-0.3)
    return [
        MapOp('tanh_fwd', 'map1', 1, lambda n, g: [_rand(n, g, (20.0, -20.0))], lambda K, x: K.tanh_fwd(x),
              lambda got, x: close('tanh_fwd', got, torch.tanh(x.double()), TOL)),
        MapOp('tanh_bwd', 'map2', 2, tanh_y, lambda K, gy, y: K.tanh_bwd(gy, y),
              lambda got, gy, y: close('tanh_bwd', got, gy.double() * (1 - y.double() ** 2), TOL)),
        MapOp('sigmoid_fwd', 'map1', 1, lambda n, g: [_rand(n, g, (100.0, -100.0))], lambda K, x: K.sigmoid_fwd(x),
              lambda got, x: close('sigmoid_fwd', got, torch.sigmoid(x.double()), TOL)),
        MapOp('sigmoid_bwd', 'map2', 2, sig_y, lambda K, gy, y: K.sigmoid_bwd(gy, y),
              lambda got, gy, y: close('sigmoid_bwd', got, gy.double() * y.double() * (1 - y.double()), TOL)),
        MapOp('axpby', 'map2', 2, lambda n, g: [_rand(n, g), _rand(n, g)], lambda K, x, y: K.axpby(x, y, a, b),
              lambda got, x, y: close('axpby', got, a * x.double() + b * y.double(), TOL)),
        MapOp('axpby(y=None)', 'map1', 1, lambda n, g: [_rand(n, g)], lambda K, x: K.axpby(x, None, a, 0.0),
              lambda got, x: exact('axpby, one operand', got, torch.tensor(a, dtype=torch.float32) * x)),
    ]


def _ln_ops():
    eps = f32(1e-5)

    def rsqrt_in(n, g):
        return [_plant(torch.rand(n, generator=g) * 4, (0.0,))]

    def chk_rsqrt(got, x):
        ref = 1.0 / torch.sqrt(x.double() + eps)
        within('rsqrt', got, ref, ref.abs(), 4)
    return [MapOp('mul', 'map2', 2, lambda n, g: [_rand(n, g), _rand(n, g)], lambda K, x, y: K.mul(x, y), lambda got, x, y: exact('mul', got, x * y)),
            MapOp('rsqrt', 'map1', 1, rsqrt_in, lambda K, x: K.rsqrt(x, eps), chk_rsqrt)]


MAP_OPS = {op.name: op for op in _lrelu_ops() + _dropout_ops() + _smooth_ops()}
LN_MAP_OPS = {op.name: op for op in _ln_ops()}
LN_MAP_SIZES = (1, 5, 1025)
# one operation per kernel template at the size of the second grid-stride pass
MAP_BIG_OPS = ('lrelu_fwd(0.2)', 'axpby')


def _map_op(name):
    return MAP_OPS.get(name) or LN_MAP_OPS[name]


def check_map(be, name, n, misaligned=None):
    """one map operation on 1-D operands of n elements; misaligned: the index of the operand that comes from off16"""
    op = _map_op(name)
    ins = op.make(n, gen('map', name, n))
    dv = [be.put(t, 'off16' if misaligned == i else 'dense') for i, t in enumerate(ins)]
    got = op.run(be.K, *dv)
    assert tuple(got.shape) == (n,)
    if n == 0:
        return
    op.check(got, *ins)


def check_map_empty(be, name):
    op = _map_op(name)
    ins = [torch.empty(0) for _ in range(op.nin)]
    got = op.run(be.K, *[be.dev(t) for t in ins])
    be.sync()
    assert got.numel() == 0


def check_axpby_in_place(be, n):
    g = gen('axpby-in-place', n)
    x, y = torch.randn(n, generator=g), torch.randn(n, generator=g)
    a, b = f32(0.9), f32(0.1)
    xd = be.dev(x)
    out = be.K.axpby(xd, be.dev(y), a, b, out=xd)
    assert out is xd
    close('axpby', xd, a * x.double() + b * y.double(), TOL)
    xo = be.off16(x)                                        # out from off16 (and x with it): the scalar branch writes in place as well
    assert be.K.axpby(xo, be.dev(y), a, b, out=xo) is xo
    close('axpby', xo, a * x.double() + b * y.double(), TOL)


# the second operand in the other memory layout: the wrappers repack it (match_layout -> copy4d) to the first one's
REPACK_OPS = ('dropout(0.8)', 'tanh_bwd', 'lrelu_bwd(0.2)')


def check_map_repack(be, name, first_cl):
    op = MAP_OPS[name]
    shape = (2, 5, 4, 6)
    n = 2 * 5 * 4 * 6
    ins = [t.view(shape) for t in op.make(n, gen('repack', name))]
    if name.startswith('dropout'):                     # (x, u): u follows x;  the others (gy, ref): gy follows ref
        lead, follow = 0, 1
    else:
        lead, follow = 1, 0
    dv = [None, None]
    dv[lead] = be.cl(ins[lead]) if first_cl else be.dev(ins[lead])
    dv[follow] = be.dev(ins[follow]) if first_cl else be.cl(ins[follow])
    got = op.run(be.K, *dv)
    assert got.stride() == dv[lead].stride()
    op.check(got, *ins)


# ------------------------------------------------------------------------------------------------------------------ copy4d
COPY_CASES = ('nchw->cl', 'cl->nchw', 'C = 1', 'H = W = 1', 'permuted source', 'every second row', 'into a larger buffer', 'past 4096 blocks')


def _cl_empty(be, shape, fill=None):
    n, c, h, w = shape
    t = torch.empty((n, h, w, c), device=be.device).permute(0, 3, 1, 2)
    if fill is not None:
        t.fill_(fill)
    return t


def check_copy4d(be, case):
    g = gen('copy4d', case)
    rnd = lambda *s: torch.randn(*s, generator=g)
    new = lambda *s: torch.full(s, SENTINEL, device=be.device)
    buf = None
    if case == 'nchw->cl':
        x = rnd(3, 5, 4, 6); src = be.dev(x); dst = _cl_empty(be, x.shape, SENTINEL)
    elif case == 'cl->nchw':
        x = rnd(3, 5, 4, 6); src = be.cl(x); dst = new(*x.shape)
    elif case == 'C = 1':                                   # ys = (24, 1, 6, 1): the channel stride ties with w's in the sort on output strides
        x = rnd(3, 1, 4, 6); src = be.dev(x); dst = _cl_empty(be, x.shape, SENTINEL)
        assert dst.stride() == (24, 1, 6, 1)
    elif case == 'H = W = 1':                               # ys = (5, 1, 1, 1): three equal strides
        x = rnd(3, 5, 1, 1); src = be.cl(x); dst = new(*x.shape)
        assert src.stride() == (5, 1, 5, 5) and dst.stride() == (5, 1, 1, 1)
    elif case == 'permuted source':
        base = rnd(3, 5, 6, 4); x = base.permute(0, 1, 3, 2); src = be.dev(base).permute(0, 1, 3, 2); dst = _cl_empty(be, x.shape, SENTINEL)
    elif case == 'every second row':
        base = rnd(3, 5, 8, 6); x = base[:, :, ::2]; src = be.dev(base)[:, :, ::2]; dst = new(*x.shape)
        assert not src.is_contiguous()
    elif case == 'into a larger buffer':
        x = rnd(3, 5, 4, 6); src = be.dev(x)
        buf = _cl_empty(be, (5, 5, 4, 6), SENTINEL); dst = buf[:3]
    else:
        x = rnd(2, 8, 256, 257); src = be.dev(x); dst = _cl_empty(be, x.shape, SENTINEL)
        assert x.numel() > 4096 * 256
    out = be.K.copy4d(src, dst)
    assert out is dst
    exact('copy4d', dst, x)
    if buf is not None:
        be.sync()
        assert (buf[3:] == SENTINEL).all()


# ------------------------------------------------------------------------------------------------------------------ pool2 / upsample2
RESAMPLE_SHAPES = ((1, 1, 2, 2), (3, 5, 8, 10), (2, 130, 4, 6))
RESAMPLE_LAYOUTS = ('nchw', 'cl', 'slice')
RESAMPLE_SCALES = (0.25, 1.0, 0.5)
POOL_BIG, UP_BIG = (1, 2, 1026, 2048), (1, 1, 513, 1024)          # past 4096 * 256 outputs


def _source(be, x, layout, g):
    if layout == 'nchw':
        return be.dev(x)
    if layout == 'cl':
        return be.cl(x)
    n, c, h, w = x.shape                                   # a window of a larger NCHW tensor: no dense layout at all
    big = torch.randn(n, c + 1, h + 1, w + 2, generator=g)
    big[:, 1:, :h, 1:1 + w] = x
    v = be.dev(big)[:, 1:, :h, 1:1 + w]
    assert tuple(v.shape) == tuple(x.shape)
    return v


def ref_pool2(x, scale):
    """elementwise.hip: y[n,c,p,q] = scale * (x[n,c,2p,2q] + x[n,c,2p+1,2q] + x[n,c,2p,2q+1] + x[n,c,2p+1,2q+1])"""
    return scale * (x[:, :, ::2, ::2] + x[:, :, 1::2, ::2] + x[:, :, ::2, 1::2] + x[:, :, 1::2, 1::2])


def ref_upsample2(x, scale):
    """y[n,c,h,w] = scale * x[n,c,h/2,w/2]"""
    n, c, h, w = x.shape
    idx_h = torch.arange(2 * h) // 2; idx_w = torch.arange(2 * w) // 2
    return scale * x[:, :, idx_h][:, :, :, idx_w]


def check_pool2(be, shape, layout, scale):
    g = gen('pool2', shape, layout)
    x = torch.randn(*shape, generator=g)
    y = be.K.pool2(_source(be, x, layout, g), scale)
    ref = ref_pool2(x.double(), f32(scale))
    if scale == 0.25:
        assert torch.equal(ref, tf_ops.mean_pool2(x.double()))
    within('pool2', y, ref, ref_pool2(x.double().abs(), abs(f32(scale))), be.d(2 + 1, 4))


def check_upsample2(be, shape, layout, scale):
    g = gen('upsample2', shape, layout)
    x = torch.randn(*shape, generator=g)
    y = be.K.upsample2(_source(be, x, layout, g), scale)
    want = ref_upsample2(x, torch.tensor(scale, dtype=torch.float32))
    if scale == 1.0:
        assert torch.equal(want, tf_ops.upsample2(x))
    exact('upsample2', y, want)


# ------------------------------------------------------------------------------------------------------------------ spatial_sum / spatial_bcast
SPATIAL_HW = {1: (1, 1), 3: (1, 3), 4: (2, 2), 5: (5, 1), 64: (8, 8)}
SPATIAL_C = (1, 63, 64, 65, 130)
SPATIAL_N = (1, 3)


def spatial_sum_d(hw):
    """spatial_sum_kernel: a lane adds every fourth position, (r0 + r1) + (r2 + r3) combines the four lanes, then the scale"""
    return -(-hw // 4) + 2 + 1


def check_spatial(be, n, hw, c):
    H, W = SPATIAL_HW[hw]
    g = gen('spatial', n, hw, c)
    x = torch.randn(n, c, H, W, generator=g)
    scale = f32(1.0 / 3)
    for src in (be.cl(x), be.dev(x)):                      # the NCHW form goes through to_channels_last first
        y = be.K.spatial_sum(src, scale)
        assert tuple(y.shape) == (n, c)
        within('spatial_sum', y, scale * x.double().sum(dim=(2, 3)), scale * x.double().abs().sum(dim=(2, 3)), be.d(spatial_sum_d(hw), hw))
    v = torch.randn(n, c, generator=g)
    for sc in (1.0, 0.5, scale):
        y = be.K.spatial_bcast(be.dev(v), H, W, sc)
        assert y.permute(0, 2, 3, 1).is_contiguous()
        exact('spatial_bcast', y, (torch.tensor(sc, dtype=torch.float32) * v)[:, :, None, None].expand(n, c, H, W))


# ------------------------------------------------------------------------------------------------------------------ sample_sum / sample_bcast
SAMPLE_M = {1: (1, 1, 1), 255: (5, 3, 17), 256: (4, 8, 8), 257: (257, 1, 1), 768: (3, 16, 16), 769: (769, 1, 1), 1024: (4, 16, 16),
            1025: (5, 5, 41), 16384: (16, 32, 32)}
SAMPLE_N = (1, 5)


def sample_sum_d(m):
    """sample_sum_kernel: a thread's s0 takes one addition per pass of either loop (at most ceil(m / 256)); (s0 + s1) + (s2 + s3); six
    shuffle steps; the four wave partials as a two-level tree; the scale"""
    return -(-m // 256) + 2 + 6 + 2 + 1


def check_sample(be, n, m):
    C, H, W = SAMPLE_M[m]
    assert C * H * W == m
    g = gen('sample', n, m)
    x = torch.randn(n, m, generator=g)
    scale = f32(1.0 / m)
    ref = scale * x.double().sum(dim=1)
    mag = scale * x.double().abs().sum(dim=1)
    x4 = x.view(n, H, W, C).permute(0, 3, 1, 2)            # the same memory read as a channels-last [n, C, H, W]
    for src in (be.dev(x), be.cl(x4)):
        y = be.K.sample_sum(src, scale)
        assert tuple(y.shape) == (n,)
        within('sample_sum', y, ref, mag, be.d(sample_sum_d(m), m))
    v = torch.randn(n, generator=g)
    for like, shape in ((be.dev(x), (n, m)), (be.cl(x4), (n, C, H, W))):
        for sc in (1.0, scale):
            y = be.K.sample_bcast(be.dev(v), like, sc)
            assert y.stride() == like.stride()
            exact('sample_bcast', y, (torch.tensor(sc, dtype=torch.float32) * v).reshape([n] + [1] * (len(shape) - 1)).expand(shape))


# ------------------------------------------------------------------------------------------------------------------ channel_affine
AFFINE_CASES = [(dims, c, off) for dims in (2, 4) for c in (1, 3, 128) for off in (True, False)]


def check_channel_affine(be, dims, c, with_offset):
    g = gen('affine', dims, c)
    x = torch.randn((7, c) if dims == 2 else (3, c, 5, 2), generator=g)
    s = torch.randn(c, generator=g); o = torch.randn(c, generator=g) if with_offset else None
    shp = [1, c] + [1] * (dims - 2)
    xs = x.double() * s.double().reshape(shp)
    ref = xs + (o.double().reshape(shp) if with_offset else 0.0)
    mag = xs.abs() + (o.double().abs().reshape(shp) if with_offset else 0.0)
    y = be.K.channel_affine(be.dev(x) if dims == 2 else be.cl(x), be.dev(s), be.dev(o) if with_offset else None)
    assert tuple(y.shape) == tuple(x.shape)
    within('channel_affine', y, ref, mag, 4)


# ------------------------------------------------------------------------------------------------------------------ real_prep / interpolate
REAL_PREP_CASES = [(n, denom, noise) for n in (1, 3073) for denom in (256.0, 255.0) for noise in (False, True)]


def check_real_prep(be, n, denom, noise):
    g = gen('real_prep', n, denom)
    xi = torch.randint(0, 256, (n,), generator=g, dtype=torch.int32)
    _plant(xi, (255, 0) if n > 1 else ((255,) if denom == 255.0 else (0,)))
    nz = torch.rand(n, generator=g) / 128 if noise else None
    y = be.K.real_prep(be.dev(xi), be.dev(nz) if noise else None, denom)
    ref = 2.0 * (xi.double() / denom - 0.5)
    if noise:
        close('real_prep', y, ref + nz.double(), TOL)
    else:
        exact('real_prep', y, 2.0 * (xi.float() / torch.tensor(denom, dtype=torch.float32) - 0.5))
        close('real_prep', y, ref, TOL)


INTERP_CASES = [(b, d) for b in (1, 6) for d in (1, 3072)]


def check_interpolate(be, b, d):
    g = gen('interp', b, d)
    r, f = torch.randn(b, d, generator=g), torch.randn(b, d, generator=g)
    alphas = [torch.tensor([v]) for v in (0.0, 1.0, 0.3)] if b == 1 else [_plant(torch.rand(b, generator=g), (0.0, 1.0))]
    for a in alphas:
        a = a.float()
        y = be.K.interpolate(be.dev(r), be.dev(f), be.dev(a.view(b, 1)))
        close('interpolate', y, r.double() + a.double().view(b, 1) * (f.double() - r.double()), TOL)
        yc = y.detach().cpu()
        for row in range(b):
            if a[row] == 0.0:
                assert torch.equal(yc[row], r[row])
            if a[row] == 1.0:
                assert torch.equal(yc[row], r[row] + (f[row] - r[row]))


# ------------------------------------------------------------------------------------------------------------------ colsum
COLSUM_ROWS = (1, 4, 31, 32, 33, 256, 257, 65536, 65537)
COLSUM_COLS = (1, 63, 64, 65, 130)
COLSUM_CASES = [(r, c) for r in COLSUM_ROWS for c in COLSUM_COLS if r < 65536 or c in (1, 65)]


def colsum_plan(rows):
    """elementwise.hip colsum_plan -> (blocks of stage 1, rows per block)"""
    nblk = max(1, min(256, (rows + 255) // 256))
    rpb = (rows + nblk - 1) // nblk
    return (rows + rpb - 1) // rpb, rpb


def colsum_d(rows):
    """colsum_stage_kernel: each of four row lanes adds every fourth row of its block, (r0 + r1) + (r2 + r3); stage 2 the same over the blocks"""
    nblk, rpb = colsum_plan(rows)
    return -(-rpb // 4) + 2 + ((-(-nblk // 4) + 2) if nblk > 1 else 0)


def colsum_inputs(rows, cols, ld):
    g = gen('colsum', rows, cols)
    buf = torch.randn(rows, ld, generator=g)
    x = buf[:, :cols]
    return buf, x.double().sum(dim=0), x.double().abs().sum(dim=0)


def check_colsum_channels(be, layout):
    N, Kc, P, Q = 3, 65, 5, 7
    x = torch.randn(N, Kc, P, Q, generator=gen('colsum_channels'))
    y = be.K.colsum_channels(be.dev(x) if layout == 'nchw' else be.cl(x))
    rows = N * P * Q
    within('colsum', y, x.double().sum(dim=(0, 2, 3)), x.double().abs().sum(dim=(0, 2, 3)), be.d(colsum_d(rows), rows))


# ------------------------------------------------------------------------------------------------------------------ filters
ROTATE, PHASES, SPREAD, SPREAD_FLIP = 0, 1, 2, 3
SPREAD_D = 4 + 1               # four additions onto the zero accumulator, then the scale
SPREAD_FILTERS = ((1, 1, 3, 128), (3, 3, 128, 3), (3, 1, 5, 7), (3, 3, 40, 24))
# scalar path (C = 3 | K = 3 | both ragged), 16-byte path with ragged tiles, several tiles each way; then 4 and 5 taps for PHASES
BATCH_FILTERS = ((1, 1, 3, 128), (3, 3, 128, 3), (3, 1, 5, 7), (3, 3, 40, 72), (3, 3, 68, 100), (4, 4, 5, 7), (5, 5, 8, 4), (2, 4, 3, 5))
PADS = ((0, 0), (0, 1), (1, 0), (1, 1))


def np_spread(w, scale, flip):
    """ctgan_hip.h: out[u,v,c,k] = scale * sum_{a,b in {0,1}} w[u-a, v-b, c, k]; flip writes out[R-u, S-v, k, c] instead"""
    R, S, C, K = w.shape
    out = np.zeros((R + 1, S + 1, C, K))
    for a in (0, 1):
        for b in (0, 1):
            out[a:a + R, b:b + S] += w
    out *= scale
    if flip:
        fl = np.zeros((R + 1, S + 1, K, C))
        for u in range(R + 1):
            for v in range(S + 1):
                fl[R - u, S - v] = out[u, v].T
        out = fl
    return out


def np_fold(w4, scale, flip):
    """ctgan_hip.h: out[r,s,c,k] = scale * sum_{a,b} W[r+a, s+b, c, k], W = w4 or (flip) W[u,v,c,k] = w4[R-u, S-v, k, c]"""
    R, S = w4.shape[0] - 1, w4.shape[1] - 1
    if flip:
        W = np.zeros((R + 1, S + 1, w4.shape[3], w4.shape[2]))
        for u in range(R + 1):
            for v in range(S + 1):
                W[u, v] = w4[R - u, S - v].T
    else:
        W = w4
    out = np.zeros((R, S) + W.shape[2:])
    for a in (0, 1):
        for b in (0, 1):
            out += W[a:a + R, b:b + S]
    return scale * out


def np_rotate(e):
    """igemm.hip: wT[r',s',k,c] = w[R-1-r', S-1-s', c, k]"""
    R, S, C, K = e.shape
    out = np.zeros((R, S, K, C), dtype=e.dtype)
    for r in range(R):
        for s in range(S):
            out[r, s] = e[R - 1 - r, S - 1 - s].T
    return out


def np_phases(e, pad_t, pad_l):
    """igemm.hip: wt[ph=(a,b)][t][v][k][c] = w[u][x][c][k], u = ((a + pad_t) & 1) + 2 (Tr-1-t), x = ((b + pad_l) & 1) + 2 (Ts-1-v); 0 where
    u >= R or x >= S"""
    R, S, C, K = e.shape
    Tr, Ts = (R + 1) // 2, (S + 1) // 2
    out = np.zeros((4, Tr, Ts, K, C), dtype=e.dtype)
    for ph in range(4):
        a, b = ph >> 1, ph & 1
        for t in range(Tr):
            for v in range(Ts):
                u, x = ((a + pad_t) & 1) + 2 * (Tr - 1 - t), ((b + pad_l) & 1) + 2 * (Ts - 1 - v)
                if u < R and x < S:
                    out[ph, t, v] = e[u, x].T
    return out


def filt(R, S, C, K, *key):
    return torch.randn(R, S, C, K, generator=gen('filter', R, S, C, K, *key))


def check_spread_fold(be, R, S, C, K, flip):
    K_ = be.K
    w = filt(R, S, C, K)
    scale = f32(0.3)
    sp = K_.filter_spread(be.dev(w), scale, flip)
    ref = np_spread(npf(w), scale, flip)
    assert tuple(sp.shape) == ref.shape
    within('filter_spread', sp, torch.from_numpy(ref), torch.from_numpy(np_spread(np.abs(npf(w)), scale, flip)), SPREAD_D)
    u = torch.randn(*ref.shape, generator=gen('fold', R, S, C, K, flip))
    fo = K_.filter_fold(be.dev(u), scale, flip)
    fref = np_fold(npf(u), scale, flip)
    assert tuple(fo.shape) == (R, S, C, K)
    within('filter_fold', fo, torch.from_numpy(fref), torch.from_numpy(np_fold(np.abs(npf(u)), scale, flip)), SPREAD_D)
    buf = torch.full((R + 1, S, C, K), SENTINEL, device=be.device)
    assert K_.filter_fold(be.dev(u), scale, flip, out=buf[:R]).data_ptr() == buf.data_ptr()
    be.sync()
    assert torch.equal(buf[:R], fo) and (buf[R:] == SENTINEL).all()
    # the adjoint identity <spread(w), u> = <w, fold(u)> on the code's own outputs, in fp64, to the bound of the two sums
    lhs = float((npf(sp) * npf(u)).sum()); rhs = float((npf(w) * npf(fo)).sum())
    bound = SPREAD_D * U * (float((np_spread(np.abs(npf(w)), scale, flip) * np.abs(npf(u))).sum()) +
                            float((np.abs(npf(w)) * np_fold(np.abs(npf(u)), scale, flip)).sum()))
    note('spread / fold adjoint (of bound)', abs(lhs - rhs) / bound)
    assert abs(lhs - rhs) <= bound


def job_shape(kind, R, S, C, K):
    if kind == ROTATE:
        return (R * S * C * K,)
    if kind == PHASES:
        return (4 * ((R + 1) // 2) * ((S + 1) // 2) * C * K,)
    return (R + 1, S + 1, K, C) if kind == SPREAD_FLIP else (R + 1, S + 1, C, K)


def filter_jobs(shapes, phases=True):
    """every kind x pre the entry point accepts, PHASES at all four pads -> [(w, kind, pad_t, pad_l, scale, pre, pre_scale)]"""
    jobs = []
    for i, shape in enumerate(shapes):
        w = filt(*shape, 'batch', i)
        for pre in (0, SPREAD, SPREAD_FLIP):
            ps = f32(0.25) if pre else 1.0
            jobs.append((w, ROTATE, 0, 0, 1.0, pre, ps))
            if phases:
                jobs.extend((w, PHASES, pt, pl, 1.0, pre, ps) for pt, pl in PADS)
        jobs.append((w, SPREAD, 0, 0, f32(0.25), 0, 1.0))
        jobs.append((w, SPREAD_FLIP, 0, 0, f32(0.7), 0, 1.0))
    return jobs


def check_filter_jobs(be, jobs):
    """one K.filter_batch call over `jobs`; every destination is the head of a sentinel-filled buffer"""
    call, bufs = [], []
    for w, kind, pt, pl, scale, pre, ps in jobs:
        R, S, C, K = w.shape
        eff = (R, S, C, K) if not pre else ((R + 1, S + 1, K, C) if pre == SPREAD_FLIP else (R + 1, S + 1, C, K))
        shape = job_shape(kind, *eff)
        n = int(np.prod(shape))
        buf = torch.full((n + 64,), SENTINEL, device=be.device)
        bufs.append((buf, n, shape))
        call.append((be.dev(w), buf[:n].view(shape), kind, pt, pl, scale, pre, ps))
    be.K.filter_batch(call)
    be.sync()
    for (w, kind, pt, pl, scale, pre, ps), (buf, n, shape) in zip(jobs, bufs):
        got = buf[:n].cpu()
        assert (buf[n:] == SENTINEL).all() and not (got == SENTINEL).any(), (tuple(w.shape), kind, pre)
        wn, an = npf(w), np.abs(npf(w))
        if kind in (SPREAD, SPREAD_FLIP):
            ref, mag = np_spread(wn, scale, kind == SPREAD_FLIP), np_spread(an, scale, kind == SPREAD_FLIP)
        else:
            lay = np_rotate if kind == ROTATE else (lambda e: np_phases(e, pt, pl))
            if pre:
                ref, mag = lay(np_spread(wn, ps, pre == SPREAD_FLIP)), lay(np_spread(an, ps, pre == SPREAD_FLIP))
            else:
                exact('filter_batch layout', got, torch.from_numpy(lay(w.numpy())).reshape(-1))
                continue
        within('filter_batch', got, torch.from_numpy(ref).reshape(-1), torch.from_numpy(mag).reshape(-1), SPREAD_D)


def check_fold_jobs(be, shapes):
    """one K.filter_fold_batch call: job i folds a [(R+1),(S+1),..] gradient of shape i, flip alternating"""
    call, keep = [], []
    for i, (R, S, C, K) in enumerate(shapes):
        flip = bool(i % 2)
        u = torch.randn((R + 1, S + 1, K, C) if flip else (R + 1, S + 1, C, K), generator=gen('foldjob', i, R, S, C, K))
        n = R * S * C * K
        buf = torch.full((n + 64,), SENTINEL, device=be.device)
        scale = f32(0.25 + 0.01 * i)
        call.append((be.dev(u), scale, flip, buf[:n].view(R, S, C, K)))
        keep.append((u, scale, flip, buf, n))
    be.K.filter_fold_batch(call)
    be.sync()
    for u, scale, flip, buf, n in keep:
        assert (buf[n:] == SENTINEL).all()
        within('filter_fold_batch', buf[:n], torch.from_numpy(np_fold(npf(u), scale, flip)).reshape(-1),
               torch.from_numpy(np_fold(np.abs(npf(u)), scale, flip)).reshape(-1), SPREAD_D)


FOLD_BIG = [(3, 3, 256, 128), (1, 1, 3, 128)]            # 294912 elements: more than 1024 blocks of 256 cover in one pass, beside a 1x1 job
FOLD_MANY = [(1 + i % 3, 1 + (i // 3) % 2, 3 + i, 5 + 2 * i) for i in range(17)]


# ------------------------------------------------------------------------------------------------------------------ small linear
# (N, C, K, x, w, kernel): x / w: 'dense', 'off16', or ('ld', row stride); kernel: the name ctgan_last_kernel must report, None = not a linear_ one
ROW, GEMV = 'linear_small_fwd', 'linear_gemv_fwd'
LIN_SHAPES = ((1, 1, 1), (3, 63, 2), (4, 64, 9), (5, 65, 16), (70, 128, 1), (37, 130, 10), (17, 1000, 1))
LIN_FWD_CASES = [(N, C, K, 'dense', 'dense', ROW) for N, C, K in LIN_SHAPES] + [(5, 128, 17, 'dense', 'dense', None)]
LIN_FWD_CASES += [(5, 65, 16, ('ld', 70), 'dense', ROW), (3, 63, 2, 'off16', 'off16', ROW)]       # a row stride larger than C; both operands off 16 bytes
for _N in (1, 5):
    LIN_FWD_CASES += [
        (_N, 1024, 1, 'dense', 'dense', GEMV), (_N, 1028, 1, 'dense', 'dense', GEMV), (_N, 8192, 1, 'dense', 'dense', GEMV),
        (_N, 1020, 1, 'dense', 'dense', ROW), (_N, 1022, 1, 'dense', 'dense', ROW), (_N, 1024, 2, 'dense', 'dense', ROW),
        (_N, 1024, 1, 'off16', 'dense', ROW), (_N, 1024, 1, 'dense', 'off16', ROW),
        (_N, 1024, 1, ('ld', 1025), 'dense', ROW), (_N, 1024, 1, ('ld', 1028), 'dense', GEMV)]
LIN_FWD_IDS = ['%d-%d-%d-x:%s-w:%s-%s' % (N, C, K, 'ld%d' % x[1] if isinstance(x, tuple) else x, w, k or 'gemm') for N, C, K, x, w, k in LIN_FWD_CASES]
LIN_FWD_LARGE = [(65536, 4, 1, ROW), (65537, 4, 1, None)]


def lin_fwd_d(C, kernel):
    if kernel == ROW:
        return -(-C // 64) + 6 + 1                         # a lane's fused multiply-adds, six shuffle steps, the bias
    if kernel == GEMV:
        return 4 * -(-C // 1024) + 6 + 2 + 1               # ... four per pass, six shuffle steps, the four wave partials as a tree, the bias
    return C + 2                                           # the GEMM path: any order


def lin_x(be, x, how):
    N, C = x.shape
    if isinstance(how, tuple):
        buf = torch.full((N, how[1]), SENTINEL, device=be.device)
        buf[:, :C] = x.to(be.device)
        v = buf[:, :C].unsqueeze(-1).unsqueeze(-1)
        assert v.stride(0) == how[1] and v.stride(1) == 1
        return v
    return be.put(x, how).view(N, C, 1, 1)


def lin_inputs(N, C, K, relu, *key):
    """x, w, b with (under the ReLU flag) no pre-activation within 1e-4 of zero relative to its term magnitudes: the first seed that has"""
    for trial in range(64):
        g = gen('lin', N, C, K, trial, *key)
        x, w, b = torch.randn(N, C, generator=g), torch.randn(C, K, generator=g), torch.randn(K, generator=g)
        pre = x.double() @ w.double()
        mag = x.double().abs() @ w.double().abs()
        if not relu or (bool((pre.abs() >= 1e-4 * mag).all()) and bool(((pre + b.double()).abs() >= 1e-4 * (mag + b.double().abs())).all())):
            return x, w, b
    raise AssertionError('no seed met the input condition')


def check_last_kernel(be, want, prefix='linear_'):
    if not be.gpu:
        return
    name = be.K.last_kernel()
    if want is None:
        assert not name.startswith(prefix), name
    else:
        assert name == want, (name, want)


def check_lin_fwd(be, N, C, K, xhow, whow, kernel, combos=((True, False), (True, True), (False, False), (False, True))):
    g = be.K.ConvGeom(C, 1, 1, K, 1, 1)
    for with_bias, relu in combos:
        x, w, b = lin_inputs(N, C, K, relu)
        pre = x.double() @ w.double() + (b.double() if with_bias else 0.0)
        mag = x.double().abs() @ w.double().abs() + (b.double().abs() if with_bias else 0.0)
        if relu:
            assert (pre.abs() >= 1e-4 * mag).all()
        ref = torch.relu(pre) if relu else pre
        y = be.K.conv_fwd(lin_x(be, x, xhow), be.put(w.view(1, 1, C, K), whow), be.dev(b) if with_bias else None, g, relu=relu)
        check_last_kernel(be, kernel)
        assert tuple(y.shape) == (N, K, 1, 1)
        within('small-linear forward%s' % (', GEMM path' if kernel is None else ''), y, ref, mag, be.d(lin_fwd_d(C, kernel), C))


LIN_DGRAD_CASES = [s + ('linear_small_dgrad',) for s in LIN_SHAPES] + [(5, 128, 17, None)]


def check_lin_dgrad(be, N, C, K, kernel):
    g = be.K.ConvGeom(C, 1, 1, K, 1, 1)
    gn = gen('lin-dgrad', N, C, K)
    gy, w, b = torch.randn(N, K, generator=gn), torch.randn(C, K, generator=gn), torch.randn(C, generator=gn)
    d = be.d(K + 1, K) if kernel else K + 2             # the GEMM path: any order
    for with_bias, strided, gy_cl in itertools.product((False, True), (False, True), (False, True)):
        ref = gy.double() @ w.double().t() + (b.double() if with_bias else 0.0)
        mag = gy.double().abs() @ w.double().abs().t() + (b.double().abs() if with_bias else 0.0)
        gyd = be.cl(gy.view(N, K, 1, 1)) if gy_cl else be.dev(gy.view(N, K, 1, 1))
        gx = be.K.conv_dgrad(gyd, be.dev(w.view(1, 1, C, K)), g, N, out_strides=(C + 3, 1, 1, 1) if strided else None,
                             bias=be.dev(b) if with_bias else None)
        check_last_kernel(be, kernel)
        assert tuple(gx.shape) == (N, C, 1, 1) and (not strided or gx.stride(0) == C + 3)
        within('small-linear data gradient%s' % ('' if kernel else ', GEMM path'), gx, ref, mag, d)


LIN_WGRAD_ROWS = (1, 15, 16, 17, 70)
LIN_WGRAD_C = (1, 63, 64, 65, 130)
LIN_WGRAD_K = (1, 10, 16)


def lin_wgrad_d(rows):
    """linear_small_wgrad_kernel: each of 16 row lanes takes every sixteenth row, then the 16 partials are added in order"""
    return -(-rows // 16) + 16


def check_lin_wgrad(be, rows, with_bias, C=None, K=None, gy_slice=False, kernel='linear_small_wgrad'):
    for C_, K_ in itertools.product(LIN_WGRAD_C if C is None else (C,), LIN_WGRAD_K if K is None else (K,)):
        g = be.K.ConvGeom(C_, 1, 1, K_, 1, 1)
        gn = gen('lin-wgrad', rows, C_, K_)
        x, gy = torch.randn(rows, C_, generator=gn), torch.randn(rows, K_, generator=gn)
        xd = be.dev(x.view(rows, C_, 1, 1))
        if gy_slice:
            buf = torch.full((rows, K_ + 5), SENTINEL, device=be.device)
            buf[:, 2:2 + K_] = gy.to(be.device)
            gyd = buf[:, 2:2 + K_].unsqueeze(-1).unsqueeze(-1)
            assert gyd.stride(0) == K_ + 5
        else:
            gyd = be.dev(gy.view(rows, K_, 1, 1))
        d = be.d(lin_wgrad_d(rows), rows) if kernel else rows + 2
        outs = []
        for _ in range(2):
            res = be.K.conv_wgrad(xd, gyd, g, with_bias=with_bias)
            check_last_kernel(be, kernel)
            outs.append(res if with_bias else (res, None))
        dw, db = outs[0]
        assert tuple(dw.shape) == (1, 1, C_, K_)
        within('small-linear weight gradient', dw, x.double().t() @ gy.double(), x.double().abs().t() @ gy.double().abs(), d)
        assert (db is not None) == with_bias
        if with_bias:
            assert tuple(db.shape) == (K_,)
            within('small-linear bias gradient', db, gy.double().sum(dim=0), gy.double().abs().sum(dim=0), d)
            assert torch.equal(outs[1][1], db)
        assert torch.equal(outs[1][0], dw)                 # documented as deterministic: the same bits twice
