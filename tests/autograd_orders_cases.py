"""The derivative order of every torch.autograd.Function of ctgan_amd/functional.py, declared in one table and checked against fp64: shared by
tests/test_gpu_autograd_orders.py (the HIP kernels) and tests/test_autograd_orders_standins.py (the CPU stand-ins made opaque to autograd,
which is what a kernel that writes into a fresh torch.empty through ctypes is).  A plain helper module: no fixtures, no marks.

TABLE holds one or more entries per Function class (the completeness test compares its class names with the classes found in the module):
  order     'twice': the backward is built from Functions of the set, so a gradient penalty may differentiate through it a second time;
            'once': the backward calls kernel wrappers directly - it must refuse a second differentiation, never return a number
  make      seed -> Case: tiny fp32 inputs, a builder that reaches the class through its public entry point where one exists, and an fp64
            reference of the same operation in plain torch ops (its derivatives are torch's own)
The check of a 'twice' entry takes inputs xs, a cotangent gy that requires grad and random u_i:
  first = grad(y, xs, gy, create_graph=True);  second = grad(sum <first_i, u_i>, xs + [gy], allow_unused=True)
and compares y, every first_i and every second_j with the same in fp64 as max |a - b| / max |b|.  Where the fp64 cotangent is identically
zero the result must be None or exactly zero; where it is not, None is a failure - the missing edge.  The same op is then run as
op(MulFn(x, w)), with w among the inputs: a cut that an isolated op reports as torch's "does not require grad" is silent inside a network,
and the chain is the form that catches it.  The check of a 'once' entry: a plain backward matches fp64, and a second differentiation
raises RuntimeError (functional._once / _first_order_only) - it never returns a number, and never None in a number's place.

Bounds: 2e-5 forward, 3e-5 first and second order (the project's own, tests/test_gpu_ssl_cifar.py and tests/test_gpu_kernels.py; a second-order
cotangent of these ops is one or two more launches of the same kernels); the batch-norm entries keep the 1e-4 of tests/test_gpu_arch64.py.
Kinked ops: the inputs are drawn again under the next seed until every fp64 pre-activation has |z| >= 1e-3, asserted before the backend runs.
Dropout-family references read the diagonal (mask / keep [x slope]) off the op applied to ones; the draws are pinned by the Philox tests.
"""
import contextlib
import zlib

import pytest
import torch
import torch.nn.functional as TF
from torch.autograd import Function

from oracle import tf_ops

FWD_TOL, GRAD_TOL, SECOND_TOL, BN_TOL = 2e-5, 3e-5, 3e-5, 1e-4
KINK = 1e-3
REFUSAL = 'first order only'
MEASURED = {}


def note(group, err):
    MEASURED[group] = max(MEASURED.get(group, 0.0), float(err))


def report():
    return '\n'.join('%-44s %.3g' % kv for kv in sorted(MEASURED.items()))


def gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()) % 100000)


class Backend:
    """Where the code under test runs: K = ctgan_amd.kernels (HIP, or the opaque stand-ins), F = ctgan_amd.functional over the same K."""

    def __init__(self, K, F, device):
        self.K, self.F, self.device = K, F, device
        self.gpu = device != 'cpu'

    def dev(self, t):
        return t.detach().clone().contiguous().to(self.device)

    def cl(self, t):
        n, c, h, w = t.shape
        out = torch.empty((n, h, w, c), device=self.device, dtype=t.dtype).permute(0, 3, 1, 2)
        out.copy_(t.to(self.device))
        return out

    def put(self, t, lay=None):
        return self.cl(t) if (lay or ('cl' if t.dim() == 4 else 'dense')) == 'cl' else self.dev(t)

    def like(self, t, ref):
        out = torch.empty_strided(ref.shape, ref.stride(), dtype=ref.dtype, device=ref.device)
        out.copy_(t.to(ref.device))
        return out

    def ctr(self, step=3):
        return torch.tensor([step], dtype=torch.int64, device=self.device)

    def rng(self, seed=7):
        from ctgan_amd import rng as R
        return R.DeviceRNG(seed=seed, rank=0, device=self.device)


def make_opaque(K, monkeypatch):
    """Every stand-in installed in K runs under torch.no_grad(): its result has no grad_fn, as a kernel's has none.  (Detaching the result
    is not enough - copy4d(g, out) writes into its argument.)  -> the names wrapped"""
    names = [n for n, f in vars(K).items() if callable(f) and not isinstance(f, type) and (getattr(f, '__module__', None) or '').startswith('tests.')]
    for n in names:
        monkeypatch.setattr(K, n, torch.no_grad()(getattr(K, n)))
    return names


def function_classes(F):
    return {n for n, c in vars(F).items() if isinstance(c, type) and issubclass(c, Function) and c is not Function and c.__module__ == F.__name__}


# ------------------------------------------------------------------------------------------------------------------ table
class Case:
    """xs: fp32 CPU inputs that take a gradient; run(be, *xs_backend) and ref(*xs_fp64) -> tensor or tuple (None entries dropped);
    lay: layout per input ('cl', 'dense'; default channels-last for 4-D); pre(*xs_fp64) -> pre-activations of the kinks;
    feed: per input, what the backend is given for x where that is not x itself (the tail heads take y = relu(z) * mask and return d/dz);
    param: the first input is handed over as a parameter of the tflib registry; setup(be): run before the reference (the dropout family
    reads its diagonal off the backend there); contract: the inputs whose first-order gradients enter the second-order contraction
    (default all - the fused Layernorm leaves out its parameter gradients, whose derivatives no loss uses and its backward refuses)."""

    def __init__(self, xs, run, ref, lay=None, pre=None, feed=None, tol=None, param=False, setup=None, contract=None):
        self.xs, self.run, self.ref, self.pre, self.param, self.setup = xs, run, ref, pre, param, setup
        self.contract = contract if contract is not None else list(range(len(xs)))
        self.lay = lay or [None] * len(xs)
        self.feed = feed or [None] * len(xs)
        self.tol = tol


class Entry:
    def __init__(self, cls, order, name, make, chain):
        self.cls, self.order, self.name, self.make, self.chain = cls, order, name, make, chain

    @property
    def id(self):
        return '%s-%s' % (self.cls, self.name)


TABLE = []


def entry(cls, order, name, chain=True):
    def deco(make):
        TABLE.append(Entry(cls, order, name, make, chain and order == 'twice'))
        return make
    return deco


def entries(order):
    return [e for e in TABLE if e.order == order]


def declared():
    """class name -> its one declared order"""
    out = {}
    for e in TABLE:
        assert out.setdefault(e.cls, e.order) == e.order, e.cls
    return out


# ------------------------------------------------------------------------------------------------------------------ the checks
def _flat(y):
    return tuple(t for t in (y if isinstance(y, (tuple, list)) else (y,)) if t is not None)


def _scalars_as_one(y):
    """several scalar outputs (the loss heads' cost and its terms) are compared as one vector: the cost is a sum in which the terms may cancel"""
    return (torch.stack([t.detach().cpu().double() for t in y]),) if len(y) > 1 and all(t.dim() == 0 for t in y) else y


def relerr(a, b):
    a = a.detach().cpu().double(); b = b.detach().cpu().double()
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-30)).item()


def compare(group, what, got, ref, tol):
    if ref is None or not bool(ref.ne(0).any()):
        assert got is None or not bool(got.ne(0).any()), '%s %s: fp64 is identically zero, got a non-zero tensor' % (group, what)
        return
    assert got is not None, '%s %s: None where fp64 is not zero - a missing edge' % (group, what)
    assert tuple(got.shape) == tuple(ref.shape), (group, what, got.shape, ref.shape)
    assert bool(torch.isfinite(got).all()), (group, what)
    e = relerr(got, ref)
    note('%s %s' % (group, what.split('[')[0]), e)
    print('%s %s %.3g' % (group, what, e))
    assert e < tol, (group, what, e, tol)


@contextlib.contextmanager
def spy(cls):
    """counts the forward calls of a Function class"""
    calls = [0]
    orig = cls.__dict__['forward']

    def forward(*a, **k):
        calls[0] += 1
        return orig.__func__(*a, **k)
    cls.forward = staticmethod(forward)
    try:
        yield calls
    finally:
        cls.forward = orig


def draw(e, chained):
    """The first seed whose kinks are clear of the inputs -> (case, w or None, the effective fp64 inputs' kink margin)."""
    for seed in range(64):
        case = e.make(seed)
        w = None
        xs = [x.double() for x in case.xs]
        if chained:
            w = 1.0 + 0.5 * (torch.rand(case.xs[0].shape, generator=gen(e.id, 'w', seed)) - 0.5)
            xs[0] = xs[0] * w.double()
        if case.pre is None:
            return case, w
        with torch.no_grad():
            zs = _flat(case.pre(*xs))
        if all(bool((z.abs() >= 2 * KINK).all()) for z in zs):
            return case, w
    raise AssertionError('%s: no seed keeps the kinks clear' % e.id)


def _reference(case, w, gys, us, second):
    xs = [x.double().requires_grad_(True) for x in case.xs]
    leaves = list(xs)
    ins = list(xs)
    if w is not None:
        wl = w.double().requires_grad_(True)
        ins[0] = xs[0] * wl
        leaves.insert(1, wl)
    if case.pre is not None:           # asserted BEFORE the backend runs: a sign flip at a kink can neither mask nor fake an error
        with torch.no_grad():
            for z in _flat(case.pre(*ins)):
                assert bool((z.abs() >= KINK).all()), z.abs().min().item()
    y = _flat(case.ref(*ins))
    if gys is None:
        return y, None, None, None
    gl = [g.double().requires_grad_(True) for g in gys]
    first = torch.autograd.grad(y, leaves, gl, create_graph=second, allow_unused=True)
    sec = None
    if second:
        s = sum((f * u.double()).sum() for f, u in zip(first, us) if f is not None and u is not None)
        sec = torch.autograd.grad(s, leaves + gl, allow_unused=True) if s.requires_grad else [None] * (len(leaves) + len(gl))
    return y, first, sec, leaves


def _backend_graph(be, case, w):
    leaves = [be.put(f(x) if f is not None else x, lay).requires_grad_(True) for x, lay, f in zip(case.xs, case.lay, case.feed)]
    if case.param:
        import ctgan_amd.tflib as lib
        lib.delete_all_params()
        leaves[0] = lib.param('Orders.w', leaves[0].detach())
    ins = list(leaves)
    if w is not None:
        wl = be.like(w, leaves[0]).requires_grad_(True)
        ins[0] = be.F.MulFn.apply(leaves[0], wl)
        leaves.insert(1, wl)
    return leaves, _flat(case.run(be, *ins))


def _cotangents(e, y, n_leaves, shapes):
    g = gen(e.id, 'cot')
    gys = [torch.randn(t.shape, generator=g) for t in y]
    us = [torch.randn(s, generator=g) if s is not None else None for s in shapes]
    return gys, us


def check_twice(be, e, chained=False):
    group = e.id + ('+mul' if chained else '')
    case, w = draw(e, chained)
    tol = case.tol or {}
    if case.setup is not None:
        case.setup(be)
    y0, _, _, _ = _reference(case, w, None, None, False)
    shapes = [x.shape if i in case.contract else None for i, x in enumerate(case.xs)]
    if w is not None:
        shapes.insert(1, w.shape if 0 in case.contract else None)
    gys, us = _cotangents(e, y0, len(shapes), shapes)
    yr, fr, sr, _ = _reference(case, w, gys, us, True)
    with spy(getattr(be.F, e.cls)) as calls:
        leaves, y = _backend_graph(be, case, w)
        assert len(y) == len(yr)
        for i, (a, b) in enumerate(zip(_scalars_as_one(y), _scalars_as_one(yr))):
            compare(group, 'y[%d]' % i, a, b.detach(), tol.get('y', FWD_TOL))
        gl = [be.like(g, t).requires_grad_(True) for g, t in zip(gys, y)]
        first = torch.autograd.grad(y, leaves, gl, create_graph=True, allow_unused=True)
        for i, (a, b) in enumerate(zip(first, fr)):
            compare(group, 'first[%d]' % i, a, None if b is None else b.detach(), tol.get('first', GRAD_TOL))
        s = sum((f * u.to(f.device)).sum() for f, u in zip(first, us) if f is not None and u is not None)
        if torch.is_tensor(s) and s.requires_grad:
            sec = torch.autograd.grad(s, leaves + gl, allow_unused=True)
        else:
            sec = [None] * (len(leaves) + len(gl))                 # nothing of `first` is connected to the graph
        for i, (a, b) in enumerate(zip(sec, sr)):
            compare(group, 'second[%d]' % i, a, b, tol.get('second', SECOND_TOL))
        assert calls[0] > 0, '%s: the builder never reached %s' % (group, e.cls)
    if be.gpu:
        torch.cuda.synchronize()


def check_once(be, e):
    group = e.id
    case, _ = draw(e, False)
    tol = case.tol or {}
    if case.setup is not None:
        case.setup(be)
    y0, _, _, _ = _reference(case, None, None, None, False)
    gys, us = _cotangents(e, y0, len(case.xs), [x.shape for x in case.xs])
    yr, fr, _, _ = _reference(case, None, gys, us, False)
    with spy(getattr(be.F, e.cls)) as calls:
        leaves, y = _backend_graph(be, case, None)
        assert len(y) == len(yr)
        for i, (a, b) in enumerate(zip(_scalars_as_one(y), _scalars_as_one(yr))):
            compare(group, 'y[%d]' % i, a, b.detach(), tol.get('y', FWD_TOL))
        gl = [be.like(g, t) for g, t in zip(gys, y)]
        first = torch.autograd.grad(y, leaves, gl, allow_unused=True)
        for i, (a, b) in enumerate(zip(first, fr)):
            compare(group, 'first[%d]' % i, a, b, tol.get('first', GRAD_TOL))
        assert calls[0] > 0, '%s: the builder never reached %s' % (group, e.cls)
    # a second differentiation refuses, already at the first backward under create_graph
    leaves, y = _backend_graph(be, case, None)
    gl = [be.like(g, t).requires_grad_(True) for g, t in zip(gys, y)]
    with pytest.raises(RuntimeError, match=REFUSAL):
        first = torch.autograd.grad(y, leaves, gl, create_graph=True, allow_unused=True)
        s = sum((f * u.to(f.device)).sum() for f, u in zip(first, us) if f is not None and u is not None)
        assert torch.is_tensor(s) and s.requires_grad, '%s: the first-order gradient is a constant to autograd - a silent cut' % group
        sec = torch.autograd.grad(s, leaves + gl, allow_unused=True)
        raise AssertionError('%s: differentiated twice and returned %s' % (group, [None if t is None else tuple(t.shape) for t in sec]))
    if be.gpu:
        torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------------------------ inputs and references
SHAPES = {'cl6': ((3, 6, 4, 4), 'cl'), 'cl8': ((2, 8, 4, 4), 'cl'), '2d': ((5, 7), 'dense'), 'nchw': ((3, 6, 4, 4), 'dense')}
ALL, CL, FOUR = ('cl6', 'cl8', '2d', 'nchw'), ('cl6', 'cl8'), ('cl6', 'cl8', 'nchw')


def away(x, eps=0.1):
    """no value within eps of zero"""
    return x + eps * torch.where(x >= 0, torch.ones_like(x), -torch.ones_like(x))


def rnd(g, *shape):
    return torch.randn(*shape, generator=g)


def ident(*xs):
    return xs


def conv_ref(x, w, b, stride):
    y = tf_ops.conv2d_same(x, w, stride)
    return y if b is None else y + b.view(1, -1, 1, 1)


def dgrad_ref(gy, w, shape, stride):
    """the adjoint of x -> conv_same(x, w) at gy, as a differentiable function of (gy, w)"""
    z = torch.zeros(shape, dtype=gy.dtype, requires_grad=True)
    with torch.enable_grad():
        (dx,) = torch.autograd.grad(conv_ref(z, w, None, stride), z, gy, create_graph=True)
    return dx


def wgrad_ref(x, gy, wshape, stride):
    z = torch.zeros(wshape, dtype=gy.dtype, requires_grad=True)
    with torch.enable_grad():
        (dw,) = torch.autograd.grad(conv_ref(x, z, None, stride), z, gy, create_graph=True)
    return dw


def im2col_ref(x, R, S, stride, cpad):
    """cols[n, (r S + s) C + c, p, q] = SAME-padded x[n, c, p stride + r, q stride + s]; channels past R S C are zero"""
    N, C, H, W = x.shape
    P, Q = -(-H // stride), -(-W // stride)
    _, pt, pb = tf_ops.same_pads(H, R, stride)
    _, pl, pr = tf_ops.same_pads(W, S, stride)
    xp = TF.pad(x, (pl, pr, pt, pb))
    parts = [xp[:, :, r:r + (P - 1) * stride + 1:stride, s:s + (Q - 1) * stride + 1:stride] for r in range(R) for s in range(S)]
    parts.append(x.new_zeros(N, cpad - R * S * C, P, Q))
    return torch.cat(parts, 1)


def adjoint_of(fn, shape, g):
    """the adjoint of the linear map fn at g, differentiable in g"""
    z = torch.zeros(shape, dtype=g.dtype, requires_grad=True)
    with torch.enable_grad():
        (a,) = torch.autograd.grad(fn(z), z, g, create_graph=True)
    return a


def spread_ref(w, scale, flip):
    """[R,S,C,K] -> scale * (the sum of the four one-tap shifts) [(R+1),(S+1),C,K]; flip: rotated by 180 degrees, I/O swapped"""
    out = sum(TF.pad(w, (0, 0, 0, 0, ds, 1 - ds, dr, 1 - dr)) for dr in (0, 1) for ds in (0, 1)) * scale
    return torch.flip(out, (0, 1)).permute(0, 1, 3, 2) if flip else out


def ln_ref(x, scale, offset, eps, relu=False, labels=None):
    dims = tuple(range(1, x.dim()))
    m = x.mean(dim=dims, keepdim=True)
    v = ((x - m) ** 2).mean(dim=dims, keepdim=True)
    xh = (x - m) / torch.sqrt(v + eps)
    tail = [1] * (x.dim() - 2)
    if labels is not None:
        s, o = scale[labels.long()].reshape([x.shape[0], -1] + tail), offset[labels.long()].reshape([x.shape[0], -1] + tail)
    else:
        s, o = scale.reshape([1, -1] + tail), offset.reshape([1, -1] + tail)
    y = xh * s + o
    return torch.relu(y) if relu else y


def bn_ref(x, scale, offset, groups, eps):
    """training-mode batch norm per statistic group over (n, h, w), biased variance; scale / offset [C]"""
    x4 = x if x.dim() == 4 else x.reshape(x.shape[0], x.shape[1], 1, 1)
    per = x4.shape[0] // groups
    outs = []
    for gi in range(groups):
        xs = x4[gi * per:(gi + 1) * per]
        m = xs.mean(dim=(0, 2, 3), keepdim=True)
        v = ((xs - m) ** 2).mean(dim=(0, 2, 3), keepdim=True)
        outs.append((xs - m) / torch.sqrt(v + eps) * scale.reshape(1, -1, 1, 1) + offset.reshape(1, -1, 1, 1))
    return torch.cat(outs).reshape(x.shape)


def gate_ref(z):
    return torch.sigmoid(z[:, ::2]) * torch.tanh(z[:, 1::2])


def elu_ref(x):
    return torch.where(x > 0, x, torch.expm1(torch.clamp(x, max=0)))


def lrelu_ref(x, alpha):
    return torch.where(x > 0, x, alpha * x)


def hinge(t):
    return torch.where(t >= 0, t, torch.zeros_like(t))


def ce_ref(logits, labels):
    return -torch.log_softmax(logits, 1)[torch.arange(logits.shape[0]), labels.long()].mean()


def lse(x):
    return torch.logsumexp(x, 1)


def ct_rows(d, d_, f, f_, lam2):
    return lam2 * (d - d_) ** 2 + lam2 * 0.1 * ((f - f_) ** 2).mean(dim=1)


def critic_heads_ref(d, f, a, labels, B, lam2, M, scale, gp):
    wgan = d[B:2 * B].mean() - d[:B].mean()
    ct = hinge(ct_rows(d[:B], d[2 * B:], f[:B], f[2 * B:], lam2) - M).mean()
    ac = ce_ref(a[:B], labels) if a is not None else torch.zeros((), dtype=d.dtype)
    return wgan + ct + gp + scale * ac, wgan, ct, ac


def diag_of(op, be, x, lay):
    """the diagonal of a linear masking op, read off the op applied to ones (fp64, CPU)"""
    with torch.no_grad():
        return op(be, be.put(torch.ones_like(x), lay)).detach().cpu().double()


# ------------------------------------------------------------------------------------------------------------------ 'twice': elementwise, rows, layout
def _shaped(cls, name, keys, build, order='twice', chain=True):
    """one entry per shape key: build(g, shape, lay) -> Case"""
    for k in keys:
        shape, lay = SHAPES[k]
        entry(cls, order, '%s[%s]' % (name, k), chain)(lambda seed, shape=shape, lay=lay, k=k: build(gen(cls, name, k, seed), shape, lay))


def _unary(cls, name, keys, run, ref, kinked=False, order='twice', tol=None):
    def build(g, shape, lay):
        x = rnd(g, *shape)
        return Case([away(x) if kinked else x], run, ref, lay=[lay], pre=ident if kinked else None, tol=tol)
    _shaped(cls, name, keys, build, order)


_unary('LReluFn', 'leaky_relu', ALL, lambda be, x: be.F.leaky_relu(x, 0.2), lambda x: lrelu_ref(x, 0.2), kinked=True)
_unary('LReluFn', 'relu', ('cl6',), lambda be, x: be.F.relu(x), torch.relu, kinked=True)
_unary('Pool2Fn', 'mean_pool2', FOUR, lambda be, x: be.F.mean_pool2(x), tf_ops.mean_pool2)
_unary('Upsample2Fn', 'upsample2', FOUR, lambda be, x: be.F.upsample2(x), tf_ops.upsample2)
_unary('SpatialMeanFn', 'spatial_mean', FOUR, lambda be, x: be.F.spatial_mean(x), lambda x: x.mean(dim=(2, 3)))
_unary('_SpatialSumScaled', 'apply', CL, lambda be, x: be.F._SpatialSumScaled.apply(x, 0.37), lambda x: 0.37 * x.sum(dim=(2, 3)))
_unary('Copy4dFn', 'to_nchw', CL, lambda be, x: be.F.to_nchw(x), lambda x: x)
_unary('Copy4dFn', 'to_channels_last', ('nchw',), lambda be, x: be.F.to_channels_last(x), lambda x: x)
_unary('ScaleFn', 'apply', ALL, lambda be, x: be.F.ScaleFn.apply(x, 0.37), lambda x: 0.37 * x)
_unary('SampleSumFn', 'apply', ('cl6', 'cl8', '2d'), lambda be, x: be.F.SampleSumFn.apply(x, 0.37),
       lambda x: 0.37 * x.reshape(x.shape[0], -1).sum(dim=1))
_unary('ChannelSumFn', 'apply', FOUR, lambda be, x: be.F.ChannelSumFn.apply(x), lambda x: x.sum(dim=(0, 2, 3)))
_unary('RowsSelectFn', 'rows_select', ALL, lambda be, x: be.F.rows_select(x, ((0, 1), (1, x.shape[0]), (0, 1))),
       lambda x: torch.cat([x[0:1], x[1:], x[0:1]], 0))


def _binary(cls, name, keys, run, ref):
    _shaped(cls, name, keys, lambda g, shape, lay: Case([rnd(g, *shape), rnd(g, *shape)], run, ref, lay=[lay, lay]))


_binary('AddFn', 'add', ALL, lambda be, x, y: be.F.add(x, y), lambda x, y: x + y)
_binary('AddFn', 'axpby', ('cl6', '2d'), lambda be, x, y: be.F.AddFn.apply(x, y, 0.5, -2.0), lambda x, y: 0.5 * x - 2.0 * y)
_binary('MulFn', 'apply', ALL, lambda be, x, y: be.F.MulFn.apply(x, y), lambda x, y: x * y)


@entry('_ChannelSum2dFn', 'twice', 'apply[2d]')
def _(seed):
    return Case([rnd(gen('cs2', seed), 5, 7)], lambda be, x: be.F._ChannelSum2dFn.apply(x), lambda x: x.sum(dim=0))


def _rsqrt(g, shape, lay):
    return Case([torch.rand(*shape, generator=g) + 0.5], lambda be, v: be.F.RsqrtFn.apply(v, 1e-5), lambda v: 1.0 / torch.sqrt(v + 1e-5), lay=[lay])


_shaped('RsqrtFn', 'apply', ('cl6', '2d'), _rsqrt)
entry('RsqrtFn', 'twice', 'apply[n]')(lambda seed: Case([torch.rand(5, generator=gen('rs', seed)) + 0.5], lambda be, v: be.F.RsqrtFn.apply(v, 1e-5),
                                                        lambda v: 1.0 / torch.sqrt(v + 1e-5)))


def _lrelu_bwd(g, shape, lay):
    ref = away(rnd(g, *shape))
    return Case([rnd(g, *shape)], lambda be, gy: be.F.LReluBwdFn.apply(gy, be.put(ref, lay), 0.2, 0.37),
                lambda gy: gy * torch.where(ref.double() > 0, 1.0, 0.2) * 0.37, lay=[lay])


_shaped('LReluBwdFn', 'apply', ALL, _lrelu_bwd)


def _masked(cls, name, keys, op, slope=None, order='twice', rows=None):
    """dropout family: op(be, x) is linear with a diagonal matrix (after the optional LeakyReLU); rows: the concat of RowsCatDropFn"""
    def build(g, shape, lay):
        x = rnd(g, *shape)
        x = away(x) if slope is not None else x
        box = {}

        def ref(xr):
            a = lrelu_ref(xr, slope) if slope is not None else xr
            a = torch.cat([a, a[:rows]], 0) if rows else a
            return a * box['d']
        return Case([x], op, ref, lay=[lay], pre=ident if slope is not None else None, setup=lambda be: box.update(d=diag_of(op, be, x, lay)))
    _shaped(cls, name, keys, build, order)


def _u_for(x):
    return torch.rand(x.shape, generator=gen('u', tuple(x.shape)))


_masked('DropoutFn', 'dropout_u', ('cl6', 'cl8', '2d'), lambda be, x: be.F.dropout(x, 0.8, u=be.like(_u_for(x), x)))
_masked('DropoutRngFn', 'dropout', ALL, lambda be, x: be.F.dropout(x, 0.8, rng=be.rng()))
_masked('LReluDropFn', 'lrelu_dropout', ALL, lambda be, x: be.F.lrelu_dropout(x, 0.2, 0.8, be.rng()), slope=0.2)


def _rows_cat(n):
    """RowsCatDropFn leaves the mask of its backward to its consumer (a conv with in_drop): the entry is the pair"""
    def make(seed):
        g = gen('rcd', n, seed)
        x, w = rnd(g, n, 8, 4, 4), rnd(g, 3, 3, 8, 8) * 0.2
        box = {}

        def cat(be, xb):
            return be.F.rows_cat_dropout(xb, 1, be.F.drop_spec(be.rng(), 0.8))

        def run(be, xb):
            spec = be.F.drop_spec(be.rng(), 0.8)
            return be.F.conv2d(be.F.rows_cat_dropout(xb, 1, spec), be.dev(w), epi={'in_drop': spec})
        return Case([x], run, lambda xr: conv_ref(torch.cat([xr, xr[:1]], 0) * box['d'], w.double(), None, 1),
                    setup=lambda be: box.update(d=diag_of(cat, be, x, 'cl')))
    return make


entry('RowsCatDropFn', 'once', 'rows_cat_dropout+conv2d[n2]')(_rows_cat(2))
entry('RowsCatDropFn', 'once', 'rows_cat_dropout+conv2d[n3]')(_rows_cat(3))


def _lrelu_drop_bwd(g, shape, lay):
    ref, gy = away(rnd(g, *shape)), rnd(g, *shape)
    op = lambda be, t: be.F.LReluDropBwdFn.apply(t, be.put(ref, lay), 0.2, 0.8, 7, 5, be.ctr())        # noqa: E731
    box = {}
    return Case([gy], op, lambda t: t * box['d'], lay=[lay], setup=lambda be: box.update(d=diag_of(op, be, gy, lay)))


_shaped('LReluDropBwdFn', 'apply', ('cl6', 'cl8', '2d'), _lrelu_drop_bwd)


def _spatial_bcast(seed, n, c):
    return Case([rnd(gen('sb', n, c, seed), n, c)], lambda be, v: be.F.SpatialBcastFn.apply(v, 4, 4, 0.37),
                lambda v: 0.37 * v[:, :, None, None].expand(-1, -1, 4, 4))


entry('SpatialBcastFn', 'twice', 'apply[3x6]')(lambda seed: _spatial_bcast(seed, 3, 6))
entry('SpatialBcastFn', 'twice', 'apply[2x8]')(lambda seed: _spatial_bcast(seed, 2, 8))


def _sample_bcast(g, shape, lay):
    like = torch.zeros(shape)
    return Case([rnd(g, shape[0])], lambda be, v: be.F.SampleBcastFn.apply(v, be.put(like, lay), 0.37),
                lambda v: 0.37 * v.reshape([-1] + [1] * (len(shape) - 1)).expand(shape))


_shaped('SampleBcastFn', 'apply', ('cl6', 'cl8', '2d'), _sample_bcast)


def _channel_affine(g, shape, lay):
    c = shape[1]
    tail = [1] * (len(shape) - 2)
    return Case([rnd(g, *shape), torch.rand(c, generator=g) + 0.5, rnd(g, c)], lambda be, x, s, o: be.F.ChannelAffineFn.apply(x, s, o),
                lambda x, s, o: x * s.reshape([1, -1] + tail) + o.reshape([1, -1] + tail), lay=[lay, None, None])


_shaped('ChannelAffineFn', 'apply', ('cl6', 'cl8', '2d'), _channel_affine)


# ------------------------------------------------------------------------------------------------------------------ 'twice': Layernorm and its parts
EPS = 1e-5


@contextlib.contextmanager
def ln_fused(F, on):
    old, F.LN_FUSED = F.LN_FUSED, on
    try:
        yield
    finally:
        F.LN_FUSED = old


def _ln(cls, name, shape, fused, relu, cond=False):
    """F.layer_norm at `shape`: the fused Function where kernels.layernorm_supported accepts the shape, the composition where it refuses
    (or with LN_FUSED off)."""
    def make(seed):
        g = gen('ln', name, seed)
        c, n_labels = shape[1], 3
        x = rnd(g, *shape)
        tab = (n_labels, c) if cond else (c,)
        s, o = torch.rand(*tab, generator=g) + 0.5, rnd(g, *tab)
        labels = torch.randint(0, n_labels, (shape[0],), generator=g, dtype=torch.int32) if cond else None

        def run(be, xb, sb, ob):
            assert be.K.layernorm_supported(xb) == (fused is not None), (shape, fused)
            with ln_fused(be.F, bool(fused)):
                return be.F.layer_norm(xb, sb, ob, EPS, relu, labels=be.dev(labels) if cond else None)
        return Case([x, s, o], run, lambda xr, sr, orr: ln_ref(xr, sr, orr, EPS, relu, labels),
                    pre=(lambda xr, sr, orr: ln_ref(xr, sr, orr, EPS, False, labels)) if relu else None, contract=[0] if fused else None)
    entry(cls, 'twice', name)(make)


_ln('LayerNormFn', 'layer_norm[cl8]', (2, 8, 4, 4), True, False)
_ln('LayerNormFn', 'layer_norm[2x4]', (2, 4), True, False)                      # the smallest shape the fused kernels accept
_ln('LayerNormFn', 'layer_norm[2d,relu]', (5, 8), True, True)
_ln('LayerNormBwdFn', 'layer_norm[cl8,relu]', (2, 8, 4, 4), True, True)
_ln('LayerNormBwdFn', 'layer_norm[2d]', (5, 8), True, False)
_ln('SampleSumFn', 'layer_norm[composed,cl6]', (3, 6, 4, 4), None, False)            # the shape the fused kernels refuse
_ln('RsqrtFn', 'layer_norm[composed,2d,relu]', (5, 7), None, True)
_ln('ChannelAffineFn', 'layer_norm[LN_FUSED=0,cl8]', (2, 8, 4, 4), False, False)
_ln('CondLayerNormFn', 'layer_norm[labels,cl8]', (2, 8, 4, 4), True, False, cond=True)
_ln('CondLayerNormFn', 'layer_norm[labels,2d,relu]', (5, 8), True, True, cond=True)
_ln('CondLayerNormBwdFn', 'layer_norm[labels,cl8,relu]', (2, 8, 4, 4), True, True, cond=True)
_ln('RowsGatherFn', 'layer_norm[labels,composed,cl6]', (3, 6, 4, 4), None, False, cond=True)
_ln('RowsSumByLabelFn', 'layer_norm[labels,LN_FUSED=0,cl8,relu]', (2, 8, 4, 4), False, True, cond=True)
_LABELS = torch.tensor([2, 0, 2, 1, 0], dtype=torch.int32)


@entry('RowsGatherFn', 'twice', 'rows_gather')
def _(seed):
    return Case([rnd(gen('rg', seed), 3, 7)], lambda be, t: be.F.rows_gather(t, be.dev(_LABELS)), lambda t: t[_LABELS.long()])


@entry('RowsSumByLabelFn', 'twice', 'apply')
def _(seed):
    return Case([rnd(gen('rsl', seed), 5, 7)], lambda be, r: be.F.RowsSumByLabelFn.apply(r, be.dev(_LABELS), 4),
                lambda r: torch.zeros(4, 7, dtype=r.dtype).index_add(0, _LABELS.long(), r))


# ------------------------------------------------------------------------------------------------------------------ 'twice': the conv family
def geom(C, H, W, Kout, R, S, stride):
    from ctgan_amd.kernels import ConvGeom
    return ConvGeom(C, H, W, Kout, R, S, stride, False)


def _conv(stride, relu_in=False, bias=True):
    def make(seed):
        g = gen('conv', stride, relu_in, seed)
        xs = [rnd(g, 2, 8, 6, 6), rnd(g, 3, 3, 8, 8) * 0.2] + ([rnd(g, 8)] if bias else [])
        act = torch.relu if relu_in else (lambda t: t)
        return Case(xs, lambda be, x, w, b=None: be.F.conv2d(x, w, b, stride=stride, relu_in=relu_in),
                    lambda x, w, b=None: conv_ref(act(x), w, b, stride), lay=['cl', 'dense', None][:len(xs)], pre=(lambda x, *r: x) if relu_in else None)
    return make


entry('ConvFn', 'twice', 'conv2d[s1]')(_conv(1))
entry('ConvFn', 'twice', 'conv2d[s2]')(_conv(2))
entry('ConvFn', 'twice', 'conv2d[s1,relu_in]')(_conv(1, relu_in=True, bias=False))
entry('ConvWgradBiasFn', 'twice', 'conv2d[s2]')(_conv(2))                 # reached by the first backward under create_graph
entry('ConvWgradFn', 'twice', 'conv2d[s1,no bias]')(_conv(1, bias=False))


def _conv_transpose(stride):
    def make(seed):
        g = gen('deconv', stride, seed)
        xs = [rnd(g, 2, 8, 3, 3), rnd(g, 3, 3, 8, 8) * 0.2, rnd(g, 8)]          # w [k, k, out, in]
        return Case(xs, lambda be, x, w, b: be.F.conv2d_transpose(x, w, b, stride=stride),
                    lambda x, w, b: dgrad_ref(x, w, (2, 8, 3 * stride, 3 * stride), stride) + b.view(1, -1, 1, 1), lay=['cl', 'dense', None])
    return make


entry('ConvDgradFn', 'twice', 'conv2d_transpose[s2]')(_conv_transpose(2))
entry('ConvDgradFn', 'twice', 'conv2d_transpose[s1]')(_conv_transpose(1))


def _wgrad(stride, bias):
    def make(seed):
        g = gen('wgrad', stride, bias, seed)
        P = -(-6 // stride)
        xs = [rnd(g, 2, 8, 6, 6), rnd(g, 2, 8, P, P)]

        def run(be, x, gy):
            cg = geom(8, 6, 6, 8, 3, 3, stride)
            return be.F.ConvWgradBiasFn.apply(x, gy, cg, False) if bias else be.F.ConvWgradFn.apply(x, gy, cg, False)

        def ref(x, gy):
            dw = wgrad_ref(x, gy, (3, 3, 8, 8), stride)
            return (dw, gy.sum(dim=(0, 2, 3))) if bias else dw
        return Case(xs, run, ref)
    return make


entry('ConvWgradFn', 'twice', 'apply[s1]')(_wgrad(1, False))
entry('ConvWgradFn', 'twice', 'apply[s2]')(_wgrad(2, False))
entry('ConvWgradBiasFn', 'twice', 'apply[s1]')(_wgrad(1, True))
CPAD = 32


def _im2col(stride):
    return lambda seed: Case([rnd(gen('i2c', stride, seed), 2, 3, 6, 6)], lambda be, x: be.F.Im2colFn.apply(x, geom(3, 6, 6, 8, 3, 3, stride), CPAD),
                             lambda x: im2col_ref(x, 3, 3, stride, CPAD))


def _col2im(stride):
    P = -(-6 // stride)
    return lambda seed: Case([rnd(gen('c2i', stride, seed), 2, CPAD, P, P)],
                             lambda be, c: be.F.Col2imFn.apply(c, geom(3, 6, 6, 8, 3, 3, stride), 2, None),
                             lambda c: adjoint_of(lambda z: im2col_ref(z, 3, 3, stride, CPAD), (2, 3, 6, 6), c))


for _s in (1, 2):
    entry('Im2colFn', 'twice', 'apply[s%d]' % _s)(_im2col(_s))
    entry('Col2imFn', 'twice', 'apply[s%d]' % _s)(_col2im(_s))


@entry('Im2colFn', 'twice', 'conv2d[3->8]')
def _(seed):
    g = gen('fewconv', seed)
    return Case([rnd(g, 2, 3, 6, 6), rnd(g, 3, 3, 3, 8) * 0.3, rnd(g, 8)], lambda be, x, w, b: be.F.conv2d(x, w, b), lambda x, w, b: conv_ref(x, w, b, 1),
                lay=['cl', 'dense', None])


def _spread(flip):
    return lambda seed: Case([rnd(gen('spread', flip, seed), 3, 3, 6, 8)], lambda be, w: be.F.FilterSpreadFn.apply(w, 0.25, flip),
                             lambda w: spread_ref(w, 0.25, flip), lay=['dense'])


def _fold(flip):
    shape = (4, 4, 8, 6) if flip else (4, 4, 6, 8)
    return lambda seed: Case([rnd(gen('fold', flip, seed), *shape)], lambda be, w4: be.F.FilterFoldFn.apply(w4, 0.25, flip),
                             lambda w4: adjoint_of(lambda z: spread_ref(z, 0.25, flip), (3, 3, 6, 8), w4), lay=['dense'])


for _f in (False, True):
    entry('FilterSpreadFn', 'twice', 'apply[flip=%d]' % _f)(_spread(_f))
    entry('FilterFoldFn', 'twice', 'apply[flip=%d]' % _f)(_fold(_f))


def _gemm_filter(kind):
    """The input is a registry parameter (the buffer is cached per parameter), so this entry has no MulFn chain: its backward is a reshape,
    a slice and a transpose of torch's own."""
    def make(seed):
        w = rnd(gen('gemm', kind, seed), 3, 3, 3, 8)

        def run(be, p):
            return be.F.GemmFilterFn.apply(p, kind, CPAD)

        def ref(wr):
            w2 = wr.reshape(27, 8)
            return torch.cat([w2, w2.new_zeros(CPAD - 27, 8)], 0) if kind == 'cols' else torch.cat([w2.t(), w2.new_zeros(8, CPAD - 27)], 1)
        return Case([w], run, ref, lay=['dense'], param=True)
    return make


entry('GemmFilterFn', 'twice', 'apply[cols]', chain=False)(_gemm_filter('cols'))
entry('GemmFilterFn', 'twice', 'apply[taps]', chain=False)(_gemm_filter('taps'))
DA_SHAPE, DA_N, DA_SPEC = (3, 4, 6), 3, (9, (2 << 16) | 0xFF02, 4)


def _diffaug(adjoint):
    def make(seed):
        from tests import diffaug_oracle as O
        c, h, w = DA_SHAPE
        p = O.params(DA_SPEC[0], DA_SPEC[1], DA_SPEC[2], DA_N, h, w, 7)
        spec = lambda be: (DA_SPEC[0], DA_SPEC[1], be.ctr(DA_SPEC[2]))          # noqa: E731
        x = rnd(gen('da', adjoint, seed), DA_N, c * h * w)
        if adjoint:
            return Case([x], lambda be, g: be.F.DiffAugAdjFn.apply(g, DA_SHAPE, 7, spec(be)), lambda g: O.adjoint(g, DA_SHAPE, p).reshape(g.shape))
        return Case([x], lambda be, t: be.F.diffaug(t, DA_SHAPE, 7, spec(be)), lambda t: O.forward(t, DA_SHAPE, p).reshape(t.shape))
    return make


entry('DiffAugFn', 'twice', 'diffaug')(_diffaug(False))
entry('DiffAugAdjFn', 'twice', 'apply')(_diffaug(True))


# ------------------------------------------------------------------------------------------------------------------ 'once': activations, batch norms
_unary('TanhFn', 'tanh', ALL, lambda be, x: be.F.tanh(x), torch.tanh, order='once')
_unary('SigmoidFn', 'sigmoid', ALL, lambda be, x: be.F.sigmoid(x), torch.sigmoid, order='once')
_unary('EluFn', 'elu', ALL, lambda be, x: be.F.elu(x), elu_ref, kinked=True, order='once')
_unary('CropFn', 'crop', FOUR, lambda be, x: be.F.crop(x, 2, 3, 1, 0), lambda x: x[:, :, 1:3, 0:3], order='once')
_unary('ChannelSplitFn', 'apply', FOUR, lambda be, x: be.F.ChannelSplitFn.apply(x), lambda x: (x[:, ::2], x[:, 1::2]), order='once')
_unary('GateFn', 'gate', ('cl6', 'cl8'), lambda be, x: be.F.gate(x), gate_ref, order='once')
_unary('ChannelSplitFn', 'gate_composed', ('cl6', 'cl8'), lambda be, x: be.F.gate_composed(x), gate_ref, order='once')
BN = {'y': BN_TOL, 'first': BN_TOL}


def _bn_inputs(g, shape):
    c = shape[1]
    return [rnd(g, *shape) * 2 + 3.0, torch.rand(c, generator=g) + 0.5, rnd(g, c)]


def _batch_norm(g, shape, lay, groups=1, relu=False):
    pre = (lambda x, s, o: bn_ref(x, s, o, groups, EPS)) if relu else None
    return Case(_bn_inputs(g, shape), lambda be, x, s, o: be.F.batch_norm(x, s.reshape(1, -1), o.reshape(1, -1), None, groups, relu, EPS),
                lambda x, s, o: (torch.relu if relu else (lambda t: t))(bn_ref(x, s, o, groups, EPS)), lay=[lay, None, None], pre=pre, tol=BN)


_shaped('BatchNormFn', 'batch_norm', ('cl6', 'cl8', '2d'), _batch_norm, order='once')
_shaped('BatchNormFn', 'batch_norm[relu]', ('cl8',), lambda g, s, l: _batch_norm(g, s, l, 2, True), order='once')


def _bn_act(act, fused):
    def build(g, shape, lay):
        fn = {'lrelu': lambda z: lrelu_ref(z, 0.2), 'tanh': torch.tanh, 'gate': gate_ref}[act]

        def run(be, x, s, o):
            old, be.F.BN_ACT_FUSED = be.F.BN_ACT_FUSED, fused
            try:
                return be.F.batch_norm_act(x, s, o, act, 0.2, 1, EPS)
            finally:
                be.F.BN_ACT_FUSED = old
        return Case(_bn_inputs(g, shape), run, lambda x, s, o: fn(bn_ref(x, s, o, 1, EPS)), lay=[lay, None, None],
                    pre=(lambda x, s, o: bn_ref(x, s, o, 1, EPS)) if act == 'lrelu' else None, tol=BN)
    return build


for _a in ('lrelu', 'tanh', 'gate'):
    _shaped('BatchNormActFn', 'batch_norm_act[%s]' % _a, ('cl6', 'cl8'), _bn_act(_a, True), order='once')
# CTGAN_BN_ACT_FUSED=0, the composed layer the fused one's error message used to recommend: first order only as well
_shaped('BatchNormFn', 'batch_norm_act[composed,lrelu]', ('cl6',), _bn_act('lrelu', False), order='once')
_shaped('TanhFn', 'batch_norm_act[composed,tanh]', ('cl6',), _bn_act('tanh', False), order='once')
_shaped('SigmoidFn', 'batch_norm_act[composed,gate]', ('cl8',), _bn_act('gate', False), order='once')


def _score_bn(g, shape, lay):
    xs = _bn_inputs(g, shape) + [rnd(g, *shape)]

    def ref(x, s, o, sc):
        y = sc + 0.7 * bn_ref(x, s, o, 1, EPS)
        return y, elu_ref(y)
    return Case(xs, lambda be, x, s, o, sc: be.F.batch_norm_moving(x, s, o, None, sc, 0.7, False, True, EPS), ref, lay=[lay, None, None, lay],
                pre=lambda *a: ref(*a)[0], tol=BN)


_shaped('ScoreBNFn', 'batch_norm_moving[shortcut,elu]', ('cl6', 'cl8'), _score_bn, order='once')
_shaped('ScoreBNFn', 'batch_norm_moving[relu]', ('cl6', '2d'), lambda g, shape, lay: Case(
    _bn_inputs(g, shape), lambda be, x, s, o: be.F.batch_norm_moving(x, s, o, relu=True, eps=EPS),
    lambda x, s, o: torch.relu(bn_ref(x, s, o, 1, EPS)), lay=[lay, None, None], pre=lambda x, s, o: bn_ref(x, s, o, 1, EPS), tol=BN), order='once')


@entry('BatchNorm2dFn', 'once', 'batch_norm_2d[softplus]')
def _(seed):
    g = gen('bn2d', seed)
    return Case([rnd(g, 5, 7) * 2 + 1, rnd(g, 7)], lambda be, x, o: be.F.batch_norm_2d(x, o, 1e-6, True),
                lambda x, o: TF.softplus((x - x.mean(0)) / torch.sqrt(1e-6 + ((x - x.mean(0)) ** 2).mean(0)) + o), tol=BN)


@entry('BatchNorm2dFn', 'once', 'batch_norm_2d')
def _(seed):
    g = gen('bn2d', 0, seed)
    return Case([rnd(g, 5, 7) * 2 + 1, rnd(g, 7)], lambda be, x, o: be.F.batch_norm_2d(x, o, 1e-6, False),
                lambda x, o: (x - x.mean(0)) / torch.sqrt(1e-6 + ((x - x.mean(0)) ** 2).mean(0)) + o, tol=BN)


# ------------------------------------------------------------------------------------------------------------------ 'once': weight norm, dense noise
@entry('WeightNormFn', 'once', 'weight_norm')
def _(seed):
    g = gen('wn', seed)
    return Case([rnd(g, 7, 5), torch.rand(5, generator=g) + 0.5], lambda be, t, s: be.F.weight_norm(t, s, 1e-6),
                lambda t, s: t * (s / torch.sqrt(1e-6 + (t * t).sum(dim=0)))[None, :])


@entry('WeightNormFn', 'once', 'weight_norm_filter')
def _(seed):
    g = gen('wnf', seed)
    return Case([rnd(g, 3, 3, 2, 5), torch.rand(5, generator=g) + 0.5], lambda be, t, s: be.F.weight_norm_filter(t, s),
                lambda t, s: t * (s / torch.sqrt(1e-6 + (t * t).sum(dim=(0, 1, 2))))[None, None, None, :], lay=['dense', None])


@entry('WeightNormMidFn', 'once', 'weight_norm_mid')
def _(seed):
    g = gen('wnm', seed)
    return Case([rnd(g, 3, 3, 5, 2), torch.rand(5, generator=g) + 0.5], lambda be, t, s: be.F.weight_norm_mid(t, s),
                lambda t, s: t * (s / torch.sqrt(1e-6 + (t * t).sum(dim=(0, 1, 3))))[None, None, :, None], lay=['dense', None])


def _dense_noise(relu, bias):
    def make(seed):
        g = gen('dn', relu, bias, seed)
        xs = [rnd(g, 5, 7)] + ([rnd(g, 7)] if bias else [])
        box = {}

        def run(be, y, b=None):
            return be.F.dense_noise(y, b, relu, 0.3, (7, 5, be.ctr()), 0, True)

        def setup(be):                                                      # the noise is additive, a constant of every derivative
            with torch.no_grad():
                h, a = run(be, *[be.put(t) for t in xs])
            box['noise'] = (h - a).cpu().double()

        def ref(y, b=None):
            a = y if b is None else y + b[None, :]
            a = torch.relu(a) if relu else a
            return a + box['noise'], a
        return Case(xs, run, ref, pre=(lambda y, b=None: y if b is None else y + b[None, :]) if relu else None, setup=setup)
    return make


entry('DenseNoiseFn', 'once', 'dense_noise[relu,bias]')(_dense_noise(True, True))
entry('DenseNoiseFn', 'once', 'dense_noise[bias]')(_dense_noise(False, True))


# ------------------------------------------------------------------------------------------------------------------ 'once': loss heads
LAM2 = 2.0


def _mid(v):
    """a threshold between the two middle values of v, at least 2 KINK from every one of them"""
    s = v.detach().double().sort().values
    k = s.numel() // 2
    return float((s[k - 1] + s[k]) / 2) if s.numel() > 1 else float(s[0]) - 1.0


@entry('GradPenaltyFn', 'once', 'gradient_penalty')
def _(seed):
    return Case([rnd(gen('gp', seed), 5, 7) * 0.5], lambda be, g: be.F.gradient_penalty(g, 10.0)[0],
                lambda g: 10.0 * ((torch.sqrt((g * g).sum(dim=1)) - 1) ** 2).mean())


@entry('ConsistencyFn', 'once', 'consistency_term')
def _(seed):
    g = gen('ct', seed)
    xs = [rnd(g, 5), rnd(g, 5), rnd(g, 5, 7), rnd(g, 5, 7)]
    M = _mid(ct_rows(*[t.double() for t in xs], LAM2))
    return Case(xs, lambda be, *a: be.F.consistency_term(*a, LAM2, M), lambda *a: hinge(ct_rows(*a, LAM2) - M).mean(),
                pre=lambda *a: ct_rows(*a, LAM2) - M)


_CE_LABELS = torch.tensor([1, 0, 3, 3, 2], dtype=torch.int32)


@entry('SoftmaxCEFn', 'once', 'softmax_cross_entropy')
def _(seed):
    return Case([rnd(gen('ce', seed), 5, 4) * 2], lambda be, x: be.F.softmax_cross_entropy(x, be.dev(_CE_LABELS))[0], lambda x: ce_ref(x, _CE_LABELS))


@entry('MeanDiffFn', 'once', 'mean_diff')
def _(seed):
    return Case([rnd(gen('md', seed), 7)], lambda be, x: be.F.mean_diff(x, 3, 4, 1.0, -1.0), lambda x: x[:3].mean() - x[3:].mean())


def _critic_heads(with_a):
    def make(seed):
        g = gen('ch', with_a, seed)
        B, nf, ncls = 3, 6, 4
        xs = [rnd(g, 3 * B), rnd(g, 3 * B, nf)] + ([rnd(g, 3 * B, ncls) * 2] if with_a else []) + [torch.tensor(0.37)]
        lab = torch.randint(0, ncls, (B,), generator=g, dtype=torch.int32)
        rows = lambda d, f: ct_rows(d[:B], d[2 * B:], f[:B], f[2 * B:], LAM2)        # noqa: E731
        M = _mid(rows(xs[0].double(), xs[1].double()))
        scale = 0.7 if with_a else 0.0

        def run(be, d, f, *r):
            return be.F.critic_heads(d, f, r[0] if with_a else None, be.dev(lab) if with_a else None, B, LAM2, M, scale, gp=r[-1])[:4 if with_a else 3]

        def ref(d, f, *r):
            return critic_heads_ref(d, f, r[0] if with_a else None, lab, B, LAM2, M, scale, r[-1])[:4 if with_a else 3]
        return Case(xs, run, ref, pre=lambda d, f, *r: rows(d, f) - M)
    return make


entry('CriticHeadsFn', 'once', 'critic_heads[class head]')(_critic_heads(True))
entry('CriticHeadsFn', 'once', 'critic_heads')(_critic_heads(False))
KEEP = 0.5


def _tail_inputs(g, rows, nf, H, W):
    """z away from the ReLU's kink and the dropout mask (with its 1 / keep): y = relu(z) * mask is what the last conv's epilogue writes"""
    z = away(rnd(g, rows, nf, H, W), 0.01)
    mask = (torch.rand(rows, nf, H, W, generator=g) < KEEP).float() / KEEP
    return z, mask


def _heads(y, w_out, b_out, w_ac=None, b_ac=None, emb_rows=None):
    f = y.mean(dim=(2, 3))
    d = (f * (w_out.reshape(1, -1) + emb_rows)).sum(dim=1) + b_out if emb_rows is not None else f @ w_out.reshape(-1) + b_out
    return f, d, (f @ w_ac + b_ac if w_ac is not None else None)


def _critic_tail(kind):
    """kind 'class': both Linear heads; 'plain': the critic head alone; 'proj': the projection head (CriticTailHeadsProjFn)"""
    def make(seed):
        g = gen('tail', kind, seed)
        B, nf, H, W, ncls = 2, 8, 2, 2, 3
        z, mask = _tail_inputs(g, 3 * B, nf, H, W)
        lab = torch.randint(0, ncls, (B,), generator=g, dtype=torch.int32)
        b_out = rnd(g, 1)           # a constant here: d cost / d b_out is a sum that is analytically zero, there is nothing to compare it with
        params = [rnd(g, nf, 1) * 0.7] + {'class': [rnd(g, nf, ncls) * 0.7, rnd(g, ncls)], 'plain': [], 'proj': [rnd(g, ncls, nf) * 0.7]}[kind]
        scale = 0.7 if kind == 'class' else 0.0

        def outs(zr, w_out, *r):
            y = torch.relu(zr) * mask.to(zr.dtype)
            emb_rows = r[0][lab.long().repeat(3)] if kind == 'proj' else None
            f, d, a = _heads(y, w_out, b_out.to(zr.dtype), *(r[:2] if kind == 'class' else ()), emb_rows=emb_rows)
            return critic_heads_ref(d, f, a, lab, B, LAM2, M, scale, r[-1]), f, d
        M = 0.0
        with torch.no_grad():
            _, f0, d0 = outs(z.double(), *[p.double() for p in params], torch.tensor(0.37).double())
            M = _mid(ct_rows(d0[:B], d0[2 * B:], f0[:B], f0[2 * B:], LAM2))

        def run(be, y, w_out, *r):
            labd, bo = be.dev(lab), be.dev(b_out)
            if kind == 'proj':
                return be.F.critic_tail_heads(y, w_out, bo, None, None, labd, B, LAM2, M, 0.0, 1.0 / KEEP, gp=r[-1], emb=r[0])[:3]
            w_ac, b_ac = (r[0], r[1]) if kind == 'class' else (None, None)
            return be.F.critic_tail_heads(y, w_out, bo, w_ac, b_ac, labd, B, LAM2, M, scale, 1.0 / KEEP, gp=r[-1])[:4 if kind == 'class' else 3]

        def pre(zr, *r):
            _, f, d = outs(zr, *r)
            return ct_rows(d[:B], d[2 * B:], f[:B], f[2 * B:], LAM2) - M
        return Case([z] + params + [torch.tensor(0.37)], run, lambda *a: outs(*a)[0][:4 if kind == 'class' else 3], pre=pre,
                    feed=[lambda t: torch.relu(t) * mask] + [None] * (len(params) + 1))
    return make


entry('CriticTailHeadsFn', 'once', 'critic_tail_heads[class head]')(_critic_tail('class'))
entry('CriticTailHeadsFn', 'once', 'critic_tail_heads')(_critic_tail('plain'))
entry('CriticTailHeadsProjFn', 'once', 'critic_tail_heads[emb]')(_critic_tail('proj'))


def _gen_tail(kind):
    def make(seed):
        g = gen('gen', kind, seed)
        n, nf, H, W, ncls = 5, 8, 2, 2, 3
        z, mask = _tail_inputs(g, n, nf, H, W)
        lab = torch.randint(0, ncls, (n,), generator=g, dtype=torch.int32)
        w_out, b_out, w_ac, b_ac, emb = rnd(g, nf, 1) * 0.7, rnd(g, 1), rnd(g, nf, ncls) * 0.7, rnd(g, ncls), rnd(g, ncls, nf) * 0.7

        def run(be, y):
            if kind == 'proj':
                return be.F.gen_tail_heads(y, be.dev(w_out), be.dev(b_out), None, None, be.dev(lab), 0.0, 1.0 / KEEP, emb=be.dev(emb))[0]
            cls_head = (be.dev(w_ac), be.dev(b_ac)) if kind == 'class' else (None, None)
            return be.F.gen_tail_heads(y, be.dev(w_out), be.dev(b_out), *cls_head, be.dev(lab), 0.1, 1.0 / KEEP)[0]

        def ref(zr):
            y = torch.relu(zr) * mask.double()
            f, d, a = _heads(y, w_out.double(), b_out.double(), *((w_ac.double(), b_ac.double()) if kind == 'class' else ()),
                             emb_rows=emb.double()[lab.long()] if kind == 'proj' else None)
            return -d.mean() + (0.1 * ce_ref(a, lab) if a is not None else 0.0)
        return Case([z], run, ref, feed=[lambda t: torch.relu(t) * mask])
    return make


entry('GenTailHeadsFn', 'once', 'gen_tail_heads[class head]')(_gen_tail('class'))
entry('GenTailHeadsFn', 'once', 'gen_tail_heads')(_gen_tail('plain'))
entry('GenTailHeadsProjFn', 'once', 'gen_tail_heads[emb]')(_gen_tail('proj'))


def _gp_head(proj):
    """The seed of the penalty's first backward, dD/dz; its own backward - the adjoint w.r.t. the head's weights - is what the penalty's
    second differentiation runs, and is where this class's order ends."""
    def make(seed):
        g = gen('gph', proj, seed)
        n, nf, H, W, ncls = 5, 8, 2, 2, 3
        z, mask = _tail_inputs(g, n, nf, H, W)
        y = torch.relu(z) * mask
        lab = torch.randint(0, ncls, (n,), generator=g, dtype=torch.int32)
        xs = [rnd(g, nf, 1)] + ([rnd(g, ncls, nf)] if proj else [])

        def run(be, w_out, emb=None):
            return be.F.gp_head_grad(be.cl(y), w_out, 1.0 / KEEP, emb, be.dev(lab) if proj else None)

        def ref(w_out, emb=None):
            w = w_out.reshape(1, -1) + (emb[lab.long()] if proj else 0.0)
            return (y.double() > 0).double() * w[:, :, None, None] / (H * W) / KEEP
        return Case(xs, run, ref)
    return make


entry('GpHeadGradFn', 'once', 'gp_head_grad')(_gp_head(False))
entry('GpHeadGradProjFn', 'once', 'gp_head_grad[emb]')(_gp_head(True))


def _gan_loss(loss, net):
    def make(seed):
        B = 3
        d = rnd(gen('gl', loss, net, seed), 2 * B if net == 'd' else B)

        def ref(x):
            if loss == 'bce':
                return (TF.softplus(x[B:]).mean() + TF.softplus(-x[:B]).mean()) / 2 if net == 'd' else TF.softplus(-x).mean()
            return (((x[:B] - 1) ** 2).mean() + (x[B:] ** 2).mean()) / 2 if net == 'd' else ((x - 1) ** 2).mean()
        return Case([d], lambda be, x: be.F.gan_loss(x, B, loss, net), ref)
    return make


for _l in ('bce', 'ls'):
    for _n in ('d', 'g'):
        entry('GanLossFn', 'once', 'gan_loss[%s,%s]' % (_l, _n))(_gan_loss(_l, _n))
_SSL_LABELS = torch.tensor([1, 0, 3], dtype=torch.int32)


@entry('SSLHeadFn', 'once', 'ssl_head')
def _(seed):
    from tests import ssl_oracle as O
    B = 3
    x = rnd(gen('ssl', seed), 4 * B, 4) * 2
    ct = lambda t: LAM2 * ((torch.softmax(t[B:2 * B], 1) - torch.softmax(t[2 * B:3 * B], 1)) ** 2).mean(dim=1)        # noqa: E731
    M = _mid(ct(x.double()))
    return Case([x], lambda be, t: be.F.ssl_head(t, be.dev(_SSL_LABELS), B, LAM2, M)[0][:2], lambda t: O._head_terms(t, _SSL_LABELS, B, LAM2, M)[0][:2],
                pre=lambda t: ct(t) - M)


@entry('TEHeadFn', 'once', 'te_head')
def _(seed):
    from tests import ssl_cifar_te_oracle as O
    g = gen('te', seed)
    B, nc, nf, rows = 3, 4, 6, 5
    xs = [rnd(g, 3 * B, nc) * 2, rnd(g, 3 * B, nf)]
    idx = torch.tensor([4, 0, 2], dtype=torch.int32)
    tg, tg2 = rnd(g, rows, nc), torch.rand(rows, nf, generator=g) * 0.5
    terms = lambda lo, fe, M: O.te_terms(lo, fe, _SSL_LABELS, tg.to(lo.dtype)[idx.long()], tg2.to(lo.dtype)[idx.long()], B, LAM2, 0.5, M)        # noqa: E731
    M = _mid(terms(xs[0].double(), xs[1].double(), 0.0)['CT_i'])

    def run(be, lo, fe):
        z = lambda w: torch.zeros(rows, w, device=be.device)        # noqa: E731
        return be.F.te_head(lo, fe, be.dev(_SSL_LABELS), be.dev(idx), be.dev(tg), be.dev(tg2), z(nc), z(nf), B, LAM2, 0.5, M)[:2]

    def ref(lo, fe):
        t = terms(lo, fe, M)
        return torch.stack([t['loss_lab'], t['loss_unl']])
    return Case(xs, run, ref, pre=lambda lo, fe: terms(lo, fe, M)['CT_i'])


def _featmatch(l1):
    def make(seed):
        B = 3
        f = rnd(gen('fm', l1, seed), 2 * B, 7)
        diff = lambda t: t[:B].mean(dim=0) - t[B:].mean(dim=0)        # noqa: E731
        if l1:
            return Case([f], lambda be, t: be.F.feature_matching_l1(t, B), lambda t: diff(t).abs().mean(), pre=diff)
        return Case([f], lambda be, t: be.F.feature_matching(t, B), lambda t: (diff(t) ** 2).mean())
    return make


entry('FeatMatchFn', 'once', 'feature_matching')(_featmatch(False))
entry('FeatMatchL1Fn', 'once', 'feature_matching_l1')(_featmatch(True))


@entry('FeatConsFn', 'once', 'feature_consistency')
def _(seed):
    B = 3
    g = gen('fc', seed)
    logits = rnd(g, 4 * B, 4)
    return Case([rnd(g, 4 * B, 7)], lambda be, f: be.F.feature_consistency(f, B, be.dev(logits))[:1],
                lambda f: ((f[B:2 * B] - f[2 * B:3 * B]) ** 2).mean().reshape(1))
