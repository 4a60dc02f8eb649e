"""Case tables, input makers, fp64 references, bounds and checks of the fused Layernorm (ctgan_amd/csrc/layernorm.hip: six kernels behind ten C
entry points), shared by tests/test_gpu_layernorm_paths.py (the HIP kernels) and tests/test_layernorm_standins.py (their fp32 stand-ins in
tests/cpu_kernels.py and tests/cond_layernorm_cpu_kernels.py).  A plain helper module: no fixtures, no marks.

References (`reference`): written once in fp64 after the header comment of layernorm.hip and TF/tflib/ops/layernorm.py, LS/tflib/ops/layernorm.py:
y = (x - mean) * rsqrt(var + eps) * scale + offset with the biased variance, [then ReLU]; gx, gscale, goffset are torch.autograd.grad of y;
the bwd2 outputs are torch.autograd.grad of <gx, u> with respect to (gy, x, scale).  The closed forms of the kernel header are not restated.
Labels are clamped to the table; relu'(0) = 0 (torch's).  Nothing here calls ctgan_amd.kernels, ctgan_amd.functional or tests/cpu_kernels.py.

Bounds, U = 2^-24, none taken from the code under test.  kappa_n = U |mean_n| rstd_n (on the reference) is the shift of every xh of sample n
caused by holding mean[n] in fp32, the ABI's contract; a constant sample's mean is its value, an fp32 number, so kappa_n = 0 there (and its
mean is asserted bit-equal).  M(.) is the per-sample mean of magnitudes, X = |xh| + 1 (the + 1 carries the kappa shift where xh is near 0),
g = gy * scale [* mask], r = rstd.
  mean   U |ref| + D 2^-53 M|x|                       one cast; fp64 summation of D terms in any order
  rstd   ref (U + (3 D + 8) 2^-53 E[x^2] / (var + eps))
         one cast; E[x^2] carries (D + 1) 2^-53 relative (squares and their sum), mean^2 <= E[x^2] carries 2 (D + 1) 2^-53, the division, the
         subtraction, the addition of eps, the square root and the reciprocal six more: <= (3 D + 8) 2^-53 E[x^2] absolute on var + eps, taken
         whole as the relative error of rstd (it is half of that).  At mean -300, std 0.01, D = 8192 this is 2e-3 and not negligible.
         A constant sample whose moments are exact in fp64 (every partial sum of its squares fits 53 bits; checked on the value): U + 4 2^-53,
         and the product's rstd is asserted to be 1 / sqrt(eps) to that.  A constant sample whose moments are not: E[x^2] - mean^2 is
         rounding noise of either sign and the bound above says nothing; asserted instead is what the `var < 0` clamp guarantees,
         0 < rstd <= 1 / sqrt(eps), and for everything that carries rstd (gx, cot_gy, cot_x, cot_scale) U + kappa_n is replaced by U + rho_n,
         rho_n = that cancellation term: finiteness is what is left of the check there.  mean, y, gscale and goffset do not depend on rstd
         for a constant sample (xh is exactly 0) and keep their bounds.
  per element  |got - ref| <= (U + kappa_n) sum_i c_i T_i, T_i the terms of T and c_i the roundings on the path of the apply kernel's expression
         to that term, counted with xh = (x - mu) * r as 3 (subtraction, product, the cast of r), a product or sum as 1, the cast of a
         per-sample mean as 1, so a = mean g is 2, mean u 1, b = mean(g xh) 6, m = mean(u xh) 5, mean(u g) 3, r * r 3:
    y      = xh * s + o                          5 (X |s| + |o|): xh 3, * s, + o
    gx     = r * (g - a - xh * b)                r (5 |g| + 6 M|g| + 13 X M(|g| X)): g 1, two subtractions, * r 2;  a 2 + 4;  b 6, xh 3, product,
                                                 subtraction, * r 2
    cot_gy = r * (u - mean u - xh * m) * s       r |s| mask (5 |u| + 6 M|u| + 13 X M(|u| X)): two subtractions, * r 2, * s;  mean u 1 + 5;  m 5, xh 3,
                                                 product, subtraction, * r 2, * s
    cot_x  = r * (q - mean q) - xh * k_xh, q = -r (b u + m g), mean q = -r (b mean u + m a), k_xh = r (-2 r b m) + r r (mean(u g) - a mean u - b m):
             r^2 (14 (B |u| + Mm |g|) + 15 (B M|u| + Mm M|g|)) + X r^2 ((2 * 22 + 24) B Mm + 16 M|u g| + 16 M|g| M|u|), B = M(|g| X), Mm = M(|u| X):
             b u: b 6, product, sum, * r 2, - mean q, * r 2, last subtraction = 14 (m g: 5 + 1 + the same 8);  b mean u: 6 + 1 + product, sum, * r 2,
             subtraction, * r 2, last subtraction = 15 (m a: 5 + 2 + 8);  r (-2 r b m): b 6, m 5, two products, cast of r, * r 2, the sum = 17,
             xh 3, product, last subtraction = 22;  the b m of the second part: 6 + 5, product, two subtractions, r r 3, product, sum, xh 3, product,
             last subtraction = 24;  mean(u g) 3 and a mean u (2 + 1 + product): two subtractions, r r 3, product, sum, xh 3, product, last = 16
         The per-thread fp32 accumulation behind a mean (at most 16 visits of a float4, then fp64 across threads and chunks) is not counted at its
         worst case of 64 roundings one way: the partial sums of independent threads enter one mean.
  per parameter gradient element  |got - ref| <= d sum_n (U + kappa_n) sum |term|: gscale terms |gy| X, goffset |gy|, cot_scale |gy| r (|u| + M|u| +
         X M(|u| X)); d = the additions on the longest path: 16 visits of a thread in fp32 + the NT*4/C terms of the LDS fold in fp32 (the row
         reductions are fp64); for the stand-ins, terms + 2 if that is more
  rows_gather  exact;  rows_sum_by_label  U |ref| + N 2^-53 sum |rows|
Input condition with ReLU, asserted on the final reference: no pre-activation within 8 (U + kappa_n) T_y of zero; offending x elements are moved
away by four margins and the reference recomputed, at most 5 passes, else the case fails.
"""
import zlib

import torch

U = 2.0 ** -24
U64 = 2.0 ** -53
SENTINEL = 123.0
NT, CHUNK = 256, 16384                                 # layernorm.hip
RLN = 16                                               # row lanes of the two row reductions
GRID_YZ_MAX = 65535
C_Y = 5
I32_MIN, I32_MAX = -2 ** 31, 2 ** 31 - 1

MEASURED = {}


def note(group, v):
    MEASURED[group] = max(MEASURED.get(group, 0.0), float(v))


def report():
    return '\n'.join('%-44s %.3g' % kv for kv in sorted(MEASURED.items()))


def f32(v):
    return float(torch.tensor(v, dtype=torch.float32))


def gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()) % 100000)


def chunks_of(D):
    return -(-D // CHUNK)


def ws_bytes(N, D, C):
    """the partials [N][chunks][5] doubles, then the partial rows [2][N * chunks][C] floats"""
    return N * chunks_of(D) * 5 * 8 + 2 * N * chunks_of(D) * C * 4


def ln_ok(D, C):
    return C > 0 and C % 4 == 0 and (NT * 4) % C == 0 and D % C == 0


def param_d(C):
    """the additions on the longest path of a parameter-gradient element: 16 visits of a thread and the NT*4/C terms of the LDS fold (fp32)"""
    return 16 + NT * 4 // C


class Backend:
    """Where the code under test runs: K = ctgan_amd.kernels (HIP, or patched with the stand-ins), F = ctgan_amd.functional over the same K."""

    def __init__(self, K, F, device):
        self.K, self.F, self.device = K, F, device
        self.gpu = device != 'cpu'

    def dev(self, t):
        return t.detach().clone().contiguous().to(self.device)

    def cf(self, t):
        """dense, channel fastest: channels-last for [N,C,H,W], contiguous for [N,C]"""
        if t.dim() == 2:
            return self.dev(t)
        n, c, h, w = t.shape
        buf = torch.empty((n, h, w, c), device=self.device, dtype=t.dtype).permute(0, 3, 1, 2)
        buf.copy_(t.to(self.device))
        return buf

    def d(self, kernel_d, nterms):
        return kernel_d if self.gpu else max(kernel_d, nterms + 2)

    def poison(self, N, D, C):
        """the cached workspace of the next call filled with 0xFF bytes: NaN as float and as double"""
        if self.gpu:
            self.K.workspace(ws_bytes(N, D, C), torch.device(self.device, torch.cuda.current_device())).fill_(0xFF)

    def sync(self):
        if self.gpu:
            torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------------------------ cases
class Case:
    """shape [N,C,H,W] or [N,C]; labels: None, ('cycle', L) or ('bad', L); values: see `_values`; params: see `make_inputs`"""

    def __init__(self, shape, labels=None, relu=False, values='nominal', eps=1e-5, params='random'):
        self.shape, self.labels, self.relu, self.values, self.eps, self.params = tuple(shape), labels, relu, values, f32(eps), params
        self.N, self.C = shape[0], shape[1]
        self.D = 1
        for s in shape[1:]:
            self.D *= s

    @property
    def id(self):
        lab = 'plain' if self.labels is None else '%s%d' % self.labels
        bits = ['x'.join(map(str, self.shape)), lab, 'relu' if self.relu else 'lin']
        if self.values != 'nominal':
            bits.append(self.values)
        if self.eps != f32(1e-5):
            bits.append('eps%g' % self.eps)
        if self.params != 'random':
            bits.append(self.params)
        return '-'.join(bits)


def _grid(shapes, labelings=(None, ('cycle', 10)), **kw):
    return [Case(s, labels=lab, relu=relu, **kw) for s in shapes for lab in labelings for relu in (False, True)]


GEOMETRY_SHAPES = ((5, 4), (3, 4, 2, 3), (2, 16, 8, 8), (2, 16, 5, 13), (2, 4, 64, 64), (2, 4, 17, 241), (2, 32, 24, 24), (2, 512, 4, 4),
                   (2, 1024, 4, 4), (2, 1024, 1, 17), (3, 1024), (2, 128, 32, 32))
GEOMETRY = _grid(GEOMETRY_SHAPES)
# rows of the parameter-gradient reductions (N * chunks): around the 16 row lanes and the 4 x 16 unrolled loop (entered from 49 rows)
ROW_SHAPES = tuple((n, 4) for n in (15, 16, 17, 48, 49, 64, 65, 113)) + ((33, 128, 11, 12),)
ROWS = _grid(ROW_SHAPES, labelings=(None, ('cycle', 10), ('cycle', 1), ('cycle', 1000)))
BAD_LABELS = _grid(((6, 8, 4, 4), (9, 4)), labelings=(('bad', 3), ('bad', 1)))
VALUE_SHAPES = ((3, 128, 8, 8), (3, 8, 16, 16), (5, 16))
VALUES = (_grid(VALUE_SHAPES, values='mean1000') + _grid(VALUE_SHAPES, values='mean-300') + _grid(VALUE_SHAPES, values='std300') +
          _grid(VALUE_SHAPES, values='const') + _grid(VALUE_SHAPES, values='const', eps=1e-12) + _grid(VALUE_SHAPES, eps=0.0) +
          _grid(VALUE_SHAPES, eps=1e-12) + _grid(VALUE_SHAPES, eps=1.0) + _grid(VALUE_SHAPES, params='zero-neg') +
          [c for c in _grid(VALUE_SHAPES, params='mask-off') + _grid(VALUE_SHAPES, params='zero-chan') if c.relu])
ALL_CASES = GEOMETRY + ROWS + BAD_LABELS + VALUES
CONST_VALUE = 2.5                                       # k * 2.5 and k * 6.25 are exact in fp64 for every k here: the moments of that sample are exact
# constants whose squares do not add up exactly in fp64: E[x^2] - mean^2 comes out as rounding noise of either sign, some 1e-10 against an
# eps of 1e-12 or 1e-30, and only the `var < 0` clamp keeps rstd real.  Ten of them, in three sum orders (one visit per thread, two visits, two
# chunks): a build without the clamp has to meet a negative one (a sum order that adds
# equal values in a power-of-two tree is exact at D = 1024 and 2048: there D = 16896 is the case that counts).  eps = 1e-30 is the smallest power of a thousand at which cot_x, which carries
# rstd^2 = 1 / eps, still has room in fp32.
INEXACT_CONSTANTS = (1000.1, -300.7, 77.3, 3333.333, -1234.567, 512.3, 99.9, -2048.7, 640.05, 1428.5714)
CLAMP_SHAPES = ((12, 1024),(12, 8, 16, 16), (12, 128, 11, 12))
CLAMP = _grid(CLAMP_SHAPES, values='const-inexact', eps=1e-12) + _grid(CLAMP_SHAPES, values='const-inexact', eps=1e-30)
ALL_CASES = ALL_CASES + CLAMP
ROWS_DIRECT = ((1, 1), (7, 40), (5, 65), (300, 3), (17, 130), (100, 64))


def _values(kind, shape, g):
    z = torch.randn(*shape, generator=g)
    if kind == 'mean1000':
        return 1000.0 + z
    if kind == 'mean-300':
        return -300.0 + 0.01 * z
    if kind == 'std300':
        return 300.0 * z
    x = 1.7 * z + 0.3
    if kind == 'const':
        x[1] = CONST_VALUE
    if kind == 'const-inexact':
        for i, v in enumerate(INEXACT_CONSTANTS):
            x[1 + i] = v
    return x


def make_labels(kind, N, g):
    """-> (n_labels, int32 labels [N]) or (0, None)"""
    if kind is None:
        return 0, None
    how, L = kind
    if how == 'cycle':
        return L, (torch.arange(N) % L).to(torch.int32)
    bad = [-1, I32_MIN, L, I32_MAX]
    lab = torch.randint(0, L, (N,), generator=g, dtype=torch.int64)
    for i, b in enumerate(bad):
        lab[(1 + i) % N] = b
    if N > 5:
        lab[5] = L - 1
    return L, lab.to(torch.int32)


class Inputs:
    pass


def _forward64(x, sb, ob, eps):
    """the definition, in fp64: (mean, var, r, xh, pre) with the biased variance"""
    dims = tuple(range(1, x.dim()))
    c = x.detach().flatten(1)[:, :1].reshape([-1] + [1] * (x.dim() - 1))
    mean = c + (x - c).mean(dim=dims, keepdim=True)     # shifted by the sample's first element: a constant sample's mean and variance are exact
    var = ((x - mean) ** 2).mean(dim=dims, keepdim=True)
    r = 1.0 / torch.sqrt(var + eps)
    xh = (x - mean) * r
    return mean, var, r, xh, xh * sb + ob


def _kappa(x, mean, r):
    dims = tuple(range(1, x.dim()))
    const = (x == x.flatten(1)[:, :1].reshape(mean.shape)).all(dim=dims, keepdim=True)
    return torch.where(const, torch.zeros_like(mean), U * mean.abs() * r)


def _table_rows(t, labels, N, C, nd):
    """[C] vector or [L, C] table -> broadcastable to x: the row of each sample, labels clamped to the table"""
    if labels is None:
        return t.reshape([1, C] + [1] * (nd - 2))
    return t[labels.long().clamp(0, t.shape[0] - 1)].reshape([N, C] + [1] * (nd - 2))


def make_inputs(case):
    g = gen('layernorm', case.id)
    N, C, D = case.N, case.C, case.D
    inp = Inputs()
    inp.case = case
    x = _values(case.values, case.shape, g).float()
    inp.L, inp.labels = make_labels(case.labels, N, g)
    tshape = (inp.L, C) if inp.labels is not None else (C,)
    s = 1.0 + 0.5 * torch.randn(*tshape, generator=g)
    o = 0.5 * torch.randn(*tshape, generator=g)
    if case.params == 'zero-neg':                      # a zero channel and negative entries
        s[..., 0] = 0.0
        s[..., 1::2] = -s[..., 1::2].abs()
    elif case.params == 'mask-off':                    # |xh| <= sqrt(D): every pre-activation is negative
        o = -(D ** 0.5 * s.abs().max() + 1.0 + o.abs())
    elif case.params == 'zero-chan':                   # y is exactly 0 on channel 0
        s[..., 0] = 0.0
        o[..., 0] = 0.0
    inp.scale, inp.offset = s.float(), o.float()
    inp.gy = torch.randn(*case.shape, generator=g)
    inp.u = torch.randn(*case.shape, generator=g)
    if case.relu:
        sb = _table_rows(inp.scale.double(), inp.labels, N, C, x.dim())
        ob = _table_rows(inp.offset.double(), inp.labels, N, C, x.dim())
        for _ in range(5):
            mean, var, r, xh, pre = _forward64(x.double(), sb, ob, case.eps)
            margin = 8 * (U + _kappa(x, mean, r)) * ((xh.abs() + 1) * sb.abs() + ob.abs())
            bad = pre.abs() < margin
            if not bad.any():
                break
            sign = torch.where(pre < 0, -1.0, 1.0) * torch.where(sb < 0, -1.0, 1.0)
            step = sign * 4 * margin / (r * sb.abs()).clamp_min(1e-300)
            x = torch.where(bad, x.double() + step, x.double()).float()
        else:
            raise AssertionError('%s: pre-activations within the margin of zero after 5 passes' % case.id)
    inp.x = x
    return inp


_REF_CACHE = {}


def reference(case):
    """(inputs, fp64 reference outputs and bounds) of a case, computed once per process and left unchanged"""
    if case.id not in _REF_CACHE:
        _REF_CACHE[case.id] = _reference(make_inputs(case))
    return _REF_CACHE[case.id]


def _reference(inp):
    case = inp.case
    N, C, D = case.N, case.C, case.D
    x = inp.x
    nd = x.dim()
    dims = tuple(range(1, nd))
    sp = tuple(range(2, nd))
    xd = x.double().requires_grad_(True)
    sd = inp.scale.double().requires_grad_(True)
    od = inp.offset.double().requires_grad_(True)
    gyd = inp.gy.double().requires_grad_(True)
    ud = inp.u.double()
    sb, ob = _table_rows(sd, inp.labels, N, C, nd), _table_rows(od, inp.labels, N, C, nd)
    mean, var, r, xh, pre = _forward64(xd, sb, ob, case.eps)
    y = torch.relu(pre) if case.relu else pre
    gx, gs, go = torch.autograd.grad(y, [xd, sd, od], gyd, create_graph=True)
    cots = torch.autograd.grad(gx, [gyd, xd, sd], ud, allow_unused=True)
    cg, cx, cs = (torch.zeros_like(t) if c is None else c for c, t in zip(cots, (gyd, xd, sd)))

    ref = Inputs()
    ref.inp = inp
    with torch.no_grad():
        M = lambda t: t.mean(dim=dims, keepdim=True)
        mask = (pre > 0).double() if case.relu else torch.ones_like(pre)
        sa, oa = sb.abs(), ob.abs()
        X = xh.abs() + 1
        ga, ua, gya = gyd.abs() * sa * mask, ud.abs(), gyd.abs() * mask
        kappa = _kappa(x, mean, r)
        w = U + kappa
        e2 = M(xd * xd)
        # constant samples: exact moments (every partial sum of the squares fits 53 bits) or not; the others' rstd is whatever the fp64
        # cancellation leaves under the clamp, and everything that carries rstd is held to that (rho_n) instead of to U
        const = ((kappa == 0) & (var == 0)).reshape(N)
        exact = torch.zeros(N, dtype=torch.bool)
        for n in torch.nonzero(const).flatten().tolist():
            p, _ = float(x[n].flatten()[0]).as_integer_ratio()
            exact[n] = p * p * D < 2 ** 53
        cancel = (3 * D + 8) * U64 * e2 / (var + case.eps)
        shp = [N] + [1] * (nd - 1)
        wr = w + torch.where((const & ~exact).reshape(shp), cancel, torch.zeros_like(cancel))
        ref.T_y = X * sa + oa
        if case.relu:                                  # the input condition, on the final reference
            assert not (pre.abs() < 8 * w * ref.T_y).any(), case.id
        B, Mm = M(ga * X), M(ua * X)
        cgmag = r * (ua + M(ua) + X * Mm)
        ref.b_y = C_Y * w * ref.T_y
        ref.b_gx = wr * r * (5 * ga + 6 * M(ga) + 13 * X * B)
        ref.b_cg = wr * r * (5 * ua + 6 * M(ua) + 13 * X * Mm) * sa * mask
        ref.b_cx = wr * r * r * (14 * (B * ua + Mm * ga) + 15 * (B * M(ua) + Mm * M(ga)) +
                                 X * ((2 * 22 + 24) * B * Mm + 16 * M(ua * ga) + 16 * M(ga) * M(ua)))

        def by_param(t):
            t = t.sum(dim=sp) if sp else t
            if inp.labels is None:
                return t.sum(dim=0)
            return torch.zeros(inp.L, C, dtype=torch.float64).index_add_(0, inp.labels.long().clamp(0, inp.L - 1), t)
        ref.m_gs, ref.m_go, ref.m_cs = by_param(w * gya * X), by_param(w * gya), by_param(wr * gya * cgmag)
        if inp.labels is None:
            ref.nterms = N * D // C
        else:
            ref.nterms = int(torch.bincount(inp.labels.long().clamp(0, inp.L - 1)).max()) * D // C
        ref.mean, ref.rstd = mean.detach().reshape(N), r.detach().reshape(N)
        ref.b_mean = (U * mean.abs() + D * U64 * M(xd.abs())).reshape(N)
        ref.b_rstd = (r * (U + torch.where(exact.reshape(shp), torch.full_like(cancel, 4 * U64), cancel))).reshape(N)
        ref.const, ref.exact = const, exact
    for k, v in dict(y=y, gx=gx, gs=gs, go=go, cg=cg, cx=cx, cs=cs).items():
        setattr(ref, k, v.detach())
    return ref


# ------------------------------------------------------------------------------------------------------------------ checks
def bounded(group, got, ref, bound):
    """|got - ref| <= bound per element (exactly equal where the bound is 0); records the largest fraction of the bound used"""
    got = got.detach().cpu().double()
    assert tuple(got.shape) == tuple(ref.shape) == tuple(bound.shape), (group, got.shape, ref.shape, bound.shape)
    assert torch.isfinite(got).all(), group
    diff = (got - ref).abs()
    assert (diff[bound == 0] == 0).all(), group
    frac = float((diff / bound.clamp_min(1e-300)).max()) if diff.numel() else 0.0
    note(group + ' (of bound)', frac)
    assert frac <= 1.0, (group, frac)


def same_bits(group, a, b):
    assert (a is None) == (b is None), group
    if a is not None:
        assert torch.equal(a.detach().cpu().view(torch.int32), b.detach().cpu().view(torch.int32)), group


class Run:
    """the device (or stand-in) tensors and outputs of one case"""


def device_inputs(be, ref):
    inp = ref.inp
    run = Run()
    run.x, run.gy, run.u = be.cf(inp.x), be.cf(inp.gy), be.cf(inp.u)
    run.scale, run.offset = be.dev(inp.scale), be.dev(inp.offset)
    run.labels = be.dev(inp.labels) if inp.labels is not None else None
    return run


def call_fwd(be, case, run):
    K = be.K
    if run.labels is None:
        return K.layernorm_fwd(run.x, run.scale, run.offset, case.eps, case.relu)
    return K.layernorm_cond_fwd(run.x, run.scale, run.offset, run.labels, case.eps, case.relu)


def call_bwd(be, case, run, want_params=True, gy=None):
    K = be.K
    gy = run.gy if gy is None else gy
    ymask = run.y if case.relu else None
    if run.labels is None:
        return K.layernorm_bwd(gy, run.x, run.scale, run.mean, run.rstd, want_params, ymask)
    return K.layernorm_cond_bwd(gy, run.x, run.scale, run.labels, run.mean, run.rstd, want_params, ymask)


def call_bwd2(be, case, run, want=(True, True, True), gy=None, u=None):
    K = be.K
    gy = run.gy if gy is None else gy
    u = run.u if u is None else u
    ymask = run.y if case.relu else None
    if run.labels is None:
        return K.layernorm_bwd2(u, gy, run.x, run.scale, run.mean, run.rstd, want[0], want[1], want[2], ymask)
    return K.layernorm_cond_bwd2(u, gy, run.x, run.scale, run.labels, run.mean, run.rstd, want[0], want[1], want[2], ymask)


def run_case(be, case, poison=True):
    """fwd, bwd (with the parameter gradients) and bwd2 (all outputs) of a case at the kernel level; bwd / bwd2 get the product's own mean / rstd"""
    ref = reference(case)
    run = device_inputs(be, ref)
    pz = (lambda: be.poison(case.N, case.D, case.C)) if poison else (lambda: None)
    pz()
    run.y, run.mean, run.rstd = call_fwd(be, case, run)
    pz()
    run.gx, run.gs, run.go = call_bwd(be, case, run)
    pz()
    run.cg, run.cx, run.cs = call_bwd2(be, case, run)
    be.sync()
    return ref, run


OUTPUTS = ('y', 'mean', 'rstd', 'gx', 'gs', 'go', 'cg', 'cx', 'cs')


GROUPS = dict(y='y', mean='mean', rstd='rstd', gx='gx', gs='gscale', go='goffset', cg='cot_gy', cx='cot_x', cs='cot_scale')


def bounds(be, case, ref):
    """output name -> (reference, bound)"""
    C = case.C
    return dict(mean=(ref.mean, ref.b_mean), rstd=(ref.rstd, ref.b_rstd), y=(ref.y, ref.b_y), gx=(ref.gx, ref.b_gx), cg=(ref.cg, ref.b_cg),
                cx=(ref.cx, ref.b_cx), gs=(ref.gs, be.d(param_d(C), ref.nterms) * ref.m_gs),
                go=(ref.go, be.d(param_d(C), ref.nterms) * ref.m_go), cs=(ref.cs, be.d(param_d(C), ref.nterms) * ref.m_cs))


def agree(be, case, ref, name, got, full, tag):
    """the bits of `full` on the device; for the stand-ins (no bit contracts) the bound of that output"""
    if be.gpu:
        same_bits(name + tag, got, full)
    else:
        bounded(GROUPS[name] + tag, got, *bounds(be, case, ref)[name])


def check_outputs(be, case, ref, run, tag=''):
    C, inp = case.C, ref.inp
    for t in (run.y, run.gx, run.cg, run.cx):
        assert t.stride() == run.x.stride() and tuple(t.shape) == case.shape
    for name, (want, bound) in bounds(be, case, ref).items():
        bounded(GROUPS[name] + tag, getattr(run, name), want, bound)
    # a constant sample: mean is its value, y its offset row [relu of it], bit for bit.  The product's rstd is 1 / sqrt(eps) to one rounding
    # where the moments are exact; where they are not, the clamp at var = 0 makes 1 / sqrt(eps) its upper limit (a negative var + eps is NaN,
    # a negative var above -eps a larger rstd)
    top = case.eps ** -0.5 if case.eps else float('inf')          # no constant sample at eps = 0
    for n in torch.nonzero(ref.const).flatten().tolist():
        assert float(run.mean[n]) == float(inp.x[n].flatten()[0]), case.id
        row = inp.offset if inp.labels is None else inp.offset[int(inp.labels[n].long().clamp(0, inp.L - 1))]
        want = (torch.relu(row) if case.relu else row).reshape([C] + [1] * (inp.x.dim() - 2)).expand(inp.x.shape[1:])
        assert torch.equal(run.y[n].detach().cpu(), want), case.id
        assert abs(float(ref.rstd[n]) - top) <= 1e-12 * top
        got = float(run.rstd[n])
        if ref.exact[n]:
            assert abs(got - top) <= (U + 4 * U64) * top, (case.id, n, got, top)
        else:
            assert 0 < got <= (1 + U + 4 * U64) * top, (case.id, n, got, top)
    if case.params == 'mask-off':
        for name in ('y', 'gx', 'cg', 'gs', 'go', 'cs'):
            assert (getattr(run, name) == 0).all(), (case.id, name)
    if case.params == 'zero-chan':
        assert (run.y[:, 0] == 0).all(), case.id


def check_case(be, case):
    ref, run = run_case(be, case)
    check_outputs(be, case, ref, run)
    return ref, run


# ------------------------------------------------------------------------------------------------------------------ the other contracts
def check_small_after_large(be):
    """A small shape on the workspace a larger call left behind (finite, stale partials and rows): the same bits as on a poisoned one."""
    big, small = Case((2, 128, 32, 32), labels=('cycle', 10), relu=True), Case((5, 4), labels=('cycle', 10), relu=True)
    _, want = run_case(be, small)
    run_case(be, big)
    ref, got = run_case(be, small, poison=False)
    check_outputs(be, small, ref, got, tag=', stale workspace')
    if be.gpu:
        for name in OUTPUTS:
            same_bits(name, getattr(got, name), getattr(want, name))


SELECT_CASES = [Case((2, 4, 17, 241), labels=lab, relu=relu) for lab in (None, ('cycle', 10)) for relu in (False, True)]


def check_output_selection(be, case):
    """bwd with and without the parameter gradients, bwd2 with all eight subsets: every requested output has the bits of the all-outputs call."""
    ref, run = check_case(be, case)
    be.poison(case.N, case.D, case.C)
    gx, gs, go = call_bwd(be, case, run, want_params=False)
    assert gs is None and go is None
    agree(be, case, ref, 'gx', gx, run.gx, ', no parameter gradients')
    full = (run.cg, run.cx, run.cs)
    for k in range(8):
        want = (bool(k & 1), bool(k & 2), bool(k & 4))
        be.poison(case.N, case.D, case.C)
        outs = call_bwd2(be, case, run, want=want)
        for w, o, f, name in zip(want, outs, full, ('cg', 'cx', 'cs')):
            if w:
                agree(be, case, ref, name, o, f, ', subset')
            else:
                assert o is None


def check_determinism(be, case, other):
    _, a = run_case(be, case)
    run_case(be, other)
    _, b = run_case(be, case)
    for name in OUTPUTS:
        same_bits(name, getattr(a, name), getattr(b, name))


LAYOUT_CASES = [Case((3, 8, 6, 10), labels=lab, relu=relu) for lab in (None, ('cycle', 10)) for relu in (False, True)]


def check_layouts(be, case):
    """F.layer_norm on an NCHW-contiguous x (repacked to channels-last, differentiated twice through autograd); gy and u NCHW-contiguous
    against a channels-last x (the match_layout branch of the wrappers)."""
    ref, run = check_case(be, case)
    inp = ref.inp
    x = be.dev(inp.x).requires_grad_(True)
    s, o = run.scale.clone().requires_grad_(True), run.offset.clone().requires_grad_(True)
    assert x.is_contiguous()
    y = be.F.layer_norm(x, s, o, eps=case.eps, relu=case.relu, labels=run.labels)
    bounded('y, NCHW x', y, ref.y, ref.b_y)
    gyd, ud = be.dev(inp.gy).requires_grad_(True), be.dev(inp.u)
    gx, gs, go = torch.autograd.grad(y, [x, s, o], gyd, create_graph=True)
    bounded('gx, NCHW x', gx, ref.gx, ref.b_gx)
    bounded('gscale, NCHW x', gs, ref.gs, be.d(param_d(case.C), ref.nterms) * ref.m_gs)
    bounded('goffset, NCHW x', go, ref.go, be.d(param_d(case.C), ref.nterms) * ref.m_go)
    cg, cx, cs = torch.autograd.grad(gx, [gyd, x, s], ud)
    bounded('cot_gy, NCHW x', cg, ref.cg, ref.b_cg)
    bounded('cot_x, NCHW x', cx, ref.cx, ref.b_cx)
    bounded('cot_scale, NCHW x', cs, ref.cs, be.d(param_d(case.C), ref.nterms) * ref.m_cs)
    gyn, un = be.dev(inp.gy), be.dev(inp.u)
    assert gyn.stride() != run.x.stride()
    gx2, gs2, go2 = call_bwd(be, case, run, gy=gyn)
    c2 = call_bwd2(be, case, run, gy=gyn, u=un)
    for name, got in zip(('gx', 'gs', 'go', 'cg', 'cx', 'cs'), (gx2, gs2, go2) + tuple(c2)):
        agree(be, case, ref, name, got, getattr(run, name), ', NCHW gy / u')
    assert gx2.stride() == run.x.stride() and c2[0].stride() == run.x.stride()


def check_rows_direct(be, N, C, labeling):
    """K.rows_gather (exact) and K.rows_sum_by_label (fp64, fixed order, one cast) on their own, labels clamped to the table"""
    g = gen('rows', N, C, labeling)
    L, labels = make_labels(labeling, N, g)
    table = torch.randn(L, C, generator=g)
    rows = torch.randn(N, C, generator=g)
    clamped = labels.long().clamp(0, L - 1)
    be.poison(1, 4, 4)
    out = be.K.rows_gather(be.dev(table), be.dev(labels))
    assert tuple(out.shape) == (N, C) and torch.equal(out.detach().cpu(), table[clamped])
    got = be.K.rows_sum_by_label(be.dev(rows), be.dev(labels), L)
    ref = torch.zeros(L, C, dtype=torch.float64).index_add_(0, clamped, rows.double())
    mag = torch.zeros(L, C, dtype=torch.float64).index_add_(0, clamped, rows.double().abs())
    bounded('rows_sum_by_label', got, ref, U * ref.abs() + N * U64 * mag)
    absent = torch.ones(L, dtype=torch.bool)
    absent[clamped] = False
    assert (got.detach().cpu()[absent] == 0).all()
