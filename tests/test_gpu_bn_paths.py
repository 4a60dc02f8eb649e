"""The generator's training-mode batch norm (csrc/bn.hip) at every branch of its launch plan, and its two conv-fused forms (batch norm applied
while a conv stages its input: conv16x3hf_kernel<true, TN, true> in csrc/igemm16.hip, m2f_px_kernel with bn_mean in csrc/fewch.hip), each against
an fp64 reference built from oracle.tf_ops: moments over [0,2,3] per statistic group (biased variance), batch_normalization(..., eps) with the
scale / offset rows gathered by label, relu, conv2d_same / bias_add_nchw; gradients by torch.autograd.grad in double.

  A  bn_fwd / bn_bwd where mk() picks the other plan (pos = 256), where chunks are ragged, on every reason for the scalar fallback, at both ends
     of the vector kernels' lane split, through both loops of the finalisation, and with labels that no / every sample carries;
  B  bn_fwd_f64 on a channel whose spread is far below its mean;
  C  batch norm on load in the split mode's halo kernel, with label tables whose rows DIFFER (with the initial ones / zeros of the generator a wrong
     label, channel quad or chunk cannot show), on each tile shape, and its refusals;
  D  batch norm on load in the many -> few pixel kernel on partial 8-row tiles;
  E  conv_fwd_bn_in_supported never promises a launch that conv_fwd_bn_in refuses.
"""
import zlib

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import tf_ops  # noqa: E402


@pytest.fixture(scope='module')
def K():
    import ctgan_amd.kernels as K
    hybrid = K.X3_HYBRID
    yield K
    K.set_mma_dtype(None)
    K.X3_HYBRID = hybrid
    K.debug_x3_hk(1)
    K.debug_x3_halo_always(False)


def cl(t):
    d = t.to('cuda')
    out = torch.empty((d.shape[0], d.shape[2], d.shape[3], d.shape[1]), device='cuda', dtype=d.dtype).permute(0, 3, 1, 2)
    out.copy_(d)
    return out


def dev(t):
    return t.to('cuda').contiguous()


def relerr(a, b):
    a = a.detach().cpu().double(); b = b.detach().cpu().double()
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-30)).item()


def rel_l2(a, b):
    a = a.detach().cpu().double(); b = b.detach().cpu().double()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


def _seed(*key):
    return zlib.crc32(repr(key).encode()) % 100000


def bn_inputs(g, n, c, h, w, cond, labels=None):
    """x = randn * 2 + 3 (a normalised zero is far from zero), scale = rand + 0.5, offset = randn ([10, C] tables when conditional)."""
    x = torch.randn(n, c, h, w, generator=g) * 2 + 3.0
    nl = 10 if cond else 1
    scale = torch.rand(nl, c, generator=g) + 0.5
    offset = torch.randn(nl, c, generator=g)
    if cond and labels is None:
        labels = torch.randint(0, 10, (n,), generator=g, dtype=torch.int32)
    return x, scale, offset, (labels if cond else None)


def bn_ref(x, scale, offset, labels, groups, relu, eps=1e-5):
    """fp64: x, scale, offset double (leaves or not) -> relu?(bn(x)), [mean per group], [var per group]."""
    n = x.shape[0]
    per = n // groups
    outs, means, vars_ = [], [], []
    for gi in range(groups):
        xs = x[gi * per:(gi + 1) * per]
        mean, var = tf_ops.moments(xs, [0, 2, 3])
        lab = labels[gi * per:(gi + 1) * per].long() if labels is not None else torch.zeros(per, dtype=torch.long)
        outs.append(tf_ops.batch_normalization(xs, mean, var, offset[lab][:, :, None, None], scale[lab][:, :, None, None], eps))
        means.append(mean.reshape(-1)); vars_.append(var.reshape(-1))
    y = torch.cat(outs)
    return (torch.relu(y) if relu else y), torch.stack(means), torch.stack(vars_)


# ------------------------------------------------------------------------------------------------------------------------------------ A
# (n, c, H, W, groups, cond, relu, fixed label): what the case reaches in csrc/bn.hip
BN_CASES = [
    (512, 8, 3, 3, 2, True, True, None),      # pos = 256 (512 x 1 >= 512), hc = 1; vector path, 128 row lanes over 9 positions; 256 partial rows per group
    (256, 4, 16, 20, 1, False, True, None),   # pos = 256 (256 x 2), hc = 2 with a 64-position second chunk; c4n = 1 (256 row lanes); three APOS blocks, the last 64
    (3, 16, 11, 13, 1, True, False, None),    # pos = 64, hc = 3 with a 15-position tail; APOS tail of 15; at least seven absent labels
    (70, 8, 3, 3, 1, True, True, None),       # 70 partial rows: one unrolled pass on every finalisation lane, the remainder on six; > 16 samples per label job
    (70, 8, 3, 3, 2, True, True, None),       # 35 rows per group: the remainder loop only; group boundary at an odd sample
    (4, 1024, 2, 4, 2, True, True, None),     # c4n = 256: one row lane; hw = 8, the vector path's lower limit
    (5, 6, 5, 7, 1, True, True, None),        # scalar kernels: c % 4 != 0, with labels and ReLU
    (4, 130, 3, 3, 2, False, True, None),     # scalar: three 64-channel blocks, the last with two channels
    (6, 24, 4, 4, 2, True, True, None),       # scalar because c/4 = 6 does not divide 256
    (8, 128, 2, 2, 2, True, True, None),      # scalar because hw = 4 < 8, channels aligned
    (2, 2048, 3, 3, 1, False, True, None),    # scalar because c/4 > 256
    (6, 16, 8, 8, 1, True, True, 7),          # one label carries the whole batch
]


def _bn_check(K, x, scale, offset, labels, groups, relu, gy, two_d=False):
    cond = labels is not None
    xr = x.double().requires_grad_(True); sr = scale.double().requires_grad_(True); orr = offset.double().requires_grad_(True)
    ref, _, _ = bn_ref(xr, sr, orr, labels, groups, relu)
    gr = torch.autograd.grad(ref, [xr, sr, orr], gy.double())
    labd = dev(labels) if cond else None
    if two_d:
        xin, gyin = dev(x[:, :, 0, 0]), dev(gy[:, :, 0, 0])
    else:
        xin, gyin = cl(x), cl(gy)
    y, mean, rstd, x4 = K.bn_fwd(xin, dev(scale), dev(offset), labd, groups, relu)
    if two_d:
        assert y.dim() == 2 and x4.dim() == 4
    e = relerr(y.reshape(ref.shape), ref)
    print('bn_fwd y %.3g' % e)
    assert e < 2e-5, e
    gx, gs, go = K.bn_bwd(gyin, x4, mean, rstd, dev(scale), dev(offset), labd, groups, relu)
    es = relerr(gx.reshape(ref.shape), gr[0]), relerr(gs, gr[1]), relerr(go, gr[2])
    print('bn_bwd gx %.3g gscale %.3g goffset %.3g' % es)
    assert es[0] < 1e-4 and es[1] < 1e-4 and es[2] < 1e-4, es
    if cond:
        absent = sorted(set(range(scale.shape[0])) - set(labels.tolist()))
        for l in absent:          # a label no sample carries: a WRITTEN row of exact zeros (the fp64 reference gives exact zeros there)
            assert gr[1][l].abs().max().item() == 0.0 and gr[2][l].abs().max().item() == 0.0
            assert gs[l].abs().max().item() == 0.0 and go[l].abs().max().item() == 0.0, l
        return absent
    return []


@pytest.mark.parametrize('case', BN_CASES, ids=lambda c: 'n%d_c%d_%dx%d_g%d_%s%s%s' % (c[0], c[1], c[2], c[3], c[4], 'cond' if c[5] else 'plain',
                                                                                          '_relu' if c[6] else '', '' if c[7] is None else '_all%d' % c[7]))
def test_batchnorm_plan_branches(K, case):
    n, c, h, w, groups, cond, relu, fixed = case
    g = torch.Generator().manual_seed(_seed('A', case))
    labels = torch.full((n,), fixed, dtype=torch.int32) if fixed is not None else None
    x, scale, offset, labels = bn_inputs(g, n, c, h, w, cond, labels)
    gy = torch.randn(n, c, h, w, generator=g)
    absent = _bn_check(K, x, scale, offset, labels, groups, relu, gy)
    if case[:4] == (3, 16, 11, 13):
        assert len(absent) >= 7
    if fixed is not None:
        assert len(absent) == 9


@pytest.mark.parametrize('n,c,groups,relu', [(8, 128, 2, True), (8, 6, 1, False)])
def test_batchnorm_two_dimensional_input(K, n, c, groups, relu):
    """bn_fwd / bn_bwd with an [N, C] input and gradient: the x.dim() == 2 wrapper path (hw = 1: the scalar kernels)."""
    g = torch.Generator().manual_seed(_seed('A2', n, c))
    x, scale, offset, labels = bn_inputs(g, n, c, 1, 1, True)
    gy = torch.randn(n, c, 1, 1, generator=g)
    _bn_check(K, x, scale, offset, labels, groups, relu, gy, two_d=True)


# ------------------------------------------------------------------------------------------------------------------------------------ B
@pytest.mark.parametrize('shape', [(8, 16, 8, 8), (4, 128, 4, 4)], ids=lambda s: 'x'.join(map(str, s)))
def test_batchnorm_f64_statistics_keep_a_variance_far_below_the_mean(K, shape):
    """K.bn_fwd_f64 (ctgan_bn_stats_f64) where fp32 partial sums lose the variance: x = 0.5 + 1e-3 * randn, eps = 1e-6; the fp64 reference is
    computed from the float32 values of x."""
    n, c, h, w = shape
    g = torch.Generator().manual_seed(_seed('B', shape))
    x = (0.5 + 1e-3 * torch.randn(n, c, h, w, generator=g)).float()
    scale = torch.rand(1, c, generator=g) + 0.5
    offset = torch.randn(1, c, generator=g)
    ref, mean_ref, var_ref = bn_ref(x.double(), scale.double(), offset.double(), None, 1, False, eps=1e-6)
    rstd_ref = torch.rsqrt(var_ref + 1e-6)
    y, mean, rstd, _ = K.bn_fwd_f64(cl(x), dev(scale), dev(offset), None, 1, False, eps=1e-6)
    em = ((mean.cpu().double() - mean_ref).abs() / mean_ref.abs()).max().item()
    er = ((rstd.cpu().double() - rstd_ref).abs() / rstd_ref.abs()).max().item()
    ey = relerr(y, ref)
    print('bn_fwd_f64 mean %.3g rstd %.3g y %.3g' % (em, er, ey))
    # A CPU emulation of the entry point (fp64 sums, cast to float32, float32 apply) gives 4e-8 .. 6e-8 for rstd and 3e-6 .. 6e-6 for y on
    # these inputs; the same emulation with 8-term fp32 partial sums puts rstd off by 2e-3 .. 7e-3.  1e-6 sits ~16x above the rounding of the
    # result and > 1000x below what the entry point exists to avoid.
    assert em <= 1e-6, em
    assert er <= 1e-6, er
    assert ey < 2e-5, ey


# ------------------------------------------------------------------------------------------------------------------------------------ C
def conv_inputs(g, N, C, H, W, Ko, cond, resid):
    x, scale, offset, labels = bn_inputs(g, N, C, H, W, cond)
    w = torch.randn(3, 3, C, Ko, generator=g) / np.sqrt(9 * C)
    b = torch.randn(Ko, generator=g)
    r = None
    if resid == 'same':
        r = torch.randn(N, Ko, H, W, generator=g)
    elif resid == 'up':
        r = torch.randn(N, Ko, H // 2, W // 2, generator=g)
    return x, scale, offset, labels, w, b, r


def conv_ref(x, scale, offset, labels, groups, w, b, r, resid):
    h, mean, var = bn_ref(x.double(), scale.double(), offset.double(), labels, groups, True)
    y = tf_ops.bias_add_nchw(tf_ops.conv2d_same(h, w.double(), 1), b.double())
    if resid == 'same':
        y = y + r.double()
    elif resid == 'up':
        y = y + r.double().repeat_interleave(2, dim=2).repeat_interleave(2, dim=3)
    return y, mean, var


def _fused_vs_unfused(K, case, kernel, seed_key):
    """One case of C in the mode the caller set: fused and unfused against fp64 and against each other, then again with the labels rotated."""
    N, C, H, W, Ko, groups, cond, resid = case
    g = torch.Generator().manual_seed(_seed(seed_key, case))
    x, scale, offset, labels, w, b, r = conv_inputs(g, N, C, H, W, Ko, cond, resid)
    geom = K.ConvGeom(C, H, W, Ko, 3, 3, 1)
    xd, wd, bd, sd, od = cl(x), dev(w), dev(b), dev(scale), dev(offset)
    rd = cl(r) if r is not None else None
    up = resid == 'up'
    # the unfused composition reads the half-resolution residual through the SAME halo kernel's epilogue only on launches the routing sends
    # there; a launch of a few tiles would take it to the fp32 MFMA family (another summation order).  Materialised, it is the same addend.
    rd_full = K.upsample2(rd, 1.0) if up else rd
    assert K.conv_fwd_bn_in_supported(xd, geom, labels=labels, resid=rd)
    mean, rstd = K.bn_stats(xd, groups)
    outs = []
    for lab in ([labels, (labels + 1) % 10] if cond else [None]):
        labd = dev(lab) if cond else None
        ref, mean_ref, var_ref = conv_ref(x, scale, offset, lab, groups, w, b, r, resid)
        assert relerr(mean, mean_ref) < 2e-5 and relerr(rstd, torch.rsqrt(var_ref + 1e-5)) < 2e-5
        fused = K.conv_fwd_bn_in(xd, wd, bd, geom, mean, rstd, sd, od, groups, relu_in=True, labels=labd, resid=rd, resid_up=up)
        kf = K.last_kernel()
        assert kf.endswith(',bn>') and kf == kernel, kf
        unfused = K.conv_fwd(K.bn_fwd(xd, sd, od, labd, groups, True)[0], wd, bd, geom, resid=rd_full)
        ku = K.last_kernel()
        e_unfused, e_fused = rel_l2(unfused, ref), rel_l2(fused, ref)
        diff = float((fused - unfused).abs().max()) / float(unfused.abs().max())
        print('%s: %s (unfused: %s) e_unfused %.3g e_fused %.3g max|fused - unfused| / max %.3g equal %s'
              % (case, kf, ku, e_unfused, e_fused, diff, torch.equal(fused, unfused)))
        assert e_fused <= max(2 * e_unfused, 2e-5), (e_fused, e_unfused)
        assert ku == kernel.replace(',bn>', '>'), ku      # the same conv kernel, without the norm on load
        assert diff <= 1e-6, diff
        assert torch.equal(fused, unfused), diff
        outs.append(fused)
    if cond:          # a kernel that ignores the label, or reads another sample's, gives the same result twice or misses its own reference
        assert not torch.equal(outs[0], outs[1])
        assert float((outs[0] - outs[1]).abs().max()) > 1e-2 * float(outs[0].abs().max())


# (N, C, H, W, Kout, groups, cond, resid) -> the kernel conv16x3hf_tile picks
HALO_CASES = [
    ((4, 64, 8, 8, 128, 2, True, 'same'), 'conv16x3hf<32x128,k32,bn>'),        # half-image tiles, two channel chunks
    ((2, 32, 12, 8, 128, 1, True, None), 'conv16x3hf<32x128,k32,bn>'),         # 32-pixel tiles of four rows, three per image, H != W
    ((2, 64, 16, 16, 128, 2, True, 'up'), 'conv16x3hf<64x128,k32,bn>'),
    ((2, 32, 32, 32, 256, 1, False, 'same'), 'conv16x3hf<128x128,k32,bn>'),    # two kout tiles
    ((3, 96, 16, 16, 128, 3, True, 'up'), 'conv16x3hf<64x128,k32,bn>'),        # three chunks, one sample per group, odd N
]


@pytest.fixture
def split_mode(K):
    """The split mode with both forms on the pixel-tiled halo kernel: no chunk-per-wave kernel (another summation order), and the unfused conv of
    these few-tile launches on the halo kernel too instead of the slice kernels the routing would give them."""
    K.debug_x3_hk(0)
    K.debug_x3_halo_always(True)
    try:
        with K.mma_dtype('f32x3'):
            yield
    finally:
        K.debug_x3_halo_always(False)
        K.debug_x3_hk(1)


@pytest.mark.parametrize('case,kernel', HALO_CASES, ids=lambda v: 'x'.join(map(str, v)) if isinstance(v, tuple) else None)
def test_batchnorm_on_load_in_the_halo_kernel(K, split_mode, case, kernel):
    _fused_vs_unfused(K, case, kernel, 'C')


def test_batchnorm_on_load_in_the_default_mode(K):
    """MMA_DTYPE None with the hybrid routing: 64 rows of 16x16 are 256 tiles of 64 pixels, which the routing hands to the halo kernel."""
    hybrid, K.X3_HYBRID = K.X3_HYBRID, True
    K.debug_x3_hk(0)
    try:
        assert K.MMA_DTYPE is None
        _fused_vs_unfused(K, (64, 32, 16, 16, 128, 2, True, 'same'), 'conv16x3hf<64x128,k32,bn>', 'C0')
    finally:
        K.debug_x3_hk(1)
        K.X3_HYBRID = hybrid


def _refusal_args(K, N, C, H, Ko, stride=1):
    g = torch.Generator().manual_seed(_seed('R', N, C, H, Ko, stride))
    x, scale, offset, labels, w, b, _ = conv_inputs(g, N, C, H, H, Ko, True, None)
    geom = K.ConvGeom(C, H, H, Ko, 3, 3, stride)
    xd = cl(x)
    mean, rstd = K.bn_stats(xd, 1)
    return geom, (xd, dev(w), dev(b), geom, mean, rstd, dev(scale), dev(offset), 1), dev(labels)


def test_batchnorm_on_load_refusals(K):
    """What the launch does not take raises NotImplementedError (an error code before any launch), never a tensor."""
    K.debug_x3_hk(0)
    try:
        with K.mma_dtype('f32x3'):
            for N, C, H, Ko, stride, relu_in in [(4, 64, 8, 128, 1, False),      # no ReLU behind the norm
                                                 (2, 32, 4, 128, 1, True),       # 4x4 images: a tile spans two samples
                                                 (4, 64, 8, 64, 1, True),        # Kout = 64
                                                 (4, 64, 8, 128, 2, True)]:      # stride 2
                geom, args, labels = _refusal_args(K, N, C, H, Ko, stride)
                with pytest.raises(NotImplementedError):
                    K.conv_fwd_bn_in(*args, relu_in=relu_in, labels=labels)
                if relu_in:
                    assert not K.conv_fwd_bn_in_supported(args[0], geom, labels=labels)
        hybrid, K.X3_HYBRID = K.X3_HYBRID, True
        try:          # the default mode: a launch too small for the routing
            assert K.MMA_DTYPE is None
            geom, args, labels = _refusal_args(K, 2, 32, 8, 128)
            assert not K.conv_fwd_bn_in_supported(args[0], geom, labels=labels)
            with pytest.raises(NotImplementedError):
                K.conv_fwd_bn_in(*args, relu_in=True, labels=labels)
        finally:
            K.X3_HYBRID = hybrid
    finally:
        K.debug_x3_hk(1)


# ------------------------------------------------------------------------------------------------------------------------------------ D
@pytest.mark.parametrize('N,C,H,groups', [(4, 64, 12, 2),      # the second 8-row tile is partial
                                          (2, 128, 5, 2),      # a single partial tile
                                          (3, 256, 32, 1)])
def test_batchnorm_on_load_in_the_many_to_few_pixel_kernel(K, N, C, H, groups):
    g = torch.Generator().manual_seed(_seed('D', N, C, H))
    x, scale, offset, _ = bn_inputs(g, N, C, H, 32, False)
    w = torch.randn(3, 3, C, 3, generator=g) / np.sqrt(9 * C)
    b = torch.randn(3, generator=g)
    geom = K.ConvGeom(C, H, 32, 3, 3, 3, 1)
    xd, wd, bd, sd, od = cl(x), dev(w), dev(b), dev(scale), dev(offset)
    assert K.conv_fwd_bn_in_supported(xd, geom, tanh=True) and K.conv_fwd_bn_in_supported(xd, geom)
    mean, rstd = K.bn_stats(xd, groups)
    h, mean_ref, var_ref = bn_ref(x.double(), scale.double(), offset.double(), None, groups, True)
    assert relerr(mean, mean_ref) < 2e-5 and relerr(rstd, torch.rsqrt(var_ref + 1e-5)) < 2e-5
    pre = tf_ops.bias_add_nchw(tf_ops.conv2d_same(h, w.double(), 1), b.double())
    nchw = (3 * geom.P * geom.Q, geom.P * geom.Q, geom.Q, 1)          # the generator's output layout
    for tanh in (True, False):
        for strides in ((nchw, None) if (N, tanh) == (4, True) else (nchw,)):      # one case also with the default channels-last result
            ref = torch.tanh(pre) if tanh else pre
            fused = K.conv_fwd_bn_in(xd, wd, bd, geom, mean, rstd, sd, od, groups, relu_in=True, tanh=tanh, out_strides=strides)
            assert K.last_kernel() == 'fewch_m2f(bn)', K.last_kernel()
            unfused = K.conv_fwd(K.bn_fwd(xd, sd, od, None, groups, True)[0], wd, bd, geom, out_strides=strides)
            if tanh:
                unfused = K.tanh_fwd(unfused)
            assert fused.stride() == unfused.stride() and (strides is None or fused.stride() == nchw)
            e_unfused, e_fused = rel_l2(unfused, ref), rel_l2(fused, ref)
            diff = float((fused - unfused).abs().max()) / float(unfused.abs().max())
            print('m2f N%d C%d H%d tanh=%s %s: e_unfused %.3g e_fused %.3g max|fused - unfused| / max %.3g equal %s'
                  % (N, C, H, tanh, 'nchw' if strides else 'cl', e_unfused, e_fused, diff, torch.equal(fused, unfused)))
            assert e_fused <= max(2 * e_unfused, 2e-5), (e_fused, e_unfused)
            assert diff <= 1e-6, diff
            assert torch.equal(fused, unfused), diff
    labels = torch.zeros(N, dtype=torch.int32, device='cuda')
    with pytest.raises(NotImplementedError):
        K.conv_fwd_bn_in(xd, wd, bd, geom, mean, rstd, sd, od, groups, relu_in=True, labels=labels)
    with pytest.raises(NotImplementedError):
        K.conv_fwd_bn_in(xd, wd, bd, geom, mean, rstd, sd, od, groups, relu_in=True, resid=torch.zeros(N, 3, H, 32, device='cuda'))


# ------------------------------------------------------------------------------------------------------------------------------------ E
@pytest.mark.parametrize('mode', ['f32x3', None])
def test_supported_never_promises_a_launch_that_is_refused(K, mode):
    """conv_fwd_bn_in_supported is asked before the moments so that a caller who falls back does not pay a bn_stats launch twice: whenever it
    says yes, conv_fwd_bn_in must run."""
    g = torch.Generator().manual_seed(_seed('E'))
    hybrid, K.X3_HYBRID = K.X3_HYBRID, True
    yes = 0
    try:
        with K.mma_dtype(mode):
            for N in (2, 64):
                for H in (4, 8, 12, 16, 32):
                    for C in (32, 48, 64):
                        x = cl(torch.randn(N, C, H, H, generator=g))
                        mean, rstd = K.bn_stats(x, 2)
                        scale = dev(torch.rand(10, C, generator=g) + 0.5); offset = dev(torch.randn(10, C, generator=g))
                        labels = dev(torch.randint(0, 10, (N,), generator=g, dtype=torch.int32))
                        for Ko in (64, 128):
                            geom = K.ConvGeom(C, H, H, Ko, 3, 3, 1)
                            w = dev(torch.randn(3, 3, C, Ko, generator=g) / np.sqrt(9 * C)); b = dev(torch.randn(Ko, generator=g))
                            resid = cl(torch.randn(N, Ko, H, H, generator=g))
                            if not K.conv_fwd_bn_in_supported(x, geom, labels=labels, resid=resid):
                                continue
                            yes += 1
                            y = K.conv_fwd_bn_in(x, w, b, geom, mean, rstd, scale, offset, 2, relu_in=True, labels=labels, resid=resid)
                            assert K.last_kernel().endswith(',bn>'), (N, C, H, Ko, K.last_kernel())
                            assert tuple(y.shape) == (N, Ko, H, H)
    finally:
        K.X3_HYBRID = hybrid
    assert yes >= (1 if mode is None else 8), yes          # the sweep is not vacuous
