"""Every kernel and every branch of the host planner in csrc/fewch.hip (convs with <= 4 channels on one side), reached through the public conv
entry points of ctgan_amd.kernels.  Each case (a) compares with the fp64 oracle - oracle.tf_ops.conv2d_same / bias_add_nchw, and
torch.autograd.grad of it for the gradients - and (b) asserts the device symbol that ran (K.last_symbol()), so that a planner change which
reroutes a case fails here instead of passing on another kernel.

  A  many -> few forward: row-ring kernel (16- and 32-pixel rows, H != W, partial and short strips, one and three outputs), one-pixel-per-lane
     kernel on a partial tile, band kernel on all four tap cases (odd P, H != W, 64 lanes per pixel, a second trip of the task loop), and both
     sides of the 150 KB LDS guard;
  B  the same kernels as the data gradient of the mirrored few -> many conv (rotated filter, the many index with unit stride);
  C  few -> many forward (KM = 64 / 128 / 256, stride 2, grown and partial bands, NCHW and channels-last image) with its residual / ReLU / mask
     epilogues, as a data gradient with bias, and the batch at which the band has to be capped for its tile to fit;
  D  weight gradients: direct and MFMA kernel per tap case, few_in and few_out, persistent task loops, partial row bands, stride 2, two segments
     whose boundary falls inside a task loop, and result buffers between sentinels;
  E  calls that fewch_handles accepts and the entry point hands back to the GEMM kernels, and the Python mirror of the dispatch predicate.

Tolerances (fp32 FMA against fp64, as test_gpu_kernels.py): 2e-5 forward / data gradient, 3e-5 weight gradient, 1e-6 x max sum|dy| bias gradient,
1e-5 against the forced generic route.  Every figure is printed before it is asserted (pytest -s shows the headroom).
"""
import ctypes
import zlib

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import tf_ops  # noqa: E402


@pytest.fixture(scope='module')
def K():
    """The fp32 family itself: the routing of large layers to the split mode (kernels.X3_HYBRID) is off, as in test_gpu_kernels.py."""
    import ctgan_amd.kernels as K
    old, K.X3_HYBRID = K.X3_HYBRID, False
    yield K
    K.X3_HYBRID = old
    K.debug_m2f_px(True)
    K.debug_force_generic(False)


def dev(t):
    return t.to('cuda')


def cl(t):
    """channels-last copy on device"""
    d = t.to('cuda')
    out = torch.empty((d.shape[0], d.shape[2], d.shape[3], d.shape[1]), device='cuda', dtype=d.dtype).permute(0, 3, 1, 2)
    out.copy_(d)
    return out


def relerr(a, b):
    a = a.detach().cpu().double(); b = b.detach().cpu().double()
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-30)).item()


def gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))      # hash() of a str is per-process random


def close(got, ref, tol, what):
    e = relerr(got, ref)
    print('relerr %-40s %.3e (< %.0e)' % (what, e, tol))
    assert tuple(got.shape) == tuple(ref.shape) and e < tol, (what, e)


def bias_close(db, gy, what):
    scale = gy.double().abs().sum(dim=(0, 2, 3)).max().item()                  # a sum of N(0,1) draws may cancel to ~0
    e = (db.cpu().double() - gy.double().sum(dim=(0, 2, 3))).abs().max().item() / scale
    print('biaserr %-39s %.3e (< 1e-06)' % (what, e))
    assert e < 1e-6, (what, e)


def nchw_strides(n, c, h, w):
    return (c * h * w, h * w, w, 1)


def filt(g, k, C, Ko):
    return torch.randn(k, k, C, Ko, generator=g) / np.sqrt(k * k * C)


class px_off:
    """3x3 many -> few convs on the row-ring kernel instead of the one-pixel-per-lane kernel."""

    def __init__(self, K, on):
        self.K, self.on = K, on

    def __enter__(self):
        if self.on:
            self.K.debug_m2f_px(False)

    def __exit__(self, *a):
        self.K.debug_m2f_px(True)


RING3, RING1, PX3 = 'm2f_ring_kernel<3>', 'm2f_ring_kernel<1>', 'm2f_px_kernel<3>'
BAND = 'm2f_kernel<%d, %d, %d>'
F2M = 'f2m_kernel<%d, %d, %d>'

# ------------------------------------------------------------------------------------------------------------------------------------ A / B
# (N, C, H, W, Ko, k, symbol, px switched off, also as the data gradient of the mirrored conv): what the case reaches
M2F_CASES = [
    (3, 128, 16, 16, 3, 3, RING3, False, True),          # W == 16: one direct load per wave and row; the default kernel there
    (2, 128, 12, 16, 3, 3, RING3, False, False),         # H != W, second strip has 4 rows
    (2, 128, 5, 32, 3, 3, RING3, True, False),           # P < 8: one strip of 5 rows
    (2, 128, 20, 32, 3, 3, RING3, True, True),           # third strip has 4 rows
    (3, 128, 32, 32, 1, 3, RING1, False, True),          # one output: the px kernel has three only
    (3, 128, 16, 16, 1, 3, RING1, False, True),
    (4, 128, 12, 32, 3, 3, PX3, False, True),            # second 8-row tile has 4 rows, no batch norm on load
    (3, 64, 7, 10, 3, 3, BAND % (3, 3, 3), False, True),     # odd P: a one-row last band; 16 lanes per pixel
    (2, 256, 5, 6, 3, 3, BAND % (3, 3, 3), False, True),     # 64 lanes per pixel (4 pixel groups), odd P
    (2, 128, 9, 12, 3, 3, BAND % (3, 3, 3), False, False),   # 128 channels where the ring kernel does not apply (W not 16 / 32)
    (70, 64, 16, 16, 3, 3, BAND % (3, 3, 3), False, False),  # 70 x 8 = 560 tasks on 512 workgroups: a second trip of the task loop
    (3, 64, 14, 14, 1, 5, BAND % (5, 5, 1), False, True),
    (2, 128, 9, 7, 1, 5, BAND % (5, 5, 1), False, True),
    (3, 64, 8, 12, 1, 3, BAND % (3, 3, 1), False, True),
    (3, 128, 6, 10, 3, 1, BAND % (1, 1, 3), False, True),
    (2, 256, 20, 20, 1, 5, BAND % (5, 5, 1), False, False),  # tile 6 x 24 x 256 x 4 = 147 456 B <= 150 KB: the largest launch
    (2, 256, 28, 28, 1, 5, None, False, False),              # 6 x 32 x 256 x 4 = 196 608 B: handed back to the GEMM kernels
]
M2F_IDS = ['N%d_C%d_%dx%d_K%d_k%d%s' % (c[:6] + ('_ring' if c[7] else '',)) for c in M2F_CASES]


@pytest.mark.parametrize('relu_in', [False, True], ids=['plain', 'relu_in'])
@pytest.mark.parametrize('case', M2F_CASES, ids=M2F_IDS)
def test_many_to_few_forward(K, case, relu_in):
    """y = conv(relu?(x), w) + b with the default (channels-last) and an NCHW-strided result."""
    N, C, H, W, Ko, k, sym, off, _ = case
    g = gen('m2f', case)
    geom = K.ConvGeom(C, H, W, Ko, k, k, 1, False)
    assert K.fewch_handles(geom)
    x, w, b = torch.randn(N, C, H, W, generator=g), filt(g, k, C, Ko), torch.randn(Ko, generator=g)
    xin = torch.relu(x.double()) if relu_in else x.double()
    ref = tf_ops.bias_add_nchw(tf_ops.conv2d_same(xin, w.double(), 1), b.double())
    xd, wd, bd = cl(x), dev(w), dev(b)
    with px_off(K, off):
        for strides in (None, nchw_strides(N, Ko, H, W)):
            y = K.conv_fwd(xd, wd, bd, geom, relu_in=relu_in, out_strides=strides)
            if sym is None:
                assert 'fewch' not in K.last_kernel(), K.last_kernel()
            else:
                assert K.last_symbol() == sym and K.last_kernel() == 'fewch_m2f', (K.last_symbol(), K.last_kernel())
            assert (strides is None) or y.is_contiguous()
            close(y, ref, 2e-5, 'fwd ' + str(sym))
        if sym is not None and not relu_in:
            K.debug_force_generic(True)
            try:
                y_gen = K.conv_fwd(xd, wd, bd, geom)
                assert 'fewch' not in K.last_kernel()
            finally:
                K.debug_force_generic(False)
            close(y, y_gen, 1e-5, 'fwd vs generic ' + sym)


@pytest.mark.parametrize('case', [c for c in M2F_CASES if c[8]], ids=[i for i, c in zip(M2F_IDS, M2F_CASES) if c[8]])
def test_many_to_few_as_data_gradient(K, case):
    """dx = conv^T(dy, w) + b of the mirrored few -> many conv (few = Ko of the table, many = C): the same kernels on the rotated filter."""
    N, many, H, W, few, k, sym, off, _ = case
    g = gen('m2f-dgrad', case)
    geom = K.ConvGeom(few, H, W, many, k, k, 1, False)
    assert K.fewch_handles(geom)
    gy, w, b = torch.randn(N, many, H, W, generator=g), filt(g, k, few, many), torch.randn(few, generator=g)
    x_ = torch.zeros(N, few, H, W, dtype=torch.float64, requires_grad=True)
    (ref,) = torch.autograd.grad(tf_ops.conv2d_same(x_, w.double(), 1), x_, gy.double())
    ref = tf_ops.bias_add_nchw(ref, b.double())
    gyd, wd, bd = cl(gy), dev(w), dev(b)
    with px_off(K, off):
        for strides in (None, nchw_strides(N, few, H, W)):
            dx = K.conv_dgrad(gyd, wd, geom, N, out_strides=strides, bias=bd)
            assert K.last_symbol() == sym and K.last_kernel() == 'fewch_m2f(dgrad)', (K.last_symbol(), K.last_kernel())
            close(dx, ref, 2e-5, 'dgrad ' + sym)


# ------------------------------------------------------------------------------------------------------------------------------------ C
# (N, C, H, W, Ko, k, stride, symbol, also with the residual / ReLU / mask epilogues)
F2M_CASES = [
    (3, 3, 6, 9, 256, 3, 1, F2M % (3, 3, 3), True),      # KQ = 64: 4 pixels per pass
    (3, 3, 6, 9, 64, 3, 1, F2M % (3, 3, 3), True),       # KQ = 16: 16 pixels per pass, more than a row
    (3, 3, 9, 7, 128, 3, 2, F2M % (3, 3, 3), False),     # stride 2, P x Q = 5 x 4, pads (1, 1)
    (4, 1, 10, 6, 64, 3, 1, F2M % (3, 3, 1), False),
    (4, 1, 9, 9, 128, 3, 2, F2M % (3, 3, 1), False),
    (3, 3, 5, 8, 128, 1, 1, F2M % (1, 1, 3), False),
    (3, 3, 5, 8, 128, 1, 2, F2M % (1, 1, 3), False),     # stride-2 1x1: no padding at all, P x Q = 3 x 4
    (3, 1, 9, 11, 64, 5, 2, F2M % (5, 5, 1), False),     # the MNIST tap case off the square image, asymmetric pads
    (260, 3, 12, 12, 64, 3, 1, F2M % (3, 3, 3), True),   # pick_band: 8 rows (260 x 2 >= 512), the second band has 4
]
F2M_IDS = ['N%d_C%d_%dx%d_K%d_k%d_s%d' % c[:7] for c in F2M_CASES]


@pytest.mark.parametrize('layout', ['nchw', 'cl'])
@pytest.mark.parametrize('case', F2M_CASES, ids=F2M_IDS)
def test_few_to_many_forward(K, case, layout):
    N, C, H, W, Ko, k, st, sym, epi = case
    g = gen('f2m', case)
    geom = K.ConvGeom(C, H, W, Ko, k, k, st, False)
    assert K.fewch_handles(geom)
    x, w, b = torch.randn(N, C, H, W, generator=g), filt(g, k, C, Ko), torch.randn(Ko, generator=g)
    ref = tf_ops.bias_add_nchw(tf_ops.conv2d_same(x.double(), w.double(), st), b.double())
    xd, wd, bd = (cl(x) if layout == 'cl' else dev(x)), dev(w), dev(b)
    y = K.conv_fwd(xd, wd, bd, geom)
    assert K.last_symbol() == sym and K.last_kernel() == 'fewch_f2m', (K.last_symbol(), K.last_kernel())
    close(y, ref, 2e-5, 'fwd ' + sym)
    if layout == 'nchw':
        K.debug_force_generic(True)
        try:
            y_gen = K.conv_fwd(xd, wd, bd, geom)
            assert 'fewch' not in K.last_kernel()
        finally:
            K.debug_force_generic(False)
        close(y, y_gen, 1e-5, 'fwd vs generic ' + sym)
    if not epi:
        return
    r = torch.randn(ref.shape, generator=g)
    ref_in = tf_ops.bias_add_nchw(tf_ops.conv2d_same(torch.relu(x.double()), w.double(), st), b.double())
    y2 = K.conv_fwd(xd, wd, bd, geom, resid=cl(r), relu=True, relu_in=True)
    assert K.last_symbol() == sym, K.last_symbol()
    close(y2, torch.relu(ref_in + r.double()), 2e-5, 'fwd resid relu relu_in ' + sym)
    # out-mask epilogue: the result kept where mask > 0 == the unmasked launch, then the mask - bit for bit
    m = torch.randn(ref.shape, generator=g)
    md = cl(m)
    y3 = K.conv_fwd(xd, wd, bd, geom, mask=md)
    assert K.last_symbol() == sym, K.last_symbol()
    assert torch.equal(y3, K.lrelu_bwd(y, md, 0.0))
    close(y3, ref * (m > 0), 2e-5, 'fwd mask ' + sym)
    assert 0.3 < (y3 == 0).float().mean().item() < 0.7


@pytest.mark.parametrize('N,C,H,W,Ko,k', [(3, 128, 6, 9, 3, 3), (3, 64, 7, 5, 1, 3), (3, 64, 14, 14, 1, 5), (3, 256, 5, 8, 3, 1)])
def test_few_to_many_as_data_gradient_with_bias(K, N, C, H, W, Ko, k):
    """dx = conv^T(dy, w) + b of a many -> few conv: f2m_kernel with the filter's few index at stride K (the scalar filter loads)."""
    g = gen('f2m-dgrad', N, C, H, W, Ko, k)
    geom = K.ConvGeom(C, H, W, Ko, k, k, 1, False)
    assert K.fewch_handles(geom)
    gy, w, b = torch.randn(N, Ko, H, W, generator=g), filt(g, k, C, Ko), torch.randn(C, generator=g)
    x_ = torch.zeros(N, C, H, W, dtype=torch.float64, requires_grad=True)
    (ref,) = torch.autograd.grad(tf_ops.conv2d_same(x_, w.double(), 1), x_, gy.double())
    ref = tf_ops.bias_add_nchw(ref, b.double())
    for gyd in (dev(gy), cl(gy)):
        dx = K.conv_dgrad(gyd, dev(w), geom, N, bias=dev(b))
        assert K.last_symbol() == F2M % (k, k, Ko) and K.last_kernel() == 'fewch_f2m(dgrad)', (K.last_symbol(), K.last_kernel())
        close(dx, ref, 2e-5, 'dgrad ' + F2M % (k, k, Ko))


def test_few_to_many_band_is_capped_where_the_whole_image_tile_outgrows_lds(K):
    """512 x 3 x 64 x 64 -> 64, 3x3: pick_band alone gives one band of 64 rows, a tile of 3 x 66 x 66 x 4 = 52 272 B.  The launch must succeed on
    f2m_kernel<3, 3, 3>; images 0, 1, 510 and 511 against fp64 (every band of the first and last workgroups)."""
    N, C, H, Ko = 512, 3, 64, 64
    g = gen('f2m-cap')
    geom = K.ConvGeom(C, H, H, Ko, 3, 3, 1, False)
    x, w, b = torch.randn(N, C, H, H, generator=g), filt(g, 3, C, Ko), torch.randn(Ko, generator=g)
    idx = torch.tensor([0, 1, 510, 511])
    ref = tf_ops.bias_add_nchw(tf_ops.conv2d_same(x[idx].double(), w.double(), 1), b.double())
    y = K.conv_fwd(dev(x), dev(w), dev(b), geom)
    torch.cuda.synchronize()
    assert K.last_symbol() == F2M % (3, 3, 3) and K.last_kernel() == 'fewch_f2m', (K.last_symbol(), K.last_kernel())
    close(y[idx.cuda()], ref, 2e-5, 'fwd N=512 64x64 ' + F2M % (3, 3, 3))


# ------------------------------------------------------------------------------------------------------------------------------------ D
DIRECT, MFMA = 'fw_wgrad_kernel<%d, %d, %d>', 'fw_wgrad_mfma_kernel<%d, %d, %d>'
# (N, C, H, W, Ko, k, stride, symbol, row bands per image of the plan)
WGRAD_CASES = [
    (3, 3, 7, 7, 128, 3, 1, DIRECT % (3, 3, 3), 1),      # CM = 128 with an odd row length: the direct kernel
    (3, 3, 7, 8, 128, 3, 1, MFMA % (3, 3, 3), 1),        # band 8 > 7 rows
    (520, 3, 8, 8, 128, 3, 1, MFMA % (3, 3, 3), 1),      # 520 tasks on 512 workgroups
    (260, 3, 8, 8, 64, 3, 1, DIRECT % (3, 3, 3), 1),     # 260 tasks on 256 workgroups
    (3, 128, 12, 10, 3, 3, 1, MFMA % (3, 3, 3), 2),      # few_out; bands of 8 and 4 rows
    (2, 256, 5, 6, 3, 3, 1, DIRECT % (3, 3, 3), 2),      # few_out; 4 lane groups: bands of 4 rows and 1 row
    (3, 1, 10, 6, 64, 3, 1, DIRECT % (3, 3, 1), 1),
    (3, 1, 8, 8, 128, 3, 1, MFMA % (3, 3, 1), 1),
    (3, 64, 8, 12, 1, 3, 1, DIRECT % (3, 3, 1), 1),      # few_out
    (3, 128, 8, 12, 1, 3, 1, MFMA % (3, 3, 1), 1),       # few_out
    (3, 64, 14, 14, 1, 5, 1, DIRECT % (5, 5, 1), 1),     # few_out
    (3, 128, 8, 8, 1, 5, 1, MFMA % (5, 5, 1), 1),        # few_out; 25 of the 31 A rows
    (3, 1, 11, 9, 64, 5, 2, DIRECT % (5, 5, 1), 1),      # few_in, stride 2
    (3, 3, 9, 8, 128, 3, 2, MFMA % (3, 3, 3), 1),        # stride 2: P x Q = 5 x 4
    (3, 3, 9, 10, 128, 3, 2, DIRECT % (3, 3, 3), 1),     # stride 2: P x Q = 5 x 5
    (3, 3, 5, 8, 128, 1, 1, MFMA % (1, 1, 3), 1),
    (3, 3, 5, 7, 64, 1, 1, DIRECT % (1, 1, 3), 1),
    (3, 64, 20, 6, 3, 3, 1, DIRECT % (3, 3, 3), 2),      # few_out, 16 lane groups: bands of 16 and 4 rows
]
WGRAD_IDS = ['N%d_C%d_%dx%d_K%d_k%d_s%d' % c[:7] for c in WGRAD_CASES]


def wgrad_operands(case, g):
    N, C, H, W, Ko, k, st = case[:7]
    x = torch.randn(N, C, H, W, generator=g)
    P, Q = -(-H // st), -(-W // st)
    gy = torch.randn(N, Ko, P, Q, generator=g)
    xd = dev(x) if C <= 4 else cl(x)                      # the few-channel side may be plain NCHW
    gyd = cl(gy) if C <= 4 else dev(gy)
    return x, gy, xd, gyd


def wgrad_ref(x, gy, k, C, Ko, st, relu_x):
    w_ = torch.zeros(k, k, C, Ko, dtype=torch.float64, requires_grad=True)
    xin = torch.relu(x.double()) if relu_x else x.double()
    (gw,) = torch.autograd.grad(tf_ops.conv2d_same(xin, w_, st), w_, gy.double())
    return gw


def plan_bands(K, geom, N, xd, gyd):
    """Row bands per image of the weight gradient's plan: the few-channel workspace is one slab of n_out floats per (image, band)."""
    d = geom.desc(N, xd.stride(), gyd.stride())
    nb = K.lib.ctgan_conv2d_wgrad_multi_workspace_bytes(ctypes.byref(d), 1, (ctypes.c_int32 * 1)(N))
    n_out = geom.R * geom.S * geom.C * geom.K + (geom.K + 3) // 4 * 4
    assert nb % (N * n_out * 4) == 0
    return nb // (N * n_out * 4)


@pytest.mark.parametrize('case', WGRAD_CASES, ids=WGRAD_IDS)
def test_weight_gradient(K, case):
    """dw (and db) with and without the bias gradient and with ReLU on load of x; every launch twice, bit for bit."""
    N, C, H, W, Ko, k, st, sym, bands = case
    g = gen('wgrad', case)
    geom = K.ConvGeom(C, H, W, Ko, k, k, st, False)
    assert K.fewch_handles(geom)
    x, gy, xd, gyd = wgrad_operands(case, g)
    assert plan_bands(K, geom, N, xd, gyd) == bands
    kernel = 'fewch_wgrad(few_in)' if C <= 4 else 'fewch_wgrad(few_out)'
    ref = wgrad_ref(x, gy, k, C, Ko, st, False)
    gw = K.conv_wgrad(xd, gyd, geom)
    assert K.last_symbol() == sym and K.last_kernel() == kernel, (K.last_symbol(), K.last_kernel())
    close(gw, ref, 3e-5, 'wgrad ' + sym)
    assert torch.equal(gw, K.conv_wgrad(xd, gyd, geom))
    gw_b, gb = K.conv_wgrad(xd, gyd, geom, with_bias=True)
    assert K.last_symbol() == sym and K.last_kernel() == kernel, (K.last_symbol(), K.last_kernel())
    close(gw_b, ref, 3e-5, 'wgrad+bias ' + sym)
    bias_close(gb, gy, 'wgrad+bias ' + sym)
    gw_b2, gb2 = K.conv_wgrad(xd, gyd, geom, with_bias=True)
    assert torch.equal(gw_b, gw_b2) and torch.equal(gb, gb2)
    gw_r, gb_r = K.conv_wgrad(xd, gyd, geom, with_bias=True, relu_x=True)
    assert K.last_symbol() == sym, K.last_symbol()
    close(gw_r, wgrad_ref(x, gy, k, C, Ko, st, True), 3e-5, 'wgrad relu_x ' + sym)
    bias_close(gb_r, gy, 'wgrad relu_x ' + sym)
    gw_r2, gb_r2 = K.conv_wgrad(xd, gyd, geom, with_bias=True, relu_x=True)
    assert torch.equal(gw_r, gw_r2) and torch.equal(gb_r, gb_r2)


def test_weight_gradient_two_segments_meet_inside_a_task_loop(K):
    """conv_wgrad_multi on 5 + 520 images of 3 x 8 x 8 -> 128: 525 tasks on 512 workgroups, so workgroups 0 .. 4 take an image of the first
    segment (bias, no ReLU) and then one of the second (ReLU on load, no bias)."""
    C, H, Ko, k = 3, 8, 128, 3
    geom = K.ConvGeom(C, H, H, Ko, k, k, 1, False)
    g = gen('wgrad-2seg')
    segs, sum_w, ref_w = [], 0, 0
    for i, n in enumerate((5, 520)):
        x, gy = torch.randn(n, C, H, H, generator=g), torch.randn(n, Ko, H, H, generator=g)
        relu_x, with_bias = (i == 1), (i == 0)
        segs.append((dev(x), cl(gy), relu_x, with_bias))
        r = K.conv_wgrad(segs[-1][0], segs[-1][1], geom, with_bias=with_bias, relu_x=relu_x)
        sum_w = sum_w + (r[0] if with_bias else r).double()
        ref_w = ref_w + wgrad_ref(x, gy, k, C, Ko, 1, relu_x)
        if with_bias:
            one_b, gy_b = r[1], gy
    dw = torch.empty(k, k, C, Ko, device='cuda'); db = torch.empty(Ko, device='cuda')
    K.conv_wgrad_multi(segs, geom, dw, db)
    assert K.last_symbol() == MFMA % (3, 3, 3) and K.last_kernel() == 'fewch_wgrad(few_in)', (K.last_symbol(), K.last_kernel())
    close(dw, ref_w, 3e-5, 'wgrad two segments ' + MFMA % (3, 3, 3))
    close(dw, sum_w, 1e-5, 'wgrad two segments vs single launches')
    bias_close(db, gy_b, 'wgrad two segments')
    close(db, one_b, 1e-5, 'wgrad two segments bias vs single launch')
    dw2 = torch.empty_like(dw); db2 = torch.empty_like(db)
    K.conv_wgrad_multi(segs, geom, dw2, db2)
    assert torch.equal(dw, dw2) and torch.equal(db, db2)


@pytest.mark.parametrize('case', [WGRAD_CASES[1], WGRAD_CASES[4], WGRAD_CASES[5]], ids=[WGRAD_IDS[1], WGRAD_IDS[4], WGRAD_IDS[5]])
def test_weight_gradient_writes_nothing_outside_dw_and_db(K, case):
    """dw and db as interior slices of sentinel-filled buffers: the slab reduction (whose last column block is partial when the few_out bias
    section of 4 follows the filter) leaves both neighbours of each slice alone - db has 3 elements where the slab has 4."""
    N, C, H, W, Ko, k, st, sym, _ = case
    g = gen('wgrad', case)
    geom = K.ConvGeom(C, H, W, Ko, k, k, st, False)
    x, gy, xd, gyd = wgrad_operands(case, g)
    want_w, want_b = K.conv_wgrad(xd, gyd, geom, with_bias=True)
    n, pad, S = k * k * C * Ko, 64, -12345.0
    for with_bias in (True, False):
        bw = torch.full((n + 2 * pad,), S, device='cuda'); bb = torch.full((Ko + 2 * pad,), S, device='cuda')
        dw, db = bw[pad:pad + n].view(k, k, C, Ko), bb[pad:pad + Ko]
        K.conv_wgrad(xd, gyd, geom, with_bias=with_bias, out=(dw, db if with_bias else None))
        assert K.last_symbol() == sym, K.last_symbol()
        torch.cuda.synchronize()
        assert torch.equal(dw, want_w) and (bw[:pad] == S).all() and (bw[pad + n:] == S).all()
        assert (bb[:pad] == S).all() and (bb[pad + Ko:] == S).all()
        assert torch.equal(db, want_b) if with_bias else (db == S).all()


# ------------------------------------------------------------------------------------------------------------------------------------ E
def offset_cl(t):
    """channels-last copy on device that starts one float into its storage: not 16-byte aligned"""
    n, c, h, w = t.shape
    buf = torch.empty(n * c * h * w + 1, device='cuda')
    out = buf[1:].view(n, h, w, c).permute(0, 3, 1, 2)
    out.copy_(t.to('cuda'))
    assert out.data_ptr() % 16 == 4
    return out


@pytest.mark.parametrize('how', ['nchw', 'misaligned'])
def test_many_to_few_operand_the_direct_kernels_refuse_runs_on_the_gemm_kernels(K, how):
    """3 x 128 x 16 x 16 -> 3, 3x3: fewch_handles says yes, but the wide operand is not channels-last / not 16-byte aligned - forward and the
    mirrored data gradient fall through to the GEMM kernels with the right values."""
    N, C, H, Ko = 3, 128, 16, 3
    g = gen('refuse', how)
    put = dev if how == 'nchw' else offset_cl
    geom = K.ConvGeom(C, H, H, Ko, 3, 3, 1, False)
    assert K.fewch_handles(geom)
    x, w, b = torch.randn(N, C, H, H, generator=g), filt(g, 3, C, Ko), torch.randn(Ko, generator=g)
    ref = tf_ops.bias_add_nchw(tf_ops.conv2d_same(x.double(), w.double(), 1), b.double())
    y = K.conv_fwd(put(x), dev(w), dev(b), geom)
    assert K.last_kernel() and 'fewch' not in K.last_kernel(), K.last_kernel()
    close(y, ref, 2e-5, 'fwd refused (%s) %s' % (how, K.last_kernel()))
    y_ok = K.conv_fwd(cl(x), dev(w), dev(b), geom)
    assert K.last_symbol() == RING3
    close(y, y_ok, 1e-5, 'fwd refused vs ring')
    # data gradient of 3 -> 128 with that dy
    geom2 = K.ConvGeom(Ko, H, H, C, 3, 3, 1, False)
    w2 = filt(g, 3, Ko, C)
    x_ = torch.zeros(N, Ko, H, H, dtype=torch.float64, requires_grad=True)
    (gx_ref,) = torch.autograd.grad(tf_ops.conv2d_same(x_, w2.double(), 1), x_, x.double())
    gx = K.conv_dgrad(put(x), dev(w2), geom2, N)
    assert K.last_kernel() and 'fewch' not in K.last_kernel(), K.last_kernel()
    close(gx, gx_ref, 2e-5, 'dgrad refused (%s) %s' % (how, K.last_kernel()))


@pytest.mark.parametrize('how', ['nchw', 'misaligned'])
def test_weight_gradient_the_direct_kernels_refuse_runs_on_the_gemm_kernels(K, how):
    N, C, H, Ko = 3, 3, 16, 128
    g = gen('refuse-wgrad', how)
    put = dev if how == 'nchw' else offset_cl
    geom = K.ConvGeom(C, H, H, Ko, 3, 3, 1, False)
    assert K.fewch_handles(geom)
    x, gy = torch.randn(N, C, H, H, generator=g), torch.randn(N, Ko, H, H, generator=g)
    gw = K.conv_wgrad(dev(x), put(gy), geom)
    assert K.last_kernel() and 'fewch' not in K.last_kernel(), K.last_kernel()
    close(gw, wgrad_ref(x, gy, 3, C, Ko, 1, False), 3e-5, 'wgrad refused (%s) %s' % (how, K.last_kernel()))


# (C, H, W, Ko, k, stride, x_up): around every edge of ctgan_fewch_handles
MIRROR_CASES = [
    (32, 6, 10, 3, 3, 1, False),      # 8 lanes per pixel would make row16_sum add two pixels together: only many_ok keeps this out
    (64, 6, 10, 3, 3, 1, False), (96, 6, 10, 3, 3, 1, False), (128, 6, 10, 3, 3, 1, False), (256, 6, 10, 3, 3, 1, False),
    (3, 6, 10, 32, 3, 1, False), (3, 6, 10, 64, 3, 1, False), (3, 6, 10, 96, 3, 1, False), (3, 6, 10, 128, 3, 1, False), (3, 6, 10, 256, 3, 1, False),
    (2, 6, 10, 128, 3, 1, False), (128, 6, 10, 2, 3, 1, False),       # 3x3x2
    (4, 6, 10, 128, 3, 1, False), (128, 6, 10, 4, 3, 1, False),       # 3x3x4
    (3, 6, 10, 128, 5, 1, False), (128, 6, 10, 3, 5, 1, False),       # 5x5x3
    (1, 6, 10, 128, 1, 1, False), (128, 6, 10, 1, 1, 1, False),       # 1x1x1
    (1, 6, 10, 64, 5, 1, False), (64, 6, 10, 1, 5, 1, False),         # 5x5x1
    (128, 6, 10, 3, 3, 2, False), (64, 6, 10, 1, 5, 2, False),        # stride 2 on the many -> few side
    (3, 6, 10, 128, 3, 2, False),
    (128, 8, 12, 3, 3, 1, True), (3, 8, 12, 128, 3, 1, True),         # x_up
]


@pytest.mark.parametrize('case', MIRROR_CASES, ids=lambda c: 'C%d_%dx%d_K%d_k%d_s%d%s' % (c[:6] + ('_up' if c[6] else '',)))
def test_python_mirror_of_the_dispatch_predicate(K, case):
    """K.fewch_handles(g) == a direct kernel served an aligned channels-last forward, and either way the values are right."""
    C, H, W, Ko, k, st, up = case
    N = 2
    g = gen('mirror', case)
    geom = K.ConvGeom(C, H, W, Ko, k, k, st, up)
    x = torch.randn(N, C, H // 2, W // 2, generator=g) if up else torch.randn(N, C, H, W, generator=g)
    w, b = filt(g, k, C, Ko), torch.randn(Ko, generator=g)
    xin = tf_ops.upsample2(x.double()) if up else x.double()
    ref = tf_ops.bias_add_nchw(tf_ops.conv2d_same(xin, w.double(), st), b.double())
    y = K.conv_fwd(cl(x), dev(w), dev(b), geom)
    assert K.last_kernel() and K.fewch_handles(geom) == ('fewch' in K.last_kernel()), (K.fewch_handles(geom), K.last_kernel())
    close(y, ref, 2e-5, 'mirror %s' % K.last_kernel())
