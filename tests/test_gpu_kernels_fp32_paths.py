"""Every kernel and every branch of the host planner in csrc/igemm.hip (the fp32 MFMA family: the default route of every conv that the
few-channel and split-mode families do not take), reached through the public conv entry points of ctgan_amd.kernels.  Each case (a) compares
with the fp64 oracle - oracle.tf_ops.conv2d_same / bias_add_nchw / upsample2, and torch.autograd.grad of them for the gradients - and (b)
asserts the device symbol that ran (K.last_symbol()) exactly, so that a planner change which reroutes a case fails here instead of passing on
another kernel.  The expected symbols are written down in the case tables (worked out by hand from the planner's source), not recomputed.

Branch -> test map
  dispatch_fwd_pipe, rows = M * phases * ceil(Ng / 128)                                                 test_pipelined_forward  (FWD_CASES)
    cfg 5   rows <= 2048                     N32 (2048), ragged N2 / N1 5x7, Ng 68, x_up N3, 1x1 N3, 5x5 stride 2
    cfg 10  2048 < rows <= 4096, C % 128     N33 (2112), N64 (4096), ragged 57 x 6x6 / 36 x 6x10, Ng 68, x_up N40, 1x1 N40 (one K slice)
    cfg 11  4096 < rows <= 8192, C % 128     N65 (4160), N128 (8192), ragged 114 x 6x6 / 123 x 5x7
    cfg 4   8192 < rows <= 12288             N129 (8256), N192 (12288); C % 128 != 0 below 8192: N33 C64, ragged 57 / 36 C64, 5x5 stride 2 C64
    cfg 8   12288 < rows <= 24576, C % 64    N193 (12352), 48 x 16x16 K256 (24576, two N tiles), ragged 205 x 6x10 / 199 x 7x9
    cfg 3   fallbacks: C % 64 != 0 of cfg 8 / cfg 4 (N193 C32, N193 C96 K96, N129 C32), C % 128 != 0 of cfg 5 (N20 C64, ragged N1 / N4 C32)
    cfg 2   24576 < rows < 65536             25 x 32x32 (25600), 63 x 32x32 (64512), ragged 46 x 18x30 / 38 x 22x30;  e2 > e1: 80 x 32x32 (81920)
    cfg 1   rows >= 65536 and e1 >= e2       64 x 32x32 (65536), ragged 55 x 30x30 / 59 x 28x30 K256
    every case runs RELU_IN = false (plain, NCHW result: the scalar epilogue) and RELU_IN = true (with residual and ReLU);
    "ragged" = M no multiple of the M tile, once with a grid that is no multiple of 8 (no XCD reorder) and once with one that is.
    cfg 6, 7 and 9 - and with them every KSUB = 2 instantiation - cannot be reached from dispatch_fwd_pipe as written: no case.
  phases > 1 (four-phase data gradient)                                                                 test_phase_mode_data_gradient
    cfg 5 (768), cfg 3 (5x5 taps, K 64), cfg 4 (H != W, partial M and N tiles), cfg 2 (40960), cfg 1 (65536 and 130048),
    the override rows >= 131072 -> cfg 2 (without it e1 = 1 >= e2 = 0.84 picks cfg 1); repack into the workspace and pre-repacked filter
  data-gradient filter forms                                                                            test_stride1_data_gradient
    stride-1 repack (3x3, 1x1, ragged cfg 11) and pre-repacked; the strided view of the original filter with negative tap
    strides (K % 32 != 0 or C % 4 != 0: BVEC = false, table-driven, all three N-tile classes)
  non-phase stride-2 gather (shift / mask, odd H)                                                       test_non_phase_stride2_data_gradient
    pipelined (non-affine loader), the same call forced to the table-driven kernel, and the filter view
  epilogue dropout: in the vector epilogue, and the fallback when run_fwd answers unsupported (NCHW dx)  test_data_gradient_dropout_epilogue_and_its_fallback
  dispatch_fwd_tile: 128x128 (M >= 65536), 64x128 (M >= 24576), 32x128, 64x64, 128x32                   test_table_driven_forward_tiles_and_loaders
    each with the four loader combinations (AVEC x BVEC) on the same values, equal bits;  M = 65535 and M = 24575;     .._just_below_..
    NCHW x, C % 32 != 0, K % 4 != 0                                                                      test_table_driven_forward_generic_operands
  wgrad_plan, vector arm: 128x128 / 64x128 / 64x64 / 32x128 by C and Kg (32768 / 32512, 8192 / 7936); Ng <= 64; Ng <= 32 (128x32 and 32x128)
                                                                                                        test_weight_gradient (WGRAD_CASES)
  wgrad_plan, generic arm: 128x128 / 64x128 / 32x128 by Mtot; 64x64 and 32x128 (Ng <= 64); 128x32 and 32x128 (Ng <= 32)      "
  ctgan_wgrad_split, tiles <= 2: Kg / 384 (N32 32x32 1x1, N200), 256 / tiles (N100 32x32 1x1), floor of 1 (Kg < 384)          "
    (the max_splits cap of that arm can never bind: Kg / 384 <= ceil(Kg / 128))
  ctgan_wgrad_split, loop: fill at k = 2 / 3 / 4, max_splits, exhausted (216 tiles)                                          "
  launch_wgrad_pipe: direct (one split, no bias) against the slab with bias                              N2 128 4x4, N70 1x1 K2048, ...
  launch_splitk_reduce: lanes kernel (splits >= 16, < 65536 float4 columns) against the plain one, equal bits: every case with >= 16 splits;
    16 and 15 splits (N96 / N90 1x1), 28 splits of 73760 columns (N128 C256)
  128x32 tile on the table-driven kernel despite vector operands, unfused bias                           N5 C128 K24
  operands the pipelined kernel refuses (NCHW dy, misaligned x)                                          test_weight_gradient_operands_the_pipelined_kernel_refuses
  result buffers between sentinels                                                                       test_weight_gradient_writes_nothing_outside_dw_and_db
  multi_plan growth loop (splits > target: the chunk grows; planned splits < segments: the loop's second exit)  test_multi_segment_weight_gradient
  igemm_wgrad_pipe_group_kernel, all four tiles                                                          test_grouped_weight_gradient

Out of scope: the < 4 GiB extent fallbacks (not reachable at test sizes); the few-channel, small-linear and 16-bit / split-mode routes (own
modules); CTGAN_B_DIRECT builds.

Tolerances (fp32 FMA against fp64, as test_gpu_kernels.py and test_gpu_fewch_paths.py): 2e-5 forward / data gradient, 3e-5 weight gradient,
1e-6 x max sum|dy| bias gradient, 1e-5 against the forced table-driven route where the summation order differs (WAVES_K > 1), equal bits where
it is the same.  Every figure is printed before it is asserted (pytest -s shows the headroom).
"""
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
    try:
        yield K
    finally:
        K.X3_HYBRID = old
        K.debug_force_generic(False)
        K.lib.ctgan_debug_reduce_lanes(1)


def dev(t):
    return t.to('cuda')


def cl(t):
    """channels-last copy on device"""
    d = t.to('cuda')
    out = torch.empty((d.shape[0], d.shape[2], d.shape[3], d.shape[1]), device='cuda', dtype=d.dtype).permute(0, 3, 1, 2)
    out.copy_(d)
    return out


def offset_cl(t):
    """channels-last copy on device that starts one float into its storage: not 16-byte aligned"""
    n, c, h, w = t.shape
    buf = torch.empty(n * c * h * w + 1, device='cuda')
    out = buf[1:].view(n, h, w, c).permute(0, 3, 1, 2)
    out.copy_(t.to('cuda'))
    assert out.data_ptr() % 16 == 4
    return out


def offset_flat(t):
    """contiguous copy on device that starts one float into its storage"""
    buf = torch.empty(t.numel() + 1, device='cuda')
    out = buf[1:].view(t.shape)
    out.copy_(t.to('cuda'))
    assert out.data_ptr() % 16 == 4 and out.is_contiguous()
    return out


def relerr(a, b):
    a = a.detach().cpu().double(); b = b.detach().cpu().double()
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-30)).item()


def gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))      # hash() of a str is per-process random


def close(got, ref, tol, what):
    e = relerr(got, ref)
    print('relerr %-58s %.3e (< %.0e)' % (what, e, tol))
    assert tuple(got.shape) == tuple(ref.shape) and e < tol, (what, e)


def bias_close(db, gy, what):
    scale = gy.double().abs().sum(dim=(0, 2, 3)).max().item()                  # a sum of N(0,1) draws may cancel to ~0
    e = (db.cpu().double() - gy.double().sum(dim=(0, 2, 3))).abs().max().item() / scale
    print('biaserr %-57s %.3e (< 1e-06)' % (what, e))
    assert tuple(db.shape) == (gy.shape[1],) and e < 1e-6, (what, e)


def nchw_strides(n, c, h, w):
    return (c * h * w, h * w, w, 1)


def filt(g, k, C, Ko):
    return torch.randn(k, k, C, Ko, generator=g) / np.sqrt(k * k * C)


class forced_generic:
    """The table-driven kernels for operands the pipelined ones would take."""

    def __init__(self, K, on=True):
        self.K, self.on = K, on

    def __enter__(self):
        if self.on:
            self.K.debug_force_generic(True)

    def __exit__(self, *a):
        self.K.debug_force_generic(False)


def ran(K, symbol, kernel=None):
    assert K.last_symbol() == symbol, (K.last_symbol(), symbol, K.last_kernel())
    if kernel is not None:
        assert K.last_kernel() == kernel, (K.last_kernel(), kernel)


# igemm_fwd_pipe_kernel<WAVES_M, WAVES_N, WAVES_K, TM, TN, RD, RELU_IN, KSUB> per configuration number of dispatch_fwd_pipe
CFG = {1: '2, 2, 1, 2, 2, 1', 2: '1, 4, 1, 2, 1, 1', 3: '1, 4, 1, 1, 1, 1', 4: '1, 2, 2, 1, 1, 1', 5: '1, 1, 4, 1, 1, 1', 8: '2, 2, 2, 1, 1, 1',
       10: '1, 2, 4, 1, 1, 1', 11: '2, 2, 4, 1, 1, 1'}
# ... and the tile and K-group part of K.last_kernel()
CFG_NAME = {1: '128x128,k1', 2: '64x128,k1', 3: '32x128,k1', 4: '32x64,k2', 5: '32x32,k4', 8: '64x64,k2', 10: '32x64,k4', 11: '64x64,k4'}
SAME_ORDER = (1, 2, 3)              # WAVES_K == 1: the K slices are summed in the table-driven kernel's order


def pipe(cfg, relu_in=False):
    return 'igemm_fwd_pipe_kernel<%s, %s, 1>' % (CFG[cfg], 'true' if relu_in else 'false')


def pipe_name(cfg, relu_in=False, ph4=False):
    return 'igemm_fwd_pipe<%s%s%s>' % (CFG_NAME[cfg], ',relu' if relu_in else '', ',ph4' if ph4 else '')


# <WAVES_M, WAVES_N, TM, TN> of the five tiles (table-driven forward, both weight-gradient kernels, the grouped kernel)
T128x128, T64x128, T32x128, T64x64, T128x32 = '2, 2, 2, 2', '1, 4, 2, 1', '1, 4, 1, 1', '2, 2, 1, 1', '4, 1, 1, 1'
TILE_NAME = {T128x128: '128x128', T64x128: '64x128', T32x128: '32x128', T64x64: '64x64', T128x32: '128x32'}


def table(avec, bvec, tile):
    return 'igemm_fwd_kernel<%s, %s, %s>' % ('true' if avec else 'false', 'true' if bvec else 'false', tile)


def table_name(avec, bvec, tile, ph4=False):
    return 'igemm_fwd<%s,%s,%s%s>' % ('avec' if avec else 'agen', 'bvec' if bvec else 'bgen', TILE_NAME[tile], ',ph4' if ph4 else '')


# ------------------------------------------------------------------------------------------------------------------------------------ A
# (N, C, H, W, Ko, k, stride, x_up, configuration): what the case reaches
FWD_CASES = [
    (32, 128, 8, 8, 128, 3, 1, False, 5),         # rows 2048: the last of cfg 5
    (33, 128, 8, 8, 128, 3, 1, False, 10),        # rows 2112
    (64, 128, 8, 8, 128, 3, 1, False, 10),        # rows 4096
    (65, 128, 8, 8, 128, 3, 1, False, 11),        # rows 4160
    (128, 128, 8, 8, 128, 3, 1, False, 11),       # rows 8192
    (129, 128, 8, 8, 128, 3, 1, False, 4),        # rows 8256
    (192, 128, 8, 8, 128, 3, 1, False, 4),        # rows 12288
    (193, 128, 8, 8, 128, 3, 1, False, 8),        # rows 12352
    (33, 64, 8, 8, 128, 3, 1, False, 4),          # rows 2112, C % 128 != 0
    (20, 64, 8, 8, 128, 3, 1, False, 3),          # rows 1280: cfg 5 falls back to cfg 3 (C % 128 != 0)
    (193, 32, 8, 8, 128, 3, 1, False, 3),         # rows 12352, C % 64 != 0
    (193, 96, 8, 8, 96, 3, 1, False, 3),          # the same with a partial N tile (Ng = 96)
    (129, 32, 8, 8, 128, 3, 1, False, 3),         # rows 8256: cfg 4 falls back to cfg 3 (C % 64 != 0)
    (48, 64, 16, 16, 256, 3, 1, False, 8),        # rows 24576 on two N tiles: the last of cfg 8
    (25, 32, 32, 32, 128, 3, 1, False, 2),        # rows 25600
    (63, 32, 32, 32, 128, 3, 1, False, 2),        # rows 64512: the last below the wave-quantisation choice
    (64, 32, 32, 32, 128, 3, 1, False, 1),        # rows 65536: 512 tiles of 128 rows, e1 = 1
    (80, 32, 32, 32, 128, 3, 1, False, 2),        # rows 81920: 640 tiles of 128 (e1 = 0.625) against 1280 of 64 (e2 = 0.79)
    # M no multiple of the M tile; the grid no multiple of 8 (tiles in launch order), then a multiple of 8 (XCD reorder)
    (2, 128, 5, 7, 128, 3, 1, False, 5),          # M 70, grid 3 x 4 = 12
    (1, 128, 5, 7, 128, 3, 1, False, 5),          # M 35, grid 2 x 4 = 8
    (57, 128, 6, 6, 128, 3, 1, False, 10),        # M 2052, grid 65 x 2 = 130
    (36, 128, 6, 10, 128, 3, 1, False, 10),       # M 2160, grid 68 x 2 = 136
    (114, 128, 6, 6, 128, 3, 1, False, 11),       # M 4104, grid 65 x 2 = 130
    (123, 128, 5, 7, 128, 3, 1, False, 11),       # M 4305, grid 68 x 2 = 136
    (57, 64, 6, 6, 128, 3, 1, False, 4),          # M 2052, grid 130
    (36, 64, 6, 10, 128, 3, 1, False, 4),         # M 2160, grid 136
    (205, 64, 6, 10, 128, 3, 1, False, 8),        # M 12300, grid 193 x 2 = 386
    (199, 64, 7, 9, 128, 3, 1, False, 8),         # M 12537, grid 196 x 2 = 392
    (1, 32, 5, 7, 128, 3, 1, False, 3),           # M 35, grid 2
    (4, 32, 6, 10, 128, 3, 1, False, 3),          # M 240, grid 8
    (46, 32, 18, 30, 128, 3, 1, False, 2),        # M 24840, grid 389
    (38, 32, 22, 30, 128, 3, 1, False, 2),        # M 25080, grid 392
    (55, 32, 30, 30, 256, 3, 1, False, 1),        # M 49500 on two N tiles (rows 99000: e1 = 0.76, e2 = 0.64), grid 387 x 2 = 774
    (59, 32, 28, 30, 256, 3, 1, False, 1),        # M 49560, grid 388 x 2 = 776
    # Ng = 68: one float4 past the first 64 columns (Ng > 64 keeps the launch pipelined)
    (5, 128, 8, 8, 68, 3, 1, False, 5),           # three N tiles of 32, the last with 4 columns; grid 30
    (40, 128, 8, 8, 68, 3, 1, False, 10),         # two N tiles of 64, the second with 4 columns
    # upsampled input: the non-affine loader
    (3, 128, 8, 8, 128, 3, 1, True, 5),
    (40, 128, 8, 8, 128, 3, 1, True, 10),
    # 1x1: one tap; with four K groups of 32 the whole K extent is ONE slice (no steady state of the pipeline)
    (3, 128, 8, 8, 128, 1, 1, False, 5),
    (40, 128, 8, 8, 128, 1, 1, False, 10),
    # 5x5 stride 2 on 7 x 8: P x Q = 4 x 4, pads (2, 2) on the odd extent and (1, 2) on the even one
    (40, 128, 7, 8, 128, 5, 2, False, 5),
    (200, 64, 7, 8, 128, 5, 2, False, 4),
]
FWD_IDS = ['N%d_C%d_%dx%d_K%d_k%d_s%d%s_cfg%d' % (c[:7] + ('_up' if c[7] else '', c[8])) for c in FWD_CASES]


@pytest.mark.parametrize('case', FWD_CASES, ids=FWD_IDS)
def test_pipelined_forward(K, case):
    """y = conv(x, w) + b on the channels-last result (vector epilogue) and on an NCHW one (scalar epilogue), relu(conv(relu(x), w) + b + r)
    on the RELU_IN instantiation - and the same call on the table-driven kernel."""
    N, C, H, W, Ko, k, st, up, cfg = case
    g = gen('fwd', case)
    geom = K.ConvGeom(C, H, W, Ko, k, k, st, up)
    x = torch.randn(N, C, H // 2, W // 2, generator=g) if up else torch.randn(N, C, H, W, generator=g)
    w, b = filt(g, k, C, Ko), torch.randn(Ko, generator=g)
    xin = tf_ops.upsample2(x.double()) if up else x.double()
    ref = tf_ops.bias_add_nchw(tf_ops.conv2d_same(xin, w.double(), st), b.double())
    r = torch.randn(ref.shape, generator=g)
    ref_r = torch.relu(tf_ops.bias_add_nchw(tf_ops.conv2d_same(torch.relu(xin), w.double(), st), b.double()) + r.double())
    xd, wd, bd, rd = cl(x), dev(w), dev(b), cl(r)
    y = K.conv_fwd(xd, wd, bd, geom)
    ran(K, pipe(cfg), pipe_name(cfg))
    close(y, ref, 2e-5, 'fwd ' + pipe(cfg))
    y_r = K.conv_fwd(xd, wd, bd, geom, resid=rd, relu=True, relu_in=True)
    ran(K, pipe(cfg, True), pipe_name(cfg, True))
    close(y_r, ref_r, 2e-5, 'fwd relu_in resid relu ' + pipe(cfg, True))
    y_n = K.conv_fwd(xd, wd, bd, geom, out_strides=nchw_strides(N, Ko, geom.P, geom.Q))
    ran(K, pipe(cfg), pipe_name(cfg))
    assert y_n.is_contiguous()
    close(y_n, ref, 2e-5, 'fwd NCHW result ' + pipe(cfg))
    assert torch.equal(y_n, y)                        # the two epilogues store the same sums
    with forced_generic(K):
        y_g = K.conv_fwd(xd, wd, bd, geom)
        assert K.last_symbol().startswith('igemm_fwd_kernel<true, true, '), K.last_symbol()
    if cfg in SAME_ORDER:
        assert torch.equal(y, y_g), cfg
    else:
        close(y, y_g, 1e-5, 'fwd vs table-driven ' + pipe(cfg))


# ------------------------------------------------------------------------------------------------------------------------------------ B
# (N, C_in, H, W, Ko, k, configuration, every variant?): H x W = the size of dx; rows = N * (H / 2) * (W / 2) * 4 * ceil(C_in / 128)
PHASE_CASES = [
    (3, 128, 16, 16, 128, 4, 5, True),            # rows 768
    (3, 128, 16, 16, 64, 5, 3, True),             # 5x5: phases of 3 and 2 taps, zero padded; 64 dy channels: cfg 5 falls back to cfg 3
    (70, 96, 8, 12, 64, 4, 4, True),              # H != W; rows 6720: cfg 11 -> cfg 4 (64 dy channels); M 1680 per phase = 52.5 tiles, Ng 96 = 1.5
    (40, 128, 32, 32, 32, 4, 2, False),           # rows 40960
    (64, 128, 32, 32, 32, 4, 1, False),           # rows 65536: e1 = 1
    (127, 128, 32, 32, 32, 4, 1, False),          # rows 130048: e1 = 0.99 >= e2 = 0.84, the last below the override
    (128, 128, 32, 32, 32, 4, 2, False),          # rows 131072: e1 = 1 >= e2 = 0.84 would pick cfg 1; the override
]
PHASE_IDS = ['N%d_C%d_%dx%d_K%d_k%d_cfg%d' % c[:7] for c in PHASE_CASES]


def dgrad_ref(gy, w, N, C, H, W, st):
    x_ = torch.zeros(N, C, H, W, dtype=torch.float64, requires_grad=True)
    (ref,) = torch.autograd.grad(tf_ops.conv2d_same(x_, w.double(), st), x_, gy.double())
    return ref


def dgrad_epilogue_operands(g, ref):
    C = ref.shape[1]
    b, m, r = torch.randn(C, generator=g), torch.randn(ref.shape, generator=g), torch.randn(ref.shape, generator=g)
    ref_e = torch.where(m.double() > 0, ref + b.double().view(1, -1, 1, 1), torch.zeros_like(ref)) + r.double()
    return dev(b), cl(m), cl(r), ref_e


@pytest.mark.parametrize('case', PHASE_CASES, ids=PHASE_IDS)
def test_phase_mode_data_gradient(K, case):
    """Stride-2 data gradient as four stride-1 convs of dy in one launch: the filter repacked per call into the workspace, pre-repacked
    (equal bits), with the bias / mask / residual epilogue, and onto an NCHW dx (the scalar epilogue with the phase offsets)."""
    N, C, H, W, Ko, k, cfg, full = case
    g = gen('phase', case)
    geom = K.ConvGeom(C, H, W, Ko, k, k, 2, False)
    gy, w = torch.randn(N, Ko, H // 2, W // 2, generator=g), filt(g, k, C, Ko)
    ref = dgrad_ref(gy, w, N, C, H, W, 2)
    gyd, wd = cl(gy), dev(w)
    dx = K.conv_dgrad(gyd, wd, geom, N)
    ran(K, pipe(cfg), pipe_name(cfg, ph4=True))
    close(dx, ref, 2e-5, 'dgrad ph4 ' + pipe(cfg))
    bd, md, rd, ref_e = dgrad_epilogue_operands(g, ref)
    dx_e = K.conv_dgrad(gyd, wd, geom, N, bias=bd, mask=md, resid=rd)
    ran(K, pipe(cfg), pipe_name(cfg, ph4=True))
    close(dx_e, ref_e, 2e-5, 'dgrad ph4 bias mask resid ' + pipe(cfg))
    if not full:
        return
    wt = K.repack_filter(wd, geom)
    dx_p = K.conv_dgrad(gyd, wd, geom, N, wt=wt)
    ran(K, pipe(cfg), pipe_name(cfg, ph4=True))
    assert torch.equal(dx_p, dx)
    dx_n = K.conv_dgrad(gyd, wd, geom, N, out_strides=nchw_strides(N, C, H, W))
    ran(K, pipe(cfg), pipe_name(cfg, ph4=True))
    assert dx_n.is_contiguous() and torch.equal(dx_n, dx)
    with forced_generic(K):
        dx_g = K.conv_dgrad(gyd, wd, geom, N)
        assert K.last_symbol().startswith('igemm_fwd_kernel<true, true, ') and K.last_kernel().endswith(',ph4>'), (K.last_symbol(), K.last_kernel())
    if cfg in SAME_ORDER:
        assert torch.equal(dx, dx_g)
    else:
        close(dx, dx_g, 1e-5, 'dgrad ph4 vs table-driven ' + pipe(cfg))


# (N, C_in, H, W, Ko, k, symbol, kernel name): stride-1 data gradients; the filter repacked (C_in % 4 == 0 and Ko % 32 == 0) or viewed in place
STRIDE1_CASES = [
    (5, 128, 8, 8, 128, 3, pipe(5), pipe_name(5)),
    (5, 96, 8, 8, 64, 1, pipe(3), pipe_name(3)),                                          # 1x1; 64 dy channels: cfg 5 falls back to cfg 3
    (70, 128, 6, 10, 128, 3, pipe(11), pipe_name(11)),                                    # M 4200 = 65.6 tiles, grid 132
    (7, 40, 6, 5, 24, 3, table(False, False, T64x64), table_name(False, False, T64x64)),  # Ko % 32 != 0: the view; nothing aligned
    (5, 42, 6, 5, 64, 3, table(True, False, T64x64), table_name(True, False, T64x64)),    # C_in % 4 != 0: the view under a vector dy loader
    (5, 70, 6, 5, 24, 3, table(False, False, T32x128), table_name(False, False, T32x128)),
    (5, 24, 6, 5, 40, 3, table(False, False, T128x32), table_name(False, False, T128x32)),
]
STRIDE1_IDS = ['N%d_C%d_%dx%d_K%d_k%d' % c[:6] for c in STRIDE1_CASES]


@pytest.mark.parametrize('case', STRIDE1_CASES, ids=STRIDE1_IDS)
def test_stride1_data_gradient(K, case):
    N, C, H, W, Ko, k, sym, name = case
    g = gen('dgrad1', case[:6])
    geom = K.ConvGeom(C, H, W, Ko, k, k, 1, False)
    assert not K.fewch_handles(geom)
    gy, w = torch.randn(N, Ko, H, W, generator=g), filt(g, k, C, Ko)
    ref = dgrad_ref(gy, w, N, C, H, W, 1)
    gyd, wd = cl(gy), dev(w)
    dx = K.conv_dgrad(gyd, wd, geom, N)
    ran(K, sym, name)
    close(dx, ref, 2e-5, 'dgrad ' + sym)
    bd, md, rd, ref_e = dgrad_epilogue_operands(g, ref)
    dx_e = K.conv_dgrad(gyd, wd, geom, N, bias=bd, mask=md, resid=rd)
    ran(K, sym, name)
    close(dx_e, ref_e, 2e-5, 'dgrad bias mask resid ' + sym)
    dx_n = K.conv_dgrad(gyd, wd, geom, N, out_strides=nchw_strides(N, C, H, W))
    ran(K, sym, name)
    assert dx_n.is_contiguous() and torch.equal(dx_n, dx)
    if K.dgrad_wants_repack(geom):
        dx_p = K.conv_dgrad(gyd, wd, geom, N, wt=K.repack_filter(wd, geom))
        ran(K, sym, name)
        assert torch.equal(dx_p, dx)
    else:
        assert 'pipe' not in name              # the view has no unit stride over the GEMM's N index: never pipelined


def test_non_phase_stride2_data_gradient(K):
    """5x5 stride 2 onto 7 x 8 (odd H: no phase mode): rows enumerate the dx pixels and every tap reads dy[(i - pad + r) / 2] where that is
    whole - the shift / mask gather - on the pipelined kernel, on the table-driven one with the same repacked filter, and with the filter view."""
    N, C, H, W, Ko, k = 6, 128, 7, 8, 128, 5
    g = gen('dgrad-s2-odd')
    geom = K.ConvGeom(C, H, W, Ko, k, k, 2, False)
    gy, w = torch.randn(N, Ko, geom.P, geom.Q, generator=g), filt(g, k, C, Ko)
    ref = dgrad_ref(gy, w, N, C, H, W, 2)
    gyd, wd = cl(gy), dev(w)
    dx = K.conv_dgrad(gyd, wd, geom, N)
    ran(K, pipe(5), pipe_name(5))                 # M 336, no ',ph4'
    close(dx, ref, 2e-5, 'dgrad stride 2 odd ' + pipe(5))
    bd, md, rd, ref_e = dgrad_epilogue_operands(g, ref)
    close(K.conv_dgrad(gyd, wd, geom, N, bias=bd, mask=md, resid=rd), ref_e, 2e-5, 'dgrad stride 2 odd bias mask resid')
    assert torch.equal(K.conv_dgrad(gyd, wd, geom, N, wt=K.repack_filter(wd, geom)), dx)
    with forced_generic(K):
        dx_g = K.conv_dgrad(gyd, wd, geom, N)
        ran(K, table(True, True, T32x128), table_name(True, True, T32x128))
    close(dx_g, ref, 2e-5, 'dgrad stride 2 odd ' + table(True, True, T32x128))
    close(dx, dx_g, 1e-5, 'dgrad stride 2 odd vs table-driven')
    # nothing aligned: the gather and the filter view together
    N, C, Ko = 7, 40, 24
    geom = K.ConvGeom(C, H, W, Ko, k, k, 2, False)
    gy, w = torch.randn(N, Ko, geom.P, geom.Q, generator=g), filt(g, k, C, Ko)
    dx = K.conv_dgrad(cl(gy), dev(w), geom, N)
    ran(K, table(False, False, T64x64), table_name(False, False, T64x64))
    close(dx, dgrad_ref(gy, w, N, C, H, W, 2), 2e-5, 'dgrad stride 2 odd ' + table(False, False, T64x64))


def test_data_gradient_dropout_epilogue_and_its_fallback(K):
    """conv_dgrad(drop=...) == dropout_rng(conv_dgrad(...)) bit for bit: inside the vector epilogue of the pipelined kernel, and - an NCHW dx
    has no vector epilogue, run_fwd answers unsupported - as the separate pass kernels.py falls back to."""
    N, C, H, W, Ko, k = 5, 128, 8, 8, 128, 3
    g = gen('dgrad-drop')
    geom = K.ConvGeom(C, H, W, Ko, k, k, 1, False)
    gy, w = torch.randn(N, Ko, H, W, generator=g), filt(g, k, C, Ko)
    ref = dgrad_ref(gy, w, N, C, H, W, 1)
    gyd, wd = cl(gy), dev(w)
    keep = 0.8
    drop = (keep, 77, 3, torch.full((1,), 5, dtype=torch.int64, device='cuda'))
    for strides in (None, nchw_strides(N, C, H, W)):
        plain = K.conv_dgrad(gyd, wd, geom, N, out_strides=strides)
        ran(K, pipe(5), pipe_name(5))
        want = K.dropout_rng(plain, *drop)
        got = K.conv_dgrad(gyd, wd, geom, N, out_strides=strides, drop=drop)
        ran(K, pipe(5), pipe_name(5))
        assert got.stride() == plain.stride() and torch.equal(got, want)
        kept = (got != 0).cpu()
        frac = kept.double().mean().item()
        print('kept %.4f of %d' % (frac, kept.numel()))
        assert abs(frac - keep) < 0.02
        close(got.cpu().double() * keep, ref * kept, 2e-5, 'dgrad dropout ' + ('NCHW fallback' if strides else 'vector epilogue'))


def test_null_ext_and_an_ext_with_nothing_on_take_the_same_path(K):
    """ctgan_conv2d_fwd / ctgan_conv2d_dgrad with ext = NULL and with an ext that switches nothing on: the same kernel and the same bits.  (The
    entry points that took no ext used to forward NULL to these; one entry per operation leaves the equivalence to this test.)"""
    import ctypes
    from ctgan_amd._lib import EpilogueExt
    N, C, H, W, Ko, k = 2, 32, 8, 8, 32, 3
    g = gen('null-ext')
    geom = K.ConvGeom(C, H, W, Ko, k, k, 1, False)
    x, gy, w = cl(torch.randn(N, C, H, W, generator=g)), cl(torch.randn(N, Ko, H, W, generator=g)), dev(filt(g, k, C, Ko))
    d = geom.desc(N, x.stride(), gy.stride())
    ws = torch.empty(K.lib.ctgan_conv2d_workspace_bytes(ctypes.byref(d), 1), dtype=torch.uint8, device='cuda')
    p, st, runs = K._ptr, K._stream(), []
    for fill, e in ((1.0, None), (2.0, EpilogueExt(0.0, 0, 0, None))):
        ext = None if e is None else ctypes.byref(e)
        y, dx = K.empty_cl(N, Ko, H, W, x.device).fill_(fill), K.empty_cl(N, C, H, W, x.device).fill_(fill)
        K.check(K.lib.ctgan_conv2d_fwd(ctypes.byref(d), p(x), p(w), None, None, p(y), 0, ext, st), 'conv2d_fwd')
        sym_fwd = K.last_symbol()
        K.check(K.lib.ctgan_conv2d_dgrad(ctypes.byref(d), p(gy), p(w), None, None, None, p(dx), p(ws), ws.numel(), 0, ext, st), 'conv2d_dgrad')
        runs.append((y, sym_fwd, dx, K.last_symbol()))
    (y0, sf0, dx0, sd0), (y1, sf1, dx1, sd1) = runs
    print('fwd %s | dgrad %s' % (sf0, sd0))
    assert sf0 == sf1 and sd0 == sd1 and sf0 and sd0
    assert torch.equal(y0, y1) and torch.equal(dx0, dx1)


# ------------------------------------------------------------------------------------------------------------------------------------ C
# (N, C, H, W, Ko, k, tile): C % 32 == 0 and Ko % 4 == 0, so that every loader combination can run the same values
TILE_CASES = [
    (64, 32, 32, 32, 128, 3, T128x128),           # M 65536
    (24, 32, 32, 32, 128, 3, T64x128),            # M 24576
    (3, 32, 6, 10, 128, 3, T32x128),              # M 180: 5.6 tiles
    (5, 32, 6, 10, 40, 3, T64x64),                # 32 < Ng <= 64: pipelined never; M 300 = 4.7 tiles, Ng 40 of 64
    (5, 32, 6, 10, 24, 3, T128x32),               # Ng <= 32 with Ko > 4 (the few-channel family declines); M 300 = 2.3 tiles
]
TILE_IDS = ['N%d_C%d_%dx%d_K%d_%s' % (c[:5] + (TILE_NAME[c[6]],)) for c in TILE_CASES]


@pytest.mark.parametrize('case', TILE_CASES, ids=TILE_IDS)
def test_table_driven_forward_tiles_and_loaders(K, case):
    """The vector loaders only change how tiles reach LDS: with x and / or w one float off 16-byte alignment the scalar gathers run the same
    tile on the same values - equal bits in all four combinations."""
    N, C, H, W, Ko, k, tile = case
    g = gen('tile', case)
    geom = K.ConvGeom(C, H, W, Ko, k, k, 1, False)
    assert not K.fewch_handles(geom)
    x, w, b = torch.randn(N, C, H, W, generator=g), filt(g, k, C, Ko), torch.randn(Ko, generator=g)
    ref = tf_ops.bias_add_nchw(tf_ops.conv2d_same(x.double(), w.double(), 1), b.double())
    r = torch.randn(ref.shape, generator=g)
    ref_r = torch.relu(tf_ops.bias_add_nchw(tf_ops.conv2d_same(torch.relu(x.double()), w.double(), 1), b.double()) + r.double())
    bd, rd = dev(b), cl(r)
    y0 = yr0 = None
    for avec in (True, False):
        for bvec in (True, False):
            xd = cl(x) if avec else offset_cl(x)
            wd = dev(w) if bvec else offset_flat(w)
            sym, name = table(avec, bvec, tile), table_name(avec, bvec, tile)
            with forced_generic(K, avec and bvec and Ko > 64):        # (Ng <= 64 is the table-driven kernel's by default)
                y = K.conv_fwd(xd, wd, bd, geom)
                ran(K, sym, name)
                y_r = K.conv_fwd(xd, wd, bd, geom, resid=rd, relu=True, relu_in=True)
                ran(K, sym, name)
                y_n = K.conv_fwd(xd, wd, bd, geom, out_strides=nchw_strides(N, Ko, H, W))
                ran(K, sym, name)
            if y0 is None:
                y0, yr0 = y, y_r
                close(y, ref, 2e-5, 'fwd ' + sym)
                close(y_r, ref_r, 2e-5, 'fwd relu_in resid relu ' + sym)
            assert torch.equal(y, y0) and torch.equal(y_r, yr0) and torch.equal(y_n, y0), sym


@pytest.mark.parametrize('N,H,W,tile', [(257, 15, 17, T64x128), (983, 5, 5, T32x128)], ids=['M65535', 'M24575'])
def test_table_driven_forward_just_below_the_tile_thresholds(K, N, H, W, tile):
    C, Ko, k = 32, 128, 3
    g = gen('tile-below', N, H, W)
    geom = K.ConvGeom(C, H, W, Ko, k, k, 1, False)
    x, w, b = torch.randn(N, C, H, W, generator=g), filt(g, k, C, Ko), torch.randn(Ko, generator=g)
    ref = tf_ops.bias_add_nchw(tf_ops.conv2d_same(x.double(), w.double(), 1), b.double())
    with forced_generic(K):
        y = K.conv_fwd(cl(x), dev(w), dev(b), geom)
        ran(K, table(True, True, tile), table_name(True, True, tile))
    close(y, ref, 2e-5, 'fwd M = %d %s' % (N * H * W, table(True, True, tile)))


# (N, C, H, W, Ko, k, layout of x, AVEC, BVEC, tile)
GENERIC_CASES = [
    (7, 40, 6, 5, 24, 3, 'cl', False, False, T128x32),        # C % 32 != 0, and the filter one float off 16-byte alignment
    (5, 20, 6, 10, 70, 3, 'nchw', False, False, T32x128),     # C % 32 != 0 and Ko % 4 != 0
    (5, 32, 6, 10, 42, 3, 'cl', True, False, T64x64),         # Ko % 4 != 0 alone
    (5, 20, 6, 10, 64, 3, 'cl', False, True, T64x64),         # C % 32 != 0 alone
    (5, 32, 6, 10, 128, 3, 'nchw', False, True, T32x128),     # an NCHW x: the channel stride is not 1
    (24, 20, 32, 32, 70, 3, 'nchw', False, False, T64x128),   # M 24576
    (64, 20, 32, 32, 70, 3, 'nchw', False, False, T128x128),  # M 65536
]
GENERIC_IDS = ['N%d_C%d_%dx%d_K%d_%s_%s' % (c[:5] + (c[6], TILE_NAME[c[9]])) for c in GENERIC_CASES]


@pytest.mark.parametrize('case', GENERIC_CASES, ids=GENERIC_IDS)
def test_table_driven_forward_generic_operands(K, case):
    N, C, H, W, Ko, k, layout, avec, bvec, tile = case
    g = gen('generic', case)
    geom = K.ConvGeom(C, H, W, Ko, k, k, 1, False)
    assert not K.fewch_handles(geom)
    x, w, b = torch.randn(N, C, H, W, generator=g), filt(g, k, C, Ko), torch.randn(Ko, generator=g)
    ref = tf_ops.bias_add_nchw(tf_ops.conv2d_same(x.double(), w.double(), 1), b.double())
    r = torch.randn(ref.shape, generator=g)
    ref_r = torch.relu(tf_ops.bias_add_nchw(tf_ops.conv2d_same(torch.relu(x.double()), w.double(), 1), b.double()) + r.double())
    xd = cl(x) if layout == 'cl' else dev(x)
    wd = dev(w) if (bvec or Ko % 4) else offset_flat(w)
    sym, name = table(avec, bvec, tile), table_name(avec, bvec, tile)
    y = K.conv_fwd(xd, wd, dev(b), geom)
    ran(K, sym, name)
    close(y, ref, 2e-5, 'fwd ' + sym)
    y_r = K.conv_fwd(xd, wd, dev(b), geom, resid=cl(r), relu=True, relu_in=True)
    ran(K, sym, name)
    close(y_r, ref_r, 2e-5, 'fwd relu_in resid relu ' + sym)
    y_n = K.conv_fwd(xd, wd, dev(b), geom, out_strides=nchw_strides(N, Ko, H, W))
    ran(K, sym, name)
    assert y_n.is_contiguous() and torch.equal(y_n, y)


# ------------------------------------------------------------------------------------------------------------------------------------ D
WPIPE, WTABLE, WGROUP = 'igemm_wgrad_pipe_kernel<%s>', 'igemm_wgrad_kernel<%s, %s, %s>', 'igemm_wgrad_pipe_group_kernel<%s>'
VV, GV = 'avec,bvec', 'agen,bvec'
# (N, C, H, W, Ko, k, stride, x_up, pipelined kernel or the table-driven kernel's loaders, tile, splits): tiles, chunk and what the case reaches
WGRAD_CASES = [
    (128, 128, 16, 16, 128, 3, 1, False, 'pipe', T128x128, 54),   # 9 tiles, chunk 608: the loop fills at k = 2; lanes reduction
    (32, 64, 16, 16, 128, 3, 1, False, 'pipe', T64x128, 52),      # Kg 8192: the first of 64x128; 9 tiles, chunk 160
    (31, 64, 16, 16, 128, 3, 1, False, 'pipe', T64x64, 28),       # Kg 7936: 18 tiles, chunk 288, the last split has 160 of 288 rows
    (5, 96, 8, 8, 128, 3, 1, False, 'pipe', T32x128, 3),          # C % 64 != 0; 27 tiles, max_splits ends the loop at k = 2; plain reduction
    (5, 64, 8, 8, 64, 3, 1, False, 'pipe', T64x64, 3),            # 32 < Ng <= 64
    (5, 96, 8, 8, 64, 3, 1, False, 'pipe', T32x128, 3),           # 32 < Ng <= 64 with C % 64 != 0: the N tile twice as wide as Ng
    (5, 96, 8, 8, 40, 3, 1, False, 'pipe', T32x128, 3),           # N tile wider than Ng
    (5, 96, 8, 8, 24, 3, 1, False, 'pipe', T32x128, 3),           # Ng <= 32 with C % 128 != 0
    (5, 128, 8, 8, 24, 3, 1, False, VV, T128x32, 3),              # the 128x32 tile: table-driven despite vector operands; bias by column sums
    (2, 128, 4, 4, 128, 3, 1, False, 'pipe', T64x64, 1),          # Kg 32: one split - straight into dw, through the slab with bias
    (32, 128, 32, 32, 128, 1, 1, False, 'pipe', T128x128, 79),    # one tile: 32768 / 384 = 85 splits asked, chunk 416 gives 79
    (200, 64, 8, 8, 128, 1, 1, False, 'pipe', T64x128, 31),       # one tile: 12800 / 384 = 33 asked, chunk 416 gives 31
    (100, 128, 32, 32, 128, 1, 1, False, 'pipe', T128x128, 247),  # one tile: 102400 / 384 = 266 capped at 256, chunk 416 gives 247
    (2, 64, 8, 8, 128, 1, 1, False, 'pipe', T64x64, 1),           # two tiles, Kg 128 < 384: the floor of 1
    (70, 128, 1, 1, 2048, 1, 1, False, 'pipe', T64x64, 1),        # linear layer, 64 tiles: max_splits = 1 ends the loop
    (32, 128, 8, 8, 320, 3, 1, False, 'pipe', T64x64, 8),         # 90 tiles: 5 splits at k = 2 (450 < 461), fills at k = 3 with 8; chunk 256
    (32, 160, 8, 8, 320, 3, 1, False, 'pipe', T32x128, 7),        # 135 tiles: 3 (405), 5 (675 < 691), fills at k = 4 with 7 (945 >= 922); chunk 320
    (32, 192, 8, 8, 512, 3, 1, False, 'pipe', T64x64, 4),         # 216 tiles: 2 (432), 3 (648), 4 (864 < 922): the loop runs out; chunk 512
    (7, 40, 6, 6, 96, 3, 1, False, GV, T128x128, 2),              # generic arm, Mtot 360 > 64: 2.8 x 0.75 tiles
    (7, 40, 6, 6, 48, 3, 1, False, GV, T64x64, 2),
    (7, 40, 6, 6, 24, 3, 1, False, GV, T128x32, 2),
    (3, 40, 4, 4, 96, 1, 1, False, GV, T64x128, 1),               # Mtot 40 <= 64
    (3, 20, 4, 4, 96, 1, 1, False, GV, T32x128, 1),               # Mtot 20 <= 32
    (3, 20, 4, 4, 48, 1, 1, False, GV, T32x128, 1),               # ... with Ng <= 64
    (3, 20, 4, 4, 24, 1, 1, False, GV, T32x128, 1),               # ... with Ng <= 32
    (6, 128, 16, 16, 128, 4, 2, False, 'pipe', T64x64, 3),        # stride 2, pads (1, 1): 64 tiles, Kg 384
    (6, 64, 7, 8, 128, 5, 2, False, 'pipe', T64x64, 1),           # stride 2 on 7 x 8, pads (2, 1): 50 tiles, Kg 96
    (4, 128, 8, 8, 128, 3, 1, True, 'pipe', T64x64, 2),           # x read through the 2x upsample
    (127, 128, 16, 16, 128, 3, 1, False, 'pipe', T64x128, 28),    # Kg 32512: the last of 64x128 for C % 128 == 0; 18 tiles, chunk 1184
    (128, 256, 16, 16, 128, 3, 1, False, 'pipe', T128x128, 28),   # 18 tiles; 28 slabs of 73760 float4 columns (>= 65536): the plain reduction
    (96, 64, 8, 8, 128, 1, 1, False, 'pipe', T64x64, 16),         # two tiles, Kg 6144 = 16 x 384: the first split count of the lanes reduction
    (90, 64, 8, 8, 128, 1, 1, False, 'pipe', T64x64, 15),         # Kg 5760 = 15 x 384: the last of the plain one
]
WGRAD_IDS = ['N%d_C%d_%dx%d_K%d_k%d_s%d%s' % (c[:7] + ('_up' if c[7] else '',)) for c in WGRAD_CASES]


def wgrad_names(how, tile, splits):
    if how == 'pipe':
        return WPIPE % tile, 'igemm_wgrad_pipe<%s,split%d>' % (TILE_NAME[tile], splits), 'igemm_wgrad_pipe<%s,split%d,bias>' % (TILE_NAME[tile], splits)
    a, b = how.split(',')
    name = 'igemm_wgrad<%s,%s,split%d>' % (how, TILE_NAME[tile], splits)
    return WTABLE % ('true' if a == 'avec' else 'false', 'true' if b == 'bvec' else 'false', tile), name, name


def wgrad_operands(case, g):
    N, C, H, W, Ko, k, st, up = case[:8]
    x = torch.randn(N, C, H // 2, W // 2, generator=g) if up else torch.randn(N, C, H, W, generator=g)
    gy = torch.randn(N, Ko, -(-H // st), -(-W // st), generator=g)
    return x, gy


def wgrad_ref(x, gy, k, C, Ko, st, relu_x, up=False):
    w_ = torch.zeros(k, k, C, Ko, dtype=torch.float64, requires_grad=True)
    xin = tf_ops.upsample2(x.double()) if up else x.double()
    xin = torch.relu(xin) if relu_x else xin
    (gw,) = torch.autograd.grad(tf_ops.conv2d_same(xin, w_, st), w_, gy.double())
    return gw


@pytest.mark.parametrize('case', WGRAD_CASES, ids=WGRAD_IDS)
def test_weight_gradient(K, case):
    """dw without and with the bias gradient (the bias row does not perturb the weights), with ReLU on load of x, and - where the slabs are
    summed by the lanes kernel - the plain reduction on the same slabs, bit for bit."""
    N, C, H, W, Ko, k, st, up, how, tile, splits = case
    g = gen('wgrad', case[:8])
    geom = K.ConvGeom(C, H, W, Ko, k, k, st, up)
    assert not K.fewch_handles(geom)
    sym, name, name_b = wgrad_names(how, tile, splits)
    x, gy = wgrad_operands(case, g)
    xd, gyd = cl(x), cl(gy)
    ref = wgrad_ref(x, gy, k, C, Ko, st, False, up)
    dw = K.conv_wgrad(xd, gyd, geom)
    ran(K, sym, name)
    close(dw, ref, 3e-5, 'wgrad %s split%d' % (sym, splits))
    dw_b, db = K.conv_wgrad(xd, gyd, geom, with_bias=True)
    ran(K, sym, name_b)
    assert torch.equal(dw_b, dw)
    bias_close(db, gy, 'wgrad+bias %s split%d' % (sym, splits))
    dw_r, db_r = K.conv_wgrad(xd, gyd, geom, with_bias=True, relu_x=True)
    ran(K, sym, name_b)
    close(dw_r, wgrad_ref(x, gy, k, C, Ko, st, True, up), 3e-5, 'wgrad relu_x %s' % sym)
    assert torch.equal(db_r, db)
    if splits >= 15:                                          # (16 or more slabs of fewer than 65536 float4 columns: the lanes kernel ran above)
        K.lib.ctgan_debug_reduce_lanes(0)
        try:
            dw_0, db_0 = K.conv_wgrad(xd, gyd, geom, with_bias=True)
            ran(K, sym, name_b)
            dw_1 = K.conv_wgrad(xd, gyd, geom)
        finally:
            K.lib.ctgan_debug_reduce_lanes(1)
        assert torch.equal(dw_0, dw) and torch.equal(db_0, db) and torch.equal(dw_1, dw)
    if how == 'pipe':
        with forced_generic(K):
            dw_g = K.conv_wgrad(xd, gyd, geom)
            ran(K, WTABLE % ('true', 'true', tile), 'igemm_wgrad<avec,bvec,%s,split%d>' % (TILE_NAME[tile], splits))
        assert torch.equal(dw_g, dw)                          # same plan, same MFMA order


@pytest.mark.parametrize('how', ['nchw_dy', 'misaligned_x'])
def test_weight_gradient_operands_the_pipelined_kernel_refuses(K, how):
    """5 x 64 x 8 x 8 -> 128, 3x3 (64x64 tiles, 3 splits) with an NCHW dy (no unit stride over the GEMM's N index: BVEC off) or an x one float
    off 16-byte alignment (AVEC off): the table-driven kernel with the pipelined kernel's plan - and its bits."""
    case = (5, 64, 8, 8, 128, 3, 1, False)
    N, C, H, W, Ko, k, st, up = case
    g = gen('wgrad-refused')
    geom = K.ConvGeom(C, H, W, Ko, k, k, st, up)
    x, gy = wgrad_operands(case, g)
    want = K.conv_wgrad(cl(x), cl(gy), geom)
    ran(K, WPIPE % T64x64, 'igemm_wgrad_pipe<64x64,split3>')
    if how == 'nchw_dy':
        dw = K.conv_wgrad(cl(x), dev(gy), geom)
        ran(K, WTABLE % ('true', 'false', T64x64), 'igemm_wgrad<avec,bgen,64x64,split3>')
    else:
        dw = K.conv_wgrad(offset_cl(x), cl(gy), geom)
        ran(K, WTABLE % ('false', 'true', T64x64), 'igemm_wgrad<agen,bvec,64x64,split3>')
    close(dw, wgrad_ref(x, gy, k, C, Ko, st, False), 3e-5, 'wgrad ' + how)
    assert torch.equal(dw, want)


@pytest.mark.parametrize('case', [WGRAD_CASES[6], WGRAD_CASES[1], WGRAD_CASES[18], WGRAD_CASES[20], WGRAD_CASES[8]],
                         ids=[WGRAD_IDS[6], WGRAD_IDS[1], WGRAD_IDS[18], WGRAD_IDS[20], WGRAD_IDS[8]])
def test_weight_gradient_writes_nothing_outside_dw_and_db(K, case):
    """dw and db as interior slices of sentinel-filled buffers, with and without the bias gradient: the pipelined kernel (a partial N tile - its
    M tiles lie inside one filter tap and are never partial - and the lanes reduction), the table-driven one (partial M and N tiles; the
    128x32 tile with the column-sum bias)."""
    N, C, H, W, Ko, k, st, up, how, tile, splits = case
    g = gen('wgrad', case[:8])
    geom = K.ConvGeom(C, H, W, Ko, k, k, st, up)
    sym, name, name_b = wgrad_names(how, tile, splits)
    x, gy = wgrad_operands(case, g)
    xd, gyd = cl(x), cl(gy)
    want_w, want_b = K.conv_wgrad(xd, gyd, geom, with_bias=True)
    n, pad, S = k * k * C * Ko, 64, -12345.0
    for with_bias in (True, False):
        bw = torch.full((n + 2 * pad,), S, device='cuda'); bb = torch.full((Ko + 2 * pad,), S, device='cuda')
        dw, db = bw[pad:pad + n].view(k, k, C, Ko), bb[pad:pad + Ko]
        K.conv_wgrad(xd, gyd, geom, with_bias=with_bias, out=(dw, db if with_bias else None))
        ran(K, sym, name_b if with_bias else name)
        torch.cuda.synchronize()
        assert torch.equal(dw, want_w) and (bw[:pad] == S).all() and (bw[pad + n:] == S).all()
        assert (bb[:pad] == S).all() and (bb[pad + Ko:] == S).all()
        assert torch.equal(db, want_b) if with_bias else (db == S).all()


# ------------------------------------------------------------------------------------------------------------------------------------ E
def segments(geom, Ns, flags, g):
    """[(x, gy, relu_x, with_bias)] on the device, the fp64 sum of the segments' weight gradients, and the dy of the segments with the bias flag"""
    segs, ref_w, gy_b = [], 0, []
    for n, (relu_x, with_bias) in zip(Ns, flags):
        x = torch.randn(n, geom.C, geom.H, geom.W, generator=g); gy = torch.randn(n, geom.K, geom.P, geom.Q, generator=g)
        segs.append((cl(x), cl(gy), relu_x, with_bias))
        ref_w = ref_w + wgrad_ref(x, gy, geom.R, geom.C, geom.K, geom.stride, relu_x)
        if with_bias:
            gy_b.append(gy)
    return segs, ref_w, (torch.cat(gy_b) if gy_b else None)


# (C, H, Ko, k, Ns, (relu_x, with_bias) per segment, tile, splits): the plan for the summed Kg, then the growth loop
MULTI_CASES = [
    (128, 4, 128, 3, (1, 1, 1), ((True, True), (False, False), (True, False)), T64x64, 3),     # Kg 48: ONE planned split for three segments (the loop that
                                                                                               # never ended leaves by splits <= nseg)
    (64, 8, 128, 3, (3, 2, 1), ((False, False), (True, True), (False, True)), T64x64, 3),      # Kg 384: 3 planned, chunk 128 gives 2 + 1 + 1 = 4: grows twice
    (128, 8, 128, 3, (7, 3), ((True, True), (False, False)), T64x64, 5),                       # Kg 640: 5 planned, chunk 128 gives 4 + 2 = 6: 160 gives 3 + 2
    (128, 8, 128, 3, (12, 4), ((False, False), (True, False)), T64x64, 8),                     # Kg 1024: 8 planned, 6 + 2 fits at once; no bias at all
    (96, 8, 128, 3, (5, 3), ((False, True), (True, True)), T32x128, 4),                        # Kg 512: 4 planned, 3 + 2 = 5: 160 gives 2 + 2; both biased
]
MULTI_IDS = ['C%d_%dx%d_K%d_k%d_%s' % (c[0], c[1], c[1], c[2], c[3], '+'.join(map(str, c[4]))) for c in MULTI_CASES]


@pytest.mark.parametrize('case', MULTI_CASES, ids=MULTI_IDS)
def test_multi_segment_weight_gradient(K, case):
    C, H, Ko, k, Ns, flags, tile, splits = case
    g = gen('multi', case[:5])
    geom = K.ConvGeom(C, H, H, Ko, k, k, 1, False)
    segs, ref_w, gy_b = segments(geom, Ns, flags, g)
    dw = torch.empty(k, k, C, Ko, device='cuda'); db = torch.empty(Ko, device='cuda') if gy_b is not None else None
    K.conv_wgrad_multi(segs, geom, dw, db)
    ran(K, WPIPE % tile, 'igemm_wgrad_pipe<%s,split%d%s>' % (TILE_NAME[tile], splits, ',bias' if db is not None else ''))
    close(dw, ref_w, 3e-5, 'wgrad %d segments %s split%d' % (len(Ns), WPIPE % tile, splits))
    if db is not None:
        bias_close(db, gy_b, 'wgrad %d segments' % len(Ns))
    dw2 = torch.empty_like(dw)
    K.conv_wgrad_multi([(x, gy, r, False) for x, gy, r, _ in segs], geom, dw2, None)
    ran(K, WPIPE % tile, 'igemm_wgrad_pipe<%s,split%d>' % (TILE_NAME[tile], splits))
    assert torch.equal(dw, dw2)                                    # the bias row does not perturb the weights


def test_grouped_weight_gradient(K):
    """conv_wgrad_group on filters of all four tiles: one launch of igemm_wgrad_pipe_group_kernel per tile in the order 128x128, 64x128, 64x64,
    32x128 (the symbol of the call is its last launch's) and one batched reduction; against fp64 and, bit for bit, conv_wgrad_multi per filter."""
    g = gen('group')
    # (C, H, Ko, k, stride, Ns, flags)
    members = [
        (128, 32, 128, 1, 1, (32,), ((False, True),)),                                     # 128x128 (Kg 32768)
        (64, 16, 128, 3, 1, (20, 12), ((True, True), (False, False))),                     # 64x128 (Kg 8192)
        (128, 8, 128, 3, 1, (7, 3), ((True, False), (False, False))),                      # 64x64, the chunk grown; no bias
        (128, 16, 128, 4, 2, (4, 2, 1), ((False, True), (True, False), (False, True))),    # 64x64, stride 2
        (96, 8, 40, 3, 1, (5, 3), ((False, True), (True, True))),                          # 32x128 with a partial N tile
    ]
    tiles = [T128x128, T64x128, T64x64, T64x64, T32x128]
    built = []
    for C, H, Ko, k, st, Ns, flags in members:
        geom = K.ConvGeom(C, H, H, Ko, k, k, st, False)
        segs, ref_w, gy_b = segments(geom, Ns, flags, g)
        dw_m = torch.empty(k, k, C, Ko, device='cuda'); db_m = torch.empty(Ko, device='cuda') if gy_b is not None else None
        K.conv_wgrad_multi(segs, geom, dw_m, db_m)
        built.append((segs, geom, ref_w, gy_b, dw_m, db_m))
    for pick in ([0, 1, 2, 3, 4], [0, 1, 2, 3], [0, 1], [0]):
        groups = []
        for i in pick:
            segs, geom, ref_w, gy_b, dw_m, db_m = built[i]
            groups.append((segs, geom, torch.full_like(dw_m, float('nan')), torch.full_like(db_m, float('nan')) if db_m is not None else None))
        K.conv_wgrad_group(groups)
        ran(K, WGROUP % tiles[pick[-1]], 'igemm_wgrad_pipe_group<n%d>' % len(pick))
        for i, (segs, geom, dw, db) in zip(pick, groups):
            _, _, ref_w, gy_b, dw_m, db_m = built[i]
            close(dw, ref_w, 3e-5, 'wgrad group of %d, member %d %s' % (len(pick), i, WGROUP % tiles[i]))
            assert torch.equal(dw, dw_m)
            if db is not None:
                bias_close(db, gy_b, 'wgrad group of %d, member %d' % (len(pick), i))
                assert torch.equal(db, db_m)
