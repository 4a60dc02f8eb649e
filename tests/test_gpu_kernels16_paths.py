"""Every kernel and every branch of the host planners of the 16-bit / split-mode conv family (csrc/igemm16.hip, csrc/conv16s2.h and the
single-problem path into csrc/wgrad16c.hip), reached through the public conv entry points of ctgan_amd.kernels.  Each case (a) compares with
the fp64 oracle - oracle.tf_ops.conv2d_same / bias_add_nchw and torch.autograd.grad of them - and (b) asserts the device symbol that ran
(K.last_symbol(), and K.last_kernel() where it carries the K split or the tile) exactly, so that a planner change which reroutes a case
fails here instead of passing on another kernel.  The expected symbols are written down in the case tables (worked out by hand from the
planner's source), never recomputed.

Branch -> test map
  dispatch_conv16 / dispatch_conv16_tiles, one-plane modes (bf16 and fp16, forward and data gradient)         test_one_plane_tiles (A_CASES)
    conv16<64x64,k64>        no K split: nk < 32 (N3 64 10x14); blocks >= 256 with Ng % 128 != 0 (N40 256 K160: 264 blocks; N38: 252 -> split)
    conv16<64x64,k64,ksplit> the loop lowers the count (nk 36: 8 -> 3), stays at 8 (5x5 x 256: nk 100), partial kout tile (K 96),
                             four phases: nk_min is the smallest phase's (3x3 stride 2 K1024: one-tap phase nk 16 -> no split although the
                             four-tap phase has 64; K2048: 32 -> split; 5x5 stride 2 K512: 2x2-tap phase nk 32)
    conv16<128x64,k64>       192 <= big_tiles, t128 < 512: forward N43 K512 (M 6020: 47.03 pixel tiles), stride-1 and four-phase data gradient
    conv16<128x128,k64>      t128 >= 512: forward N117 K512 (M 16380), stride-1 and four-phase (N29 20x28: 4 x 32 x 4) data gradient
    conv16<64x64,k32> / ,ksplit>   C = 32; C = 96 with 5x5 (nk 75: 8 -> 6); data gradient of K = 160
    conv16<128x128,k32>      C = 96 forward, K = 96 data gradient, big_tiles = 192
    thresholds               big_tiles 191 / 192 and t128 511 / 512 (1x1, C = K = 128, N x 8x16)                test_one_plane_thresholds
    slab cap after conv16_ksplit: never binds through kernels.py (ctgan_conv2d16_workspace_bytes sizes the slab for 8 splits); reached by a
    direct C-ABI call with a workspace of two slabs for a plan of three                                         test_one_plane_slab_cap_falls_back_to_one_split
  the same dispatch in split mode ('f32x3')                                                                   test_split_mode (X3_CASES)
    conv16x3hk_kernel        8x8, 16x16, 8x16; 256 workgroups taken, 258 refused; refusals 32x32 (NPX 136), 5x5 on 8x8 (NPX 144), C 64, C 256;
                             debug_x3_hk(2) forces, (0) forbids
    conv16x3hf_kernel<.,4|2|1>  PQ >= 1024: 128 (192 tiles), 64 (96 / 192), 32 (48 / 96 / 192); PQ >= 256: 64 (192), 32 (96 / 192); PQ < 256: 32;
                             "first that qualifies" under debug_x3_halo_always(1): 128 / 64 / 32 on one image; IMGS = 2 (4x4 images on
                             32-pixel tiles); `small` launch on the halo kernel at 96 tiles, slice kernel at 95 / 94; LDS refusal of the
                             128-pixel tile (5x5 on 16x16 -> 64), n_it refusal of every tile (5x5 on 32x32 -> slice kernel)
    conv16x3h_kernel         debug_x3_halo_version(1): 32x32 and 8x8 (IMGS = 2 at 128 pixels), both RELU_IN
    conv16x3sf_kernel fwd    tile 128 (M 16384 / 16256 -> 64), 64 (M 6144), 64 + K split (M 6080, 2560; 2496 -> slice kernel; C 32 -> slice),
                             32 (2x2: M 6080, 1536; 1472 -> slice), 0 (4x4x160 = 2560 terms, 3x3x288); debug_x3_s2fwd(0 | 2) partners
    conv16x3sf_kernel 4 phases  768 workgroups (N48 C512 16x16); 752 -> conv16x3p_kernel<1>; big_tiles 96 -> <1>, 92 -> slice kernel;
                             conv16x3p_kernel<2> only with ctgan_debug_x3_s2dgrad_sf(-1) (from 256 tiles conv16x3sf always takes the launch)
    slice kernels            conv16x3<64x64,k32> / ,ksplit>, <128x64,k32>, <128x128,k32>: 1x1 convs (no halo form), ragged grids, four phases
    conv16_splitk_epilogue   bias + resid + relu (forward), bias + mask + resid (data gradient, also in four phases) behind the slice kernel
                             and conv16x3sf: every ',ksplit' case runs both epilogues; the forward's out-mask      test_splitk_epilogue_applies_the_out_mask
    same products            conv16x3sf against the slice kernel (2e-6 of the largest element), conv16x3sf four-phase against conv16x3p and
                             conv16x3hf against conv16x3h (equal bits)                                          test_split_mode_partners
  wgrad16_plan                                                                                                test_weight_gradient (W_CASES)
    tiles 256x256, 256x128 (K 128, 384), 128x128 (C 128, 384), 128x64 (K 64, 96, 160), 64x128, 64x64 (K 64, 96); C 256 with K 96: not wide;
    split mode: wgrad16_kernel<3, 2, 2, .>;  non-power-of-two grids 12x12, 6x8, 5x12 at stride 1 and 2: the wide tiles are not chosen;
    splits: 1 direct / through the slab with bias (every splits == 1 case), Kg 48, max_s binding (Kg 256; Kg 272: the + 0.03 rule), fullest last
    round (3 of 4; ragged last chunk 256 of 384), chunk rounding (15 -> 13), cand <= 64 (49), 8 x resident (2 where 21 would be fuller)
    sentinels around dw / db                                                                                  test_weight_gradient_writes_nothing_outside_dw_and_db
  single conv_wgrad on wgrad16c_group_kernel<mma>: 8-, 16-, 32- (all modes) and 64-wide (one-plane) grids, stride 1 / 2, one / several splits;
    refusals pq < 64, H != stride * P, non-dense images -> wgrad16<128x128>                                    test_column_weight_gradient
  ctgan_conv2d16_x3_prefers / _supported / _bn_in_takes at their thresholds, and the default mode follows them  test_routing_predicates, test_default_mode_follows_the_predicate

No case: in conv16x3hf_tile the 64- / 128-pixel tile on images below 256 pixels and the 128-pixel tile ahead of the 64-pixel one
on 256 .. 1023 pixels - with square filters the smaller tile qualifies wherever the larger one does (fewer patch rows); prefer_v1 in
launch_conv16x3h (x3_8x8_mode() is 1); conv16x3p_kernel<2> without the debug switch (from 256 tiles of 64 positions conv16x3sf takes the launch);
the slab cap of dispatch_conv16 from kernels.py; the `cand * tiles <= 8 * resident` cap of wgrad16_plan is reached, the LDS reservation
failures are not.  The BN-on-load instantiations of conv16x3hf_kernel belong to test_gpu_bn_paths.py, the grouped weight-gradient launches to
test_gpu_wgrad_col.py, test_planner_fuzz.py and test_gpu_kernels16.py.

Tolerances (all the project's own, tests/test_gpu_kernels16.py): one-plane modes - operands on a grid both formats hold exactly (quarter
steps; the products and, at these sizes, every partial sum are exact in fp32): relerr < 2e-5; generic fp32 operands: relative L2 <= 2 * EPS
(2^-9 bf16, 2^-12 fp16).  Split mode - against the fp32 MFMA family's distance to fp64 on the same inputs: rel_l2 <= max(2 e1, 3e-7), relerr
<= max(3 m1, 2e-6).  Bias gradient: 1e-6 x max sum|dy|.  Every figure is printed before it is asserted (pytest -s shows the headroom).
Measured on an MI355X: exact check <= 8.6e-8 (the sums are exact; what is left is the fp32 bias / residual add), rounding check <= 0.64 of its
bound in both formats, split mode <= 0.88 of the relative-L2 bound and <= 0.45 of the largest-element bound, bias gradient <= 6.3e-8,
conv16x3sf against the slice kernel 5.6e-7.  The cap of 64 candidates in wgrad16_plan binds for one-tile filters from 16,385 pixels; the case
uses 16,640.  At 65,536 pixels (49 splits of 1,344 pixels against the fp32 family's 170 of 416) the split mode measured rel_l2 7.4e-7 against
3.8e-7: fp32 summation noise that grows with the chain length, outside the criterion's factor of two - the reduction length was shortened,
the bound was not touched.
"""
import ctypes
import zlib

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import tf_ops  # noqa: E402

EPS = {'bf16': 2.0 ** -9, 'f16': 2.0 ** -12}
MMA = {'bf16': 1, 'f16': 2, 'f32x3': 3}
B16 = ('bf16', 'f16')
ALL = ('bf16', 'f16', 'f32x3')


def reset_hooks(K):
    K.debug_x3_halo_version(0)
    K.debug_x3_hk(1, 256)
    K.debug_x3_halo_always(False)
    K.debug_x3_s2fwd(True)
    K.debug_x3_s2halo(True)
    K.lib.ctgan_debug_x3_s2dgrad_sf(0)


@pytest.fixture(scope='module')
def K():
    import ctgan_amd.kernels as K
    hybrid, mode = K.X3_HYBRID, K.MMA_DTYPE
    K.set_mma_dtype(None)
    try:
        yield K
    finally:
        K.X3_HYBRID = hybrid
        K.set_mma_dtype(mode)
        reset_hooks(K)


class hooks:
    """The debug switches of the split mode for the duration of a block: hk = (mode), halo_always, halo_version, s2fwd, s2halo, s2dgrad_sf."""

    def __init__(self, K, **kw):
        self.K, self.kw = K, kw

    def __enter__(self):
        K, kw = self.K, self.kw
        if 'hk' in kw: K.debug_x3_hk(kw['hk'])
        if 'halo_always' in kw: K.debug_x3_halo_always(kw['halo_always'])
        if 'halo_version' in kw: K.debug_x3_halo_version(kw['halo_version'])
        if 's2fwd' in kw: K.debug_x3_s2fwd(kw['s2fwd'])
        if 's2halo' in kw: K.debug_x3_s2halo(kw['s2halo'])
        if 's2dgrad_sf' in kw: K.lib.ctgan_debug_x3_s2dgrad_sf(kw['s2dgrad_sf'])

    def __exit__(self, *a):
        reset_hooks(self.K)


class fp32_family:
    """The fp32 MFMA family: no 16-bit mode and no routing of large layers to the split mode."""

    def __init__(self, K):
        self.K = K

    def __enter__(self):
        self.old = (self.K.X3_HYBRID, self.K.set_mma_dtype(None))
        self.K.X3_HYBRID = False

    def __exit__(self, *a):
        self.K.X3_HYBRID = self.old[0]
        self.K.set_mma_dtype(self.old[1])


def cl(t):
    """channels-last copy on device"""
    d = t.to('cuda')
    out = torch.empty((d.shape[0], d.shape[2], d.shape[3], d.shape[1]), device='cuda', dtype=d.dtype).permute(0, 3, 1, 2)
    out.copy_(d)
    return out


def relerr(a, b):
    a = a.detach().cpu().double(); b = b.detach().cpu().double()
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-30)).item()


def rel_l2(a, b):
    a = a.detach().cpu().double(); b = b.detach().cpu().double()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


def gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))      # hash() of a str is per-process random


def grid(t):
    """quarter steps: at most 6 significant bits - exact in bf16 and in fp16"""
    return (t * 4).round().clamp(-24, 24) / 4


def ran(K, symbol, kernel):
    assert K.last_symbol() == symbol, (K.last_symbol(), symbol, K.last_kernel())
    assert K.last_kernel() == kernel, (K.last_kernel(), kernel)


def close16(got, ref, dt, exact, what):
    """the two checks of test_gpu_kernels16.py"""
    assert tuple(got.shape) == tuple(ref.shape)
    if exact:
        e = relerr(got, ref)
        print('relerr %-5s %-64s %.3e (< 2e-05)' % (dt, what, e))
        assert e < 2e-5, (what, dt, e)
    else:
        e = rel_l2(got, ref)
        print('rel_l2 %-5s %-64s %.3e (<= %.2e)' % (dt, what, e, 2 * EPS[dt]))
        assert e <= 2 * EPS[dt], (what, dt, e)


def close_x3(got3, got1, ref, what):
    """the criterion of test_f32x3_split_mode_is_as_accurate_as_the_fp32_mfma_family: got1 = the fp32 MFMA family on the same inputs"""
    assert tuple(got3.shape) == tuple(ref.shape)
    e3, e1, m3, m1 = rel_l2(got3, ref), rel_l2(got1, ref), relerr(got3, ref), relerr(got1, ref)
    print('f32x3 %-60s rel_l2 %.3e (fp32 family %.3e)  relerr %.3e (fp32 family %.3e)' % (what, e3, e1, m3, m1))
    assert e3 <= max(2.0 * e1, 3e-7), (what, e3, e1)
    assert m3 <= max(3.0 * m1, 2e-6), (what, m3, m1)


def bias_close(db, gy, what):
    scale = gy.double().abs().sum(dim=(0, 2, 3)).max().item()                  # a sum of N(0,1) draws may cancel to ~0
    e = (db.cpu().double() - gy.double().sum(dim=(0, 2, 3))).abs().max().item() / scale
    print('biaserr %-69s %.3e (< 1e-06)' % (what, e))
    assert tuple(db.shape) == (gy.shape[1],) and e < 1e-6, (what, e)


def tf(b):
    return 'true' if b else 'false'


class Problem:
    """Operands and fp64 references of one geometry: forward plain and relu(conv(relu(x)) + b + r); data gradient plain and
    where(m > 0, dx + bc, 0) + rr; weight gradient without and with ReLU on load of x.  exact: conv operands on the 16-bit grid."""

    def __init__(self, K, case, exact, want=('fwd', 'dgrad'), tag='p'):
        N, C, H, W, Ko, k, st = case
        g = gen(tag, case, exact)
        self.case, self.geom = case, K.ConvGeom(C, H, W, Ko, k, k, st, False)
        P, Q = self.geom.P, self.geom.Q
        x, gy = torch.randn(N, C, H, W, generator=g), torch.randn(N, Ko, P, Q, generator=g)
        w = torch.randn(k, k, C, Ko, generator=g)
        scale = 2.0 ** -round(np.log2(np.sqrt(k * k * C)))
        if exact:
            x, gy, w = grid(x), grid(gy), grid(w)
        w = w * scale
        self.x, self.gy, self.w = x, gy, w
        self.b, self.r = torch.randn(Ko, generator=g), torch.randn(N, Ko, P, Q, generator=g)
        self.bc, self.m, self.rr = torch.randn(C, generator=g), torch.randn(N, C, H, W, generator=g), torch.randn(N, C, H, W, generator=g)
        xd, wd = x.double(), w.double()
        if 'fwd' in want:
            self.y = tf_ops.bias_add_nchw(tf_ops.conv2d_same(xd, wd, st), self.b.double())
            self.y_full = torch.relu(tf_ops.bias_add_nchw(tf_ops.conv2d_same(torch.relu(xd), wd, st), self.b.double()) + self.r.double())
        if 'dgrad' in want:
            x_ = torch.zeros(N, C, H, W, dtype=torch.float64, requires_grad=True)
            (self.dx,) = torch.autograd.grad(tf_ops.conv2d_same(x_, wd, st), x_, gy.double())
            self.dx_full = torch.where(self.m.double() > 0, self.dx + self.bc.double().view(1, -1, 1, 1), torch.zeros_like(self.dx)) + self.rr.double()
        if 'wgrad' in want:
            w_ = torch.zeros(k, k, C, Ko, dtype=torch.float64, requires_grad=True)
            (self.dw,) = torch.autograd.grad(tf_ops.conv2d_same(xd, w_, st), w_, gy.double())
            (self.dw_relu,) = torch.autograd.grad(tf_ops.conv2d_same(torch.relu(xd), w_, st), w_, gy.double())
        self.xd, self.wd, self.gyd, self.bd, self.rd = cl(x), w.cuda(), cl(gy), self.b.cuda(), cl(self.r)
        self.bcd, self.md, self.rrd = self.bc.cuda(), cl(self.m), cl(self.rr)

    def run(self, K, what):
        N = self.case[0]
        if what == 'fwd':
            return K.conv_fwd(self.xd, self.wd, self.bd, self.geom)
        if what == 'fwd_full':
            return K.conv_fwd(self.xd, self.wd, self.bd, self.geom, resid=self.rd, relu=True, relu_in=True)
        if what == 'dgrad':
            return K.conv_dgrad(self.gyd, self.wd, self.geom, N)
        assert what == 'dgrad_full'
        return K.conv_dgrad(self.gyd, self.wd, self.geom, N, bias=self.bcd, mask=self.md, resid=self.rrd)

    def ref(self, what):
        return {'fwd': 'y', 'fwd_full': 'y_full', 'dgrad': 'dx', 'dgrad_full': 'dx_full'}[what]


RUNS = {'fwd': (('fwd', False), ('fwd_full', True)), 'dgrad': (('dgrad', False), ('dgrad_full', False))}      # (launch, RELU_IN of its symbol)
cid = lambda c: 'N%d_C%d_%dx%d_K%d_k%d_s%d' % c

# ------------------------------------------------------------------------------------------------------------------------------------ A
# conv16_kernel<MMA, TM, TN, BK, RELU_IN, one wave> and the tile part of K.last_kernel()
T64K64, T128X64K64, T128K64, T64K32, T128X64K32, T128K32 = '1, 1, 64', '2, 1, 64', '2, 2, 64', '1, 1, 32', '2, 1, 32', '2, 2, 32'
TNAME = {T64K64: '64x64,k64', T128X64K64: '128x64,k64', T128K64: '128x128,k64', T64K32: '64x64,k32', T128X64K32: '128x64,k32', T128K32: '128x128,k32'}
SPLIT, WHOLE = True, False


def conv16_names(mma, tile, ksplit, relu_in):
    return ('conv16_kernel<%d, %s, %s, false>' % (mma, tile, tf(relu_in)),
            'conv16%s<%s%s>' % ('x3' if mma == 3 else '', TNAME[tile], ',ksplit' if ksplit else ''))


# ((N, C, H, W, K, k, stride), forward (tile, K split) or None, data gradient (tile, K split) or None): M = output pixels (per phase), Ng = kout,
# big_tiles = phases * ceil(M / 128) * ceil(Ng / 128), blocks = phases * ceil(M / 64) * ceil(Ng / 64), nk = taps * reduction channels / BK
A_CASES = [
    # forward M 420 Ng 128 nk 9; data gradient Ng 64 nk 18: nk < 32
    ((3, 64, 10, 14, 128, 3, 1), (T64K64, WHOLE), (T64K64, WHOLE)),
    # forward Ng 160 (partial kout tile), M 5600: 88 x 3 = 264 blocks >= 256 although nk 36; data gradient reduces over 160 channels: k32, 352 blocks
    ((40, 256, 10, 14, 160, 3, 1), (T64K64, WHOLE), (T64K32, WHOLE)),
    # ... M 5320: 84 x 3 = 252 blocks -> 512 / 252 = 2 splits of 18 slices; data gradient 84 x 4 = 336 blocks
    ((38, 256, 10, 14, 160, 3, 1), (T64K64, SPLIT), (T64K32, WHOLE)),
    # forward M 180, 6 blocks, nk 36: 8 -> 3 (36 / 3 = 12); data gradient nk 18
    ((3, 256, 6, 10, 128, 3, 1), (T64K64, SPLIT), (T64K64, WHOLE)),
    # 5x5 x 256: nk 100 stays at 8 (100 / 8 = 12); data gradient nk 50: 8 -> 4
    ((3, 256, 6, 10, 128, 5, 1), (T64K64, SPLIT), (T64K64, SPLIT)),
    # 5x5 stride 2: forward nk 50; data gradient in four phases of 3x3 / 3x2 / 2x3 / 2x2 taps over 512 channels: nk_min 4 x 8 = 32 -> 2 splits
    ((3, 128, 12, 20, 512, 5, 2), (T64K64, SPLIT), (T64K64, SPLIT)),
    # 3x3 stride 2, SAME pad (0, 1): phases of 2x2 / 2x1 / 1x2 / 1x1 taps; K 1024: the one-tap phase has nk 16 < 32 (the 2x2 phase 64): no split
    ((3, 128, 8, 12, 1024, 3, 2), (T64K64, WHOLE), (T64K64, WHOLE)),
    # ... K 2048: nk_min 32 -> 8 blocks, 8 -> 2
    ((3, 128, 8, 12, 2048, 3, 2), (T64K64, WHOLE), (T64K64, SPLIT)),
    # forward Ng 512, M 6020 = 47.03 tiles of 128: big_tiles 48 x 4 = 192, t128 192 < 512; data gradient Ng 64: 95 blocks, nk 72: 5 splits
    ((43, 64, 10, 14, 512, 3, 1), (T128X64K64, WHOLE), (T64K64, SPLIT)),
    ((43, 512, 10, 14, 64, 3, 1), (T64K64, SPLIT), (T128X64K64, WHOLE)),
    # M 16380 = 127.97 tiles: t128 128 x 4 = 512 (the mirrored operator of these two is left out: 20 GFLOP of fp64 each)
    ((117, 64, 10, 14, 512, 3, 1), (T128K64, WHOLE), None),
    ((117, 512, 10, 14, 64, 3, 1), None, (T128K64, WHOLE)),
    # four-phase data gradient, Ng 512: M 1540 per phase: big_tiles 4 x 13 x 4 = 208, t128 208; forward Ng 64: 25 blocks, nk 128
    ((11, 512, 20, 28, 64, 4, 2), (T64K64, SPLIT), (T128X64K64, WHOLE)),
    # ... M 4060: t128 4 x 32 x 4 = 512
    ((29, 512, 20, 28, 64, 4, 2), (T64K64, SPLIT), (T128K64, WHOLE)),
    # C 32: 32-deep slices, nk 9; data gradient Ng 32 (half a kout tile)
    ((3, 32, 10, 14, 128, 3, 1), (T64K32, WHOLE), (T64K64, WHOLE)),
    # C 96 with 5x5: nk 75: 8 -> 6 (75 / 6 = 12); data gradient Ng 96 (1.5 kout tiles), nk 50: 8 -> 4
    ((3, 96, 6, 10, 128, 5, 1), (T64K32, SPLIT), (T64K64, SPLIT)),
    # C 96, big_tiles 192: the 32-deep family has no 128x64 tile; data gradient Ng 96: 95 x 2 = 190 blocks, nk 72: 2 splits on a partial kout tile
    ((43, 96, 10, 14, 512, 3, 1), (T128K32, WHOLE), (T64K64, SPLIT)),
    ((43, 512, 10, 14, 96, 3, 1), (T64K64, SPLIT), (T128K32, WHOLE)),
]


def check_one_plane(K, case, fwd, dgrad, tag='A'):
    want = [op for op, e in (('fwd', fwd), ('dgrad', dgrad)) if e is not None]
    for exact in (True, False):
        pr = Problem(K, case, exact, want, tag)
        for dt in B16:
            with K.mma_dtype(dt):
                for op, expect in (('fwd', fwd), ('dgrad', dgrad)):
                    if expect is None:
                        continue
                    for what, relu_in in RUNS[op]:
                        got = pr.run(K, what)
                        sym, name = conv16_names(MMA[dt], expect[0], expect[1], relu_in)
                        ran(K, sym, name)
                        close16(got, getattr(pr, pr.ref(what)), dt, exact, '%s %s' % (what, name))


@pytest.mark.parametrize('case', A_CASES, ids=lambda c: cid(c[0]))
def test_one_plane_tiles(K, case):
    check_one_plane(K, *case)


# 1x1, C = K = 128 on N images of 8x16 (one pixel tile each): big_tiles = t128 = N for both operators
@pytest.mark.parametrize('N,tile', [(191, T64K64), (192, T128X64K64), (511, T128X64K64), (512, T128K64)])
def test_one_plane_thresholds(K, N, tile):
    check_one_plane(K, (N, 128, 8, 16, 128, 1, 1), (tile, WHOLE), (tile, WHOLE), 'A-threshold')


def test_one_plane_slab_cap_falls_back_to_one_split(K):
    """dispatch_conv16 drops the K split when its slabs exceed the workspace.  kernels.py always passes 8 slabs' worth, so the branch needs a
    direct C-ABI call: (3, 256, 6x10, K128, 3x3) plans 3 splits (276,480 B of slabs); with 2 slabs' worth the launch runs whole."""
    case = (3, 256, 6, 10, 128, 3, 1)
    pr = Problem(K, case, True, ('fwd',), 'A')
    N, Ko, g = case[0], case[4], pr.geom
    slab = N * g.P * g.Q * Ko * 4
    ws = torch.empty(3 * slab, dtype=torch.uint8, device='cuda')
    for dt in B16:
        for nbytes, split in ((3 * slab, SPLIT), (3 * slab - 4, WHOLE), (2 * slab, WHOLE)):
            y = K.empty_cl(N, Ko, g.P, g.Q, pr.xd.device)
            d = g.desc(N, pr.xd.stride(), y.stride())
            wp = K._packed16(pr.wd, d, 0, g, dt)
            K.check(K.lib.ctgan_conv2d16_fwd(ctypes.byref(d), MMA[dt], K._ptr(pr.xd), K._ptr(wp), K._ptr(pr.bd), None, K._ptr(y), 0, None, K._ptr(ws),
                                             nbytes, K._stream()), 'conv2d16_fwd')
            ran(K, *conv16_names(MMA[dt], T64K64, split, False))
            close16(y, pr.y, dt, True, 'fwd with %d B of workspace' % nbytes)


def test_null_ext_and_an_ext_with_nothing_on_take_the_same_path(K):
    """ctgan_conv2d16_fwd / ctgan_conv2d16_dgrad (bf16) with ext = NULL and with an ext that switches nothing on: the same kernel and the same
    bits.  (The entry points that took no ext used to forward NULL to these; one entry per operation leaves the equivalence to this test.)"""
    from ctgan_amd._lib import EpilogueExt
    N, C, H, W, Ko, k = 2, 64, 8, 8, 64, 3
    g = gen('null-ext')
    geom = K.ConvGeom(C, H, W, Ko, k, k, 1, False)
    x, gy = cl(torch.randn(N, C, H, W, generator=g)), cl(torch.randn(N, Ko, H, W, generator=g))
    w = (torch.randn(k, k, C, Ko, generator=g) / np.sqrt(k * k * C)).to('cuda')
    d = geom.desc(N, x.stride(), gy.stride())
    wp = [K._packed16(w, d, op, geom, 'bf16') for op in (0, 1)]
    nb = [K.lib.ctgan_conv2d16_workspace_bytes(ctypes.byref(d), op) for op in (0, 1)]
    ws = torch.empty(max(nb + [16]), dtype=torch.uint8, device='cuda')
    p, st, runs = K._ptr, K._stream(), []
    for fill, e in ((1.0, None), (2.0, EpilogueExt(0.0, 0, 0, None))):
        ext = None if e is None else ctypes.byref(e)
        y, dx = K.empty_cl(N, Ko, H, W, x.device).fill_(fill), K.empty_cl(N, C, H, W, x.device).fill_(fill)
        K.check(K.lib.ctgan_conv2d16_fwd(ctypes.byref(d), MMA['bf16'], p(x), p(wp[0]), None, None, p(y), 0, ext, p(ws), nb[0], st), 'conv2d16_fwd')
        sym_fwd = K.last_symbol()
        K.check(K.lib.ctgan_conv2d16_dgrad(ctypes.byref(d), MMA['bf16'], p(gy), p(wp[1]), None, None, None, p(dx), 0, ext, p(ws), nb[1], st),
                'conv2d16_dgrad')
        runs.append((y, sym_fwd, dx, K.last_symbol()))
    (y0, sf0, dx0, sd0), (y1, sf1, dx1, sd1) = runs
    print('fwd %s | dgrad %s' % (sf0, sd0))
    assert sf0 == sf1 and sd0 == sd1 and sf0 and sd0
    assert torch.equal(y0, y1) and torch.equal(dx0, dx1)


# ------------------------------------------------------------------------------------------------------------------------------------ B
def x3_names(spec, relu_in):
    kind = spec[0]
    if kind == 'hk':
        return 'conv16x3hk_kernel<%s>' % tf(relu_in), 'conv16x3hk<64x64,chunk/wave>'
    if kind == 'hf':
        return 'conv16x3hf_kernel<%s, %d, false>' % (tf(relu_in), spec[1] // 32), 'conv16x3hf<%dx128,k32>' % spec[1]
    if kind == 'h':
        return 'conv16x3h_kernel<%s>' % tf(relu_in), 'conv16x3h<128x128,k32>'
    if kind == 'sf':
        return 'conv16x3sf_kernel<%s, %d>' % (tf(relu_in), spec[1] // 32), 'conv16x3sf<%dx128,k32%s>' % (spec[1], ',ksplit' if spec[2] else '')
    if kind == 'p':
        return 'conv16x3p_kernel<%d>' % (spec[1] // 32), 'conv16x3p<4x%dx128,k32>' % spec[1]
    assert kind == 'slice'
    return conv16_names(3, spec[1], spec[2], relu_in)


HK, H128 = ('hk',), ('h',)
HF128, HF64, HF32 = ('hf', 128), ('hf', 64), ('hf', 32)
SF128, SF64, SF64S, SF32 = ('sf', 128, WHOLE), ('sf', 64, WHOLE), ('sf', 64, SPLIT), ('sf', 32, WHOLE)
P64, P32 = ('p', 64), ('p', 32)
S64, S64S, S128X64, S128 = ('slice', T64K32, WHOLE), ('slice', T64K32, SPLIT), ('slice', T128X64K32, WHOLE), ('slice', T128K32, WHOLE)

# ((N, C, H, W, K, k, stride), debug switches, forward kernel or None, data gradient kernel or None).  The data gradient reduces over K and has
# C kout channels: "tiles" = (M / tile pixels) * (kout / 128)
X3_CASES = [
    # --- conv16x3hk_kernel: C_red = 128, 64-pixel tiles inside one image, NPX = (rows + 2) * (Q + 2) <= 112, at most 256 workgroups of 64 x 64
    ((1, 128, 8, 8, 128, 3, 1), {}, HK, HK),                       # NPX 100, 2 workgroups
    ((1, 128, 16, 16, 128, 3, 1), {}, HK, HK),                     # 4 rows of 16: NPX 6 x 18 = 108
    ((1, 128, 8, 16, 128, 3, 1), {}, HK, HK),                      # P != Q
    ((128, 128, 8, 8, 128, 3, 1), {}, HK, HK),                     # 128 x 2 = 256 workgroups: the last it takes
    ((129, 128, 8, 8, 128, 3, 1), {}, HF32, HF32),                 # 258 workgroups: refused; 258 tiles of 32 pixels
    ((129, 128, 8, 8, 128, 3, 1), {'hk': 2}, HK, HK),              # forced
    ((1, 128, 8, 8, 128, 3, 1), {'hk': 0}, S64S, S64S),            # forbidden: 2 tiles of 32, small -> slice kernel, nk 36: 3 splits
    ((1, 128, 32, 32, 128, 3, 1), {}, S64S, S64S),                 # 2 rows of 32: NPX 4 x 34 = 136 > 112; 8 tiles: small; 32 blocks, nk 36
    ((1, 128, 8, 8, 128, 5, 1), {}, S64S, S64S),                   # 5x5: NPX 12 x 12 = 144
    ((1, 64, 8, 8, 128, 3, 1), {}, S64, S64S),                     # C 64: forward nk 18; data gradient kout 64 (Ng % 128), nk 36
    ((1, 256, 8, 8, 256, 3, 1), {}, S64S, S64S),                   # C 256 (both operators reduce over 256): nk 72
    # --- conv16x3hf_kernel: the preference orders of conv16x3hf_tile
    ((24, 32, 32, 32, 128, 3, 1), {}, HF128, S64),                 # 32x32 (128, 64, 32): 192 tiles of 128; data gradient kout 32: slice kernel, 1536 blocks
    ((24, 128, 32, 32, 32, 3, 1), {}, None, HF128),                # ... the data gradient's turn
    ((12, 32, 32, 32, 128, 3, 1), {}, HF64, S64S),                 # 96 tiles of 128, 192 of 64; data gradient 192 blocks, nk 9 x 4 = 36: 2 splits
    ((12, 128, 32, 32, 32, 3, 1), {}, None, HF64),
    ((6, 32, 32, 32, 128, 3, 1), {}, HF32, S64S),                  # 48 / 96 / 192 tiles; small, 32 < 128 and >= 96 tiles: stays on the halo kernel
    ((6, 128, 32, 32, 32, 3, 1), {}, None, HF32),
    ((48, 32, 16, 16, 128, 3, 1), {}, HF64, S64S),                 # 16x16 (64, 128, 32): 192 tiles of 64
    ((24, 32, 16, 16, 128, 3, 1), {}, HF32, S64S),                 # 96 of 64, 192 of 32
    ((24, 128, 16, 16, 32, 3, 1), {}, None, HF32),
    ((96, 32, 8, 8, 128, 3, 1), {}, HF32, S64S),                   # 8x8 (32, 64, 128): 192 tiles of 32
    ((48, 32, 8, 8, 128, 3, 1), {}, HF32, S64S),                   # 96 tiles of 32: "first that qualifies", the small launch that rides the halo kernel
    ((48, 128, 8, 8, 32, 3, 1), {}, None, HF32),
    ((47, 128, 8, 8, 32, 3, 1), {}, None, S64),                    # 94 tiles: slice kernel (47 x 2 = 94 blocks... of 64 x 64: M 3008 -> 47 x 2), nk 9: whole
    ((192, 32, 4, 4, 128, 3, 1), {}, HF32, S64S),                  # 4x4 images, two per tile (IMGS = 2): 96 tiles
    ((190, 32, 4, 4, 128, 3, 1), {}, S64, S64S),                   # 95 tiles: slice kernel
    # tiny launches on every tile: "first that qualifies" with no tile count reaching 192
    ((1, 32, 32, 32, 128, 3, 1), {'halo_always': 1}, HF128, S64S),
    ((1, 32, 16, 16, 128, 3, 1), {'halo_always': 1}, HF64, S64S),
    ((2, 32, 8, 8, 128, 3, 1), {'halo_always': 1}, HF32, S64S),
    ((6, 32, 4, 4, 128, 3, 1), {'halo_always': 1}, HF32, S64S),    # IMGS = 2
    ((1, 128, 32, 32, 32, 3, 1), {'halo_always': 1}, None, HF128),
    ((1, 128, 16, 16, 32, 3, 1), {'halo_always': 1}, None, HF64),
    # conv16x3h_ok refusals: 5x5 on 16x16 at 128 pixels: NPX 12 x 20 = 240, LDS 3 x 368 x 80 = 88,320 B > 80 KB -> 64 pixels (NPX 8 x 20 = 160);
    # 5x5 on 32x32: n_it 9 / 7 / 6 against 8 / 6 / 4 at 128 / 64 / 32 pixels: no tile, slice kernel even with halo_always
    ((2, 32, 16, 16, 128, 5, 1), {'halo_always': 1}, HF64, S64S),
    ((1, 32, 32, 32, 128, 5, 1), {'halo_always': 1}, S64, S64S),
    ((3, 64, 10, 14, 128, 3, 1), {'halo_always': 1}, S64, S64S),   # M 420: no whole-row tile
    # --- conv16x3h_kernel (filter through LDS, 128-pixel tiles only)
    ((1, 32, 32, 32, 128, 3, 1), {'halo_always': 1, 'halo_version': 1, 'hk': 0}, H128, S64S),
    ((2, 32, 8, 8, 128, 3, 1), {'halo_always': 1, 'halo_version': 1, 'hk': 0}, H128, S64S),       # IMGS = 2: two 8x8 images per tile
    ((1, 128, 32, 32, 32, 3, 1), {'halo_always': 1, 'halo_version': 1, 'hk': 0}, None, H128),
    ((2, 32, 16, 16, 128, 5, 1), {'halo_always': 1, 'halo_version': 1, 'hk': 0}, S64, S64S),      # the LDS refusal has no smaller tile here
    # --- conv16x3sf_kernel, forward: kt = K / 128 = 4
    ((128, 32, 16, 32, 512, 4, 2), {}, SF128, None),               # M 16384: 128 x 4 = 512 tiles of 128
    ((127, 32, 16, 32, 512, 4, 2), {}, SF64, None),                # M 16256: 508 tiles of 128; 1016 of 64
    ((512, 32, 16, 32, 128, 4, 2), {}, SF128, None),               # kt = 1: exactly 512 tiles of 128
    ((511, 32, 16, 32, 128, 4, 2), {}, SF64, None),                # 511
    ((96, 64, 16, 16, 512, 4, 2), {}, SF64, None),                 # M 6144: 384 tiles of 64
    ((95, 64, 16, 16, 512, 4, 2), {}, SF64S, None),                # M 6080: 380 tiles: K split (16 taps, C 64)
    ((95, 64, 16, 16, 512, 2, 2), {}, SF32, None),                 # ... four taps: no K split; 760 tiles of 32
    ((40, 64, 16, 16, 512, 4, 2), {}, SF64S, None),                # M 2560: 160 tiles, the first with the K split
    ((40, 64, 16, 16, 512, 4, 2), {'s2fwd': 2}, S64, None),        # ... without it: slice kernel; big_tiles 80: small, 320 blocks
    ((39, 64, 16, 16, 512, 4, 2), {}, S64, None),                  # M 2496: 156 tiles; 312 blocks
    ((40, 32, 16, 16, 512, 4, 2), {}, S64, None),                  # C 32 < 64: no K split
    ((24, 64, 16, 16, 512, 2, 2), {}, SF32, None),                 # 2x2, M 1536: 192 tiles of 32
    ((23, 64, 16, 16, 512, 2, 2), {}, S64, None),                  # M 1472: 184 tiles; slice kernel, nk 4 x 2 = 8 < 32: whole
    ((40, 160, 16, 16, 512, 4, 2), {}, S64, None),                 # 4 x 4 x 160 = 2560 terms > 2304 (C 64 above: K split); 320 blocks: whole
    ((40, 256, 16, 16, 512, 3, 2), {}, SF64S, None),               # 3 x 3 x 256 = 2304 terms: the last it takes
    ((40, 288, 16, 16, 512, 3, 2), {}, S64, None),                 # 2592
    ((96, 64, 16, 16, 512, 4, 2), {'s2fwd': 0}, S128X64, None),
    # --- four-phase data gradient of the folded 4x4 filters (dx 16x16 from an 8x8 dy grid): workgroups = (M / 64) * 4 * (C / 128)
    ((48, 512, 16, 16, 32, 4, 2), {}, None, SF64),                 # M 3072: 48 x 16 = 768
    ((47, 512, 16, 16, 32, 4, 2), {}, None, P32),                  # 752; 47 x 4 = 188 < 256 tiles of 64: 32 positions
    ((47, 128, 16, 16, 32, 4, 2), {}, None, P32),                  # big_tiles 4 x 24 = 96
    ((46, 128, 16, 16, 32, 4, 2), {}, None, S64),                  # big_tiles 92: slice kernel, 4 x 46 x 2 = 368 blocks
    ((64, 512, 16, 16, 32, 4, 2), {'s2dgrad_sf': -1}, None, P64),  # 64 x 4 = 256 tiles of 64 (conv16x3sf would take it)
    ((63, 512, 16, 16, 32, 4, 2), {'s2dgrad_sf': -1}, None, P32),  # 252
    ((48, 512, 16, 16, 32, 4, 2), {'s2halo': 0}, None, S128X64),   # big_tiles 4 x 24 x 4 = 384 < 512
    ((3, 128, 12, 20, 256, 4, 2), {}, None, S64S),                 # M 180: no position tile; 16 blocks, nk_min 4 x 8 = 32: 2 splits, four-phase slab epilogue
    # --- slice kernels: 1x1 convs have no halo form and no fragment image
    ((3, 64, 10, 14, 128, 1, 1), {}, S64, S64),
    ((3, 1024, 6, 10, 128, 1, 1), {}, S64S, S64),                  # nk 32: 6 blocks, 8 -> 2
    ((43, 128, 10, 14, 512, 1, 1), {}, S128X64, S64),              # big_tiles 192
    ((43, 512, 10, 14, 128, 1, 1), {}, S64, S128X64),
    ((117, 64, 10, 14, 512, 1, 1), {}, S128, S64),                 # t128 512
    ((117, 512, 10, 14, 64, 1, 1), {}, S64, S128),
    ((11, 512, 20, 28, 64, 4, 2), {}, S64S, S128X64),              # ragged four-phase data gradient: t128 208; forward 25 blocks, nk 256
    ((29, 512, 20, 28, 64, 4, 2), {}, S64S, S128),                 # t128 512
    ((43, 96, 10, 14, 512, 3, 1), {}, S128X64, S64S),              # ragged 3x3 (M 6020: no whole-row tile)
]
X3_IDS = ['%s%s' % (cid(c[0]), ''.join('_%s%s' % kv for kv in sorted(c[1].items()))) for c in X3_CASES]


@pytest.mark.parametrize('case', X3_CASES, ids=X3_IDS)
def test_split_mode(K, case):
    geomc, sw, fwd, dgrad = case
    want = [op for op, e in (('fwd', fwd), ('dgrad', dgrad)) if e is not None]
    pr = Problem(K, geomc, False, want, 'B')
    runs = [(what, relu_in, e) for op, e in (('fwd', fwd), ('dgrad', dgrad)) if e is not None for what, relu_in in RUNS[op]]
    with fp32_family(K):
        base = {what: pr.run(K, what) for what, _, _ in runs}
        assert not K.last_symbol().startswith('conv16'), K.last_symbol()
    with K.mma_dtype('f32x3'), hooks(K, **sw):
        for what, relu_in, expect in runs:
            got = pr.run(K, what)
            sym, name = x3_names(expect, relu_in)
            ran(K, sym, name)
            close_x3(got, base[what], getattr(pr, pr.ref(what)), '%s %s' % (what, name))


def test_split_mode_partners(K):
    """The same products on two kernels: conv16x3sf against the slice kernel in another summation order (2e-6 of the largest element);
    the four-phase conv16x3sf against conv16x3p and conv16x3hf against conv16x3h in the same order (equal bits)."""
    def both(case, what, first, second):
        pr = Problem(K, case, False, (what.split('_')[0],), 'B')
        out = []
        with K.mma_dtype('f32x3'):
            for sw, expect in (first, second):
                with hooks(K, **sw):
                    out.append(pr.run(K, what))
                    ran(K, *x3_names(expect, what == 'fwd_full'))
        return out
    for case, what, first, second in [((96, 64, 16, 16, 512, 4, 2), 'fwd_full', ({}, SF64), ({'s2fwd': 0}, S128X64)),
                                      ((40, 64, 16, 16, 512, 4, 2), 'fwd_full', ({}, SF64S), ({'s2fwd': 0}, S64))]:
        a, b = both(case, what, first, second)
        e = float((a - b).abs().max()) / float(b.abs().max())
        print('conv16x3sf vs slice kernel %s: %.3e (<= 2e-06)' % (cid(case), e))
        assert e <= 2e-6, (case, e)
    for case, what, first, second in [((48, 512, 16, 16, 32, 4, 2), 'dgrad_full', ({}, SF64), ({'s2dgrad_sf': -1}, P32)),
                                      ((1, 32, 32, 32, 128, 3, 1), 'fwd_full', ({'halo_always': 1}, HF128), ({'halo_always': 1, 'halo_version': 1}, H128)),
                                      ((2, 32, 8, 8, 128, 3, 1), 'fwd', ({'halo_always': 1}, HF32), ({'halo_always': 1, 'halo_version': 1}, H128))]:
        a, b = both(case, what, first, second)
        assert torch.equal(a, b), case


def test_splitk_epilogue_applies_the_out_mask(K):
    """conv_fwd(mask=) on launches with a K split: where(mask > 0, conv + bias, 0) from conv16_splitk_epilogue_kernel behind the slice kernel
    (bf16 / fp16, operands on the grid) and behind conv16x3sf (split mode)."""
    pr = Problem(K, (3, 256, 6, 10, 128, 3, 1), True, ('fwd',), 'B-mask')
    mk = torch.randn(pr.y.shape, generator=gen('B-mask', 1))
    ref = torch.where(mk.double() > 0, pr.y, torch.zeros_like(pr.y))
    for dt in B16:
        with K.mma_dtype(dt):
            got = K.conv_fwd(pr.xd, pr.wd, pr.bd, pr.geom, mask=cl(mk))
            ran(K, *conv16_names(MMA[dt], T64K64, SPLIT, False))
        close16(got, ref, dt, True, 'fwd out-mask conv16<64x64,k64,ksplit>')
    pr = Problem(K, (40, 64, 16, 16, 512, 4, 2), False, ('fwd',), 'B-mask')
    mk = torch.randn(pr.y.shape, generator=gen('B-mask', 2))
    ref = torch.where(mk.double() > 0, pr.y, torch.zeros_like(pr.y))
    with fp32_family(K):
        base = K.conv_fwd(pr.xd, pr.wd, pr.bd, pr.geom, mask=cl(mk))
        assert K.last_symbol().startswith('igemm_'), K.last_symbol()
    with K.mma_dtype('f32x3'):
        got = K.conv_fwd(pr.xd, pr.wd, pr.bd, pr.geom, mask=cl(mk))
        ran(K, *x3_names(SF64S, False))
    close_x3(got, base, ref, 'fwd out-mask conv16x3sf<64x128,k32,ksplit>')
    assert 0.3 < (got == 0).float().mean().item() < 0.7


# ------------------------------------------------------------------------------------------------------------------------------------ C
# wgrad16_kernel<MMA, TM, TN, RELU_X>: the (TM, TN) part and the tile of K.last_kernel()
W256, W256X128, W128, W128X64, W64X128, W64 = '4, 4', '4, 2', '2, 2', '2, 1', '1, 2', '1, 1'
WNAME = {W256: '256x256', W256X128: '256x128', W128: '128x128', W128X64: '128x64', W64X128: '64x128', W64: '64x64'}
X3 = ('f32x3',)
BF = ('bf16',)

# ((N, C, H, W, K, k, stride), modes, tile, splits): Kg = N * P * Q pixels; tiles = taps * (C / tile) * ceil(K / tile); a candidate split count
# c <= min(ceil(Kg / 256), 64, 8 * resident / tiles) replaces the best so far when its last-round efficiency c * tiles / (rounds * resident)
# is more than 0.03 better (resident = 512 workgroups, 256 for the 256-wide tiles); chunk = ceil(Kg / c) rounded up to 64 pixels
W_CASES = [
    # 4x4 dy grids (16 pixels per image: the column kernel stays out), Kg 32: less than one 64-pixel slice, one split
    ((2, 256, 4, 4, 256, 3, 1), B16, W256, 1),
    ((2, 256, 4, 4, 256, 3, 1), X3, W128, 1),
    ((2, 256, 4, 4, 128, 3, 1), B16, W256X128, 1),
    ((2, 256, 4, 4, 384, 3, 1), B16, W256X128, 1),
    ((2, 128, 4, 4, 128, 3, 1), ALL, W128, 1),
    ((2, 384, 4, 4, 128, 3, 1), ALL, W128, 1),
    ((2, 128, 4, 4, 64, 3, 1), B16, W128X64, 1),
    ((2, 128, 4, 4, 96, 3, 1), B16, W128X64, 1),                  # partial kout tile: 1.5
    ((2, 128, 4, 4, 160, 3, 1), B16, W128X64, 1),                 # 2.5
    ((2, 256, 4, 4, 96, 3, 1), B16, W128X64, 1),                  # C % 256 == 0 but K % 128 != 0: not wide
    ((2, 64, 4, 4, 128, 3, 1), B16, W64X128, 1),
    ((2, 64, 4, 4, 64, 3, 1), B16, W64, 1),
    ((2, 64, 4, 4, 96, 3, 1), B16, W64, 1),
    # non-power-of-two pixel grids (the division path): never the wide tiles
    ((3, 256, 12, 12, 256, 3, 1), B16, W128, 2),                  # Kg 432: c <= 2; 36 tiles: 0.07 -> 0.14; chunk 256: the last split has 176 pixels
    ((3, 256, 6, 8, 256, 3, 1), B16, W128, 1),                    # Kg 144
    ((3, 256, 5, 12, 256, 3, 1), B16, W128, 1),                   # Kg 180
    ((3, 256, 24, 24, 256, 3, 2), B16, W128, 2),                  # stride 2 onto 12x12
    ((3, 256, 12, 16, 256, 4, 2), B16, W128, 1),                  # onto 6x8
    ((3, 256, 10, 24, 256, 3, 2), B16, W128, 1),                  # onto 5x12
    ((3, 64, 12, 12, 96, 3, 1), B16, W64, 2),
    # split counts (9 tiles unless noted)
    ((3, 128, 4, 4, 128, 3, 1), ALL, W128, 1),                    # Kg 48 < one slice
    ((16, 128, 4, 4, 128, 3, 1), BF, W128, 1),                    # Kg 256: c <= 1
    ((17, 128, 4, 4, 128, 3, 1), BF, W128, 1),                    # Kg 272: c <= 2, but 18 / 512 is not 0.03 above 9 / 512
    ((64, 128, 4, 4, 128, 3, 1), ALL, W128, 3),                   # Kg 1024: c <= 4; 0.018, 0.035, 0.053 (taken), 0.070; chunk 384: last split 256 pixels
    ((256, 128, 4, 4, 128, 3, 1), BF, W128, 13),                  # Kg 4096: c 15 (0.018, 0.053, 0.088 ... every second one); chunk 274 -> 320: 13 splits
    ((1040, 128, 4, 4, 128, 1, 1), BF + X3, W128, 44),            # one tile, Kg 16640: c <= 65; c = 1, 17, 33, 49 (steps of 16 / 512); 65 is past the cap of 64;
                                                                  # chunk 340 -> 384: 44 splits
    ((384, 192, 4, 4, 576, 3, 1), BF, W64, 2),                    # 243 tiles: c <= 16; 0.47, 0.95 (c = 2); c = 21 (0.997) is past 8 x resident
]
W_IDS = ['%s_%s' % (cid(c[0]), '+'.join(c[1])) for c in W_CASES]


def wgrad_names(mode, tile, relu_x):
    return ('wgrad16_kernel<%d, %s, %s>' % (MMA[mode], tile, tf(relu_x)), 'wgrad16%s<%s>' % ('x3' if mode == 'f32x3' else '', WNAME[tile]))


def planned_splits(K, pr, mode):
    N, C, H, W, Ko, k, st = pr.case
    d = pr.geom.desc(N, pr.xd.stride(), pr.gyd.stride())
    nbytes = K.lib.ctgan_conv2d16_wgrad_workspace_bytes(ctypes.byref(d), MMA[mode])
    assert nbytes % ((k * k * C + 1) * Ko * 4) == 0
    return nbytes // ((k * k * C + 1) * Ko * 4)


def check_wgrad(K, case, modes, names_of, splits_ok, tag):
    for exact in ((True, False) if any(m in B16 for m in modes) else (False,)):
        pr = Problem(K, case, exact, ('wgrad',), tag)
        base = None
        for mode in modes:
            if mode == 'f32x3':
                if exact:
                    continue
                with fp32_family(K):
                    base = (K.conv_wgrad(pr.xd, pr.gyd, pr.geom), K.conv_wgrad(pr.xd, pr.gyd, pr.geom, relu_x=True))
                    assert K.last_symbol().startswith('igemm_wgrad'), K.last_symbol()
            with K.mma_dtype(mode):
                splits_ok(planned_splits(K, pr, mode), mode)
                dw = K.conv_wgrad(pr.xd, pr.gyd, pr.geom)
                ran(K, *names_of(mode, False))
                dw_b, db = K.conv_wgrad(pr.xd, pr.gyd, pr.geom, with_bias=True)
                ran(K, *names_of(mode, False))
                dw_r, db_r = K.conv_wgrad(pr.xd, pr.gyd, pr.geom, with_bias=True, relu_x=True)
                ran(K, *names_of(mode, True))
            what = '%s %s' % (mode, names_of(mode, False)[1])
            if mode == 'f32x3':
                close_x3(dw, base[0], pr.dw, 'wgrad ' + what)
                close_x3(dw_r, base[1], pr.dw_relu, 'wgrad relu_x ' + what)
            else:
                close16(dw, pr.dw, mode, exact, 'wgrad ' + what)
                close16(dw_r, pr.dw_relu, mode, exact, 'wgrad relu_x ' + what)
            assert torch.equal(dw_b, dw)                          # the bias row does not perturb the weights
            bias_close(db, pr.gy, 'wgrad+bias ' + what)
            assert torch.equal(db_r, db)


@pytest.mark.parametrize('case', W_CASES, ids=W_IDS)
def test_weight_gradient(K, case):
    geomc, modes, tile, splits = case

    def splits_ok(got, mode):
        print('splits %s %s: %d (planned by hand: %d)' % (cid(geomc), mode, got, splits))
        assert got == splits, (got, splits)
    check_wgrad(K, geomc, modes, lambda mode, relu_x: wgrad_names(mode, tile, relu_x), splits_ok, 'C')


@pytest.mark.parametrize('case', [W_CASES[0], W_CASES[1], W_CASES[7], W_CASES[13], W_CASES[23]], ids=[W_IDS[0], W_IDS[1], W_IDS[7], W_IDS[13], W_IDS[23]])
def test_weight_gradient_writes_nothing_outside_dw_and_db(K, case):
    """dw and db as interior slices of sentinel-filled buffers, with and without the bias gradient: one split straight into dw and through the
    slab, a partial kout tile, a ragged last split on the division path, three splits."""
    geomc, modes, tile, splits = case
    N, C, H, W, Ko, k, st = geomc
    pr = Problem(K, geomc, False, (), 'C')
    n, pad, S = k * k * C * Ko, 64, -12345.0
    for mode in modes:
        with K.mma_dtype(mode):
            want_w, want_b = K.conv_wgrad(pr.xd, pr.gyd, pr.geom, with_bias=True)
            for with_bias in (True, False):
                bw = torch.full((n + 2 * pad,), S, device='cuda'); bb = torch.full((Ko + 2 * pad,), S, device='cuda')
                dw, db = bw[pad:pad + n].view(k, k, C, Ko), bb[pad:pad + Ko]
                K.conv_wgrad(pr.xd, pr.gyd, pr.geom, with_bias=with_bias, out=(dw, db if with_bias else None))
                ran(K, *wgrad_names(mode, tile, False))
                torch.cuda.synchronize()
                assert torch.equal(dw, want_w) and (bw[:pad] == S).all() and (bw[pad + n:] == S).all()
                assert (bb[:pad] == S).all() and (bb[pad + Ko:] == S).all()
                assert torch.equal(db, want_b) if with_bias else (db == S).all()


# ((N, C, H, W, K, k, stride), modes, several splits?): dy grids the filter-column kernel takes (C, K multiples of 128; rows of 8 / 16 / 32 pixels,
# 64 in the one-plane modes; a power-of-two grid of >= 64 pixels; H = stride * P)
COL_CASES = [
    ((1, 128, 8, 8, 128, 3, 1), ALL, False),                      # Kg 64: one slice
    ((64, 128, 8, 8, 128, 3, 1), ALL, True),                      # Kg 4096
    ((2, 128, 16, 16, 128, 4, 2), ALL, False),                    # stride 2 onto 8x8, Kg 128
    ((2, 256, 16, 16, 128, 5, 2), ALL, False),                    # 5x5 stride 2: three-tap columns
    ((4, 128, 16, 16, 256, 3, 1), ALL, None),                     # 16-wide
    ((2, 128, 32, 32, 128, 3, 1), ALL, True),                     # 32-wide, Kg 2048
    ((2, 128, 64, 64, 128, 4, 2), ALL, None),                     # stride 2 onto 32x32
    ((1, 128, 64, 64, 128, 3, 1), B16, True),                     # 64-wide: one-plane modes only (a slice is 64 pixels)
]


@pytest.mark.parametrize('case', COL_CASES, ids=lambda c: cid(c[0]))
def test_column_weight_gradient(K, case):
    geomc, modes, several = case

    def names_of(mode, relu_x):
        return 'wgrad16c_group_kernel<%d>' % MMA[mode], 'wgrad16x3_group<col>' if mode == 'f32x3' else 'wgrad16_group<col>'

    def splits_ok(got, mode):
        print('splits %s %s: %d' % (cid(geomc), mode, got))
        assert several is None or (got > 1) == several, (got, several)
    check_wgrad(K, geomc, modes, names_of, splits_ok, 'C-col')


def test_column_weight_gradient_refusals(K):
    """What ctgan_wgrad16c_takes refuses lands on wgrad16<128x128> (C = K = 128): fewer than 64 pixels per image, H != stride * P, the 64-wide
    grid in split mode, and images that are not dense in memory (a sample stride of two images)."""
    for geomc, modes in (((2, 128, 4, 8, 128, 3, 1), ALL), ((2, 128, 15, 16, 128, 3, 2), ALL), ((1, 128, 64, 64, 128, 3, 1), X3)):
        check_wgrad(K, geomc, modes, lambda mode, relu_x: wgrad_names(mode, W128, relu_x), lambda got, mode: None, 'C-refused')
    geomc = (4, 128, 8, 8, 128, 3, 1)
    pr = Problem(K, geomc, False, ('wgrad',), 'C-refused')
    N, C, H, W = geomc[:4]
    wide = torch.zeros(N, 2, H, W, C, device='cuda')
    wide[:, 0].copy_(pr.xd.permute(0, 2, 3, 1))
    x2 = wide[:, 0].permute(0, 3, 1, 2)
    assert x2.stride(0) == 2 * C * H * W and torch.equal(x2, pr.xd)
    with fp32_family(K):
        base = K.conv_wgrad(pr.xd, pr.gyd, pr.geom)
    for mode in ALL:
        with K.mma_dtype(mode):
            dw = K.conv_wgrad(x2, pr.gyd, pr.geom)
            ran(K, *wgrad_names(mode, W128, False))
            dw_dense = K.conv_wgrad(pr.xd, pr.gyd, pr.geom)
            ran(K, 'wgrad16c_group_kernel<%d>' % MMA[mode], 'wgrad16x3_group<col>' if mode == 'f32x3' else 'wgrad16_group<col>')
        if mode == 'f32x3':
            close_x3(dw, base, pr.dw, 'wgrad non-dense images f32x3')
            close_x3(dw_dense, base, pr.dw, 'wgrad dense images f32x3')
        else:
            close16(dw, pr.dw, mode, False, 'wgrad non-dense images')
            close16(dw_dense, pr.dw, mode, False, 'wgrad dense images')


# ------------------------------------------------------------------------------------------------------------------------------------ D
FWD, DGRAD, WGRAD = 0, 1, 2


def desc_of(K, case, layout='cl'):
    N, C, H, W, Ko, k, st = case[:7]
    g = K.ConvGeom(C, H, W, Ko, k, k, st, layout == 'x_up')
    xs, ys = (C * H * W, 1, W * C, C), (Ko * g.P * g.Q, 1, g.Q * Ko, Ko)
    if layout == 'nchw':
        xs, ys = (C * H * W, H * W, W, 1), (Ko * g.P * g.Q, g.P * g.Q, g.Q, 1)
    if layout == 'odd_strides':
        xs = (C * H * W + 2, 1, W * C, C)
    return g.desc(N, xs, ys)


# ((N, C, H, W, K, k, stride), operator, ctgan_conv2d16_x3_prefers)
PREFERS = [
    # stride 1: the 192-tile rule on images of >= 256 pixels (the preferred tile of conv16x3hf_tile)
    ((24, 32, 32, 32, 128, 3, 1), FWD, 1),                        # 192 tiles of 128
    ((12, 32, 32, 32, 128, 3, 1), FWD, 1),                        # 192 of 64
    ((6, 32, 32, 32, 128, 3, 1), FWD, 1),                         # 192 of 32
    ((5, 32, 32, 32, 128, 3, 1), FWD, 0),                         # 160
    ((48, 32, 16, 16, 128, 3, 1), FWD, 1),
    ((24, 32, 16, 16, 128, 3, 1), FWD, 1),                        # 192 of 32
    ((23, 32, 16, 16, 128, 3, 1), FWD, 0),                        # 184
    ((24, 128, 16, 16, 32, 3, 1), DGRAD, 1),
    ((23, 128, 16, 16, 32, 3, 1), DGRAD, 0),
    # the 8x8 rule: 32-pixel tiles, >= 256 of them, PQ == 64
    ((128, 32, 8, 8, 128, 3, 1), FWD, 1),                         # 256 tiles
    ((127, 32, 8, 8, 128, 3, 1), FWD, 0),                         # 254
    ((64, 32, 8, 8, 256, 3, 1), FWD, 1),                          # two kout tiles
    ((1024, 32, 4, 4, 128, 3, 1), FWD, 0),                        # 512 tiles of 32 on 4x4 images: PQ != 64
    # the chunk-per-wave short cut: C_red = 128 launches of <= 256 workgroups, whatever their size
    ((1, 128, 8, 8, 128, 3, 1), FWD, 1),
    ((64, 128, 8, 8, 128, 3, 1), FWD, 1),
    ((64, 128, 8, 8, 128, 3, 1), DGRAD, 1),
    ((128, 128, 8, 8, 128, 3, 1), FWD, 1),                        # 256 workgroups (and 256 tiles of 32: either way)
    ((64, 64, 8, 8, 128, 3, 1), FWD, 0),                          # C 64: 128 tiles of 32
    ((23, 128, 16, 16, 128, 3, 1), FWD, 1),                       # 184 tiles of 32 (C 32 above: 0), 184 workgroups
    ((64, 128, 8, 16, 128, 3, 1), FWD, 1),                        # 8x16 images (no tile rule applies): 256 workgroups
    ((65, 128, 8, 16, 128, 3, 1), FWD, 0),                        # 260
    # no halo form
    ((64, 128, 16, 16, 128, 1, 1), FWD, 0),                       # 1x1
    ((43, 128, 10, 14, 512, 3, 1), FWD, 0),                       # ragged grid
    # stride 2: forward from 96, data gradient from 192 tiles of 128x128
    ((24, 64, 16, 16, 512, 4, 2), FWD, 0),                        # M 1536: t128 12 x 4 = 48
    ((96, 64, 32, 32, 128, 4, 2), FWD, 1),                        # M 24576: 192
    ((48, 64, 32, 32, 128, 4, 2), FWD, 1),                        # 96
    ((47, 64, 32, 32, 128, 4, 2), FWD, 0),                        # 94
    ((48, 64, 32, 32, 96, 4, 2), FWD, 0),                         # K % 128
    ((48, 128, 32, 32, 64, 3, 2), DGRAD, 1),                      # 3x3 (no stride-2 halo shape): 4 x 96 x 1 = 384 >= 192
    ((24, 128, 32, 32, 64, 3, 2), DGRAD, 1),                      # 192
    ((23, 128, 32, 32, 64, 3, 2), DGRAD, 0),                      # 184
    # the stride-2 halo clause (4x4, pad 1; dy grid 8- or 16-wide, pq % 32 == 0): the same 192
    ((96, 128, 16, 16, 128, 4, 2), DGRAD, 1),                     # 4 x 48 = 192
    ((94, 128, 16, 16, 128, 4, 2), DGRAD, 0),                     # 4 x 47 = 188 (N 95: ceil(47.5) = 48)
    ((24, 128, 32, 32, 128, 4, 2), DGRAD, 1),                     # dy 16x16: 4 x 48
    ((23, 128, 32, 32, 128, 4, 2), DGRAD, 0),                     # 4 x 46 = 184
    # weight gradient from 32,768 pixels (and only what the split mode's one tile supports)
    ((128, 128, 16, 16, 128, 3, 1), WGRAD, 1),
    ((127, 128, 16, 16, 128, 3, 1), WGRAD, 0),
    ((128, 64, 16, 16, 128, 3, 1), WGRAD, 0),                     # C % 128
    ((256, 128, 12, 12, 128, 3, 1), WGRAD, 0),                    # 36,864 pixels on a grid that is no power of two
]


def test_routing_predicates(K):
    """ctgan_conv2d16_x3_prefers at its thresholds, the shape_ok_* refusals behind _supported and _x3_prefers, and _bn_in_takes - no launch."""
    lib = K.lib
    for case, op, want in PREFERS:
        d = desc_of(K, case)
        got = lib.ctgan_conv2d16_x3_prefers(ctypes.byref(d), op)
        print('x3_prefers %s op %d: %d' % (cid(case), op, got))
        assert got == want, (case, op, got, want)
    ok = (24, 32, 32, 32, 128, 3, 1)
    okd = (24, 128, 32, 32, 32, 3, 1)
    okw = (128, 128, 16, 16, 128, 3, 1)
    # (case, layout, operator, supported in bf16, in f32x3, preferred)
    refusals = [
        (ok, 'cl', FWD, 1, 1, 1), (okd, 'cl', DGRAD, 1, 1, 1), (okw, 'cl', WGRAD, 1, 1, 1),
        ((24, 48, 32, 32, 128, 3, 1), 'cl', FWD, 0, 0, 0),         # C % 32
        ((24, 32, 32, 32, 126, 3, 1), 'cl', FWD, 0, 0, 0),         # K % 4
        (ok, 'odd_strides', FWD, 0, 0, 0),                         # strides % 4
        (ok, 'nchw', FWD, 0, 0, 0),                                # not channels-last
        (ok, 'x_up', FWD, 0, 0, 0),
        ((24, 128, 32, 32, 48, 3, 1), 'cl', DGRAD, 0, 0, 0),       # K % 32
        ((24, 126, 32, 32, 32, 3, 1), 'cl', DGRAD, 0, 0, 0),       # C % 4
        (okd, 'nchw', DGRAD, 0, 0, 0),
        ((96, 128, 15, 16, 128, 4, 2), 'cl', DGRAD, 0, 0, 0),      # odd H under stride 2
        ((96, 128, 16, 16, 128, 4, 3), 'cl', DGRAD, 0, 0, 0),      # stride 3
        ((128, 96, 16, 16, 128, 3, 1), 'cl', WGRAD, 0, 0, 0),      # C % 64
        ((128, 64, 16, 16, 128, 3, 1), 'cl', WGRAD, 1, 0, 0),      # one-plane only: the split mode needs C % 128
        ((128, 128, 16, 18, 128, 3, 1), 'cl', WGRAD, 0, 0, 0),     # Q % 4
        ((228, 128, 12, 12, 128, 3, 1), 'cl', WGRAD, 1, 0, 0),     # one-plane only: the split mode needs a power-of-two grid
        (okw, 'nchw', WGRAD, 0, 0, 0),
        (okw, 'x_up', WGRAD, 0, 0, 0),
    ]
    for case, layout, op, s16, s3, pref in refusals:
        d = desc_of(K, case, layout)
        got = (lib.ctgan_conv2d16_supported(ctypes.byref(d), op, 1), lib.ctgan_conv2d16_supported(ctypes.byref(d), op, 3), lib.ctgan_conv2d16_x3_prefers(ctypes.byref(d), op))
        print('supported %s %s op %d: bf16 %d f32x3 %d prefers %d' % (cid(case), layout, op, *got))
        assert got == (s16, s3, pref), (case, layout, op, got)
    assert lib.ctgan_conv2d16_supported(ctypes.byref(desc_of(K, ok)), FWD, 4) == 0 and lib.ctgan_conv2d16_supported(ctypes.byref(desc_of(K, ok)), 3, 1) == 0
    # input batch norm on load: the fragment-streaming kernel with tiles inside ONE image
    for case, layout, want in [((1, 32, 32, 32, 128, 3, 1), 'cl', 1), ((2, 32, 8, 8, 128, 3, 1), 'cl', 1), ((2, 32, 4, 4, 128, 3, 1), 'cl', 0),      # IMGS = 2
                               ((1, 32, 32, 32, 128, 1, 1), 'cl', 0), ((1, 32, 32, 32, 96, 3, 1), 'cl', 0), ((1, 32, 32, 32, 128, 5, 1), 'cl', 0),
                               ((4, 32, 32, 32, 128, 4, 2), 'cl', 0), ((1, 32, 32, 32, 128, 3, 1), 'nchw', 0), ((3, 32, 10, 14, 128, 3, 1), 'cl', 0)]:
        d = desc_of(K, case, layout)
        got = lib.ctgan_conv2d16_bn_in_takes(ctypes.byref(d))
        print('bn_in_takes %s %s: %d' % (cid(case), layout, got))
        assert got == want, (case, layout, got)


# one case per clause of the predicate: (case, operator, the split-mode kernel the default mode runs, or None: the fp32 MFMA family)
DEFAULT_MODE = [
    ((6, 32, 32, 32, 128, 3, 1), 'fwd', HF32),                    # the 192-tile rule
    ((5, 32, 32, 32, 128, 3, 1), 'fwd', None),
    ((128, 32, 8, 8, 128, 3, 1), 'fwd', HF32),                    # the 8x8 rule
    ((127, 32, 8, 8, 128, 3, 1), 'fwd', None),
    ((1, 128, 8, 8, 128, 3, 1), 'fwd', HK),                       # the chunk-per-wave short cut
    ((64, 128, 8, 8, 128, 3, 1), 'dgrad', HK),
    ((65, 128, 8, 16, 128, 3, 1), 'fwd', None),
    ((48, 64, 32, 32, 128, 4, 2), 'fwd', SF64S),                  # stride 2 forward from 96 tiles of 128x128: M 12288, 192 tiles of 64: K split
    ((47, 64, 32, 32, 128, 4, 2), 'fwd', None),
    ((24, 128, 32, 32, 64, 3, 2), 'dgrad', S128X64),              # stride 2 data gradient from 192 (3x3: slice kernel, t128 192)
    ((23, 128, 32, 32, 64, 3, 2), 'dgrad', None),
    ((24, 128, 32, 32, 128, 4, 2), 'dgrad', P32),                 # the stride-2 halo clause: 96 tiles of 64 positions < 256
    ((23, 128, 32, 32, 128, 4, 2), 'dgrad', None),
]


@pytest.mark.parametrize('case', DEFAULT_MODE, ids=lambda c: '%s_%s' % (cid(c[0]), c[1]))
def test_default_mode_follows_the_predicate(K, case):
    geomc, op, expect = case
    pr = Problem(K, geomc, False, (op,), 'D')
    assert K.X3_HYBRID and K.MMA_DTYPE is None
    with fp32_family(K):
        base = pr.run(K, op)
        assert K.last_symbol().startswith('igemm_'), K.last_symbol()
    got = pr.run(K, op)
    if expect is None:
        assert K.last_symbol().startswith('igemm_'), K.last_symbol()
        assert torch.equal(got, base)
    else:
        ran(K, *x3_names(expect, False))
    close_x3(got, base, getattr(pr, pr.ref(op)), 'default mode %s %s' % (op, K.last_kernel()))


def test_default_mode_weight_gradient_follows_the_predicate(K):
    """From 32,768 pixels the default mode's single weight gradient is the split mode's (here on the filter-column kernel); below, the fp32 family's."""
    for N, sym in ((128, 'wgrad16c_group_kernel<3>'), (127, None)):
        pr = Problem(K, (N, 128, 16, 16, 128, 3, 1), False, ('wgrad',), 'D')
        with fp32_family(K):
            base = K.conv_wgrad(pr.xd, pr.gyd, pr.geom)
        dw = K.conv_wgrad(pr.xd, pr.gyd, pr.geom)
        if sym is None:
            assert K.last_symbol().startswith('igemm_wgrad'), K.last_symbol()
        else:
            ran(K, sym, 'wgrad16x3_group<col>')
        close_x3(dw, base, pr.dw, 'default mode wgrad N%d %s' % (N, K.last_kernel()))
