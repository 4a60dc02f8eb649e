"""Every kernel and host branch of ctgan_amd/csrc/elementwise.hip (all but the two pixels_u8 kernels, which tests/test_gpu_eval.py covers) and the
four small-linear kernels of ctgan_amd/csrc/skinny.hip against the fp64 references of tests/elementwise_cases.py, at the shapes where they can go
wrong: both branches of map1_kernel / map2_kernel (an operand off a 16-byte boundary), their n % 4 tail and their second grid-stride pass,
copy4d on strided, tied and windowed layouts, pool2 / upsample2 on non-square and non-dense sources, the reductions around their loop and tile
boundaries, colsum with one stage, two stages, the block cap and ld != cols, the scalar path of filter_batch_kernel (the 1x1x3x128 shortcut
filter of the ResNet critic), every kind x pre of filter_batch against numpy restatements of the layouts (not against the product's other
kernels), the two-launch forms of both batch entry points, and the small-linear kernels at every width, with the kernel each case must report.
The case tables, the references, the input conditions and the bounds are in tests/elementwise_cases.py (DESIGN.md section 23 lists which case
reaches which branch); tests/test_elementwise_standins.py runs the same tables on the fp32 stand-ins.

Largest figures measured on an MI355X (relerr = max-abs over the reference's max-abs; "of bound" = the largest fraction of the per-element
bound d U sum|terms| used; what is not listed is bit-equal to its fp32 expression):
  lrelu_fwd 1.1e-8, lrelu_bwd_scaled 5.5e-8    dropout values 5.4e-8 (mask bit-equal)      axpby 4.8e-8
  tanh fwd 5.7e-8, bwd 5.7e-8                  sigmoid fwd 7.4e-8, bwd 7.0e-8              real_prep 5.9e-8, interpolate 1.2e-7
  of bound: rsqrt 0.42, channel_affine 0.25    pool2 0.63, spatial_sum 0.45, sample_sum 0.018, colsum 0.43
  of bound: filter_spread 0.54, filter_fold 0.57, filter_batch 0.52, filter_fold_batch 0.51, the adjoint identity 0.0061
  of bound: small-linear forward 0.29 (GEMM path 0.34), data gradient 0.51 (GEMM path 0.15), weight gradient 0.30, bias gradient 0.088
The figures above one half belong to sums of two to four terms, where the bound counts hardly more than the roundings that happen.
(379 cases, 3.3 s.)  The stand-ins' figures for the same cases are in DESIGN.md section 23.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import elementwise_cases as C  # noqa: E402


@pytest.fixture(scope='module')
def K():
    import ctgan_amd.kernels as K
    return K


@pytest.fixture(scope='module')
def be(K):
    import ctgan_amd.functional as F
    return C.Backend(K, F, 'cuda')


@pytest.fixture(scope='module', autouse=True)
def _report():
    C.MEASURED.clear()
    yield
    print('\nelementwise.hip and the small-linear kernels, largest figures against fp64:\n' + C.report())


# ------------------------------------------------------------------------------------------------------------------------------------ map kernels
@pytest.mark.parametrize('n', C.MAP_SIZES)
@pytest.mark.parametrize('name', sorted(C.MAP_OPS))
def test_map(be, name, n):
    """map1_kernel / map2_kernel on aligned operands: the float4 body (n >= 4) and the tail (n % 4), one block and several."""
    C.check_map(be, name, n)


@pytest.mark.parametrize('name', sorted(C.MAP_OPS))
def test_map_misaligned_and_empty(be, name):
    """The scalar branch: each operand in turn one float past a 16-byte boundary; n = 0 returns success and writes nothing."""
    for i in range(C.MAP_OPS[name].nin):
        C.check_map(be, name, 1025, misaligned=i)
    C.check_map_empty(be, name)


@pytest.mark.parametrize('name', C.MAP_BIG_OPS)
def test_map_second_grid_stride_pass(be, name):
    """More float4s than 2048 blocks of 256 threads hold, and a tail: the second pass of both loops, once per kernel template."""
    C.check_map(be, name, C.MAP_BIG)


@pytest.mark.parametrize('name', sorted(C.LN_MAP_OPS))
def test_mul_rsqrt(be, name):
    for n in C.LN_MAP_SIZES:
        C.check_map(be, name, n)
    C.check_map(be, name, 1025, misaligned=0)
    C.check_map_empty(be, name)


def test_axpby_in_place(be):
    C.check_axpby_in_place(be, 1025)


@pytest.mark.parametrize('first_cl', [True, False])
@pytest.mark.parametrize('name', C.REPACK_OPS)
def test_map_repacks_the_second_operand(be, name, first_cl):
    C.check_map_repack(be, name, first_cl)


# ------------------------------------------------------------------------------------------------------------------------------------ layout, resampling
@pytest.mark.parametrize('case', C.COPY_CASES)
def test_copy4d(be, case):
    C.check_copy4d(be, case)


@pytest.mark.parametrize('scale', C.RESAMPLE_SCALES)
@pytest.mark.parametrize('layout', C.RESAMPLE_LAYOUTS)
@pytest.mark.parametrize('shape', C.RESAMPLE_SHAPES)
def test_pool2_upsample2(be, shape, layout, scale):
    C.check_pool2(be, shape, layout, scale)
    C.check_upsample2(be, shape, layout, scale)


def test_pool2_upsample2_past_the_block_cap(be):
    C.check_pool2(be, C.POOL_BIG, 'nchw', 0.25)
    C.check_upsample2(be, C.UP_BIG, 'cl', 0.5)


@pytest.mark.parametrize('n', C.SPATIAL_N)
@pytest.mark.parametrize('c', C.SPATIAL_C)
@pytest.mark.parametrize('hw', sorted(C.SPATIAL_HW))
def test_spatial_sum_bcast(be, hw, c, n):
    C.check_spatial(be, n, hw, c)


@pytest.mark.parametrize('n', C.SAMPLE_N)
@pytest.mark.parametrize('m', sorted(C.SAMPLE_M))
def test_sample_sum_bcast(be, m, n):
    C.check_sample(be, n, m)


@pytest.mark.parametrize('dims,c,with_offset', C.AFFINE_CASES)
def test_channel_affine(be, dims, c, with_offset):
    C.check_channel_affine(be, dims, c, with_offset)


@pytest.mark.parametrize('n,denom,noise', C.REAL_PREP_CASES)
def test_real_prep(be, n, denom, noise):
    C.check_real_prep(be, n, denom, noise)


@pytest.mark.parametrize('b,d', C.INTERP_CASES)
def test_interpolate(be, b, d):
    C.check_interpolate(be, b, d)


# ------------------------------------------------------------------------------------------------------------------------------------ column sums
def _colsum(K, rows, cols, ld):
    from ctgan_amd._lib import check, lib
    buf, ref, mag = C.colsum_inputs(rows, cols, ld)
    x = buf.cuda()
    out = torch.full((cols + 8,), C.SENTINEL, device='cuda')
    nb = lib.ctgan_colsum_workspace_bytes(rows, cols)
    assert nb == C.colsum_plan(rows)[0] * cols * 4
    ws = torch.empty(nb, dtype=torch.uint8, device='cuda')
    check(lib.ctgan_colsum(K._ptr(x), rows, cols, ld, K._ptr(out), K._ptr(ws), nb, K._stream()), 'colsum')
    torch.cuda.synchronize()
    assert (out[cols:] == C.SENTINEL).all()
    C.within('colsum', out[:cols], ref, mag, C.colsum_d(rows))


@pytest.mark.parametrize('rows,cols', C.COLSUM_CASES)
def test_colsum(K, rows, cols):
    """colsum_stage_kernel through the C ABI: one stage (rows <= 256), two, the 256-block cap (rows > 65536), the 32-row unroll boundary."""
    _colsum(K, rows, cols, cols)


@pytest.mark.parametrize('rows,cols', [(33, 65), (257, 63)])
def test_colsum_with_a_row_stride(K, rows, cols):
    _colsum(K, rows, cols, cols + 3)


@pytest.mark.parametrize('layout', ['nchw', 'cl'])
def test_colsum_channels(be, layout):
    C.check_colsum_channels(be, layout)


# ------------------------------------------------------------------------------------------------------------------------------------ filters
@pytest.mark.parametrize('flip', [False, True])
@pytest.mark.parametrize('R,S,Cc,Kc', C.SPREAD_FILTERS)
def test_filter_spread_fold(be, R, S, Cc, Kc, flip):
    C.check_spread_fold(be, R, S, Cc, Kc, flip)


@pytest.mark.parametrize('shape', C.BATCH_FILTERS)
def test_filter_batch(be, shape):
    """filter_batch_kernel: every kind x pre on one filter, PHASES at all four pads, into sentinel-guarded destinations."""
    C.check_filter_jobs(be, C.filter_jobs([shape]))


def test_filter_batch_two_launches(be):
    jobs = C.filter_jobs(C.BATCH_FILTERS[2:5])[:41]
    assert len(jobs) == 41
    C.check_filter_jobs(be, jobs)


def test_filter_fold_batch(be):
    """filter_fold_batch_kernel: a job longer than one pass of its 1024 blocks beside a 1x1 job; 17 jobs (two launches)."""
    C.check_fold_jobs(be, C.FOLD_BIG)
    C.check_fold_jobs(be, C.FOLD_MANY)


# ------------------------------------------------------------------------------------------------------------------------------------ small linear
@pytest.mark.parametrize('N,Cc,Kc,xhow,whow,kernel', C.LIN_FWD_CASES, ids=C.LIN_FWD_IDS)
def test_small_linear_fwd(be, N, Cc, Kc, xhow, whow, kernel):
    """linear_small_fwd_kernel / linear_gemv_fwd_kernel with and without bias and ReLU; each case asserts the kernel name it must report."""
    C.check_lin_fwd(be, N, Cc, Kc, xhow, whow, kernel)


@pytest.mark.parametrize('N,Cc,Kc,kernel', C.LIN_FWD_LARGE)
def test_small_linear_fwd_row_limit(be, N, Cc, Kc, kernel):
    C.check_lin_fwd(be, N, Cc, Kc, 'dense', 'dense', kernel, combos=((True, False), (False, False)))


@pytest.mark.parametrize('N,Cc,Kc,kernel', C.LIN_DGRAD_CASES)
def test_small_linear_dgrad(be, N, Cc, Kc, kernel):
    C.check_lin_dgrad(be, N, Cc, Kc, kernel)


@pytest.mark.parametrize('with_bias', [False, True])
@pytest.mark.parametrize('rows', C.LIN_WGRAD_ROWS)
def test_small_linear_wgrad(be, rows, with_bias):
    C.check_lin_wgrad(be, rows, with_bias)


@pytest.mark.parametrize('with_bias', [False, True])
def test_small_linear_wgrad_strided_gy_and_fall_through(be, with_bias):
    C.check_lin_wgrad(be, 17, with_bias, C=65, K=10, gy_slice=True)
    C.check_lin_wgrad(be, 5, with_bias, C=128, K=17, kernel=None)


# ------------------------------------------------------------------------------------------------------------------------------------ refusals
def _refusals(K):
    """name -> (C entry point, arguments, outputs): each names one `return ctgan_fail` of elementwise.hip's entry points.  All of them are
    argument checks that return before any launch; the outputs are filled with a sentinel."""
    from ctgan_amd._lib import FilterJob, FoldJob, I32x4, I64x4
    p, st = K._ptr, K._stream()
    keep, R = [], {}

    def sent(k):
        keep.append(torch.full((k + 8,), C.SENTINEL, device='cuda'))
        return keep[-1]

    def rnd(k):
        keep.append(torch.rand(k + 8, device='cuda'))
        return keep[-1]

    y = sent(16)
    R['lrelu_fwd n < 0'] = ('ctgan_lrelu_fwd', [p(rnd(16)), p(y), -1, 0.2, st], [y])
    R['lrelu_fwd null x'] = ('ctgan_lrelu_fwd', [None, p(y), 16, 0.2, st], [y])
    R['lrelu_bwd n < 0'] = ('ctgan_lrelu_bwd', [p(rnd(16)), p(rnd(16)), p(y), -1, 0.2, st], [y])
    R['lrelu_bwd null ref'] = ('ctgan_lrelu_bwd', [p(rnd(16)), None, p(y), 16, 0.2, st], [y])
    for name, kp in (('0', 0.0), ('above 1', 1.5), ('NaN', float('nan'))):
        R['dropout keep ' + name] = ('ctgan_dropout', [p(rnd(16)), p(rnd(16)), p(y), 16, kp, st], [y])
    xs, ys = I64x4(4, 4, 2, 1), I64x4(12, 12, 4, 1)
    keep.extend([xs, ys])
    R['upsample2 odd output'] = ('ctgan_upsample2', [p(rnd(16)), xs, p(y), ys, I32x4(1, 1, 3, 4), 1.0, st], [y])
    R['sample_sum n = 0'] = ('ctgan_sample_sum', [p(rnd(16)), p(y), 0, 16, 1.0, st], [y])
    R['sample_sum m = 0'] = ('ctgan_sample_sum', [p(rnd(16)), p(y), 1, 0, 1.0, st], [y])
    R['spatial_sum hw = 0'] = ('ctgan_spatial_sum', [p(rnd(16)), p(y), 1, 0, 4, 1.0, st], [y])
    R['spatial_sum c = 0'] = ('ctgan_spatial_sum', [p(rnd(16)), p(y), 1, 4, 0, 1.0, st], [y])
    R['channel_affine rows = 0'] = ('ctgan_channel_affine', [p(rnd(16)), p(rnd(4)), None, p(y), 0, 4, st], [y])
    R['channel_affine c = 0'] = ('ctgan_channel_affine', [p(rnd(16)), p(rnd(4)), None, p(y), 4, 0, st], [y])
    R['interpolate b = 0'] = ('ctgan_interpolate', [p(rnd(16)), p(rnd(16)), p(rnd(4)), p(y), 0, 4, st], [y])
    R['interpolate d = 0'] = ('ctgan_interpolate', [p(rnd(16)), p(rnd(16)), p(rnd(4)), p(y), 4, 0, st], [y])
    xi = torch.zeros(16, dtype=torch.int32, device='cuda')
    keep.append(xi)
    R['real_prep denom = 0'] = ('ctgan_real_prep', [p(xi), None, p(y), 16, 0.0, st], [y])
    ws = sent(2 * 4)
    R['colsum workspace one byte short'] = ('ctgan_colsum', [p(rnd(300 * 4)), 300, 4, 4, p(y), p(ws), 2 * 4 * 4 - 1, st], [y, ws])
    w = rnd(3 * 3 * 4 * 4)

    def fjob(name, dst, kind, pre):
        arr = (FilterJob * 1)(FilterJob(w.data_ptr(), dst.data_ptr() if dst is not None else None, 3, 3, 4, 4, kind, 0, 0, 1.0, pre, 1.0))
        keep.append(arr)
        R['filter_batch ' + name] = ('ctgan_filter_batch', [arr, 1, st], [y])
    fjob('kind = 4', y, 4, 0); fjob('kind = -1', y, -1, 0); fjob('pre on a SPREAD kind', y, C.SPREAD, C.SPREAD)
    fjob('pre out of range', y, C.ROTATE, 1); fjob('null dst', None, C.ROTATE, 0)
    arr = (FoldJob * 1)(FoldJob(w.data_ptr(), y.data_ptr(), 0, 3, 4, 4, 1.0, 0))
    keep.append(arr)
    R['filter_fold_batch R = 0'] = ('ctgan_filter_fold_batch', [arr, 1, st], [y])
    R['filter_spread C = 0'] = ('ctgan_filter_spread', [p(w), p(y), 3, 3, 0, 4, 1.0, 0, st], [y])
    R['filter_spread null w'] = ('ctgan_filter_spread', [None, p(y), 1, 1, 2, 2, 1.0, 0, st], [y])
    R['filter_fold S = 0'] = ('ctgan_filter_fold', [p(w), p(y), 1, 0, 2, 2, 1.0, 1, st], [y])
    R['filter_fold null out'] = ('ctgan_filter_fold', [p(w), None, 1, 1, 2, 2, 1.0, 0, st], [y])
    return R, keep


def test_entry_points_refuse_before_any_launch(K):
    """Each refusal returns CTGAN_E_BADARG (the ValueError of test_errors_surface_as_python_exceptions) and writes nothing."""
    from ctgan_amd._lib import check, lib
    R, keep = _refusals(K)
    assert len(R) >= 28
    for name, (fn, args, outs) in R.items():
        rc = getattr(lib, fn)(*args)
        assert rc == -1, (name, rc)
        with pytest.raises(ValueError):
            check(rc, name)
    torch.cuda.synchronize()
    for name, (fn, args, outs) in R.items():
        for o in outs:
            assert (o == C.SENTINEL).all(), name
