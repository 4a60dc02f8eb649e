"""The fp32 torch stand-ins of the elementwise, layout, filter and conv wrappers (tests/cpu_kernels.py: every host-logic test runs on them)
against the fp64 references of tests/elementwise_cases.py, over the case tables of tests/test_gpu_elementwise_paths.py - that module's fp32
twin on the CPU.  The references and the input conditions are checked here before a GPU sees them, and a stand-in that disagrees with its
kernel's definition is caught.  Cases that exist for a device branch only (pointer alignment, the grid-stride sizes) stay in: they are cheap.
Left out is what a stand-in has no notion of: the direct C-ABI cases (colsum's `ld`, the refusals), the kernel names, and the PHASES layout of
filter_batch - the stand-in's conv_dgrad multiplies with the rotated filter whatever the stride, and its filter_batch documents that it
fills the head of a phase buffer with that.

Largest figures measured: see DESIGN.md section 23.
"""
import pytest
import torch

from tests import elementwise_cases as C


@pytest.fixture
def be(cpu_kernels):
    import ctgan_amd.functional as F
    import ctgan_amd.kernels as K
    return C.Backend(K, F, 'cpu')


@pytest.fixture(scope='module', autouse=True)
def _report():
    C.MEASURED.clear()
    yield
    print('\nelementwise / small-linear stand-ins, largest figures against fp64:\n' + C.report())


def test_case_tables_reach_what_they_claim():
    """The sizes and shapes the tables promise, computed from the constants of elementwise.hip and skinny.hip."""
    assert C.MAP_BIG > 2048 * 256 * 4 and C.MAP_BIG % 4 and {C.MAP_OPS[n].template for n in C.MAP_BIG_OPS} == {'map1', 'map2'}
    assert {n % 4 for n in C.MAP_SIZES} == {0, 1, 3} and {op.template for op in C.MAP_OPS.values()} == {'map1', 'map2'}
    out = lambda s, f: s[0] * s[1] * int(s[2] * f) * int(s[3] * f)
    assert out(C.POOL_BIG, 0.5) > 4096 * 256 and out(C.UP_BIG, 2) > 4096 * 256
    for m, (c, h, w) in C.SAMPLE_M.items():
        assert c * h * w == m
    for hw, (h, w) in C.SPATIAL_HW.items():
        assert h * w == hw
    # colsum: one stage up to 256 rows, the 256-block cap past 65536, the 8 x 4-row unroll entered by three of the four row lanes at 31 rows, by all at 32, with a tail at 33
    assert C.colsum_plan(256) == (1, 256) and C.colsum_plan(257)[0] == 2 and C.colsum_plan(65536) == (256, 256) and C.colsum_plan(65537) == (256, 257)
    assert all(r * c * 4 <= 70e6 for r, c in C.COLSUM_CASES) and len(C.COLSUM_CASES) == 7 * 5 + 2 * 2
    # filter_batch: both sides of (C | K) & 3, ragged and several 32 x 32 tiles, even and odd taps for PHASES
    F = C.BATCH_FILTERS
    assert any((c | k) & 3 for _, _, c, k in F) and any((c | k) & 3 == 0 and (c % 32 or k % 32) for _, _, c, k in F)
    assert any(c > 64 and k > 64 for _, _, c, k in F) and {4, 5} <= {r for r, _, _, _ in F} and any(r != s for r, s, _, _ in F)
    assert len(C.filter_jobs(C.BATCH_FILTERS[2:5])[:41]) == 41 and len(C.FOLD_MANY) == 17
    assert C.FOLD_BIG[0][0] * C.FOLD_BIG[0][1] * C.FOLD_BIG[0][2] * C.FOLD_BIG[0][3] > 1024 * 256
    # small linear: every condition of the GEMV route from both sides, each expectation restated from ctgan_small_linear_fwd
    for N, Cc, K, xh, wh, kernel in C.LIN_FWD_CASES:
        ld = xh[1] if isinstance(xh, tuple) else Cc
        gemv = K == 1 and Cc % 4 == 0 and Cc >= 1024 and ld % 4 == 0 and xh != 'off16' and wh != 'off16'
        assert kernel == (None if K > 16 else (C.GEMV if gemv else C.ROW)), (N, Cc, K, xh, wh)
    assert {k for *_, k in C.LIN_FWD_CASES} == {C.ROW, C.GEMV, None}


def test_references_against_the_oracle_ops():
    """The restated formulas against oracle/tf_ops.py where it has the operation, and the layouts against each other."""
    import numpy as np
    from oracle import tf_ops
    x = torch.randn(2, 3, 4, 6, dtype=torch.float64, generator=C.gen('ref'))
    assert torch.equal(C.ref_pool2(x, 0.25), tf_ops.mean_pool2(x)) and torch.equal(C.ref_upsample2(x, 1.0), tf_ops.upsample2(x))
    w = np.random.RandomState(0).randn(3, 2, 4, 5)
    # fold is the adjoint of spread, for both orientations; a flipped spread is the rotated layout of the plain one
    for flip in (False, True):
        s = C.np_spread(w, 0.5, flip)
        u = np.random.RandomState(1).randn(*s.shape)
        assert abs((s * u).sum() - (w * C.np_fold(u, 0.5, flip)).sum()) < 1e-12
    assert np.array_equal(C.np_spread(w, 0.5, True), C.np_rotate(C.np_spread(w, 0.5, False)))
    # a 1 x 1 filter has one phase plane per phase, and only the phase of parity (pad_t, pad_l) holds it
    p = C.np_phases(w[:1, :1], 1, 0)
    assert p.shape == (4, 1, 1, 5, 4) and np.array_equal(p[2, 0, 0], w[0, 0].T) and not p[[0, 1, 3]].any()
    # the crafted dropout draws sit on the mask's threshold; the draw just below 1 - keep is kept at keep = 0.5, where the fp32 sum
    # 1 - 2^-25 is a tie that rounds to 1 (in fp64 it would be dropped): the mask is defined by the fp32 addition
    for keep in (0.5, 0.8):
        u = C.dropout_u(8, keep, C.gen('u'))
        assert C.dropout_mask(u, keep)[:4].tolist() == [0.0, 1.0, 1.0, 1.0] and float(u[4]) < 1 - keep
    u = C.dropout_u(8, 0.5, C.gen('u'))
    assert C.dropout_mask(u, 0.5)[4] == 1.0 and np.floor(0.5 + float(u[4])) == 0.0
    assert float(np.float32(1) + np.float32(1 - 2.0 ** -24)) == 2.0 and C.dropout_mask(C.dropout_u(8, 1.0, C.gen('u')), 1.0).eq(1).all()


@pytest.mark.parametrize('n', C.MAP_SIZES)
@pytest.mark.parametrize('name', sorted(C.MAP_OPS))
def test_map(be, name, n):
    C.check_map(be, name, n)


@pytest.mark.parametrize('name', sorted(C.MAP_OPS))
def test_map_misaligned_and_empty(be, name):
    for i in range(C.MAP_OPS[name].nin):
        C.check_map(be, name, 1025, misaligned=i)
    C.check_map_empty(be, name)


@pytest.mark.parametrize('name', C.MAP_BIG_OPS)
def test_map_second_grid_stride_pass(be, name):
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


@pytest.mark.parametrize('layout', ['nchw', 'cl'])
def test_colsum_channels(be, layout):
    C.check_colsum_channels(be, layout)


@pytest.mark.parametrize('flip', [False, True])
@pytest.mark.parametrize('R,S,Cc,K', C.SPREAD_FILTERS)
def test_filter_spread_fold(be, R, S, Cc, K, flip):
    C.check_spread_fold(be, R, S, Cc, K, flip)


@pytest.mark.parametrize('shape', C.BATCH_FILTERS)
def test_filter_batch(be, shape):
    C.check_filter_jobs(be, C.filter_jobs([shape], phases=False))


def test_filter_fold_batch(be):
    C.check_fold_jobs(be, C.FOLD_BIG)
    C.check_fold_jobs(be, C.FOLD_MANY)


@pytest.mark.parametrize('N,Cc,K,xhow,whow,kernel', C.LIN_FWD_CASES, ids=C.LIN_FWD_IDS)
def test_small_linear_fwd(be, N, Cc, K, xhow, whow, kernel):
    C.check_lin_fwd(be, N, Cc, K, xhow, whow, kernel)


@pytest.mark.parametrize('N,Cc,K,kernel', C.LIN_FWD_LARGE)
def test_small_linear_fwd_row_limit(be, N, Cc, K, kernel):
    C.check_lin_fwd(be, N, Cc, K, 'dense', 'dense', kernel, combos=((True, False), (False, False)))


@pytest.mark.parametrize('N,Cc,K,kernel', C.LIN_DGRAD_CASES)
def test_small_linear_dgrad(be, N, Cc, K, kernel):
    C.check_lin_dgrad(be, N, Cc, K, kernel)


@pytest.mark.parametrize('with_bias', [False, True])
@pytest.mark.parametrize('rows', C.LIN_WGRAD_ROWS)
def test_small_linear_wgrad(be, rows, with_bias):
    C.check_lin_wgrad(be, rows, with_bias)


@pytest.mark.parametrize('with_bias', [False, True])
def test_small_linear_wgrad_strided_gy_and_fall_through(be, with_bias):
    C.check_lin_wgrad(be, 17, with_bias, C=65, K=10, gy_slice=True)
    C.check_lin_wgrad(be, 5, with_bias, C=128, K=17, kernel=None)
