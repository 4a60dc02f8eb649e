"""Every Philox-drawing entry point of ctgan_amd.kernels against the numpy generator (oracle/philox.py through the written-once
specification tests/philox_spec.py), element for element, at the key, counter and size corners (`-m gpu`).

The corners (philox_spec.CORNERS): A = the suite's first anchor; B = a 64-bit seed, a stream id with rank bits and a step past 2^32
(high key word, `rank << 16` and counter word 3 all non-zero); C = every word saturated.  The sizes (philox_spec.SIZES) end in
2,097,157 = 4*256*2048 + 5, the smallest at which a lane of the capped grid takes a second block and a ragged tail exists.  The case
tables live in tests/philox_checks.py and run against the CPU stand-ins as well (tests/test_philox_standins.py).

Draws, labels, keep/drop patterns and kept values are compared bit for bit; rng_normal, critic_prep and the one (lo, hi) pair whose
scaling a fused multiply-add rounds differently are compared with a float64 evaluation under bounds derived in philox_checks."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import philox_checks as C  # noqa: E402
from tests import philox_spec as S  # noqa: E402

CORNERS = sorted(S.CORNERS)


@pytest.fixture(scope='module')
def be():
    import ctgan_amd.kernels as K
    b = C.Backend(K, 'cuda', exact=True)
    yield b
    print('largest observed distances:', {k: '%.3g' % v for k, v in sorted(b.seen.items())})


@pytest.mark.parametrize('n', S.SIZES)
@pytest.mark.parametrize('corner', CORNERS)
def test_uniform_is_the_numpy_stream(be, corner, n):
    C.check_uniform(be, corner, n)


@pytest.mark.parametrize('corner', CORNERS)
def test_uniform_indexes_a_channels_last_tensor_by_its_physical_element(be, corner):
    C.check_uniform_channels_last(be, corner)


@pytest.mark.parametrize('n', C.NORMAL_SIZES)
@pytest.mark.parametrize('corner', CORNERS)
def test_normal_is_box_muller_on_the_numpy_stream(be, corner, n):
    """Element by element against the float64 Box-Muller pair; tolerance 4 d_ref = 9.28e-7 (philox_checks.D_REF: measured, 2.31e-7)."""
    C.check_normal(be, corner, n, C.DEVICE_NORMAL_TOL)


@pytest.mark.parametrize('n', S.SIZES)
@pytest.mark.parametrize('corner', CORNERS)
def test_labels_are_the_numpy_labels(be, corner, n):
    C.check_labels(be, corner, n)


@pytest.mark.parametrize('n', S.SIZES)
@pytest.mark.parametrize('corner', CORNERS)
def test_dropout_family_on_aligned_and_misaligned_tensors(be, corner, n):
    """dropout_rng, lrelu_dropout_rng and dropout_rng_mask: the 16-byte-aligned tensor takes the float4 body (and the scalar one for a
    ragged tail), the view base[1:1+n] the scalar fallback."""
    C.check_dropouts_1d(be, corner, n)


@pytest.mark.parametrize('corner', CORNERS)
def test_dropout_family_on_a_channels_last_tensor(be, corner):
    C.check_dropouts_channels_last(be, corner)


@pytest.mark.parametrize('n1_rows', [0, 2, 5])
@pytest.mark.parametrize('corner', CORNERS)
def test_two_stream_lrelu_dropout(be, corner, n1_rows):
    C.check_lrelu_dropout2(be, corner, n1_rows)


def test_two_stream_lrelu_dropout_refuses_a_split_inside_a_block(be):
    x = torch.randn(3, 6, device='cuda')
    with pytest.raises(ValueError):
        be.K.lrelu_dropout_rng2(x, x, 1, 0.2, 0.5, 1, 2, 3, be.ctr(0))          # n1 = 6: not a multiple of 4


@pytest.mark.parametrize('denom', [256.0, 255.0])
@pytest.mark.parametrize('B,d', [(5, 8), (7, 3072)])
@pytest.mark.parametrize('corner', ['A', 'B'])
def test_critic_prep(be, corner, B, d, denom):
    """B = 5 and B = 7 put alpha rows on every lane of a Philox block and into a second block."""
    C.check_critic_prep(be, corner, B, d, denom)


@pytest.mark.parametrize('shape', C.ROW_SHAPES)
@pytest.mark.parametrize('corner', ['A', 'B'])
def test_rows_cat_dropout_and_its_adjoint(be, corner, shape):
    C.check_rows_cat(be, corner, shape)


@pytest.mark.parametrize('shape', C.ROW_SHAPES)
def test_rows_gather_dropout_with_six_segments(be, shape):
    C.check_rows_gather(be, 'B', shape)


def test_counter_carries_into_the_high_word(be):
    C.check_counter_arithmetic(be)


def test_keep_one_keeps_every_element_as_it_is(be):
    """keep = 1 is inside the documented (0,1].  Before the fix the five entry points computed floorf(1.0f + u) = 2 for u = 1 - 2^-24
    and returned the element doubled (K.dropout(x, u, 1.0) gave 2 x there); they return x bit for bit now."""
    C.check_keep_one(be)


# ------------------------------------------------------------------------------------------------------------- conv epilogues
def _conv_inputs(be, N, Cin, H, Ko, k, seed, scale):
    r = np.random.RandomState(seed)
    x = be.cl(r.standard_normal((N, Cin, H, H)).astype(np.float32))
    w = be.dev((r.standard_normal((k, k, Cin, Ko)) * scale).astype(np.float32))
    b = be.dev(r.standard_normal(Ko).astype(np.float32))
    return x, w, b


def _assert_ranges(be, y, y0, ranges, seed, step, what):
    """Every sample range of y = the specification's dropout of the same rows of the undropped launch y0, indexed from the range's own
    first element; a keep-1 range is y0 itself."""
    r0 = 0
    for end, (keep, sid) in ranges:
        part = C.phys(y0[r0:end])
        want, kept = S.dropout(part, keep, seed, sid, step)
        C.assert_dropped(be, C.phys(y[r0:end]), want, kept, part != 0, (what, r0, end, keep))
        if keep >= 1.0:
            assert C.same_bits(C.phys(y[r0:end]), part), (what, 'keep-1 range')
        r0 = end
    assert r0 == y.shape[0]


def test_fp32_conv_epilogue_dropout_in_three_row_ranges(be):
    """The fp32 family's epilogue dropout at corner B, three sample ranges of one launch (the middle one with keep 1: its host drops the
    dropout), against the numpy specification applied to the same launch without dropout."""
    K = be.K
    seed, sid, step = S.CORNERS['B']
    ctr = be.ctr(step)
    geom = K.ConvGeom(128, 8, 8, 128, 3, 3, 1, False)
    x, w, b = _conv_inputs(be, 5, 128, 8, 128, 3, 31, 0.03)
    r = be.cl(np.random.RandomState(32).standard_normal((5, 128, 8, 8)).astype(np.float32))
    ranges = [(2, (0.5, sid)), (4, (1.0, sid + 1)), (5, (0.8, sid + 4))]
    hybrid, K.X3_HYBRID = K.X3_HYBRID, False                 # the fp32 family itself, not the split mode large layers are routed to
    try:
        for relu in (False, True):
            y0 = K.conv_fwd(x, w, b, geom, resid=r, relu=relu, relu_in=True)
            assert K.last_kernel().startswith('igemm'), K.last_kernel()
            y = K.conv_fwd(x, w, b, geom, resid=r, relu=relu, relu_in=True,
                           drop={'ranges': [(end, (keep, seed, s, ctr)) for end, (keep, s) in ranges]})
            assert K.last_kernel().startswith('igemm'), K.last_kernel()      # the epilogue, not a dropout launch of its own
            _assert_ranges(be, y, y0, ranges, seed, step, 'igemm relu=%s' % relu)
            one = K.conv_fwd(x, w, b, geom, resid=r, relu=relu, relu_in=True, drop=(0.3, seed, sid, ctr))
            assert K.last_kernel().startswith('igemm'), K.last_kernel()
            _assert_ranges(be, one, y0, [(5, (0.3, sid))], seed, step, 'igemm one spec relu=%s' % relu)
    finally:
        K.X3_HYBRID = hybrid


@pytest.mark.parametrize('ranged', [False, True])
def test_f32x3_halo_kernel_epilogue_dropout(be, ranged):
    """The split mode's halo-patch kernel at corner B on the geometry of test_gpu_kernels16's epilogue-dropout test: the launch with
    dropout = the specification applied to the same launch with every keep at 1 (which its host turns into no dropout)."""
    K = be.K
    seed, sid, step = S.CORNERS['B']
    ctr = be.ctr(step)
    N, Cin, H, Ko = 384, 32, 8, 128
    geom = K.ConvGeom(Cin, H, H, Ko, 3, 3, 1, False)
    x, w, b = _conv_inputs(be, N, Cin, H, Ko, 3, 13, 1.0 / 17)
    ranges = [(128, (0.5, sid)), (192, (1.0, sid + 1)), (384, (0.8, sid + 4))] if ranged else [(384, (0.5, sid))]

    def drop(keeps_one):
        specs = [(end, (1.0 if keeps_one else keep, seed, s, ctr)) for end, (keep, s) in ranges]
        return {'ranges': specs} if ranged or keeps_one else specs[0][1]      # (ranges always take the halo-patch kernel, dropping or not)
    try:
        with K.mma_dtype('f32x3'):
            y0 = K.conv_fwd(x, w, b, geom, relu=True, relu_in=True, drop=drop(True))
            k0 = K.last_kernel()
            y = K.conv_fwd(x, w, b, geom, relu=True, relu_in=True, drop=drop(False))
            assert K.last_kernel().startswith('conv16x3h') and K.last_kernel() == k0, (k0, K.last_kernel())
            plain = K.conv_fwd(x, w, b, geom, relu=True, relu_in=True)
            kp = K.last_kernel()
    finally:
        K.set_mma_dtype(None)
    # keep 1 is no dropout: the launch without an epilogue extension, bit for bit where it is the same kernel (otherwise to the 2e-6 of
    # max |y| that test_gpu_kernels16 allows between kernels of this mode; a doubled element is off by its own size)
    if kp == k0:
        assert torch.equal(y0, plain)
    else:
        print('plain launch on', kp, 'keep-1 launch on', k0)
        assert ((y0 - plain).abs().max() / plain.abs().max()).item() < 2e-6
    _assert_ranges(be, y, y0, ranges, seed, step, 'conv16x3h ranged=%s' % ranged)
    assert 0.2 < (y == 0).float().mean().item() < 0.9


def test_bf16_fused_lrelu_dropout_epilogue(be):
    """The LeakyReLU + dropout pair inside the 16-bit slice kernels' epilogue at corner B, on the smallest geometry of
    test_gpu_kernels16's test of it: forward with one stream and with two sample ranges (the second indexed from its own first element),
    and the pair's backward on the data gradient - each the specification applied to the plain conv."""
    K = be.K
    seed, sid, step = S.CORNERS['B']
    ctr = be.ctr(step)
    N, Cin, H, Ko, k = 12, 64, 16, 96, 3
    geom = K.ConvGeom(Cin, H, H, Ko, k, k, 1)
    x, w, b = _conv_inputs(be, N, Cin, H, Ko, k, 21, 1.0 / (k * Cin ** 0.5))
    b = b * 0.1
    n1, sid2 = 9, sid + 4
    r = np.random.RandomState(22)
    gy = be.cl(r.standard_normal((N, Ko, geom.P, geom.Q)).astype(np.float32))
    ref = be.cl(r.standard_normal((N, Cin, H, H)).astype(np.float32))
    K.set_mma_dtype('bf16')
    try:
        assert K.ACT_EPILOGUE
        c = K.conv_fwd(x, w, b, geom)
        cp = C.phys(c)
        row = c[0].numel()
        for keep in (0.5, 0.8):
            y = K.conv_fwd(x, w, b, geom, act={'alpha': 0.2, 'ref': None, 'drop': (keep, seed, sid, ctr)})
            assert 'conv16' in K.last_kernel(), K.last_kernel()
            want, kept = S.lrelu_dropout(cp, cp, 0.2, keep, seed, sid, step)
            C.assert_dropped(be, C.phys(y), want, kept, cp != 0, ('act fwd', keep))
            y2 = K.conv_fwd(x, w, b, geom, act={'alpha': 0.2, 'ref': None,
                                               'drop': {'ranges': [(n1, (keep, seed, sid, ctr)), (N, (keep, seed, sid2, ctr))]}})
            assert 'conv16' in K.last_kernel(), K.last_kernel()
            want2, kept2 = S.lrelu_dropout2(cp, cp, n1 * row, 0.2, keep, seed, sid, sid2, step)
            C.assert_dropped(be, C.phys(y2), want2, kept2, cp != 0, ('act fwd two ranges', keep))
        plain = K.conv_dgrad(gy, w, geom, N)
        dx = K.conv_dgrad(gy, w, geom, N, act={'alpha': 0.2, 'ref': ref, 'drop': (0.5, seed, sid, ctr)})
        assert 'conv16' in K.last_kernel(), K.last_kernel()
        want, kept = S.lrelu_dropout(C.phys(plain), C.phys(ref), 0.2, 0.5, seed, sid, step)
        C.assert_dropped(be, C.phys(dx), want, kept, C.phys(plain) != 0, 'act bwd')
    finally:
        K.set_mma_dtype(None)
