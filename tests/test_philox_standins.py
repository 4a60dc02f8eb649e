"""The CPU stand-ins of tests/cpu_kernels.py against the written-once specification tests/philox_spec.py, on the case tables that
tests/test_gpu_philox_streams.py runs on the device (tests/philox_checks.py).  No GPU.

The host tests and the golden fixtures rest on these stand-ins, so they are pinned to the contract the HIP kernels are pinned to: draws,
labels and keep/drop patterns exact at the key, counter and size corners; kept values to 2^-23 relative (the stand-in divides by keep
where the kernels multiply by float32(1/keep)).  The 2,097,157-element size (a second block per lane on the device) is included once
per entry point."""
import numpy as np
import pytest
import torch

from oracle import philox
from tests import philox_checks as C
from tests import philox_spec as S

SMALL = S.SIZES[:-1]
BIG = S.SIZES[-1]
CORNERS = sorted(S.CORNERS)


@pytest.fixture
def be(cpu_kernels):
    return C.Backend(cpu_kernels, 'cpu', exact=False)


def test_specification_restates_the_oracle_streams():
    """philox_spec keeps its streams between cases and restates labels and the Box-Muller pair: both are oracle.philox's."""
    assert [hex(v) for v in philox.philox_blocks(0, 0, 0, 1)[0]] == ['0x6627e8d5', '0xe169c58d', '0xbc57ac4c', '0x9b00dbd8']
    for corner in CORNERS:
        seed, sid, step = S.CORNERS[corner]
        assert np.array_equal(S.uniform(seed, sid, step, 1001), philox.uniform(seed, sid, step, 1001))
        assert np.array_equal(S.uniform(seed, sid, step, 37, first=964), philox.uniform(seed, sid, step, 1001)[964:])
        for nlab in C.LABEL_COUNTS:
            assert np.array_equal(S.labels(seed, sid, step, 1001, nlab), philox.labels(seed, sid, step, 1001, nlab))
    # the three corners are three different streams, and every word of the key and the counter matters
    seed, sid, step = S.CORNERS['B']
    base = S.uniform(seed, sid, step, 64)
    for other in ((seed & 0xffffffff, sid, step), (seed, sid & 0xffff, step), (seed, sid, step & 0xffffffff)):
        assert not np.array_equal(philox.uniform(*other, 64), base)
    # dropout reports the pattern separately, and keep = 1 keeps everything although floor(1.0f + u) is 2 for the largest u
    x = np.arange(1, 9, dtype=np.float32)
    u = np.array([S.U_MAX, 0, 0.5, 0.19, 0.21, 0.79, 0.81, S.U_MAX], dtype=np.float32)
    y, kept = S.dropout_given_u(x, u, 0.8)
    assert kept.tolist() == [True, False, True, False, True, True, True, True] and np.array_equal(y != 0, kept)
    assert np.array_equal(y[kept], (x * (np.float32(1) / np.float32(0.8)))[kept])
    y1, k1 = S.dropout_given_u(x, u, 1.0)
    assert k1.all() and np.array_equal(y1, x)


def test_d_ref_is_what_the_float32_oracle_is_away_from_the_float64_pair():
    """philox_checks.D_REF, the figure the device tolerance of rng_normal is 4 times of, measured again on this machine."""
    worst = 0.0
    for corner in CORNERS:
        seed, sid, step = S.CORNERS[corner]
        for n in C.NORMAL_SIZES:
            worst = max(worst, S.normal_distance(philox.normal(seed, sid, step, n), S.normal64(seed, sid, step, n)))
    print('d_ref measured %.4g, constant %.4g' % (worst, C.D_REF))
    assert 0.5 * C.D_REF < worst <= C.D_REF
    # wrong by order 1 where it matters: a swapped pair, the other lane pair, u1 without its half-step offset at the smallest draw
    seed, sid, step = S.CORNERS['B']
    ref = S.normal64(seed, sid, step, 1000)
    assert S.normal_distance(ref.reshape(-1, 2)[:, ::-1].reshape(-1), ref) > 0.5
    assert S.normal_distance(ref.reshape(-1, 2, 2)[:, ::-1].reshape(-1), ref) > 0.5


@pytest.mark.parametrize('n', SMALL)
@pytest.mark.parametrize('corner', CORNERS)
def test_uniform(be, corner, n):
    C.check_uniform(be, corner, n)


@pytest.mark.parametrize('corner', CORNERS)
def test_uniform_channels_last(be, corner):
    C.check_uniform_channels_last(be, corner)


@pytest.mark.parametrize('n', C.NORMAL_SIZES[:-1])
@pytest.mark.parametrize('corner', CORNERS)
def test_normal(be, corner, n):
    C.check_normal(be, corner, n, C.D_REF)          # the stand-in IS the float32 oracle: d_ref itself, not the device's 4 d_ref


@pytest.mark.parametrize('n', SMALL)
@pytest.mark.parametrize('corner', CORNERS)
def test_labels(be, corner, n):
    C.check_labels(be, corner, n)


@pytest.mark.parametrize('n', SMALL)
@pytest.mark.parametrize('corner', CORNERS)
def test_dropout_family(be, corner, n):
    C.check_dropouts_1d(be, corner, n)


@pytest.mark.parametrize('corner', CORNERS)
def test_dropout_family_channels_last(be, corner):
    C.check_dropouts_channels_last(be, corner)


@pytest.mark.parametrize('what', ['uniform', 'normal', 'labels', 'dropout'])
def test_the_size_of_a_second_block_per_lane(be, what):
    if what == 'uniform':
        C.check_uniform(be, 'B', BIG)
    elif what == 'normal':
        C.check_normal(be, 'B', BIG, C.D_REF)
    elif what == 'labels':
        C.check_labels(be, 'B', BIG)
    else:
        C.check_dropouts_1d(be, 'B', BIG, keeps=(0.8,))


@pytest.mark.parametrize('n1_rows', [0, 2, 5])
@pytest.mark.parametrize('corner', CORNERS)
def test_two_stream_lrelu_dropout(be, corner, n1_rows):
    C.check_lrelu_dropout2(be, corner, n1_rows)


@pytest.mark.parametrize('denom', [256.0, 255.0])
@pytest.mark.parametrize('B,d', [(5, 8), (7, 3072)])
@pytest.mark.parametrize('corner', ['A', 'B'])
def test_critic_prep(be, corner, B, d, denom):
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
    C.check_keep_one(be)
    # the stand-in's own arithmetic would have doubled the element
    x, u = torch.tensor([3.0]), torch.tensor([float(S.U_MAX)])
    assert float(x / 1.0 * torch.floor(1.0 + u)) == 6.0
