"""The fp32 torch stand-ins of the Layernorm wrappers (tests/cpu_kernels.py, tests/cond_layernorm_cpu_kernels.py: every host-logic test of the
layer-normalised critics runs on them) against the fp64 references of tests/layernorm_cases.py, over the case tables of
tests/test_gpu_layernorm_paths.py - that module's twin on the CPU.  The references, the ReLU input condition and the bounds are checked here
before a GPU sees them, and a stand-in that disagrees with its kernel's definition is caught.  Left out is what a stand-in has no notion of: the
C ABI refusals, the workspace guard and the bit-equality contracts (where the GPU module asserts equal bits, the stand-ins are held to the
bound of that output instead).

Largest figures measured: see DESIGN.md section 24.
"""
import pytest
import torch

from tests import layernorm_cases as C
from tests.cond_layernorm_cpu_kernels import cond_cpu_kernels  # noqa: F401


@pytest.fixture
def be(cond_cpu_kernels):  # noqa: F811
    import ctgan_amd.functional as F
    import ctgan_amd.kernels as K
    return C.Backend(K, F, 'cpu')


@pytest.fixture(scope='module', autouse=True)
def _report():
    C.MEASURED.clear()
    yield
    print('\nLayernorm stand-ins, largest figures against fp64:\n' + C.report())


def _ids(cases):
    return [c.id for c in cases]


def test_case_tables_reach_what_they_claim():
    """The branches the tables promise, computed from the constants of layernorm.hip."""
    ids = _ids(C.ALL_CASES)
    assert len(set(ids)) == len(ids)
    geo = {c.shape: c for c in C.GEOMETRY}
    assert [geo[s].D for s in C.GEOMETRY_SHAPES[:6]] == [4, 24, 1024, 1040, 16384, 16388]
    assert [C.chunks_of(geo[s].D) for s in C.GEOMETRY_SHAPES] == [1, 1, 1, 1, 1, 2, 2, 1, 1, 2, 1, 8]
    assert all(C.ln_ok(c.D, c.C) for c in C.ALL_CASES) and {4, 8, 16, 32, 128, 512, 1024} <= {c.C for c in C.ALL_CASES}
    # the 4 x 16-row unrolled loop of ln_rows_reduce_kernel is entered from 49 rows; 113 = 64 + 49: twice by row lane 0, with a tail
    rows = sorted({c.N * C.chunks_of(c.D) for c in C.ROWS})
    assert rows == [15, 16, 17, 48, 49, 64, 65, 66, 113] and sum(r > 3 * C.RLN for r in rows) == 5
    assert {c.labels for c in C.ROWS} == {None, ('cycle', 10), ('cycle', 1), ('cycle', 1000)}
    for c in C.BAD_LABELS:
        L, lab = C.make_labels(c.labels, c.N, C.gen('t'))
        assert {-1, C.I32_MIN, L, C.I32_MAX} <= set(lab.tolist()) and any(0 <= v < L for v in lab.tolist())
    assert C.ws_bytes(2, 16388, 4) == 2 * 2 * 40 + 2 * 2 * 2 * 4 * 4
    assert C.param_d(4) == 16 + 256 and C.param_d(1024) == 16 + 1
    # the clamp cases: ten constants per case whose squares do not add up exactly in fp64 (at every D of the table), eps far below that noise
    for c in C.CLAMP:
        ref = C.reference(c)
        assert int(ref.const.sum()) == len(C.INEXACT_CONSTANTS) == 10 and not ref.exact.any() and c.eps <= 1e-12
    assert [C.chunks_of(c.D) for c in C.CLAMP[::4][:3]] == [1, 1, 2]


def test_reference_against_the_closed_form_of_a_plain_sample():
    """The autograd references against torch's own layer_norm in fp64 (first order), and the constant sample's exact moments."""
    case = C.Case((3, 8, 16, 16), values='const')
    ref = C.reference(case)
    x = ref.inp.x.double()
    want = torch.nn.functional.layer_norm(x, x.shape[1:], eps=case.eps)
    want = want * ref.inp.scale.double().reshape(1, -1, 1, 1) + ref.inp.offset.double().reshape(1, -1, 1, 1)
    assert (ref.y - want).abs().max() < 1e-11
    assert ref.const.tolist() == [False, True, False] == ref.exact.tolist() and float(ref.mean[1]) == C.CONST_VALUE
    assert abs(float(ref.rstd[1]) - case.eps ** -0.5) < 1e-9


@pytest.mark.parametrize('case', C.GEOMETRY, ids=_ids(C.GEOMETRY))
def test_geometry(be, case):
    C.check_case(be, case)


@pytest.mark.parametrize('case', C.ROWS, ids=_ids(C.ROWS))
def test_row_counts(be, case):
    C.check_case(be, case)


@pytest.mark.parametrize('case', C.BAD_LABELS, ids=_ids(C.BAD_LABELS))
def test_labels_outside_the_table(be, case):
    C.check_case(be, case)


@pytest.mark.parametrize('case', C.VALUES, ids=_ids(C.VALUES))
def test_values(be, case):
    C.check_case(be, case)


@pytest.mark.parametrize('case', C.CLAMP, ids=_ids(C.CLAMP))
def test_constant_samples_under_the_variance_clamp(be, case):
    C.check_case(be, case)


def test_small_shape_after_a_large_one(be):
    C.check_small_after_large(be)


@pytest.mark.parametrize('case', C.SELECT_CASES, ids=_ids(C.SELECT_CASES))
def test_output_selection(be, case):
    C.check_output_selection(be, case)


@pytest.mark.parametrize('case', C.LAYOUT_CASES, ids=_ids(C.LAYOUT_CASES))
def test_layouts(be, case):
    C.check_layouts(be, case)


@pytest.mark.parametrize('labeling', [('cycle', 10), ('cycle', 1), ('bad', 3)], ids=['cycle10', 'one-label', 'bad3'])
@pytest.mark.parametrize('N,Cc', C.ROWS_DIRECT)
def test_rows_gather_and_sum_by_label(be, N, Cc, labeling):
    C.check_rows_direct(be, N, Cc, labeling)
