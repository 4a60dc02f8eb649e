"""Every kernel and host branch of ctgan_amd/csrc/layernorm.hip against the fp64 references of tests/layernorm_cases.py, at the shapes and values
where they can go wrong: one float4 per sample up to 8 chunks, a second chunk of one float4, every channel count from 4 to 1024 with and
without labels (the ownership patterns of channel_rows and the `c < C` guard of the row reductions), 15 to 113 partial rows (the 16 row lanes
and the 4 x 16 unrolled loop of ln_rows_reduce_kernel, entered from 49 rows), label tables of 1, 10 and 1000 rows, labels outside the table,
|mean| >> std (the fp64 moments), a constant sample, eps from 0 to 1, zero and negative scales, an all-zero ReLU mask and an output that is
exactly 0, every output subset of bwd / bwd2, the match_layout branch of the wrappers, the row gather / by-label sum on their own, and every
refusal of the ten entry points.  fwd / bwd / bwd2 are called at the kernel level (K.layernorm_*, K.layernorm_cond_*), bwd / bwd2 with the
product's own mean / rstd, which are checked against fp64 on their own; before every call the cached workspace is filled with 0xFF bytes (NaN
as float and as double), so a partial or a row that is read but not written shows in the output.  The case tables, references, the ReLU input
condition and the bounds are in tests/layernorm_cases.py (DESIGN.md section 24 lists which case reaches which branch);
tests/test_layernorm_standins.py runs the same tables on the fp32 stand-ins.

Largest fraction of its bound that each output used on an MI355X (bounds (U + kappa_n) sum c_i T_i per element, d sum (U + kappa_n) sum |term|
per parameter gradient):
  y 0.37, gx 0.32, cot_gy 0.26, cot_x 0.043        gscale 0.108, goffset 0.133, cot_scale 0.065
  mean 0.999, rstd 0.993, rows_sum_by_label 0.997 (one cast of an fp64 value: the bound is one half-ulp)
(309 tests, 5.1 s; the slowest 0.9 s, the first call of the process.)  The stand-ins' figures are in DESIGN.md section 24.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import layernorm_cases as C  # noqa: E402


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
    print('\nlayernorm.hip, largest figures against fp64:\n' + C.report())


def _ids(cases):
    return [c.id for c in cases]


# ------------------------------------------------------------------------------------------------------------------------------------ values
@pytest.mark.parametrize('case', C.GEOMETRY, ids=_ids(C.GEOMETRY))
def test_geometry(be, case):
    """Chunk geometry and channel ownership at nominal values: D from 4 to 131072, C from 4 to 1024."""
    C.check_case(be, case)


@pytest.mark.parametrize('case', C.ROWS, ids=_ids(C.ROWS))
def test_row_counts(be, case):
    """The column and by-label reductions of the partial rows: around the 16 row lanes and the unrolled loop; absent labels are exact zero rows."""
    C.check_case(be, case)


@pytest.mark.parametrize('case', C.BAD_LABELS, ids=_ids(C.BAD_LABELS))
def test_labels_outside_the_table(be, case):
    """-1, -2^31, n_labels and 2^31 - 1 among valid labels: clamped in table_row and in the by-label reduction."""
    C.check_case(be, case)


@pytest.mark.parametrize('case', C.VALUES, ids=_ids(C.VALUES))
def test_values(be, case):
    C.check_case(be, case)


@pytest.mark.parametrize('case', C.CLAMP, ids=_ids(C.CLAMP))
def test_constant_samples_under_the_variance_clamp(be, case):
    """The `var < 0` clamp of ln_fwd_apply_kernel: ten constant samples per case whose fp64 E[x^2] - mean^2 is rounding noise of either sign,
    far above eps.  Every output is finite, mean and y are exact, rstd is at most 1 / sqrt(eps).  (On the device the noise appears at
    D = 16896 only: 1024 or 2048 equal values add exactly in its power-of-two tree.)"""
    C.check_case(be, case)


def test_small_shape_after_a_large_one(be):
    C.check_small_after_large(be)


@pytest.mark.parametrize('case', C.SELECT_CASES, ids=_ids(C.SELECT_CASES))
def test_output_selection(be, case):
    C.check_output_selection(be, case)


@pytest.mark.parametrize('case', C.LAYOUT_CASES, ids=_ids(C.LAYOUT_CASES))
def test_layouts(be, case):
    C.check_layouts(be, case)


def test_a_non_dense_x_raises(be, K):
    x = torch.randn(2, 8, 8, 8, device='cuda').permute(0, 3, 1, 2)           # [N,C,H,W] = [2,8,8,8], channels-last
    s, o = torch.ones(8, device='cuda'), torch.zeros(8, device='cuda')
    for v in (x[:, :, ::2], x[:, :4], torch.randn(4, 16, device='cuda')[:, ::2]):
        assert not K.layernorm_supported(v)
        with pytest.raises((TypeError, ValueError, AssertionError)):
            K.layernorm_fwd(v, s[:v.shape[1]], o[:v.shape[1]], 1e-5)


def test_past_the_grid_limit_the_operator_is_composed(be, K):
    """65536 samples: layernorm_supported is false and functional.layer_norm composes the operator from the elementwise kernels (two-pass
    moments in fp32 over D = 4: some sixteen roundings on the way to y, against the five of the fused kernel)."""
    case = C.Case((C.GRID_YZ_MAX + 1, 4))
    ref = C.reference(case)
    x = be.dev(ref.inp.x)
    assert not K.layernorm_supported(x)
    with torch.no_grad():
        y = be.F.layer_norm(x, be.dev(ref.inp.scale), be.dev(ref.inp.offset), eps=case.eps)
    C.bounded('y, composed past the grid limit', y, ref.y, 16 / C.C_Y * ref.b_y)


@pytest.mark.parametrize('case', [C.Case((2, 4, 17, 241), relu=True), C.Case((33, 128, 11, 12), labels=('cycle', 10)), C.Case((113, 4), labels=('cycle', 1000))],
                         ids=lambda c: c.id)
def test_two_calls_give_the_same_bits(be, case):
    """Documented as deterministic: identical bits in every output, on a poisoned workspace and with a different-shaped call in between."""
    C.check_determinism(be, case, C.Case((3, 1024), relu=True))


@pytest.mark.parametrize('labeling', [('cycle', 10), ('cycle', 1), ('bad', 3)], ids=['cycle10', 'one-label', 'bad3'])
@pytest.mark.parametrize('N,Cc', C.ROWS_DIRECT)
def test_rows_gather_and_sum_by_label(be, N, Cc, labeling):
    C.check_rows_direct(be, N, Cc, labeling)


# ------------------------------------------------------------------------------------------------------------------------------------ the C ABI
ENTRY = {       # entry point -> (arguments in order, required pointers, outputs)
    'fwd': ('x scale offset y mean rstd N D C eps relu ws wsb st', 'x scale offset y mean rstd', 'y mean rstd'),
    'bwd': ('gy x scale mean rstd ymask gx gscale goffset N D C ws wsb st', 'gy x scale mean rstd gx', 'gx gscale goffset'),
    'bwd2': ('u gy x scale mean rstd ymask cot_gy cot_x cot_scale N D C ws wsb st', 'u gy x scale mean rstd', 'cot_gy cot_x cot_scale'),
    'cond_fwd': ('x scale offset labels L y mean rstd N D C eps relu ws wsb st', 'x scale offset labels y mean rstd', 'y mean rstd'),
    'cond_bwd': ('gy x scale mean rstd ymask labels L gx gscale goffset N D C ws wsb st', 'gy x scale mean rstd labels gx', 'gx gscale goffset'),
    'cond_bwd2': ('u gy x scale mean rstd ymask labels L cot_gy cot_x cot_scale N D C ws wsb st', 'u gy x scale mean rstd labels',
                  'cot_gy cot_x cot_scale'),
}
BIG_N = C.GRID_YZ_MAX + 1


class Pool:
    """Operands large enough for every refused shape ([65536, 4] is the largest), outputs and workspace filled with a sentinel."""

    def __init__(self, K):
        n = BIG_N * 4
        self.K = K
        self.t = {k: torch.rand(n, device='cuda') for k in ('x', 'gy', 'u', 'ymask')}
        self.t.update({k: torch.rand(4096, device='cuda') for k in ('scale', 'offset')})
        self.t['labels'] = torch.zeros(BIG_N, dtype=torch.int32, device='cuda')
        self.inputs = {'mean_in': torch.rand(BIG_N, device='cuda'), 'rstd_in': torch.rand(BIG_N, device='cuda') + 0.5}
        self.out = {k: torch.full((n,), C.SENTINEL, device='cuda') for k in ('y', 'gx', 'cot_gy', 'cot_x')}
        self.out.update({k: torch.full((BIG_N,), C.SENTINEL, device='cuda') for k in ('mean', 'rstd')})
        self.out.update({k: torch.full((4096,), C.SENTINEL, device='cuda') for k in ('gscale', 'goffset', 'cot_scale')})
        self.ws = torch.full((C.ws_bytes(BIG_N, 4, 4) // 4 + 64,), C.SENTINEL, device='cuda')

    def args(self, entry, **over):
        names, _, outs = ENTRY[entry]
        outs = outs.split()
        a = dict(N=4, D=16, C=8, L=3, eps=1e-5, relu=0, st=self.K._stream())
        a.update({k: v for k, v in over.items() if k in a})
        a.setdefault('wsb', over.get('wsb', self.ws.numel() * 4))
        vals = []
        for k in names.split():
            if k in a:
                vals.append(a[k])
                continue
            if k == 'ws':
                t = self.ws
            elif k in outs:
                t = self.out[k]
            elif k in ('mean', 'rstd'):
                t = self.inputs[k + '_in']
            else:
                t = self.t[k]
            if k == 'ymask':
                t = None                                # no fused ReLU
            vals.append(None if k in over and over[k] is None else self.K._ptr(t))
        return vals

    def untouched(self):
        torch.cuda.synchronize()
        return all(bool((t == C.SENTINEL).all()) for t in list(self.out.values()) + [self.ws])


def _refusals():
    """(entry, overrides, code, part of the message)"""
    R = []
    for e, (names, required, outs) in ENTRY.items():
        for c in (0, -4, 2, 6, 12, 40, 2048):
            R.append((e, dict(C=c, D=4 * c if c > 0 else 16), -2, 'outside the fused kernels'))
        R.append((e, dict(C=8, D=12), -2, 'outside the fused kernels'))
        R.append((e, dict(N=0), -1, 'bad argument'))
        R.append((e, dict(N=-3), -1, 'bad argument'))
        for k in required.split():
            R.append((e, {k: None}, -1, 'bad argument'))
        R.append((e, dict(ws=None), -1, 'bad argument'))
        R.append((e, dict(wsb=C.ws_bytes(4, 16, 8) - 1), -1, 'workspace too small'))
        R.append((e, dict(N=3, D=16388, C=4, wsb=C.ws_bytes(3, 16388, 4) - 1), -1, 'workspace too small'))
        R.append((e, dict(N=BIG_N, D=4, C=4), -2, 'launch grid'))
        if e.endswith('bwd'):
            R.append((e, dict(gscale=None), -1, 'bad argument'))
            R.append((e, dict(goffset=None), -1, 'bad argument'))
        if e.startswith('cond'):
            R.append((e, dict(L=0), -1, 'bad argument'))
            R.append((e, dict(L=-1), -1, 'bad argument'))
            R.append((e, dict(L=BIG_N), -2, 'launch grid'))
    return R


def test_supported_and_workspace_bytes(K):
    """ctgan_layernorm_supported on both sides of every condition; the workspace size against a restatement of the partials-plus-rows layout."""
    from ctgan_amd._lib import lib
    for c in (0, -4, 2, 6, 12, 40, 2048):
        assert lib.ctgan_layernorm_supported(4 * c if c > 0 else 16, c) == 0
    assert lib.ctgan_layernorm_supported(12, 8) == 0
    for case in C.ALL_CASES:
        assert lib.ctgan_layernorm_supported(case.D, case.C) == 1
        assert lib.ctgan_layernorm_workspace_bytes(case.N, case.D, case.C) == C.ws_bytes(case.N, case.D, case.C), case.id
    assert lib.ctgan_layernorm_workspace_bytes(BIG_N, 4, 4) == C.ws_bytes(BIG_N, 4, 4)
    assert not K.layernorm_supported(torch.empty(BIG_N, 4, device='cuda')) and K.layernorm_supported(torch.empty(BIG_N - 1, 4, device='cuda'))


def test_entry_points_refuse_before_any_launch(K):
    """Each refusal returns its documented code and message and leaves the sentinel-filled outputs and workspace untouched."""
    from ctgan_amd._lib import check, lib
    pool = Pool(K)
    R = _refusals()
    assert len(R) >= 6 * 21
    for e, over, code, msg in R:
        rc = getattr(lib, 'ctgan_layernorm_' + e)(*pool.args(e, **over))
        err = lib.ctgan_last_error().decode()
        assert rc == code and msg in err and err.startswith('layernorm_' + e + ':'), (e, over, rc, err)
        with pytest.raises(NotImplementedError if code == -2 else ValueError):
            check(rc, e)
    p, st = K._ptr, K._stream()
    tab, lab, out = pool.t['scale'], pool.t['labels'], pool.out['y']
    for fn in ('ctgan_layernorm_rows_gather', 'ctgan_layernorm_rows_sum_by_label'):
        for args in ([None, p(lab), 3, p(out), 4, 8, st], [p(tab), None, 3, p(out), 4, 8, st], [p(tab), p(lab), 3, None, 4, 8, st],
                     [p(tab), p(lab), 0, p(out), 4, 8, st], [p(tab), p(lab), 3, p(out), 0, 8, st], [p(tab), p(lab), 3, p(out), 4, 0, st]):
            assert getattr(lib, fn)(*args) == -1 and 'bad argument' in lib.ctgan_last_error().decode(), (fn, args)
    assert lib.ctgan_layernorm_rows_sum_by_label(p(pool.t['x']), p(lab), BIG_N, p(out), 4, 8, st) == -2
    assert 'launch grid' in lib.ctgan_last_error().decode()
    assert pool.untouched()


@pytest.mark.parametrize('case', [C.Case((3, 4, 17, 241), relu=True), C.Case((3, 4, 17, 241), labels=('cycle', 10), relu=True), C.Case((17, 1024))],
                         ids=lambda c: c.id)
def test_a_workspace_of_exactly_the_queried_size(be, K, case):
    """The entry points given exactly ctgan_layernorm_workspace_bytes inside a larger buffer: the guard region after it stays intact (an overrun
    shows as a failed assertion, not as a fault) and every output has the bits of the wrapper's call."""
    from ctgan_amd._lib import check, lib
    ref, run = C.check_case(be, case)
    N, D, Cc = case.N, case.D, case.C
    need = lib.ctgan_layernorm_workspace_bytes(N, D, Cc)
    guard = 1 << 16
    p, st = K._ptr, K._stream()
    cond = run.labels is not None
    lab = [p(run.labels), ref.inp.L] if cond else []
    pre = 'ctgan_layernorm_cond_' if cond else 'ctgan_layernorm_'
    ymask = p(run.y) if case.relu else None

    def fresh():
        buf = torch.full((need + guard,), 0xA5, dtype=torch.uint8, device='cuda')
        buf[:need] = 0xFF
        return buf

    def intact(buf):
        torch.cuda.synchronize()
        assert (buf[need:] == 0xA5).all(), case.id

    new = lambda t: torch.full_like(t, C.SENTINEL)
    y, mean, rstd = new(run.y), new(run.mean), new(run.rstd)
    ws = fresh()
    check(getattr(lib, pre + 'fwd')(p(run.x), p(run.scale), p(run.offset), *lab, p(y), p(mean), p(rstd), N, D, Cc, case.eps, int(case.relu),
                                   p(ws), need, st), 'fwd')
    intact(ws)
    gx, gs, go = new(run.gx), new(run.gs), new(run.go)
    ws = fresh()
    check(getattr(lib, pre + 'bwd')(p(run.gy), p(run.x), p(run.scale), p(run.mean), p(run.rstd), ymask, *lab, p(gx), p(gs), p(go), N, D, Cc,
                                   p(ws), need, st), 'bwd')
    intact(ws)
    cg, cx, cs = new(run.cg), new(run.cx), new(run.cs)
    ws = fresh()
    check(getattr(lib, pre + 'bwd2')(p(run.u), p(run.gy), p(run.x), p(run.scale), p(run.mean), p(run.rstd), ymask, *lab, p(cg), p(cx), p(cs),
                                    N, D, Cc, p(ws), need, st), 'bwd2')
    intact(ws)
    for name, got in zip(C.OUTPUTS, (y, mean, rstd, gx, gs, go, cg, cx, cs)):
        C.same_bits(name, got, getattr(run, name))
