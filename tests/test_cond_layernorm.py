"""The label-conditioned Layernorm (LS/tflib/ops/layernorm.py:21-30; csrc/layernorm.hip ctgan_layernorm_cond_{fwd,bwd,bwd2}) against its fp64
restatement (tests/cond_layernorm_oracle.py): values, first-order gradients with respect to x and both tables, then the gradient
penalty mean((||dy/dx|| - 1)^2) differentiated with respect to x, gy and the scale table (the double-backward map).  On the torch-CPU
stand-ins (host wiring) and on the device.  Tolerances are those of tests/test_layernorm.py: relative max error 2e-5 on the stand-ins,
3e-5 on the GPU, 20x for the penalty's second-order gradients."""
import pytest
import torch

from tests import cond_layernorm_oracle as O
from tests.cond_layernorm_cpu_kernels import cond_cpu_kernels  # noqa: F401  (fixture)

SHAPES = [(6, 128, 8, 8),       # one partial chunk, the critic's 8x8 site
          (5, 128, 16, 16),     # D = 32768: two full 16384-element chunks, the 16x16 site
          (3, 8, 48, 48),       # C = 8, the smallest channel-ownership pattern; D = 18432: the second chunk is partial
          (1, 128, 8, 8),       # N = 1
          (5, 256),             # 2-D, fused
          (9, 40)]              # composed fallback (C = 40 is outside the fused kernels)


def _labels(pattern, N):
    """-> (labels list, n_labels)"""
    if pattern == 'distinct':
        return [(3 * i + 1) % 10 for i in range(N)], 10
    if pattern == 'all9':
        return [9] * N, 10
    if pattern == 'only_0_and_9':                    # eight table rows get a zero gradient
        return [9 if i % 2 == 0 else 0 for i in range(N)], 10
    if pattern == 'one_label':
        return [0] * N, 1
    if pattern == 'three_labels_n7':                 # labels repeat
        assert N == 7
        return [2, 0, 1, 1, 2, 0, 2], 3
    if pattern == 'descending':
        return [9 - i for i in range(N)], 10
    raise KeyError(pattern)


def _cases():
    out, seen = [], set()
    for shape in SHAPES:
        for pattern in ('distinct', 'all9', 'only_0_and_9', 'one_label', 'three_labels_n7', 'descending'):
            shp = (7,) + shape[1:] if pattern == 'three_labels_n7' else shape
            if (shp, pattern) not in seen:
                seen.add((shp, pattern))
                out.append((shp, pattern))
    return out


CASES = _cases()
IDS = ['%s-%s' % ('x'.join(map(str, s)), p) for s, p in CASES]


def _rel(a, b):
    a = a.detach().cpu().double(); b = b.detach().cpu().double()
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-30)).item()


def _inputs(shape, pattern, equal_rows=False):
    g = torch.Generator().manual_seed(3)
    lab, L = _labels(pattern, shape[0])
    C = shape[1]
    x = torch.randn(*shape, generator=g) * 1.7 + 0.3
    if equal_rows:
        scale = (torch.rand(1, C, generator=g) + 0.5).expand(L, C).contiguous()
        offset = torch.randn(1, C, generator=g).expand(L, C).contiguous()
    else:
        scale = torch.rand(L, C, generator=g) + 0.5           # drawn at random, not left at ones / zeros
        offset = torch.randn(L, C, generator=g)
    gy = torch.randn(*shape, generator=g)
    return x, scale, offset, torch.tensor(lab, dtype=torch.int32), gy


_REF = {}


def _reference(shape, pattern, relu, equal_rows=False):
    """fp64: (y, gx, gscale, goffset, pen, d pen / d x, d pen / d gy, d pen / d scale); computed once per case and shared."""
    key = (shape, pattern, relu, equal_rows)
    if key not in _REF:
        x, scale, offset, lab, gy = _inputs(shape, pattern, equal_rows)
        xr, sr, orr, gyr = (t.double().requires_grad_(True) for t in (x, scale, offset, gy))
        y = O.layer_norm(xr, sr, orr, lab)
        if relu:
            y = torch.relu(y)
        g1 = torch.autograd.grad(y, [xr, sr, orr], gyr, create_graph=True)
        pen = ((g1[0].reshape(shape[0], -1).pow(2).sum(dim=1).sqrt() - 1) ** 2).mean()
        g2 = torch.autograd.grad(pen, [xr, gyr, sr])
        _REF[key] = tuple(t.detach() for t in (y,) + tuple(g1) + (pen,) + tuple(g2))
    return _REF[key]


def _run(dev, shape, pattern, relu, equal_rows=False, labels=True):
    """The product: -> the same tuple as _reference (labels=False: the unconditional operator on row 0 of the tables)."""
    import ctgan_amd.functional as F
    x, scale, offset, lab, gy = _inputs(shape, pattern, equal_rows)
    if not labels:
        scale, offset = scale[0].contiguous(), offset[0].contiguous()
    if len(shape) == 4:
        x, gy = x.to(dev).contiguous(memory_format=torch.channels_last), gy.to(dev).contiguous(memory_format=torch.channels_last)
    xd, sd, od, gyd = (t.to(dev).requires_grad_(True) for t in (x, scale, offset, gy))
    y = F.layer_norm(xd, sd, od, 1e-5, relu=relu, labels=lab.to(dev) if labels else None)
    g1 = torch.autograd.grad(y, [xd, sd, od], gyd, create_graph=True)
    pen, _ = F.gradient_penalty(g1[0].reshape(shape[0], -1), 1.0)
    g2 = torch.autograd.grad(pen, [xd, gyd, sd])
    return tuple(t.detach() for t in (y,) + tuple(g1) + (pen,) + tuple(g2))


NAMES = ('y', 'gx', 'gscale', 'goffset', 'pen', 'cot_x', 'cot_gy', 'cot_scale')


def _check(dev, shape, pattern, relu, tol):
    got = _run(dev, shape, pattern, relu)
    ref = _reference(shape, pattern, relu)
    errs = {n: _rel(a, b) for n, a, b in zip(NAMES, got, ref)}
    print('%s %s relu=%s: %s' % (shape, pattern, relu, ' '.join('%s=%.2e' % kv for kv in errs.items())))
    for n, a, b in zip(NAMES, got, ref):
        assert tuple(a.shape) == tuple(b.shape), n
    for n in ('y', 'gx', 'gscale', 'goffset'):
        assert errs[n] < tol, (n, errs[n])
    assert abs(got[4].item() - ref[4].item()) < tol * max(1.0, abs(ref[4].item()))
    for n in ('cot_x', 'cot_gy', 'cot_scale'):
        assert errs[n] < 20 * tol, (n, errs[n])
    # gradient rows of labels absent from the batch: written, and exactly zero
    lab, L = _labels(pattern, shape[0])
    absent = [l for l in range(L) if l not in lab]
    for n in ('gscale', 'goffset', 'cot_scale'):
        t = got[NAMES.index(n)].cpu()
        assert tuple(t.shape) == (L, shape[1])
        for l in absent:
            assert torch.equal(t[l], torch.zeros(shape[1])), (n, l)
    # two identical calls: identical bits in every output
    again = _run(dev, shape, pattern, relu)
    for n, a, b in zip(NAMES, got, again):
        assert torch.equal(a, b), n
    return got


@pytest.mark.parametrize('relu', [False, True])
@pytest.mark.parametrize('shape,pattern', CASES, ids=IDS)
def test_cond_layernorm_values_gradients_and_double_backward(cond_cpu_kernels, shape, pattern, relu):
    _check('cpu', shape, pattern, relu, 2e-5)


@pytest.mark.gpu
@pytest.mark.parametrize('relu', [False, True])
@pytest.mark.parametrize('shape,pattern', CASES, ids=IDS)
def test_cond_layernorm_on_gpu(shape, pattern, relu):
    _check('cuda', shape, pattern, relu, 3e-5)


def _equal_rows(dev, shape, pattern, relu, tol, bitwise):
    """Tables whose rows all equal one vector: the operator is the unconditional one."""
    cond = _run(dev, shape, pattern, relu, equal_rows=True)
    plain = _run(dev, shape, pattern, relu, equal_rows=True, labels=False)
    c, p = dict(zip(NAMES, cond)), dict(zip(NAMES, plain))
    for n in ('y', 'gx', 'cot_gy', 'cot_x'):
        if bitwise:
            assert torch.equal(c[n], p[n]), n
        else:
            assert _rel(c[n], p[n]) < (tol if n in ('y', 'gx') else 20 * tol), n
    # the table gradients summed over the labels are the unconditional parameter gradients
    assert _rel(c['gscale'].sum(0), p['gscale']) < tol and _rel(c['goffset'].sum(0), p['goffset']) < tol
    assert _rel(c['cot_scale'].sum(0), p['cot_scale']) < 20 * tol


EQ_CASES = [(s, 'only_0_and_9') for s in SHAPES] + [((7, 128, 8, 8), 'three_labels_n7')]


@pytest.mark.parametrize('relu', [False, True])
@pytest.mark.parametrize('shape,pattern', EQ_CASES)
def test_equal_table_rows_are_the_unconditional_operator(cond_cpu_kernels, shape, pattern, relu):
    _equal_rows('cpu', shape, pattern, relu, 2e-5, bitwise=False)


@pytest.mark.gpu
@pytest.mark.parametrize('relu', [False, True])
@pytest.mark.parametrize('shape,pattern', EQ_CASES)
def test_equal_table_rows_are_the_unconditional_operator_bit_for_bit_on_gpu(shape, pattern, relu):
    import ctgan_amd.kernels as K
    x = _inputs(shape, pattern)[0].cuda()
    if len(shape) == 4:
        x = x.contiguous(memory_format=torch.channels_last)
    # bit equality is the contract of the fused kernels; the composed fallback multiplies by a gathered row in another order
    _equal_rows('cuda', shape, pattern, relu, 3e-5, bitwise=K.layernorm_supported(x))


def _composed_vs_fused(dev, shape, pattern, relu, tol, monkeypatch):
    import ctgan_amd.functional as F
    fused = _run(dev, shape, pattern, relu)
    monkeypatch.setattr(F, 'LN_FUSED', False)                # what CTGAN_LN_FUSED=0 sets at import
    composed = _run(dev, shape, pattern, relu)
    for n, a, b in zip(NAMES, composed, fused):
        if n == 'pen':
            assert abs(a.item() - b.item()) < tol * max(1.0, abs(b.item()))
        else:
            assert _rel(a, b) < (tol if n in ('y', 'gx', 'gscale', 'goffset') else 20 * tol), n


AB_CASES = [((6, 128, 8, 8), 'distinct'), ((3, 8, 48, 48), 'only_0_and_9'), ((5, 256), 'descending'), ((7, 128, 8, 8), 'three_labels_n7')]


@pytest.mark.parametrize('relu', [False, True])
@pytest.mark.parametrize('shape,pattern', AB_CASES)
def test_composed_path_agrees_with_the_fused_kernels(cond_cpu_kernels, monkeypatch, shape, pattern, relu):
    _composed_vs_fused('cpu', shape, pattern, relu, 2e-5, monkeypatch)


@pytest.mark.gpu
@pytest.mark.parametrize('relu', [False, True])
@pytest.mark.parametrize('shape,pattern', AB_CASES)
def test_composed_path_agrees_with_the_fused_kernels_on_gpu(monkeypatch, shape, pattern, relu):
    _composed_vs_fused('cuda', shape, pattern, relu, 3e-5, monkeypatch)


# ------------------------------------------------------------------------------------------------ operator surface (CPU)
def test_layernorm_with_labels_registers_tables(cond_cpu_kernels):
    import ctgan_amd.tflib as lib
    from ctgan_amd.tflib.ops import layernorm as ln
    x = torch.randn(4, 16, 8, 8)
    lab = torch.tensor([1, 9, 0, 1], dtype=torch.int32)
    y = ln.Layernorm('T', [1, 2, 3], x, labels=lab, n_labels=10)
    assert tuple(y.shape) == (4, 16, 8, 8)
    assert tuple(lib._params['T.offset'].shape) == (10, 16) and tuple(lib._params['T.scale'].shape) == (10, 16)
    assert torch.equal(lib._params['T.offset'].detach(), torch.zeros(10, 16)) and torch.equal(lib._params['T.scale'].detach(), torch.ones(10, 16))
    ref = O.layer_norm(x.double(), torch.ones(10, 16).double(), torch.zeros(10, 16).double(), lab)
    assert _rel(y, ref) < 2e-5


def test_layernorm_with_labels_over_other_axes_is_unsupported(cond_cpu_kernels):
    from ctgan_amd.tflib.ops import layernorm as ln
    with pytest.raises(Exception, match='^unsupported$'):
        ln.Layernorm('T', [1], torch.randn(4, 16), labels=torch.zeros(4, dtype=torch.int32), n_labels=10)


def test_layernorm_keyword_relu_call_still_works(cond_cpu_kernels):
    import ctgan_amd.tflib as lib
    from ctgan_amd.tflib.ops import layernorm as ln
    x = torch.randn(4, 16, 8, 8)
    y = ln.Layernorm('T', [1, 2, 3], x, relu=True)
    assert tuple(lib._params['T.scale'].shape) == (16,) and float(y.detach().min()) >= 0.0
    ref = torch.relu(O.layer_norm(x.double(), torch.ones(16).double(), torch.zeros(16).double()))
    assert _rel(y, ref) < 2e-5
