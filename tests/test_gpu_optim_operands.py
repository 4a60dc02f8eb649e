"""The two optional operands of the optimizer's update entries on the MI355X (`-m gpu`): `avg` (the weight average) and `scaler` (the
dynamic loss scale) pick one of four instantiations of each update kernel (csrc/optim_rng.hip launch_update), and `scaler` one of the two
end-of-step kernels.  Every check is bit for bit and pins the choice by what each instantiation is documented to do:
  * with `avg`, theta, the slots, the skip count and the bucket equal the run without it, and avg = a + rate * (theta_new - a) in fp32,
    one rounding per operation (contraction is off in the kernel);
  * with scaler = {S = 2^k, found = 0, ..}, the result equals the run without a scaler given grad_scale / S (exact for a power of two);
  * with found = 1 the update is dropped: theta and the slots stay, the skip count does not move, the average still follows the weights
    and a positive RMSProp clip still clips;
  * each call moves ctgan_debug_optim_launches by exactly one, in the kind of its scaler operand."""
import pytest
import torch

pytestmark = pytest.mark.gpu

RATE, S, GS, CLIP = 0.125, 1024.0, 0.5, 0.01
SIZES = [37, 1, 128, 5]          # packed: odd lengths on the scalar path; the third, sourceless, on the 4-wide one (offset 40)
OFFS = [0, 37, 40, 168]          # (elements 38, 39 belong to no segment: nothing may touch them)
ENTRIES = [('adam', n) for n in (1, 1027)] + [('rmsprop', n) for n in (1, 1027)] + [('adam', None), ('rmsprop', None)]       # None: packed


@pytest.fixture
def K():
    import ctgan_amd.kernels as K
    return K


def counted(kind, call):
    """Run `call`: exactly one optimizer launch, of `kind`."""
    from ctgan_amd._lib import lib
    before = [lib.ctgan_debug_optim_launches(k) for k in range(5)]
    call()
    diff = [lib.ctgan_debug_optim_launches(k) - before[k] for k in range(5)]
    assert diff == [1 if k == kind else 0 for k in range(5)], (kind, diff)


def _start(opt, n):
    """The same start for every run of one entry: weights on both sides of the clip bound, used slots, an average away from the weights,
    a gradient with one inf (n > 1): an applied update skips and counts that element, a dropped one does not."""
    g = torch.Generator().manual_seed(5)
    total = n if n is not None else OFFS[-1] + SIZES[-1]
    theta, a0, grad = torch.randn(total, generator=g) * 0.02, torch.randn(total, generator=g), torch.randn(total, generator=g) * 300.0
    slots = [torch.randn(total, generator=g) * 0.1, torch.rand(total, generator=g) + 0.5][0 if opt == 'adam' else 1:]
    theta[0] = 0.03
    if total > 1:
        grad[5] = float('inf')
    return theta, slots, a0, grad


def _state0(opt):
    return torch.tensor([0.003, 0.5, 0.9, 0.0] if opt == 'adam' else [0.003, 1.0, 1.0, 0.0])


def _run(K, opt, n, averaging, found, grad_scale):
    """One update through the K wrapper -> {theta, slots, state, bucket, avg} on the host.  found None: no scaler."""
    theta0, slots0, a0, grad = _start(opt, n)
    theta, slots, grad = theta0.cuda(), [s.cuda() for s in slots0], grad.cuda()
    state = _state0(opt).cuda()
    avg = a0.cuda() if averaging else None
    scaler = torch.tensor([S, float(found), 7.0, 3.0], device='cuda') if found is not None else None
    kw = dict({'avg': avg, 'avg_rate': RATE} if averaging else {}, **({'scaler': scaler} if scaler is not None else {}))
    hyper = (0.5, 0.9, 1e-8) if opt == 'adam' else (0.9, 1e-10, CLIP)
    if n is not None:
        flat = grad
        fn = K.adam_step if opt == 'adam' else K.rmsprop_step
        call = lambda: fn(theta, flat, *slots, state, *hyper, grad_scale, **kw)                                   # noqa: E731
    else:
        flat = torch.full_like(grad, -7.0)
        srcs = [None if i == 2 else grad[o:o + s].clone() for i, (o, s) in enumerate(zip(OFFS, SIZES))]
        fn = K.adam_step_packed if opt == 'adam' else K.rmsprop_step_packed
        call = lambda: fn(srcs, OFFS, SIZES, flat, theta, *slots, state, *hyper, grad_scale, **kw)                # noqa: E731
    counted(0 if scaler is None else 3, call)
    if scaler is not None:
        assert scaler.tolist() == [S, float(found), 7.0, 3.0]          # an update only reads it
    return {'theta': theta.cpu(), 'slots': [s.cpu() for s in slots], 'state': state.cpu(), 'flat': flat.cpu(),
            'avg': avg.cpu() if averaging else None}


def _same_but_avg(a, b):
    return all(torch.equal(x, y) for x, y in zip([a['theta'], a['state'], a['flat']] + a['slots'], [b['theta'], b['state'], b['flat']] + b['slots']))


def _moved_avg(a0, theta_new, n):
    d = theta_new - a0                                   # three fp32 operations, one rounding each
    p = torch.tensor(RATE, dtype=torch.float32) * d
    out = a0 + p
    if n is None:
        out[38:40] = a0[38:40]
    return out


@pytest.mark.parametrize('opt,n', ENTRIES)
def test_avg_and_scaler_pick_the_instantiation(K, opt, n):
    theta0, slots0, a0, grad = _start(opt, n)
    base = _run(K, opt, n, False, None, GS / S)
    # the base itself: an update happened, the inf was skipped and counted, and the factor matters (so the identity below says something)
    assert not torch.equal(base['theta'], theta0) and base['state'][3].item() == (0.0 if n == 1 else 1.0)
    assert not _same_but_avg(base, _run(K, opt, n, False, None, GS))
    if n is None:
        want = torch.full_like(grad, -7.0)
        for i, (o, s) in enumerate(zip(OFFS, SIZES)):
            want[o:o + s] = 0.0 if i == 2 else grad[o:o + s]
        assert torch.equal(base['flat'].view(torch.int32), want.view(torch.int32))
        assert torch.equal(base['theta'][38:40], theta0[38:40])
    # avg alone
    with_avg = _run(K, opt, n, True, None, GS / S)
    assert _same_but_avg(with_avg, base)
    assert torch.equal(with_avg['avg'], _moved_avg(a0, base['theta'], n)) and not torch.equal(with_avg['avg'], a0)
    # an applied update under the scaler: the static update at grad_scale / S, with and without the average
    for averaging in (False, True):
        got = _run(K, opt, n, averaging, 0, GS)
        assert _same_but_avg(got, base), (opt, n, averaging)
        assert got['avg'] is None if not averaging else torch.equal(got['avg'], with_avg['avg'])
    # a dropped one: nothing but the clip, the bucket and the average
    kept = theta0.clamp(-CLIP, CLIP) if opt == 'rmsprop' else theta0
    if n is None:
        kept[38:40] = theta0[38:40]
    assert opt == 'adam' or not torch.equal(kept, theta0)
    for averaging in (False, True):
        got = _run(K, opt, n, averaging, 1, GS)
        assert torch.equal(got['theta'], kept), (opt, n, averaging)
        assert all(torch.equal(x, y) for x, y in zip(got['slots'], slots0))
        assert torch.equal(got['state'], _state0(opt))          # (state[3]: the inf of a dropped update is not counted)
        assert torch.equal(got['flat'].view(torch.int32), base['flat'].view(torch.int32))
        if averaging:
            assert torch.equal(got['avg'], _moved_avg(a0, kept, n)) and not torch.equal(got['avg'], a0)


def test_step_advance_picks_its_kernel_by_the_scaler(K):
    consts = (2, 1.0, 65536.0)
    state = torch.tensor([0.003, 0.5, 0.25, 4.0], device='cuda')
    ctr = torch.tensor([10], dtype=torch.int64, device='cuda')
    counted(1, lambda: K.step_advance(state, 0.5, 0.5, ctr, 3))
    assert state.tolist()[1:] == [0.25, 0.125, 4.0] and ctr.item() == 13
    for found, scale_after, good_after, skipped_after, powers in ((0, S, 1.0, 3.0, [0.125, 0.0625]), (1, S / 2, 0.0, 4.0, [0.25, 0.125])):
        state = torch.tensor([0.003, 0.25, 0.125, 4.0], device='cuda')
        scaler = torch.tensor([S, float(found), 0.0, 3.0], device='cuda')
        counted(4, lambda: K.step_advance(state, 0.5, 0.5, ctr, 1, scaler=scaler, scaler_consts=consts))
        assert scaler.tolist() == [scale_after, 0.0, good_after, skipped_after], found
        assert state.tolist()[1:] == powers + [4.0], found
    assert ctr.item() == 15
