"""TEST-ONLY torch stand-ins for what ctgan_amd.kernels gained with the dynamic loss scale (csrc/optim_rng.hip: nonfinite_scan_kernel, the
SCALED forms of the four update kernels, step_advance_scaled_kernel).  Layered on the stand-ins that are installed when the fixture
`scale_kernels` below runs (tests/avg_cpu_kernels.py through `avg_kernels`, and what that one is layered on): an update stand-in here
called WITHOUT `scaler=` forwards to the one it replaces with the unchanged arguments; called with it, it either forwards with
grad_scale / S in place of grad_scale - so a good step IS the static step at that factor - or, when the flag is set, does what a dropped
update does: writes the bucket (packed forms), clips (RMSProp), moves the average, and touches nothing else.  Written in torch ops on
whatever device the tensors live on: the GPU tests point `_BASE` at the real static launches and compare the scaled launches with these
bit for bit.  Nothing under ctgan_amd/ imports this file."""
import pytest
import torch

from tests.avg_cpu_kernels import avg_kernels, mode_kernels, move_average        # noqa: F401  (fixtures)

__all__ = ['adam_step', 'adam_step_packed', 'rmsprop_step', 'rmsprop_step_packed', 'step_advance', 'grads_nonfinite']

_BASE = {}          # name -> the callable this file's wrapper forwards to (set by the fixture, or by a GPU test)

# number of positional parameters up to and including grad_scale, the position of theta, of the clip (None: no clip)
_LAYOUT = {'adam_step': (9, 0, None), 'adam_step_packed': (12, 4, None), 'rmsprop_step': (8, 0, 6), 'rmsprop_step_packed': (11, 4, 9)}


def grads_nonfinite(srcs, scaler):
    """scaler[1] = 1 when any element of the sources (a list with None entries, or one tensor) is NaN or +-inf."""
    srcs = [srcs] if torch.is_tensor(srcs) else srcs
    assert scaler.dtype == torch.float32 and scaler.numel() == 4
    if any(s is not None and not bool(torch.isfinite(s).all()) for s in srcs):
        scaler[1] = 1.0


def _scaled(name):
    n_pos, i_theta, i_clip = _LAYOUT[name]

    def step(*args, scaler=None, **kw):
        if scaler is None:
            return _BASE[name](*args, **kw)
        args = list(args)
        if len(args) == n_pos:
            gscale = args.pop()
        else:
            gscale = kw.pop('grad_scale', 1.0)
        if float(scaler[1]) == 0.0:
            return _BASE[name](*args, grad_scale=float(gscale) / float(scaler[0]), **kw)
        theta = args[i_theta]
        if name.endswith('_packed'):
            srcs, offs, counts, flat = args[:4]
            for s, o, c in zip(srcs, offs, counts):
                flat[o:o + c] = 0 if s is None else s.reshape(-1)
        clip = 0.0 if i_clip is None else (args[i_clip] if len(args) > i_clip else kw.get('clip', 0.0))
        if clip > 0:
            theta.clamp_(-clip, clip)
        if kw.get('avg') is not None:
            move_average(kw['avg'], theta, float(kw['avg_rate']))
    step.__name__ = name
    return step


adam_step = _scaled('adam_step')
adam_step_packed = _scaled('adam_step_packed')
rmsprop_step = _scaled('rmsprop_step')
rmsprop_step_packed = _scaled('rmsprop_step_packed')


def advance_scaler(scaler, growth_interval, min_scale, max_scale):
    """The scaler's part of the end of a step, in place -> True when the update was applied (the beta powers then advance)."""
    found = float(scaler[1]) != 0.0
    if found:
        scaler[0] = max(float(scaler[0]) * 0.5, min_scale)
        scaler[2] = 0.0
        scaler[3] += 1.0
    else:
        good = float(scaler[2]) + 1.0
        if good >= growth_interval:
            scaler[0] = min(float(scaler[0]) * 2.0, max_scale)
            good = 0.0
        scaler[2] = good
    scaler[1] = 0.0
    return not found


def step_advance(state, beta1, beta2, rng_ctr=None, rng_by=1, scaler=None, scaler_consts=None):
    if scaler is None:
        return _BASE['step_advance'](state, beta1, beta2, rng_ctr, rng_by)
    if advance_scaler(scaler, *scaler_consts):
        state[1:3].mul_(torch.tensor([beta1, beta2], dtype=torch.float32, device=state.device))
    if rng_ctr is not None:
        rng_ctr += rng_by


def install(K, setitem=None, setattr_=None):
    """Put the stand-ins of this file over whatever `K` (ctgan_amd.kernels) holds now; through monkeypatch's setters when given."""
    import sys
    mod = sys.modules[__name__]
    for name in __all__:
        base = getattr(K, name, None)
        if setitem is not None:
            setitem(_BASE, name, base)
        else:
            _BASE[name] = base
        (setattr_ or setattr)(K, name, getattr(mod, name))


@pytest.fixture
def scale_kernels(avg_kernels, monkeypatch):        # noqa: F811
    """avg_kernels (cpu_kernels + the RMSProp / GAN-loss + weight-average stand-ins) plus the stand-ins of this file."""
    import ctgan_amd.kernels as K
    install(K, monkeypatch.setitem, monkeypatch.setattr)
    yield avg_kernels
