"""TF-form Adam and RMSProp over one flat fp32 buffer per network (csrc/optim_rng.hip: adam_kernel, rmsprop_kernel).

FlatAdam mirrors `tf.train.AdamOptimizer(learning_rate=LR*decay, beta1, beta2)` + compute_gradients /
apply_gradients (TF/CT_gan_cifar_resnet.py:333-338; TF/CT_gan_cifar.py:153-154); FlatRMSProp
`tf.train.RMSPropOptimizer(learning_rate)` of the 'wgan' / 'lsgan' objectives (TF/CT_gan_mnist.py:125-131,
TF/CT_gan_64x64.py:548-576), with the 'wgan' weight clip fused into its update.  The flat parameter /
gradient buffers double as the all-reduce buckets of the batch-sharded step (ddp.py).
"""
import contextlib
import math

import torch

from . import kernels as K
from . import tflib as lib


def _power_of_two(name, x):
    x = float(x)
    if not (x > 0 and math.isfinite(x) and math.frexp(x)[0] == 0.5 and 2.0 ** -126 <= x <= 2.0 ** 127):
        raise ValueError('%s must be a power of two (an fp32 one: dividing by it must stay exact): %r' % (name, x))
    return x


class LossScaler:
    """Dynamic loss scale of the fp16 matrix-core mode, kept on the device (NOT in the reference).  `state` = device float[4]
    {S, found, good, skipped}: S the power-of-two scale, found the flag the gradient scan of a step sets on a NaN / inf, good the updates
    applied in a row since S last changed, skipped the updates dropped so far.  The backward of a step is seeded with S read FROM THE
    DEVICE (`seed()`), the update kernels divide it out again and drop the whole update when `found` is set, the end-of-step launch
    halves S after a dropped update (down to min_scale) and doubles it after growth_interval applied ones in a row (up to max_scale):
    no host code between a step's backward and its update, so a captured graph carries the scheme.  One scaler serves both optimizers of
    a trainer: growth_interval counts updates of either network.  The counts are floats, exact to 2^24: a growth_interval beyond that is
    never reached (a way to hold the scale)."""

    def __init__(self, init_scale=2.0 ** 16, growth_interval=2000, min_scale=1.0, max_scale=2.0 ** 24, device=None):
        self.init_scale = _power_of_two('init_scale', init_scale)
        self.min_scale = _power_of_two('min_scale', min_scale)
        self.max_scale = _power_of_two('max_scale', max_scale)
        if not self.min_scale <= self.init_scale <= self.max_scale:
            raise ValueError('min_scale <= init_scale <= max_scale does not hold: %r, %r, %r' % (min_scale, init_scale, max_scale))
        if int(growth_interval) != growth_interval or growth_interval < 1:
            raise ValueError('growth_interval must be a positive integer: %r' % (growth_interval,))
        self.growth_interval = int(growth_interval)
        self.state = torch.tensor([self.init_scale, 0.0, 0.0, 0.0], dtype=torch.float32, device=device if device is not None else lib._dev())

    @property
    def consts(self):
        """(growth_interval, min_scale, max_scale): they ride in the end-of-step launch's arguments."""
        return (self.growth_interval, self.min_scale, self.max_scale)

    def seed(self):
        """The 0-dim device VIEW of the scale: the backward's seed.  A view, so a captured graph reads the value current at each replay."""
        return self.state[0]

    def scale(self):
        """The current scale as a float.  Reads device memory: outside captured regions, at logging cadence."""
        return float(self.state[0].item())

    def skipped_steps(self):
        """Updates (of either network) dropped so far because their gradients held a NaN / inf.  Reads device memory, as scale()."""
        return int(self.state[3].item())

    def good_steps(self):
        """Updates applied in a row since the scale last changed.  Reads device memory, as scale()."""
        return int(self.state[2].item())

    def state_dict(self):
        return {'state': self.state.cpu().clone()}

    def load_state_dict(self, sd):
        """sd None (a checkpoint of a run without a dynamic scale): start over at init_scale."""
        if sd is None:
            self.state.copy_(torch.tensor([self.init_scale, 0.0, 0.0, 0.0]))
            return
        st = sd['state'].to(torch.float32)
        _power_of_two('the saved scale', st[0].item())
        self.state.copy_(st)
        self.state[1:2].zero_()           # (the flag lives within one step)


class FlatAdam:
    kind = 'adam'

    def __init__(self, named_params, beta1, beta2, eps=1e-8, state=None, avg_rate=0.0, scaler=None):
        """named_params: [(name, Parameter)] - the trainable variable list, in registry order.  state: optional float[4] device
        slice to keep {lr, beta1^t, beta2^t, -} in (two optimizers sharing one allocation take a common learning rate in one fill).
        avg_rate > 0 (NOT in the reference; the GAN trainers' `g_average`): keep `avg`, an exponential moving average of the weights laid
        out like `theta` - avg <- avg + avg_rate (theta - avg), moved by the update's own launch (csrc/optim_rng.hip avg_elem), so a rate
        of 1e-4 is a decay of 0.9999 - starting at a COPY of the weights (FlatAdamTheano's starts at zeros, as its script's does).  0: no
        average, and nothing differs from an optimizer built without the argument (launches, slots(), state_dict()).
        scaler (NOT in the reference): a LossScaler, shared with the trainer's other optimizer - update() and step() then run scan ->
        update -> end of step (kernels.grads_nonfinite, then the `scaler=` operand of the other two), one launch more than without; the
        grad_scale they are given is the host's factor only (1 / world), the division by the scale happens on the device.  None: nothing
        differs.  `t` counts ATTEMPTED updates on the host, dropped ones included: with a scaler the beta powers on the device (state[1],
        state[2]) are what knows how many were applied.
        `spectral` (NOT in the reference) is no argument: a SpectralNorm is built FROM the finished optimizer - SpectralNorm(named_params,
        opt) - and attaches itself (attach_spectral); step() then runs [scan] -> spectral.grad_(grad) -> update -> end of step ->
        spectral.normalise(), and update() goes through gather_grads + step (the packed update has no bucket to transform).  Without one
        nothing differs."""
        self.scaler = scaler
        self.spectral = None
        self.avg_rate = float(avg_rate)
        if not 0.0 <= self.avg_rate <= 1.0:
            raise ValueError('avg_rate must be in [0, 1] (it is the rate 1 - decay, e.g. 1e-4 for a decay of 0.9999): %r' % (avg_rate,))
        self.names = [n for n, _ in named_params]
        self.params = [p for _, p in named_params]
        if not self.params:
            raise ValueError('empty parameter list')
        heads = {n.split('.')[0] for n in self.names}
        self.group = heads.pop() if len(heads) == 1 else None     # one network per optimizer: only its caches go stale on step()
        dev = self.params[0].device
        self.beta1, self.beta2, self.eps = float(beta1), float(beta2), float(eps)
        self.sizes = [p.numel() for p in self.params]
        total = sum(self.sizes)
        self.theta = torch.empty(total, dtype=torch.float32, device=dev)
        self.grad = torch.zeros(total, dtype=torch.float32, device=dev)
        self._alloc_slots(total, dev)
        # re-home every parameter inside the flat buffer (same values, same shapes)
        off = 0
        with torch.no_grad():
            for p, n in zip(self.params, self.sizes):
                self.theta[off:off + n].copy_(p.reshape(-1))
                p.data = self.theta[off:off + n].view(p.shape)
                off += n
        # (the subclass FlatAdamTheano keeps an average of its own, from zeros: this one is only allocated when the rate came in HERE)
        self._avg_own = self.avg_rate > 0
        self.avg = self.theta.clone() if self._avg_own else None
        # {lr, beta1^t, beta2^t, skipped}; TF initialises the power accumulators to beta (t = 1).  skipped: elements the update
        # kernels left untouched because their gradient was not finite, accumulated over the run (skipped())
        init = torch.tensor([0.0, self.beta1, self.beta2, 0.0], dtype=torch.float32, device=dev)
        if state is None:
            self.state = init
        else:
            assert state.shape == (4,) and state.dtype == torch.float32 and state.device.type == dev.type and state.is_contiguous()
            self.state = state
            self.state.copy_(init)
        self._lr_last = None      # value currently in state[0] if written by set_lr (None = unknown)
        self.t = 0
        self._keepalive = []
        self.offsets = [sum(self.sizes[:i]) for i in range(len(self.sizes))]

    def attach_spectral(self, spectral):
        """Make `spectral` (a SpectralNorm built over this optimizer; its constructor calls this) part of every step from here on."""
        if spectral.opt is not self:
            raise ValueError('attach_spectral: the SpectralNorm was built over another optimizer')
        if getattr(self, 'clip', 0.0) > 0:
            raise ValueError('spectral normalisation and weight clipping (clip=%r) are two answers to one question: use one' % self.clip)
        self.spectral = spectral

    def _alloc_slots(self, total, dev):
        self.m = torch.zeros(total, dtype=torch.float32, device=dev)
        self.v = torch.zeros(total, dtype=torch.float32, device=dev)

    def set_lr(self, lr):
        """Write the scalar learning rate into the device-resident state (outside any captured graph).  The value rides in
        the fill kernel's ARGUMENTS - no host staging buffer a later call could overwrite before an asynchronous copy of it
        has run - and the launch is skipped while the rate does not change (the N_CRITIC critic steps of an iteration)."""
        lr = float(lr)
        if self._lr_last == lr:
            return
        self.state[0:1].fill_(lr)
        self._lr_last = lr

    def skipped(self):
        """Number of parameter elements the update kernels have left untouched so far because their (scaled) gradient was NaN / inf
        (csrc/optim_rng.hip adam_elem; the reference's tf.train.AdamOptimizer would propagate the NaN instead).  Non-zero means the
        run overflowed (fp16 mode under its fixed loss scale) or diverged: the trainers log it, bench.py fails its loss guard on it.
        Reads device memory: call it outside captured regions, at logging cadence."""
        return int(self.state[3].item())

    def gather_grads(self, grads, lo=0, hi=None):
        """Pack per-parameter gradients (None = zero) into the flat bucket with ONE kernel (the pointer table rides
        in the kernel arguments: no per-variable copy, hipGraph-capture safe).  lo / hi: only parameters [lo, hi) - `grads` still
        lists all of them - for a step that hands its bucket to the all-reduce in two parts; returns that part of the bucket."""
        hi = len(self.sizes) if hi is None else hi
        end = self.offsets[hi] if hi < len(self.sizes) else self.grad.numel()
        part = self.grad[self.offsets[lo]:end] if lo < hi else self.grad[0:0]
        if lo >= hi:
            return part
        if self.grad.device.type != 'cuda':
            for i in range(lo, hi):
                g, off, n = grads[i], self.offsets[i], self.sizes[i]
                if g is None:
                    self.grad[off:off + n].zero_()
                else:
                    self.grad[off:off + n].copy_(g.reshape(-1))
            return part
        srcs = [g.contiguous() if g is not None else None for g in grads[lo:hi]]
        K.pack(srcs, self.offsets[lo:hi], self.sizes[lo:hi], self.grad)
        self._keepalive = (self._keepalive if lo else []) + srcs          # sources stay allocated until the next step's first gather
        return part

    def step(self, grad_scale=1.0, rng=None):
        """theta <- Adam(theta, grad); then ONE launch advances the beta-power accumulators and, with `rng`, that stream's step
        counter (DeviceRNG.end_step)."""
        if self.scaler is not None:
            K.grads_nonfinite(self.grad, self.scaler.state)         # (the bucket after the all-reduce: every rank sees the same bits)
        if self.spectral is not None:
            self.spectral.grad_(self.grad, self.scaler)             # gradients w.r.t. the normalised weights -> w.r.t. the raw ones
        self._launch(grad_scale)
        self._end(rng)
        if self.spectral is not None:
            # one power iteration per weight version, the last launches of a step; none after an update the loss scaler dropped
            self.spectral.normalise(held=self.scaler is not None)

    def _launch(self, grad_scale, srcs=None):
        """The update launch of a step, the one thing an optimizer on these buffers has of its own: over the bucket, or (srcs) gathering
        the bucket in the same launch."""
        if srcs is None:
            K.adam_step(self.theta, self.grad, self.m, self.v, self.state, self.beta1, self.beta2, self.eps, grad_scale, **self._extras())
        else:
            K.adam_step_packed(srcs, self.offsets, self.sizes, self.grad, self.theta, self.m, self.v, self.state, self.beta1, self.beta2,
                               self.eps, grad_scale, **self._extras())

    def _extras(self):
        """The keywords of an update launch beyond the static one's: each is OMITTED when its feature is off."""
        kw = {'avg': self.avg, 'avg_rate': self.avg_rate} if self._avg_own else {}
        if self.scaler is not None:
            kw['scaler'] = self.scaler.state
        return kw

    def avg_views(self):
        """[(name, view of the average shaped like the parameter)]"""
        return [(n, self.avg[o:o + s].view(p.shape)) for n, p, o, s in zip(self.names, self.params, self.offsets, self.sizes)]

    def _end(self, rng):
        kw = {'scaler': self.scaler.state, 'scaler_consts': self.scaler.consts} if self.scaler is not None else {}
        K.step_advance(self.state, self.beta1, self.beta2, rng.ctr if rng is not None else None, 1, **kw)
        self.t += 1
        lib.bump_epoch(self.group)    # this network's weights changed: its derived-filter caches are stale

    def update(self, grads, grad_scale=1.0, rng=None):
        """gather_grads + step with the bucket and the update in ONE launch: the single-rank form of a step (no collective between
        gather and update)."""
        if self.grad.device.type != 'cuda' or len(grads) > K.ADAM_PACKED_MAX or self.spectral is not None:
            self.gather_grads(grads)
            return self.step(grad_scale, rng)
        srcs = [g.contiguous() if g is not None else None for g in grads]
        if self.scaler is not None:
            K.grads_nonfinite(srcs, self.scaler.state)
        self._launch(grad_scale, srcs)
        self._keepalive = srcs
        self._end(rng)

    def update_clipped(self, grads, clip_norm, rng=None):
        """gather_grads, tf.clip_by_global_norm over the whole bucket (LS/tflib/train_loop_2.py:76-79), step.  Returns the norm BEFORE
        the clip as a float32 device scalar [1]; nothing crosses to the host (kernels.global_norm / clip_by_norm_)."""
        if self.scaler is not None:
            raise NotImplementedError('update_clipped: not under a dynamic loss scale (the norm would be the scaled gradient\'s)')
        if self.spectral is not None:
            raise NotImplementedError('update_clipped: not with spectral normalisation (which gradient the norm is of is undecided)')
        self.gather_grads(grads)
        norm = K.global_norm(self.grad)
        K.clip_by_norm_(self.grad, norm, clip_norm)
        self.step(1.0, rng)
        return norm

    def slots(self):
        """The device tensors a step writes besides the weights: what a graph capture's warm-up steps must leave as they found them (the
        average too: on a resumed run avg != theta, and a step at learning rate 0 still moves it; the state of the loss scaler too: a
        warm-up step that overflows must not halve the scale of the real run)."""
        return [self.m, self.v, self.state] + self._avg_slot()

    def _avg_slot(self):
        """(and the scaler's state: the tail of every slots() list)"""
        return (([self.avg] if self._avg_own else []) + (self.spectral.slots() if self.spectral is not None else [])
                + ([self.scaler.state] if self.scaler is not None else []))

    def _avg_state(self, sd):
        if self._avg_own:
            sd['avg'] = self.avg.cpu().clone()
        if self.spectral is not None:
            sd['spectral'] = self.spectral.state_dict()
        return sd

    def _load_avg(self, sd):
        """checkpoint.load restores the parameters BEFORE the optimizers, so `theta` already holds the loaded weights here: a state
        without 'avg' (a checkpoint of a run that kept none) starts the average at them - averaging can be switched on at a resume.
        A state with 'avg' loaded into an optimizer that keeps none ignores it."""
        if self._avg_own:
            self.avg.copy_(sd['avg'] if sd.get('avg') is not None else self.theta)
        if self.spectral is not None:
            self.spectral.load_state_dict(sd.get('spectral'))

    def load_named_slots(self, m_by_name, v_by_name, t):
        """Overwrite the Adam slots from per-parameter tensors (teacher-forced parity tests, resume)."""
        off = 0
        for name, n in zip(self.names, self.sizes):
            self.m[off:off + n].copy_(m_by_name[name].reshape(-1).to(self.m.device, torch.float32))
            self.v[off:off + n].copy_(v_by_name[name].reshape(-1).to(self.v.device, torch.float32))
            off += n
        self.t = int(t)
        self.state[1] = self.beta1 ** (self.t + 1)
        self.state[2] = self.beta2 ** (self.t + 1)

    def state_dict(self):
        return self._avg_state({'kind': self.kind, 'm': self.m.cpu().clone(), 'v': self.v.cpu().clone(), 'state': self.state.cpu().clone(),
                                't': self.t})

    def _check_kind(self, sd):
        kind = sd.get('kind', 'adam')          # (checkpoints written before the tag are Adam's)
        if kind != self.kind:
            raise ValueError('optimizer state of a %s optimizer cannot be loaded into a %s optimizer (another MODE?)' % (kind, self.kind))

    def load_state_dict(self, sd):
        """(Parameters first, then this: see _load_avg.)"""
        self._check_kind(sd)
        self.m.copy_(sd['m']); self.v.copy_(sd['v']); self.state.copy_(sd['state']); self.t = int(sd['t'])
        self._load_avg(sd)
        self.state[3:4].zero_()            # skipped() counts THIS session's skips: a resumed run does not inherit the saved run's
        self._lr_last = None


@contextlib.contextmanager
def averaged(opt):
    """`with averaged(trainer.g_opt):` - inside, the network's parameters hold the weight average (`opt.avg`) instead of the live weights:
    sample and score from it.  Entry and exit are ONE launch each (kernels.exchange_) that swaps the CONTENTS of `theta` and `avg`, so
    every address a captured graph or a pointer-keyed derived-filter cache has seen stays valid and no third buffer is needed, and each
    bumps the network's registry epoch, so no derived / packed filter image built from the other set of weights is served.  A pure
    exchange: after the exit - also when the body raised - both buffers hold the bits they held before, and graph replay goes on as if
    the context had never been entered.  Do not step the optimizer inside.  ValueError when the optimizer keeps no average; not inside a
    stream capture (the swap must happen once, now, and not at every replay)."""
    if not getattr(opt, '_avg_own', False):
        raise ValueError('averaged(): this optimizer keeps no weight average (g_average = 0)')
    if opt.theta.is_cuda and torch.cuda.is_current_stream_capturing():
        raise RuntimeError('averaged(): not inside a stream capture')
    K.exchange_(opt.theta, opt.avg)
    lib.bump_epoch(opt.group)
    try:
        yield opt
    finally:
        K.exchange_(opt.theta, opt.avg)
        lib.bump_epoch(opt.group)


def spectral_normalised(name):
    """The name rule of spectral normalisation: conv filters and Linear weights (the projection table `Discriminator.Projection.W`
    too); not biases, not the scales / offsets / tables of Layernorm and BatchNorm, not moving statistics."""
    return name.endswith(('.Filters', '.W'))


class SpectralNorm:
    """Spectral normalisation of an optimizer's weight matrices (Miyato et al., ICLR 2018; NOT in the reference).  Every
    parameter of `opt` whose name ends in `.Filters` or `.W` is read, in its stored layout, as M[K, N] with N the last axis, and keeps
    u[N], v[K], sigma.  `theta_bar` is laid out like `opt.theta` and holds M / max(sigma, 1e-12) for those and a copy for the rest: it
    is what the network reads (`views()`, installed with lib.alias_params by the trainer), while the optimizer, the registry and the
    checkpoints keep the raw weights.  normalise() runs one power iteration (kernels.spectral_normalize) - once here, then as the last
    launches of every opt.step() - so everything between two updates sees one theta_bar; grad_() turns the gradient with respect to
    theta_bar into the one with respect to theta, u and v held constant, in place in the flat bucket (kernels.spectral_grad).  u starts
    from lib.rng_for(name + '.u'): every rank starts, and stays, identical, nothing is communicated."""

    def __init__(self, named_params, opt):
        if [n for n, _ in named_params] != opt.names:
            raise ValueError('SpectralNorm: named_params is not the list the optimizer was built from')
        self.opt = opt
        self.names = [n for n in opt.names if spectral_normalised(n)]
        if not self.names:
            raise ValueError('SpectralNorm: no parameter name ends in .Filters or .W')
        jobs, u0 = [], []
        for n, p, o in zip(opt.names, opt.params, opt.offsets):
            if not spectral_normalised(n):
                continue
            N = p.shape[-1] if p.dim() else 1
            jobs.append((o, p.numel() // N, N))
            x = lib.rng_for(n + '.u').standard_normal(N)
            u0.append(torch.from_numpy(x / max(float((x * x).sum()) ** 0.5, 1e-12)).to(torch.float32))
        dev = opt.theta.device
        self.table = K.SpectralTable(jobs, opt.theta.numel(), dev)
        self.theta_bar = torch.empty_like(opt.theta)
        self.u = torch.cat(u0).to(dev)
        self._u0 = self.u.clone()
        self.v = torch.zeros(self.table.v_size, dtype=torch.float32, device=dev)
        self.sigma = torch.zeros(self.table.njobs, dtype=torch.float32, device=dev)
        self.scratch = torch.empty(max(self.table.scratch_floats, 1), dtype=torch.float32, device=dev)
        # under a dynamic loss scale: the flag of the step's gradient scan, kept past the end-of-step launch that clears it (grad_ writes
        # it, the normalise of the same step reads it; nothing else does, so it is no slot)
        self.hold = torch.zeros(1, dtype=torch.float32, device=dev) if opt.scaler is not None else None
        self._views = [(n, torch.nn.Parameter(self.theta_bar[o:o + s].view(p.shape)))
                       for n, p, o, s in zip(opt.names, opt.params, opt.offsets, opt.sizes)]
        opt.attach_spectral(self)
        self.normalise()

    def normalise(self, iterate=True, held=False):
        """One power iteration and theta_bar (three launches); iterate=False: theta_bar from the sigma held (one launch; after a load).
        held (opt.step() under a dynamic loss scale): the iteration is skipped ON THE DEVICE when the update since the last grad_(bucket,
        scaler) was dropped - no new weight version, so u, v, sigma and theta_bar keep their bits."""
        kw = {'hold': self.hold} if held and self.hold is not None else {}
        K.spectral_normalize(self.opt.theta, self.theta_bar, self.table, self.u, self.v, self.sigma, self.scratch, iterate=iterate, **kw)

    def grad_(self, bucket, scaler=None):
        """bucket (laid out like opt.grad) holds dL/d theta_bar; afterwards dL/d theta (two launches).  scaler (a LossScaler, after its
        scan of the bucket): its flag is also kept for the normalise(held=True) that follows the update."""
        kw = {'scaler': scaler.state, 'hold': self.hold} if scaler is not None and self.hold is not None else {}
        K.spectral_grad(bucket, self.theta_bar, self.table, self.u, self.v, self.sigma, self.scratch, **kw)

    def sigmas(self):
        """name -> sigma as floats.  Reads device memory: outside captured regions, at logging cadence."""
        return dict(zip(self.names, self.sigma.cpu().tolist()))

    def views(self):
        """[(name, the parameter's part of theta_bar, shaped like it)] for EVERY parameter of the optimizer, normalised or copied: leaf
        Parameters that require a gradient, the same objects at every call."""
        return list(self._views)

    def aliases(self):
        """{raw parameter: its view of theta_bar}: the argument of lib.alias_params."""
        return {p: v for p, (_, v) in zip(self.opt.params, self._views)}

    def install(self):
        """Make the network read theta_bar: the aliases into the registry's table, the network's derived-filter caches stale.  They stay
        until remove() or lib.delete_all_params(): a trainer built later on the same registry reads theta_bar too until then."""
        lib.alias_params(self.aliases())
        lib.bump_epoch(self.opt.group)

    def remove(self):
        """Undo install() - only this object's aliases - and leave the optimizer: the network reads the raw weights again and the
        optimizer steps as one built without spectral normalisation."""
        lib.delete_param_aliases(self.aliases())
        lib.bump_epoch(self.opt.group)
        if self.opt.spectral is self:
            self.opt.spectral = None

    def slots(self):
        """What a step writes here (a graph capture's warm-up at learning rate 0 still iterates)."""
        return [self.theta_bar, self.u, self.v, self.sigma]

    def state_dict(self):
        return {'u': self.u.cpu().clone(), 'v': self.v.cpu().clone(), 'sigma': self.sigma.cpu().clone()}

    def load_state_dict(self, sd):
        """After the parameters are restored (checkpoint.load: parameters first).  With the saved state theta_bar is recomputed from the
        saved sigma and nothing iterates - a resumed run has the bits of the uninterrupted one; sd None (a checkpoint of a run without
        spectral normalisation): one iteration from the constructor's u."""
        if sd is None:
            self.u.copy_(self._u0)
            self.normalise()
            return
        self.u.copy_(sd['u']); self.v.copy_(sd['v']); self.sigma.copy_(sd['sigma'])
        self.normalise(iterate=False)


class FlatRMSProp(FlatAdam):
    """tf.train.RMSPropOptimizer(learning_rate) with TF 1.x's defaults - decay rho = 0.9, momentum 0, epsilon 1e-10, not centered - over
    the flat buffer (kernels.rmsprop_step):  ms <- ms + (g^2 - ms)(1 - rho);  theta <- theta - lr g / sqrt(ms + eps).  With momentum 0
    TF's `mom` slot only ever holds the step just applied, so it is not kept.  TF creates the `rms` slot at ONES, not zeros (its
    slot initialiser; not visible in the reference tree): the first step is ~ lr g, not lr sign(g) sqrt(10).

    `clip` > 0: theta <- clip_by_value(theta, -clip, clip) fused into every update - the 'wgan' objective's clip op run after every critic
    update (TF/CT_gan_mnist.py:134-143, :248-249).  The same interface as FlatAdam; state = device float[4] {lr, 1, 1, skipped}."""

    kind = 'rmsprop'

    def __init__(self, named_params, rho=0.9, eps=1e-10, clip=None, state=None, avg_rate=0.0, scaler=None):
        # (FlatAdam's flat buffers, gather and end-of-step launch; its beta powers stay 1, so step_advance only moves the Philox counter)
        super().__init__(named_params, 1.0, 1.0, eps, state, avg_rate, scaler)
        self.rho, self.clip = float(rho), float(clip or 0.0)

    def _alloc_slots(self, total, dev):
        self.ms = torch.ones(total, dtype=torch.float32, device=dev)

    def slots(self):
        """The device tensors a step writes besides the weights - and the weights too when the update clips them (a step at learning
        rate 0, as in a graph capture's warm-up, still clips)."""
        return [self.ms, self.state] + ([self.theta] if self.clip > 0 else []) + self._avg_slot()

    def _launch(self, grad_scale, srcs=None):
        if srcs is None:
            K.rmsprop_step(self.theta, self.grad, self.ms, self.state, self.rho, self.eps, self.clip, grad_scale, **self._extras())
        else:
            K.rmsprop_step_packed(srcs, self.offsets, self.sizes, self.grad, self.theta, self.ms, self.state, self.rho, self.eps, self.clip,
                                  grad_scale, **self._extras())

    def load_named_slots(self, ms_by_name, t):
        off = 0
        for name, n in zip(self.names, self.sizes):
            self.ms[off:off + n].copy_(ms_by_name[name].reshape(-1).to(self.ms.device, torch.float32))
            off += n
        self.t = int(t)

    def state_dict(self):
        return self._avg_state({'kind': self.kind, 'ms': self.ms.cpu().clone(), 'state': self.state.cpu().clone(), 't': self.t})

    def load_state_dict(self, sd):
        self._check_kind(sd)
        self.ms.copy_(sd['ms']); self.state.copy_(sd['state']); self.t = int(sd['t'])
        self._load_avg(sd)
        self.state[3:4].zero_()
        self._lr_last = None


class FlatAdamTheano(FlatAdam):
    """The Adam of the reference's Theano classifier (TH/nn.py:30-47 `adam_updates`; TH/ = CT-GANs/Theano_classifier) over the flat
    buffer (kernels.adam_theano_step):  m <- b1 m + (1-b1) g;  v <- b2 v + (1-b2) g^2;
    theta <- theta - lr (m / (1-b1^t)) / sqrt(v / (1-b2^t) + 1e-8)  - the epsilon INSIDE the root, t from 1, one counter per optimizer.
    `avg_rate` > 0 keeps the parameter average of TH/CT_MNIST.py:104-105, avg <- avg + avg_rate (theta - avg) from zeros, moved in the
    update's own launch (`avg`, laid out like the flat parameter buffer; `avg_views()` gives it per parameter).  The same interface
    and device state {lr, b1^t, b2^t, skipped} as FlatAdam."""

    kind = 'adam_theano'

    def __init__(self, named_params, beta1, beta2, eps=1e-8, avg_rate=0.0, state=None, scaler=None):
        if scaler is not None:
            raise ValueError('FlatAdamTheano takes no loss scaler: the classifiers it trains have no 16-bit mode with a loss scale')
        super().__init__(named_params, beta1, beta2, eps, state)
        self.avg_rate = float(avg_rate)
        self.avg = torch.zeros_like(self.theta) if self.avg_rate > 0 else None          # (its own: the base class was given no rate)

    def attach_spectral(self, spectral):
        raise NotImplementedError('FlatAdamTheano: no spectral normalisation (the classifiers it trains are weight-normalised)')

    def step(self, grad_scale=1.0, rng=None):
        assert grad_scale == 1.0
        K.adam_theano_step(self.theta, self.grad, self.m, self.v, self.avg, self.state, self.beta1, self.beta2, self.eps, self.avg_rate)
        self._end(rng)

    def update(self, grads, grad_scale=1.0, rng=None):
        self.gather_grads(grads)
        self.step(grad_scale, rng)

    def slots(self):
        return [self.m, self.v, self.state] + ([self.avg] if self.avg is not None else [])

    def state_dict(self):
        sd = super().state_dict()
        if self.avg is not None:
            sd['avg'] = self.avg.cpu().clone()
        return sd

    def load_state_dict(self, sd):
        super().load_state_dict(sd)
        if self.avg is not None:
            self.avg.copy_(sd['avg'])
