"""hipGraph-captured D/G steps.

A critic step is ~700 kernel launches issued from Python autograd; at MI355X speeds the host cannot
keep up (launch-bound), so the whole (loss graph + backward + gradient packing [+ Adam]) of each step
is captured once into a hipGraph and replayed.  Replay-safety: every random draw reads its Philox
step counter from device memory, Adam reads lr / beta powers from device memory, inputs live in
static buffers.  With world_size > 1 the all-reduce and the Adam kernels stay outside the graph.
"""
import os as _os
import time

import torch

from . import functional as F
from . import kernels as K
from . import gan_cifar_resnet as R
from . import tflib as lib

# A/B switch: the whole iteration (G step + fake batches + N_CRITIC critic steps) as ONE hipGraph when world == 1
ITERATION_GRAPH = _os.environ.get('CTGAN_ITERATION_GRAPH', '1') != '0'
# world > 1: capture the gradient all-reduce (RCCL supports stream capture) and the Adam step INSIDE the step graphs, so that the
# multi-GPU loop is the same one-graph-per-iteration replay as the single-GPU loop (no graph boundaries, no eager launches between
# the steps).  Default (round 4) when the process group's backend is RCCL ('nccl'); the eager side-stream all-reduce
# (ddp.FlatAllReduce) stays the path for gloo (its CUDA collectives stage through the host: not capturable) and is what the CPU tests
# cover.  CTGAN_AR_IN_GRAPH=0 / 1 forces either.  Covered on one GPU by a 1-rank RCCL group incl. grad_scale = 1 / world != 1
# (tests/test_gpu_graph_loop.py); bench.py falls back to the side-stream path on every rank if any rank's capture fails.
_AR_ENV = _os.environ.get('CTGAN_AR_IN_GRAPH')
AR_IN_GRAPH = None if _AR_ENV is None else (_AR_ENV != '0')


def ar_in_graph_default():
    """In-graph collectives by default exactly when they are RCCL collectives."""
    if AR_IN_GRAPH is not None:
        return AR_IN_GRAPH
    import torch.distributed as dist
    return bool(dist.is_available() and dist.is_initialized() and dist.get_backend() == 'nccl')


def _capture_kw():
    """Keyword arguments of torch.cuda.graph for this process.  With a process group alive, the c10d RCCL watchdog thread polls its work
    events (hipEventQuery) at any time - under the default GLOBAL capture error mode a poll that lands inside a capture aborts the
    process ("operation not permitted when stream is capturing": seen once in four runs of the 1-rank test).  THREAD_LOCAL mode restricts
    the capture's legality checks to the capturing thread, which is what the PyTorch notes prescribe for graphs next to NCCL."""
    import torch.distributed as dist
    return {'capture_error_mode': 'thread_local'} if (dist.is_available() and dist.is_initialized()) else {}


def quiesce_collectives():
    """Call before a capture when a process group is alive.  Collectives enqueued eagerly (warm-up passes, communicator start-up) leave
    work items on the c10d watchdog's list; it retires them by polling their events every ~100 ms, and a poll that lands inside a
    capture raised a HIP error in the watchdog thread on this stack even under THREAD_LOCAL mode (2 of 3 runs once the warm-up got
    shorter).  After a device synchronize every item is complete: one poll period later the list is empty and nothing is polled
    while capturing (collectives enqueued under capture are never put on that list)."""
    import torch.distributed as dist
    if dist.is_available() and dist.is_initialized() and torch.cuda.is_available():
        torch.cuda.synchronize()
        time.sleep(0.35)


def _capture_graphs(eng, warmup, opts, extra_bufs, bodies, warm=None, it_body=None):
    """THE capture protocol of every Graphed* wrapper: `warmup` passes over the callables of `warm` (default: the bodies, in order) on one
    side stream, then each (graph attribute, result attribute or None, body) of `bodies` captured in order and stored on `eng`, then
    the optional whole-iteration graph `it_body` (-> eng.it_graph / it_out, or eng.it_graph_error).

    Everything a body changes besides its outputs is restored afterwards (also when capture fails): the optimizers' slots and host step
    counts, and `extra_bufs` - the Philox step counter, prediction tables, moving statistics - so a captured trainer continues exactly
    where the eager one would (checkpoint resume, graph-vs-eager parity tests).

    Each graph owns a PRIVATE memory pool.  The graphs are replayed in an order other than the capture order (g, f, then d x N_CRITIC)
    and their outputs outlive other graphs' replays - `fake_all` is read by all N_CRITIC critic replays.  With one shared pool a block
    freed while capturing graph A is handed to graph B as storage of a live OUTPUT, and A's next replay scribbles over it (round 1: the
    fake batches of critic steps 2..5 were whatever the first critic replay left in that memory, hence a critic cost of -6e18).  A
    private pool costs ~3 GB per graph of the 288 GB and makes an output valid until its own graph is replayed again."""
    def capture(body):
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, **_capture_kw()):
            return g, body()
    K.reset_capture_workspaces()
    bufs = [b for o in opts for b in o.slots()] + extra_bufs
    snap = [b.clone() for b in bufs]
    steps = [o.t for o in opts]
    for o in opts:
        o.set_lr(0.0)       # warm-up / capture passes must not move the weights
    try:
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            for _ in range(warmup):
                for body in warm or [b for _, _, b in bodies]:
                    body()
        torch.cuda.current_stream().wait_stream(s)
        torch.cuda.synchronize()
        quiesce_collectives()
        for g_name, out_name, body in bodies:
            g, out = capture(body)
            setattr(eng, g_name, g)
            if out_name is not None:
                setattr(eng, out_name, out)
        if it_body is not None:
            # Seven graph launches per iteration leave ~150 us of idle GPU at each boundary (profiles/r02_steady_state_resnet_v2.txt:
            # 1.07 ms of 20.5 ms; the DCGAN engine: ~20 gaps of 8-20 us, 4 % of the iteration); one graph per iteration has one boundary.
            # Optional: if only this capture fails (one more private pool), the per-step graphs stay in use.
            try:
                eng.it_graph, eng.it_out = capture(it_body)
            except Exception as e:
                eng.it_graph = eng.it_out = None
                eng.it_graph_error = '%s: %s' % (type(e).__name__, e)
                torch.cuda.synchronize()
                # an exception inside an active capture can leave the stream / pools in a bad state: prove the per-step graphs
                # still replay (weights do not move: the learning rate is 0 here) before relying on them
                for g_name, _, _ in bodies:
                    getattr(eng, g_name).replay()
                torch.cuda.synchronize()
    finally:
        torch.cuda.synchronize()
        for b, sn in zip(bufs, snap):
            b.copy_(sn)
        for o, n in zip(opts, steps):
            o.t, o._lr_last = n, None
        torch.cuda.synchronize()


def _capture_gan_graphs(eng, warmup, f_warm, d_body, g_body):
    """_capture_graphs for the two GAN engines: the critic and generator graphs, then - when the fake batches of an iteration come from one
    generator forward (warmed up by `f_warm`, ahead of the two steps) - the fake-batch graph and, with Adam inside the graphs, the
    whole-iteration graph."""
    t = eng.t
    warm, bodies = [d_body, g_body], [('d_graph', 'd_out', d_body), ('g_graph', 'g_out', g_body)]
    if eng.batch_fakes:
        warm.insert(0, f_warm)
        bodies.append(('f_graph', 'fake_all', eng._f_body))
    it_body = eng._it_body if eng.batch_fakes and eng.adam_in_graph and ITERATION_GRAPH else None
    _capture_graphs(eng, warmup, (t.d_opt, t.g_opt), [t.rng.ctr], bodies, warm, it_body)


def _capture_or_fall_back(eng, warmup):
    """The end of a wrapper's constructor: eng._capture(warmup), or - whatever it raised - eager launches with the reason in
    eng.graph_error (bench.py reports it) and every graph handle and graph output of the class (`_HANDLES`) None again."""
    try:
        eng._capture(warmup)
    except Exception as e:
        eng.graph_error = '%s: %s' % (type(e).__name__, e)
        for name in eng._HANDLES:
            setattr(eng, name, None)
        torch.cuda.synchronize()


class GraphedTrainer:
    def __init__(self, trainer, use_graphs=True, warmup=2, ar_in_graph=None):
        self.t = trainer
        B = R.cfg.BATCH_SIZE
        dev = trainer.dev
        self.real = torch.zeros(B, R.cfg.OUTPUT_DIM, dtype=torch.int32, device=dev)
        self.labels = torch.zeros(B, dtype=torch.int32, device=dev)
        # fake batches come from one batched generator forward per iteration (Trainer.generate_fakes)
        self.batch_fakes = R.BATCH_FAKES
        # static inputs of a whole iteration: the N_CRITIC real batches and their labels in ONE allocation, so that an iteration's
        # inputs are staged by one launch (K.pack with a pointer table) instead of 2 x N_CRITIC copies
        n_real = R.cfg.N_CRITIC * B * R.cfg.OUTPUT_DIM if self.batch_fakes else 0
        self._stage = torch.zeros(n_real + B * R.cfg.N_CRITIC, dtype=torch.int32, device=dev)
        self.labels_all = self._stage[n_real:]
        self.fake = torch.zeros(B, R.cfg.OUTPUT_DIM, dtype=torch.float32, device=dev) if self.batch_fakes else None
        self.f_graph = None
        self.fake_all = None
        self.it_graph = None          # ONE graph for a whole iteration (G step + fake batches + N_CRITIC critic steps), world == 1
        self.it_out = None
        self.real_all = self._stage[:n_real].view(R.cfg.N_CRITIC, B, R.cfg.OUTPUT_DIM) if self.batch_fakes else None
        self.ar_in_graph = bool(use_graphs and trainer.allreduce is not None and (trainer.world > 1 or getattr(trainer.allreduce, 'always', False))
                                and (ar_in_graph_default() if ar_in_graph is None else ar_in_graph))
        self.adam_in_graph = trainer.world == 1 or self.ar_in_graph
        self.d_graph = self.g_graph = None
        self.d_out = self.g_out = None
        self.graph_error = None
        self.it_graph_error = None    # only the whole-iteration graph failed to capture: the per-step graphs are in use (still `graphed`)
        if use_graphs:
            _capture_or_fall_back(self, warmup)

    def _weights_moved(self, group=None):
        """A replay with Adam inside the graph changed the weights AFTER the graph's own rebuild of the derived / packed filter
        images: tell the host-side version counter, so that an eager consumer after the replay (a stand-alone step, bench.py's
        instrumented passes, sample grids) rebuilds them instead of mixing fresh weights with images one step old."""
        if self.adam_in_graph:
            lib.bump_epoch(group)

    # -- the region that is captured (everything between input copy and all-reduce / Adam)
    def _d_body(self, real=None, labels=None, fake=None):
        t = self.t
        real = self.real if real is None else real
        labels = self.labels if labels is None else labels
        fake = self.fake if fake is None else fake
        # the critic's weights change between replays (its Adam step): its derived filter layouts must be rebuilt INSIDE
        # this graph - all of them in one or two launches.  The generator's are not used here (fake batches are inputs).
        lib.bump_epoch('Discriminator' if self.batch_fakes else None)
        F.prepare_filters()
        t.rng.begin_step()
        handed = [0]
        early = None
        if t.split_flush and t.world > 1 and t.allreduce is not None and t._n_early and self.ar_in_graph:
            # the bucket's prefix (blocks 1-2) goes to its all-reduce from inside the step: on the side stream - forked into the capture
            # when the collectives are graph nodes (RCCL) - under the rest of the penalty's double backward.  Not with the collective outside
            # the graph (gloo under graph replay): there the graph ends at the packed bucket.
            def early(gpart):
                handed[0] = t.early_reduce(gpart)
        out, grads = t.d_grads(real, labels, fake=fake, early=early)
        self._finish(t.d_opt, grads, lo=handed[0])
        return {k: out[k].detach() for k in ('cost', 'wgan', 'acgan', 'acc_real', 'acc_fake', 'ct', 'gp') if out.get(k) is not None}

    def _finish(self, opt, grads, lo=0):
        """End of a captured step body.  Adam inside the graph: bucket + update in one launch and the step end in another (single rank), or bucket,
        in-graph all-reduce, update + step end.  Adam outside (side-stream all-reduce): the graph ends at the packed bucket and at
        the Philox counter's own advance - Trainer.reduce_and_update must not advance it again, hence rng=None there."""
        t = self.t
        if self.adam_in_graph and not self.ar_in_graph:
            opt.update(grads, 1.0 / t.world, rng=t.rng)
            return
        part = opt.gather_grads(grads, lo)
        self._reduce_in_graph(part)
        if lo and hasattr(t.allreduce, 'wait'):
            t.allreduce.wait()              # join the forked collective of the bucket's prefix (Trainer.early_reduce)
        if self.adam_in_graph:
            opt.step(1.0 / t.world, rng=t.rng)
        else:
            t.rng.end_step()

    def _reduce_in_graph(self, flat):
        """The flat gradient bucket (or its remaining part) summed over the ranks ON the capturing stream: the collective becomes a node of
        the step graph."""
        if self.ar_in_graph:
            self.t.allreduce.inline(flat)

    def _it_body(self):
        """A whole iteration of the loop body (TF/CT_gan_cifar_resnet.py:393-404) with it > 0: generator step, the fake batches
        of the N_CRITIC critic steps, then the critic steps on rows of the static batch buffers."""
        B = R.cfg.BATCH_SIZE
        g_out = self._g_body()
        fakes = self._f_body()
        d_outs = [self._d_body(self.real_all[i], self.labels_all[i * B:(i + 1) * B], fakes[i]) for i in range(R.cfg.N_CRITIC)]
        return {'g': g_out, 'd': d_outs}

    def _f_body(self):
        lib.bump_epoch('Generator')      # runs after the generator update of the iteration
        return self.t.generate_fakes(self.labels_all)

    def _g_body(self):
        t = self.t
        lib.bump_epoch()
        F.prepare_filters()
        t.rng.begin_step()
        out = t.g_losses()
        with F.deferred_wgrads():
            grads = torch.autograd.grad(out['cost'], t.g_params, grad_outputs=t.cost_seed(out['cost']), allow_unused=True)
        self._finish(t.g_opt, grads)
        return {'cost': out['cost'].detach()}

    _HANDLES = ('d_graph', 'g_graph', 'f_graph', 'it_graph', 'd_out', 'g_out', 'fake_all', 'it_out')

    def _capture(self, warmup):
        _capture_gan_graphs(self, warmup, self._f_body, self._d_body, self._g_body)

    @property
    def graphed(self):
        return self.d_graph is not None

    def _stage_d_inputs(self, real_int, labels, fake):
        self.real.copy_(real_int, non_blocking=True)
        self.labels.copy_(labels, non_blocking=True)
        if self.batch_fakes:
            if fake is None:          # stand-alone critic step: draw its fake batch now (eager, no-grad)
                fake = self.t.generate_fakes(self.labels)[0]
            self.fake.copy_(fake, non_blocking=True)

    def _stage_iteration(self, batches):
        """The iteration's N_CRITIC (data, labels) batches -> the static input buffers, in one launch when they are device-resident
        dense int32 tensors (4-byte elements move as bit patterns through the gradient-bucket gather kernel)."""
        B, n_out = R.cfg.BATCH_SIZE, R.cfg.OUTPUT_DIM
        srcs = [d for d, _ in batches] + [lab for _, lab in batches]
        ok = all(x.is_cuda and x.device == self._stage.device and x.dtype == torch.int32 and x.is_contiguous() for x in srcs)
        ok = ok and all(d.numel() == B * n_out for d, _ in batches) and all(lab.numel() == B for _, lab in batches)
        if not ok or len(batches) != R.cfg.N_CRITIC:
            for i, (data, lab) in enumerate(batches):
                self.labels_all[i * B:(i + 1) * B].copy_(lab, non_blocking=True)
                self.real_all[i].copy_(data, non_blocking=True)
            return
        n = len(batches)
        offs = [i * B * n_out for i in range(n)] + [n * B * n_out + i * B for i in range(n)]
        counts = [B * n_out] * n + [B] * n
        K.pack([x.view(torch.float32) for x in srcs], offs, counts, self._stage.view(torch.float32))

    def d_step(self, real_int, labels, iteration=0, fake=None, staged=False, between=None):
        """One critic update.  world > 1: the graph ends at the packed gradient; the all-reduce runs on the side stream
        while `between()` (the NEXT step's input staging) is enqueued, then Adam (Trainer.reduce_and_update)."""
        t = self.t
        if not self.graphed:
            return t.d_step(real_int, labels, iteration=iteration, fake=fake)
        if not staged:
            self._stage_d_inputs(real_int, labels, fake)
        t.d_opt.set_lr(t.lr(iteration))
        self.d_graph.replay()
        if not self.adam_in_graph:
            t.reduce_and_update(t.d_opt, t.d_opt.grad, between, end_rng=False)
        else:
            t.d_opt.t += 1
            self._weights_moved('Discriminator')
            if between is not None:
                between()
        return self.d_out

    def g_step(self, iteration=0, between=None):
        t = self.t
        if not self.graphed:
            return t.g_step(iteration=iteration)
        t.g_opt.set_lr(t.lr(iteration))
        self.g_graph.replay()
        if not self.adam_in_graph:
            t.reduce_and_update(t.g_opt, t.g_opt.grad, between, end_rng=False)
        else:
            t.g_opt.t += 1
            self._weights_moved('Generator')
            if between is not None:
                between()
        return self.g_out

    def train_iteration(self, iteration, next_batch):
        """[G step if it>0] + N_CRITIC x (next batch, D step)   (TF/CT_gan_cifar_resnet.py:393-404).  The inputs of step
        k+1 are staged into the static buffers right after step k's graph has been enqueued - stream order keeps that
        safe - i.e. while step k's gradient all-reduce is in flight on the side stream (world > 1)."""
        if not self.batch_fakes:
            if iteration > 0:
                self.g_step(iteration)
            out = None
            for _ in range(R.cfg.N_CRITIC):
                data, labels = next_batch()
                out = self.d_step(data, labels, iteration)
            return out
        batches = [next_batch() for _ in range(R.cfg.N_CRITIC)]
        B = R.cfg.BATCH_SIZE
        if not self.graphed:
            if iteration > 0:
                self.g_step(iteration)
            fakes = self.t.generate_fakes(torch.cat([lab for _, lab in batches], 0))
            out = None
            for i, (data, labels) in enumerate(batches):
                out = self.d_step(data, labels, iteration, fake=fakes[i])
            return out

        def stage_labels():
            for i, (_, lab) in enumerate(batches):
                self.labels_all[i * B:(i + 1) * B].copy_(lab, non_blocking=True)
        if self.it_graph is not None and iteration > 0:
            t = self.t
            self._stage_iteration(batches)
            t.set_lr(t.lr(iteration))
            self.it_graph.replay()
            t.g_opt.t += 1
            t.d_opt.t += len(batches)
            self._weights_moved()
            self.g_out = self.it_out['g']
            return self.it_out['d'][-1]
        if iteration > 0:
            self.g_step(iteration, between=stage_labels)
        else:
            stage_labels()
        self.f_graph.replay()
        fakes = self.fake_all
        self._stage_d_inputs(batches[0][0], batches[0][1], fakes[0])
        out = None
        for i in range(len(batches)):
            nxt = None
            if i + 1 < len(batches):
                nxt = (lambda j: lambda: self._stage_d_inputs(batches[j][0], batches[j][1], fakes[j]))(i + 1)
            out = self.d_step(None, None, iteration, staged=True, between=nxt)
        return out


class GraphedDCGANTrainer:
    """hipGraph replay of the shared unconditional CT-WGAN step (dcgan_step.DCGANTrainer: the DCGAN scripts, the 64x64 and
    128x128 ResNets).  Same rules as GraphedTrainer: one private memory pool per graph, the Philox step counter / Adam state
    live in device memory, capture leaves no trace in them, Adam inside the graph when world == 1."""

    def __init__(self, trainer, real_shape, real_dtype, use_graphs=True, warmup=2):
        from . import dcgan_step
        self.t = trainer
        self.real = torch.zeros(real_shape, dtype=real_dtype, device=trainer.dev)
        # the fake batches of an iteration's critic steps come from ONE generator forward (a third graph, replayed once per iteration):
        # the critic graph then neither runs the generator nor rebuilds its derived / packed filters five times per iteration
        self.batch_fakes = dcgan_step.BATCH_FAKES
        self.fake = torch.zeros(real_shape[0], trainer.mod.cfg.OUTPUT_DIM, dtype=torch.float32, device=trainer.dev) if self.batch_fakes else None
        self.f_graph = None
        self.fake_all = None
        # ONE graph for a whole iteration (generator step, the fake batches, CRITIC_ITERS critic steps on rows of a static batch buffer),
        # as GraphedTrainer's: seven graph launches and their input copies per iteration leave ~20 idle gaps of 8-20 us (rocprofv3,
        # config[1]: 4 % of the iteration)
        self.it_graph = None
        self.it_out = None
        self.it_graph_error = None
        n_it = trainer.disc_iters
        self.real_all = torch.zeros((n_it,) + tuple(real_shape), dtype=real_dtype, device=trainer.dev) if self.batch_fakes else None
        self.adam_in_graph = trainer.world == 1
        self.d_graph = self.g_graph = None
        self.d_out = self.g_out = None
        self.graph_error = None
        if use_graphs:
            _capture_or_fall_back(self, warmup)

    def _it_body(self):
        g_out = self._body('g')
        fakes = self._f_body()
        return {'g': g_out, 'd': [self._body('d', self.real_all[i], fakes[i]) for i in range(self.t.disc_iters)]}

    def _f_body(self):
        lib.bump_epoch('Generator')       # runs after the generator update of the iteration
        F.prepare_filters()
        return self.t.generate_fakes(self.t.disc_iters)

    def _body(self, which, real=None, fake=None):
        t = self.t
        # weights changed since the last replay: derived / packed filters are rebuilt in-graph - the critic's only in the critic graph
        # when its fake batch is an input (the generator's are rebuilt by the fake-batch graph)
        lib.bump_epoch('Discriminator' if (which == 'd' and self.batch_fakes) else None)
        F.prepare_filters()
        t.rng.begin_step()
        if which == 'd':
            out, grads = t.d_grads(self.real if real is None else real, fake=self.fake if fake is None else fake)
            opt = t.d_opt
        else:
            out = t.g_losses()
            params, opt = t.g_params, t.g_opt
            with F.deferred_wgrads():       # the step's queued weight gradients in one grouped launch, as the ResNet step
                grads = torch.autograd.grad(out['cost'], params, grad_outputs=t.cost_seed().reshape(out['cost'].shape), allow_unused=True)
        if self.adam_in_graph:
            opt.update(grads, 1.0 / t.loss_scale, rng=t.rng)
        else:
            opt.gather_grads(grads)
            t.rng.end_step()
        return {k: out[k].detach() for k in ('cost', 'wgan_only', 'ct', 'gp') if out.get(k) is not None}

    _HANDLES = GraphedTrainer._HANDLES

    def _capture(self, warmup):
        # (the warm-up's critic steps read a real fake batch, not the zeros the static buffer starts with)
        _capture_gan_graphs(self, warmup, lambda: self.fake.copy_(self._f_body()[0]), lambda: self._body('d'), lambda: self._body('g'))

    @property
    def graphed(self):
        return self.d_graph is not None

    def _lr(self):
        return self.t.lr()

    def d_step(self, real_in, fake=None):
        t = self.t
        if not self.graphed:
            return t.d_step(real_in, fake=fake)
        self.real.copy_(real_in, non_blocking=True)
        if self.batch_fakes:
            if fake is None:            # a stand-alone critic step: draw its fake batch now
                fake = t.generate_fakes(1)[0]
            self.fake.copy_(fake, non_blocking=True)
        t.d_opt.set_lr(self._lr())
        self.d_graph.replay()
        if self.adam_in_graph:
            t.d_opt.t += 1
            lib.bump_epoch()           # the in-graph Adam step ran after the graph's own filter rebuild (see GraphedTrainer._weights_moved)
        else:
            self._reduce_update(t.d_opt)
        t.clip_stats()
        return self.d_out

    def g_step(self):
        t = self.t
        if not self.graphed:
            return t.g_step()
        t.g_opt.set_lr(self._lr())
        self.g_graph.replay()
        if self.adam_in_graph:
            t.g_opt.t += 1
            lib.bump_epoch()
        else:
            self._reduce_update(t.g_opt)
        return self.g_out

    def _reduce_update(self, opt):
        t = self.t
        if t.allreduce is not None and t.world > 1:
            t.allreduce(opt.grad)
            if hasattr(t.allreduce, 'wait'):
                t.allreduce.wait()
        opt.step(1.0 / (t.world * t.loss_scale))

    def train_iteration(self, iteration, next_batch):
        """[G step if it > 0] + disc_iters x (batch, D step)  (TF/CT_gan_cifar.py:190-204; disc_iters = CRITIC_ITERS, or 1 for the
        'dcgan' / 'lsgan' objectives)."""
        self.t.iteration = iteration
        n = self.t.disc_iters
        if self.it_graph is not None and iteration > 0:
            t = self.t
            for i in range(n):
                self.real_all[i].copy_(next_batch(), non_blocking=True)
            lr = self._lr()
            t.d_opt.set_lr(lr); t.g_opt.set_lr(lr)
            self.it_graph.replay()
            t.g_opt.t += 1
            t.d_opt.t += n
            lib.bump_epoch()
            t.clip_stats()
            self.g_out = self.it_out['g']
            return self.it_out['d'][-1]
        if iteration > 0:
            self.g_step()
        out = None
        fakes = None
        if self.batch_fakes:
            if self.graphed:
                self.f_graph.replay()
                fakes = self.fake_all
            else:
                fakes = self.t.generate_fakes(n)
        for i in range(n):
            out = self.d_step(next_batch(), fake=None if fakes is None else fakes[i])
        return out


class GraphedSSLTrainer:
    """hipGraph replay of the two steps of ct_mnist.SSLTrainer.  Each step - forward, backward, gradient packing, Theano-form Adam with
    the parameter average, the advance of Adam's beta powers and of the Philox step counter - is captured once on a single stream (no
    parallel branches) and replayed; the batches are staged into fixed buffers, the learning rate, beta powers and stream counter live
    in device memory.  The capture's warm-up runs at learning rate 0 and every slot it touches (Adam m, v, state, the averages, the
    stream counter) is restored afterwards, so a graphed run equals an eager one bit for bit."""

    def __init__(self, trainer, use_graphs=True, warmup=2):
        self.t = trainer
        self._alloc_staging()
        self.d_graph = self.g_graph = None
        self.d_out = self.g_out = None
        self.graph_error = None
        if use_graphs:
            _capture_or_fall_back(self, warmup)

    def _alloc_staging(self):
        """The fixed buffers the batches are staged into (what the captured steps read)."""
        from . import ct_mnist as M
        B, dev = M.cfg.BATCH_SIZE, self.t.dev
        self.x_lab = torch.zeros(B, M.cfg.IN_DIM, dtype=torch.float32, device=dev)
        self.x_unl = torch.zeros(B, M.cfg.IN_DIM, dtype=torch.float32, device=dev)
        self.x_unl2 = torch.zeros(B, M.cfg.IN_DIM, dtype=torch.float32, device=dev)
        self.labels = torch.zeros(B, dtype=torch.int32, device=dev)

    def _d_body(self):
        return self.t.d_body(self.x_lab, self.labels, self.x_unl)

    def _g_body(self):
        return self.t.g_body(self.x_unl2)

    def _extra_slots(self):
        """Further device buffers the bodies write, snapshotted and restored around the capture with the optimizers' slots."""
        return []

    _HANDLES = ('d_graph', 'g_graph', 'd_out', 'g_out')

    def _capture(self, warmup):
        t = self.t
        _capture_graphs(self, warmup, (t.d_opt, t.g_opt), [t.rng.ctr] + self._extra_slots(),
                        [('d_graph', 'd_out', self._d_body), ('g_graph', 'g_out', self._g_body)])

    @property
    def graphed(self):
        return self.d_graph is not None

    def d_step(self, x_lab, labels, x_unl):
        t = self.t
        if not self.graphed:
            dev = t.dev
            return t.d_step(x_lab.to(dev), labels.to(dev), x_unl.to(dev))
        self.x_lab.copy_(x_lab, non_blocking=True)
        self.labels.copy_(labels, non_blocking=True)
        self.x_unl.copy_(x_unl, non_blocking=True)
        t.d_opt.set_lr(t.lr())
        self.d_graph.replay()
        t.d_opt.t += 1
        lib.bump_epoch('Classifier')
        return self.d_out

    def g_step(self, x_unl2):
        t = self.t
        if not self.graphed:
            return t.g_step(x_unl2.to(t.dev))
        self.x_unl2.copy_(x_unl2, non_blocking=True)
        t.g_opt.set_lr(t.lr())
        self.g_graph.replay()
        t.g_opt.t += 1
        lib.bump_epoch('Generator')
        return self.g_out

    def train_iteration(self, x_lab, labels, x_unl, x_unl2):
        out = dict(self.d_step(x_lab, labels, x_unl))
        out.update(self.g_step(x_unl2))
        self.t.iteration += 1
        return out


class GraphedCifarSSLTrainer(GraphedSSLTrainer):
    """GraphedSSLTrainer for ct_cifar.CifarSSLTrainer: what is staged are the INDEX batches into the trainer's device-resident uint8
    set, and the augmenting gathers (kernels.aug_gather, drawn at the step's own counter value) are the first launches of the two
    captured graphs.  The steps take int32 index / label tensors (host or device)."""

    def _alloc_staging(self):
        from . import ct_cifar as M
        assert self.t.data is not None, 'bind the uint8 training set first (CifarSSLTrainer.bind_data)'
        B, dev = M.cfg.BATCH_SIZE, self.t.dev
        self.x_lab = torch.zeros(B, dtype=torch.int32, device=dev)
        self.x_unl = torch.zeros(B, dtype=torch.int32, device=dev)
        self.x_unl2 = torch.zeros(B, dtype=torch.int32, device=dev)
        self.labels = torch.zeros(B, dtype=torch.int32, device=dev)

    def _d_body(self):
        return self.t.d_body_idx(self.x_lab, self.labels, self.x_unl)

    def _g_body(self):
        return self.t.g_body_idx(self.x_unl2)

    def d_step(self, i_lab, labels, i_unl):
        t = self.t
        if not self.graphed:
            dev = t.dev
            t.d_opt.set_lr(t.lr())
            return t.d_body_idx(i_lab.to(dev), labels.to(dev), i_unl.to(dev))
        return super().d_step(i_lab, labels, i_unl)

    def g_step(self, i_unl2):
        t = self.t
        if not self.graphed:
            t.g_opt.set_lr(t.lr())
            return t.g_body_idx(i_unl2.to(t.dev))
        return super().g_step(i_unl2)


class GraphedCifarTETrainer(GraphedCifarSSLTrainer):
    """GraphedCifarSSLTrainer for ct_cifar_te.CifarTETrainer.  Staged are i_lab, labels, i_unl and i_unl2; the staged i_unl serves the
    augmenting gather AND the loss head, which reads the target rows and writes the prediction rows of those indices inside the
    captured classifier graph (kernels.te_head_fwd / te_head_bwd) - no table row crosses to the host within an epoch.  One stream,
    no parallel branches.  The capture's warm-up runs on the staged all-zero indices (duplicates: memory-safe) and so writes row 0
    of the two prediction tables: both tables are snapshotted and restored with the other slots, so a graphed run equals an eager
    one bit for bit, tables included.  The graphs hold the tables' addresses: CifarTETrainer changes them in place only
    (end_epoch, load_te_state); bind the data before building the engine.  end_epoch() is not captured - two launches per epoch."""

    def _extra_slots(self):
        t = self.t
        assert t.epoch_pred is not None, 'bind the uint8 training set first (CifarTETrainer.bind_data allocates the tables)'
        return [t.epoch_pred, t.epoch_pred2]


class GraphedScoreTrainer:
    """hipGraph replay of score_mnist.ScoreTrainer's train step (forward, backward, gradient packing, global-norm clip, Adam) and of its
    statistics pass (the training-mode forward that moves the moving statistics), on the pattern of GraphedSSLTrainer: one stream, no
    parallel branches, the batch staged into fixed buffers; the learning rate, Adam's beta powers and `stats_iter` live in device
    memory, so both graphs replay with the values current at replay.  The warm-up runs at learning rate 0 and every buffer it writes
    (Adam's slots, the moving statistics, stats_iter) is restored afterwards: a graphed run equals an eager one bit for bit."""

    def __init__(self, trainer, use_graphs=True, warmup=2):
        from . import score_mnist as M
        self.t = trainer
        B, dev = M.cfg.BATCH_SIZE, trainer.dev
        self.x = torch.zeros(B, 784, dtype=torch.float32, device=dev)
        self.y = torch.zeros(B, dtype=torch.int32, device=dev)
        self.step_graph = self.stats_graph = None
        self.step_out = None
        self.graph_error = None
        if use_graphs:
            _capture_or_fall_back(self, warmup)

    def _step_body(self):
        lib.bump_epoch('InceptionScore')      # weights changed since the last replay: derived / packed filters are rebuilt in-graph
        F.prepare_filters()
        return self.t.body(self.x, self.y)

    def _stats_body(self):
        lib.bump_epoch('InceptionScore')
        F.prepare_filters()
        self.t.stats_body(self.x)

    _HANDLES = ('step_graph', 'stats_graph', 'step_out')

    def _capture(self, warmup):
        t = self.t
        _capture_graphs(self, warmup, (t.opt,), [p.data for _, p in t.moving_stats()] + [t.stats_iter],
                        [('step_graph', 'step_out', self._step_body), ('stats_graph', None, self._stats_body)])

    @property
    def graphed(self):
        return self.step_graph is not None

    def step(self, x, y):
        """-> cost, acc, gradnorm of one train step on (x [B,784] float32, y [B] int32), host or device tensors."""
        t = self.t
        if not self.graphed:
            return t.step(x, y)
        self.x.copy_(x, non_blocking=True)
        self.y.copy_(y, non_blocking=True)
        t.opt.set_lr(t.lr())
        t.stats_iter.fill_(0)
        self.step_graph.replay()
        t.opt.t += 1
        t.iteration += 1
        lib.bump_epoch('InceptionScore')
        out = self.step_out
        return out['cost'], out['acc'], out['gradnorm']

    def bn_stats_pass(self, x, i):
        t = self.t
        if not self.graphed:
            return t.bn_stats_pass(x, i)
        self.x.copy_(x, non_blocking=True)
        t.stats_iter.fill_(i)
        self.stats_graph.replay()
        lib.bump_epoch('InceptionScore')
