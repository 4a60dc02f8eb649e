"""The reference's self-trained MNIST score classifier: LS/inception_score.py with the parts of LS/tflib/train_loop_2.py and
LS/tflib/ops/batchnorm.py it uses (LS/ = tensorflow_generative_model/LSUN_bedrooms of the reference).  A small ELU ResNet with batch
norm, trained by softmax cross-entropy on MNIST itself - no outside weights - whose class posteriors score MNIST samples.

    script line                                               here
    LS/inception_score.py:25-35   LR, BATCH_SIZE, TIMES        Config
    :38-39                        nonlinearity = tf.nn.elu     functional.elu (csrc/score.hip)
    :52-93                        ResidualBlock                ResidualBlock ('up' and mask_type raise: build_model uses neither)
    :95-108                       build_model, the network     Classifier
    :118-130                      cost, acc                    functional.softmax_cross_entropy (loss, ncorrect)
    :132-135                      inception_score (fp64)       ScoreTrainer.evaluate -> inception_from_logits
    :139-165                      train_model                  train
    :167-178                      run_model                    InceptionScore.score
    :180-197                      InceptionScore               InceptionScore
    LS/tflib/train_loop_2.py:76-79  global norm, clip at 5     optim.FlatAdam.update_clipped (csrc/score.hip)
    :84-111                       train_fn/bn_stats_fn/eval_fn ScoreTrainer.step / bn_stats_pass / evaluate
    :196-280                      the loop                     train (_schedule)
    LS/tflib/ops/batchnorm.py:30-69                            tflib.ops.batchnorm.Batchnorm(is_training=..., stats_iter=...)

The script as written cannot run: it passes `is_training_var=` to a train_loop whose parameter is `bn_vars`, calls
Batchnorm without the `stats_iter` its `update_moving_stats=True` needs, and run_model feeds no `is_training`.  What is built here is
the meaning train_loop_2's `bn_vars = (is_training, stats_iter)` spells out: train steps run with (True, 0), every TEST_EVERY
iterations BN_STATS_ITERS forward passes over training data run with (True, i) so that the moving statistics become the plain mean of
those batches' statistics, then the dev set is evaluated with (False, 0); scoring runs in inference mode.

Kept as written: the inference-mode batch norm blends every sample's own moments with the moving statistics by the ROW COUNT of the
call (weights 1/B and (B-1)/B), so a score depends on its chunk size; `stats_iter = 0` in a train step replaces the moving statistics
by that batch's; the test pass runs at iteration % TEST_EVERY == TEST_EVERY - 1; at the end of a training epoch the loop drops the
second batch of the next one (train_loop_2.py:215-217).
"""
import os
import time

import numpy as np
import torch

from . import ct_common
from . import functional as F
from . import tflib as lib
from .optim import FlatAdam
from .tflib.ops import batchnorm as _bn
from .tflib.ops import conv2d as _conv2d
from .tflib.ops import linear as _linear

DEFAULT_PATH = '/tmp/inception_score.pt'          # (the script's /tmp/inception_score.ckpt, :186)


class Config(ct_common.Config):
    """The literals of LS/inception_score.py:25-35, :93, :102-108 and of LS/tflib/train_loop_2.py:33-36, :79 (tests shrink them)."""
    LR = 1e-3
    BETA1 = 0.9
    BETA2 = 0.999
    ADAM_EPS = 1e-8
    BATCH_SIZE = 500
    ITERS_PER_EPOCH = 100              # 50000 / BATCH_SIZE
    STOP_AFTER = 900                   # 9 epochs
    TEST_EVERY = 100
    BN_STATS_ITERS = 1000
    SAVE_EVERY = 1000
    CLIP_NORM = 5.
    RES_SCALE = .3
    WIDTHS = (32, 32, 32, 64, 64)      # Conv1, Res1 .. Res4
    N_CLASSES = 10


cfg = Config()


def configure(**kw):
    global cfg
    cfg = Config(**kw)
    return cfg


def ResidualBlock(name, input_dim, output_dim, inputs, filter_size, is_training, stats_iter=None, resample=None, he_init=True,
                  mask_type=None, elu_in=None, want_elu=False):
    """:52-93.  Build-only: elu_in = elu(inputs) where the caller already has it; want_elu: also return elu(result) - both come from
    the previous / this block's fused epilogue (Batchnorm(resid=..., want_elu=...))."""
    if mask_type is not None:
        raise NotImplementedError('ResidualBlock: masked convolutions are not used by build_model')
    if resample == 'down':
        shortcut_stride, dims_1, dims_2, stride_2 = 2, (input_dim, input_dim), (input_dim, output_dim), 2
    elif resample == 'up':
        raise NotImplementedError("ResidualBlock: resample='up' (SubpixelConv2D) is not used by build_model")
    elif resample is None:
        shortcut_stride, dims_1, dims_2, stride_2 = 1, (input_dim, output_dim), (output_dim, output_dim), 1
    else:
        raise Exception('invalid resample value')
    if output_dim == input_dim and resample is None:
        shortcut = inputs                           # identity skip-connection
    else:
        shortcut = _conv2d.Conv2D(name + '.Shortcut', input_dim, output_dim, 1, inputs, he_init=False, biases=True, stride=shortcut_stride)
    output = elu_in if elu_in is not None else F.elu(inputs)
    output = _conv2d.Conv2D(name + '.Conv1', dims_1[0], dims_1[1], filter_size, output, he_init=he_init)
    output = F.elu(output)
    output = _conv2d.Conv2D(name + '.Conv2', dims_2[0], dims_2[1], filter_size, output, he_init=he_init, stride=stride_2)
    # shortcut + 0.3 * Batchnorm(output) [and its ELU for the next block] in the normalisation's apply pass
    return _bn.Batchnorm(name + '.BN', [0, 2, 3], output, is_training, stats_iter, update_moving_stats=True, resid=shortcut,
                         resid_scale=cfg.RES_SCALE, want_elu=want_elu)


def Classifier(inputs, is_training, stats_iter=None):
    """:95-108: inputs [N,784] -> logits [N,10].  is_training: a Python bool (True needs stats_iter: an int or a device scalar)."""
    W = cfg.WIDTHS
    output = inputs.reshape(-1, 1, 28, 28)
    output = _conv2d.Conv2D('InceptionScore.Conv1', 1, W[0], 3, output, he_init=False)
    act = F.elu(output)
    output, act = ResidualBlock('InceptionScore.Res1', W[0], W[1], output, 3, is_training, stats_iter, resample='down', elu_in=act, want_elu=True)
    output, act = ResidualBlock('InceptionScore.Res2', W[1], W[2], output, 3, is_training, stats_iter, resample=None, elu_in=act, want_elu=True)
    output, act = ResidualBlock('InceptionScore.Res3', W[2], W[3], output, 3, is_training, stats_iter, resample='down', elu_in=act, want_elu=True)
    output = ResidualBlock('InceptionScore.Res4', W[3], W[4], output, 3, is_training, stats_iter, resample=None, elu_in=act)
    output = F.spatial_mean(output)
    return _linear.Linear('InceptionScore.Linear', W[4], cfg.N_CLASSES, output)


def build_params():
    """Register every parameter (lib.param creates on first use) with one tiny inference pass."""
    with torch.no_grad():
        Classifier(torch.zeros(2, 784, device=lib._dev()), False)


def inception_from_logits(logits):
    """:132-135 / :174-177 on the host in fp64: exp(mean_i sum_k p_ik (log p_ik - log mean_i p_ik)) with p = softmax(logits)."""
    z = np.asarray(logits, dtype=np.float64)
    p = np.exp(z - z.max(axis=-1, keepdims=True))
    p = p / p.sum(axis=-1, keepdims=True)
    kl = p * (np.log(p) - np.log(p.mean(axis=0, keepdims=True)))
    return float(np.exp(np.mean(np.sum(kl, axis=1))))


class ScoreTrainer:
    """train_fn / bn_stats_fn / eval_fn of LS/tflib/train_loop_2.py:84-111 for the classifier.  `stats_iter` is a float32 device
    scalar every training-mode pass reads, so the two captured graphs of engine.GraphedScoreTrainer replay with its current value."""
    cfg = property(lambda self: cfg)
    g_opt = None            # (checkpoint.py: one optimizer, no random stream)
    rng = None

    def __init__(self):
        self.dev = lib._dev()
        build_params()
        self.named = lib.named_params_with_name('InceptionScore', trainable_only=True)
        self.params = [p for _, p in self.named]
        self.opt = self.d_opt = FlatAdam(self.named, cfg.BETA1, cfg.BETA2, cfg.ADAM_EPS)
        self.stats_iter = torch.zeros(1, dtype=torch.float32, device=self.dev)
        self.iteration = 0

    def moving_stats(self):
        """[(name, tensor)] of the moving statistics, in registry order."""
        return [(n, p) for n, p in lib.named_params_with_name('InceptionScore') if n.endswith(('.moving_mean', '.moving_variance'))]

    def lr(self):
        return cfg.LR

    # ---- train step (train_fn: is_training True, stats_iter 0)
    def losses(self, x, y):
        logits = Classifier(x, True, self.stats_iter)
        cost, ncorrect = F.softmax_cross_entropy(logits, y)
        return {'cost': cost, 'acc': ncorrect.detach() / x.shape[0], 'logits': logits}

    def body(self, x, y):
        """Losses, gradients, global-norm clip, Adam - everything a replayed graph holds (learning rate and stats_iter are device state)."""
        out = self.losses(x, y)
        grads = torch.autograd.grad(out['cost'], self.params, allow_unused=True)
        gradnorm = self.opt.update_clipped(grads, cfg.CLIP_NORM)
        return {'cost': out['cost'].detach(), 'acc': out['acc'], 'gradnorm': gradnorm.reshape(())}

    def step(self, x, y):
        """-> cost, acc, gradnorm (device scalars; gradnorm is the norm before the clip)."""
        self.opt.set_lr(self.lr())
        self.stats_iter.fill_(0)
        out = self.body(x.to(self.dev), y.to(self.dev))
        self.iteration += 1
        return out['cost'], out['acc'], out['gradnorm']

    # ---- bn_stats_fn: a training-mode forward that only moves the moving statistics
    def stats_body(self, x):
        with torch.no_grad():
            Classifier(x, True, self.stats_iter)

    def bn_stats_pass(self, x, i):
        self.stats_iter.fill_(i)
        self.stats_body(x.to(self.dev))

    # ---- eval_fn and run_model's forward: inference mode
    def logits(self, x):
        with torch.no_grad():
            return Classifier(torch.as_tensor(x, dtype=torch.float32).to(self.dev), False)

    def evaluate(self, x, y):
        """-> cost, acc, inception (floats) of one batch in inference mode."""
        z = self.logits(x)
        with torch.no_grad():
            cost, ncorrect = F.softmax_cross_entropy(z, torch.as_tensor(y).to(device=self.dev, dtype=torch.int32))
        return float(cost.item()), float(ncorrect.item()) / z.shape[0], inception_from_logits(z.double().cpu().numpy())


def _schedule(train_data, dev_data, stop_after, test_every, bn_stats_iters):
    """The data side of LS/tflib/train_loop_2.py:196-280 as a stream of events (kind, at, epoch, payload, i): 'train' with the batch of
    the step after `at` completed ones; once `at` steps are complete and at % test_every == test_every - 1, the 'stats' batches
    i = 0, 1, .. of a fresh training epoch stream, the 'dev' batches and one 'test_end'.  Every factory call and every batch drawn
    happens here, in the loop's order - a resumed run replays the stream to its position."""
    gen, epoch = train_data(), 0
    for iteration in range(stop_after):
        try:
            batch = next(gen)
        except StopIteration:
            gen = train_data()
            batch = next(gen)
            next(gen, None)                          # :217, as written
            epoch += 1
        yield 'train', iteration, epoch, batch, None
        done = iteration + 1
        if dev_data is not None and done % test_every == test_every - 1:
            stats_gen = train_data()
            for i in range(bn_stats_iters):
                try:
                    b = next(stats_gen)
                except StopIteration:
                    stats_gen = train_data()
                    b = next(stats_gen)
                yield 'stats', done, epoch, b, i
            for b in dev_data():
                yield 'dev', done, epoch, b, None
            yield 'test_end', done, epoch, None, None


def _factories(data):
    if isinstance(data, (str, bytes, os.PathLike)):
        from .tflib import mnist
        return mnist.load(cfg.BATCH_SIZE, cfg.BATCH_SIZE, filepath=data)          # :144-147
    return tuple(data)


def train(data, iters=None, use_graphs=True, out_dir=None, resume=None, log=print):
    """train_model (:139-165) = LS/tflib/train_loop_2.train_loop under its bn_vars protocol.  data: the path of an mnist.pkl.gz (read
    through tflib.mnist.load; nothing is downloaded) or a (train, dev, test) triple of epoch factories yielding (images [B,784] float32,
    targets [B]).  iters: STOP_AFTER.  Train steps and statistics passes replay from hipGraphs unless use_graphs=False.  Every
    SAVE_EVERY iterations (same phase as the test pass) and at the end a checkpoint (checkpoint.py: parameters with the moving
    statistics, Adam's state) goes to `out_dir`; `resume` continues from one, bit for bit, given the same data stream (the factories'
    draws are replayed up to the checkpoint's iteration).  Returns the trainer."""
    from . import checkpoint
    from .engine import GraphedScoreTrainer
    from .train_log import Series
    train_data, dev_data, _ = _factories(data)
    lib.delete_params_with_name('InceptionScore')
    trainer = ScoreTrainer()
    start = checkpoint.load(resume, trainer) if resume else 0
    trainer.iteration = start
    eng = GraphedScoreTrainer(trainer, use_graphs=use_graphs)
    series = Series(os.path.join(out_dir, 'log.jsonl') if out_dir else None, echo=None)
    series.iteration = start
    stop = cfg.STOP_AFTER if iters is None else iters
    tests, seconds = [], 0.

    def save(done):
        if out_dir:
            checkpoint.save(os.path.join(out_dir, 'checkpoint.pt'), trainer, done)

    def wants_save(done):
        return done % cfg.SAVE_EVERY == cfg.SAVE_EVERY - 1 or done == stop

    def images(payload):
        return torch.from_numpy(np.asarray(payload[0], dtype=np.float32))

    for kind, at, epoch, payload, i in _schedule(train_data, dev_data, stop, cfg.TEST_EVERY, cfg.BN_STATS_ITERS):
        if at < start or (kind != 'train' and at == start):
            continue                                  # before the checkpoint: only the data stream moves
        if kind == 'train':
            begin = time.time()
            cost, acc, gradnorm = eng.step(images(payload), torch.from_numpy(np.asarray(payload[1]).astype(np.int32)))
            vals = torch.stack([cost, acc, gradnorm]).tolist()
            seconds += time.time() - begin
            done = at + 1
            log('epoch:%d\titeration:%d\tseconds:%.4f\ttrain cost:%.4f\ttrain acc:%.4f\ttrain gradnorm:%.4f'
                % (epoch, done, seconds, vals[0], vals[1], vals[2]))
            for k, v in zip(('train cost', 'train acc', 'train gradnorm'), vals):
                series.add(k, v)
            series.tick()
            if wants_save(done) and (dev_data is None or done % cfg.TEST_EVERY != cfg.TEST_EVERY - 1):
                series.flush()
                save(done)
        elif kind == 'stats':
            eng.bn_stats_pass(images(payload), i)
        elif kind == 'dev':
            tests.append(trainer.evaluate(payload[0], payload[1]))
        else:
            m = np.array(tests).mean(axis=0)
            tests = []
            log('epoch:%d\titeration:%d\tseconds:%.4f\ttest cost:%.4f\ttest acc:%.4f\ttest inception:%.4f' % (epoch, at, seconds, m[0], m[1], m[2]))
            for k, v in zip(('test cost', 'test acc', 'test inception'), m):
                series.add(k, float(v))
            series.flush()
            if wants_save(at):
                save(at)
    series.flush()
    return trainer


class InceptionScore:
    """:180-197.  Loads the classifier's weights from `weights`, or - retrain, or no such file - trains it on `data` (see train) and
    saves them there."""

    def __init__(self, weights=DEFAULT_PATH, retrain=False, data=None, **train_kw):
        if (not retrain) and weights is not None and os.path.isfile(weights):
            sd = torch.load(weights, map_location='cpu', weights_only=False)['params']
            lib.delete_params_with_name('InceptionScore')
            lib.load_state_dict(sd, strict=False)
            self.trainer = ScoreTrainer()
        else:
            if data is None:
                raise ValueError('InceptionScore: no saved weights at %s - pass data= (an mnist.pkl.gz path or epoch factories) to train' % weights)
            self.trainer = train(data, **train_kw)
            if weights is not None:
                torch.save({'format': 1, 'params': {n: p.detach().cpu().clone() for n, p in lib.named_params_with_name('InceptionScore')}}, weights)

    def _logits(self, x):
        return self.trainer.logits(x).double().cpu().numpy()

    def score(self, data):
        """run_model (:167-178): chunks of min(1000, len(data)) rows in inference mode, fp64 softmax and KL on the host."""
        step = min(1000, len(data))
        return inception_from_logits(np.concatenate([self._logits(data[i:i + step]) for i in range(0, len(data), step)], axis=0))

    def score_generator(self, gan_trainer, n):
        """The score of `n` samples of gan_mnist.Generator under the weights of `gan_trainer` (a dcgan_step.DCGANTrainer on gan_mnist),
        drawn on the trainer's EVALUATION stream (evaluate.eval_stream) in chunks of min(1000, n) and handed to the classifier as
        device tensors: the training stream, the weights and the optimizers are untouched."""
        from . import gan_mnist
        from .evaluate import eval_stream
        mod = getattr(gan_trainer, 'mod', gan_mnist)
        if mod is not gan_mnist:
            raise ValueError('score_generator scores gan_mnist samples (one 28x28 channel)')
        rng = eval_stream(gan_trainer)
        step, logits = min(1000, n), []
        for i in range(0, n, step):
            rng.begin_step()
            with torch.no_grad():
                x = mod.Generator(min(step, n - i), rng=rng)
            rng.end_step()
            logits.append(self._logits(x))
        return inception_from_logits(np.concatenate(logits, axis=0))
