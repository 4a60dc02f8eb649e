"""Semi-supervised CT classifier for MNIST: TH/CT_MNIST.py with the parts of TH/nn.py it uses (TH/ = CT-GANs/Theano_classifier of
the reference) - the experiment behind the paper's semi-supervised table.  `Classifier(inputs)` / `Generator(n_samples)` in the shape
of the other script modules, `SSLTrainer` for the two steps, `SSLData` for the labelled pick and the per-epoch streams, `train()` for
the script's loop.

Classifier D (TH/CT_MNIST.py:41-53): x + 0.3 N -> five weight-normalised ReLU layers 1000, 500, 250, 250, 250, each followed by
+ 0.5 N -> a weight-normalised linear layer to the 10 logits.  Trainable: every theta and b, and the weight_scale of the LAST layer
only (train_scale=True, :53); the other scales are set once by the data-dependent init (:60-62, :137) and never trained.
Generator G (:33-38): z ~ U[0,1) [B,100] -> Dense 500 (Glorot-uniform W, no bias) + batch norm (batch statistics, eps 1e-6, offset,
no gain) + softplus, twice -> Dense 784 with the l2-normalised weight W W_scale / sqrt(1e-6 + column sums of W^2), bias, sigmoid.  The
batch norm's running averages are never read by the script and are not kept.

Classifier step (:64-90, :103-110): four noisy passes - labelled, unlabelled twice, G(z) - run as ONE stacked 4B-row batch
[lab ; unl ; unl2 ; fake]; cost = loss_lab + UNLABELED_WEIGHT loss_unl, loss_unl = (CT - mean lse(unl) + mean softplus(lse(unl)) +
mean softplus(lse(fake))) / 2, CT = mean_i max(LAMBDA_2 ct_i - Factor_M, 0), ct_i = mean_k (softmax(unl) - softmax(unl2))_ik^2.  The
script's penultimate-layer consistency term (:82) is weighted 0.0 in :84 and is left out; its second generated pass (:68) feeds no
cost and is not computed.  Only the classifier moves; G(z) is a constant.  After the Adam update every trained parameter's average
moves by avg += 1e-4 (p - avg) from ZERO (:104-105) - the script's behaviour, kept: after few updates the averaged weights are
still close to zero.  Generator step (:92-94, :108, :111): loss_gen = mean_j (mean_i f(G(z))_ij - mean_i f(x)_ij)^2 with f the fifth
layer's ReLU output of a noisy pass over [G(z) ; x]; only G moves (the classifier's parameters enter as constants).  Adam is the
Theano form of TH/nn.py:30-47 (optim.FlatAdamTheano), beta1 0.5, lr 0.003 constant.  Test error (:97-98, :112): the deterministic
pass on the averaged parameters with the live weight scales of layers 1-5.

Random numbers.  Theano's MRG streams are not reproducible; as everywhere in this project the device draws Philox4x32-10 streams
(csrc/philox.h, rng.DeviceRNG) addressed by (seed, stream id, step, element), which oracle/philox.py regenerates in numpy
(`uniform` / `normal` with the same arguments).  The step counter advances by one per init pass, classifier step and generator
step.  Stream ids (= call-site index within one step, rank 0):
    init pass        0      input noise over the init rows [n, IN_DIM]           1..5   noise after hidden layer 1..5
    classifier step  0      z, uniform [B, Z_DIM]                                1      input noise over the stacked [4B, IN_DIM]
                     2..6   noise after hidden layer 1..5 over [4B, width]
    generator step   0      z                                                    1      input noise over the stacked [2B, IN_DIM]
                     2..5   noise after hidden layer 1..4 (the fifth layer's pre-noise output is the feature)
Element (r, c) of a [rows, cols] site is value r * cols + c of its stream, so pass p of a stacked batch owns rows [pB, (p+1)B).
"""
import os

import numpy as np
import torch

from . import ct_common
from . import functional as F
from . import tflib as lib
from .tflib.ops import linear as _linear
from .tflib.ops import wn_dense as _wn


class Config(ct_common.Config):
    """The literals of TH/CT_MNIST.py:14-22, 33-53, 103-105, 140-141 (tests shrink the five shape entries)."""
    Factor_M = 0.0
    LAMBDA_2 = 0.1
    SEED = 2
    SEED_DATA = 2
    UNLABELED_WEIGHT = 1.
    BATCH_SIZE = 100
    COUNT = 10
    LR = 0.003
    BETA1 = 0.5
    BETA2 = 0.999
    AVG_RATE = 0.0001
    EPOCHS = 300
    INIT_ROWS = 500
    SIGMA_IN = 0.3
    SIGMA_HIDDEN = 0.5
    IN_DIM = 784
    HIDDEN = (1000, 500, 250, 250, 250)
    N_CLASSES = 10
    Z_DIM = 100
    G_HIDDEN = (500, 500)


cfg = Config()


def configure(**kw):
    global cfg
    cfg = Config(**kw)
    return cfg


def Generator(n_samples, noise=None, rng=None):
    """:33-38 -> [n_samples, IN_DIM] in (0,1).  `noise`: z given (parity tests); else one uniform call site of `rng`."""
    if noise is None:
        noise = rng.uniform(n_samples, cfg.Z_DIM)
    output, width = noise, cfg.Z_DIM
    for i, w in enumerate(cfg.G_HIDDEN):
        name = 'Generator.%d' % (i + 1)
        output = _linear.Linear(name, width, w, output, biases=False, initialization='glorot')      # lasagne's default GlorotUniform
        offset = lib.param(name + '.bn_b', lambda r, w=w: np.zeros((w,), dtype='float32'))
        output = F.batch_norm_2d(output, offset, 1e-6, softplus=True)
        width = w
    name = 'Generator.%d' % (len(cfg.G_HIDDEN) + 1)
    std = np.sqrt(2. / (width + cfg.IN_DIM))
    W = lib.param(name + '.W', lambda r: r.uniform(-std * np.sqrt(3), std * np.sqrt(3), (width, cfg.IN_DIM)).astype('float32'))
    W_scale = lib.param(name + '.W_scale', lambda r: np.ones((cfg.IN_DIM,), dtype='float32'))
    b = lib.param(name + '.b', lambda r: np.zeros((cfg.IN_DIM,), dtype='float32'))
    return F.sigmoid(F.linear(output, F.weight_norm(W, W_scale, 1e-6), b))


def Classifier(inputs, init=False, deterministic=False, rng=None, features=False, frozen=False):
    """:41-53 -> logits [n, N_CLASSES]; features=True: the fifth layer's ReLU output before its noise (layers[-3], :92-93).
    init: the data-dependent initialisation pass; deterministic: no noise; frozen: parameters as constants."""
    kw = dict(init=init, deterministic=deterministic, rng=rng, frozen=frozen)
    output = _wn.GaussianNoise(inputs, cfg.SIGMA_IN, deterministic, rng)
    width = cfg.IN_DIM
    for i, w in enumerate(cfg.HIDDEN):
        last = i == len(cfg.HIDDEN) - 1
        sigma = 0.0 if (features and last) else cfg.SIGMA_HIDDEN
        output = _wn.WNDense('Classifier.%d' % (i + 1), width, w, output, sigma=sigma, **kw)
        width = w
    if features:
        return output
    return _wn.WNDense('Classifier.%d' % (len(cfg.HIDDEN) + 1), width, cfg.N_CLASSES, output, nonlinearity=None, train_scale=True, **kw)


def build_params():
    """Register every parameter (lib.param creates on first use) with one tiny deterministic pass."""
    with torch.no_grad():
        Classifier(Generator(2, noise=torch.zeros(2, cfg.Z_DIM, device=lib._dev())), deterministic=True)


class SSLTrainer(ct_common.SSLTrainerBase):
    """The two Theano functions train_batch_disc / train_batch_gen (:110-111), init_param (:109) and test_batch (:112); a classifier
    batch is (x_lab, labels, x_unl), train_iteration (:161-166) takes it followed by x_unl2."""
    cfg = property(lambda self: cfg)
    D_KEYS = ('out4', 'loss_lab', 'loss_unl', 'ct', 'train_err', 'ct_i')
    REPORT = ('Iteration', (('loss_lab', 'loss_lab'), ('loss_unl', 'loss_unl'), ('train err', 'train_err')), ())

    def __init__(self, seed=None):
        super().__init__(build_params, seed)

    def d_cotangents(self):
        """out4 = {loss_lab, loss_unl, CT, train_err}: cost = loss_lab + UNLABELED_WEIGHT loss_unl (:103)"""
        return {'out4': [1.0, cfg.UNLABELED_WEIGHT, 0.0, 0.0]}

    # ---- data-dependent init (:60-62, :137)
    def init_params(self, x):
        self.rng.begin_step()
        with torch.no_grad():
            Classifier(x, init=True, rng=self.rng)
        self.rng.end_step()
        lib.bump_epoch('Classifier')

    # ---- classifier step
    def d_losses(self, x_lab, labels, x_unl):
        B = x_lab.shape[0]
        self.rng.begin_step()
        with torch.no_grad():
            fake = Generator(B, rng=self.rng)
        logits = Classifier(torch.cat([x_lab, x_unl, x_unl, fake], 0), rng=self.rng)
        out4, ct_i = F.ssl_head(logits, labels, B, cfg.LAMBDA_2, cfg.Factor_M)
        return {'out4': out4, 'loss_lab': out4[0], 'loss_unl': out4[1], 'ct': out4[2], 'train_err': out4[3], 'ct_i': ct_i, 'logits': logits}

    # ---- generator step
    def g_losses(self, x_unl):
        B = x_unl.shape[0]
        self.rng.begin_step()
        fake = Generator(B, rng=self.rng)
        feats = Classifier(torch.cat([fake, x_unl], 0), rng=self.rng, features=True, frozen=True)
        return {'loss_gen': F.feature_matching(feats, B)}

    # ---- evaluation on the averaged parameters (:97-98, :106, :112)
    def predict(self, x, averaged=True):
        """Logits of the deterministic pass; averaged: every trained classifier parameter replaced by its average (`givens`, :106) -
        the weight scales of layers 1-5 are not trained, have no average and stay live."""
        return self._averaged(lambda: Classifier(x, deterministic=True), averaged)

    def test_error(self, x, y, averaged=True, batch_size=None):
        """Mean over whole batches of the per-batch argmax error (:173-176)."""
        bs = batch_size or cfg.BATCH_SIZE
        y = np.asarray(y)
        errs = []
        for t in range(len(x) // bs):
            xb = torch.as_tensor(x[t * bs:(t + 1) * bs], dtype=torch.float32).to(self.dev)
            pred = self.predict(xb, averaged).cpu().numpy().argmax(1)
            errs.append(float(np.mean(pred != y[t * bs:(t + 1) * bs])))
        return float(np.mean(errs))


class SSLData:
    """Host side of TH/CT_MNIST.py:114-154: `mnist.npz` (x_train / x_valid / x_test [n,784] in [0,1], y_*), train + valid joined, COUNT
    labelled examples per class picked after a `seed_data` permutation, and per epoch the labelled stream (N_unl / (10 COUNT)
    permutations of the labelled set) and two independently reshuffled copies of the unlabelled set.  `arrays`: the same keys in a
    dict instead of a file.  Nothing is downloaded: a missing file is an error."""

    def __init__(self, path=None, count=None, seed=None, seed_data=None, batch_size=None, arrays=None, n_classes=None):
        count = cfg.COUNT if count is None else count
        self.batch_size = cfg.BATCH_SIZE if batch_size is None else batch_size
        n_classes = cfg.N_CLASSES if n_classes is None else n_classes
        if arrays is None:
            if path is None or not os.path.isfile(path):
                raise IOError("Couldn't find the MNIST file at %s (mnist.npz with x_train/x_valid/x_test and y_*; it is not downloaded)" % path)
            arrays = np.load(path)
        trainx = np.concatenate([arrays['x_train'], arrays['x_valid']], axis=0).astype(np.float32)
        trainy = np.concatenate([arrays['y_train'], arrays['y_valid']]).astype(np.int32)
        self.unl, self.unl2 = trainx.copy(), trainx.copy()
        self.testx, self.testy = arrays['x_test'].astype(np.float32), arrays['y_test'].astype(np.int32)
        self.nr_batches_train = trainx.shape[0] // self.batch_size
        # :27-30 - the script's `rng` seeds Theano's and lasagne's generators with its first two draws, then shuffles the epochs
        self.rng = np.random.RandomState(cfg.SEED if seed is None else seed)
        self.rng.randint(2 ** 15); self.rng.randint(2 ** 15)
        data_rng = np.random.RandomState(cfg.SEED_DATA if seed_data is None else seed_data)
        inds = data_rng.permutation(trainx.shape[0])
        trainx, trainy = trainx[inds], trainy[inds]
        self.txs = np.concatenate([trainx[trainy == j][:count] for j in range(n_classes)], axis=0)
        self.tys = np.concatenate([trainy[trainy == j][:count] for j in range(n_classes)], axis=0)
        self.init_batch = trainx[:cfg.INIT_ROWS]
        self.lab_x = self.lab_y = None

    def begin_epoch(self):
        """:145-154, in the script's draw order."""
        xs, ys = [], []
        for _ in range(self.unl.shape[0] // self.txs.shape[0]):
            inds = self.rng.permutation(self.txs.shape[0])
            xs.append(self.txs[inds]); ys.append(self.tys[inds])
        self.lab_x, self.lab_y = np.concatenate(xs, axis=0), np.concatenate(ys, axis=0)
        self.unl = self.unl[self.rng.permutation(self.unl.shape[0])]
        self.unl2 = self.unl2[self.rng.permutation(self.unl2.shape[0])]
        return self.nr_batches_train

    def batch(self, t):
        """(x_lab, labels, x_unl, x_unl2) of batch t of the current epoch (:161-166)."""
        s = slice(t * self.batch_size, (t + 1) * self.batch_size)
        return self.lab_x[s], self.lab_y[s], self.unl[s], self.unl2[s]

    def test_set(self):
        return self.testx, self.testy


def train(data_path, epochs=None, seed=None, seed_data=None, use_graphs=True, out_dir=None, resume=None, checkpoint_every=1, log=print,
          max_batches=None):
    """The loop of TH/CT_MNIST.py:114-180 on an mnist.npz-format file: data-dependent init on the first 500 permuted rows, then per
    epoch one classifier and one generator step per batch (graph replay unless use_graphs=False), the test error on the averaged
    parameters, and the script's report line (also one record of train_log.Series in `out_dir`/log.jsonl).  A checkpoint
    (checkpoint.py: parameters, both Adam states with the averages, the random-stream counters) is written to `out_dir` every
    `checkpoint_every` epochs; `resume` continues from one at the epoch it was written.  max_batches: shorten the epochs (smoke runs).
    Returns the trainer."""
    from .engine import GraphedSSLTrainer
    data = SSLData(data_path, seed=seed, seed_data=seed_data)
    lib.delete_all_params()
    return ct_common.train_loop(SSLTrainer(seed=seed), data, GraphedSSLTrainer, lambda tr, d: tr.init_params(torch.from_numpy(d.init_batch).to(tr.dev)),
                                epochs, use_graphs, out_dir, resume, checkpoint_every, log, max_batches)
